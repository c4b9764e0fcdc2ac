"""Per-view bilateral grids: each TRAINING view owns a small 3-D grid g[GH][GW][L][12] of affine colour
transforms [A | b] (row-major 3x4, the identity at the start), indexed by pixel position and by the luminance of the rendered
colour, sliced trilinearly and regularised by total variation.  The rendered image C becomes C' = A(p) C + b(p) before the
RGB loss; held-out views have no grid and are rendered as they are.

All state lives on the device in one ``[n_views, 3 n + 16]`` float32 tensor, n = GH GW L 12, a row per view

    [0, n) grid | [n, 2n) exp_avg | [2n, 3n) exp_avg_sq | [3n] steps t | [3n+1] beta1^t | [3n+2] beta2^t | [3n+3 ..] 0

and is stepped by the call that reduces the gradient (``ops.bilagrid_bwd``, tgs_bilagrid_bwd): nothing of it passes through
the host during training, and a frame voided by its overflow guard leaves its row alone bit for bit.  Only the rendered
view's row is stepped, with the full TV term: gsplat applies TV / n_views to every grid on every step, which is the same
pull on average, so its weight of 10 carries over.
"""
from __future__ import annotations

import os
from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib, ops
from .colorcorr import ViewColorSet

BILAGRIDS_FILE = "bilagrids.npz"
DEFAULT_SHAPE = (16, 16, 8)     # (GW, GH, L)


def identity_grid(shape, dtype=np.float32) -> np.ndarray:
    """[GH, GW, L, 12]: the identity [I | 0] at every vertex."""
    GW, GH, L = (int(x) for x in shape)
    g = np.zeros((GH, GW, L, 12), dtype)
    g[..., 0] = g[..., 5] = g[..., 10] = 1
    return g


def to_gsplat(grid: np.ndarray) -> np.ndarray:
    """[GH, GW, L, 12] -> gsplat's [12, L, GH, GW]."""
    return np.ascontiguousarray(np.transpose(grid, (3, 2, 0, 1)))


def from_gsplat(grid: np.ndarray) -> np.ndarray:
    """gsplat's [12, L, GH, GW] -> [GH, GW, L, 12]."""
    return np.ascontiguousarray(np.transpose(grid, (2, 3, 1, 0)))


def _tv(g, axes):
    """Total variation of a grid along ``axes``: the sum of the mean squared differences of neighbouring vertices."""
    return sum(((g.narrow(a, 1, g.shape[a] - 1) - g.narrow(a, 0, g.shape[a] - 1)) ** 2).mean() for a in axes)


class BilagridSet(ViewColorSet):
    """The grid rows of ``views``, the full-resolution training views (``ViewColorSet``)."""
    name, what, rate_field, start_field, l1_index = "bilagrid", "bilateral grids", "bilagrid_lr", "bilagrid_start_step", 1

    def __init__(self, views: Sequence, device, lr: float = 2e-3, shape=DEFAULT_SHAPE, tv_weight: float = 10.0,
                 betas=(0.9, 0.999), eps: float = 1e-15, warmup_steps: int = 1000, max_steps: int = 30000):
        self.shape = tuple(int(x) for x in shape)
        if len(self.shape) != 3 or min(self.shape) < 2:
            raise ValueError(f"bilagrid_shape must be (GW, GH, L) with every dimension >= 2, got {tuple(shape)}")
        GW, GH, L = self.shape
        self.n, self.leaf_shape = GH * GW * L * 12, (GH, GW, L, 12)
        self.lr, self.tv_weight = float(lr), float(tv_weight)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.warmup_steps, self.max_steps = int(warmup_steps), max(int(max_steps), 1)
        row = torch.zeros(3 * self.n + _lib.BILAGRID_TAIL, dtype=torch.float32)
        row[:self.n] = torch.from_numpy(identity_grid(self.shape).reshape(-1))
        row[3 * self.n + 1] = row[3 * self.n + 2] = 1.0      # beta^0
        super().__init__(views, device, row)

    def lr_at(self, step: int) -> float:
        """gsplat's schedule of the grids' rate, formed on the host from the step number: linear warm-up from 1 % over
        ``warmup_steps``, chained with an exponential decay that reaches 1 % at ``max_steps``."""
        step = max(int(step), 0)
        warm = 1.0 if self.warmup_steps <= 0 else 0.01 + 0.99 * min(step / self.warmup_steps, 1.0)
        return self.lr * warm * 0.01 ** (min(step, self.max_steps) / self.max_steps)

    def adam(self, step: int) -> dict:
        """The optimizer constants of ``step`` in the form ``ops.bilagrid_bwd`` takes."""
        return dict(lr=self.lr_at(step), betas=self.betas, eps=self.eps)

    def scratch(self, W: int, H: int) -> torch.Tensor:
        """The reduction scratch of ``ops.bilagrid_bwd`` for a W x H frame, kept between steps."""
        return self._scratch_of(int(_lib.load().tgs_bilagrid_scratch_floats(W, H, *self.shape)))

    def forward(self, rgb, row):
        return ops.bilagrid_fwd(rgb, row, self.shape)

    def backward_step(self, rgb, row, gt, l1_weight, v_img, guard, step, W, H):
        return ops.bilagrid_bwd(rgb, row, self.shape, gt=gt, l1_weight=l1_weight, v_img=v_img, tv_weight=self.tv_weight,
                                guard=guard, state=row, adam=self.adam(step), want_grad=False,
                                out=(torch.empty(_lib.BILAGRID_OUT, dtype=torch.float32, device=rgb.device),
                                     self.scratch(W, H)))[:2]

    @classmethod
    def loss_terms(cls, result, config) -> dict:
        return {"bilagrid_tv_loss": config.bilagrid_tv * result[3]}

    def apply(self, rgb, leaf):
        return ops.apply_bilagrid(rgb, leaf)

    def leaf_loss_terms(self, leaf) -> dict:
        return {"bilagrid_tv_loss": self.tv_weight * _tv(leaf, (0, 1, 2))}

    def metrics(self) -> dict:
        if not self.views:
            return {}
        g = self.state[:, :self.n].view(-1, *self.leaf_shape)
        return dict(bilagrid_tv=_tv(g, (1, 2, 3)),
                    bilagrid_delta=(g - g.new_tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])).abs().mean())

    def grids(self) -> np.ndarray:
        """[n_views, GH, GW, L, 12] on the host, in the order of ``views`` (one copy; synchronises)."""
        return self.state[:, :self.n].detach().cpu().numpy().reshape(-1, *self.leaf_shape)

    def grid(self, view) -> np.ndarray:
        """The view's grid on the host, [GH, GW, L, 12].  Synchronises: for saving and reporting, not for the step."""
        return self.row(view)[:self.n].detach().cpu().numpy().reshape(self.leaf_shape)

    def state_dict(self) -> dict:
        return dict(super().state_dict(), shape=self.shape)

    def load_state_dict(self, sd: dict) -> None:
        s = sd["state"]
        if tuple(sd.get("shape", self.shape)) != self.shape or tuple(s.shape) != tuple(self.state.shape):
            raise ValueError(f"checkpoint holds bilateral-grid rows of shape {tuple(s.shape)} for a grid "
                             f"{tuple(sd.get('shape', ()))}, the set {tuple(self.state.shape)} for {self.shape}")
        super().load_state_dict(sd)

    def save(self, run_dir: str, names: Sequence[str]) -> str:
        return save_bilagrids(run_dir, self, names)


def save_bilagrids(run_dir: str, bs: BilagridSet, names: Sequence[str]) -> str:
    """<run_dir>/bilagrids.npz: per training image name its grid in gsplat's [12, L, GH, GW] order."""
    path = os.path.join(run_dir, BILAGRIDS_FILE)
    host = bs.grids()
    np.savez(path, **{n: to_gsplat(host[i]) for i, n in enumerate(names)})
    return path


def load_bilagrids(path: str) -> Dict[str, np.ndarray]:
    """bilagrids.npz -> {image name: grid [GH, GW, L, 12]} (the layout of the kernels)."""
    with np.load(path) as z:
        return {k: from_gsplat(z[k]) for k in z.files}
