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

from . import _lib

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


class BilagridSet:
    """The grid rows of ``views`` (the FULL-resolution training views, recognised by identity; a downscaled form of a view
    uses its parent's row: the caller asks with the parent)."""

    def __init__(self, views: Sequence, device, lr: float = 2e-3, shape=DEFAULT_SHAPE, tv_weight: float = 10.0,
                 betas=(0.9, 0.999), eps: float = 1e-15, warmup_steps: int = 1000, max_steps: int = 30000):
        self.views = list(views)
        self.shape = tuple(int(x) for x in shape)
        if len(self.shape) != 3 or min(self.shape) < 2:
            raise ValueError(f"bilagrid_shape must be (GW, GH, L) with every dimension >= 2, got {tuple(shape)}")
        GW, GH, L = self.shape
        self.n = GH * GW * L * 12
        self.lr, self.tv_weight = float(lr), float(tv_weight)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.warmup_steps, self.max_steps = int(warmup_steps), max(int(max_steps), 1)
        self._index: Dict[int, int] = {id(v): i for i, v in enumerate(self.views)}
        row = torch.zeros(3 * self.n + _lib.BILAGRID_TAIL, dtype=torch.float32)
        row[:self.n] = torch.from_numpy(identity_grid(self.shape).reshape(-1))
        row[3 * self.n + 1] = row[3 * self.n + 2] = 1.0      # beta^0
        self.state = row.repeat(max(len(self.views), 1), 1)[:len(self.views)].contiguous().to(device)
        self._scratch = None

    def lr_at(self, step: int) -> float:
        """gsplat's schedule of the grids' rate, formed on the host from the step number: linear warm-up from 1 % over
        ``warmup_steps``, chained with an exponential decay that reaches 1 % at ``max_steps``."""
        step = max(int(step), 0)
        warm = 1.0 if self.warmup_steps <= 0 else 0.01 + 0.99 * min(step / self.warmup_steps, 1.0)
        return self.lr * warm * 0.01 ** (min(step, self.max_steps) / self.max_steps)

    def adam(self, step: int) -> dict:
        """The optimizer constants of ``step`` in the form ``ops.bilagrid_bwd`` takes."""
        return dict(lr=self.lr_at(step), betas=self.betas, eps=self.eps)

    def owns(self, view) -> bool:
        i = self._index.get(id(view))
        return i is not None and self.views[i] is view

    def row(self, view) -> torch.Tensor:
        """The view's [3n+16] row: a view INTO the state tensor (the kernels read the grid from its head and step it in place)."""
        return self.state[self._index[id(view)]]

    def scratch(self, W: int, H: int) -> torch.Tensor:
        """The reduction scratch of ``ops.bilagrid_bwd`` for a W x H frame, kept between steps."""
        GW, GH, L = self.shape
        S = int(_lib.load().tgs_bilagrid_scratch_floats(W, H, GW, GH, L))
        if self._scratch is None or self._scratch.numel() < S or self._scratch.device != self.state.device:
            self._scratch = torch.empty(max(S, 1), dtype=torch.float32, device=self.state.device)
        return self._scratch

    def grids(self) -> np.ndarray:
        """[n_views, GH, GW, L, 12] on the host, in the order of ``views`` (one copy; synchronises)."""
        GW, GH, L = self.shape
        return self.state[:, :self.n].detach().cpu().numpy().reshape(-1, GH, GW, L, 12)

    def grid(self, view) -> np.ndarray:
        """The view's grid on the host, [GH, GW, L, 12].  Synchronises: for saving and reporting, not for the step."""
        GW, GH, L = self.shape
        return self.row(view)[:self.n].detach().cpu().numpy().reshape(GH, GW, L, 12)

    def state_dict(self) -> dict:
        return dict(state=self.state.detach().cpu().clone(), shape=self.shape)

    def load_state_dict(self, sd: dict) -> None:
        s = sd["state"]
        if tuple(sd.get("shape", self.shape)) != self.shape or tuple(s.shape) != tuple(self.state.shape):
            raise ValueError(f"checkpoint holds bilateral-grid rows of shape {tuple(s.shape)} for a grid "
                             f"{tuple(sd.get('shape', ()))}, the set {tuple(self.state.shape)} for {self.shape}")
        self.state.copy_(s.to(torch.float32))


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
