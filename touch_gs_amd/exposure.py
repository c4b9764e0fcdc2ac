"""Per-view exposure compensation: one affine colour transform E = [A | b] (3x4, identity at the start) per
TRAINING view, learned with the scene.  The rendered image C becomes C' = A C + b before the RGB loss; held-out views have no
row and are rendered as they are.

All state lives on the device in one ``[n_views, 48]`` float32 tensor, a row per view

    [0..11] E row-major | [12..23] exp_avg | [24..35] exp_avg_sq | [36] steps t | [37] beta1^t | [38] beta2^t | [39..47] 0

and is stepped by the kernel that reduces the gradient (``ops.exposure_bwd``, tgs_exposure_bwd): nothing of it passes
through the host during training, and a frame voided by its overflow guard leaves its row alone bit for bit.
"""
from __future__ import annotations

import json
import os
from typing import Sequence

import numpy as np
import torch

from . import _lib, ops
from .colorcorr import ViewColorSet

EXPOSURES_FILE = "exposures.json"


class ExposureSet(ViewColorSet):
    """The exposure rows of ``views``, the full-resolution training views (``ViewColorSet``)."""
    name, what, rate_field, start_field = "exposure", "exposure compensation", "exposure_lr", "exposure_start_step"
    l1_index, n, leaf_shape = 25, 12, (3, 4)

    def __init__(self, views: Sequence, device, lr: float, betas=(0.9, 0.999), eps: float = 1e-15, l2: float = 0.0):
        self.lr, self.betas, self.eps, self.l2 = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(l2)
        row = torch.zeros(_lib.EXPO_STATE, dtype=torch.float32)
        row[0] = row[5] = row[10] = 1.0      # E = identity
        row[37] = row[38] = 1.0              # beta^0
        super().__init__(views, device, row)

    @property
    def adam(self) -> dict:
        """The optimizer constants in the form ``ops.exposure_bwd`` takes."""
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, l2=self.l2)

    def scratch(self, W: int, H: int) -> torch.Tensor:
        """The reduction scratch of ``ops.exposure_bwd`` for a W x H frame, kept between steps."""
        return self._scratch_of(_lib.load().tgs_exposure_num_partials(W, H), _lib.EXPO_OUT)

    def forward(self, rgb, row):
        return ops.exposure_fwd(rgb, row)

    def backward_step(self, rgb, row, gt, l1_weight, v_img, guard, step, W, H):
        return ops.exposure_bwd(rgb, row, gt=gt, l1_weight=l1_weight, v_img=v_img, guard=guard, state=row, adam=self.adam,
                                out=(torch.empty(_lib.EXPO_OUT, dtype=torch.float32, device=rgb.device), self.scratch(W, H)))

    def apply(self, rgb, leaf):
        return ops.apply_exposure(rgb, leaf)

    def metrics(self) -> dict:
        if not self.views:
            return {}
        E = self.state[:, :12]
        return dict(exposure_gain=E[:, [0, 5, 10]].mean(), exposure_offset=E[:, [3, 7, 11]].mean())

    def matrix(self, view) -> np.ndarray:
        """E of the view on the host, [3,4] float32.  Synchronises: for saving and reporting, not for the step."""
        return self.row(view)[:12].detach().cpu().numpy().reshape(3, 4)

    def matrices(self) -> np.ndarray:
        """[n_views, 3, 4] on the host, in the order of ``views`` (one copy; synchronises)."""
        return self.state[:, :12].detach().cpu().numpy().reshape(-1, 3, 4)

    def save(self, run_dir: str, names: Sequence[str]) -> str:
        return save_exposures(run_dir, self, names)


def save_exposures(run_dir: str, es: ExposureSet, names: Sequence[str]) -> str:
    """<run_dir>/exposures.json: per training image its 3x4 exposure matrix and the number of steps it took."""
    path = os.path.join(run_dir, EXPOSURES_FILE)
    host = es.state.detach().cpu().numpy()
    with open(path, "w") as f:
        json.dump({n: dict(E=host[i, :12].reshape(3, 4).tolist(), steps=int(host[i, 36])) for i, n in enumerate(names)},
                  f, indent=1)
    return path
