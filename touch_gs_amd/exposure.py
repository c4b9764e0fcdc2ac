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
from typing import Dict, Sequence

import numpy as np
import torch

from . import _lib

EXPOSURES_FILE = "exposures.json"


class ExposureSet:
    """The exposure rows of ``views`` (the FULL-resolution training views, recognised by identity; a downscaled form of a
    view uses its parent's row: the caller asks with the parent)."""

    def __init__(self, views: Sequence, device, lr: float, betas=(0.9, 0.999), eps: float = 1e-15, l2: float = 0.0):
        self.views = list(views)
        self.lr, self.betas, self.eps, self.l2 = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(l2)
        self._index: Dict[int, int] = {id(v): i for i, v in enumerate(self.views)}
        row = torch.zeros(_lib.EXPO_STATE, dtype=torch.float32)
        row[0] = row[5] = row[10] = 1.0      # E = identity
        row[37] = row[38] = 1.0              # beta^0
        self.state = row.repeat(max(len(self.views), 1), 1)[:len(self.views)].contiguous().to(device)
        self._scratch = None

    @property
    def adam(self) -> dict:
        """The optimizer constants in the form ``ops.exposure_bwd`` takes."""
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, l2=self.l2)

    def owns(self, view) -> bool:
        i = self._index.get(id(view))
        return i is not None and self.views[i] is view

    def row(self, view) -> torch.Tensor:
        """The view's [48] row: a view INTO the state tensor (the kernels read E from its head and step it in place)."""
        return self.state[self._index[id(view)]]

    def scratch(self, W: int, H: int) -> torch.Tensor:
        """The reduction scratch of ``ops.exposure_bwd`` for a W x H frame, kept between steps."""
        P = _lib.load().tgs_exposure_num_partials(W, H)
        if self._scratch is None or self._scratch.shape[0] < P or self._scratch.device != self.state.device:
            self._scratch = torch.empty(max(P, 1), _lib.EXPO_OUT, dtype=torch.float32, device=self.state.device)
        return self._scratch

    def matrix(self, view) -> np.ndarray:
        """E of the view on the host, [3,4] float32.  Synchronises: for saving and reporting, not for the step."""
        return self.row(view)[:12].detach().cpu().numpy().reshape(3, 4)

    def matrices(self) -> np.ndarray:
        """[n_views, 3, 4] on the host, in the order of ``views`` (one copy; synchronises)."""
        return self.state[:, :12].detach().cpu().numpy().reshape(-1, 3, 4)

    def state_dict(self) -> dict:
        return dict(state=self.state.detach().cpu().clone())

    def load_state_dict(self, sd: dict) -> None:
        s = sd["state"]
        if tuple(s.shape) != tuple(self.state.shape):
            raise ValueError(f"checkpoint holds exposure rows of shape {tuple(s.shape)}, the set {tuple(self.state.shape)}")
        self.state.copy_(s.to(torch.float32))


def save_exposures(run_dir: str, es: ExposureSet, names: Sequence[str]) -> str:
    """<run_dir>/exposures.json: per training image its 3x4 exposure matrix and the number of steps it took."""
    path = os.path.join(run_dir, EXPOSURES_FILE)
    host = es.state.detach().cpu().numpy()
    with open(path, "w") as f:
        json.dump({n: dict(E=host[i, :12].reshape(3, 4).tolist(), steps=int(host[i, 36])) for i, n in enumerate(names)},
                  f, indent=1)
    return path
