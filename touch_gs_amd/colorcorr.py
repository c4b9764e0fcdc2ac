"""Per-view colour correction, the one seam the model talks to: a ``ViewColorSet`` holds one
device-resident row per TRAINING view -- the correction's parameters at its head, then its Adam moments and counters -- and
turns the rendered image C into C' before the RGB loss.  ``ExposureSet`` and ``BilagridSet`` are its two subclasses; a third
colour model is a third subclass and an ``enable_*`` wrapper on the model."""
from __future__ import annotations

from typing import Sequence

import torch


class ViewColorSet:
    """The rows of ``views`` (the FULL-resolution training views, recognised by identity; a downscaled form of a view uses
    its parent's row: the caller asks with the parent).  A subclass sets ``name`` (the key of ``model.last[...]``,
    ``state_dict[...]`` and ``outputs[...]``), ``what`` (the correction in words, for error texts), ``rate_field`` /
    ``start_field`` (the ModelConfig fields of its learning rate and of its first step), ``l1_index`` (where its result vector
    holds ``l1_weight * sum |C' - gt|``), ``n`` / ``leaf_shape`` (the parameters at the head of a row, and their shape on the
    autograd path), and defines, reaching the ops as ``ops.<name>`` at call time,

    ``forward(rgb, row)`` -> C', the image SSIM and the L1 term are taken on (fused path)
    ``backward_step(rgb, row, gt, l1_weight, v_img, guard, step, W, H)`` -> (a fresh result vector, K7's upstream v_rgb):
                                        forms the L1 term on C' and steps ``row`` in the same call
    ``apply(rgb, leaf)`` -> C', differentiable in both (autograd path)
    ``save(run_dir, names)`` -> the path of the file it wrote."""
    name = what = rate_field = start_field = l1_index = None

    def __init__(self, views: Sequence, device, row: torch.Tensor):
        """``row``: the initial row of every view."""
        self.views = list(views)
        self._index = {id(v): i for i, v in enumerate(self.views)}
        self.state = row.repeat(max(len(self.views), 1), 1)[:len(self.views)].contiguous().to(device)
        self._scratch = None

    def owns(self, view) -> bool:
        i = self._index.get(id(view))
        return i is not None and self.views[i] is view

    def row(self, view) -> torch.Tensor:
        """The view's row: a view INTO the state tensor (the kernels read the parameters from its head and step it in place)."""
        return self.state[self._index[id(view)]]

    def _scratch_of(self, *shape) -> torch.Tensor:
        """The reduction scratch of the backward op, at least ``shape`` along its first axis, kept between steps."""
        s = self._scratch
        if s is None or s.shape[0] < shape[0] or s.device != self.state.device:
            self._scratch = s = torch.empty(max(shape[0], 1), *shape[1:], dtype=torch.float32, device=self.state.device)
        return s

    def state_dict(self) -> dict:
        return dict(state=self.state.detach().cpu().clone())

    def load_state_dict(self, sd: dict) -> None:
        s = sd["state"]
        if tuple(s.shape) != tuple(self.state.shape):
            raise ValueError(f"checkpoint holds {self.name} rows of shape {tuple(s.shape)}, the set {tuple(self.state.shape)}")
        self.state.copy_(s.to(torch.float32))

    @classmethod
    def l1_value(cls, result):
        return result[cls.l1_index]

    @classmethod
    def loss_terms(cls, result, config) -> dict:
        """The correction's own loss terms of a fused step from its result vector, weighted as ``config`` says."""
        return {}

    def leaf(self, view, requires_grad: bool) -> torch.Tensor:
        """A detached copy of the view's parameters in ``leaf_shape``, for the autograd path."""
        return self.row(view)[:self.n].detach().clone().view(self.leaf_shape).requires_grad_(requires_grad)

    def leaf_loss_terms(self, leaf) -> dict:
        return {}

    def metrics(self) -> dict:
        """Means over the training views; {} for a set without views."""
        return {}
