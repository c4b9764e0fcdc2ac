"""The INRIA trainer's second CUDA module beside the rasterizer, ``simple_knn._C.distCUDA2``, on the HIP kernels
(``ops.knn``; csrc/knn.hip).  A trainer ported onto ``touch_gs_amd.rasterizer.GaussianRasterizer`` sizes its
initial Gaussians as it always did::

    from touch_gs_amd.simple_knn import distCUDA2
    dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)
    scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
"""
from __future__ import annotations

import torch

from . import ops


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    """[N] float32: for every point the mean of the SQUARED distances to its 3 nearest other points, ``((d0 + d1) + d2) / 3``
    in fp32 -- INRIA's semantics: squared, not clamped (the caller clamps).  Exact neighbours (the original's are exact as
    well); duplicates of a point count as its neighbours at distance 0; with fewer than 4 points the result is ``inf``.
    ``points``: [N,3] on the device, any float dtype (computed in fp32)."""
    d2, _ = ops.knn(points.detach().float().contiguous(), 3)
    three = torch.full((), 3.0, dtype=torch.float32, device=d2.device)      # a device tensor: a true division, not a reciprocal
    return ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / three
