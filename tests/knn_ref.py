"""Brute-force reference of the exact k nearest neighbours (include/tgs.h: tgs_knn_*; touch_gs_amd.ops.knn) and the
fixtures the CPU and GPU tests share.

The definition:  d2(q, r) = (dx*dx + dy*dy) + dz*dz  with dx = qx - rx ..., every operation rounded to float32 on its own (NumPy
float32 arrays: one ufunc per operation, nothing fused); a row holds the k smallest d2 in ascending order, equal d2 by the lower
reference index; `exclude_self` drops reference i from query i BY INDEX; missing neighbours are +inf / -1.  `knn(..., dtype=
np.float64)` is the same with every operation in float64 (the inputs are float32 values either way)."""
import functools

import numpy as np

ROW_BLOCK = 512


def knn(points, k, queries=None, exclude_self=None, dtype=np.float32):
    """-> (dist2 [n_q,k] dtype, idx [n_q,k] int32)."""
    ref = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    self_query = queries is None
    q = ref if self_query else np.asarray(queries, dtype=np.float32).reshape(-1, 3)
    if exclude_self is None:
        exclude_self = self_query
    assert not exclude_self or len(q) == len(ref)
    n_q, n_ref = len(q), len(ref)
    R, Q = ref.astype(dtype), q.astype(dtype)
    out_d = np.empty((n_q, k), dtype=dtype)
    out_i = np.empty((n_q, k), dtype=np.int32)
    keep = k + 1 if exclude_self else k
    for b in range(0, n_q, ROW_BLOCK):
        qb = Q[b:b + ROW_BLOCK]
        dx = qb[:, None, 0] - R[None, :, 0]
        dy = qb[:, None, 1] - R[None, :, 1]
        dz = qb[:, None, 2] - R[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        # `keep` sentinel columns behind the real ones: a stable sort leaves them behind every real +inf
        d2 = np.concatenate([d2, np.full((len(qb), keep), np.inf, dtype=dtype)], axis=1)
        order = np.argsort(d2, axis=1, kind="stable")[:, :keep]          # ties: the lower index first
        if exclude_self:
            is_self = order == np.arange(b, b + len(qb))[:, None]
            order = np.take_along_axis(order, np.argsort(is_self, axis=1, kind="stable"), axis=1)[:, :k]
        out_d[b:b + len(qb)] = np.take_along_axis(d2, order, axis=1)
        out_i[b:b + len(qb)] = np.where(order < n_ref, order, -1)
    return out_d, out_i


def dist_mean3(points):
    """INRIA's distCUDA2: ((d0 + d1) + d2) / 3 of the three smallest squared distances, in float32."""
    d, _ = knn(points, 3)
    return ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)


# ----------------------------------------------------------------------------------------------------------------------
# fixtures (float32 [n,3]); every one is built once
# ----------------------------------------------------------------------------------------------------------------------
def _ball(rng, n, radius):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius * rng.random((n, 1)) ** (1.0 / 3.0))


@functools.lru_cache(maxsize=None)
def fixture(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "uniform":                       # 1: 5 000 uniform points
        p = rng.random((5000, 3))
    elif name == "mix":                         # 2: the project's cloud -- a dense object inside a sparse fill
        p = np.concatenate([_ball(rng, 3000, 0.02) + [0.1, -0.05, 0.2], rng.random((1000, 3)) * 2 - 1])
    elif name == "dup4":                        # 3a: 512 distinct points, each four times
        p = np.tile(rng.random((512, 3)), (4, 1))[rng.permutation(2048)]
    elif name == "same300":                     # 3b: 300 identical points: every key equal
        p = np.tile(np.array([[0.25, -1.5, 3.0]]), (300, 1))
    elif name == "lattice":                     # 4: 12 x 12 x 12 integers: massive exact ties
        g = np.arange(12)
        p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[rng.permutation(1728)]
    elif name == "planar":                      # 5a: z = 0
        p = np.concatenate([rng.random((2000, 2)), np.zeros((2000, 1))], axis=1)
    elif name == "collinear":                   # 5b: a line along x
        p = np.concatenate([rng.random((1500, 1)) * 4 - 2, np.full((1500, 1), 0.5), np.full((1500, 1), -0.25)], axis=1)
    elif name.startswith("n"):                  # 6: n points
        p = rng.random((int(name[1:]), 3))
    elif name == "refs777":                     # 7: the references of the two-set form
        p = rng.random((777, 3))
    elif name == "queries1000":                 # 7: a third of the queries far outside the references' bounds
        p = rng.random((1000, 3))
        far = rng.permutation(1000)[:333]
        p[far] = p[far] * 40 - 20 + np.sign(p[far] - 0.5) * 3
    else:
        raise KeyError(name)
    return np.ascontiguousarray(p, dtype=np.float32)


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) * 7919


@functools.lru_cache(maxsize=None)
def reference(name, k=16, dtype="float32"):
    """The self-query reference of a fixture at k (the first k' columns are the reference at k' < k)."""
    d, i = knn(fixture(name), k, dtype=np.dtype(dtype).type)
    d.setflags(write=False)
    i.setflags(write=False)
    return d, i


def init_cloud(n, seed=0):
    """What touch_gs_amd.train.init_params is handed by the trainer: (points, uint8 colours) of a dense touched object."""
    rng = np.random.default_rng(seed)
    pts = _ball(rng, n, 0.05) + [0.2, 0.1, -0.1]
    return pts.astype(np.float32), rng.integers(0, 256, size=(n, 3)).astype(np.uint8)
