"""fp64 reference of the per-view bilateral grid (include/tgs.h, tgs_bilagrid_fwd / tgs_bilagrid_bwd),
evaluated from the fp32 inputs, its fp32 floor, and the input builders of the tests.

The grid g [GH,GW,L,12] holds a row-major 3x4 [A | b] per vertex; ``shape`` = (GW, GH, L).  For pixel (px, py) of a W x H
image with colour C = (r, g, b), every operation in fp32 and in this order (``coords``):

    gx = (float(px) + 0.5f) * sx,  sx = float(GW-1) / float(W);   gy likewise
    luma = (0.299f r + 0.587f g) + 0.114f b;   z = min(max(luma, 0), 1) * float(L-1)
    ix = min(int(gx), GW-2), fx = gx - float(ix);   iy, fy and iz, fz likewise;   inside = luma > 0 && luma < 1

These scalars decide the pixel's cell; the reference takes them from this fp32 evaluation, so it and the kernels never
disagree about a cell (``guide64=True`` forms them in fp64 instead: the mode that is compared with torch's grid_sample).

    A(p)      = trilinear blend of the 8 corners in lerp form a + f (b - a): x, then y (A0, A1 at levels iz, iz+1), then z
    C'[p][c]  = ((A[c][0] r + A[c][1] g) + A[c][2] b) + A[c][3]                     (no clamp)
    v'[p][c]  = v_img[p][c] + l1_weight sign(C'[p][c] - gt[p][c]),  sign(0) = 0
    v_rgb[p][k] = sum_c A[c][k] v'[p][c] + wl[k] (L-1) inside sum_c v'[p][c] ((A1 - A0) C1)[c]      C1 = (C, 1)
    G[v][c][k] = sum_p w_v(p) v'[p][c] C1[p][k],  M likewise of the absolute values  (w_v: the trilinear weight of vertex v)
    L1        = l1_weight sum |C' - gt|
    TV(g)     = sum_{axis x,y,z} (1 / n_axis) sum (g[next] - g[this])^2 over all 12 channels, n_axis = number of differences
    update:   grad = G + tv_weight dTV/dg, then Adam on every entry (tests/adam_ref.py), t and beta^t kept with the row.

Accuracy is counted in units of 2^-24 x mass (``err_units``); ``floors`` holds that figure for an fp32 NumPy evaluation that
rounds every operation as the kernels do (they are built without FMA contraction) and whose sums run pairwise; ``bars`` =
4 x the floor and never below 4 units -- the convention of tests/pose_ref.py and tests/exposure_ref.py.
"""
from types import SimpleNamespace

import numpy as np

EPS32 = 2.0 ** -24
WL = (0.299, 0.587, 0.114)


def identity_grid(shape, dtype=np.float32):
    GW, GH, L = shape
    g = np.zeros((GH, GW, L, 12), dtype)
    g[..., 0] = g[..., 5] = g[..., 10] = 1
    return g


def n_entries(shape):
    return shape[0] * shape[1] * shape[2] * 12


# ---------------------------------------------------------------------------------------------
# coordinates, slice, forward
# ---------------------------------------------------------------------------------------------
def coords(W, H, shape, C, guide64=False):
    """-> namespace of per-pixel arrays [P]: ix, iy, iz (int64), fx, fy, fz, inside.  fp32 NumPy (each operation rounded on
    its own) unless ``guide64``."""
    GW, GH, L = shape
    T = np.float64 if guide64 else np.float32
    C = np.asarray(C, np.float32).reshape(-1, 3).astype(T)

    def axis(n, G):
        s = T(G - 1) / T(n)
        g = (np.arange(n).astype(T) + T(0.5)) * s
        i = np.minimum(g.astype(np.int64), G - 2)
        return i, g - i.astype(T)

    ix, fx = axis(W, GW)
    iy, fy = axis(H, GH)
    ix, fx, iy, fy = np.tile(ix, H), np.tile(fx, H), np.repeat(iy, W), np.repeat(fy, W)
    luma = (T(np.float32(WL[0])) * C[:, 0] + T(np.float32(WL[1])) * C[:, 1]) + T(np.float32(WL[2])) * C[:, 2]
    z = np.minimum(np.maximum(luma, T(0)), T(1)) * T(L - 1)
    iz = np.minimum(z.astype(np.int64), L - 2)
    fz = z - iz.astype(T)
    assert fx.dtype == T and fz.dtype == T and luma.dtype == T
    return SimpleNamespace(ix=ix, iy=iy, iz=iz, fx=fx, fy=fy, fz=fz, inside=(luma > 0) & (luma < 1), luma=luma)


def slice_grid(grid, co, T):
    """-> (A0, A1, A) [P,12] in dtype T, the lerps in the kernels' order."""
    g = np.asarray(grid).astype(T)
    fx, fy, fz = (a.astype(T)[:, None] for a in (co.fx, co.fy, co.fz))
    lv = []
    for dl in (0, 1):
        c00, c10 = g[co.iy, co.ix, co.iz + dl], g[co.iy, co.ix + 1, co.iz + dl]
        c01, c11 = g[co.iy + 1, co.ix, co.iz + dl], g[co.iy + 1, co.ix + 1, co.iz + dl]
        a = c00 + fx * (c10 - c00)
        b = c01 + fx * (c11 - c01)
        lv.append(a + fy * (b - a))
    A0, A1 = lv
    A = A0 + fz * (A1 - A0)
    assert A.dtype == T
    return A0, A1, A


def _apply(A, C):
    """((A[c][0] r + A[c][1] g) + A[c][2] b) + A[c][3] per channel, [P,3]."""
    A = A.reshape(-1, 3, 4)
    return ((A[:, :, 0] * C[:, 0:1] + A[:, :, 1] * C[:, 1:2]) + A[:, :, 2] * C[:, 2:3]) + A[:, :, 3]


def fwd(C, grid, shape, W, H, dtype=np.float64, guide64=False):
    """C' [P,3] in ``dtype``."""
    T = np.dtype(dtype).type
    co = coords(W, H, shape, C, guide64)
    Ct = np.asarray(C, np.float32).reshape(-1, 3).astype(T)
    return _apply(slice_grid(grid, co, T)[2], Ct)


def fwd_mass(C, grid, shape, W, H):
    """sum_k |A[c][k] C[p][k]| + |b[c]| per entry, fp64 [P,3]: the unit of the forward's rounding error."""
    co = coords(W, H, shape, C)
    A = np.abs(slice_grid(grid, co, np.float64)[2]).reshape(-1, 3, 4)
    Ca = np.abs(np.asarray(C, np.float32).reshape(-1, 3).astype(np.float64))
    return (A[:, :, :3] * Ca[:, None, :]).sum(axis=2) + A[:, :, 3]


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
def _sum(X, T):
    """Column sums of X [P,k] in T; NumPy sums the contiguous axis pairwise."""
    return np.ascontiguousarray(X.T.astype(T)).sum(axis=1, dtype=T)


def _scatter(vidx, contrib, nvert, T):
    """sum of contrib [M,k] rows per vertex -> [nvert,k] in T.  fp64: bincount; otherwise a pairwise sum per vertex."""
    out = np.zeros((nvert, contrib.shape[1]), T)
    if T == np.float64:
        for j in range(contrib.shape[1]):
            out[:, j] = np.bincount(vidx, weights=contrib[:, j], minlength=nvert)
        return out
    order = np.argsort(vidx, kind="stable")
    srt = np.ascontiguousarray(contrib[order].T)
    v = vidx[order]
    uniq, first = np.unique(v, return_index=True)
    last = np.append(first[1:], v.size)
    for u, a, b in zip(uniq, first, last):
        out[u] = srt[:, a:b].sum(axis=1, dtype=T)
    return out


def bwd(C, grid, shape, W, H, gt=None, l1_weight=0.0, v_img=None, tie=None, dtype=np.float64, guide64=False):
    """-> namespace(cprime, vprime, v_rgb [P,3], v_mass [P,3], G [n], mass [n], l1, count, touched [n] bool).
    ``tie`` [P,3] bool: entries where C' - gt is taken as exactly 0 (gt planted from a forward's own output)."""
    T = np.dtype(dtype).type
    GW, GH, L = shape
    C32 = np.asarray(C, np.float32).reshape(-1, 3)
    Ct = C32.astype(T)
    P = Ct.shape[0]
    co = coords(W, H, shape, C32, guide64)
    A0, A1, A = slice_grid(grid, co, T)
    cp = _apply(A, Ct)
    vp = np.zeros((P, 3), T) if v_img is None else np.asarray(v_img).reshape(-1, 3).astype(T)
    l1 = T(0)
    if gt is not None:
        d = (cp - np.asarray(gt).reshape(-1, 3).astype(T)).astype(T)
        if tie is not None:
            d[np.asarray(tie).reshape(-1, 3)] = 0
        vp = (vp + T(np.float32(l1_weight)) * np.sign(d).astype(T)).astype(T)
        l1 = T(np.float64(np.float32(l1_weight)) * np.float64(_sum(np.abs(d).reshape(-1, 1), T)[0]))
    dA = A1 - A0
    dz = _apply(dA, Ct)
    gz = (T(0) + vp[:, 0] * dz[:, 0] + vp[:, 1] * dz[:, 1]) + vp[:, 2] * dz[:, 2]
    gz = np.where(co.inside, gz * T(L - 1), T(0)).astype(T)
    Am = A.reshape(-1, 3, 4)
    wl = np.array([np.float32(w) for w in WL]).astype(T)
    v_rgb = ((Am[:, 0, :3] * vp[:, 0:1] + Am[:, 1, :3] * vp[:, 1:2]) + Am[:, 2, :3] * vp[:, 2:3]) + wl[None, :] * gz[:, None]
    assert v_rgb.dtype == T and cp.dtype == T
    # masses in fp64: the direct term, and the guide term with |A0| + |A1| in place of their difference (what cancels)
    a64, v64 = np.abs(Am.astype(np.float64)), np.abs(vp.astype(np.float64))
    C1a = np.concatenate([np.abs(Ct.astype(np.float64)), np.ones((P, 1))], axis=1)
    dzm = ((np.abs(A0.astype(np.float64)) + np.abs(A1.astype(np.float64))).reshape(-1, 3, 4) * C1a[:, None, :]).sum(axis=2)
    gzm = np.where(co.inside, (v64 * dzm).sum(axis=1) * (L - 1), 0.0)
    v_mass = (a64[:, :, :3] * v64[:, :, None]).sum(axis=1) + wl.astype(np.float64)[None, :] * gzm[:, None]
    # to the grid
    C1 = np.concatenate([Ct, np.ones((P, 1), T)], axis=1)
    t = (vp[:, :, None] * C1[:, None, :]).reshape(P, 12)
    fx, fy, fz = (a.astype(T) for a in (co.fx, co.fy, co.fz))
    wx, wy, wz = (T(1) - fx, fx), (T(1) - fy, fy), (T(1) - fz, fz)
    vidx, contrib = [], []
    for dl in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = ((wx[dx] * wy[dy]) * wz[dl])[:, None]
                vidx.append(((co.iy + dy) * GW + co.ix + dx) * L + co.iz + dl)
                contrib.append(np.concatenate([w * t, w * np.abs(t)], axis=1))
    vidx, contrib = np.concatenate(vidx), np.concatenate(contrib)
    assert contrib.dtype == T
    nvert = GH * GW * L
    S = _scatter(vidx, contrib, nvert, T)
    touched = np.repeat(np.bincount(vidx, minlength=nvert) > 0, 12)
    return SimpleNamespace(cprime=cp, vprime=vp, v_rgb=v_rgb, v_mass=v_mass, G=S[:, :12].reshape(-1), mass=S[:, 12:].reshape(-1),
                           l1=l1, count=P, touched=touched, co=co)


def tv(grid, dtype=np.float64):
    """-> (TV value, dTV/dg [GH,GW,L,12]) in ``dtype``; axes x = 1, y = 0, z = 2."""
    T = np.dtype(dtype).type
    g = np.asarray(grid).astype(T)
    val, grad = T(0), np.zeros_like(g)
    for ax in (1, 0, 2):
        d = np.diff(g, axis=ax)
        inv = T(1) / T(d.size)
        val = T(val + inv * _sum((d * d).reshape(-1, 1), T)[0])
        pad = [(0, 0)] * 4
        pad[ax] = (1, 0)
        lo = np.pad(d, pad)       # g[this] - g[prev] at this (0 at the first)
        pad[ax] = (0, 1)
        hi = np.pad(d, pad)       # g[next] - g[this] at this (0 at the last)
        grad = grad + T(2) * inv * (lo - hi)
    return val, grad


def err_units(got, ref, mass):
    """max over the entries of |got - ref| / (2^-24 mass); an entry without mass must be exact."""
    got, ref, mass = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mass))
    d = np.abs(got - ref)
    assert (d[mass == 0] == 0).all(), "an entry whose mass is zero must be exactly zero"
    return float(np.where(mass > 0, d / np.maximum(EPS32 * mass, 1e-300), 0.0).max())


def case_bwd(case, dtype=np.float64, **kw):
    return bwd(case.C, case.grid, case.shape, case.W, case.H, case.gt, case.l1_weight, case.v_img,
               tie=getattr(case, "tie", None), dtype=dtype, **kw)


def floors(case):
    """fp32 floors of a case, in units of 2^-24 mass -> dict(fwd, G, v_rgb, l1, tv)."""
    r64, r32 = case_bwd(case), case_bwd(case, np.float32)
    c32 = fwd(case.C, case.grid, case.shape, case.W, case.H, np.float32)
    t64, t32 = tv(case.grid)[0], tv(case.grid, np.float32)[0]
    return dict(fwd=err_units(c32, r64.cprime, fwd_mass(case.C, case.grid, case.shape, case.W, case.H)),
                G=err_units(r32.G, r64.G, r64.mass), v_rgb=err_units(r32.v_rgb, r64.v_rgb, r64.v_mass),
                l1=err_units([r32.l1], [r64.l1], [r64.l1]), tv=err_units([t32], [t64], [t64]))


def bars(case):
    """4 x the floor, never below 4 units, per quantity."""
    return {k: 4.0 * max(v, 1.0) for k, v in floors(case).items()}


# ---------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------
def smooth_grid(shape, rng, amp=0.3):
    """The identity plus smooth noise within +-amp: per entry one sinusoid of at most one period across the grid."""
    GW, GH, L = shape
    v, u, t = np.meshgrid(np.linspace(0, 1, GH), np.linspace(0, 1, GW), np.linspace(0, 1, L), indexing="ij")
    k = rng.uniform(-1, 1, (12, 3))
    ph = rng.uniform(0, 2 * np.pi, 12)
    noise = amp * np.sin(2 * np.pi * (u[..., None] * k[:, 0] + v[..., None] * k[:, 1] + t[..., None] * k[:, 2]) + ph)
    return (identity_grid(shape, np.float64) + noise).astype(np.float32)


def make_case(W, H, shape, seed=0, l1_weight=0.8 / 3):
    """Colours in [-0.2, 1.2] (some pixels clamp in z on either side), grid = identity + smooth noise of +-0.3,
    gt = fp32(C'_ref + delta) with |delta| >= 1e-3: an fp32 C' cannot land on the other side of gt."""
    rng = np.random.default_rng(3000 + seed)
    P = W * H
    f = np.float32
    C = rng.uniform(-0.2, 1.2, (P, 3)).astype(f)
    grid = smooth_grid(shape, rng)
    cp = fwd(C, grid, shape, W, H)
    delta = rng.uniform(1e-3, 0.3, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))
    v_img = (rng.standard_normal((P, 3)) * 1e-2).astype(f)
    co = coords(W, H, shape, C)
    if P >= 400:
        assert (co.luma <= 0).any() and (co.luma >= 1).any(), "the builder is to clamp some pixels on both sides"
    return SimpleNamespace(W=W, H=H, shape=tuple(shape), C=C.reshape(H, W, 3), grid=grid, gt=(cp + delta).astype(f).reshape(H, W, 3),
                           v_img=v_img.reshape(H, W, 3), l1_weight=float(f(l1_weight)), tie=None)


# ---------------------------------------------------------------------------------------------
# the optimizer row and the recovery loop (fp64)
# ---------------------------------------------------------------------------------------------
TAIL = 16


def new_row(shape, dtype=np.float64):
    """One view's state row [3n+16]: identity grid, zero moments, t = 0, beta1^0 = beta2^0 = 1."""
    n = n_entries(shape)
    s = np.zeros(3 * n + TAIL, dtype)
    s[:n] = identity_grid(shape, dtype).reshape(-1)
    s[3 * n + 1] = s[3 * n + 2] = 1
    return s


def adam_row_step(row, shape, G, lr, tv_weight=0.0, betas=(0.9, 0.999), eps=1e-15):
    """One update of a row in fp64 (constants rounded to fp32 first, as the C float arguments carry them); dTV/dg is read
    from the grid BEFORE the step."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, tvw = f(lr), f(betas[0]), f(betas[1]), f(eps), f(tv_weight)
    n = n_entries(shape)
    row = np.asarray(row, np.float64).copy()
    GW, GH, L = shape
    g = np.asarray(G, np.float64).reshape(-1)
    if tvw != 0:
        g = g + tvw * tv(row[:n].reshape(GH, GW, L, 12))[1].reshape(-1)
    row[3 * n] += 1
    row[3 * n + 1] *= b1
    row[3 * n + 2] *= b2
    row[n:2 * n] = b1 * row[n:2 * n] + (1 - b1) * g
    row[2 * n:3 * n] = b2 * row[2 * n:3 * n] + (1 - b2) * g * g
    row[:n] -= lr * (row[n:2 * n] / (1 - row[3 * n + 1])) / (np.sqrt(row[2 * n:3 * n] / (1 - row[3 * n + 2])) + eps)
    return row


RECOVER = dict(W=64, H=48, shape=(5, 3, 4), steps=300, lr=0.01, seed=11, amp=0.2)


def recover_inputs():
    """64 x 48 random C in [0, 1) and gt = C sliced through a fixed smooth non-identity grid (fp32), L1 only with
    l1_weight = 1 / (3 W H): the loss is the mean |C' - gt|."""
    rng = np.random.default_rng(RECOVER["seed"])
    W, H, shape = RECOVER["W"], RECOVER["H"], RECOVER["shape"]
    C = rng.random((H, W, 3)).astype(np.float32)
    target = smooth_grid(shape, rng, RECOVER["amp"])
    gt = fwd(C, target, shape, W, H).astype(np.float32).reshape(H, W, 3)
    return C, gt, float(np.float32(1.0 / (3 * W * H)))


def recovery_loop(grad_fn, steps=None):
    """``steps`` updates from the identity; grad_fn(row) -> (G [n], L1 at the row's grid).  -> (L1 before the first step,
    L1 at the final grid, final row).  The fp64 reference is recovery_loop(ref_grad_fn(...))."""
    shape = RECOVER["shape"]
    row = new_row(shape)
    first = None
    for _ in range(steps or RECOVER["steps"]):
        G, l1 = grad_fn(row)
        first = l1 if first is None else first
        row = adam_row_step(row, shape, G, RECOVER["lr"])
    return first, grad_fn(row)[1], row


def ref_grad_fn(C, gt, l1_weight):
    W, H, shape = RECOVER["W"], RECOVER["H"], RECOVER["shape"]
    GW, GH, L = shape
    n = n_entries(shape)

    def fn(row):
        r = bwd(C, row[:n].reshape(GH, GW, L, 12), shape, W, H, gt, l1_weight, None)
        return r.G, float(r.l1)
    return fn
