"""fp64 reference of the per-view exposure compensation (include/tgs.h, tgs_exposure_fwd / tgs_exposure_bwd),
evaluated from the fp32 inputs, its fp32 floor, and the input builders of the tests.

E = [A | b] row-major 3x4, C [P,3] the rendered colours (P = W H pixels, row-major):

    C'[p][c]  = sum_k A[c][k] C[p][k] + b[c]                                   (no clamp)
    v'[p][c]  = v_img[p][c] + l1_weight sign(C'[p][c] - gt[p][c]),  sign(0) = 0
    v_rgb[p][k] = sum_c A[c][k] v'[p][c]
    G_A[c][k] = sum_p v'[p][c] C[p][k],   G_b[c] = sum_p v'[p][c]              (G [3,4] = [G_A | G_b])
    M_A[c][k] = sum_p |v'[p][c] C[p][k]|, M_b[c] = sum_p |v'[p][c]|            (the masses: the unit of G's rounding error)
    L1        = l1_weight sum |C' - gt|
    update:   g = G + l2 (E - I), then Adam on the 12 entries (tests/adam_ref.py), t and beta^t kept with the row.

Accuracy is counted in units of 2^-24 x mass (``err_units``); ``floor`` is that figure for an fp32 NumPy evaluation whose
sums run pairwise, ``bar`` = 4 x the floor and never below 4 units -- the convention of tests/pose_ref.py.
"""
from types import SimpleNamespace

import numpy as np

EPS32 = 2.0 ** -24
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def apply(C, E, dtype=np.float64):
    """C' [P,3]; every product and add in ``dtype``, the sum in the order A0 r + A1 g + A2 b + b (any order is exact for
    the dyadic builder)."""
    T = np.dtype(dtype).type
    C, E = np.asarray(C).reshape(-1, 3).astype(T), np.asarray(E).reshape(3, 4).astype(T)
    out = np.empty_like(C)
    for c in range(3):
        acc = (E[c, 0] * C[:, 0]).astype(T)
        acc = (acc + (E[c, 1] * C[:, 1]).astype(T)).astype(T)
        acc = (acc + (E[c, 2] * C[:, 2]).astype(T)).astype(T)
        out[:, c] = (acc + E[c, 3]).astype(T)
    return out


def fwd_mass(C, E):
    """sum_k |A[c][k] C[p][k]| + |b[c]| per entry, fp64 [P,3]: the unit of the forward's rounding error."""
    C, E = np.asarray(C).reshape(-1, 3).astype(np.float64), np.asarray(E).reshape(3, 4).astype(np.float64)
    return np.abs(C) @ np.abs(E[:, :3]).T + np.abs(E[:, 3])


def _sum(X, T):
    """Column sums of X [P,k] in T; NumPy sums the contiguous axis pairwise."""
    return np.ascontiguousarray(X.T.astype(T)).sum(axis=1, dtype=T)


def bwd(C, E, gt=None, l1_weight=0.0, v_img=None, dtype=np.float64):
    """-> namespace(cprime, vprime, v_rgb [P,3], v_mass [P,3] = sum_c |A[c][k] v'[p][c]|, G [3,4], mass [3,4], l1, count)."""
    T = np.dtype(dtype).type
    C = np.asarray(C).reshape(-1, 3).astype(T)
    E = np.asarray(E).reshape(3, 4).astype(T)
    P = C.shape[0]
    cp = apply(C, E, dtype)
    vp = np.zeros((P, 3), T) if v_img is None else np.asarray(v_img).reshape(-1, 3).astype(T)
    l1 = T(0)
    if gt is not None:
        d = (cp - np.asarray(gt).reshape(-1, 3).astype(T)).astype(T)
        vp = (vp + T(np.float32(l1_weight)) * np.sign(d).astype(T)).astype(T)
        l1 = T(T(np.float32(l1_weight)) * _sum(np.abs(d).reshape(-1, 1), T)[0])
    A = E[:, :3]
    v_rgb = (vp @ A).astype(T)
    v_mass = np.abs(vp).astype(np.float64) @ np.abs(A).astype(np.float64)
    G, mass = np.empty((3, 4), T), np.empty((3, 4), T)
    for c in range(3):
        prod = (vp[:, c:c + 1] * C).astype(T)
        G[c, :3], mass[c, :3] = _sum(prod, T), _sum(np.abs(prod), T)
        G[c, 3], mass[c, 3] = _sum(vp[:, c:c + 1], T)[0], _sum(np.abs(vp[:, c:c + 1]), T)[0]
    return SimpleNamespace(cprime=cp, vprime=vp, v_rgb=v_rgb, v_mass=v_mass, G=G, mass=mass, l1=l1, count=P)


def out32(r):
    """The 32 floats tgs_exposure_bwd writes for a valid frame, from a ``bwd`` result (float64)."""
    o = np.zeros(32)
    o[:12], o[12:24], o[24], o[25], o[26] = r.G.reshape(-1), r.mass.reshape(-1), 1.0, r.l1, r.count
    return o


def err_units(got, ref, mass):
    """max over the entries of |got - ref| / (2^-24 mass); an entry without mass must be exact."""
    got, ref, mass = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, mass))
    d = np.abs(got - ref)
    assert (d[mass == 0] == 0).all(), "an entry whose mass is zero must be exactly zero"
    return float(np.where(mass > 0, d / np.maximum(EPS32 * mass, 1e-300), 0.0).max())


def floor(case):
    """fp32 floor of a case -> (G in units of its masses, the L1 value in units of itself): the fp32 pairwise evaluation
    against fp64."""
    r64 = bwd(case.C, case.E, case.gt, case.l1_weight, case.v_img, np.float64)
    r32 = bwd(case.C, case.E, case.gt, case.l1_weight, case.v_img, np.float32)
    return err_units(r32.G, r64.G, r64.mass), err_units([r32.l1], [r64.l1], [r64.l1])


def bar(case):
    """4 x the floor, never below 4 units -> (for G, for the L1 value)."""
    fg, fl = floor(case)
    return 4.0 * max(fg, 1.0), 4.0 * max(fl, 1.0)


# ---------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------
def _case(W, H, C, E, gt, v_img, l1_weight, **kw):
    f = np.float32
    return SimpleNamespace(W=W, H=H, C=C.astype(f).reshape(H, W, 3), E=E.astype(f).reshape(3, 4), gt=gt.astype(f).reshape(H, W, 3),
                           v_img=v_img.astype(f).reshape(H, W, 3), l1_weight=float(f(l1_weight)), **kw)


def dyadic_case(W, H, seed=0, l1_weight=0.8 / 3):
    """C in multiples of 2^-10 in [0, 1), A of 2^-6 in [-2, 2], b of 2^-10 in [-1, 1]: C' needs under 20 bits and is exact in
    fp32 in any order, FMA included.  gt = C' + delta, delta = 0 on about 5 % of the entries (exact ties) and otherwise
    |delta| in [2^-8, 0.5] in multiples of 2^-16."""
    rng = np.random.default_rng(1000 + seed)
    P = W * H
    C = rng.integers(0, 1024, (P, 3)) / 1024.0
    E = np.concatenate([rng.integers(-128, 129, (3, 3)) / 64.0, rng.integers(-1024, 1025, (3, 1)) / 1024.0], axis=1)
    cp = apply(C, E)
    delta = rng.integers(256, 32769, (P, 3)) / 65536.0 * rng.choice([-1.0, 1.0], (P, 3))
    tie = rng.random((P, 3)) < 0.05
    delta[tie] = 0.0
    v_img = rng.standard_normal((P, 3)) * 1e-2
    return _case(W, H, C, E, cp + delta, v_img, l1_weight, tie=tie.reshape(H, W, 3))


def generic_case(W, H, seed=0, l1_weight=0.8 / 3):
    """Random floats; gt = fp32(C'_ref + delta) with |delta| >= 1e-3: an fp32 C' cannot land on the other side of gt."""
    rng = np.random.default_rng(2000 + seed)
    P = W * H
    C = rng.random((P, 3)).astype(np.float32)
    E = (IDENTITY + 0.3 * rng.standard_normal((3, 4))).astype(np.float32)
    cp = apply(C, E)
    delta = rng.uniform(1e-3, 0.3, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))
    v_img = rng.standard_normal((P, 3)) * 1e-2
    return _case(W, H, C, E, (cp + delta).astype(np.float32), v_img, l1_weight)


# ---------------------------------------------------------------------------------------------
# the optimizer row and the recovery loop (fp64)
# ---------------------------------------------------------------------------------------------
def new_row(dtype=np.float64):
    """One view's state row [48]: E = identity, zero moments, t = 0, beta1^0 = beta2^0 = 1."""
    s = np.zeros(48, dtype)
    s[:12] = IDENTITY.reshape(-1)
    s[37] = s[38] = 1
    return s


def adam_row_step(row, G, lr, betas=(0.9, 0.999), eps=1e-15, l2=0.0):
    """One update of a row in fp64 (constants rounded to fp32 first, as the C float arguments carry them)."""
    f = lambda x: float(np.float32(x))
    lr, b1, b2, eps, l2 = f(lr), f(betas[0]), f(betas[1]), f(eps), f(l2)
    row = np.asarray(row, np.float64).copy()
    g = np.asarray(G, np.float64).reshape(-1) + l2 * (row[:12] - IDENTITY.reshape(-1))
    row[36] += 1
    row[37] *= b1
    row[38] *= b2
    row[12:24] = b1 * row[12:24] + (1 - b1) * g
    row[24:36] = b2 * row[24:36] + (1 - b2) * g * g
    row[:12] -= lr * (row[12:24] / (1 - row[37])) / (np.sqrt(row[24:36] / (1 - row[38])) + eps)
    return row


RECOVER = dict(W=64, H=48, steps=300, lr=0.01, seed=7,
               A=((1.2, 0.03, -0.02), (0.01, 0.9, 0.02), (-0.03, 0.02, 1.1)), b=(0.02, -0.03, 0.01))


def recover_inputs():
    """64 x 48 random C and gt = A* C + b* (fp32), L1 only with l1_weight = 1 / (3 W H): the loss is the mean |C' - gt|."""
    rng = np.random.default_rng(RECOVER["seed"])
    W, H = RECOVER["W"], RECOVER["H"]
    C = rng.random((H, W, 3)).astype(np.float32)
    Es = np.concatenate([np.array(RECOVER["A"]), np.array(RECOVER["b"]).reshape(3, 1)], axis=1)
    gt = apply(C, Es).astype(np.float32).reshape(H, W, 3)
    return C, gt, float(np.float32(1.0 / (3 * W * H)))


def recovery_loop(grad_fn, steps=None):
    """``steps`` updates from the identity; grad_fn(row) -> (G [12], L1 at the row's E).  -> (L1 before the first step,
    L1 at the final E, final row).  The fp64 reference is recovery_loop(ref_grad_fn(...))."""
    row = new_row()
    first = None
    for _ in range(steps or RECOVER["steps"]):
        G, l1 = grad_fn(row)
        first = l1 if first is None else first
        row = adam_row_step(row, G, RECOVER["lr"])
    return first, grad_fn(row)[1], row


def ref_grad_fn(C, gt, l1_weight):
    def fn(row):
        r = bwd(C, row[:12], gt, l1_weight, None)
        return r.G.reshape(-1), float(r.l1)
    return fn
