"""fp64 oracle of the Adam update every optimizer kernel carries (``adam1``), and per-element bounds in units of the
element's own update, moment or ulp.

The oracle knows the flat layout from its documentation (include/tgs.h, TgsAdamSpec):

    means[3N] | log_scales[3N] | quats[4N] | opac_logit[N] | sh[N*K*3]

every segment starting at the next multiple of 4 floats, the total rounded up to a multiple of 4, one learning rate per
segment and the SH segment split into DC (the first 3 floats of every 3K-float row) and the rest.  The update is
torch.optim.Adam's (no weight decay, no amsgrad; tests/test_cpu_adam_ref.py ties it to torch.optim.Adam in fp64):

    g' = s g,  m1 = b1 m0 + (1 - b1) g',  v1 = b2 v0 + (1 - b2) g'^2,
    u  = lr (m1 / bc1) / (sqrt(v1 / bc2) + eps),  p1 = p0 - u,          bc1 = 1 - b1^t, bc2 = 1 - b2^t

in fp64 on the fp32 inputs, with the constants rounded to fp32 first -- the way the TgsAdamSpec fields and the C float
argument ``grad_scale`` carry them.

Bounds of ``check_step`` (E = 2^-24, the unit roundoff of fp32).  The constants count the roundings an fp32 evaluation
with fused multiply-adds needs; the "measured" column is the worst ratio of the fp32 emulation ``adam1_emulated`` over
2 M elements each of |g|, |m|, sqrt(v) log-uniform in 1e-30 .. 1e3 with exact zeros mixed in, steps 1, 2, 3, 10, 100 and
30 000, grad_scale 1, 1/8 and 1/3 (tests/test_cpu_adam_ref.py prints them again on a smaller sample):

    (a) |m1 - m_ref| <= 4E (|b1 m0| + |(1-b1) s g|) + (1-b1) s dg
            4 roundings: s g, (1 - b1), their product, the fma.                              measured 2.4 E
    (b) |v1 - v_ref| <= 8E v_ref + 2^-149 + (1-b2) s^2 (2 |g| dg + dg^2)
            7 roundings: s g twice (it is squared), (1 - b2), two products, the fma; 2^-149 is the smallest fp32
            denormal (g^2 underflows below |g| ~ 1e-19).                                     measured 4.4 E
    (c) |p1 - (p0 - lr (m1/bc1) / (sqrt(v1/bc2) + eps))| <= 1 ulp(max(|p0|, |p1|)) + 16E |u|
            the right-hand update evaluated in fp64 from the KERNEL'S OWN m1, v1, so it carries no sensitivity to (a),
            (b): it isolates learning rate, sign, bias corrections and eps of the element.  About 8 roundings with a
            correctly rounded sqrtf and divide: 1/bc1, m/bc1, lr *, sqrt v, sqrt bc2, 1/sqrt bc2, the fma with eps,
            the divide; the subtraction rounds p once (<= 1/2 ulp of the larger of p0, p1).
            measured below E max(|p0|, |p1|) + 16E |u| -- the rounding of p alone nearly fills the first term.

``dg`` is the caller's bound on how well the gradient is known (0 where the kernel reads it from a buffer).
"""
from typing import Dict, NamedTuple, Optional

import numpy as np

E = 2.0 ** -24            # unit roundoff of fp32
DENORM = 2.0 ** -149      # smallest fp32 denormal
C_M, C_V, C_U = 4.0, 8.0, 16.0   # the constants of (a), (b), (c), in units of E (see the module docstring)

SEGMENTS = ("means", "log_scales", "quats", "opac_logit", "sh")
LR_KEYS = ("means", "log_scales", "quats", "opac_logit", "sh_dc", "sh_rest")
DEFAULT_LRS = dict(means=1.6e-4, log_scales=5e-3, quats=1e-3, opac_logit=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)
MUTANTS = ("swap_dc_rest_column", "no_bias_corr2", "row_step_off_by_one", "grad_scale_m_only", "pad_takes_neighbour")

# tgs_adam_step launches one float4 per thread, 256 threads per block and at most MAX_BLOCKS blocks over its element
# range, and grid-strides beyond: one iteration covers 4 * 256 * MAX_BLOCKS = 4 194 304 flat elements.
MAX_BLOCKS = 4096
# A thread advances its column in the SH row by row_step only when it is inside the SH segment in two successive
# iterations, i.e. when the launch reaches more than one iteration beyond the start of the SH segment.  A whole-model
# launch barely beyond 4 194 304 elements does not: its second iteration is run by the lowest lanes only, which spent
# the first one in the means, and they enter the SH segment through the modulo.  These models (N, K) are the smallest
# whose SH segment alone, stepped as the range [start of sh, total), exceeds one iteration by 40 000 .. 55 000
# elements (N odd, so the segment starts behind a pad): there row_step -- 16, 16, 4 for rows of 48, 27, 12 floats --
# is read by more than 10 000 threads.  tests/test_cpu_adam_ref.py shows that the off-by-one mutant changes the
# learning-rate map of exactly these launches; tests/test_gpu_adam_oracle.py runs them.  K = 1 has no such case: a
# 3-float row is all DC, every column takes the same rate, and no row tracking fault can show.
GRID_STRIDE_SH = ((88_511, 16), (157_211, 9), (353_333, 4))


def f32(x) -> float:
    """A Python float holding the fp32 rounding of x (what a C float field carries)."""
    return float(np.float32(x))


def _al4(x: int) -> int:
    return -(-x // 4) * 4


def segments(N: int, K: int):
    """[(name, start, numel, padded_end)] of the documented layout, and the padded total."""
    out, o = [], 0
    for name, n in zip(SEGMENTS, (3 * N, 3 * N, 4 * N, N, 3 * K * N)):
        start = _al4(o)
        o = start + n
        out.append([name, start, n, None])
    total = _al4(o)
    for i, s in enumerate(out):
        s[3] = out[i + 1][1] if i + 1 < len(out) else total
    return [tuple(s) for s in out], total


def pad_mask(N: int, K: int) -> np.ndarray:
    """True at the pad elements between the segments and behind the last one."""
    segs, total = segments(N, K)
    mask = np.ones(total, dtype=bool)
    for _, start, n, _ in segs:
        mask[start:start + n] = False
    return mask


def lr_map(N: int, K: int, lrs: Dict[str, float]) -> np.ndarray:
    """One (fp32-rounded) learning rate per flat element, float64 [total].  Pads get the learning rate of the segment
    they trail (behind the SH segment: the row pattern goes on, i.e. sh_dc); a pad has p = g = m = v = 0, so its update
    is 0 whatever the rate."""
    segs, total = segments(N, K)
    lr = np.zeros(total, dtype=np.float64)
    for name, start, n, end in segs:
        if name != "sh":
            lr[start:end] = f32(lrs[name])
        else:
            col = np.arange(end - start) % max(3 * K, 1)
            lr[start:end] = np.where(col < 3, f32(lrs["sh_dc"]), f32(lrs["sh_rest"]))
    return lr


class AdamConsts(NamedTuple):
    """The fields of TgsAdamSpec as the kernel sees them: Python floats holding fp32 values."""
    beta1: float
    beta2: float
    eps: float
    bias_corr1: float
    bias_corr2: float


def consts(t: int, betas=(0.9, 0.999), eps: float = 1e-15) -> AdamConsts:
    """Step t (1-based): bias corrections 1 - beta^t evaluated in double from the unrounded betas, then every field
    rounded to fp32 (how a host fills the struct)."""
    return AdamConsts(f32(betas[0]), f32(betas[1]), f32(eps), f32(1.0 - betas[0] ** t), f32(1.0 - betas[1] ** t))


def _update64(m1, v1, lr, spec: AdamConsts):
    return lr * (m1 / spec.bias_corr1) / (np.sqrt(v1 / spec.bias_corr2) + spec.eps)


def adam_step_ref(p0, g, m0, v0, lr, spec: AdamConsts, grad_scale: float = 1.0):
    """One Adam step in fp64 on the (fp32) buffers, converted exactly -> (p1, m1, v1, u, |b1 m0| + |(1-b1) s g|), all
    float64.  float64 arrays are taken as they are, so the step can be chained without rounding the state."""
    p0, g, m0, v0 = (np.asarray(x).astype(np.float64) for x in (p0, g, m0, v0))
    lr = np.asarray(lr, dtype=np.float32).astype(np.float64)
    s = f32(grad_scale)
    b1, b2 = spec.beta1, spec.beta2
    gs = s * g
    m1 = b1 * m0 + (1.0 - b1) * gs
    v1 = b2 * v0 + (1.0 - b2) * gs * gs
    u = _update64(m1, v1, lr, spec)
    return p0 - u, m1, v1, u, np.abs(b1 * m0) + np.abs((1.0 - b1) * gs)


def _ulp32(x64):
    with np.errstate(over="ignore"):
        return np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)


def launch_stride(begin: int, end: int, max_blocks: int = MAX_BLOCKS) -> int:
    """The float4s one grid-stride iteration of a streaming launch over the elements [begin, end) covers."""
    n4 = (end - begin) // 4
    return min(max(-(-n4 // 256), 1), max_blocks) * 256


def _locate(i: int, N: int, K: int, base: int, launch=None) -> str:
    """Where flat element base + i lives: segment, column of the SH row and, where the streaming launch
    (elem_begin, elem_end, max_blocks) that wrote it is given, that launch's grid-stride iteration."""
    e = base + i
    segs, _ = segments(N, K)
    where = f"flat {e}"
    for name, start, n, end in segs:
        if start <= e < end:
            where += f": {name}[{e - start}]" + (" (pad)" if e >= start + n else "")
            if name == "sh" and K > 0:
                where += f" row {(e - start) // (3 * K)} column {(e - start) % (3 * K)}"
    if launch is not None and launch[0] <= e < launch[1]:
        where += f", grid-stride iteration {(e - launch[0]) // (4 * launch_stride(*launch))}"
    return where


def _fail(kind, err, bound, arrays, where):
    i = int(np.argmax(np.where(err > bound, err - bound, -np.inf)))
    vals = ", ".join(f"{k}={np.asarray(a).reshape(-1)[i]!r}" for k, a in arrays.items())
    n_bad = int((err > bound).sum())
    raise AssertionError(f"{kind}: {n_bad} elements beyond the bound, worst at {where(i)}: "
                         f"error {err[i]:.9g} > bound {bound[i]:.9g}; {vals}")


def _check_v_and_p(p0, m0, v0, p1, m1, v1, g, dg, lr, spec, s, where, label):
    """(b) and (c) on float64 images of fp32 buffers; returns their worst ratios in units of E."""
    b2 = spec.beta2
    gs = s * g
    v_ref = b2 * v0 + (1.0 - b2) * gs * gs
    err_v = np.abs(v1 - v_ref)
    slack_v = DENORM + (1.0 - b2) * s * s * (2.0 * np.abs(g) * dg + dg * dg)
    bound_v = C_V * E * v_ref + slack_v
    if (err_v > bound_v).any():
        _fail(f"{label}(b) exp_avg_sq", err_v, bound_v, dict(v0=v0, g=g, v1=v1, v_ref=v_ref, dg=dg), where)
    u = _update64(m1, v1, lr, spec)
    err_p = np.abs(p1 - (p0 - u))
    ulp = _ulp32(np.maximum(np.abs(p0), np.abs(p1)))
    bound_p = ulp + C_U * E * np.abs(u)
    if (err_p > bound_p).any():
        _fail(f"{label}(c) parameter", err_p, bound_p, dict(p0=p0, p1=p1, m1=m1, v1=v1, lr=lr, u=u), where)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_v = np.where(v_ref > 0, np.maximum(err_v - slack_v, 0) / (E * v_ref), 0.0)
        r_p = np.where(u != 0, np.maximum(err_p - ulp, 0) / (E * np.abs(u)), 0.0)
        r_p0 = np.where(u != 0, np.maximum(err_p - E * np.maximum(np.abs(p0), np.abs(p1)), 0) / (E * np.abs(u)), 0.0)
    mx = lambda a: float(a.max()) if a.size else 0.0
    return dict(v=mx(r_v), p=mx(r_p), p_half_ulp=mx(r_p0))


def _prep(before, after):
    arrs = []
    for x in tuple(before) + tuple(after):
        x = np.asarray(x)
        assert x.dtype == np.float32, "check the fp32 buffers themselves"
        arrs.append(x.reshape(-1).astype(np.float64))
    assert all(a.shape == arrs[0].shape for a in arrs)
    for a, name in zip(arrs[3:], ("p1", "m1", "v1")):
        assert np.isfinite(a).all(), f"{name} holds a non-finite value"
    return arrs


def check_step(before, after, g, dg, lr, spec: AdamConsts, grad_scale: float = 1.0, layout=None, base: int = 0,
               label: str = "", launch=None) -> Dict[str, float]:
    """One Adam step against the oracle, per element: (a), (b), (c) of the module docstring.

    before = (p0, m0, v0), after = (p1, m1, v1): the fp32 buffers around ONE step (numpy float32; the reference always
    starts from the state the kernel started with, so errors never compound).  g: the fp32 gradient buffer, or a float64
    reference gradient known to +-dg.  lr: per-element rates (``lr_map``).  layout = (N, K) and base (flat index of
    element 0 of the arrays) and launch = (elem_begin, elem_end, max_blocks) of the streaming launch that made the step
    only serve the failure message.  Returns the worst ratios in units of E:
    m over 4, v over 8, p over 16 would fail."""
    p0, m0, v0, p1, m1, v1 = _prep(before, after)
    g = np.asarray(g).reshape(-1).astype(np.float64)
    dg = np.broadcast_to(np.asarray(dg, dtype=np.float64), g.shape)
    lr = np.broadcast_to(np.asarray(lr, dtype=np.float32).astype(np.float64), g.shape)
    s = f32(grad_scale)
    b1 = spec.beta1
    where = (lambda i: _locate(i, layout[0], layout[1], base, launch)) if layout is not None else (lambda i: f"element {i}")
    m_ref = b1 * m0 + (1.0 - b1) * s * g
    am = np.abs(b1 * m0) + np.abs((1.0 - b1) * s * g)
    err_m = np.abs(m1 - m_ref)
    slack_m = (1.0 - b1) * s * dg
    bound_m = C_M * E * am + slack_m
    if (err_m > bound_m).any():
        _fail(f"{label}(a) exp_avg", err_m, bound_m, dict(m0=m0, g=g, m1=m1, m_ref=m_ref, dg=dg), where)
    with np.errstate(divide="ignore", invalid="ignore"):
        r_m = np.where(am > 0, np.maximum(err_m - slack_m, 0) / (E * am), 0.0)
    out = _check_v_and_p(p0, m0, v0, p1, m1, v1, g, dg, lr, spec, s, where, label)
    out["m"] = float(r_m.max()) if r_m.size else 0.0
    return out


def check_self_consistent(before, after, lr, spec: AdamConsts, layout=None, base: int = 0, label: str = "") -> Dict[str, float]:
    """For kernels whose gradient never reaches memory (grad_scale 1): the gradient the kernel used is read off its
    first moment, g_k = (m1 - b1 m0) / (1 - b1), known to dg = 4E (|b1 m0| + |m1|) / (1 - b1) (the roundings of (a)),
    and (b), (c) must hold for it.  From a zero state this is v1 = (1 - b2) (m1 / (1 - b1))^2 to 16E relative."""
    p0, m0, v0, p1, m1, v1 = _prep(before, after)
    b1 = spec.beta1
    g = (m1 - b1 * m0) / (1.0 - b1)
    dg = C_M * E * (np.abs(b1 * m0) + np.abs(m1)) / (1.0 - b1)
    lr = np.broadcast_to(np.asarray(lr, dtype=np.float32).astype(np.float64), g.shape)
    where = (lambda i: _locate(i, layout[0], layout[1], base)) if layout is not None else (lambda i: f"element {i}")
    return _check_v_and_p(p0, m0, v0, p1, m1, v1, g, dg, lr, spec, 1.0, where, label)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def stratified(n: int, rng: np.random.Generator, lo: float = 1e-30, hi: float = 1e3, zero_frac: float = 0.05,
               signed: bool = True) -> np.ndarray:
    """n values, float64: magnitudes log-uniform in [lo, hi], random signs, exact zeros mixed in."""
    x = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    if signed:
        x *= rng.choice([-1.0, 1.0], n)
    x[rng.random(n) < zero_frac] = 0.0
    return x


def stratified_state(N: int, K: int, rng: np.random.Generator, zero_moments: bool = False, only=None):
    """(p, g, m, v) float32 [total] in the flat layout, pads 0.  p: N(0, 1), a quarter of the elements exactly 0 (there
    (c) reads the update itself to 16E) and some large; g, m stratified and signed, v = (stratified >= 0)^2.
    only = (begin, end): the elements outside it are 0 (a large model of which one range is stepped)."""
    total = segments(N, K)[1]
    b, e = only or (0, total)
    n = e - b
    p = rng.standard_normal(n)
    sel = rng.random(n)
    p[sel < 0.25] = 0.0
    p[sel > 0.97] *= 1e3
    g = stratified(n, rng)
    if zero_moments:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m, v = stratified(n, rng), stratified(n, rng, signed=False) ** 2
    pads = pad_mask(N, K)
    out = []
    for x in (p, g, m, v):
        full = np.zeros(total, dtype=np.float32)
        full[b:e] = x
        full[pads] = 0.0
        out.append(full)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the streaming kernel, with deliberate faults
# ---------------------------------------------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf: the fp64 multiply-add (the product of two fp32 values is exact in fp64) rounded to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_lr_emulated(N: int, K: int, lrs, max_blocks: int = MAX_BLOCKS, mutate: Optional[str] = None,
                       elem_range=None) -> np.ndarray:
    """The learning rate each flat element gets from a streaming launch over elem_range = (begin, end) (multiples of 4;
    the whole buffer by default) that handles one float4 per thread, 256 threads per block and at most ``max_blocks``
    blocks, grid-striding beyond: inside the SH segment a thread takes its column in the 3K-float row from a modulo
    when it first enters the segment and advances it by row_step = (4 * grid stride) mod 3K per iteration afterwards.
    Elements outside the range keep the rate of ``lr_map``."""
    segs, total = segments(N, K)
    lr = lr_map(N, K, lrs).astype(np.float32)
    o_sh = segs[4][1]
    row = 3 * K if K > 0 else 4
    b, e = elem_range or (0, total)
    assert b % 4 == 0 and e % 4 == 0 and 0 <= b < e <= total
    b4, sh4 = b // 4, o_sh // 4
    stride = launch_stride(b, e, max_blocks)
    row_step = (4 * stride) % row + (1 if mutate == "row_step_off_by_one" else 0)
    i = np.arange(max(sh4, b4), e // 4, dtype=np.int64)     # the launch's float4s inside the SH segment
    lane, it = (i - b4) % stride, (i - b4) // stride
    it0 = np.maximum(0, -(-(sh4 - b4 - lane) // stride))    # the lane's first iteration inside the segment
    r = ((4 * (b4 + lane + it0 * stride) - o_sh) % row + (it - it0) * row_step) % row
    dc, rest = np.float32(lrs["sh_dc"]), np.float32(lrs["sh_rest"])
    for j in range(4):
        col = (r + j) % row
        is_dc = col < 3
        if mutate == "swap_dc_rest_column":     # column 2 (DC) takes the rest rate, column 3 (if any) the DC rate
            is_dc = (col < 2) | (col == 3)
        lr[4 * i + j] = np.where(is_dc, dc, rest)
    return lr


def adam1_emulated(N: int, K: int, p0, g, m0, v0, lrs, spec: AdamConsts, grad_scale: float = 1.0,
                   mutate: Optional[str] = None, max_blocks: int = MAX_BLOCKS, elem_range=None):
    """numpy fp32 emulation of the Adam launch over elem_range (the whole buffer by default; the elements outside it
    keep their values) -> (p1, m1, v1) float32.  Every operation rounds to fp32 where an fp32 kernel with explicit fmaf
    does:

        g' = s g;  m = fma(b1, m, (1 - b1) g');  v = fma(b2, v, ((1 - b2) g') g')
        p -= (lr (m (1 / bc1))) / fma(sqrt v, 1 / sqrt bc2, eps)

    ``mutate`` names one deliberate fault (MUTANTS): DC / rest rates swapped on one column; bias_corr2 not applied;
    row_step off by one (the DC position drifts after the first grid stride); grad_scale applied to m but not to v;
    the first pad behind the opacity segment takes its neighbour's gradient."""
    assert mutate is None or mutate in MUTANTS, mutate
    F = np.float32
    p0, g, m0, v0 = (np.asarray(x, dtype=F).reshape(-1) for x in (p0, g, m0, v0))
    lr = kernel_lr_emulated(N, K, lrs, max_blocks, mutate, elem_range)
    if mutate == "pad_takes_neighbour":
        _, start, n, end = segments(N, K)[0][3]
        assert end > start + n, "this shape has no pad behind the opacity segment"
        g = g.copy()
        g[start + n] = g[start + n - 1]
    b1, b2, eps = F(spec.beta1), F(spec.beta2), F(spec.eps)
    ibc1 = F(1) / F(spec.bias_corr1)
    isq = F(1) if mutate == "no_bias_corr2" else F(1) / np.sqrt(F(spec.bias_corr2))
    with np.errstate(under="ignore", over="ignore"):
        gs = g * F(grad_scale)
        gv = g if mutate == "grad_scale_m_only" else gs
        m1 = _fma32(np.broadcast_to(b1, m0.shape), m0, (F(1) - b1) * gs)
        v1 = _fma32(np.broadcast_to(b2, v0.shape), v0, ((F(1) - b2) * gv) * gv)
        denom = _fma32(np.sqrt(v1), np.broadcast_to(isq, v1.shape), np.broadcast_to(eps, v1.shape))
        p1 = p0 - (lr * (m1 * ibc1)) / denom
    if elem_range is not None:
        for new, old in ((p1, p0), (m1, m0), (v1, v0)):
            new[:elem_range[0]] = old[:elem_range[0]]
            new[elem_range[1]:] = old[elem_range[1]:]
    for x in (p1, m1, v1):
        assert x.dtype == F
    return p1, m1, v1
