"""References of the two MCMC kernels (csrc/mcmc.hip): the relocation by its definition in 80-digit ``decimal``, the
regulariser gradient and the noise displacement in fp64, and an fp32 NumPy emulation of the noise term.

RELOCATION (gsplat's ``compute_relocation``).  For a row with logit l (an fp32 value, converted exactly), split r ways:

    o = 1 / (1 + exp(-l)),   x = 1 - (1 - o)^(1/r),
    S = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)                       (``reloc_sum_definition``)
    new logit = logit(clamp(x, min_opacity, 1 - 2^-23)),   log-scale += log(o / S)

``reloc_sum_single`` is the hockey-stick form  S = sum_{k<r} C(r, k+1) (-1)^k x^(k+1) / sqrt(k+1)  (sum_{i=k+1..r} C(i-1, k)
= C(r, k+1)); tests/test_cpu_mcmc.py holds the two equal in ``decimal``.  The kernel evaluates the single sum in fp64 and
rounds once, so its bound is  |out - ref| <= 2^-23 |ref| + 2^-40  -- one fp32 rounding (2^-24 relative) of an fp64 result whose
own error stays below 1e-10 (cancellation sum|terms| / |S| <= 2.9e4 at o = 1 - 2^-23, r = 51, times 2^-53 per term),
with a factor 2 of room; 2^-40 absorbs a reference of exactly 0 (logit(1/2)).

REGULARISER.  d/d(ol) of lambda_o mean(sigmoid(ol)) = lambda_o / N * o (1 - o);  d/d(ls_j) of lambda_s mean(exp(ls)) (the mean
over all 3N scales) = lambda_s / (3N) * exp(ls_j)  (``reg_grad``; tied to torch autograd in fp64 by tests/test_cpu_mcmc.py).
The kernel forms  c_o * (e / ((1 + e) (1 + e))), e = expf(-|ol|), c_o = lambda_o / (float) N  and  c_s * expf(ls_j), and adds
them to the buffer's gradient.  Roundings, in units of E = 2^-24 relative to |reg|: expf <= 1 ulp = 2E; 1 + e: E of its own
+ at most E from e (e / (1 + e) <= 1/2); the square 2 x 2E + E = 5E; the quotient 2E + 5E + E = 8E; c_o one division = E; the
product E: 10E.  The scale term: expf 2E, c_s E, the product E: 4E.  The sum g + reg rounds once more: at most E |g + reg|
<= E |g| + E |reg|, of which E |reg| is counted here and E |g| sits inside the slack adam_ref's bounds keep over their measured
worst (m: 2.4E + E <= 4E; v: 4.4E + 2E <= 8E).  C_REG = 12 covers both terms:  dg = C_REG E |reg|.

NOISE.  From the UPDATED ol', ls', q' (the kernel's own fp32 results, converted exactly) and the draw n:

    o' = sigmoid(ol'),  t = gate_k (o' - gate_o0),  gate = 0 if t > 80 else 1 / (1 + exp(t)),  R = R(q' / |q'|),
    delta = (noise_lr lr_means gate) R diag(exp(ls')^2) R^T n                                              (``noise_ref``)

and its un-cancelled mass  A_j = noise_lr lr_means gate sum_k |R_jk| s_k^2 sum_l |R_lk| |n_l|.  The kernel's displacement is
held to  C_NOISE E (1 + gate_k o') A_j : the factor (1 + gate_k o') is the gate's sensitivity -- d gate / gate = -(1 - gate) dt
and dt is a few E of gate_k o' + |t| E.  Roundings of an fp32 evaluation without contraction (``noise_emulated``): o' 4 (expf
2, the sum, the divide), t 2, gate 4, the scale 2, |q|^2 4, sqrt, 1 / sqrt, each component 1, an entry of R about 6, s^2 3
(expf 2, the square), R^T n 5, times s^2 1, R v 5, times the scale 1: about 30 in a row, far fewer on average.  Measured with
``measure_noise_constant`` (2^20 samples, seed 0: ls' uniform in [-8, 1], ol' uniform in [-12, 12] with a quarter clustered
around logit(0.005), |q'| log-uniform in [0.1, 3], n standard normal):

    mass A_j (entries |R_jk|)     worst 45 406 E (seeds 1, 2: 19 673, 37 281), 99.9th percentile 67 E, 99.999th 2 800 E
    mass T_j (terms, below)       worst 12.0 E (seeds 1, 2: 11.5, 12.1),       99.9th percentile 4.5 E

The long tail under A_j is not an fp32 accident of the emulation: an entry of R such as 1 - 2 (y^2 + z^2) that cancels to nearly
0 carries an ABSOLUTE error of a few E, A_j weighs it by its small |R_jk|, and with scales of a ratio up to e^18 between the axes
the error of that entry times the large s_k^2 is compared with a mass made of the small ones.  C_NOISE = twice the measured
worst, as for every constant here, is therefore 90 813: that bound still refuses a wrong gate, a transposed rotation or a
missing square of the scale on most rows (each changes delta by a multiple of A_j), but it is 0.5 % of A_j.  The kernel is held
to a SECOND, sharper bound beside it:  C_NOISE_T E (1 + gate_k o') T_j  with the term-wise mass T_j = A_j with every |R_jk| replaced
by the sum of the absolute values of its terms (1 + 2 (y^2 + z^2), 2 (|x y| + |w z|), ...), under which nothing cancels
unseen: C_NOISE_T = 2 x 12.1 = 24.2, consistent with the count above.
"""
import math
from decimal import Decimal, getcontext

import numpy as np

E = 2.0 ** -24
C_REG = 12.0             # roundings of a regulariser term, in units of E |reg| (module docstring)
NOISE_MEASURED = 45406.5   # worst ratio of noise_emulated over 2^20 samples, in units of E (1 + gate_k o') A_j
C_NOISE = 2.0 * NOISE_MEASURED
NOISE_MEASURED_T = 12.1    # ... in units of E (1 + gate_k o') T_j, the term-wise mass
C_NOISE_T = 2.0 * NOISE_MEASURED_T
RELOC_MAX = 51
T_CUT = 80.0             # gate = 0 beyond

RELOC_O = (0.005, 0.006, 0.01, 0.05, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999, 0.99999, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -23)
RELOC_R = (1, 2, 3, 8, 20, 51)


def f32(x) -> float:
    return float(np.float32(x))


def logit32(o: float) -> float:
    """The fp32 logit of o (what a parameter buffer holds)."""
    return f32(math.log(o) - math.log1p(-o))


# ---------------------------------------------------------------------------------------------------------------------
# relocation, 80 digits
# ---------------------------------------------------------------------------------------------------------------------
def _ctx():
    getcontext().prec = 80


def reloc_x(l: float, r: int):
    """(o, x) as Decimals for the fp32 logit l."""
    _ctx()
    L = Decimal(l)
    o = 1 / (1 + (-L).exp())
    one_minus_o = 1 / (1 + L.exp())
    x = 1 - (one_minus_o.ln() / r).exp()
    return o, x


def reloc_sum_definition(x: Decimal, r: int) -> Decimal:
    _ctx()
    S = Decimal(0)
    for i in range(1, r + 1):
        for k in range(i):
            S += math.comb(i - 1, k) * (-1) ** k * x ** (k + 1) / Decimal(k + 1).sqrt()
    return S


def reloc_sum_single(x: Decimal, r: int) -> Decimal:
    _ctx()
    return sum((math.comb(r, k + 1) * (-1) ** k * x ** (k + 1) / Decimal(k + 1).sqrt() for k in range(r)), Decimal(0))


def relocation_ref(l: float, ratio: int, min_opacity: float, definition: bool = True):
    """-> (new logit, increment of every log-scale, sum|terms| / |S|) as floats; ratio is clamped to 51, min_opacity is taken
    as the fp32 value a C float carries."""
    _ctx()
    r = min(int(ratio), RELOC_MAX)
    o, x = reloc_x(l, r)
    S = reloc_sum_definition(x, r) if definition else reloc_sum_single(x, r)
    mass = sum(math.comb(r, k + 1) * x ** (k + 1) / Decimal(k + 1).sqrt() for k in range(r))
    xc = min(max(x, Decimal(f32(min_opacity))), 1 - Decimal(2) ** -23)
    return float((xc / (1 - xc)).ln()), float((o / S).ln()), float(mass / abs(S))


_GRID = {}


def relocation_grid(min_opacity: float = 0.005, extra_ratios=()):
    """The rows of the relocation tests, computed once per argument set: (logits fp32 [n], ratios int32 [n], reference new
    logit [n], reference log-scale increment [n]) over RELOC_O x (RELOC_R + extra_ratios)."""
    key = (min_opacity, tuple(extra_ratios))
    if key not in _GRID:
        ls, rs, nl, dl = [], [], [], []
        for o in RELOC_O:
            for r in RELOC_R + tuple(extra_ratios):
                l = logit32(o)
                a, b, _ = relocation_ref(l, r, min_opacity)
                ls.append(l), rs.append(r), nl.append(a), dl.append(b)
        _GRID[key] = (np.asarray(ls, np.float32), np.asarray(rs, np.int32), np.asarray(nl), np.asarray(dl))
    return _GRID[key]


# ---------------------------------------------------------------------------------------------------------------------
# regulariser, noise: fp64
# ---------------------------------------------------------------------------------------------------------------------
def reg_grad(ol, ls, opacity_reg: float, scale_reg: float):
    """-> (d/d ol [N], d/d ls [N,3]) of  opacity_reg mean(sigmoid(ol)) + scale_reg mean(exp(ls)), fp64, the weights rounded to
    fp32 first (C float fields)."""
    ol, ls = np.asarray(ol, np.float64), np.asarray(ls, np.float64)
    N = ol.shape[0]
    e = np.exp(-np.abs(ol))
    return f32(opacity_reg) / N * e / (1.0 + e) ** 2, f32(scale_reg) / (3.0 * N) * np.exp(ls)


def _rot(q, terms=False):
    """R(q) of unit quaternions [N,4] (w, x, y, z) -> [N,3,3]; terms: the sum of the absolute values of every entry's terms."""
    w, x, y, z = (q[:, i] for i in range(4))
    if terms:
        a = np.abs
        return np.stack([1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(w * z)), 2 * (a(x * z) + a(w * y)),
                         2 * (a(x * y) + a(w * z)), 1 + 2 * (x * x + z * z), 2 * (a(y * z) + a(w * x)),
                         2 * (a(x * z) + a(w * y)), 2 * (a(y * z) + a(w * x)), 1 + 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)
    return R.reshape(-1, 3, 3)


def noise_ref(ol, ls, q, n, noise_lr: float, lr_means: float, gate_k: float, gate_o0: float):
    """-> (delta [N,3], A [N,3], o' [N], gate [N], t [N], T [N,3]) in fp64 from the fp32 arrays (converted exactly) and the fp32-rounded
    constants."""
    ol, ls, q, n = (np.asarray(a, np.float64) for a in (ol, ls, q, n))
    k, o0 = f32(gate_k), f32(gate_o0)
    scale = f32(noise_lr) * f32(lr_means)
    o = 1.0 / (1.0 + np.exp(-ol))
    t = k * (o - o0)
    with np.errstate(over="ignore"):
        gate = np.where(t > T_CUT, 0.0, 1.0 / (1.0 + np.exp(t)))
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    R, Rt = _rot(qn), _rot(qn, terms=True)
    s2 = np.exp(ls) ** 2
    v = s2 * np.einsum("nlk,nl->nk", R, n)
    delta = (scale * gate)[:, None] * np.einsum("njk,nk->nj", R, v)
    A = (scale * gate)[:, None] * np.einsum("njk,nk->nj", np.abs(R), s2 * np.einsum("nlk,nl->nk", np.abs(R), np.abs(n)))
    T = (scale * gate)[:, None] * np.einsum("njk,nk->nj", Rt, s2 * np.einsum("nlk,nl->nk", Rt, np.abs(n)))
    return delta, A, o, gate, t, T


def gate_edge_slack(A, gate, t, noise_lr: float, lr_means: float):
    """Where t lies within 1e-3 of the cut an fp32 t may fall on the other side of it (its rounding is 80 E ~ 5e-6): there the
    displacement may be that of the open gate, 1 / (1 + exp(80)) ~ 1.8e-35 times the mass, or 0.  -> that much, [N,3]."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        open_mass = np.where(gate[:, None] > 0, A, A * 0.0)
    near = np.abs(t - T_CUT) < 1e-3
    # (a closed reference gate has A = 0: rebuild the open mass from an upper bound of the gate, exp(-79))
    return np.where(near[:, None], np.maximum(open_mass, math.exp(-79.0) * f32(noise_lr) * f32(lr_means) * 1e3), 0.0)


def noise_emulated(ol, ls, q, n, noise_lr: float, lr_means: float, gate_k: float, gate_o0: float):
    """The kernel's noise term operation by operation in fp32 NumPy (no contraction: csrc/build.sh compiles mcmc.hip with
    -ffp-contract=off) -> delta float32 [N,3], exactly 0 where the gate is closed."""
    F = np.float32
    ol, ls, q, n = (np.asarray(a, F) for a in (ol, ls, q, n))
    one, two = F(1), F(2)
    with np.errstate(over="ignore", under="ignore"):
        o = one / (one + np.exp(-ol))
        t = F(gate_k) * (o - F(gate_o0))
        gate = np.where(t > F(T_CUT), F(0), one / (one + np.exp(np.minimum(t, F(T_CUT)))))
        c = (F(noise_lr) * F(lr_means)) * gate
        inv = one / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        w, x, y, z = (q[:, i] * inv for i in range(4))
        R = [one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
             two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
             two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]
        v = []
        for k in range(3):
            s = np.exp(ls[:, k])
            v.append((s * s) * ((R[k] * n[:, 0] + R[3 + k] * n[:, 1]) + R[6 + k] * n[:, 2]))
        out = np.stack([c * ((R[3 * j] * v[0] + R[3 * j + 1] * v[1]) + R[3 * j + 2] * v[2]) for j in range(3)], -1)
    assert out.dtype == F
    return out


def noise_inputs(N: int, rng: np.random.Generator):
    """(ol, ls, q, n) float32: logits in [-12, 12] with a quarter clustered around logit(0.005) where the gate turns (and
    many beyond t = 80: o' > 0.805), log-scales in [-8, 1], |q| log-uniform in [0.1, 3], standard normal draws."""
    ol = rng.uniform(-12.0, 12.0, N)
    cl = rng.random(N) < 0.25
    ol[cl] = logit32(0.005) + rng.normal(0.0, 0.5, int(cl.sum()))
    ls = rng.uniform(-8.0, 1.0, (N, 3))
    q = rng.standard_normal((N, 4))
    q *= (np.exp(rng.uniform(math.log(0.1), math.log(3.0), N)) / np.linalg.norm(q, axis=1))[:, None]
    n = rng.standard_normal((N, 3))
    return tuple(a.astype(np.float32) for a in (ol, ls, q, n))


def noise_ratio(delta, ol, ls, q, n, noise_lr, lr_means, gate_k, gate_o0):
    """Worst |delta - reference| in units of E (1 + gate_k o') A_j and of E (1 + gate_k o') T_j."""
    ref, A, o, gate, t, T = noise_ref(ol, ls, q, n, noise_lr, lr_means, gate_k, gate_o0)
    err = np.maximum(np.abs(np.asarray(delta, np.float64) - ref) - gate_edge_slack(A, gate, t, noise_lr, lr_means), 0.0)
    out = []
    for mass in (A, T):
        unit = E * (1.0 + f32(gate_k) * o)[:, None] * mass
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
        out.append(float(ratio.max()))
    return tuple(out)


def measure_noise_constant(samples: int = 1 << 20, seed: int = 0):
    """The worst ratios of the fp32 emulation under both masses (NOISE_MEASURED, NOISE_MEASURED_T were taken from this call)."""
    ol, ls, q, n = noise_inputs(samples, np.random.default_rng(seed))
    kw = dict(noise_lr=5e5, lr_means=1.6e-4, gate_k=100.0, gate_o0=0.005)
    return noise_ratio(noise_emulated(ol, ls, q, n, **kw), ol, ls, q, n, **kw)
