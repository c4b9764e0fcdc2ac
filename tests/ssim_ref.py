"""Torch fp64 reference of K10 (include/tgs.h, tgs_ssim_fwd_bwd / tgs_ssim_fwd_bwd_rows) in explicit formulas -- no
autograd, so it shares nothing with oracle/torch_oracle.py but the definition -- and the input regimes the CPU and GPU
tests share.

Definitions (11-tap Gaussian window g, sigma 1.5, normalised in fp64; G = g g^T, zero padding; per channel):
  mu1 = G*x, mu2 = G*y, E11 = G*x^2, E22 = G*y^2, E12 = G*xy          (x = img, y = gt)
  s11 = E11 - mu1^2, s22 = E22 - mu2^2, s12 = E12 - mu1 mu2
  n1 = 2 mu1 mu2 + C1, n2 = 2 s12 + C2, d1 = mu1^2 + mu2^2 + C1, d2 = s11 + s22 + C2,   C1 = 1e-4, C2 = 9e-4
  map m = n1 n2 / (d1 d2)
  adjoint maps (csrc/imgloss.hip):  C = dm/dE12 = 2 n1 / (d1 d2),   B = dm/dE11 = -m / d2,
      A = dm/dmu1 (total) = 2 mu2 n2 / (d1 d2) - 2 m mu1 / d1 - 2 mu1 B - mu2 C
  v_img = weight * (G*A + 2 x (G*B) + y (G*C))  =  weight * d(sum of m)/dx

The conditioning unit of the map:  u = 2^-24 (cond / d2 + 8),
  cond = E11 + mu1^2 + E22 + mu2^2 + 2 |E12| + 2 |mu1 mu2| + C2  -- the magnitudes of the terms that cancel in n2 and d2; one
  fp32 rounding (2^-24 relative) of them moves n2 / d2 by cond / d2 roundings; the + 8 covers the closing products and the
  two 1-ulp reciprocals.  On noise cond / d2 is a few units; on a flat bright image d2 ~ C2 and it is ~ 4000.

``dtype=torch.float32`` evaluates the very same formulas in fp32 on the CPU, ``separable`` as two 11-tap passes or as one
121-tap convolution: two kernel-independent measurements of what the formula itself costs in fp32 on a given input (the
"fp32 floor" the GPU tests scale their gradient bounds with).
"""
import types

import torch
import torch.nn.functional as F

WIN, HALO = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
REGIMES = ("uniform", "smooth", "converged", "flat_bright", "white_vs_grey", "white", "black", "identical", "mixed")


def window(dtype=torch.float64):
    """The 11 weights: computed and normalised in fp64, then rounded to ``dtype`` (the kernels' constants for fp32)."""
    x = torch.arange(WIN, dtype=torch.float64) - HALO
    g = torch.exp(-(x * x) / (2 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def _filter(x, g, separable):
    """G * x, zero padded, for x [1,3,H,W]."""
    if separable:
        h = F.conv2d(x, g.view(1, 1, 1, WIN).expand(3, 1, 1, WIN), padding=(0, HALO), groups=3)
        return F.conv2d(h, g.view(1, 1, WIN, 1).expand(3, 1, WIN, 1), padding=(HALO, 0), groups=3)
    return F.conv2d(x, (g[:, None] * g[None, :]).expand(3, 1, WIN, WIN), padding=HALO, groups=3)


def ssim_ref(img, gt, weight=1.0, dtype=torch.float64, separable=True):
    """fp32 images [H,W,3] -> namespace(map, v_img, unit, mass), each [H,W,3] of ``dtype``.

    ``mass`` = |weight| (G*|A| + 2 |x| (G*|B|) + |y| (G*|C|)): the un-cancelled size of the terms v_img is summed from."""
    x = img.detach().cpu().float().to(dtype).permute(2, 0, 1)[None].contiguous()
    y = gt.detach().cpu().float().to(dtype).permute(2, 0, 1)[None].contiguous()
    g = window(dtype)
    f = lambda t: _filter(t, g, separable)
    mu1, mu2, e11, e22, e12 = f(x), f(y), f(x * x), f(y * y), f(x * y)
    s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    n1, n2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2
    d1, d2 = mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
    m = n1 * n2 / (d1 * d2)
    Cm = 2 * n1 / (d1 * d2)
    Bm = -m / d2
    Am = 2 * mu2 * n2 / (d1 * d2) - 2 * m * mu1 / d1 - 2 * mu1 * Bm - mu2 * Cm
    v = weight * (f(Am) + 2 * x * f(Bm) + y * f(Cm))
    mass = abs(weight) * (f(Am.abs()) + 2 * x.abs() * f(Bm.abs()) + y.abs() * f(Cm.abs()))
    cond = e11 + mu1 * mu1 + e22 + mu2 * mu2 + 2 * e12.abs() + 2 * (mu1 * mu2).abs() + C2
    unit = 2.0 ** -24 * (cond / d2 + 8)
    hwc = lambda t: t[0].permute(1, 2, 0).contiguous()
    return types.SimpleNamespace(map=hwc(m), v_img=hwc(v), unit=hwc(unit), mass=hwc(mass))


def row_sums(t, c0=0, c1=None):
    """Per-row sums (fp64, [c1 - c0]) of a map or unit image [H,W,3] over the rows [c0, c1)."""
    c1 = t.shape[0] if c1 is None else c1
    return t[c0:c1].double().sum(dim=(1, 2))


def fp32_floor(img, gt, weight, ref=None):
    """The two fp32 evaluations against the fp64 one -> namespace(f_max, f_l2, evals): the larger max|v32 - v64| and
    ||v32 - v64||_2 of the two, and the two fp32 results (separable, 121-tap)."""
    ref = ref if ref is not None else ssim_ref(img, gt, weight)
    evals = [ssim_ref(img, gt, weight, dtype=torch.float32, separable=s) for s in (True, False)]
    d = [(e.v_img.double() - ref.v_img) for e in evals]
    return types.SimpleNamespace(f_max=max(float(t.abs().max()) for t in d), f_l2=max(float(t.norm()) for t in d), evals=evals)


def smooth_base(W, H, g):
    """The full-size test's base image: uniform noise on a coarse grid, bilinearly interpolated."""
    lo = torch.rand(1, 3, H // 40 + 2, W // 40 + 2, generator=g, dtype=torch.float64)
    return F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)


def inputs(regime, W, H):
    """(img, gt): fp32 [H,W,3] in [0, 1], fixed seeds (a function of the regime and the size only)."""
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + 7 * W + H)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    const = lambda v: torch.full((H, W, 3), v, dtype=torch.float64)
    if regime == "uniform":
        img = rand(H, W, 3)
        gt = img + 0.2 * randn(H, W, 3)
    elif regime == "smooth":
        gt = smooth_base(W, H, g)
        img = gt + 0.1 * randn(H, W, 3)
    elif regime == "converged":
        gt = smooth_base(W, H, g)
        img = gt + 1e-3 * randn(H, W, 3)
    elif regime == "flat_bright":
        img = 0.95 + 1e-3 * randn(H, W, 3)
        gt = 0.95 + 1e-3 * randn(H, W, 3)
    elif regime == "white_vs_grey":
        img, gt = const(1.0), const(0.95)
    elif regime == "white":
        img, gt = const(1.0), const(1.0)
    elif regime == "black":
        img, gt = const(0.0), const(0.0)
    elif regime == "identical":
        img = rand(H, W, 3)
        gt = img.clone()
    elif regime == "mixed":
        img = rand(H, W, 3)
        gt = img + 0.2 * randn(H, W, 3)
        h = W // 2
        img[:, h:] = 0.95 + 1e-3 * randn(H, W - h, 3)
        gt[:, h:] = 0.95
        # one block of exact 1.0 (straddling the two halves) and one of exact 0.0 (in the noisy half), in both images
        y0, y1, y2 = H // 8, H // 8 + max(H // 4, 1), min(H // 8 + 2 * max(H // 4, 1), H)
        for t in (img, gt):
            t[y0:y1, max(h - W // 8, 0):h + max(W // 8, 1)] = 1.0
            t[y1:y2, W // 16:W // 16 + max(W // 4, 1)] = 0.0
    else:
        raise ValueError(regime)
    return img.clamp(0, 1).float().contiguous(), gt.clamp(0, 1).float().contiguous()
