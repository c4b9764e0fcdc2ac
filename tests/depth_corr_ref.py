"""NumPy fp64 reference of the scale-invariant monocular depth loss (include/tgs.h, tgs_depth_corr_fwd_bwd) and the
synthetic inputs the CPU and GPU tests share.

Definitions (restated from the feature's specification):
  alpha = max(1 - final_T, 1e-10),  x = out_depth / alpha,  y = mono
  valid  <=>  mono > 0  and  (1.0f - final_T) >= alpha_min       -- compared in fp32, on the stored bits
  over the valid pixels: n, mx, my, vx, vy, c (centred second moments / n), rho = c / sqrt(vx vy), beta = c / vx
  d rho / d x_i = ((y_i - my) - beta (x_i - mx)) / (n sqrt(vx vy)),   g_i = -weight * d rho / d x_i
  v_depth_i = g_i / alpha_i,   v_alpha_i = -g_i x_i / alpha_i   (gradient with respect to 1 - final_T);  0 on invalid pixels
  degenerate (n < 2, or vx vy not > 0 or not finite): rho = 0, loss 0, all gradients 0.
"""
import numpy as np


def valid_mask(final_T, mono, alpha_min):
    """The validity decision in fp32, as the kernel makes it."""
    T, m = np.asarray(final_T, np.float32), np.asarray(mono, np.float32)
    return (m > np.float32(0)) & ((np.float32(1.0) - T) >= np.float32(alpha_min))


def depth_corr_ref(out_depth, final_T, mono, alpha_min=0.5, weight=1.0):
    """fp32 images [H,W] -> dict(stats [8] fp64, v_depth, v_alpha, scale [H,W] fp64, valid [H,W] bool, alpha, x [H,W] fp64).

    ``scale`` = s_i = (weight / (n sqrt(vx vy))) (|y_i - my| + |beta| |x_i - mx| + sqrt(vy) + |beta| sqrt(vx)): the size of
    the terms g_i is formed from (the constant part because a pixel at the mean has a gradient of exactly the size of
    fp32's rounding of x - mx)."""
    valid = valid_mask(final_T, mono, alpha_min)
    od, T, y = (np.asarray(a, np.float32).astype(np.float64) for a in (out_depth, final_T, mono))
    alpha = np.maximum(1.0 - T, 1e-10)
    x = od / alpha
    n = int(valid.sum())
    stats = np.zeros(8)
    stats[0] = n
    out = dict(stats=stats, v_depth=np.zeros_like(x), v_alpha=np.zeros_like(x), scale=np.zeros_like(x), valid=valid,
               alpha=alpha, x=x)
    if n == 0:
        return out
    xv, yv = x[valid], y[valid]
    mx, my = xv.mean(), yv.mean()
    dx, dy = xv - mx, yv - my
    vx, vy, c = (dx * dx).mean(), (dy * dy).mean(), (dx * dy).mean()
    stats[1:6] = mx, my, vx, vy, c
    q = vx * vy
    if n < 2 or not (q > 0) or not np.isfinite(q):
        return out
    s = np.sqrt(q)
    rho, beta = c / s, c / vx
    stats[6], stats[7] = rho, weight * (1.0 - rho)
    g = -weight / (n * s) * (dy - beta * dx)
    out["v_depth"][valid] = g / alpha[valid]
    out["v_alpha"][valid] = -g * xv / alpha[valid]
    out["scale"][valid] = abs(weight) / (n * s) * (np.abs(dy) + abs(beta) * np.abs(dx) + np.sqrt(vy) + abs(beta) * np.sqrt(vx))
    return out


def synthetic_images(W, H, rel_noise, seed):
    """The test images of the specification (fp32 [H,W]: out_depth, final_T, mono).

    Depth in [0.5, 2] with smooth structure plus noise.  Alpha: 20 % of the pixels below 0.45 -- 5 % (of all) exactly 0 --,
    the rest above 0.55, so no pixel sits within 0.05 of alpha_min = 0.5.  mono = (0.37 D + 0.11) (1 + ``rel_noise`` N(0, 1)),
    kept positive; 10 % of the pixels zeroed."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    smooth = 0.5 + 0.5 * (np.sin(xx / 17.0 + 0.3) * np.cos(yy / 11.0) + 1.0) + 0.2 * (xx / max(W - 1, 1)) + 0.15 * (yy / max(H - 1, 1))
    D = np.clip(smooth + 0.15 * rng.random((H, W)), 0.5, 2.0)
    u = rng.random((H, W))
    alpha = np.where(u < 0.05, 0.0, np.where(u < 0.20, 0.45 * rng.random((H, W)), 0.55 + 0.45 * rng.random((H, W))))
    final_T = (1.0 - alpha).astype(np.float32)
    a32 = np.float32(1.0) - final_T
    assert not ((a32 > 0.45) & (a32 < 0.55)).any()
    out_depth = (D * a32).astype(np.float32)
    mono = (0.37 * D + 0.11) * (1.0 + rel_noise * rng.standard_normal((H, W)))
    mono = np.where(rng.random((H, W)) < 0.10, 0.0, np.maximum(mono, 1e-3)).astype(np.float32)
    return out_depth, final_T, mono


def max_errors(got_stats, got_vd, got_va, ref):
    """Observed errors in the units of the bounds: |rho - rho_ref|, largest relative error of n, means and moments, and the
    largest |v - v_ref| / (s_i / alpha_i) (v_depth) resp. / (s_i x_i / alpha_i) (v_alpha) over the valid pixels."""
    st = np.asarray(got_stats, np.float64)
    r = ref["stats"]
    v = ref["valid"]
    rel = np.abs(st[:6] - r[:6]) / np.abs(r[:6])
    ud = ref["scale"][v] / ref["alpha"][v]
    ua = ud * np.abs(ref["x"][v])
    ed = np.abs(np.asarray(got_vd, np.float64)[v] - ref["v_depth"][v]) / ud
    ea = np.abs(np.asarray(got_va, np.float64)[v] - ref["v_alpha"][v]) / ua
    return dict(rho=abs(st[6] - r[6]), loss=abs(st[7] - r[7]), moments=rel.max(), v_depth=ed.max(), v_alpha=ea.max())
