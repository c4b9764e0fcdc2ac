"""NumPy fp64 reference of the patch-wise (local) Pearson term beside the global one (include/tgs.h,
tgs_depth_corr_local_fwd_bwd).  Pixels, x, y, alpha and validity are those of tests/depth_corr_ref.py.

Definitions (restated from the feature's specification):
  patches: k = patch_tiles tiles of 16 x 16 pixels on a side, grid origin shifted by (off_x, off_y) tiles, 0 <= off < k:
           tile (tx, ty) belongs to patch ((tx + off_x) // k, (ty + off_y) // k);  PW = ceil((TW + off_x) / k), PH likewise
  per patch p, over its valid pixels: n_p, means, vx_p, vy_p, c_p (centred, / n_p), rho_p = c_p / sqrt(vx_p vy_p),
           beta_p = c_p / vx_p
  active  <=>  n_p >= min_count  and  vx_p >= min_var_ratio * Vx  and  vy_p >= min_var_ratio * Vy  (Vx, Vy: the global
           variances)  and  vx_p vy_p > 0 and finite  and  the global frame is not degenerate
  A = number of active patches, rho_bar = mean of rho_p over them;
  loss = weight_global (1 - rho) + weight_local (1 - rho_bar), the local part 0 with zero gradient when A = 0
  gates are constants:  g_loc,i = -(weight_local / A) ((y_i - my_p) - beta_p (x_i - mx_p)) / (n_p sqrt(vx_p vy_p)) on a
           valid pixel of an active patch,  g = g_glob + g_loc,  v_depth = g / alpha,  v_alpha = -g x / alpha;  0 on invalid
           pixels.
"""
import math

import numpy as np

from tests.depth_corr_ref import depth_corr_ref

TILE = 16


def min_count_of(patch_tiles, min_fill):
    """The count gate the Python layer passes: max(2, ceil(min_fill (16 k)^2))."""
    return max(2, math.ceil(min_fill * (TILE * patch_tiles) ** 2))


def patch_grid(W, H, patch_tiles, off):
    """-> (PW, PH, patch index [H,W] of every pixel)."""
    k, (ox, oy) = patch_tiles, off
    TW, TH = -(-W // TILE), -(-H // TILE)
    PW, PH = -(-(TW + ox) // k), -(-(TH + oy) // k)
    yy, xx = np.mgrid[0:H, 0:W]
    pid = ((yy // TILE + oy) // k) * PW + (xx // TILE + ox) // k
    return PW, PH, pid


def depth_corr_local_ref(out_depth, final_T, mono, alpha_min=0.5, weight_global=1.0, weight_local=1.0, patch_tiles=8,
                         off=(0, 0), min_count=2, min_var_ratio=1e-3, active_override=None):
    """fp32 images [H,W] -> dict(stats [16] fp64, v_depth, v_alpha, scale [H,W] fp64, valid, alpha, x as depth_corr_ref,
    PW, PH, pid [H,W], and per patch [PW * PH]: n, rho, active, counted, ratio_x, ratio_y (vx_p / Vx, vy_p / Vy; nan where
    undefined)).

    ``scale`` = the global term's s_i plus the same expression formed with the patch's statistics and weight_local / A.
    ``active_override``: {patch index: bool} replaces the decision of the variance gate for those patches (the rendered-frame
    test hands over the kernel's decision for patches whose ratio lies within 10 % of the gate)."""
    g = depth_corr_ref(out_depth, final_T, mono, alpha_min, weight_global)
    H, W = g["x"].shape
    PW, PH, pid = patch_grid(W, H, patch_tiles, off)
    P = PW * PH
    valid, x, alpha = g["valid"], g["x"], g["alpha"]
    y = np.asarray(mono, np.float32).astype(np.float64)
    st = np.zeros(16)
    st[:8] = g["stats"]
    n_all, Vx, Vy = g["stats"][0], g["stats"][3], g["stats"][4]
    q = Vx * Vy
    frame_ok = n_all >= 2 and q > 0 and np.isfinite(q)
    n = np.zeros(P, np.int64)
    rho, ratio_x, ratio_y = np.zeros(P), np.full(P, np.nan), np.full(P, np.nan)
    active, counted = np.zeros(P, bool), np.zeros(P, bool)
    mom = {}
    for p in range(P):
        sel = valid & (pid == p)
        n[p] = sel.sum()
        counted[p] = n[p] >= min_count
        if n[p] == 0:
            continue
        xv, yv = x[sel], y[sel]
        mx, my = xv.mean(), yv.mean()
        dx, dy = xv - mx, yv - my
        vx, vy, c = (dx * dx).mean(), (dy * dy).mean(), (dx * dy).mean()
        if frame_ok:
            ratio_x[p], ratio_y[p] = vx / Vx, vy / Vy
        qp = vx * vy
        ok = bool(counted[p] and frame_ok and vx >= min_var_ratio * Vx and vy >= min_var_ratio * Vy)
        if active_override is not None and p in active_override:
            ok = bool(active_override[p]) and bool(counted[p]) and frame_ok
        ok = ok and qp > 0 and np.isfinite(qp)
        if ok:
            active[p] = True
            rho[p] = c / np.sqrt(qp)
            mom[p] = (sel, mx, my, vx, vy, c)
    A = int(active.sum())
    st[8], st[9] = counted.sum(), A
    v_depth, v_alpha, scale = g["v_depth"].copy(), g["v_alpha"].copy(), g["scale"].copy()
    if A > 0:
        st[10] = rho[active].mean()
        st[11] = weight_local * (1.0 - st[10])
        for p, (sel, mx, my, vx, vy, c) in mom.items():
            s, beta = np.sqrt(vx * vy), c / vx
            dx, dy = x[sel] - mx, y[sel] - my
            w = weight_local / A / (n[p] * s)
            gl = -w * (dy - beta * dx)
            v_depth[sel] += gl / alpha[sel]
            v_alpha[sel] += -gl * x[sel] / alpha[sel]
            scale[sel] += abs(w) * (np.abs(dy) + abs(beta) * np.abs(dx) + np.sqrt(vy) + abs(beta) * np.sqrt(vx))
    st[12] = st[7] + st[11]
    return dict(stats=st, v_depth=v_depth, v_alpha=v_alpha, scale=scale, valid=valid, alpha=alpha, x=x, PW=PW, PH=PH, pid=pid,
                n=n, rho=rho, active=active, counted=counted, ratio_x=ratio_x, ratio_y=ratio_y)
