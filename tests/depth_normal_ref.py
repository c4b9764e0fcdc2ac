"""NumPy fp64 reference of the depth-derived surface normals and the normal-prior loss (include/tgs.h,
tgs_depth_normal_fwd_bwd), an fp32 emulation of the kernels' arithmetic, and the synthetic inputs the CPU and GPU tests share.

Definitions (restated from the feature's specification):
  a = 1.0f - final_T in fp32;  valid  <=>  a >= alpha_min (fp32, on the stored bits);  alpha = max(a, 1e-10),  x = out_depth / alpha
  ray r(px, py) = ((px + pix_center - cx) / fx, (py + pix_center - cy) / fy, 1),  P = x r
  centre i FORMED  <=>  interior pixel, i and its neighbours l, r, u, d valid, max(|x_r - x_l|, |x_d - x_u|) <= max_jump x_i
      decided in fp32 (max_jump <= 0: no gate), and with t_x = P_r - P_l, t_y = P_d - P_u, m = t_y x t_x: |m| > 0 and finite
  n = m / |m|   (a fronto-parallel plane gives (0, 0, -1))
  centre i SUPERVISED  <=>  formed, |prior_i| > 0 and finite, c_i > 0;  p^ = prior / |prior|,  C = sum c_i (supervised)
  L = weight sum c_i (1 - n_i . p^_i) / C
  g_n = -(weight c_k / C) p^_k, g_m = (g_n - (g_n . n) n) / |m|, g_tx = g_m x t_y, g_ty = t_x x g_m (0 on unsupervised centres)
  G_j = r_j . (g_tx(left of j) - g_tx(right of j) + g_ty(above j) - g_ty(below j))
  v_depth = G / alpha,  v_alpha = -G x / alpha;  stats = {formed, supervised, C, sum c (1 - cos) / C, weight * [3], 0, 0, 0}
Condition numbers the bounds are stated in:
  kappa_i = ((|P_r| + |P_l|) / |t_x| + (|P_d| + |P_u|) / |t_y|) |t_x| |t_y| / |m|
  S_j = |r_j| sum over the four centres k that j feeds of (|weight| c_k / C) kappa_k |t_other,k| / |m_k|
        (t_other = t_y for a horizontal neighbour, t_x for a vertical one)
"""
import numpy as np

F32 = np.float32
UNIT = 2.0 ** -24
FLT_MIN = np.finfo(np.float32).tiny
CASES = [(16, 16, 20.0), (17, 19, 20.0), (33, 18, 40.0), (157, 93, 140.0), (320, 208, 300.0), (320, 208, 1200.0),
         (1280, 720, 900.0)]


def camera(W, H, fx):
    """The test camera of the specification, its parameters rounded to fp32 as TgsCamera stores them."""
    return dict(W=W, H=H, fx=float(F32(fx)), fy=float(F32(0.97 * fx)), cx=float(F32(W / 2 + 3.3)), cy=float(F32(H / 2 - 2.1)),
                pix_center=0.5)


def _nb(a):
    """The four neighbours (l, r, u, d) of the interior pixels of a [H,W,...] array, and the interior itself."""
    return a[1:-1, :-2], a[1:-1, 2:], a[:-2, 1:-1], a[2:, 1:-1], a[1:-1, 1:-1]


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def decisions(out_depth, final_T, alpha_min, max_jump):
    """The fp32 decisions, as the kernel makes them: valid [H,W], candidate centres [H,W] (interior, five valid pixels, jump
    gate passed) and the jump-gate ratio jump / threshold of the interior centres with five valid pixels (fp64, NaN
    elsewhere; inf where the threshold is 0)."""
    od, T = np.asarray(out_depth, F32), np.asarray(final_T, F32)
    H, W = od.shape
    a = F32(1.0) - T
    valid = a >= F32(alpha_min)
    cand = np.zeros((H, W), bool)
    ratio = np.full((H, W), np.nan)
    if H < 3 or W < 3:
        return valid, cand, ratio
    with np.errstate(all="ignore"):
        x = od / np.maximum(a, F32(1e-10))
        vl, vr, vu, vd, vi = _nb(valid)
        five = vl & vr & vu & vd & vi
        xl, xr, xu, xd, xi = _nb(x)
        jump = np.maximum(np.abs(xr - xl), np.abs(xd - xu))
        thr = F32(max_jump) * xi
        gate = (jump <= thr) if max_jump > 0 else np.ones_like(five)
        cand[1:-1, 1:-1] = five & gate
        ratio[1:-1, 1:-1] = np.where(five, jump.astype(np.float64) / thr.astype(np.float64), np.nan)
    return valid, cand, ratio


def _rays(cam, dtype=np.float64):
    W, H = cam["W"], cam["H"]
    c = {k: dtype(cam[k]) for k in ("fx", "fy", "cx", "cy", "pix_center")}
    if dtype is F32:     # the kernels multiply by 1 / fx, 1 / fy rounded once
        rx = (np.arange(W).astype(dtype) + c["pix_center"] - c["cx"]) * (F32(1) / c["fx"])
        ry = (np.arange(H).astype(dtype) + c["pix_center"] - c["cy"]) * (F32(1) / c["fy"])
    else:
        rx = (np.arange(W).astype(dtype) + c["pix_center"] - c["cx"]) / c["fx"]
        ry = (np.arange(H).astype(dtype) + c["pix_center"] - c["cy"]) / c["fy"]
    r = np.empty((H, W, 3), dtype)
    r[..., 0], r[..., 1], r[..., 2] = rx[None, :], ry[:, None], dtype(1.0)
    return r


def _prior_terms(prior, conf, shape, dtype=np.float64):
    """p^ [H,W,3], c [H,W] and the mask of pixels whose prior supervises (|prior| > 0 and finite in fp32, c > 0)."""
    H, W = shape
    if prior is None:
        z3 = np.zeros((H, W, 3), dtype)
        return (z3 if dtype is np.float64 else (z3, np.ones((H, W), dtype))), np.zeros((H, W), dtype), np.zeros((H, W), bool)
    p32 = np.asarray(prior, F32)
    c32 = np.ones((H, W), F32) if conf is None else np.asarray(conf, F32)
    with np.errstate(all="ignore"):
        q2 = (p32 * p32).sum(-1, dtype=F32)       # the kernels decide on the squared length: a normal fp32 number
        ok = (q2 >= FLT_MIN) & np.isfinite(q2) & (c32 > 0)
        p = p32.astype(dtype)
        if dtype is np.float64:
            phat = np.where(ok[..., None], p / np.where(ok, _norm(p), 1)[..., None], 0.0)
        else:                                     # the kernels keep q and |q| and divide once, after their dot product
            phat = (np.where(ok[..., None], p, F32(0)), np.where(ok, np.sqrt(q2), F32(1)))
    return phat, np.where(ok, c32, 0).astype(dtype), ok


def geometry(cam, x):
    """fp64: t_x, t_y, m [H,W,3], |m| [H,W] on the interior centres (0 elsewhere) and P [H,W,3], r [H,W,3]."""
    H, W = x.shape
    r = _rays(cam)
    P = x[..., None] * r
    tx, ty = np.zeros_like(P), np.zeros_like(P)
    if H >= 3 and W >= 3:
        Pl, Pr, Pu, Pd, _ = _nb(P)
        tx[1:-1, 1:-1], ty[1:-1, 1:-1] = Pr - Pl, Pd - Pu
    m = np.cross(ty, tx)
    return tx, ty, m, _norm(m), P, r


def loss_fp64(cam, out_depth, a, sup, phat, c, weight):
    """The loss as a function of fp64 images with the supervised set and C held constant (for finite differences)."""
    x = out_depth / np.maximum(a, 1e-10)
    _, _, m, ml, _, _ = geometry(cam, x)
    n = m[sup] / ml[sup][:, None]
    C = c[sup].sum()
    return weight * (c[sup] * (1.0 - (n * phat[sup]).sum(-1))).sum() / C


def _gather(gtx, gty):
    """sum_j = g_tx(left of j) - g_tx(right of j) + g_ty(above j) - g_ty(below j), 0 outside the image."""
    s = np.zeros_like(gtx)
    s[:, 1:] += gtx[:, :-1]
    s[:, :-1] -= gtx[:, 1:]
    s[1:, :] += gty[:-1, :]
    s[:-1, :] -= gty[1:, :]
    return s


def depth_normal_ref(cam, out_depth, final_T, prior=None, conf=None, alpha_min=0.5, max_jump=0.1, weight=1.0):
    """fp32 images -> dict of fp64 results: stats [8], normals [H,W,3], formed / supervised / valid [H,W] bool, v_depth, v_alpha,
    G, kappa, S, alpha, x [H,W], phat [H,W,3], c [H,W], gate_ratio [H,W]."""
    valid, cand, ratio = decisions(out_depth, final_T, alpha_min, max_jump)
    od = np.asarray(out_depth, F32).astype(np.float64)
    a = (F32(1.0) - np.asarray(final_T, F32)).astype(np.float64)
    alpha = np.maximum(a, 1e-10)
    H, W = od.shape
    with np.errstate(all="ignore"):
        x = od / alpha
        tx, ty, m, ml, P, r = geometry(cam, x)
        formed = cand & (ml > 0) & np.isfinite(ml)
        n = np.where(formed[..., None], m / np.where(formed, ml, 1)[..., None], 0.0)
        phat, c, pok = _prior_terms(prior, conf, (H, W))
        sup = formed & pok
        stats = np.zeros(8)
        stats[0], stats[1] = formed.sum(), sup.sum()
        out = dict(stats=stats, normals=n, formed=formed, supervised=sup, valid=valid, alpha=alpha, x=x, phat=phat, c=c,
                   gate_ratio=ratio, v_depth=np.zeros((H, W)), v_alpha=np.zeros((H, W)), G=np.zeros((H, W)),
                   kappa=np.zeros((H, W)), S=np.zeros((H, W)))
        # kappa on the formed centres
        Pn = _norm(P)
        txl, tyl = _norm(tx), _norm(ty)
        if H >= 3 and W >= 3:
            pl, pr, pu, pd, _ = _nb(Pn)
            k = np.zeros((H, W))
            k[1:-1, 1:-1] = ((pr + pl) / txl[1:-1, 1:-1] + (pd + pu) / tyl[1:-1, 1:-1]) * (txl * tyl / ml)[1:-1, 1:-1]
            out["kappa"] = np.where(formed, k, 0.0)
        if not sup.any():
            return out
        C = c[sup].sum()
        cos = (n * phat).sum(-1)
        mean = (c[sup] * (1.0 - cos[sup])).sum() / C
        stats[2], stats[3], stats[4] = C, mean, weight * mean
        s3 = sup[..., None]
        gn = -(weight * c / C)[..., None] * phat
        gm = np.where(s3, (gn - (gn * n).sum(-1)[..., None] * n) / np.where(sup, ml, 1)[..., None], 0.0)
        gtx, gty = np.cross(gm, ty), np.cross(tx, gm)
        G = (r * _gather(gtx, gty)).sum(-1)
        out["G"], out["v_depth"], out["v_alpha"] = G, G / alpha, -G * x / alpha
        wk = np.where(sup, abs(weight) * c / C * out["kappa"] / np.where(sup, ml, 1), 0.0)
        wtx, wty = wk * tyl, wk * txl      # a horizontal neighbour's weight carries |t_y|, a vertical one's |t_x|
        S = np.zeros((H, W))
        S[:, 1:] += wtx[:, :-1]
        S[:, :-1] += wtx[:, 1:]
        S[1:, :] += wty[:-1, :]
        S[:-1, :] += wty[1:, :]
        out["S"] = _norm(r) * S
    return out


def depth_normal_emulated(cam, out_depth, final_T, prior=None, conf=None, alpha_min=0.5, max_jump=0.1, weight=1.0):
    """A straightforward fp32 transcription of the kernels' arithmetic (no FMA contraction; rays by a product with 1 / fx,
    the prior's length divided out once after the dot products, g_m by a product with 1 / |m|; C from an fp64 sum rounded to fp32 as the fold kernel leaves it in stats[2]) -> dict(normals [H,W,3] fp32, formed, supervised, G [H,W] fp32, stats)."""
    valid, cand, _ = decisions(out_depth, final_T, alpha_min, max_jump)
    od, T = np.asarray(out_depth, F32), np.asarray(final_T, F32)
    H, W = od.shape
    with np.errstate(all="ignore"):
        x = od / np.maximum(F32(1.0) - T, F32(1e-10))
        r = _rays(cam, F32)
        P = x[..., None] * r
        tx, ty = np.zeros_like(P), np.zeros_like(P)
        if H >= 3 and W >= 3:
            Pl, Pr, Pu, Pd, _ = _nb(P)
            tx[1:-1, 1:-1], ty[1:-1, 1:-1] = Pr - Pl, Pd - Pu
        cr = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                    a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        dt = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        m = cr(ty, tx)
        m2 = dt(m, m)
        formed = cand & (m2 >= FLT_MIN) & np.isfinite(m2)
        ml = np.sqrt(np.where(formed, m2, F32(1)))
        n = np.where(formed[..., None], m / ml[..., None], F32(0))
        (q, pl), c, pok = _prior_terms(prior, conf, (H, W), F32)
        sup = formed & pok
        assert n.dtype == F32 and q.dtype == F32 and pl.dtype == F32 and c.dtype == F32
        stats = np.zeros(8)
        stats[0], stats[1] = formed.sum(), sup.sum()
        out = dict(normals=n, formed=formed, supervised=sup, G=np.zeros((H, W), F32), stats=stats)
        if not sup.any():
            return out
        term = c * (F32(1) - dt(n, q) / pl)
        C = F32(c[sup].astype(np.float64).sum())
        stats[2] = C
        stats[3] = term[sup].astype(np.float64).sum() / float(C)
        stats[4] = weight * stats[3]
        lamC = F32(weight) / C
        gn = (-(lamC * c) / pl)[..., None] * q
        d = dt(gn, n)
        gm = np.where(sup[..., None], (F32(1) / ml)[..., None] * (gn - d[..., None] * n), F32(0))
        gtx, gty = cr(gm, ty), cr(tx, gm)
        # what a centre hands its right / left / lower / upper neighbour pixel: r . g with that neighbour's ray
        rp = np.pad(r, ((1, 1), (1, 1), (0, 0)))
        z = lambda a: np.pad(a, ((1, 1), (1, 1)))
        to_r, to_l = z(dt(rp[1:-1, 2:], gtx)), z(-dt(rp[1:-1, :-2], gtx))
        to_d, to_u = z(dt(rp[2:, 1:-1], gty)), z(-dt(rp[:-2, 1:-1], gty))
        G = ((to_r[1:-1, :-2] + to_l[1:-1, 2:]) + to_d[:-2, 1:-1]) + to_u[2:, 1:-1]
        assert G.dtype == F32
        out["G"] = G
    return out


def synthetic(W, H, seed, fx=None):
    """The test images of the specification -> dict(cam, out_depth, final_T [H,W] fp32, prior [H,W,3] fp32, conf [H,W] fp32)."""
    rng = np.random.default_rng(seed)
    py, px = np.mgrid[0:H, 0:W].astype(np.float64)
    D = 1.2 + 0.25 * np.sin(px / 23 + 0.3) * np.cos(py / 19) + 0.1 * px / (W - 1) + 0.002 * rng.standard_normal((H, W))
    box = (px > 0.55 * W) & (px < 0.8 * W) & (py > 0.2 * H) & (py < 0.6 * H)
    D = np.where(box, D - 0.4, D)
    u = rng.random((H, W))
    alpha = np.where(np.sin(px / 9) * np.sin(py / 7) > 0.93, 0.3 * u, 0.6 + 0.4 * u)
    final_T = (1.0 - alpha).astype(F32)
    a32 = F32(1.0) - final_T
    out_depth = (D * a32).astype(F32)
    prior = (np.array([0.0, 0.0, -1.0]) + 0.2 * rng.standard_normal((H, W, 3))) * (0.5 + rng.random((H, W, 1)))
    prior = np.where(rng.random((H, W, 1)) < 0.1, 0.0, prior).astype(F32)
    conf = 0.2 + rng.random((H, W))
    conf = np.where(rng.random((H, W)) < 0.1, 0.0, conf).astype(F32)
    cam = camera(W, H, fx if fx is not None else 20.0)
    return dict(cam=cam, out_depth=out_depth, final_T=final_T, prior=prior, conf=conf)


def assert_margins(out_depth, final_T, alpha_min=0.5, max_jump=0.1):
    """No alpha within 0.05 of alpha_min and no jump ratio within [0.8, 1.25] of its threshold: no count depends on a rounding."""
    a32 = F32(1.0) - np.asarray(final_T, F32)
    assert not ((a32 > alpha_min - 0.05) & (a32 < alpha_min + 0.05)).any(), "an alpha lies within 0.05 of alpha_min"
    if max_jump > 0:
        _, _, ratio = decisions(out_depth, final_T, alpha_min, max_jump)
        q = ratio[np.isfinite(ratio)]
        near = (q >= 0.8) & (q <= 1.25)
        assert not near.any(), f"{int(near.sum())} jump ratios lie within [0.8, 1.25] of the threshold"


def max_errors(got_normals, got_vd, got_va, ref):
    """The observed errors in the units of the bounds: max |n - n_ref|_inf / (kappa_i 2^-24) over the formed centres and
    max |v - v_ref| / (2^-24 S_j / alpha_j) resp. / (2^-24 S_j |x_j| / alpha_j) over the pixels with S_j > 0."""
    f, s = ref["formed"], ref["S"] > 0
    out = {}
    if got_normals is not None:
        en = np.abs(np.asarray(got_normals, np.float64) - ref["normals"]).max(-1)
        out["normals"] = float((en[f] / (ref["kappa"][f] * UNIT)).max()) if f.any() else 0.0
    if got_vd is not None and s.any():
        ud = UNIT * ref["S"][s] / ref["alpha"][s]
        out["v_depth"] = float((np.abs(np.asarray(got_vd, np.float64)[s] - ref["v_depth"][s]) / ud).max())
        out["v_alpha"] = float((np.abs(np.asarray(got_va, np.float64)[s] - ref["v_alpha"][s]) / (ud * np.abs(ref["x"][s]))).max())
    return out
