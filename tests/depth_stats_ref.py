"""fp64 reference of the depth-statistics pass (tgs_rasterize_depth_stats): per pixel the variance of depth along the
ray around the expected depth, and the median depth / Gaussian.

Composed from the untouched oracle -- ``oracle.torch_oracle.project`` + ``bin_and_sort`` make the lists
(``depth_stats_ref_scene``) -- plus a per-tile walk of its own that restates the inclusion rules of App. B.6 exactly as
``oracle.blend`` does (skip sigma < 0, skip alpha < 1/255, clamp 0.999, stop at T' <= 1e-4 excluding that entry), so that
its alpha and expected depth equal ``blend``'s (tests/test_cpu_depth_stats.py ties them to 1e-12).

    var    = sum_i w_i (d_i - Dhat)^2 / max(alpha, 1e-10),  Dhat = sum_i w_i d_i / max(alpha, 1e-10),  alpha = 1 - T_final
    median = the first INCLUDED entry, front to back, with T' = T (1 - alpha_i) <= 1/2;  id -1 / depth 0 if there is none
    med_margin = min over the included entries of |T' - 1/2| / (1/2): a pixel whose margin is tiny may pick a
                 neighbouring entry under fp32 rounding (the counterpart of blend's ``margin`` for the new threshold)
"""
import numpy as np
import torch

from oracle import torch_oracle as O


def depth_stats_ref(xy, conic, opac, depth, sorted_gid, tile_start, cam):
    """Per-tile walk on projected Gaussians (the arguments of ``oracle.blend`` without the colours) -> dict of [H,W]
    arrays: alpha, dhat, var (float64), median_gid (int64), median_depth (float64), med_margin (float64)."""
    dt = torch.float64
    xy, conic, opac, depth = (t.detach().to(dt) for t in (xy, conic, opac, depth))
    W, H = cam.W, cam.H
    TW, TH = cam.tiles
    B = O.BLOCK
    alpha_img = torch.zeros(H, W, dtype=dt)
    dhat_img = torch.zeros(H, W, dtype=dt)
    var_img = torch.zeros(H, W, dtype=dt)
    mgid_img = torch.full((H, W), -1, dtype=torch.int64)
    mdep_img = torch.zeros(H, W, dtype=dt)
    mmar_img = torch.full((H, W), float("inf"), dtype=dt)
    for ty in range(TH):
        for tx in range(TW):
            t = ty * TW + tx
            s, e = int(tile_start[t]), int(tile_start[t + 1])
            if e <= s:
                continue
            g = torch.from_numpy(np.asarray(sorted_gid[s:e]).astype(np.int64))
            ys = torch.arange(ty * B, min((ty + 1) * B, H))
            xs = torch.arange(tx * B, min((tx + 1) * B, W))
            py, px = torch.meshgrid(ys, xs, indexing="ij")
            pxf = px.reshape(-1).to(dt) + cam.pix_center
            pyf = py.reshape(-1).to(dt) + cam.pix_center
            dx = xy[g, 0][:, None] - pxf[None, :]
            dy = xy[g, 1][:, None] - pyf[None, :]
            a, b, c = conic[g, 0][:, None], conic[g, 1][:, None], conic[g, 2][:, None]
            sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
            araw = opac[g][:, None] * torch.exp(-sigma)
            al = araw + (torch.clamp(araw, max=O.ALPHA_MAX) - araw)        # (blend's own expression of the clamp)
            skip = (sigma < 0) | (al < O.ALPHA_MIN)
            a_eff = torch.where(skip, torch.zeros_like(al), al)
            Tp = torch.cumprod(1 - a_eff, dim=0)
            Tb = torch.cat([torch.ones_like(Tp[:1]), Tp[:-1]], dim=0)
            inc = (Tp > O.T_STOP) & ~skip
            w = torch.where(inc, a_eff * Tb, torch.zeros_like(a_eff))
            Tfin = torch.prod(torch.where(inc, 1 - a_eff, torch.ones_like(a_eff)), dim=0)
            alpha = 1 - Tfin
            den = torch.clamp(alpha, min=1e-10)
            d = depth[g][:, None]
            dhat = (w * d).sum(0) / den
            var = (w * (d - dhat[None, :]) ** 2).sum(0) / den
            cross = inc & (Tp <= 0.5)
            n = e - s
            pos = torch.arange(n)[:, None].expand(n, pxf.shape[0])
            first = torch.where(cross, pos, torch.full_like(pos, n)).min(dim=0).values
            has = first < n
            mg = torch.where(has, g[first.clamp(max=n - 1)], torch.full_like(first, -1))
            md = torch.where(has, depth[g][first.clamp(max=n - 1)], torch.zeros_like(dhat))
            mm = torch.where(inc, (Tp - 0.5).abs() / 0.5, torch.full_like(Tp, float("inf"))).min(dim=0).values
            hh, ww = ys.numel(), xs.numel()
            sl = (slice(ty * B, ty * B + hh), slice(tx * B, tx * B + ww))
            alpha_img[sl] = alpha.view(hh, ww)
            dhat_img[sl] = dhat.view(hh, ww)
            var_img[sl] = var.view(hh, ww)
            mgid_img[sl] = mg.view(hh, ww)
            mdep_img[sl] = md.view(hh, ww)
            mmar_img[sl] = mm.view(hh, ww)
    return dict(alpha=alpha_img.numpy(), dhat=dhat_img.numpy(), var=var_img.numpy(), median_gid=mgid_img.numpy(),
                median_depth=mdep_img.numpy(), med_margin=mmar_img.numpy())


def depth_stats_ref_scene(P, cam, deg):
    """Raw parameters -> (reference dict, oracle.blend dict with margin, projection, sorted_gid, tile_start)."""
    pr = O.project(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], cam, deg)
    gid, tstart = O.bin_and_sort(pr["rect"], pr["valid"], pr["depth"], cam)
    ref = depth_stats_ref(pr["xy"], pr["conic"], pr["opac"], pr["depth"], gid, tstart, cam)
    out = O.blend(pr["xy"], pr["conic"], pr["opac"], pr["rgb"], pr["depth"], gid, tstart, cam, want_margin=True)
    return ref, out, pr, gid, tstart


def clear_pixels(blend_out, ref, tol=1e-4):
    """Decision-clear pixels: every threshold test of the walk (alpha >= 1/255, T' > 1e-4: blend's margin) and the
    median's T' <= 1/2 test keep a relative distance >= tol from their thresholds."""
    margin = blend_out["margin"]
    margin = margin.numpy() if hasattr(margin, "numpy") else np.asarray(margin)
    return (margin >= tol) & (ref["med_margin"] >= tol)
