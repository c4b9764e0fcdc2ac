"""Developer tool: what does the scale-invariant monocular depth term (tgs_depth_corr_fwd_bwd) cost?

Part 1, kernels.  On K6's own outputs of the two frames tools/depth_stats_time.py builds -- the object-centric 720p frame
and cfg3 at 1080p -- it times, in the same process and interleaved,

    ssim_fwd_bwd          K10 SSIM forward + gradient image on the frame's colour image          <- the yardstick
    depth_corr_forward    the tile-moment and fold launches (v_depth == v_alpha == NULL)
    depth_corr_full       all three launches; full - forward = the gradient-image launch

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept.
The algorithmic floor is 32 B per pixel (6 us at 720p at 5 TB/s): the launches are latency-bound, not bandwidth-bound.

Part 2, the step.  The object-centric 720p train step of tools/host_vs_gpu.py (300 k clustered Gaussians, 8 views, the
speculative budget, the next view announced) with mono_depth_mult 0 and 0.2 on two models from the same start,
interleaved: 5 repeats of 60 steps each per model, device events around the 60 steps.  The run with the term off issues
exactly the launches of a build without the feature: it is the reference.

Writes profiles/depth_corr_time.json (or --out).

--local times the patch-wise (local) term instead (tgs_depth_corr_local_fwd_bwd at patch_tiles = 8), against
the global op above as the reference of the same run:

    depth_corr_forward / depth_corr_full                 the global op, two / three launches
    depth_corr_local_forward / depth_corr_local_full     the new op, four / five launches

Per launch, by difference of the medians: local_forward - forward = k_dcorr_patches + k_dcorr_patch_sum, local_full -
local_forward = k_dcorr_grad_local, full - forward = k_dcorr_grad.  The step: mono_depth_mult 0.2 alone against
mono_depth_mult 0.2 + mono_depth_local_mult 0.2.  Writes profiles/depth_corr_local_time.json (or --out).

    python tools/depth_corr_time.py [--out profiles/depth_corr_time.json] [--skip-step]
    python tools/depth_corr_time.py --local [--out profiles/depth_corr_local_time.json] [--skip-step]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from depth_stats_time import FRAMES, build_frame

REPEATS, LAUNCHES, WARMUP = 5, 20, 10
STEP_REPEATS, STEPS, STEP_WARMUP = 5, 60, 60


def interleaved(variants, repeats, warm):
    for f in variants.values():
        warm(f)
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            n = f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / n)
    return times


def time_kernels(name, spec, dev, local=False):
    from touch_gs_amd import _lib, ops
    from touch_gs_amd.ops import ptr
    lib = _lib.load()
    model, cam, sp, ts, sg, budget = build_frame(spec, dev)
    rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts, opts=model.tuning.raster_opts())
    budget.check()
    H, W = cam.H, cam.W
    g = torch.Generator().manual_seed(1)
    dhat = depth / (1 - fT).clamp(min=1e-10)
    mono = ((0.37 * dhat + 0.11) * (1 + 0.1 * torch.randn(H, W, generator=g).to(dev))).clamp(min=1e-3).contiguous()
    gt = torch.rand(H, W, 3, generator=g).to(dev)
    tiles = torch.empty(cam.num_tiles, 8, device=dev)
    stats = torch.empty(8, device=dev)
    vd, va = torch.empty_like(depth), torch.empty_like(depth)
    bp = torch.empty(cam.num_tiles, device=dev)
    v_img, scratch = torch.empty_like(rgb), torch.empty(9 * H * W, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def corr(grad):
        def run():
            for _ in range(LAUNCHES):
                _lib.check(lib.tgs_depth_corr_fwd_bwd(W, H, ptr(depth), ptr(fT), ptr(mono), C.c_float(0.5), C.c_float(0.2), ptr(tiles),
                                                      ptr(stats), ptr(vd) if grad else None, ptr(va) if grad else None, stream),
                           "tgs_depth_corr_fwd_bwd")
            return LAUNCHES
        return run

    def ssim():
        for _ in range(LAUNCHES):
            _lib.check(lib.tgs_ssim_fwd_bwd(W, H, ptr(rgb), ptr(gt), C.c_float(-0.2 / (3 * H * W)), ptr(bp), ptr(v_img), ptr(scratch),
                                            stream), "tgs_ssim_fwd_bwd")
        return LAUNCHES

    variants = {"ssim_fwd_bwd": ssim, "depth_corr_forward": corr(False), "depth_corr_full": corr(True)}
    if local:
        k = 8
        TW, TH = (W + 15) // 16, (H + 15) // 16
        patches = torch.empty(((TW + k - 1) // k + 1) * ((TH + k - 1) // k + 1), 8, device=dev)
        stats16 = torch.empty(16, device=dev)
        min_count = ops.depth_corr_patch_min_count(k, 0.25)

        def corr_local(grad):
            def run():
                for i in range(LAUNCHES):   # the offsets of consecutive steps
                    _lib.check(lib.tgs_depth_corr_local_fwd_bwd(
                        W, H, ptr(depth), ptr(fT), ptr(mono), C.c_float(0.5), C.c_float(0.2), C.c_float(0.2), k, i % k, (i // k) % k,
                        min_count, C.c_float(1e-3), ptr(tiles), ptr(patches), ptr(stats16), ptr(vd) if grad else None,
                        ptr(va) if grad else None, stream), "tgs_depth_corr_local_fwd_bwd")
                return LAUNCHES
            return run
        variants.update(depth_corr_local_forward=corr_local(False), depth_corr_local_full=corr_local(True))
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    st = stats.cpu().tolist()
    if local:
        st16 = stats16.cpu().tolist()
        res = dict(label=spec["label"], width=W, height=H, tiles=cam.num_tiles, patch_tiles=8, valid_pixels=int(st[0]),
                   rho=round(st[6], 6), patches_counted=int(st16[8]), patches_active=int(st16[9]), rho_bar=round(st16[10], 6),
                   us_median={k: round(v, 2) for k, v in med.items()},
                   us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
                   us_by_difference=dict(
                       tiles_and_fold=round(med["depth_corr_forward"], 2),
                       grad_global=round(med["depth_corr_full"] - med["depth_corr_forward"], 2),
                       patches_and_patch_sum=round(med["depth_corr_local_forward"] - med["depth_corr_forward"], 2),
                       grad_local=round(med["depth_corr_local_full"] - med["depth_corr_local_forward"], 2)),
                   added_us_over_global=round(med["depth_corr_local_full"] - med["depth_corr_full"], 2),
                   ratio_to_global=round(med["depth_corr_local_full"] / med["depth_corr_full"], 4),
                   ratio_to_ssim=round(med["depth_corr_local_full"] / med["ssim_fwd_bwd"], 4),
                   patch_record_bytes=32 * patches.shape[0])
        print(name, json.dumps(res), flush=True)
        return res
    res = dict(label=spec["label"], width=W, height=H, tiles=cam.num_tiles, valid_pixels=int(st[0]), rho=round(st[6], 6),
               us_median={k: round(v, 2) for k, v in med.items()},
               us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               us_gradient_launch=round(med["depth_corr_full"] - med["depth_corr_forward"], 2),
               ratio_to_ssim=round(med["depth_corr_full"] / med["ssim_fwd_bwd"], 4),
               bytes_per_pixel=32, floor_us_at_5TBps=round(32 * W * H / 5e12 * 1e6, 2))
    print(name, json.dumps(res), flush=True)
    return res


def time_step(dev, N=300_000, W=1280, H=720, deg=3, nv=8, local=False):
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_views, synthetic_gaussians
    views, _ = make_views(N, W, H, deg, 77, dev, nv, clustered=True)
    for v in views:     # a raw monocular map: an affine map of the depth wherever the view has one
        v.mono_depth = torch.where(v.depth > 0, 3.0 * v.depth + 0.7, torch.zeros_like(v.depth)).contiguous()
    P, _ = synthetic_gaussians(N, W, H, deg, 78, clustered=True)
    models = {}
    for mult in (0.0, 0.2):     # --local: the LOCAL multiplier, beside a global one of 0.2 in both models
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True,
                                                    mono_depth_mult=0.2 if local else mult,
                                                    mono_depth_local_mult=mult if local else 0.0), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        models[mult] = m

    def steps(m, n):
        def run():
            for i in range(n):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return n
        return run

    tag = "mono_depth_local_mult" if local else "mono_depth_mult"
    variants = {f"{tag}_{mult}": steps(m, STEPS) for mult, m in models.items()}
    for m in models.values():
        steps(m, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    off, on = med[f"{tag}_0.0"], med[f"{tag}_0.2"]
    last = models[0.2].last
    loss = models[0.2].loss_from(last["tile_loss"], last["ssim_sum"], last["view"])
    res = dict(label="object-centric 720p train step: 300 k clustered Gaussians, 8 views, speculative budget", gaussians=N, width=W,
               height=H, us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               added_us_per_step=round(on - off, 1), added_fraction=round(on / off - 1, 4),
               replays={k: getattr(m, "speculative_replays", 0) for k, m in models.items()},
               mono_depth_loss_last_step=round(float(loss["mono_depth_loss"]), 6))
    if local:
        res.update(reference="mono_depth_mult 0.2 in both models; off = the global op alone, exactly as without the feature",
                   mono_depth_local_loss_last_step=round(float(loss["mono_depth_local_loss"]), 6),
                   active_patches_last_step=int(last["mono_stats"][9]))
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--local", action="store_true", help="time the patch-wise term against the global op (module docstring)")
    a = ap.parse_args()
    a.out = a.out or os.path.join("profiles", "depth_corr_local_time.json" if a.local else "depth_corr_time.json")
    if not torch.cuda.is_available():
        raise SystemExit("tools/depth_corr_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/depth_corr_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up; step: device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the "
                      f"two models after {STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="ssim_fwd_bwd: tgs_ssim_fwd_bwd (K10, forward + gradient image) on the same frame in the same process; "
                         "step: the same step with mono_depth_mult = 0, which issues no launch of the term",
               kernels={}, step=None)
    if a.local:
        out["yardstick"] = ("depth_corr_full: tgs_depth_corr_fwd_bwd (the global op) on the same frame in the same process; step: the "
                            "same step with mono_depth_mult 0.2 and mono_depth_local_mult 0, which calls the global op")
    for name in ("object720", "cfg3"):
        out["kernels"][name] = time_kernels(name, FRAMES[name], dev, a.local)
        torch.cuda.empty_cache()
    if not a.skip_step:
        out["step"] = time_step(dev, local=a.local)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
