"""Developer tool: what does the normal-prior op (tgs_depth_normal_fwd_bwd) cost?

Part 1, kernels.  The protocol of tools/depth_corr_time.py: on K6's own outputs of the object-centric 720p frame and of cfg3 at
1080p it times, in the same process and interleaved,

    depth_corr_full        tgs_depth_corr_fwd_bwd, all three launches                                  <- the yardstick
    depth_normal_forward   k_dnorm_tiles + k_dnorm_fold (v_depth == v_alpha == NULL, no normals image)
    depth_normal_normals   the same two launches writing the normals image (what get_outputs(normals=True) runs)
    depth_normal_full      all three launches; full - forward = k_dnorm_grad
    depth_normal_full_acc  all three with accumulate = 1 (the gradient launch also reads the two images)

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept.  The
prior is the op's own normals plus noise, with weights.  By bytes the op moves about 70 B per pixel (x, validity, prior and
weight read in each of two passes with 1.27x / 1.56x halo re-reads, 8 B written) against the yardstick's 32: it should cost
at most 2.5 x the yardstick.

Part 2, the step.  The object-centric 720p train step of tools/depth_corr_time.py with normal_prior_mult 0 and 0.1 on two
models from the same start, interleaved: 5 repeats of 60 steps each per model.  The run with the term off issues exactly the
launches of a build without the feature.

    python tools/depth_normal_time.py [--out profiles/depth_normal_time.json] [--skip-step]
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

from depth_corr_time import LAUNCHES, REPEATS, STEP_REPEATS, STEP_WARMUP, STEPS, interleaved
from depth_stats_time import FRAMES, build_frame

BOUND = 2.5


def time_kernels(name, spec, dev):
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
    n0 = ops.depth_normals(cam, depth, fT, 0.5, 0.1)
    prior = (n0 + 0.2 * torch.randn(H, W, 3, generator=g).to(dev)).contiguous()
    conf = (0.2 + torch.rand(H, W, generator=g)).to(dev).contiguous()
    cs = cam.c_struct()
    tiles8, tiles4 = torch.empty(cam.num_tiles, 8, device=dev), torch.empty(cam.num_tiles, 4, device=dev)
    stats, nstats = torch.empty(8, device=dev), torch.empty(8, device=dev)
    vd, va = torch.zeros_like(depth), torch.zeros_like(depth)
    normals = torch.empty(H, W, 3, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def corr():
        for _ in range(LAUNCHES):
            _lib.check(lib.tgs_depth_corr_fwd_bwd(W, H, ptr(depth), ptr(fT), ptr(mono), C.c_float(0.5), C.c_float(0.2), ptr(tiles8),
                                                  ptr(stats), ptr(vd), ptr(va), stream), "tgs_depth_corr_fwd_bwd")
        return LAUNCHES

    def normal(grad, want_normals=False, acc=0):
        def run():
            if acc:
                vd.zero_(); va.zero_()     # (the sums stay finite over the repeats)
            for _ in range(LAUNCHES):
                _lib.check(lib.tgs_depth_normal_fwd_bwd(C.byref(cs), ptr(depth), ptr(fT), ptr(prior), ptr(conf), C.c_float(0.5),
                                                        C.c_float(0.1), C.c_float(0.1), ptr(tiles4), ptr(nstats),
                                                        ptr(normals) if want_normals else None, ptr(vd) if grad else None,
                                                        ptr(va) if grad else None, acc, stream), "tgs_depth_normal_fwd_bwd")
            return LAUNCHES
        return run

    variants = {"depth_corr_full": corr, "depth_normal_forward": normal(False), "depth_normal_normals": normal(False, True),
                "depth_normal_full": normal(True), "depth_normal_full_acc": normal(True, acc=1)}
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    st = nstats.cpu().tolist()
    ratio = med["depth_normal_full"] / med["depth_corr_full"]
    res = dict(label=spec["label"], width=W, height=H, tiles=cam.num_tiles, formed=int(st[0]), supervised=int(st[1]),
               mean_one_minus_cos=round(st[3], 6),
               us_median={k: round(v, 2) for k, v in med.items()},
               us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               us_by_difference=dict(tiles_and_fold=round(med["depth_normal_forward"], 2),
                                     normals_image=round(med["depth_normal_normals"] - med["depth_normal_forward"], 2),
                                     grad=round(med["depth_normal_full"] - med["depth_normal_forward"], 2),
                                     accumulate=round(med["depth_normal_full_acc"] - med["depth_normal_full"], 2)),
               ratio_to_depth_corr=round(ratio, 4), ratio_acc_to_depth_corr=round(med["depth_normal_full_acc"] / med["depth_corr_full"], 4),
               bound=BOUND, within_bound=bool(ratio <= BOUND))
    print(name, json.dumps(res), flush=True)
    return res


def time_step(dev, N=300_000, W=1280, H=720, deg=3, nv=8):
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_views, synthetic_gaussians
    views, _ = make_views(N, W, H, deg, 77, dev, nv, clustered=True)
    for v in views:     # a prior wherever the view's depth map forms a normal: the normals of that depth
        v.normal_prior = ops.depth_normals(v.cam, v.depth, (v.depth <= 0).float(), 0.5, 0.1)
    P, _ = synthetic_gaussians(N, W, H, deg, 78, clustered=True)
    models = {}
    for mult in (0.0, 0.1):
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True,
                                                    normal_prior_mult=mult), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        models[mult] = m

    def steps(m, n):
        def run():
            for i in range(n):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return n
        return run

    variants = {f"normal_prior_mult_{mult}": steps(m, STEPS) for mult, m in models.items()}
    for m in models.values():
        steps(m, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    off, on = med["normal_prior_mult_0.0"], med["normal_prior_mult_0.1"]
    last = models[0.1].last
    loss = models[0.1].loss_from(last["tile_loss"], last["ssim_sum"], last["view"])
    res = dict(label="object-centric 720p train step: 300 k clustered Gaussians, 8 views, speculative budget", gaussians=N, width=W,
               height=H, us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               added_us_per_step=round(on - off, 1), added_fraction=round(on / off - 1, 4),
               replays={k: getattr(m, "speculative_replays", 0) for k, m in models.items()},
               normal_loss_last_step=round(float(loss["normal_loss"]), 6), supervised_last_step=int(last["normal_stats"][1]))
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "depth_normal_time.json"))
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/depth_normal_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/depth_normal_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up; step: device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the "
                      f"two models after {STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="depth_corr_full: tgs_depth_corr_fwd_bwd (all three launches) on the same frame in the same process; the op "
                         f"should cost at most {BOUND} x it.  step: the same step with normal_prior_mult = 0, which issues no launch "
                         "of the term",
               kernels={}, step=None)
    for name in ("object720", "cfg3"):
        out["kernels"][name] = time_kernels(name, FRAMES[name], dev)
        torch.cuda.empty_cache()
    if not a.skip_step:
        out["step"] = time_step(dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
