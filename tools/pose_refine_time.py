"""Developer tool: what does the camera-pose gradient (tgs_pose_grad) cost?

Part 1, kernels.  On one built frame of cfg3 (1 M Gaussians, 1080p) and of the object-centric 720p model -- front half,
K6 and K7 through the model, so that the partial records are a real frame's -- it times, in the same process and interleaved,

    k8_unfused         tgs_project_bwd from the partials (k_project_bwd_lds: reads what the pose kernel reads AND writes 59 floats)
    pose_grad          tgs_pose_grad: k_pose_grad + k_pose_grad_final
    pose_grad_no_sh    the same with sh = NULL: paths 1 and 2 alone, no SH row is read
    pose_final_empty   tgs_pose_grad at N = 0: k_pose_grad_final over no rows, i.e. the floor of one launch

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept.
By its reads the pose kernel should cost about the read half of the unfused K8; no number is aimed at.

Part 2, the step.  The train step of tools/depth_corr_time.py (object-centric 720p, and cfg3) with pose refinement off and
on, two models from the same start, interleaved: 5 repeats of 60 steps per model.  The run with refinement off issues
exactly the launches of a build without the feature.

    python tools/pose_refine_time.py [--out profiles/pose_refine_time.json] [--skip-step]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from depth_corr_time import LAUNCHES, REPEATS, STEP_REPEATS, STEP_WARMUP, STEPS, interleaved
from depth_stats_time import FRAMES, build_frame


def time_kernels(name, spec, dev, deg=3):
    from touch_gs_amd import ops
    model, cam, sp, ts, sg, budget = build_frame(spec, dev)
    p = model.params
    # the frame once more with its group bases, then K6 and K7 against a random target: real partial records
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, budget)
    rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts, opts=model.tuning.raster_opts())
    budget.check()
    g = torch.Generator().manual_seed(1)
    gt = torch.rand(cam.H, cam.W, 3, generator=g).to(dev)
    partials, _ = ops.rasterize_bwd(cam, sp, gb, sg, ts, rgb, depth, fT, loss=dict(gt_rgb=gt, l1_weight=1.0 / (3 * cam.H * cam.W)),
                                    want_tile_loss=True)
    grads = p.grad_views()
    G = (p.N + 255) // 256
    out = (torch.empty(32, device=dev), torch.empty(G, 25, device=dev))
    e3, e4, e12 = torch.empty(0, 3, device=dev), torch.empty(0, 4, device=dev), torch.empty(0, 12, device=dev)

    def k8():
        for _ in range(LAUNCHES):
            ops.project_bwd(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, sp, group_base=gb, partials=partials, out=grads)
        return LAUNCHES

    def pose():
        for _ in range(LAUNCHES):
            ops.pose_grad(cam, p.means, p.log_scales, p.quats, p.sh, deg, sp, group_base=gb, partials=partials, out=out)
        return LAUNCHES

    out0 = (torch.empty(32, device=dev), torch.empty(1, 25, device=dev))

    def floor():
        for _ in range(LAUNCHES):
            ops.pose_grad(cam, e3, e3, e4, None, -1, e12, v_splats=e12, out=out0)
        return LAUNCHES

    out1 = (torch.empty(32, device=dev), torch.empty(G, 25, device=dev))

    def pose_no_sh():
        for _ in range(LAUNCHES):
            ops.pose_grad(cam, p.means, p.log_scales, p.quats, None, -1, sp, group_base=gb, partials=partials, out=out1)
        return LAUNCHES

    times = interleaved({"k8_unfused": k8, "pose_grad": pose, "pose_grad_no_sh": pose_no_sh, "pose_final_empty": floor}, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    res32 = out[0].cpu().tolist()
    res = dict(label=spec["label"], gaussians=p.N, groups=G, width=cam.W, height=cam.H, visible=int(res32[25]), valid=int(res32[24]),
               us_median={k: round(v, 2) for k, v in med.items()}, us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               ratio_to_k8_unfused=round(med["pose_grad"] / med["k8_unfused"], 4))
    print(name, json.dumps(res), flush=True)
    return res


def time_step(spec, dev, deg=3, nv=8):
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_views, synthetic_gaussians
    N, W, H = spec["N"], spec["W"], spec["H"]
    P, _ = synthetic_gaussians(N, W, H, deg, 78, clustered=spec["clustered"])
    models, vsets = {}, {}
    for on in (False, True):
        views, _ = make_views(N, W, H, deg, 77, dev, nv, clustered=spec["clustered"])   # each model its own views: poses move
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        kw = dict(pose_lr_rot=1e-5, pose_lr_trans=1e-5) if on else {}
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True, **kw), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        m.enable_pose_refinement(views)
        models[on], vsets[on] = m, views

    def steps(on, n):
        m, views = models[on], vsets[on]

        def run():
            for i in range(n):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return n
        return run

    variants = {f"refinement_{'on' if on else 'off'}": steps(on, STEPS) for on in models}
    for on, m in models.items():
        steps(on, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    off, on = med["refinement_off"], med["refinement_on"]
    dl = models[True].pose_refiner.deltas()
    res = dict(label=spec["label"] + f", {nv} views, fused optimizer, speculative budget", gaussians=N, width=W, height=H,
               us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               added_us_per_step=round(on - off, 1), added_fraction=round(on / off - 1, 4),
               replays={("on" if k else "off"): getattr(m, "speculative_replays", 0) for k, m in models.items()},
               dropped_results=sum(s.dropped for s in models[True].pose_refiner._slots.values()),
               mean_pose_delta_deg=round(sum(a for a, _ in dl) / len(dl), 5))
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "pose_refine_time.json"))
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/pose_refine_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/pose_refine_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up; step: device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the "
                      f"two models after {STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="k8_unfused: tgs_project_bwd from the same partial records in the same process.  step: the same step "
                         "with refinement off, which issues no launch of the feature",
               kernels={}, step={})
    for name in ("object720", "cfg3"):
        out["kernels"][name] = time_kernels(name, FRAMES[name], dev)
        torch.cuda.empty_cache()
        if not a.skip_step:
            out["step"][name] = time_step(FRAMES[name], dev)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
