"""Developer tool: what does the depth-statistics pass (tgs_rasterize_depth_stats) cost next to K6?

Builds the two frames the kernel work is judged on -- cfg3 (1 M Gaussians, 1080p, Morton order: bench.py's headline
frame) and the object-centric 720p frame of tools/host_vs_gpu.py (300 k clustered Gaussians, lists of 700 - 1600
entries) --, runs the front half ONCE per frame and then times, on the same lists in the same process,

    K6   tgs_rasterize_fwd in render-only form (stop_pos == NULL)         <- the yardstick
    K6s  tgs_rasterize_depth_stats with stop_pos == NULL and with the forward's stop positions

interleaved, with device events: 5 repeats of 20 back-to-back launches each after a warm-up, median of the repeats.
The pass carries two accumulators per pixel where K6 carries five: it should take no longer than K6; 10 % over K6
(the box-to-box drift of kernel times, README) is the allowance.  Writes profiles/depth_stats_time.json (or --out).

    python tools/depth_stats_time.py [--out profiles/depth_stats_time.json] [--frames cfg3 object720]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

REPEATS, LAUNCHES, WARMUP = 5, 20, 10

FRAMES = {
    "cfg3": dict(N=1_000_000, W=1920, H=1080, seed=1236, clustered=False,
                 label="cfg3: 1 M Gaussians, 1080p, Morton order"),
    "object720": dict(N=300_000, W=1280, H=720, seed=78, clustered=True,
                      label="object-centric: 300 k clustered Gaussians, 720p, Morton order"),
}


def build_frame(spec, dev, deg=3):
    """Front half of one frame through the model (so that the re-sort's per-model kernel tuning applies, as in training)."""
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_camera, synthetic_gaussians
    P, intr = synthetic_gaussians(spec["N"], spec["W"], spec["H"], deg, spec["seed"], clustered=spec["clustered"])
    params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
    model = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, spatial_sort=True), params)
    cam = make_camera(intr, 1, 8)
    # the re-sort chooses the model's kernel tuning (long_run, K6 split shape) from the cameras of its recent steps:
    # this frame's camera stands in for them, as after a training step on it
    model._recent_cams = {id(cam): cam}
    model.spatial_sort()
    p = model.params
    budget = ops.IntersectBudget()
    cam = model.tuned(cam)
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, budget)
    return model, cam, sp, ts, sg, budget


def time_frame(name, spec, dev):
    from touch_gs_amd import _lib, ops
    from touch_gs_amd.ops import _tile_start_len, ptr
    lib = _lib.load()
    model, cam, sp, ts, sg, budget = build_frame(spec, dev)
    opts = model.tuning.raster_opts()
    T = cam.num_tiles
    n = (ts[1:T + 1] - ts[:T]).long()
    # the publishing forward: images + stop positions the pass consumes
    rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts, opts=opts)
    stop = fT.stop_pos
    var = torch.empty_like(depth)
    med = torch.empty_like(depth)
    gid = torch.empty(cam.H, cam.W, dtype=torch.int32, device=dev)
    rgb2, depth2, fT2 = torch.empty_like(rgb), torch.empty_like(depth), torch.empty_like(fT)
    cs = cam.c_struct()
    order = ptr(ts.tile_order)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tlen = _tile_start_len(ts)

    def k6():
        _lib.check(lib.tgs_rasterize_fwd(C.byref(cs), ptr(sp), ptr(sg), ptr(ts), tlen, order, ptr(rgb2), ptr(depth2), ptr(fT2),
                                         None, None, None, C.byref(opts), stream), "tgs_rasterize_fwd")

    def stats(stop_pos):
        def run():
            _lib.check(lib.tgs_rasterize_depth_stats(C.byref(cs), ptr(sp), ptr(sg), ptr(ts), tlen, order, ptr(depth), ptr(fT),
                                                     ptr(stop_pos), ptr(var), ptr(med), ptr(gid), C.byref(opts), stream),
                       "tgs_rasterize_depth_stats")
        return run

    variants = {"k6_render_only": k6, "depth_stats_no_stop_pos": stats(None), "depth_stats_with_stop_pos": stats(stop)}
    for f in variants.values():
        for _ in range(WARMUP):
            f()
    torch.cuda.synchronize()
    assert torch.equal(depth2, depth) and torch.equal(fT2, fT)          # the yardstick composites the same frame
    times = {k: [] for k in variants}
    for _ in range(REPEATS):                                            # interleaved: K6, K6s, K6s, K6, ...
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    budget.check()
    med_us = {k: statistics.median(v) for k, v in times.items()}
    I = int(ts[T])
    res = dict(label=spec["label"], gaussians=spec["N"], width=spec["W"], height=spec["H"], intersections=I,
               longest_list=int(n.max()), tiles=T,
               raster_opts={f: int(getattr(opts, f)) for f, _ in opts._fields_},
               us_median={k: round(v, 2) for k, v in med_us.items()},
               us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               ratio_to_k6={k: round(med_us[k] / med_us["k6_render_only"], 4) for k in med_us if k != "k6_render_only"},
               with_a_median=round(float((gid >= 0).float().mean()), 4),
               mean_depth_std=round(float(var.sqrt().mean()), 5))
    res["within_10_percent_of_k6"] = all(r <= 1.10 for r in res["ratio_to_k6"].values())
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "depth_stats_time.json"))
    ap.add_argument("--frames", nargs="+", default=list(FRAMES), choices=list(FRAMES))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/depth_stats_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/depth_stats_time.py", device=torch.cuda.get_device_name(0),
               method=f"device events around {LAUNCHES} back-to-back launches, {REPEATS} repeats interleaved over the variants "
                      f"after {WARMUP} warm-up launches each; median of the repeats; microseconds per launch",
               yardstick="k6_render_only: tgs_rasterize_fwd with stop_pos == NULL on the same lists in the same process",
               frames={})
    for name in a.frames:
        out["frames"][name] = time_frame(name, FRAMES[name], dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
