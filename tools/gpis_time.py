"""Developer tool: what does one GPIS view cost, and what does tgs_gpis_render make of it?

One 1280 x 720 view (the first orbit camera) of the 50-touch analytic capture -- the fit of write_raw_capture: length scale
0.02, offset 0.005, noise 1e-5, max_points 1300 --, rendered at stride 1 and at stride 2 with the capture's arguments
(max_var 0.01, var_floor 1e-3, margin 24), in one process on one box:

    torch_gpu   today's path with gp.device on the GPU (fp64 torch, [rays x n] matrices per step): host clock around
                render_depth, which ends in device-to-host copies (a synchronise)
    numpy_cpu   today's path on the CPU (stride 2 only, once; --skip-cpu leaves it out)
    hip         render_depth(backend="hip"): the same host clock, and device events around the launches alone -- the whole
                call (fill + march + variance) and the call without Kinv (fill + march); variance = the difference

After a warm-up of every path, REPEATS repeats interleaved over the GPU paths, medians, all repeats kept.  The expectation
(not a test): at stride 1 the kernel is at least 2 x faster than torch_gpu, whole call against whole call.

    python tools/gpis_time.py [--out profiles/gpis_time.json] [--skip-cpu]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

REPEATS = 5
EXPECTED = 2.0


def build_gp(seed=0):
    from touch_gs_amd.analytic_scene import AnalyticScene, TRAIN_INTRINSICS, orbit_cameras, touch_readings
    from touch_gs_amd.gpis import GPIS, estimate_outward_normals
    rng = np.random.default_rng(seed)
    sc = AnalyticScene("cpu")
    cams = orbit_cameras(100, seed=seed)
    pts, sens = touch_readings(sc, 50, seed=seed)
    gp = GPIS(length_scale=0.02, offset=0.005, noise_var=1e-5).fit(pts, estimate_outward_normals(pts, sens), max_points=1300, rng=rng)
    return gp, cams[0], TRAIN_INTRINSICS


def view_args(gp, c2w, intr, W, H, near, far, margin):
    """The per-view host part of render_depth (region, march interval, step count)."""
    fx, fy, cx, cy = intr
    R = np.asarray(c2w, dtype=np.float64)[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    t = np.asarray(c2w, dtype=np.float64)[:3, 3]
    Pc = (gp.P - t) @ R
    front = Pc[:, 2] > near
    u = fx * Pc[front, 0] / Pc[front, 2] + cx
    v = fy * Pc[front, 1] / Pc[front, 2] + cy
    roi = (int(max(0, np.floor(u.min()) - margin)), int(max(0, np.floor(v.min()) - margin)),
           int(min(W - 1, np.ceil(u.max()) + margin)), int(min(H - 1, np.ceil(v.max()) + margin)))
    zs_lo = max(near, Pc[front, 2].min() - 3 * gp.l - gp.offset)
    zs_hi = min(far, Pc[front, 2].max() + 3 * gp.l + gp.offset)
    n_steps = int(np.clip(np.ceil((zs_hi - zs_lo) / (0.6 * gp.offset)), 16, 512))
    return R, t, roi, zs_lo, zs_hi, n_steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "gpis_time.json"))
    ap.add_argument("--skip-cpu", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpis_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    W, H = 1280, 720
    gp, c2w, intr = build_gp()
    kw = dict(near=0.05, far=1.5, max_var=0.01, var_floor=1e-3, roi_margin_px=24)
    out = dict(tool="tools/gpis_time.py", device=torch.cuda.get_device_name(0), width=W, height=H, gp_points=int(len(gp.X)),
               touched_points=int(len(gp.P)),
               method=f"host clock around render_depth (ends in a synchronise) and device events around the launches; one warm-up, "
                      f"{REPEATS} repeats interleaved over the GPU paths, medians, all repeats kept; milliseconds",
               expectation=f"stride 1: torch_gpu / hip (whole calls, host clock) >= {EXPECTED}", strides={})

    def host_ms(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for stride in (1, 2):
        R, t, roi, zs_lo, zs_hi, n_steps = view_args(gp, c2w, intr, W, H, kw["near"], kw["far"], kw["roi_margin_px"])
        rays = ((roi[2] - roi[0]) // stride + 1) * ((roi[3] - roi[1]) // stride + 1)

        def torch_gpu():
            gp.device = "cuda:0"
            try:
                return gp.render_depth(c2w, *intr, W, H, stride=stride, **kw)
            finally:
                gp.device = None

        def hip():
            return gp.render_depth(c2w, *intr, W, H, stride=stride, backend="hip", return_normals=True, **kw)

        def hip_events(want_var):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gp._render_hip(R, t, *intr, W, H, roi, stride, zs_lo, zs_hi, n_steps, kw["max_var"] if want_var else None,
                           kw["var_floor"], want_var=want_var, want_normals=True)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        ref = torch_gpu()                   # warm-ups; their results are compared below
        got = hip()
        hip_events(True); hip_events(False)
        times = {k: [] for k in ("torch_gpu_host", "hip_host", "hip_device_full", "hip_device_march")}
        for _ in range(REPEATS):
            times["torch_gpu_host"].append(host_ms(torch_gpu)[0])
            times["hip_host"].append(host_ms(hip)[0])
            times["hip_device_full"].append(hip_events(True))
            times["hip_device_march"].append(hip_events(False))
        med = {k: statistics.median(v) for k, v in times.items()}
        both = np.isfinite(ref[0]) & np.isfinite(got[0])
        res = dict(stride=stride, roi=list(roi), rays=int(rays), n_steps=int(n_steps), crossings=int(np.isfinite(got[0]).sum()),
                   exponentials_per_marched_ray=int(len(gp.X)) * (n_steps + 12),
                   ms_median={k: round(v, 3) for k, v in med.items()}, ms_all={k: [round(x, 3) for x in v] for k, v in times.items()},
                   ms_by_difference=dict(march=round(med["hip_device_march"], 3),
                                         variance=round(med["hip_device_full"] - med["hip_device_march"], 3)),
                   ratio_torch_gpu_to_hip=round(med["torch_gpu_host"] / med["hip_host"], 2),
                   expectation_met=bool(med["torch_gpu_host"] / med["hip_host"] >= EXPECTED),
                   against_torch_gpu=dict(status_differs=int((np.isfinite(ref[0]) != np.isfinite(got[0])).sum()),
                                          depth_max=float(np.abs(ref[0] - got[0])[both].max()) if both.any() else None,
                                          var_max=float(np.abs(ref[1] - got[1])[both].max()) if both.any() else None))
        if stride == 2 and not a.skip_cpu:
            t0 = time.perf_counter()
            gp.render_depth(c2w, *intr, W, H, stride=stride, **kw)
            res["ms_numpy_cpu_once"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(json.dumps(res), flush=True)
        out["strides"][str(stride)] = res
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
