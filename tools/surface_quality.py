"""Developer tool: how good is the exported SURFACE (touch_gs_amd.export tsdf) -- the first metric here that
compares reconstructed geometry, not a rendered image, with the analytic capture's exact geometry?

The reduced analytic capture of analytic_scene.quick_quality (24 views at 640 x 360, 4000 iterations per run), the few-view
flag set with and without the touch / depth supervision (the arms "bunny_real:1" and "bunny_real:0").  For each run the
surface is exported over the padded box of the touch cloud at --resolution voxels along its longest side from ALL views of
the capture (the model renders held-out views as well as trained ones), with

    median   + inverse_variance      (the export's defaults)
    expected + inverse_variance
    median   + uniform

and compared with the points back-projected from gt_depth/ of all views inside the object mask (export.gt_surface_points):
Chamfer distance, precision, recall and F-score at tau = 2 voxels.  It reports what comes out.

    python tools/surface_quality.py [--out profiles/surface_quality.json] [--root DIR] [--resolution 128] [--iters 4000]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

VARIANTS = (("median", "inverse_variance"), ("expected", "inverse_variance"), ("median", "uniform"))
RUNS = ("bunny_real:1", "bunny_real:0")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "surface_quality.json"))
    ap.add_argument("--root", default=None, help="where the capture and the runs go (default: a temporary directory)")
    ap.add_argument("--resolution", type=int, default=128)
    ap.add_argument("--iters", type=int, default=4000)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=640)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/surface_quality.py needs the GPU: it trains and renders")
    from touch_gs_amd.analytic_scene import quick_quality
    from touch_gs_amd.export import export_tsdf, load_run
    root = a.root or tempfile.mkdtemp(prefix="surface_quality_")
    t0 = time.perf_counter()
    q = quick_quality(root, n_views=a.views, W=a.width, iters=a.iters, runs=RUNS)
    out = dict(tool="tools/surface_quality.py", device=torch.cuda.get_device_name(0),
               capture=dict(views=a.views, width=a.width, height=a.width * 9 // 16, iters=a.iters, capture_s=q["capture_s"],
                            prepare_s=q["prepare_s"]),
               method="surface exported from all views over the padded touch box; metrics against the object's analytic surface "
                      "(gt_depth/ back-projected inside gt_object_mask/ for all views); tau = 2 voxels; metres",
               resolution=a.resolution, runs={})
    for spec in RUNS:
        res = q["runs"][spec]
        loaded = load_run(res["run_dir"], "cuda")
        entry = dict(with_depth=res["with_depth"], psnr=res.get("psnr"), exact_object_depth_median_abs_m=res.get("exact_object_depth_median_abs_m"),
                     surfaces={})
        for depth, weight in VARIANTS:
            info = export_tsdf(res["run_dir"], os.path.join(res["run_dir"], f"export_{depth}_{weight}"), resolution=a.resolution,
                               depth=depth, weight=weight, views="all", loaded=loaded)
            entry["surfaces"][f"{depth}+{weight}"] = dict(info["surface_metrics"], grid=info["grid"]["dims"],
                                                          voxel_size_m=info["grid"]["voxel_size_m"], counts=info["counts"],
                                                          seconds=info["seconds"])
            print(spec, depth, weight, json.dumps(entry["surfaces"][f"{depth}+{weight}"]), flush=True)
        out["runs"][spec] = entry
    out["total_s"] = round(time.perf_counter() - t0, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
