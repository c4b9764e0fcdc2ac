"""Developer tool: does raw monocular depth through the scale-invariant term help a capture without a depth camera?

A sibling of tools/train_quality.py on the same known-geometry capture (touch_gs_amd.analytic_scene: raw capture ->
touch_gs_amd.prepare), in the few-view regime -- the reference's bunny_real flag set, 8 training views of 100,
--preset few-view, 30 000 iterations -- with three kinds of depth supervision:

    touch_only         transforms.json registers touch_depth/ + touch_var/: the touched patches alone
    touch_plus_mono    the same + the RAW zoe_depth/ maps through --mono-depth-dir / --mono-depth-mult: no RealSense,
                       no alignment step
    touch_plus_mono_local   the same + the patch-wise term (--mono-depth-local-mult, global 0.1 and local 0.1)
    aligned_fused      today's pipeline: ZoeDepth aligned to 1 % of the RealSense depth and fused with the touch maps
                       (fused_output_dir/ + fused_output_dir_uncertainty/)

Every run is evaluated by run_eval under IS_REAL_WORLD on the held-out views (psnr, depth_mse against the run's own
supervision maps, gt_depth_mse against the sensor) and against the analytic depth (exact_depth_mse: the one number whose
reference is the same for all runs).  Whichever way the comparison comes out, the numbers are written as measured.

    python tools/mono_depth_quality.py [--root DIR] [--iters 30000] [--mono-depth-mult 0.1] [--mono-depth-local-mult 0.1]
                                       [--out profiles/mono_depth_quality.json]

profiles/mono_depth_quality.json is the record of the three runs before the patch-wise term existed;
profiles/mono_depth_local_quality.json holds the four.
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from touch_gs_amd import analytic_scene as A
from touch_gs_amd import prepare as PR

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--mono-depth-mult", type=float, default=0.1)
ap.add_argument("--mono-depth-local-mult", type=float, default=0.1)
ap.add_argument("--out", default=os.path.join("profiles", "mono_depth_quality.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/mono_depth_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="mdq_")
out = dict(tool="tools/mono_depth_quality.py", device=torch.cuda.get_device_name(0), flags="bunny_real", preset="few-view",
           iters=args.iters, mono_depth_mult=args.mono_depth_mult, mono_depth_local_mult=args.mono_depth_local_mult, views=args.views, width=args.width)
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=args.width, H=args.width * 9 // 16, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS["bunny_real"]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)

mono = ["--mono-depth-dir", "zoe_depth", "--mono-depth-mult", str(args.mono_depth_mult)]
RUNS = {   # name -> (depth dir, uncertainty dir registered in transforms.json, extra trainer flags)
    "touch_only": ("touch_depth", "touch_var", []),
    "touch_plus_mono": ("touch_depth", "touch_var", mono),
    "touch_plus_mono_local": ("touch_depth", "touch_var", mono + ["--mono-depth-local-mult", str(args.mono_depth_local_mult)]),
    "aligned_fused": ("fused_output_dir", "fused_output_dir_uncertainty", []),
}
KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "gt_object_depth_mse", "exact_depth_mse", "exact_object_depth_mse",
        "depth_mse_m2", "gt_depth_mse_m2", "exact_depth_mse_m2", "exact_depth_median_abs_m", "exact_object_depth_median_abs_m")
out["runs"] = {}
try:
    for name, (ddir, udir, extra) in RUNS.items():
        PR.add_depth_file_path_to_transforms(root, "transforms.json", ddir, udir)
        r = A.train_and_eval(root, "bunny_real", True, iters=args.iters, num_gaussians=args.num_gaussians, extra_args=extra)
        out["runs"][name] = dict(depth_supervision=ddir, uncertainty=udir, trainer_flags=extra,
                                 **{k: r[k] for k in KEYS if k in r}, train_wall_s=r["train_wall_s"],
                                 iters_per_s_wall=r["iters_per_s_wall"], split=r["split"])
        print(name, json.dumps(out["runs"][name]), flush=True)
finally:   # leave the capture as prepare left it
    PR.add_depth_file_path_to_transforms(root, "transforms.json", "fused_output_dir", "fused_output_dir_uncertainty")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
