"""Developer tool: do normal priors help the few-view regime between the touches?

A sibling of tools/mono_depth_quality.py on the same known-geometry capture (touch_gs_amd.analytic_scene: raw capture ->
touch_gs_amd.prepare), the reference's bunny_real flag set, 8 training views of 100, --preset few-view:

    touch_only            transforms.json registers touch_depth/ + touch_var/: the touched patches alone
    touch_plus_normals    the same + normal priors through --normal-dir / --normal-mult.  The priors are the EXACT surface
                          normals of the analytic scene (AnalyticScene.render(want_normal=True): the normal at each pixel
                          centre's hit, rotated into the camera's OpenCV axes), written as gt_normal/<stem>.npy (float16):
                          the best prior there can be -- an upper bound on what a GPIS-gradient or monocular normal map gives

    touch_plus_gpis_normals   (--gpis-normals only) the same with the priors a capture can actually have: the GPIS surface
                          normals of the touches themselves, rendered by GPIS.render_depth(backend="hip", return_normals=True)
                          into normals_gpis/<stem>.npy with conf = clip(1 - var / gpis_max_var, 0, 1).  They
                          exist on the touched patches only.  The result goes to profiles/gpis_normal_quality.json; the two
                          arms above compute what they compute without the flag.

All runs are evaluated by run_eval under IS_REAL_WORLD on the held-out views (psnr, gt_depth_mse against the sensor),
against the analytic depth (exact_depth_mse) and against the exact normals (normal_angle_deg: the conf-weighted mean angle
between the normals of the rendered depth and the prior over the supervised centres).  Report only: no threshold is set;
whichever way the comparison comes out, the numbers are written as measured.

    python tools/normal_prior_quality.py [--root DIR] [--iters 30000] [--normal-mult 0.05] [--out profiles/normal_prior_quality.json]
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from touch_gs_amd import analytic_scene as A
from touch_gs_amd import prepare as PR

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--normal-mult", type=float, default=0.05)
ap.add_argument("--gpis-normals", action="store_true", help="add the touch_plus_gpis_normals arm")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join("profiles", "gpis_normal_quality.json" if args.gpis_normals else "normal_prior_quality.json")
if not torch.cuda.is_available():
    raise SystemExit("tools/normal_prior_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="npq_")
out = dict(tool="tools/normal_prior_quality.py", device=torch.cuda.get_device_name(0), flags="bunny_real", preset="few-view",
           iters=args.iters, normal_mult=args.normal_mult, views=args.views, width=args.width,
           prior="exact analytic surface normals in each camera's OpenCV axes (float16 .npy)")
W, H = args.width, args.width * 9 // 16
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=W, H=H, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS["bunny_real"]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "gt_normal")):
    t = time.perf_counter()
    os.makedirs(os.path.join(root, "gt_normal"))
    with open(os.path.join(root, "transforms.json")) as f:
        meta = json.load(f)
    sc = A.AnalyticScene("cuda")
    intr = (meta["fl_x"], meta["fl_y"], meta["cx"], meta["cy"])
    for fr in meta["frames"]:
        n = sc.render(np.array(fr["transform_matrix"]), intr, W, H, want_rgb=False, want_normal=True)["normal"]
        np.save(os.path.join(root, "gt_normal", os.path.splitext(os.path.basename(fr["file_path"]))[0] + ".npy"), n.astype(np.float16))
    out["normals_s"] = round(time.perf_counter() - t, 1)

if args.gpis_normals and not os.path.exists(os.path.join(root, "normals_gpis")):
    out["gpis_normals"] = A.write_gpis_normals(root)

RUNS = {"touch_only": [], "touch_plus_normals": ["--normal-dir", "gt_normal", "--normal-mult", str(args.normal_mult)]}
if args.gpis_normals:
    RUNS["touch_plus_gpis_normals"] = ["--normal-dir", "normals_gpis", "--normal-mult", str(args.normal_mult)]
KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "gt_object_depth_mse", "exact_depth_mse", "exact_object_depth_mse",
        "gt_depth_mse_m2", "exact_depth_mse_m2", "exact_depth_median_abs_m", "exact_object_depth_median_abs_m")
out["runs"] = {}
try:
    PR.add_depth_file_path_to_transforms(root, "transforms.json", "touch_depth", "touch_var")
    for name, extra in RUNS.items():
        r = A.train_and_eval(root, "bunny_real", True, iters=args.iters, num_gaussians=args.num_gaussians, extra_args=extra)
        from touch_gs_amd.run_eval import eval_run
        os.environ["IS_REAL_WORLD"] = "True"
        try:   # the same checkpoint again with the normals rendered: the angle to the exact normals on the held-out views
            rn = eval_run(r["run_dir"], os.path.join(r["run_dir"], "run_eval_normals.json"), normals=True, normal_dir="gt_normal")
        finally:
            del os.environ["IS_REAL_WORLD"]
        out["runs"][name] = dict(depth_supervision="touch_depth", uncertainty="touch_var", trainer_flags=extra,
                                 **{k: r[k] for k in KEYS if k in r}, normal_angle_deg=rn.get("normal_angle_deg"),
                                 train_wall_s=r["train_wall_s"], iters_per_s_wall=r["iters_per_s_wall"], split=r["split"])
        print(name, json.dumps(out["runs"][name]), flush=True)
finally:   # leave the capture as prepare left it
    PR.add_depth_file_path_to_transforms(root, "transforms.json", "fused_output_dir", "fused_output_dir_uncertainty")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)
