"""Developer tool: what does the MCMC strategy (touch_gs_amd/mcmc.py) buy against clone / split / cull?

The known-geometry capture of tools/pose_refine_quality.py (touch_gs_amd.analytic_scene: raw capture -> touch_gs_amd.prepare)
at the reference's bunny_real split (8 training views of 100), --preset few-view, both arms from the same seeds:

    default   --strategy default: Splatfacto's refinement; the number of Gaussians is whatever it ends at
    mcmc      --strategy mcmc with --cap-max set to the default arm's final count, every other MCMC flag at its default

Reported per arm: held-out psnr, ssim and depth_mse (run_eval under IS_REAL_WORLD), the exact depth errors, the final number of
Gaussians (from the run's last checkpoint) and iterations per second of wall time.

One seed, nothing tuned.  Report only: no threshold is set; whichever way the comparison comes out, the numbers are written
as measured.

    python tools/mcmc_quality.py [--root DIR] [--iters 30000] [--out profiles/mcmc_quality.json]
"""
import argparse, glob, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from touch_gs_amd import analytic_scene as A

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--out", default=os.path.join("profiles", "mcmc_quality.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/mcmc_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="mcmcq_")
W, H = args.width, args.width * 9 // 16
FLAGS = "bunny_real"
out = dict(tool="tools/mcmc_quality.py", device=torch.cuda.get_device_name(0), split=FLAGS, preset="few-view", iters=args.iters,
           views=args.views, width=args.width, num_gaussians=args.num_gaussians, seeds=1, tuned=False)
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=W, H=H, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS[FLAGS]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)


def final_count(run_dir):
    ckpt = sorted(glob.glob(os.path.join(run_dir, "step-*.ckpt")))[-1]
    return int(torch.load(ckpt, map_location="cpu", weights_only=False)["N"])


def write():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "exact_depth_mse", "exact_object_depth_mse", "exact_depth_median_abs_m",
        "exact_object_depth_median_abs_m", "depth_mse_m2")
out["runs"] = {}
cap = None
for name in ("default", "mcmc"):
    extra = [] if name == "default" else ["--strategy", "mcmc", "--cap-max", str(cap)]
    # (a default arm that ends BELOW its initial count: the MCMC arm starts at the cap, it never removes a Gaussian)
    start = args.num_gaussians if cap is None else min(args.num_gaussians, cap)
    r = A.train_and_eval(root, FLAGS, True, iters=args.iters, num_gaussians=start, extra_args=extra, preset="few-view")
    n = final_count(r["run_dir"])
    if cap is None:
        cap = n
    res = dict(trainer_flags=extra, gaussians_initial=start, **{k: r[k] for k in KEYS if k in r}, gaussians_final=n, train_wall_s=r["train_wall_s"],
               iters_per_s_wall=r["iters_per_s_wall"], split=r["split"])
    out["runs"][name] = res
    print(name, json.dumps(res), flush=True)
    write()
d, m = out["runs"]["default"], out["runs"]["mcmc"]
out["mcmc_minus_default"] = {k: round(m[k] - d[k], 6) for k in ("psnr", "depth_mse") if k in d and k in m}
write()
print("wrote", args.out)
