"""Developer tool: does per-view exposure compensation undo per-image gain and offset?

The known-geometry capture of tools/pose_refine_quality.py (touch_gs_amd.analytic_scene: raw capture -> touch_gs_amd.prepare)
at the reference's bunny_real split (8 training views of 100, --preset few-view).  Every TRAINING image is multiplied, in
memory after loading (the view_hook of touch_gs_amd.train.main; the capture on disk is untouched, the held-out images keep
their true colours), by its own seeded gain in [0.7, 1.3] per channel and shifted by a small offset per channel, then
clamped to [0, 1] as a stored image would be.  Three arms:

    clean                  true images, compensation off
    perturbed              perturbed images, compensation off
    perturbed_compensated  perturbed images, --exposure-lr

Reported per arm: held-out psnr and depth_mse (run_eval under IS_REAL_WORLD; held-out views have no exposure row and are
rendered uncompensated), the exact depth errors, and -- for the compensated arm -- the recovered E (exposures.json) against
the applied one UP TO THE COMMON GAUGE: the scene's colours can absorb one affine transform common to all views, so only the
ratios between views are determined.  Per channel c the ratio r_i = A_i[c][c] / gain_i[c] is constant over the views i when
the recovery is exact; reported is the standard deviation over the views of log r_i beside that of log gain_i (what an
uncompensated run leaves), the same for the offsets after the gauge's best common shift, and the largest off-diagonal |A|.

One seed.  The rate is INRIA's 0.01 and is not tuned.  Report only: no threshold is set; whichever way the comparison
comes out, the numbers are written as measured.

    python tools/exposure_quality.py [--root DIR] [--iters 30000] [--exposure-lr 0.01] [--out profiles/exposure_quality.json]
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from touch_gs_amd import analytic_scene as A
from touch_gs_amd.exposure import EXPOSURES_FILE

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--gain-lo", type=float, default=0.7)
ap.add_argument("--gain-hi", type=float, default=1.3)
ap.add_argument("--offset", type=float, default=0.03, help="offsets are uniform in [-offset, offset] per channel")
ap.add_argument("--exposure-lr", type=float, default=0.01)
ap.add_argument("--out", default=os.path.join("profiles", "exposure_quality.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/exposure_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="expq_")
W, H = args.width, args.width * 9 // 16
FLAGS = "bunny_real"
out = dict(tool="tools/exposure_quality.py", device=torch.cuda.get_device_name(0), split=FLAGS, iters=args.iters, views=args.views,
           width=args.width, seeds=1, tuned=False,
           perturbation=dict(gain=[args.gain_lo, args.gain_hi], offset=args.offset, seed=0,
                             where="training images, in memory, per view and channel, clamped to [0, 1]"),
           compensation=dict(exposure_lr=args.exposure_lr, exposure_l2=0.0, exposure_start_step=0))
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=W, H=H, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS[FLAGS]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)


def applied(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(args.gain_lo, args.gain_hi, (n, 3)), rng.uniform(-args.offset, args.offset, (n, 3))


def perturb_hook(train_views, scale):
    gain, off = applied(len(train_views))
    for v, g, o in zip(train_views, gain, off):
        g, o = (torch.tensor(x, dtype=torch.float32, device=v.rgb.device) for x in (g, o))
        v.rgb = (v.rgb * g + o).clamp(0.0, 1.0).contiguous()
        v.__dict__.pop("_downscaled", None)


def recovered(run_dir):
    """The run's exposures against the applied gains and offsets, up to the common gauge (module docstring)."""
    path = os.path.join(run_dir, EXPOSURES_FILE)
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        rows = list(json.load(f).values())
    E = np.array([r["E"] for r in rows], np.float64)          # [n,3,4], in the order of the training views
    gain, off = applied(len(E))
    diag = np.stack([E[:, c, c] for c in range(3)], axis=1)
    logr = np.log(np.abs(diag) / gain)
    # offsets: b_i = o_i - gain_i r k for a common shift k of the gauge; per channel the best k by least squares
    resid = []
    for c in range(3):
        x, y = gain[:, c] * np.exp(logr[:, c].mean()), E[:, c, 3] - off[:, c]
        k = float(x @ y / (x @ x))
        resid.append(y - k * x)
    offd = E[:, :, :3].copy()
    for c in range(3):
        offd[:, c, c] = 0
    return dict(E=E.round(5).tolist(), applied_gain=gain.round(5).tolist(), applied_offset=off.round(5).tolist(),
                steps=[r["steps"] for r in rows],
                log_gain_ratio_std_per_channel=logr.std(0).round(5).tolist(),
                applied_log_gain_std_per_channel=np.log(gain).std(0).round(5).tolist(),
                offset_residual_rms_per_channel=[round(float(np.sqrt((r ** 2).mean())), 5) for r in resid],
                applied_offset_rms_per_channel=np.sqrt((off ** 2).mean(0)).round(5).tolist(),
                max_abs_off_diagonal=round(float(np.abs(offd).max()), 5))


def write():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


comp = ["--exposure-lr", str(args.exposure_lr)]
ARMS = {"clean": (False, []), "perturbed": (True, []), "perturbed_compensated": (True, comp)}   # arm -> (perturbed, trainer flags)
KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "exact_depth_mse", "exact_object_depth_mse", "exact_depth_median_abs_m",
        "exact_object_depth_median_abs_m")
out["runs"] = {}
for name, (pert, extra) in ARMS.items():
    r = A.train_and_eval(root, FLAGS, True, iters=args.iters, num_gaussians=args.num_gaussians, extra_args=extra,
                         preset="few-view", view_hook=perturb_hook if pert else None)
    res = dict(perturbed=pert, trainer_flags=extra, **{k: r[k] for k in KEYS if k in r}, train_wall_s=r["train_wall_s"],
               iters_per_s_wall=r["iters_per_s_wall"], split=r["split"])
    rec = recovered(r["run_dir"])
    if rec:
        res["exposure"] = rec
    out["runs"][name] = res
    print(name, json.dumps(res), flush=True)
    write()
print("wrote", args.out)
