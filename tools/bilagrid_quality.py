"""Developer tool: do per-view bilateral grids undo a per-image colour change that no single matrix removes?

The protocol of tools/exposure_quality.py: the known-geometry capture (touch_gs_amd.analytic_scene) at the reference's
bunny_real split (8 training views of 100, --preset few-view).  Every TRAINING image is changed in memory after loading
(the view_hook of touch_gs_amd.train.main; the capture on disk is untouched, the held-out images keep their true colours)
by its own seeded

    radial vignette   1 - s r^2, r = distance from the image centre / half diagonal, s in [0.1, 0.3]
    gamma             per channel, in [0.8, 1.25]
    gain and offset   those of tools/exposure_quality.py: gain in [0.7, 1.3] per channel, offset in [-0.03, 0.03]

in this order, then clamped to [0, 1] as a stored image would be.  Four arms:

    clean                true images, both features off
    perturbed            perturbed images, both features off
    perturbed_exposure   perturbed images, --exposure-lr 0.01
    perturbed_bilagrid   perturbed images, --bilagrid-lr 2e-3 (16 x 16 x 8, TV weight 10)

Reported per arm: held-out psnr, ssim, cc_psnr / cc_ssim (run_eval --color-correct: the render fitted to its ground truth by
a least-squares 3x4 affine before the metric; held-out views have no row and are rendered uncorrected), depth_mse, the
exact depth errors, iterations per second of wall time, and for the grid arm the mean |g - identity| and TV of the grids.

One seed.  The rates are gsplat's / INRIA's and are not tuned.  Report only: no threshold is set; whichever way the
comparison comes out, the numbers are written as measured.

    python tools/bilagrid_quality.py [--root DIR] [--iters 30000] [--out profiles/bilagrid_quality.json]
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from touch_gs_amd import analytic_scene as A
from touch_gs_amd.bilagrid import BILAGRIDS_FILE, load_bilagrids

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--exposure-lr", type=float, default=0.01)
ap.add_argument("--bilagrid-lr", type=float, default=2e-3)
ap.add_argument("--out", default=os.path.join("profiles", "bilagrid_quality.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/bilagrid_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="bgq_")
W, H = args.width, args.width * 9 // 16
FLAGS = "bunny_real"
PERT = dict(vignette=[0.1, 0.3], gamma=[0.8, 1.25], gain=[0.7, 1.3], offset=0.03, seed=0)
out = dict(tool="tools/bilagrid_quality.py", device=torch.cuda.get_device_name(0), split=FLAGS, iters=args.iters, views=args.views,
           width=args.width, seeds=1, tuned=False,
           perturbation=dict(PERT, where="training images, in memory, per view: vignette, gamma per channel, gain and offset per "
                                         "channel, clamped to [0, 1]"),
           arms=dict(exposure_lr=args.exposure_lr, bilagrid_lr=args.bilagrid_lr, bilagrid_shape=[16, 16, 8], bilagrid_tv=10.0),
           not_measured="more than one seed; tuned rates or TV weights; grids on unperturbed images; real captures; the grid's "
                        "recovery of the applied vignette and tone curve per view")
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=W, H=H, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS[FLAGS]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)


def perturb_hook(train_views, scale):
    rng = np.random.default_rng(PERT["seed"])
    n = len(train_views)
    gain, off = rng.uniform(*PERT["gain"], (n, 3)), rng.uniform(-PERT["offset"], PERT["offset"], (n, 3))   # exposure_quality's draws
    vig, gam = rng.uniform(*PERT["vignette"], n), rng.uniform(*PERT["gamma"], (n, 3))
    for v, g, o, s, ga in zip(train_views, gain, off, vig, gam):
        dev = v.rgb.device
        h, w = v.rgb.shape[:2]
        y, x = torch.meshgrid(torch.linspace(-1, 1, h, device=dev) * h, torch.linspace(-1, 1, w, device=dev) * w, indexing="ij")
        r2 = (x * x + y * y) / float(w * w + h * h)
        g, o, ga = (torch.tensor(t, dtype=torch.float32, device=dev) for t in (g, o, ga))
        img = v.rgb * (1.0 - float(s) * r2)[..., None]
        img = img.clamp(min=0.0) ** ga
        v.rgb = (img * g + o).clamp(0.0, 1.0).contiguous()
        v.__dict__.pop("_downscaled", None)


def grids_of(run_dir):
    path = os.path.join(run_dir, BILAGRIDS_FILE)
    if not os.path.exists(path):
        return {}
    g = np.stack(list(load_bilagrids(path).values())).astype(np.float64)      # [n, GH, GW, L, 12]
    ident = np.zeros(12)
    ident[[0, 5, 10]] = 1
    tv = sum(float((np.diff(g, axis=a) ** 2).mean()) for a in (1, 2, 3))
    return dict(mean_abs_delta=round(float(np.abs(g - ident).mean()), 5), max_abs_delta=round(float(np.abs(g - ident).max()), 5),
                tv_mean_over_views=round(tv, 6))


def write():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


ARMS = {"clean": (False, []), "perturbed": (True, []), "perturbed_exposure": (True, ["--exposure-lr", str(args.exposure_lr)]),
        "perturbed_bilagrid": (True, ["--bilagrid-lr", str(args.bilagrid_lr)])}      # arm -> (perturbed, trainer flags)
KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "exact_depth_mse", "exact_object_depth_mse", "exact_depth_median_abs_m",
        "exact_object_depth_median_abs_m")
out["runs"] = {}
for name, (pert, extra) in ARMS.items():
    r = A.train_and_eval(root, FLAGS, True, iters=args.iters, num_gaussians=args.num_gaussians, extra_args=extra,
                         preset="few-view", view_hook=perturb_hook if pert else None)
    from touch_gs_amd.run_eval import eval_run
    os.environ["IS_REAL_WORLD"] = "True"
    cc = eval_run(r["run_dir"], os.path.join(r["run_dir"], "run_eval_cc.json"), color_correct=True)
    res = dict(perturbed=pert, trainer_flags=extra, **{k: r[k] for k in KEYS if k in r}, cc_psnr=cc["cc_psnr"], cc_ssim=cc["cc_ssim"],
               train_wall_s=r["train_wall_s"], iters_per_s_wall=r["iters_per_s_wall"], split=r["split"])
    g = grids_of(r["run_dir"])
    if g:
        res["bilagrid"] = g
    out["runs"][name] = res
    print(name, json.dumps(res), flush=True)
    write()
print("wrote", args.out)
