"""Developer tool: does camera pose refinement undo pose noise?

The known-geometry capture of tools/normal_prior_quality.py (touch_gs_amd.analytic_scene: raw capture -> touch_gs_amd.prepare),
at the reference's two splits: bunny_real (8 training views of 100, --preset few-view) and block (0.8).  Seeded pose noise is
added to the TRAINING cameras in memory after loading (the view_hook of touch_gs_amd.train.main; the capture on
disk and the analytic_scene defaults are untouched; the held-out cameras keep their true poses).  Three arms per split:

    clean             true poses, refinement off
    noisy             noisy poses, refinement off
    noisy_refined     noisy poses, --pose-lr-rot / --pose-lr-trans

Reported per arm: held-out psnr and depth_mse (run_eval under IS_REAL_WORLD), the exact depth errors, and the residual
RELATIVE pose error between the training cameras: the run's training poses (refined_poses.json, else the poses it trained
with) are aligned to the true ones by a similarity transform of the camera centres (Umeyama) and what remains is reported
as mean rotation angle (degrees) and mean centre distance (metres).  Report only: no threshold is set; whichever way the
comparison comes out, the numbers are written as measured.

    python tools/pose_refine_quality.py [--root DIR] [--iters 30000] [--noise-deg 0.5] [--noise-m 0.005] [--out profiles/pose_refine_quality.json]
"""
import argparse, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from touch_gs_amd import analytic_scene as A
from touch_gs_amd import pose as PO

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--root", default=None)
ap.add_argument("--views", type=int, default=100)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--iters", type=int, default=30000)
ap.add_argument("--num-gaussians", type=int, default=100000)
ap.add_argument("--noise-deg", type=float, default=0.5)
ap.add_argument("--noise-m", type=float, default=0.005)
ap.add_argument("--pose-lr-rot", type=float, default=2e-4)
ap.add_argument("--pose-lr-trans", type=float, default=1e-4)
ap.add_argument("--pose-start-step", type=int, default=500)
ap.add_argument("--splits", default="bunny_real,block", help="flag sets to run, comma separated (block densifies to millions of Gaussians: minutes per arm)")
ap.add_argument("--out", default=os.path.join("profiles", "pose_refine_quality.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tools/pose_refine_quality.py trains: it needs the GPU")
root = args.root or tempfile.mkdtemp(prefix="prq_")
W, H = args.width, args.width * 9 // 16
out = dict(tool="tools/pose_refine_quality.py", device=torch.cuda.get_device_name(0), splits=args.splits, iters=args.iters, views=args.views, width=args.width,
           noise=dict(deg=args.noise_deg, m=args.noise_m, seed=0, where="training cameras, in memory, camera frame"),
           refinement=dict(pose_lr_rot=args.pose_lr_rot, pose_lr_trans=args.pose_lr_trans, pose_start_step=args.pose_start_step))
if not os.path.exists(os.path.join(root, "transforms.json")):
    t = time.perf_counter()
    out["capture"] = A.write_raw_capture(root, n_views=args.views, W=W, H=H, device="cuda")
    out["capture_s"] = round(time.perf_counter() - t, 1)
if not os.path.exists(os.path.join(root, "fused_output_dir")):
    t = time.perf_counter()
    out["prepare"] = A.prepare_capture(root, A.FLAG_SETS["bunny_real"]["split"])
    out["prepare_s"] = round(time.perf_counter() - t, 1)


def perturb_views(views, rot_deg, dist, seed=0):
    """Every view's camera turned by rot_deg about a seeded random axis and moved by dist (scene units) in a seeded random
    direction, in the camera frame (the parametrisation of touch_gs_amd.pose)."""
    import dataclasses
    rng = np.random.default_rng(seed)
    for v in views:
        a, d = rng.normal(size=3), rng.normal(size=3)
        V = np.array(v.cam.viewmat, np.float64)
        V[:3, :3], V[:3, 3] = PO.retract(V[:3, :3], V[:3, 3], np.radians(rot_deg) * a / np.linalg.norm(a), dist * d / np.linalg.norm(d))
        v.set_camera(dataclasses.replace(v.cam, viewmat=V))


def noise_hook(train_views, scale):
    perturb_views(train_views, args.noise_deg, args.noise_m * scale, 0)


def umeyama(X, Y):
    """Similarity (s, Q, t) minimising |s Q X + t - Y| over point sets [n,3]."""
    mx, my = X.mean(0), Y.mean(0)
    Xc, Yc = X - mx, Y - my
    U, D, Vt = np.linalg.svd(Yc.T @ Xc / len(X))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    Q = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / (Xc ** 2).sum() * len(X)
    return s, Q, my - s * Q @ mx


def residual_pose_error(run_dir, split, noise):
    """Training poses of the run against the true ones after a similarity alignment of the camera centres."""
    from touch_gs_amd.dataset import Scene
    scene = Scene(root, split, "cuda")
    idx = list(scene.i_train)
    true = [np.array(scene.views[i].cam.viewmat, np.float64) for i in idx]
    path = os.path.join(run_dir, PO.POSES_FILE)
    if os.path.exists(path):
        with open(path) as f:
            P = json.load(f)
        used = [np.array(P[scene.names[i]]["V"]) for i in idx]
    else:
        views = [scene.views[i] for i in idx]
        if noise:
            perturb_views(views, args.noise_deg, args.noise_m * scene.scale, 0)
        used = [np.array(v.cam.viewmat, np.float64) for v in views]
    C = lambda V: -V[:3, :3].T @ V[:3, 3]
    X, Y = np.stack([C(V) for V in used]), np.stack([C(V) for V in true])
    s, Q, t = umeyama(X, Y)
    ang, dist = [], []
    for Vu, Vt_ in zip(used, true):
        Rw = Q @ Vu[:3, :3].T            # aligned camera->world rotation
        ang.append(np.degrees(np.linalg.norm(PO.rot_log(Rw.T @ Vt_[:3, :3].T))))
        dist.append(np.linalg.norm(s * Q @ C(Vu) + t - C(Vt_)) / scene.scale)
    return dict(residual_rot_deg_mean=float(np.mean(ang)), residual_rot_deg_max=float(np.max(ang)),
                residual_centre_m_mean=float(np.mean(dist)), residual_centre_m_max=float(np.max(dist)), alignment_scale=float(s))


def write():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


refine = ["--pose-lr-rot", str(args.pose_lr_rot), "--pose-lr-trans", str(args.pose_lr_trans), "--pose-start-step", str(args.pose_start_step)]
ARMS = {"clean": (False, []), "noisy": (True, []), "noisy_refined": (True, refine)}     # arm -> (pose noise, trainer flags)
KEYS = ("psnr", "ssim", "depth_mse", "gt_depth_mse", "exact_depth_mse", "exact_object_depth_mse", "exact_depth_median_abs_m",
        "exact_object_depth_median_abs_m")
out["runs"] = {}
for flags in args.splits.split(","):
    out["runs"][flags] = {}
    for name, (noisy, extra) in ARMS.items():
        r = A.train_and_eval(root, flags, True, iters=args.iters, num_gaussians=args.num_gaussians, extra_args=extra,
                             preset="few-view" if flags == "bunny_real" else "reference", view_hook=noise_hook if noisy else None)
        res = dict(pose_noise=noisy, trainer_flags=extra, **{k: r[k] for k in KEYS if k in r}, train_wall_s=r["train_wall_s"],
                   iters_per_s_wall=r["iters_per_s_wall"], split=r["split"], **residual_pose_error(r["run_dir"], r["split"], noisy))
        out["runs"][flags][name] = res
        print(flags, name, json.dumps(res), flush=True)
        write()      # after every arm: the block split trains millions of Gaussians for minutes per arm
print("wrote", args.out)
