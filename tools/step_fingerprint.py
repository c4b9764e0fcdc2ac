"""Developer tool: what the host layer of the train step enqueues, and the bits that come out, per single-process mode.

Run from the root of the tree under test (the package is imported from the current directory), with two trees and ONE
library (TGS_LIB_PATH) to compare the host code of two commits: every line must be identical.  Eight steps per mode on
the scene of the data-parallel worker of tests/test_gpu_api_surfaces.py (4001 Gaussians, 160x96, SH degree 3, four
views, seeds 7 / 99).  One line per mode:

    mode  step  optimizer.t  params.N  sha256(params.flat) sha256(exp_avg) sha256(exp_avg_sq)  C entry points of the last two steps
    [color_set=sha256(state of the exposure / bilateral-grid set)]

The entry points are recorded by wrapping the callables of the object ``_lib.load()`` returns (runs of one name as
``name*k``).  ``--dump DIR`` also saves the three buffers of every mode (to compare by largest difference if a mode is not
reproducible from run to run)."""
import argparse, hashlib, os, sys, torch
sys.path.insert(0, '.')
from touch_gs_amd import _lib
from touch_gs_amd.densify import DensifyConfig
from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
from touch_gs_amd.optim import GaussianParams
from touch_gs_amd.scene import make_view, synthetic_gaussians

ap = argparse.ArgumentParser()
ap.add_argument("--dump", default=None)
ap.add_argument("--modes", nargs="*", default=None)
args = ap.parse_args()
N, W, H, deg, STEPS = 4001, 160, 96, 3, 8
dev = torch.device('cuda:0')
P, _ = synthetic_gaussians(N, W, H, deg, 99)

calls = []
lib = _lib.load()
for name in _lib.SIGNATURES:
    if name != "tgs_last_error":
        setattr(lib, name, (lambda fn, name: lambda *a: (calls.append(name), fn(*a))[1])(getattr(lib, name), name))


def densify(m):
    m.enable_densification(DensifyConfig(warmup_length=2, refine_every=4, densify_grad_thresh=1e-5, densify_size_thresh=0.02,
                                         cull_alpha_thresh=0.01, reset_alpha_every=0))


def priors(views):      # seeded random monocular depth (positive) and normal priors
    g = torch.Generator().manual_seed(5)
    for v in views:
        v.mono_depth = (0.5 + torch.rand(H, W, generator=g)).to(dev)
        v.normal_prior = torch.randn(H, W, 3, generator=g).to(dev)


# mode -> (config, set-up of the model given its views, announce the next view, set-up of the views)
MODES = {
    "fused_next": (dict(), None, True, None),
    "fused": (dict(), None, False, None),
    "separate_adam": (dict(), lambda m, v: setattr(m, "fuse_adam", False), False, None),
    "densify_resort": (dict(spatial_sort=True, resort_every_refines=1), lambda m, v: densify(m), True, None),
    "speculative_overflow": (dict(), lambda m, v: m.enable_speculative_budget(capacity=3000, max_in_flight=2), True, None),
    "coarse_to_fine": (dict(num_downscales=1, resolution_schedule=4), None, True, None),
    "step_graphs": (dict(), lambda m, v: m.capture_step_graphs(v), False, None),
    "pose_exposure": (dict(pose_lr_rot=1e-3, pose_lr_trans=1e-3, exposure_lr=1e-2),
                      lambda m, v: (m.enable_pose_refinement(v), m.enable_exposure(v)), True, None),
    "mono_local_normal": (dict(mono_depth_local_mult=0.1, normal_prior_mult=0.1), None, True, priors),
    "bilagrid": (dict(bilagrid_lr=2e-3, bilagrid_shape=(5, 3, 4)), lambda m, v: m.enable_bilagrid(v), True, None),
    "exposure_c2f": (dict(exposure_lr=1e-2, num_downscales=1, resolution_schedule=4), lambda m, v: m.enable_exposure(v),
                     False, None),
}
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
for mode in args.modes or MODES:
    cfg, setup, announce, view_setup = MODES[mode]
    views = [make_view(N, W, H, deg, 7, dev, view=v, n_views=4) for v in range(4)]   # fresh: pose refinement moves the cameras
    if view_setup is not None:
        view_setup(views)
    params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
    m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, **cfg), params)
    if setup is not None:
        setup(m, views)
    for i in range(STEPS):
        if i == STEPS - 2:
            del calls[:]
        m.train_step(views[i % 4], next_view=views[(i + 1) % 4] if announce else None)
    last_two = list(calls)
    m.flush()
    torch.cuda.synchronize()
    runs = []
    for name in last_two:
        if runs and runs[-1][0] == name:
            runs[-1][1] += 1
        else:
            runs.append([name, 1])
    bufs = (m.params.flat, m.optimizer.exp_avg, m.optimizer.exp_avg_sq)
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        torch.save([b.cpu() for b in bufs], os.path.join(args.dump, mode + ".pt"))
    color_set = m.exposure_set or m.bilagrid_set    # the per-view colour correction's rows, where the mode has one
    print(mode, m.step, m.optimizer.t, m.params.N, *[sha(b) for b in bufs],
          " ".join(n if k == 1 else f"{n}*{k}" for n, k in runs), f"replays={getattr(m, 'speculative_replays', 0)}",
          *([] if color_set is None else [f"color_set={sha(color_set.state)}"]), flush=True)
