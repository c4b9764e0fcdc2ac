"""Self-contained trainer for the ``depth-gaussian-splatting`` method (the build's counterpart of
``ns-train`` / ``ns-eval``, which never travel to the GPU box).

Flags keep the reference's names (scripts/train_bunny_real.sh:52, train_block_data.sh:50):
    python -m touch_gs_amd.train --data <scene> --depth-loss-mult 0.2 \
        --depth-loss-type DEPTH_UNCERTAINTY_WEIGHTED_LOSS --uncertainty-weight 1 \
        --train-split-fraction 0.8 [--max-num-iterations 30000] [--output-dir outputs]
    python -m torch.distributed.run --nproc-per-node 8 -m touch_gs_amd.train ...   # data parallel
    python -m touch_gs_amd.train --synthetic 100000 800 800 ...                    # no data needed

Outputs ``<output-dir>/<scene>/depth-gaussian-splatting/<timestamp>/`` with config.json, checkpoints
``step-<n>.ckpt`` (every --steps-per-save) and ``eval.json`` whose ``results`` keys are the ones the
reference aggregates (experiment_utils/get_results.py:35-52: psnr, ssim, depth_mse,
supervised_depth_mse; lpips is written as NaN -- it needs pretrained network weights).
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import math
import os
import time

import torch

from . import ops, parallel
from .model import DEPTH_LOSS_TYPES, DepthGaussianSplattingModel, ModelConfig, View
from .optim import GaussianParams

SH_C0 = 0.28209479177387814


def knn_scale_hip(means_dev: torch.Tensor) -> torch.Tensor:
    """[N] on the device: the mean distance to the 3 nearest neighbours from the exact HIP k-NN (ops.knn),
    clamped like the torch path of ``init_params``: ``mean(sqrt(dist2[:, :3]), 1).clamp_min(1e-5)``."""
    dist2, _ = ops.knn(means_dev, 3)
    return dist2[:, :3].sqrt().mean(1).clamp_min(1e-5)


def init_params(n: int, K: int, device, seed_points=None, extent: float = 1.0, seed: int = 0,
                seed_fraction: float = 0.5, knn: str = "torch") -> GaussianParams:
    """``n`` initial Gaussians: the touch point cloud (points_touch.npy -- the object's touched surface,
    utils/create_point_cloud_from_touches.py:243-244) + a uniform random fill of the cube [-extent, extent]^3 for
    everything the fingers never reached (table, background), Splatfacto-style: scales from the mean distance to the
    3 nearest neighbours, random rotations, opacity 0.1, SH dc from the point colour.

    A touch cloud can hold far more points than ``n`` (every touch-depth pixel of every training view): it is then
    SUBSAMPLED uniformly at random to ``seed_fraction * n`` points, so that all views contribute and the rest of the
    scene still gets its random fill.  (Rounds 1-4 kept the first ``n`` points in file order -- the first views'
    touches only -- and dropped the fill whenever the cloud was larger than ``n``.)

    ``knn``: how the neighbour distances are found -- "torch" (the default): blocked ``cdist`` + ``topk``, N^2 distances;
    "hip": the spatially indexed exact k-NN kernels (``knn_scale_hip``), which need the device to be a GPU."""
    if knn not in ("torch", "hip"):
        raise ValueError(f"init_params: knn must be 'torch' or 'hip', got {knn!r}")
    g = torch.Generator().manual_seed(seed)
    pts, cols = [], []
    if seed_points is not None and len(seed_points[0]):
        sp, sc = seed_points[0].float(), seed_points[1].float() / 255.0
        cap = max(int(n * seed_fraction), 1)
        if len(sp) > cap:
            sel = torch.randperm(len(sp), generator=g)[:cap]
            sp, sc = sp[sel], sc[sel]
        pts.append(sp)
        cols.append(sc)
    n_rand = max(n - sum(len(p) for p in pts), 0)
    if n_rand:
        pts.append((torch.rand(n_rand, 3, generator=g) - 0.5) * 2 * extent)
        cols.append(torch.rand(n_rand, 3, generator=g))
    means = torch.cat(pts)[:n].float()
    colors = torch.cat(cols)[:n].float()
    N = means.shape[0]
    # mean distance to the 3 nearest neighbours, exact, in blocks (the cloud mixes a dense object with a sparse fill:
    # a subsampled estimate would give the object's points the fill's spacing)
    md = means.to(device)
    blk = max(64, min(4096, (1 << 28) // max(N, 1)))   # <= 1 GiB of distances per block whatever N is
    if knn == "hip":
        kd = knn_scale_hip(md)
    else:
        kd = torch.empty(N, device=md.device)
        for b in range(0, N, blk):
            d = torch.cdist(md[b:b + blk], md)
            kd[b:b + blk] = d.topk(4, largest=False).values[:, 1:].mean(1).clamp_min(1e-5)
    scale = kd.cpu()
    sh = torch.zeros(N, K, 3)
    sh[:, 0] = (colors - 0.5) / SH_C0
    quats = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=1)
    return GaussianParams.from_tensors(means.to(device), torch.log(scale)[:, None].repeat(1, 3).to(device),
                                       quats.to(device), torch.full((N,), math.log(0.1 / 0.9)).to(device),
                                       sh.to(device))


@torch.no_grad()
def color_corrected(rgb: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """``rgb`` [H,W,3] through the 3x4 affine colour transform that fits it to ``gt`` in the least-squares sense (the normal
    equations in fp64; a rank-deficient fit, e.g. a constant render, takes the minimum-norm solution): the common gauge of
    evaluation under per-view colour models (gsplat's evaluation under bilateral grids).  No clamp."""
    X = torch.cat([rgb.reshape(-1, 3).double(), torch.ones(rgb.shape[0] * rgb.shape[1], 1, dtype=torch.float64, device=rgb.device)], dim=1)
    M = torch.linalg.pinv((X.T @ X).cpu(), hermitian=True).to(rgb.device) @ (X.T @ gt.reshape(-1, 3).double())
    return (X @ M).reshape(rgb.shape).float().contiguous()


def evaluate(model: DepthGaussianSplattingModel, views, depth_stats: bool = False, normals: bool = False,
             color_correct: bool = False) -> dict:
    """Mean of the eval metrics over ``views``.  ``depth_stats``: also median_depth_mse / gt_depth_mse_median /
    gt_object_depth_mse_median (the median depth under the masks of the expected-depth keys, whose values do not change).
    ``normals``: also normal_angle_deg over the views that carry a normal prior.  ``color_correct``: also cc_psnr / cc_ssim,
    psnr and ssim of each render after ``color_corrected`` against its ground truth; no other key changes."""
    acc = {}
    kw = dict(normals=True) if normals else {}
    for v in views:
        out = (model.get_outputs(v.cam, sh_degree=model.active_sh_degree(), depth_stats=True, **kw) if depth_stats else
               model.get_outputs(v.cam, sh_degree=model.active_sh_degree(), **kw))
        m, _ = model.get_image_metrics_and_images(out, v)
        if color_correct:
            cc = color_corrected(out["rgb"].detach(), v.rgb)
            H, W = v.rgb.shape[:2]
            m["cc_psnr"] = float(-10.0 * torch.log10(((cc - v.rgb) ** 2).mean()))
            m["cc_ssim"] = float(ops.ssim_fwd_bwd(cc, v.rgb, want_grad=False)[0]) / (3 * H * W)
        for k, x in m.items():
            acc.setdefault(k, []).append(x)
    return {k: float(sum(x) / len(x)) for k, x in acc.items()}


def uncertainty_png(depth_var, dataparser_scale: float = 1.0):
    """Rendered depth variance [H,W] (scene units squared) -> the uint16 image of the pipeline's uncertainty maps
    (utils/fuse_touch_vision.py:372-376): back to m^2 with the dataparser scale squared, clipped to [0, 10], x 1000,
    truncated -- ``plumbing.to_uint16_mm``, so the file loads through the reader of the input maps (dataset.py)."""
    import numpy as np
    from .plumbing import to_uint16_mm
    var_m2 = depth_var.detach().double().cpu().numpy() / (float(dataparser_scale) ** 2)
    return to_uint16_mm(np.clip(var_m2, 0.0, 10.0))


def render_views(model: DepthGaussianSplattingModel, views, out_dir: str, names=None, depth_stats: bool = False,
                 dataparser_scale: float = 1.0, normals: bool = False) -> None:
    """The build's counterpart of ``ns-render dataset`` (reference experiment_utils/run_eval.py:48):
    ``<out_dir>/rgb/<name>.png`` (8-bit) and ``<out_dir>/depth/<name>.png`` (uint16 millimetres, the
    convention of the dataset's own depth maps: utils/fuse_touch_vision.py:372-376).
    ``depth_stats``: also ``median_depth/<name>.png`` (like depth/) and ``uncertainty/<name>.png``, the rendered depth
    variance in the format of the input uncertainty maps (``uncertainty_png``; ``dataparser_scale`` = Scene.scale).
    ``normals``: also ``normal/<name>.png``, the normals of the rendered depth in the camera's OpenCV axes as 8-bit RGB
    (n + 1) / 2, black where none is formed -- the encoding ``dataset.read_normal_map`` reads back."""
    from PIL import Image
    from .plumbing import write_png16
    os.makedirs(os.path.join(out_dir, "rgb"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "depth"), exist_ok=True)
    if depth_stats:
        os.makedirs(os.path.join(out_dir, "median_depth"), exist_ok=True)
        os.makedirs(os.path.join(out_dir, "uncertainty"), exist_ok=True)
    kw = dict(normals=True) if normals else {}
    if normals:
        os.makedirs(os.path.join(out_dir, "normal"), exist_ok=True)
    for i, v in enumerate(views):
        out = (model.get_outputs(v.cam, sh_degree=model.active_sh_degree(), depth_stats=True, **kw) if depth_stats else
               model.get_outputs(v.cam, sh_degree=model.active_sh_degree(), **kw))
        name = os.path.splitext(os.path.basename(names[i]))[0] if names else f"{i:05d}"
        rgb = (out["rgb"].clamp(0, 1) * 255.0 + 0.5).to(torch.uint8).cpu().numpy()
        Image.fromarray(rgb).save(os.path.join(out_dir, "rgb", name + ".png"))
        mm = (out["depth"].reshape(v.cam.H, v.cam.W) * 1000.0).clamp(0, 65535).round().to(torch.int32).cpu().numpy()
        write_png16(os.path.join(out_dir, "depth", name + ".png"), mm.astype("uint16"))
        if normals:
            n = out["normal"]
            img = torch.where(n.abs().sum(-1, keepdim=True) > 0, (0.5 * (n + 1.0) * 255.0 + 0.5).clamp(1, 255), torch.zeros_like(n))
            Image.fromarray(img.to(torch.uint8).cpu().numpy()).save(os.path.join(out_dir, "normal", name + ".png"))
        if depth_stats:
            mm = (out["median_depth"].reshape(v.cam.H, v.cam.W) * 1000.0).clamp(0, 65535).round().to(torch.int32).cpu().numpy()
            write_png16(os.path.join(out_dir, "median_depth", name + ".png"), mm.astype("uint16"))
            write_png16(os.path.join(out_dir, "uncertainty", name + ".png"),
                        uncertainty_png(out["depth_var"].reshape(v.cam.H, v.cam.W), dataparser_scale))


def main(argv=None, view_hook=None):
    """``view_hook(train_views, dataparser_scale)``, if given, is called once the training views are loaded and before anything
    is built on them (experiments that edit the views in memory, e.g. tools/pose_refine_quality.py); not a command-line option."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", type=str, default=None)
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("N", "W", "H"), default=None)
    ap.add_argument("--depth-loss-mult", type=float, default=0.2)
    ap.add_argument("--depth-loss-type", type=str, default="DEPTH_UNCERTAINTY_WEIGHTED_LOSS", choices=DEPTH_LOSS_TYPES)
    ap.add_argument("--uncertainty-weight", "--uncertainty_weight", type=float, default=1.0, dest="uncertainty_weight")
    ap.add_argument("--train-split-fraction", type=float, default=0.9)
    ap.add_argument("--uncertainty-scaling", type=str, default="linear", choices=("linear", "variance", "none"),
                    help="units of the uncertainty map in the scaled scene (dataset.py docstring; UNVERIFIED-PRIOR)")
    ap.add_argument("--uncertainty-floor", type=float, default=None,
                    help="lower bound of the uncertainty map, in the map's own units (dataset.py docstring: without it "
                         "the touched pixels pile the refinement onto the object); default 0 = off = the reference's loss "
                         "for the reference's flags (0.05 under --preset few-view)")
    ap.add_argument("--cull-unseen", dest="cull_unseen", action="store_true", default=None,
                    help="cull Gaussians no training view has had in its frustum for a whole refinement window "
                         "(densify.py; not in Splatfacto; on under --preset few-view)")
    ap.add_argument("--preset", type=str, default="reference", choices=("reference", "few-view"),
                    help="reference: the reference's flags mean what they mean there (uncertainty floor 0, no unseen cull). "
                         "few-view: the two additions that make touch-cloud seeds + a random fill train in the 8-13 view "
                         "regime (DESIGN.md section 10: --uncertainty-floor 0.05, --cull-unseen); explicit flags win")
    ap.add_argument("--mono-depth-dir", type=str, default=None,
                    help="folder under --data with one raw monocular depth map per image (<image stem>.png uint16 or .npy, "
                         "e.g. zoe_depth): supervises through the scale-invariant correlation term, no depth sensor needed")
    ap.add_argument("--mono-depth-mult", type=float, default=0.0,
                    help="weight of mono_depth_mult * (1 - Pearson correlation of rendered depth and the monocular map); 0 = off")
    ap.add_argument("--mono-depth-alpha-min", type=float, default=0.5,
                    help="pixels with less accumulated opacity than this stay out of the correlation")
    ap.add_argument("--mono-depth-local-mult", type=float, default=0.0,
                    help="weight of the patch-wise term: (1 - mean Pearson correlation over patches of the image); 0 = off, "
                         "independent of --mono-depth-mult")
    ap.add_argument("--mono-depth-patch-tiles", type=int, default=8, help="patch side in 16-pixel tiles (1...16; 8 = 128 pixels)")
    ap.add_argument("--mono-depth-patch-min-fill", type=float, default=0.25,
                    help="a patch counts with at least this share of its area valid")
    ap.add_argument("--mono-depth-patch-min-var", type=float, default=1e-3,
                    help="a patch counts with both variances at least this share of the image's")
    ap.add_argument("--normal-dir", type=str, default=None,
                    help="folder under --data with one normal prior per image (<image stem>.npy float [H,W,3], or .png RGB with "
                         "n = 2 v / max - 1; optional <stem>_conf.npy weights): supervises the normals of the rendered depth")
    ap.add_argument("--normal-frame", type=str, default="opencv", choices=("opencv", "opengl"),
                    help="camera axes of the maps; opengl (y up, z towards the viewer) flips y and z on load")
    ap.add_argument("--normal-mult", type=float, default=0.0,
                    help="weight of the conf-weighted mean of 1 - cos(angle between rendered-depth normal and prior); 0 = off")
    ap.add_argument("--normal-max-jump", type=float, default=0.1,
                    help="no normal across a depth step larger than this share of the depth (<= 0: no such gate)")
    ap.add_argument("--eval-normals", action="store_true",
                    help="final evaluation also renders the normals of the depth: eval.json gains normal_angle_deg (views "
                         "with a prior), --render-output gains normal/")
    ap.add_argument("--max-num-iterations", type=int, default=30000)
    ap.add_argument("--steps-per-save", type=int, default=2000)
    ap.add_argument("--steps-per-eval", type=int, default=500)
    ap.add_argument("--num-gaussians", type=int, default=100000)
    ap.add_argument("--random-extent", type=float, default=1.0,
                    help="half side of the cube the random fill of the initial Gaussians is drawn from (scaled scene units)")
    ap.add_argument("--seed-fraction", type=float, default=0.5,
                    help="largest share of the initial Gaussians taken from the touch point cloud")
    ap.add_argument("--eval-views-during-training", type=int, default=0,
                    help="at every --steps-per-eval also print held-out PSNR / depth MSE over this many eval views")
    ap.add_argument("--sh-degree", type=int, default=3)
    ap.add_argument("--sync-budget", action="store_true",
                    help="read the intersection count back every step instead of the sync-free speculative budget")
    ap.add_argument("--render-output", type=str, default=None,
                    help="also dump the eval views' renders (rgb/ + 16-bit mm depth/), like ns-render dataset")
    ap.add_argument("--eval-depth-stats", action="store_true",
                    help="final evaluation also renders median depth and per-pixel depth variance: eval.json gains "
                         "median_depth_mse (+ gt_depth_mse_median / gt_object_depth_mse_median), --render-output gains "
                         "median_depth/ and uncertainty/ (the format of the input uncertainty maps)")
    ap.add_argument("--output-dir", type=str, default="outputs")
    ap.add_argument("--load-checkpoint", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-spatial-sort", action="store_true",
                    help="keep the Gaussians in their initial row order instead of 3-D Morton order")
    ap.add_argument("--densify", dest="densify", action="store_true", default=True,
                    help="Splatfacto-style clone/split/cull refinement (default: on, as in the method the reference trains)")
    ap.add_argument("--no-densify", dest="densify", action="store_false", help="fixed set of Gaussians")
    ap.add_argument("--num-downscales", type=int, default=2,
                    help="Splatfacto's coarse-to-fine schedule: start at 1/2^n resolution (default 2; 0 = off)")
    ap.add_argument("--resolution-schedule", type=int, default=250, help="double the resolution every this many steps")
    ap.add_argument("--refine-every", type=int, default=100)
    ap.add_argument("--warmup-length", type=int, default=500)
    ap.add_argument("--densify-grad-thresh", type=float, default=0.0002)
    ap.add_argument("--pose-lr-rot", type=float, default=0.0,
                    help="camera pose refinement of the TRAINING views: Adam learning rate of the rotation (radians, camera "
                         "frame); 0 with --pose-lr-trans 0 = off (the default under both presets)")
    ap.add_argument("--pose-lr-trans", type=float, default=0.0, help="... of the translation (scene units)")
    ap.add_argument("--pose-l2-rot", type=float, default=0.0, help="pull of the accumulated rotation towards the original pose")
    ap.add_argument("--pose-l2-trans", type=float, default=0.0, help="... of the accumulated translation")
    ap.add_argument("--pose-start-step", type=int, default=0, help="first step that refines poses")
    ap.add_argument("--exposure-lr", type=float, default=0.0,
                    help="per-view exposure compensation of the TRAINING views: Adam learning rate of each view's 3x4 affine "
                         "colour transform (INRIA's exposure_lr is 0.01); 0 = off (the default under both presets)")
    ap.add_argument("--exposure-l2", type=float, default=0.0, help="pull of the exposure matrices towards the identity")
    ap.add_argument("--exposure-start-step", type=int, default=0, help="first step that compensates and learns exposures")
    ap.add_argument("--bilagrid-lr", type=float, default=0.0,
                    help="per-view bilateral grids of the TRAINING views (spatially varying colour correction, gsplat's "
                         "use_bilateral_grid): peak Adam learning rate of each view's grid of 3x4 affine colour transforms "
                         "(gsplat's is 2e-3; warm-up from 1 %% over 1000 steps, decay to 1 %% at the last step); 0 = off (the "
                         "default under both presets).  Does not combine with --exposure-lr")
    ap.add_argument("--bilagrid-shape", type=int, nargs=3, default=(16, 16, 8), metavar=("GW", "GH", "L"),
                    help="vertices of a grid along x, y and the luminance axis")
    ap.add_argument("--bilagrid-tv", type=float, default=10.0, help="weight of the grids' total variation")
    ap.add_argument("--bilagrid-start-step", type=int, default=0, help="first step that corrects and learns the grids")
    ap.add_argument("--strategy", type=str, default="default", choices=("default", "mcmc"),
                    help="refinement strategy: default = Splatfacto's clone / split / cull (--densify); mcmc = fixed-budget "
                         "3DGS-MCMC (touch_gs_amd/mcmc.py): relocation of dead Gaussians, growth by 5 %% up to --cap-max, opacity "
                         "and scale regularisers and noise on the means every step; single process only")
    ap.add_argument("--cap-max", type=int, default=1_000_000, help="mcmc: the largest number of Gaussians")
    ap.add_argument("--mcmc-noise-lr", type=float, default=5e5, help="mcmc: rate of the noise on the means (times the position rate)")
    ap.add_argument("--opacity-reg", type=float, default=0.01, help="mcmc: weight of the mean opacity in the loss")
    ap.add_argument("--scale-reg", type=float, default=0.01, help="mcmc: weight of the mean scale in the loss")
    ap.add_argument("--mcmc-min-opacity", type=float, default=0.005, help="mcmc: a Gaussian at or below this opacity is dead")
    ap.add_argument("--init-knn", type=str, default="torch", choices=("torch", "hip"),
                    help="how the initial scales find each seed's 3 nearest neighbours: torch = blocked cdist + topk (N^2 "
                         "distances); hip = the exact k-NN kernels (csrc/knn.hip).  Recorded in config.json; a config "
                         "without the key was initialised with torch")
    args = ap.parse_args(argv)

    few = args.preset == "few-view"
    if args.uncertainty_floor is None:
        args.uncertainty_floor = 0.05 if few else 0.0
    if args.cull_unseen is None:
        args.cull_unseen = few
    use_mcmc = args.strategy == "mcmc"
    dp = parallel.init_from_env()
    dev = torch.device("cuda", dp.local_rank)
    torch.cuda.set_device(dev)
    K = (args.sh_degree + 1) ** 2
    if args.synthetic:
        from .scene import make_view, synthetic_gaussians
        N, W, H = args.synthetic
        views = [make_view(N, W, H, args.sh_degree, 1235, dev, view=v, n_views=8) for v in range(8)]
        i_train, i_eval = list(range(7)), [7]
        P, _ = synthetic_gaussians(N, W, H, args.sh_degree, 4321)  # a *different* scene to fit from
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        scene_name = f"synthetic_{N}_{W}x{H}"
    else:
        from .dataset import Scene
        scene = Scene(args.data, args.train_split_fraction, dev, uncertainty_scaling=args.uncertainty_scaling,
                      uncertainty_floor=args.uncertainty_floor, mono_depth_dir=args.mono_depth_dir,
                      normal_dir=args.normal_dir, normal_frame=args.normal_frame)
        if args.normal_mult > 0 and not any(v.normal_prior is not None for v in scene.views):
            raise SystemExit("--normal-mult > 0 needs --normal-dir with at least one map")
        if (args.mono_depth_mult > 0 or args.mono_depth_local_mult > 0) and not any(v.mono_depth is not None for v in scene.views):
            raise SystemExit("--mono-depth-mult > 0 needs --mono-depth-dir with at least one map")
        views, i_train, i_eval = scene.views, list(scene.i_train), list(scene.i_eval)
        params = init_params(args.num_gaussians, K, dev, scene.seed_points(), extent=args.random_extent, seed=args.seed,
                             seed_fraction=args.seed_fraction, knn=args.init_knn)
        scene_name = os.path.basename(os.path.normpath(args.data))
    cfg = ModelConfig(sh_degree=args.sh_degree, depth_loss_mult=args.depth_loss_mult,
                      depth_loss_type=args.depth_loss_type, uncertainty_weight=args.uncertainty_weight,
                      spatial_sort=not args.no_spatial_sort, num_downscales=args.num_downscales,
                      resolution_schedule=args.resolution_schedule, mono_depth_mult=args.mono_depth_mult,
                      mono_depth_alpha_min=args.mono_depth_alpha_min, mono_depth_local_mult=args.mono_depth_local_mult,
                      mono_depth_patch_tiles=args.mono_depth_patch_tiles, mono_depth_patch_min_fill=args.mono_depth_patch_min_fill,
                      mono_depth_patch_min_var=args.mono_depth_patch_min_var, normal_prior_mult=args.normal_mult,
                      normal_max_jump=args.normal_max_jump, pose_lr_rot=args.pose_lr_rot, pose_lr_trans=args.pose_lr_trans,
                      pose_l2_rot=args.pose_l2_rot, pose_l2_trans=args.pose_l2_trans, pose_start_step=args.pose_start_step,
                      exposure_lr=args.exposure_lr, exposure_l2=args.exposure_l2, exposure_start_step=args.exposure_start_step,
                      bilagrid_lr=args.bilagrid_lr, bilagrid_shape=tuple(args.bilagrid_shape), bilagrid_tv=args.bilagrid_tv,
                      bilagrid_start_step=args.bilagrid_start_step,
                      opacity_reg=args.opacity_reg if use_mcmc else 0.0, scale_reg=args.scale_reg if use_mcmc else 0.0,
                      mcmc_noise_lr=args.mcmc_noise_lr if use_mcmc else 0.0)
    model = DepthGaussianSplattingModel(cfg, params)
    train_views = [views[i] for i in i_train]
    train_names = [f"view_{i}" for i in i_train] if args.synthetic else [scene.names[i] for i in i_train]
    if (cfg.pose_lr_rot > 0 or cfg.pose_lr_trans > 0) and dp.active:
        raise ValueError("--pose-lr-rot / --pose-lr-trans: pose refinement is not supported in data-parallel runs")
    if cfg.exposure_lr > 0 and dp.active:
        raise ValueError("--exposure-lr: exposure compensation is not supported in data-parallel runs")
    if cfg.bilagrid_lr > 0 and dp.active:
        raise ValueError("--bilagrid-lr: bilateral grids are not supported in data-parallel runs")
    if use_mcmc and dp.active:
        raise ValueError("--strategy mcmc: the MCMC strategy is not supported in data-parallel runs")
    if view_hook is not None:
        view_hook(train_views, 1.0 if args.synthetic else scene.scale)
    model.enable_pose_refinement(train_views)     # held-out views are never refined; before a checkpoint is loaded
    model.enable_exposure(train_views)            # likewise: held-out views have no row and are rendered uncompensated
    if model.enable_bilagrid(train_views) is not None:    # likewise: held-out views have no grid and are rendered uncorrected
        model.bilagrid_set.max_steps = max(args.max_num_iterations, 1)    # the schedule decays to 1 % at the run's last step
    if cfg.spatial_sort:
        model.spatial_sort()
    if use_mcmc:
        from .mcmc import MCMCConfig
        model.enable_mcmc(MCMCConfig(cap_max=args.cap_max, refine_every=args.refine_every, warmup_length=args.warmup_length,
                                     min_opacity=args.mcmc_min_opacity, opacity_reg=args.opacity_reg, scale_reg=args.scale_reg,
                                     noise_lr=args.mcmc_noise_lr, seed=args.seed, num_train_data=len(i_train)))
    elif args.densify:
        from .densify import DensifyConfig
        model.enable_densification(DensifyConfig(refine_every=args.refine_every, warmup_length=args.warmup_length,
                                                 num_train_data=len(i_train), densify_grad_thresh=args.densify_grad_thresh,
                                                 cull_unseen=bool(args.cull_unseen)))
    trainer_state = dict(uncertainty_scaling=args.uncertainty_scaling, uncertainty_floor=args.uncertainty_floor, densify=bool(args.densify),
                         num_downscales=args.num_downscales, cull_unseen=bool(args.cull_unseen), strategy=args.strategy)
    if dp.rank == 0 and (args.uncertainty_floor > 0 or args.cull_unseen):
        print(f"note: this run deviates from the reference's objective / Splatfacto's refinement: uncertainty floor "
              f"{args.uncertainty_floor} (no depth weight above 1 / (uncertainty_weight * floor)), cull_unseen={bool(args.cull_unseen)} "
              f"(--preset {args.preset}; DESIGN.md section 10)", flush=True)
    if args.load_checkpoint:
        sd = torch.load(args.load_checkpoint, map_location=dev)
        model.load_state_dict(sd)
        # the defaults of these three changed between rounds (uncertainty maps linear instead of squared, densification
        # and the resolution schedule on by default): resuming under different settings silently trains a different
        # objective, so the checkpoint records them and a mismatch is reported
        was = sd.get("trainer")
        if was is None:
            print("warning: the checkpoint predates the recorded trainer settings; this run uses "
                  f"{trainer_state} -- pass the flags of the original run explicitly if they differed", flush=True)
        else:
            for k, v in trainer_state.items():
                if k in was and was[k] != v:
                    print(f"warning: checkpoint was trained with {k}={was[k]!r}, this run uses {k}={v!r}", flush=True)
    run_dir = os.path.join(args.output_dir, scene_name, "depth-gaussian-splatting", time.strftime("%Y-%m-%d_%H%M%S"))
    if dp.rank == 0:
        os.makedirs(run_dir, exist_ok=True)
        with open(os.path.join(run_dir, "config.json"), "w") as f:
            json.dump(dict(vars(args), model=dataclasses.asdict(cfg), world_size=dp.world,
                           scene=None if args.synthetic else scene.describe()), f, indent=2)
    if not args.sync_budget and (dp.world == 1 or model.optimizer.can_gather_sh()):
        # no per-step host sync; an overflow is detected late and replayed (data parallel: the ranks
        # agree on it on the device and replay the same steps)
        # TGS_SPEC_CAPACITY: test hook -- an initial capacity far too small forces the overflow / replay path
        model.enable_speculative_budget(capacity=int(os.environ.get("TGS_SPEC_CAPACITY", "0")))
    eval_views = [views[i] for i in i_eval] or train_views[:1]
    t0 = time.time()
    seen_refine, n_refines = None, 0
    for step in range(model.step, args.max_num_iterations):
        view = train_views[dp.views_for_step(step, len(train_views))]
        # single process: tell the step which view follows (colour prefetch, model.train_step)
        nxt = train_views[dp.views_for_step(step + 1, len(train_views))]   # this rank's next view (prefetches)
        model.train_step(view, dp if dp.active else None, next_view=nxt)
        if getattr(model, "_refined_at", None) == model.step and seen_refine != model.step:
            seen_refine, n_refines = model.step, n_refines + 1
        at_eval = (step + 1) % args.steps_per_eval == 0
        at_save = (step + 1) % args.steps_per_save == 0 or step + 1 == args.max_num_iterations
        if at_eval or at_save:
            # EVERY rank drains its pending overflow verdicts at the same steps: a drain that finds an agreed
            # overflow replays steps, collectives included, so a rank-0-only flush would leave the ranks'
            # collectives unmatched (and break "every rank inspects step s - L at step s")
            model.flush()
            dp.check_transport()      # peer transport: a wait that timed out (a rank never delivered) raises here
        if dp.rank == 0 and at_eval:
            loss = model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], model.last["view"])
            print(f"step {step + 1}: " + " ".join(f"{k}={float(v):.5f}" for k, v in loss.items()) +
                  f"  N={model.params.N}  {(step + 1 - 0) / (time.time() - t0):.1f} it/s", flush=True)
            if args.eval_views_during_training > 0:
                k = max(len(eval_views) // args.eval_views_during_training, 1)
                r = evaluate(model, eval_views[::k][:args.eval_views_during_training])
                print(f"   held-out: " + " ".join(f"{a}={b:.5g}" for a, b in r.items()), flush=True)
        if dp.rank == 0 and at_save:
            torch.save(dict(model.state_dict(), trainer=trainer_state), os.path.join(run_dir, f"step-{step + 1:09d}.ckpt"))
            if model.pose_refiner is not None:
                from .pose import save_refined_poses
                save_refined_poses(run_dir, model.pose_refiner, train_names)
            if model.color_set is not None:     # exposures.json / bilagrids.npz
                model.color_set.save(run_dir, train_names)
    model.flush()
    if dp.world > 1:
        dp.assert_replicas_identical(model.params.flat)
    if dp.rank == 0:
        print(f"gaussians {model.params.N}  refinements {n_refines}  speculative replays "
              f"{getattr(model, 'speculative_replays', 0)}", flush=True)
    if dp.rank == 0:
        results = evaluate(model, eval_views, depth_stats=args.eval_depth_stats, normals=args.eval_normals)
        # the reference's aggregator indexes results['lpips'] unconditionally
        # (experiment_utils/get_results.py:38); LPIPS needs pretrained network weights that cannot be
        # fetched here, so the key is present and NaN rather than absent
        results.setdefault("lpips", float("nan"))
        with open(os.path.join(run_dir, "eval.json"), "w") as f:
            json.dump({"experiment_name": scene_name, "method_name": "depth-gaussian-splatting",
                       "checkpoint": run_dir, "results": results}, f, indent=2)
        print(json.dumps(results))
        if args.render_output:
            render_views(model, eval_views, args.render_output,
                         None if args.synthetic is not None else [scene.names[i] for i in i_eval] if i_eval else None,
                         depth_stats=args.eval_depth_stats, dataparser_scale=1.0 if args.synthetic is not None else scene.scale,
                         normals=args.eval_normals)
    dp.barrier()
    if dp.peer is not None:
        dp.peer.close()
        dp.peer = None
    return run_dir


if __name__ == "__main__":
    main()
