"""Splatfacto-style Gaussian model for the ``depth-gaussian-splatting`` method of Touch-GS.

The reference trains through ``ns-train depth-gaussian-splatting --pipeline.model.depth-loss-mult ..
--pipeline.model.depth-loss-type {DEPTH_UNCERTAINTY_WEIGHTED_LOSS,SIMPLE_LOSS}
--pipeline.model.uncertainty_weight ..`` (reference scripts/train_bunny_real.sh:52,
train_block_data.sh:50, train_bunny_blender.sh:50); the model class itself lives in an absent
submodule, so the method surface mirrors the in-tree nerfstudio plugin evidence
(legacy/model_tactile.py:68,77,103,138,192: populate_modules / get_outputs / get_metrics_dict /
get_loss_dict / get_image_metrics_and_images) and the loss follows SURVEY section 8 row a11.

Two execution paths over the same kernels:
* ``get_outputs`` + ``get_loss_dict`` -- autograd path (ops.render is a torch.autograd.Function);
* ``train_step``                      -- fused path: forward, SSIM, compositing backward with the
  L1 + tactile depth/uncertainty loss evaluated in-kernel, projection backward straight into the
  flat gradient buffer, optional RCCL all-reduce, fused Adam.  No autograd graph, no host sync.
"""
from __future__ import annotations

import collections
import os
import dataclasses
import math
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .bilagrid import BilagridSet
from .camera import Camera
from .exposure import ExposureSet
from .optim import FusedAdam, GaussianParams

DEPTH_LOSS_TYPES = ("DEPTH_UNCERTAINTY_WEIGHTED_LOSS", "SIMPLE_LOSS")
# the per-view colour corrections (colorcorr.ViewColorSet): at most one is active, in ``model.color_set``
COLOR_SETS = (ExposureSet, BilagridSet)


@dataclasses.dataclass
class ModelConfig:
    """Flag names follow the reference's tyro flags (scripts/train_*.sh) and Splatfacto defaults
    (SURVEY App. A.3)."""
    sh_degree: int = 3
    ssim_lambda: float = 0.2
    # run SSIM on a second stream, pipelined by image bands behind K7 (ops.rasterize_bwd_ssim_pipelined): same
    # results.  OFF by default -- measured slower: a band launch of K7 no longer fills the GPU (1080p: four
    # launches of 2040 one-wave tiles take 4 x 210 us against 450 us for the whole image; 4K: 4.60 against
    # 4.43 ms per step), although SSIM itself hides almost completely under K7
    pipeline_ssim: bool = False
    pipeline_ssim_min_tiles: int = 0
    depth_loss_mult: float = 0.2          # scripts/train_block_data.sh:50
    depth_loss_type: str = "DEPTH_UNCERTAINTY_WEIGHTED_LOSS"
    uncertainty_weight: float = 1.0
    depth_eps: float = 1e-6
    # scale-invariant monocular depth term  mono_depth_mult * (1 - rho(D_hat, View.mono_depth))  (ops.depth_corr_fwd_bwd):
    # Pearson correlation over the pixels with a map value and alpha >= mono_depth_alpha_min -- the expected depth of a
    # near-empty pixel is not a depth, and one such outlier wrecks a correlation.  0 = off: no launch, nothing changes
    mono_depth_mult: float = 0.0
    mono_depth_alpha_min: float = 0.5
    # patch-wise (local) term beside it  mono_depth_local_mult * (1 - mean over the active patches of rho_p)
    # (ops.depth_corr_local_fwd_bwd): a monocular network is affine-consistent only locally.  0 = off,
    # independent of mono_depth_mult.  Patches of mono_depth_patch_tiles x mono_depth_patch_tiles tiles (8 = 128 pixels) on a
    # grid that moves by one tile per step (patch_offset); a patch counts with at least mono_depth_patch_min_fill of its
    # area valid and both variances at least mono_depth_patch_min_var of the image's (1e-3: a spread under about 3 % of
    # the image's -- a hyper-parameter, run at this one value)
    mono_depth_local_mult: float = 0.0
    mono_depth_patch_tiles: int = 8
    mono_depth_patch_min_fill: float = 0.25
    mono_depth_patch_min_var: float = 1e-3
    # normal-prior term  normal_prior_mult * (conf-weighted mean of 1 - cos(angle between the normal of the rendered depth
    # and View.normal_prior))  (ops.depth_normal_fwd_bwd).  0 = off: no launch, nothing changes.  A normal is
    # formed where a pixel and its four neighbours have alpha >= normal_alpha_min and the depth steps by at most
    # normal_max_jump of the centre's depth (<= 0: no such gate)
    normal_prior_mult: float = 0.0
    normal_alpha_min: float = 0.5
    normal_max_jump: float = 0.1
    sh_degree_interval: int = 1000
    # Splatfacto's coarse-to-fine schedule (num_downscales 2, resolution_schedule 250): training
    # starts on images downscaled by 2^num_downscales and doubles the resolution every resolution_schedule steps.
    # 0 = always full resolution (the default of this library's ops and of bench.py; the trainers set 2 / 250)
    num_downscales: int = 0
    resolution_schedule: int = 250
    background_color: tuple = (0.0, 0.0, 0.0)
    # Adam learning rates per group (Splatfacto defaults)
    lr_means: float = 1.6e-4
    # Splatfacto's position learning rate decays exponentially 1.6e-4 -> 1.6e-6 over the run
    # (UNVERIFIED-PRIOR); lr_means_final = None keeps it constant
    lr_means_final: Optional[float] = 1.6e-6
    lr_means_max_steps: int = 30000
    lr_scales: float = 5e-3
    lr_quats: float = 1e-3
    lr_opac: float = 5e-2
    lr_sh_dc: float = 2.5e-3
    lr_sh_rest: float = 1.25e-4
    # keep the Gaussians in 3-D Morton order (model.spatial_sort() after every densification); the
    # trainer and bench.py switch it on, library users keep their own row order by default
    spatial_sort: bool = False
    # full Morton re-sort every this many refinements (in between, refine() keeps children next to parents)
    resort_every_refines: int = 10
    # spatial_sort deals the Gaussians that covered more than 32 tiles in the last frame evenly over the binning groups
    # (optim.balanced_order): a layout choice like the Morton order itself, results unchanged
    balance_long_runs: bool = True
    long_run: int = 0          # tiles beyond which a Gaussian is a long run (Camera.long_run); 0 = chosen at every re-sort (32, or 8 for object-centric frames)
    # camera pose refinement (touch_gs_amd.pose): Adam learning rates of the per-view rotation (radians) and
    # translation (scene units) in the camera frame.  Both 0 = off: no launch, nothing changes.  pose_l2_*: pull of the
    # accumulated change towards the original pose; pose_start_step: the first step that produces a pose gradient
    pose_lr_rot: float = 0.0
    pose_lr_trans: float = 0.0
    pose_l2_rot: float = 0.0
    pose_l2_trans: float = 0.0
    pose_start_step: int = 0
    # per-view exposure compensation (touch_gs_amd.exposure): Adam learning rate of the 3x4 affine colour
    # transform of every registered training view.  0 = off: no launch, nothing changes.  exposure_l2: pull of E towards
    # the identity; exposure_start_step: the first step that compensates (and learns)
    exposure_lr: float = 0.0
    exposure_l2: float = 0.0
    exposure_start_step: int = 0
    # per-view bilateral grids (touch_gs_amd.bilagrid): peak Adam learning rate of the (GW, GH, L) grid of 3x4
    # affine colour transforms of every registered training view (gsplat's schedule: warm-up from 1 %, decay to 1 % at
    # lr_means_max_steps).  0 = off: no launch, nothing changes.  bilagrid_tv: weight of the grid's total variation;
    # bilagrid_start_step: the first step that corrects (and learns).  Does not combine with exposure_lr
    bilagrid_lr: float = 0.0
    bilagrid_shape: Tuple[int, int, int] = (16, 16, 8)
    bilagrid_tv: float = 10.0
    bilagrid_start_step: int = 0
    # fixed-budget MCMC strategy (touch_gs_amd.mcmc): weights of the L1 regularisers on opacity and scale and
    # the rate of the noise on the means (times lr_means), written by ``enable_mcmc`` from its MCMCConfig.  All 0 = off: no
    # launch, nothing changes
    opacity_reg: float = 0.0
    scale_reg: float = 0.0
    mcmc_noise_lr: float = 0.0

    def downscale_factor(self, step: int) -> int:
        """2 ** max(num_downscales - step // resolution_schedule, 0)  (Splatfacto._get_downscale_factor)."""
        if self.num_downscales <= 0 or self.resolution_schedule <= 0:
            return 1
        return 2 ** max(self.num_downscales - step // self.resolution_schedule, 0)

    def lr_means_at(self, step: int) -> float:
        """ExponentialDecay schedule: lr_init * (lr_final / lr_init) ** min(step / max_steps, 1)."""
        if self.lr_means_final is None or self.lr_means_max_steps <= 0:
            return self.lr_means
        t = min(max(step, 0) / self.lr_means_max_steps, 1.0)
        return float(math.exp(math.log(self.lr_means) * (1 - t) + math.log(self.lr_means_final) * t))

    def lrs(self) -> Dict[str, float]:
        return dict(means=self.lr_means, log_scales=self.lr_scales, quats=self.lr_quats,
                    opac_logit=self.lr_opac, sh_dc=self.lr_sh_dc, sh_rest=self.lr_sh_rest)


def mcmc_configured(c: ModelConfig) -> bool:
    return c.opacity_reg > 0 or c.scale_reg > 0 or c.mcmc_noise_lr > 0


@dataclasses.dataclass(frozen=True)
class Tuning:
    """The launch-shape rules ONE model runs its kernels under, chosen by its re-sort (``spatial_sort``) and handed to
    every launch the model issues: ``long_run`` in the camera (TgsCamera.long_run), the K6 split rule in the per-call
    TgsRasterOpts.  0 / None = the process-wide default (environment, ``ops.set_*``), which the model never writes."""
    long_run: int = 0
    k6_split: Optional[int] = None
    k6_split_floor: Optional[int] = None
    k6_split_heads: Optional[int] = None

    def raster_opts(self):
        return ops.raster_opts(k6_split=self.k6_split, k6_split_floor=self.k6_split_floor, k6_split_heads=self.k6_split_heads)


@dataclasses.dataclass
class View:
    """One training view: camera + supervision images on the device.

    ``depth`` (metres x dataparser scale, 0 = unsupervised) and ``uncertainty`` are what the
    reference's plumbing writes as 16-bit mm PNGs (utils/fuse_touch_vision.py:372-376) and
    registers in transforms.json (utils/add_depth_file_path_to_transforms.py:37-50).
    """
    cam: Camera
    rgb: torch.Tensor                      # [H,W,3] in [0,1]
    depth: Optional[torch.Tensor] = None   # [H,W]
    uncertainty: Optional[torch.Tensor] = None  # [H,W]
    n_valid_depth: Optional[int] = None    # cached count of depth>0 (dataset constant)
    # evaluation only (IS_REAL_WORLD runs, reference scripts/train_bunny_real.sh:54): the sensor's
    # ground-truth depth and the object mask behind results.gt_depth_mse / gt_object_depth_mse
    # (experiment_utils/get_results.py:47-51)
    gt_depth: Optional[torch.Tensor] = None     # [H,W], 0 = no measurement
    object_mask: Optional[torch.Tensor] = None  # [H,W] bool
    # raw monocular depth (e.g. ZoeDepth), 0 = no value, any positive units: supervises through the correlation term
    # (ModelConfig.mono_depth_mult), which is invariant to its scale and shift -- no alignment to a depth sensor needed
    mono_depth: Optional[torch.Tensor] = None   # [H,W]
    # surface-normal prior in this camera's OpenCV axes (x right, y down, z forward: a surface seen head-on is (0, 0, -1)),
    # any length, length 0 = no prior at that pixel, and optional weights >= 0: supervise the normals of the rendered depth
    # (ModelConfig.normal_prior_mult)
    normal_prior: Optional[torch.Tensor] = None  # [H,W,3]
    normal_conf: Optional[torch.Tensor] = None   # [H,W]
    _downscaled: dict = dataclasses.field(default_factory=dict, init=False, repr=False, compare=False)   # d -> downscaled(d)

    def valid_count(self) -> int:
        if self.n_valid_depth is None:
            self.n_valid_depth = int((self.depth > 0).sum().item()) if self.depth is not None else 0
        return self.n_valid_depth

    def set_camera(self, cam: Camera) -> None:
        """Replace the camera (pose refinement), also under the cached downscaled forms of this view."""
        self.cam = cam
        for d, v in self._downscaled.items():
            v.cam = cam.downscaled(d)

    def downscaled(self, d: int) -> "View":
        """This view at 1/d of its resolution (cached): the colour image resized bilinearly to (H // d, W // d) --
        what Splatfacto's ``_downscale_if_required`` does (torchvision resize of a tensor, no antialiasing) --
        depth, uncertainty, mono_depth, normal_prior and normal_conf by nearest neighbour, so that 0 stays "unsupervised" and
        no depth (or normal) is invented across an object boundary; camera as ``Camera.downscaled``."""
        if d <= 1:
            return self
        cache = self._downscaled
        if d not in cache:
            H, W = self.rgb.shape[0] // d, self.rgb.shape[1] // d
            F = torch.nn.functional
            rgb = F.interpolate(self.rgb.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False,
                                antialias=False)[0].permute(1, 2, 0).contiguous()
            near = lambda t: None if t is None else F.interpolate(t[None, None].float(), size=(H, W), mode="nearest")[0, 0].to(t.dtype).contiguous()
            near3 = lambda t: None if t is None else F.interpolate(t.permute(2, 0, 1)[None].float(), size=(H, W),
                                                                   mode="nearest")[0].permute(1, 2, 0).to(t.dtype).contiguous()
            cache[d] = View(cam=self.cam.downscaled(d), rgb=rgb, depth=near(self.depth), uncertainty=near(self.uncertainty),
                            gt_depth=near(self.gt_depth), object_mask=near(self.object_mask), mono_depth=near(self.mono_depth),
                            normal_prior=near3(self.normal_prior), normal_conf=near(self.normal_conf))
        return cache[d]


class DepthGaussianSplattingModel:
    """The trainable scene: flat SoA parameters + the render/loss/step methods."""
    list_hint = True          # speculative budget: learn a bound on the longest tile list, skip the unused sort launches
    LIST_HINT_AFTER = 16      # ... after this many settled frames since the last refinement / replay

    def __init__(self, config: ModelConfig, params: GaussianParams):
        self.config = config
        self.params = params
        self.step = 0
        self.populate_modules()

    # -- nerfstudio Model surface -------------------------------------------------------------
    def populate_modules(self):
        self.optimizer = FusedAdam(self.params, self.config.lrs())
        self.budget = ops.IntersectBudget()
        self._sync_budget = ops.IntersectBudget()   # render / eval path when `budget` is sync-free
        self.fuse_adam = True   # single-process steps use the fused K8+K9 kernel when it applies
        self.dp_factored_sh = True   # data-parallel steps exchange colour gradients, not SH rows
        # single-process steps that know the next view: its K1 runs inside this step's optimizer kernel
        self.front_prefetch = os.environ.get("TGS_FRONT_PREFETCH", "1") != "0"
        # ... and, with a list bound on the budget, bins its pairs directly (ops.set_front_bins / TGS_FRONT_BINS is the process-wide
        # switch and ceiling; this is the model's own)
        self.front_bins = True
        self.last = {}
        self.tuning = Tuning()      # until the first re-sort that has seen a frame: the process defaults
        self._tuned_cams = {}
        self.pose_refiner = None    # enable_pose_refinement(views)
        self._pose_scratch = None
        self.color_set = None       # enable_exposure(views) / enable_bilagrid(views): the one active ViewColorSet
        # every other field the train step keeps between calls is declared HERE: no method creates an attribute
        self.density = None         # enable_densification(): the DensityController | enable_mcmc(): the MCMCController
        self.mcmc = self._mcmc_gen = None   # enable_mcmc(): the TgsMcmcSpec of the step's kernel | the device generator of its noise
        self.last_refine = self._refined_at = None      # what the last density.refine reported, and the step it ran at
        self._recent_cams = collections.OrderedDict()   # id -> full-resolution camera of the last <= 16 steps (spatial_sort)
        self._last_downscale = None     # coarse-to-fine factor of the previous step; None = no step yet, no change of level
        self._graphs = {}           # capture_step_graphs: id(view) -> (graph, last, SH degree, N)
        self._side_stream = None    # pipeline_ssim: the SSIM stream, made on first use
        self._prefetch_ready = self._prefetch_bufs = None   # the ColorPrefetch armed for this step's view | the two that alternate
        # factored data-parallel exchange (_exchange_buffers): the rank's block, its all-gathered image, their per-chunk views
        self._color_block = self._color_all = self._color_rows = self._color_blocks = self._color_blocks_all = None
        self._backward_chunk = None     # K8 of one row chunk, left by forward_backward for the pipelined exchange
        self._dp = self._dp_status = None   # this step's GradSync if data parallel | device {0, any rank overflowed}
        self._pending, self._max_in_flight, self._pinned = None, 4, []      # speculative budget; `_pending is None` = never enabled
        self._seen_need = self._seen_longest = self._good_frames = self.speculative_replays = self._refines_since_sort = 0

    def enable_exposure(self, views):
        """Learn an exposure matrix for each of ``views`` (the full-resolution TRAINING views; held-out views are not
        given and are rendered uncompensated) with the rate of the config; -> the ExposureSet, or None when the rate is 0."""
        return self._enable_color_set(ExposureSet, views, l2=self.config.exposure_l2)

    def enable_bilagrid(self, views):
        """Learn a bilateral grid of colour transforms for each of ``views`` (the full-resolution TRAINING views; held-out
        views are not given and are rendered uncorrected) with the rate, shape and TV weight of the config; -> the
        BilagridSet, or None when the rate is 0."""
        c = self.config
        return self._enable_color_set(BilagridSet, views, shape=c.bilagrid_shape, tv_weight=c.bilagrid_tv,
                                      max_steps=c.lr_means_max_steps)

    def _enable_color_set(self, cls, views, **kw):
        """``color_set`` = ``cls(views, device, the rate of the config, **kw)``, or None when that rate is 0; -> it."""
        c, cs = self.config, self.color_set
        if getattr(c, cls.rate_field) <= 0:
            if isinstance(cs, cls):
                self.color_set = None
            return None
        if self._graphs:
            raise ValueError(f"{cls.what} ({cls.rate_field}) cannot be used with capture_step_graphs: the captured step "
                             "has no launches for it")
        for other in COLOR_SETS:
            if other is not cls and (isinstance(cs, other) or getattr(c, other.rate_field) > 0):
                raise ValueError(f"{cls.what} ({cls.rate_field}) cannot be combined with {other.what} ({other.rate_field}): "
                                 "a grid holds the global transform too")
        self.color_set = cls(views, self.params.flat.device, getattr(c, cls.rate_field), **kw)
        return self.color_set

    exposure_set = property(lambda self: self.color_set if isinstance(self.color_set, ExposureSet) else None)
    bilagrid_set = property(lambda self: self.color_set if isinstance(self.color_set, BilagridSet) else None)

    def enable_pose_refinement(self, views):
        """Refine the poses of ``views`` (the full-resolution TRAINING views; held-out views are not given) with the
        learning rates of the config; -> the PoseRefiner, or None when both rates are 0."""
        c = self.config
        if c.pose_lr_rot <= 0 and c.pose_lr_trans <= 0:
            self.pose_refiner = None
            return None
        if self._graphs:
            raise ValueError("pose refinement (pose_lr_rot / pose_lr_trans) does not combine with capture_step_graphs: a "
                             "captured graph bakes the camera in")
        from .pose import PoseRefiner
        self.pose_refiner = PoseRefiner(views, c.pose_lr_rot, c.pose_lr_trans, l2_rot=c.pose_l2_rot, l2_trans=c.pose_l2_trans,
                                        model=self)
        return self.pose_refiner

    def tuned(self, cam: Camera, keep: bool = True) -> Camera:
        """``cam`` carrying this model's ``tuning.long_run``: what every launch of the model is given, so that K1's
        counting box, ``k_fill_bins`` and K8's sums of one frame -- and the K1 a step runs for the NEXT view -- agree.
        Memoised per camera object (the prefetch and the front buffers recognise their camera by identity) until the
        next re-sort; ``keep=False`` for cameras that may never come back (rendering for evaluation)."""
        lr = self.tuning.long_run
        if lr == 0 or lr == cam.long_run:
            return cam
        hit = self._tuned_cams.get(id(cam))
        if hit is None or hit[0] is not cam or hit[1].long_run != lr:
            hit = (cam, dataclasses.replace(cam, long_run=lr))
            if keep:
                self._tuned_cams[id(cam)] = hit
        return hit[1]

    @property
    def num_points(self) -> int:
        return self.params.N

    def active_sh_degree(self, step: Optional[int] = None) -> int:
        c = self.config
        max_deg = int(round(math.sqrt(self.params.K))) - 1
        if c.sh_degree_interval <= 0:
            return min(c.sh_degree, max_deg)
        return min((self.step if step is None else step) // c.sh_degree_interval, c.sh_degree, max_deg)

    def get_outputs(self, cam: Camera, sh_degree: Optional[int] = None, depth_stats: bool = False,
                    normals: bool = False, exposure_of: Optional["View"] = None,
                    bilagrid_of: Optional["View"] = None) -> Dict[str, torch.Tensor]:
        """Camera -> {rgb, depth, accumulation} (differentiable; autograd path).

        ``exposure_of``: a full-resolution training view; where it owns an exposure row (``enable_exposure``), ``rgb`` is
        the compensated image ``ops.apply_exposure(rgb, E)`` (differentiable in the scene; E is a constant here) and
        ``rgb_raw`` the rendered one.  Any other view, and the default call, give the rendered image.
        ``bilagrid_of``: likewise for a view that owns a bilateral grid (``enable_bilagrid``): ``rgb`` is
        ``ops.apply_bilagrid(rgb, grid)``, the grid a constant.

        ``normals=True`` adds ``normal`` [H,W,3]: the unit normals of the rendered depth in the camera's OpenCV axes
        (ops.depth_normals with the config's normal_alpha_min / normal_max_jump; exactly 0 where none is formed), detached.

        ``depth_stats=True`` adds ``median_depth`` [H,W,1] (depth of the Gaussian behind which the transmittance first is
        <= 1/2; 0 where alpha < 1/2), ``depth_var`` / ``depth_std`` [H,W,1] (spread of depth along the ray around the
        expected depth, scene units squared / scene units) and ``median_gid`` int32 [H,W] (-1 = none): a second walk
        over the frame's lists (ops.rasterize_depth_stats), detached -- no gradients flow through them.  The other
        keys and their values are those of the default call."""
        p = self.params
        deg = self.active_sh_degree() if sh_degree is None else sh_degree
        # the autograd / eval path has no replay logic: it always bins with a synchronous budget (a
        # sync-free training budget would turn an eval view that needs more pairs into background)
        budget = self.budget if self.budget.sync else self._sync_budget
        rgb, depth_acc, alpha, radii, *stats = ops.render(p.means, p.log_scales, p.quats, p.opac_logit, p.sh,
                                                          self.tuned(cam, keep=False), deg, budget=budget,
                                                          opts=self.tuning.raster_opts(), depth_stats=depth_stats)
        depth = depth_acc / torch.clamp(alpha, min=1e-10)
        out = dict(rgb=rgb, depth=depth[..., None], accumulation=alpha[..., None],
                   depth_acc=depth_acc, alpha=alpha, radii=radii)
        if depth_stats:
            var, med, gid = stats
            out.update(median_depth=med[..., None], depth_var=var[..., None], depth_std=torch.sqrt(var)[..., None],
                       median_gid=gid)
        if normals:
            out["normal"] = ops.depth_normals(cam, depth_acc, 1.0 - alpha.detach(), self.config.normal_alpha_min,
                                              self.config.normal_max_jump)
        cs = self.color_set
        of = exposure_of if isinstance(cs, ExposureSet) else bilagrid_of if isinstance(cs, BilagridSet) else None
        if of is not None and cs.owns(of):
            out.update(rgb_raw=rgb, rgb=cs.apply(rgb, cs.leaf(of, False)))
        return out

    def depth_loss(self, depth_acc, alpha, view: View) -> torch.Tensor:
        """mean over valid (D_gt > 0) of (D_hat - D_gt)^2 [ / (uw * U + eps) ]."""
        c = self.config
        if c.depth_loss_type not in DEPTH_LOSS_TYPES:
            raise ValueError(c.depth_loss_type)
        m = view.depth > 0
        cnt = m.sum()
        dhat = depth_acc / torch.clamp(alpha, min=1e-10)
        r2 = (dhat - view.depth) ** 2
        # a view without an uncertainty map is supervised with the SIMPLE form (same rule as loss_spec)
        if c.depth_loss_type == "DEPTH_UNCERTAINTY_WEIGHTED_LOSS" and view.uncertainty is not None:
            r2 = r2 / (c.uncertainty_weight * view.uncertainty + c.depth_eps)
        return torch.where(m, r2, torch.zeros_like(r2)).sum() / torch.clamp(cnt, min=1)

    def get_loss_dict(self, outputs, view: View) -> Dict[str, torch.Tensor]:
        c = self.config
        rgb = outputs["rgb"]
        cs, own_terms = self.color_set, {}
        if cs is not None and cs.owns(view) and self.step >= getattr(c, cs.start_field) and "rgb_raw" not in outputs:
            # the autograd path of the colour correction: the loss is taken on the corrected image; its parameters are a leaf
            # whose gradient the caller may read from outputs[cs.name].grad (the fused step learns them on the device)
            leaf = outputs[cs.name] = cs.leaf(view, True)
            rgb = cs.apply(rgb, leaf)
            own_terms = cs.leaf_loss_terms(leaf)
        l1 = (rgb - view.rgb).abs().mean()
        loss = {"main_loss": (1 - c.ssim_lambda) * l1, **own_terms}
        if c.ssim_lambda > 0:
            loss["main_loss"] = loss["main_loss"] + c.ssim_lambda * (1 - _SSIM.apply(rgb, view.rgb))
        if c.depth_loss_mult > 0 and view.depth is not None:
            loss["depth_loss"] = c.depth_loss_mult * self.depth_loss(outputs["depth_acc"], outputs["alpha"], view)
        if self.mono_depth_local_active(view):
            rho, rho_bar = ops.depth_correlation_local(outputs["depth_acc"], outputs["alpha"], view.mono_depth,
                                                       c.mono_depth_alpha_min, c.mono_depth_patch_tiles, self.patch_offset(),
                                                       c.mono_depth_patch_min_fill, c.mono_depth_patch_min_var)
            if c.mono_depth_mult > 0:
                loss["mono_depth_loss"] = c.mono_depth_mult * (1 - rho)
            loss["mono_depth_local_loss"] = c.mono_depth_local_mult * (1 - rho_bar)
        elif self.mono_depth_active(view):
            rho = ops.depth_correlation(outputs["depth_acc"], outputs["alpha"], view.mono_depth, c.mono_depth_alpha_min)
            loss["mono_depth_loss"] = c.mono_depth_mult * (1 - rho)
        if self.normal_prior_active(view):
            loss["normal_loss"] = c.normal_prior_mult * ops.depth_normal_loss(
                view.cam, outputs["depth_acc"], outputs["alpha"], view.normal_prior, view.normal_conf, c.normal_alpha_min,
                c.normal_max_jump)
        return loss

    def normal_prior_active(self, view: View) -> bool:
        return self.config.normal_prior_mult > 0 and view.normal_prior is not None

    def mono_depth_active(self, view: View) -> bool:
        return self.config.mono_depth_mult > 0 and view.mono_depth is not None

    def mono_depth_local_active(self, view: View) -> bool:
        return self.config.mono_depth_local_mult > 0 and view.mono_depth is not None

    def patch_offset(self, step: Optional[int] = None):
        """(off_x, off_y), in tiles, of the patch grid of the local monocular depth term at ``step`` (default: the current
        one): off_x = step % k, off_y = (step // k) % k.  All k^2 alignments in turn; no RNG, no sync, the same on resume.
        A step graph (``capture_step_graphs``) replays the offset its view was captured with."""
        k = self.config.mono_depth_patch_tiles
        step = self.step if step is None else step
        return step % k, (step // k) % k

    @torch.no_grad()
    def get_metrics_dict(self, outputs, view: View) -> Dict[str, torch.Tensor]:
        mse = ((outputs["rgb"] - view.rgb) ** 2).mean()
        m = {"psnr": -10.0 * torch.log10(mse), "gaussian_count": torch.tensor(self.num_points)}
        if view.depth is not None:
            valid = view.depth > 0
            d = outputs["depth"][..., 0]
            m["depth_mse"] = ((d - view.depth)[valid] ** 2).mean() if valid.any() else torch.tensor(0.0)
        if self.pose_refiner is not None:   # mean change of the refined poses against the originals
            dl = self.pose_refiner.deltas()
            m["pose_delta_deg"] = torch.tensor(sum(a for a, _ in dl) / max(len(dl), 1))
            m["pose_delta_m"] = torch.tensor(sum(b for _, b in dl) / max(len(dl), 1))
        if self.color_set is not None:
            m.update(self.color_set.metrics())
        return m

    @torch.no_grad()
    def get_image_metrics_and_images(self, outputs, view: View):
        """Eval metrics with the key names the reference aggregates
        (experiment_utils/get_results.py:35-52); lpips needs pretrained weights and is omitted."""
        mse = ((outputs["rgb"] - view.rgb) ** 2).mean()
        ssim_sum, _ = ops.ssim_fwd_bwd(outputs["rgb"], view.rgb, want_grad=False)
        H, W = view.rgb.shape[:2]
        metrics = {"psnr": float(-10.0 * torch.log10(mse)), "ssim": float(ssim_sum) / (3 * H * W)}
        if view.depth is not None:
            valid = view.depth > 0
            d = outputs["depth"][..., 0]
            metrics["depth_mse"] = float(((d - view.depth)[valid] ** 2).mean()) if valid.any() else 0.0
            metrics["supervised_depth_mse"] = metrics["depth_mse"]
        if view.gt_depth is not None:   # keys the reference's aggregator averages when present
            d = outputs["depth"][..., 0]
            valid = view.gt_depth > 0
            metrics["gt_depth_mse"] = float(((d - view.gt_depth)[valid] ** 2).mean()) if valid.any() else 0.0
            if view.object_mask is not None:
                obj = valid & view.object_mask
                metrics["gt_object_depth_mse"] = float(((d - view.gt_depth)[obj] ** 2).mean()) if obj.any() else 0.0
        images = {"img": torch.cat([view.rgb, outputs["rgb"]], dim=1),
                  "depth": outputs["depth"], "accumulation": outputs["accumulation"]}
        if "median_depth" in outputs:   # get_outputs(depth_stats=True): the same three errors for the median depth
            # same masks as the expected-depth keys; a pixel without a median (alpha < 1/2) counts with its expected depth
            dm = torch.where(outputs["median_gid"] >= 0, outputs["median_depth"][..., 0], outputs["depth"][..., 0])
            mse_of = lambda ref, m: float(((dm - ref)[m] ** 2).mean()) if m.any() else 0.0
            if view.depth is not None:
                metrics["median_depth_mse"] = mse_of(view.depth, view.depth > 0)
            if view.gt_depth is not None:
                valid = view.gt_depth > 0
                metrics["gt_depth_mse_median"] = mse_of(view.gt_depth, valid)
                if view.object_mask is not None:
                    metrics["gt_object_depth_mse_median"] = mse_of(view.gt_depth, valid & view.object_mask)
            images["median_depth"] = outputs["median_depth"]
            images["depth_std"] = outputs["depth_std"]
        if "normal" in outputs:   # get_outputs(normals=True)
            images["normal"] = 0.5 * (outputs["normal"] + 1.0)
            if view.normal_prior is not None:
                # conf-weighted mean angle to the prior over the supervised centres (formed, prior of non-zero length, c > 0)
                n, p = outputs["normal"], view.normal_prior
                pl = p.norm(dim=-1)
                w = torch.ones_like(pl) if view.normal_conf is None else view.normal_conf
                sup = (n.abs().sum(-1) > 0) & (pl > 0) & torch.isfinite(pl) & (w > 0)
                cos = ((n * p).sum(-1) / pl.clamp(min=1e-30)).clamp(-1.0, 1.0)
                ang = torch.rad2deg(torch.acos(cos))
                metrics["normal_angle_deg"] = float((w * ang)[sup].sum() / w[sup].sum()) if sup.any() else 0.0
        return metrics, images

    # -- fused train step ---------------------------------------------------------------------
    def loss_spec(self, view: View) -> dict:
        c = self.config
        H, W = view.rgb.shape[:2]
        spec = dict(gt_rgb=view.rgb, l1_weight=(1 - c.ssim_lambda) / (3 * H * W))
        if c.depth_loss_mult > 0 and view.depth is not None:
            if c.depth_loss_type not in DEPTH_LOSS_TYPES:
                raise ValueError(c.depth_loss_type)
            cnt = max(view.valid_count(), 1)
            spec.update(gt_depth=view.depth, depth_weight=c.depth_loss_mult / cnt,
                        uncertainty=view.uncertainty if c.depth_loss_type == "DEPTH_UNCERTAINTY_WEIGHTED_LOSS" else None,
                        uncertainty_weight=c.uncertainty_weight, eps=c.depth_eps)
        return spec

    def _image_terms(self, view: View, cam: Camera, depth_acc, fT):
        """Monocular depth, then the normal prior -> (their keys of ``last``: those of the terms that ran, v_depth, v_alpha)."""
        c, ran = self.config, {}
        v_depth = v_alpha = None
        if self.mono_depth_local_active(view):   # global + patch-wise term in one op: the same two images
            patch_off = ran["mono_patch_offset"] = self.patch_offset()
            ran["mono_stats"], v_depth, v_alpha = ops.depth_corr_local_fwd_bwd(
                depth_acc, fT, view.mono_depth, c.mono_depth_alpha_min, weight_global=max(c.mono_depth_mult, 0.0),
                weight_local=c.mono_depth_local_mult, patch_tiles=c.mono_depth_patch_tiles, offset=patch_off,
                min_fill=c.mono_depth_patch_min_fill, min_var_ratio=c.mono_depth_patch_min_var)
        elif self.mono_depth_active(view):
            ran["mono_stats"], v_depth, v_alpha = ops.depth_corr_fwd_bwd(
                depth_acc, fT, view.mono_depth, c.mono_depth_alpha_min, weight=c.mono_depth_mult)
        if self.normal_prior_active(view):   # after the Pearson op: the term adds to its two images
            ran["normal_stats"], _, v_depth, v_alpha = ops.depth_normal_fwd_bwd(
                cam, depth_acc, fT, view.normal_prior, view.normal_conf, c.normal_alpha_min, c.normal_max_jump,
                weight=c.normal_prior_mult, accumulate_into=(v_depth, v_alpha) if "mono_stats" in ran else None)
        return ran, v_depth, v_alpha

    def _rgb_loss_backward(self, view: View, cam: Camera, lists, images, v_depth, v_alpha, color_row, guard, may_pipeline: bool):
        """SSIM + K7, band-pipelined or in sequence (with the view's ``color_row``: SSIM on the corrected image)
        -> (partials, tile_loss, ssim_sum, color_out); ``lists`` = (splats, group_base, sorted_gid, tile_start),
        ``images`` = (rgb, depth_acc, final_T)."""
        c, cs, rgb = self.config, self.color_set, images[0]
        w_ssim = -c.ssim_lambda / (3 * cam.H * cam.W)
        spec = self.loss_spec(view)
        if (color_row is None and c.ssim_lambda > 0 and c.pipeline_ssim and cam.num_tiles >= c.pipeline_ssim_min_tiles
                and may_pipeline and not torch.cuda.is_current_stream_capturing()):
            if self._side_stream is None:
                self._side_stream = torch.cuda.Stream(device=rgb.device)
            return ops.rasterize_bwd_ssim_pipelined(cam, *lists, *images, view.rgb, w_ssim, spec, self._side_stream) + (None,)
        ssim_sum = v_rgb = color_out = None
        img = rgb if color_row is None else cs.forward(rgb, color_row)
        if c.ssim_lambda > 0:
            ssim_sum, v_rgb = ops.ssim_fwd_bwd(img, view.rgb, weight=w_ssim, reduce=False)
        if color_row is not None:   # forms the L1 term on the corrected image, hands K7 its upstream image, steps the row
            color_out, v_rgb = cs.backward_step(rgb, color_row, view.rgb, spec["l1_weight"], v_rgb, guard, self.step,
                                                cam.W, cam.H)
            spec.update(gt_rgb=None, l1_weight=0.0)     # the L1 term went in through v_rgb; the depth terms stay fused
        partials, tile_loss = ops.rasterize_bwd(cam, *lists, *images, v_rgb=v_rgb, v_depth=v_depth, v_alpha=v_alpha,
                                                loss=spec, want_tile_loss=True)
        return partials, tile_loss, ssim_sum, color_out

    def forward_backward(self, view: View, want_v_xy: bool = False, fuse_adam: bool = False,
                         color_block: Optional[torch.Tensor] = None, begin_step: bool = True,
                         colors=None, prefetch=None, next_front=None, pose_grad: bool = False,
                         color_row: Optional[torch.Tensor] = None):
        """Forward + loss + backward of one view into ``params.grad`` (overwritten) -- or, with
        ``fuse_adam``, straight through the optimizer update (K8+K9 fused, ``params.grad`` untouched).
        ``pose_grad``: also ``last["pose_grad"]`` = ``ops.pose_grad`` of this frame, launched before the optimizer
        kernel changes the parameters it was rendered with.
        ``color_row``: the view's row in ``color_set`` (``ViewColorSet.row``): the RGB loss is taken on the corrected image
        C' -- the set's ``forward``, SSIM on C', its ``backward_step`` (which forms the L1 term, hands K7 its upstream image
        and steps the row), K7 without its fused L1 term -- and ``last[color_set.name]`` = the result vector of that call.
        No host sync unless ``budget.sync``.  Returns device tensors (l1+depth tile losses, ssim sum)."""
        p, cam, deg = self.params, self.tuned(view.cam), self.active_sh_degree()
        splats, radii, group_base, tile_start, sorted_gid, status = ops.project_bin_sort(
            cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, self.budget, want_radii=want_v_xy,
            colors=colors, next_front=next_front)
        guard = None if self.budget.sync else status   # overflowed frame => optimizer kernels are no-ops
        rgb, depth_acc, fT, fidx = ops.rasterize_fwd(cam, splats, sorted_gid, tile_start, opts=self.tuning.raster_opts())
        ran, v_depth, v_alpha = self._image_terms(view, cam, depth_acc, fT)
        if color_row is not None and color_block is not None:
            raise ValueError(f"{self.color_set.what} ({self.color_set.rate_field}) cannot be used in data-parallel steps")
        partials, tile_loss, ssim_sum, color_out = self._rgb_loss_backward(
            view, cam, (splats, group_base, sorted_gid, tile_start), (rgb, depth_acc, fT), v_depth, v_alpha, color_row, guard,
            may_pipeline=not ran)
        if color_out is not None:
            ran[self.color_set.name] = color_out
        if pose_grad:
            if color_block is not None:
                raise ValueError("pose refinement (pose_lr_rot / pose_lr_trans) is not supported in data-parallel steps")
            G = ops._lib.load().tgs_num_groups(p.N)
            if self._pose_scratch is None or self._pose_scratch.shape[0] < G or self._pose_scratch.device != p.flat.device:
                self._pose_scratch = torch.empty(max(G, 1), ops._lib.POSE_ROW, dtype=torch.float32, device=p.flat.device)
            ran["pose_grad"] = ops.pose_grad(cam, p.means, p.log_scales, p.quats, p.sh, deg, splats, group_base, partials,
                                            guard=guard, out=(torch.empty(ops._lib.POSE_OUT, dtype=torch.float32, device=p.flat.device),
                                                              self._pose_scratch))
        if fuse_adam:
            v_xy = self.optimizer.backward_and_step(cam, deg, splats, group_base, partials, want_v_xy,
                                                    begin=begin_step, guard=guard, prefetch=prefetch)
        elif color_block is not None:   # data-parallel: geometry gradients + colour-gradient block(s)
            if isinstance(color_block, (list, tuple)):
                # pipelined exchange: K8 is launched chunk by chunk by the caller (train_step), between the gathers
                rows, blocks = color_block
                v_xy = torch.empty(p.N, 2, dtype=torch.float32, device=p.flat.device) if want_v_xy else None
                out4 = p.grad_views()[:4]
                def backward_chunk(c):
                    ops.project_bwd_color(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, splats,
                                          group_base, partials, out4, blocks[c], guard=guard, rows=rows[c], v_xy=v_xy)
                self._backward_chunk = backward_chunk
            else:
                v_xy = ops.project_bwd_color(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, splats,
                                             group_base, partials, p.grad_views()[:4], color_block, want_v_xy,
                                             guard=guard)
        else:
            v_xy = ops.project_bwd(cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, splats,
                                   group_base, partials, out=p.grad_views(), want_v_xy=want_v_xy, guard=guard)[5]
        self.last = dict(rgb=rgb, depth_acc=depth_acc, final_T=fT, splats=splats, v_xy=v_xy, radii=radii,
                         tile_loss=tile_loss, ssim_sum=ssim_sum, status=status, guard=guard, view=view, **ran)
        return tile_loss, ssim_sum

    def loss_from(self, tile_loss, ssim_sum, view: View, mono_stats=None, exposure=None, bilagrid=None) -> Dict[str, torch.Tensor]:
        """The loss values of a fused step from what ``forward_backward`` returned.  ``mono_stats``: the statistics of the
        monocular depth term; default = those of the last ``forward_backward`` when ``tile_loss`` is that call's.
        ``exposure`` / ``bilagrid``: the [32] / [8] result of the step's ``ops.exposure_bwd`` / ``ops.bilagrid_bwd``
        (``last["exposure"]`` / ``last["bilagrid"]``) when the step corrected the view's colours -- its L1 value is then in that
        result, not in ``tile_loss``, and ``bilagrid_tv_loss`` = bilagrid_tv x its TV value; the same default.  A caller that
        keeps a ``tile_loss`` beyond its step, or passes a copy of it, keeps and passes that step's result too."""
        c = self.config
        H, W = view.rgb.shape[:2]
        t = tile_loss.sum(0)
        main = t[0]
        kind, result = (ExposureSet, exposure) if exposure is not None else (BilagridSet, bilagrid)
        if result is None and self.color_set is not None and self.last.get("tile_loss") is tile_loss:
            kind, result = type(self.color_set), self.last.get(self.color_set.name)
        if result is not None:
            main = main + kind.l1_value(result)     # the L1 term was taken on the corrected image: K7's column is 0
        if ssim_sum is not None:   # per-block partial sums (or an already reduced scalar)
            main = main + c.ssim_lambda * (1 - ssim_sum.sum() / (3 * H * W))
        out = {"main_loss": main, "depth_loss": t[1]}
        if result is not None:
            out.update(kind.loss_terms(result, c))
        if mono_stats is None and self.last.get("tile_loss") is tile_loss:
            mono_stats = self.last.get("mono_stats")
        if mono_stats is not None:
            if mono_stats.numel() == 8 or c.mono_depth_mult > 0:
                out["mono_depth_loss"] = mono_stats[7]    # weight * (1 - rho), weight = mono_depth_mult
            if mono_stats.numel() == 16:                  # the local term was active in that step
                out["mono_depth_local_loss"] = mono_stats[11]     # mono_depth_local_mult * (1 - rho_bar)
        if self.last.get("tile_loss") is tile_loss and self.last.get("normal_stats") is not None:
            out["normal_loss"] = self.last["normal_stats"][4]     # normal_prior_mult * (mean of 1 - cos)
        return out

    def spatial_sort(self) -> torch.Tensor:
        """Put the Gaussians (parameters, gradients, Adam moments, densification statistics) in 3-D
        Morton order (long-run Gaussians dealt over the groups once a frame has been rendered: ``balance_long_runs``).  Purely a memory-layout choice -- the scene and every result are the same up to
        the permutation -- that makes a binning group of 256 consecutive Gaussians project onto a few
        dozen tiles: K1 then counts per (group, tile) in LDS and issues one global atomic per touched
        tile instead of one per pair, and `k_fill_bins` writes runs instead of single 8-byte pairs.
        Call at start-up and after densification (the trainer and bench.py do).  Returns the
        permutation (new row i = old row perm[i])."""
        from .optim import balanced_order
        # the last frame's tile count per Gaussian (the packed rect of its record): Gaussians with LONG runs of tiles are
        # dealt evenly over the binning groups instead of sitting next to their spatial neighbours (optim.balanced_order)
        hits = None
        cams = list(self._recent_cams.values()) if self.config.balance_long_runs else []
        if os.environ.get("TGS_BALANCE_LONG_RUNS", "1") == "0":     # A/B switch
            cams = []
        if cams:
            # tiles per Gaussian summed over the cameras of the last steps (K1 alone, once per camera: the sort runs every
            # few hundred steps): a Gaussian that is long in one view of a few-view orbit is short in another, and a
            # layout balanced for ONE view left groups of 22 000 pairs in the next (profiles/r6_b_ckpt_loop_bunny.json)
            p, hits = self.params, 0
            for cam in cams:
                sp = ops.project_fwd(cam, p.means, p.log_scales, p.quats, p.opac_logit, None, -1)
                rect = sp[:, 10].contiguous().view(torch.int32)
                hits = hits + ((rect >> 16) & 255) * ((rect >> 24) & 255)
            if self._dp is not None and self._dp.active:
                # data parallel: every rank has seen ITS views only, and the replicas must agree on the row order -- sum the
                # counts over the ranks (the same collective on every rank: re-sorts happen at refinements, which are
                # barrier points) and divide by the rank-independent total
                import torch.distributed as dist
                n_cams = torch.tensor([len(cams)], dtype=torch.int64, device=hits.device)
                hits = hits.to(torch.int64)
                dist.all_reduce(hits, op=dist.ReduceOp.SUM)
                dist.all_reduce(n_cams, op=dist.ReduceOp.SUM)
                hits = (hits + int(n_cams) - 1) // int(n_cams)
            else:
                hits = (hits + len(cams) - 1) // len(cams)    # mean tiles per view (rounded up)
        if hits is not None:
            # which Gaussians count as long runs (Camera.long_run: the kernels' counting box, K8's shared sums AND the rows
            # dealt over the groups here -- one number): 32 tiles, but 8 where the long runs ARE the frame -- an object on a
            # table: 7 % of the Gaussians hold 60 % of the pairs, and a group's pairs set the length of K1's counting,
            # k_fill_bins and K8 (largest group 8 951 -> 5 098 pairs, step -2.9 % / -2.2 % on the saved 720p checkpoints;
            # cfg3 -0.5 ... -1.3 % if it were applied there: profiles/r6_ab_runs.txt).  ModelConfig.long_run fixes it.
            # The same regime wants K6 to split more of its lists (factor 1, floor 128, 2048 heads: -1.7 % of the step on the
            # 720p checkpoints, +1 % on uniform frames, which keep the process's own settings).  The choice is THIS model's
            # (self.tuning, carried by its cameras and raster options): nothing process-wide is written.
            if self.config.long_run > 0:
                self.tuning = Tuning(long_run=self.config.long_run)
            elif float(hits[hits > 32].sum()) / max(float(hits.sum()), 1.0) > 0.3:
                self.tuning = Tuning(long_run=8, k6_split=1, k6_split_floor=128, k6_split_heads=2048)
            else:
                self.tuning = Tuning(long_run=32)
        long_run = self.tuning.long_run or 32     # (0 only while hits is None: plain Morton order, the value is not read)
        perm = balanced_order(self.params.means, hits, long_run=long_run)
        self.params.permute_(perm, self.optimizer.exp_avg, self.optimizer.exp_avg_sq)
        density = self.density
        if density is not None:
            density.grad_norm_sum = density.grad_norm_sum[perm]
            density.vis_count = density.vis_count[perm]
            density.max_radius = density.max_radius[perm]
        self._graphs = {}
        self._tuned_cams = {}
        self._prefetch_ready = None
        self._refines_since_sort = 0
        return perm

    def enable_mcmc(self, cfg=None):
        """Train with the fixed-budget MCMC strategy (touch_gs_amd.mcmc) instead of clone / split / cull: ``density`` becomes
        the MCMCController, and every single-process ``train_step`` runs the unfused backward followed by ONE launch that
        does regularisers + geometry Adam + noise (ops.mcmc_adam_geom) and the SH Adam.  The mode gives up the fused K8+Adam
        kernel with its colour / front prefetch (the noise moves the means after the optimizer: a prefetched K1 would be
        stale), step graphs and data-parallel steps.  -> the controller."""
        from .mcmc import MCMCConfig, MCMCController
        cfg = cfg or MCMCConfig()
        if self.density is not None and not isinstance(self.density, MCMCController):
            raise ValueError("the MCMC strategy (enable_mcmc) does not combine with enable_densification: one refinement "
                             "strategy per model")
        if self._graphs:
            raise ValueError("the MCMC strategy (enable_mcmc) does not combine with capture_step_graphs: the captured step "
                             "is the fused one and has no noise draw")
        dev = self.params.flat.device
        c = self.config
        c.opacity_reg, c.scale_reg, c.mcmc_noise_lr = cfg.opacity_reg, cfg.scale_reg, cfg.noise_lr
        self.density = MCMCController(cfg, self.params.N, dev)
        self.mcmc = cfg.spec()
        self._mcmc_gen = torch.Generator(device=dev).manual_seed(cfg.seed)
        self._prefetch_ready = None
        return self.density

    def _mcmc_step(self, guard) -> None:
        """The optimizer half of an MCMC step from ``params.grad``: one launch for the geometry (regularisers, Adam, noise
        from this model's generator), the SH rows through K9."""
        opt = self.optimizer
        opt.begin_step()
        noise = None
        if self.mcmc.noise_lr > 0:
            noise = torch.randn(self.params.N, 3, generator=self._mcmc_gen, device=self.params.flat.device, dtype=torch.float32)
        ops.mcmc_adam_geom(opt, self.mcmc, noise, guard=guard)
        opt.step_range(opt.geom_end(), -1, guard=guard)

    def enable_densification(self, cfg=None):
        """Turn on Splatfacto-style clone / split / cull refinement (touch_gs_amd.densify)."""
        from .densify import DensifyConfig, DensityController
        if self.mcmc is not None:
            raise ValueError("enable_densification does not combine with the MCMC strategy (enable_mcmc): one refinement "
                             "strategy per model")
        self.density = DensityController(cfg or DensifyConfig(), self.params.N, self.params.flat.device)

    # -- sync-free intersection budget ---------------------------------------------------------
    def enable_speculative_budget(self, capacity: int = 0, max_in_flight: int = 4) -> None:
        """Train without the per-step read-back of the intersection count.  Densification: every
        refinement is a barrier -- the pending verdicts are settled (and overflowed steps replayed) before
        the Gaussians change, overflowed frames add nothing to the refinement statistics, and the
        capacity follows the Gaussian count afterwards.  Every
        step's status word is copied to pinned host memory asynchronously and looked at a few steps
        later.  Data parallel (factored exchange only): the ranks agree on the overflow verdict on the
        device (the flag rides in the pad of the all-gathered colour block, ops.dp_agree_overflow), the
        optimizer kernels of ALL ranks are no-ops from the overflowing step on, and every rank inspects
        the verdict of step s - max_in_flight exactly at step s -- so all ranks notice at the same
        step and replay the same steps (the collectives stay matched).  Correctness does not depend on guessing the capacity right: a
        frame that overflows sets a sticky device word that empties every later frame and turns the
        guarded optimizer kernels into no-ops, so when the host notices it clears the word, grows the
        buffers, rewinds its step counters and replays the affected views -- the model ends up exactly
        where the synchronous budget would have put it (tests/test_gpu_api_surfaces.py)."""
        self.budget = ops.IntersectBudget(capacity=capacity, sync=False, speculative=True)
        self._pending, self._max_in_flight, self._pinned = collections.deque(), max_in_flight, []
        self._dp = self._dp_status = None
        # longest tile list the settled frames have shown (status[3]) -> the budget's max_list_hint: after LIST_HINT_AFTER
        # good frames the sort launches for list classes beyond 1.5 x that are no longer issued (two near-empty launches,
        # ~9 us per step at cfg3); a frame that breaks the bound is void and replayed like an overflow, with the hint off
        self._seen_longest, self._good_frames = 0, 0

    def _speculative_track(self, view: View, distributed: bool = False) -> None:
        # pinned int32[7]: {#intersections, overflow, sufficient capacity, -} of this rank's frame | the verdict | the
        # peer transport's error word (a wait that timed out; the device has already voided the step, see tgs_peer_wait)
        host = self._pinned.pop() if self._pinned else torch.zeros(7, dtype=torch.int32).pin_memory()
        host[:4].copy_(self.budget.last_status4, non_blocking=True)
        # data parallel: the verdict is the agreed flag, not this rank's own.  Single process: the frame's own status word
        # IS words 0, 1 of the four just copied (one 4.6 us copy on the stream per step instead of two, round 6)
        if distributed:
            host[4:6].copy_(self._dp_status, non_blocking=True)
        peer = getattr(self._dp, "peer", None) if distributed else None
        if peer is not None:
            host[6:].copy_(peer.err_word, non_blocking=True)
        else:
            host[6] = 0
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((view, host, ev))
        if distributed:   # deterministic: every rank looks at step s - max_in_flight exactly at step s
            if len(self._pending) > self._max_in_flight:
                self._speculative_poll(block=True, only_one=True)
        else:
            self._speculative_poll(block=len(self._pending) > self._max_in_flight)

    def _speculative_poll(self, block: bool = False, drain: bool = False, only_one: bool = False) -> None:
        while self._pending and (drain or block or (not only_one and self._dp is None and self._pending[0][2].query())):
            view, host, ev = self._pending[0]
            ev.synchronize()
            block = False
            if int(host[6]) != 0:      # surfaces at most max_in_flight steps after the wait gave up, before any replay
                self._dp.peer.raise_if(int(host[6]))
            if int(host[5] if self._dp is not None else host[1]) == 0:
                self._pending.popleft()
                self._seen_need = max(self._seen_need, int(host[2]), int(host[0]))
                self._seen_longest = max(self._seen_longest, int(host[3]))
                self._good_frames += 1
                # armed once every training view of the current resolution level can have been seen (with more
                # than 16 views the bound came from a subset, and a later view beyond 1.5 x + 64 voided its frame)
                need_frames = max(self.LIST_HINT_AFTER, len(self._recent_cams),
                                  self.density.cfg.num_train_data if self.density is not None else 0)
                if self.list_hint and self._good_frames >= need_frames:
                    self.budget.max_list_hint = max(self.budget.max_list_hint, int(1.5 * self._seen_longest) + 64)
                self._pinned.append(host)
                if only_one:
                    return
                continue
            # overflow: this step and everything enqueued after it did nothing on the device
            torch.cuda.synchronize()
            redo = list(self._pending)
            self._pending.clear()
            need = max(int(h[0]) for _, h, _ in redo)      # this rank's own largest frame
            self.budget.capacity = max(self.budget.capacity, int(need * self.budget.growth) + 1024)
            # (if a list longer than the hint voided the frame: every sort class again until enough frames have been seen)
            self._seen_longest = max([self._seen_longest] + [int(h[3]) for _, h, _ in redo])
            self.budget.max_list_hint, self._good_frames = -1, 0
            self.budget.sticky.zero_()
            self._prefetch_ready = None     # announced by a voided step: its front buffers were cleared under the sticky word
            self.optimizer.t -= len(redo)
            self.step -= len(redo)
            self.speculative_replays += len(redo)
            for v, h, _ in redo:
                self._pinned.append(h)
                self.train_step(v, self._dp)

    def flush(self) -> None:
        """Wait for every enqueued step and settle pending overflow checks (call before reading
        ``last``, saving a checkpoint or evaluating when the speculative budget is on)."""
        if self._pending is not None and self.budget.speculative:
            self._speculative_poll(drain=True)
        if self.pose_refiner is not None:
            self.pose_refiner.flush(self)

    # -- hipGraph replay of the step (small scenes are launch bound) ----------------------------
    def capture_step_graphs(self, views, headroom: float = 1.3, share_pool: bool = True) -> None:
        """Capture the fused single-process train step of every view into a hipGraph (via
        torch.cuda.CUDAGraph: memset + K1..K8/K9 nodes, one graph per view because the camera and
        the ground-truth pointers are launch arguments; all graphs share one memory pool).
        ``train_step`` then replays the view's graph: one launch per step instead of ~12, no Python
        between the kernels.  The only per-step scalars, Adam's bias corrections, live in device
        memory (TgsAdamSpec.device_bias_corr).  The intersection buffers are sized once from the
        views (x ``headroom``) and the overflow flag is checked lazily (``budget.check``).
        Graphs are dropped when the active SH degree or the number of Gaussians changes."""
        opt, deg = self.optimizer, self.active_sh_degree()
        if self.pose_refiner is not None or self.config.pose_lr_rot > 0 or self.config.pose_lr_trans > 0:
            raise ValueError("capture_step_graphs does not combine with pose refinement (pose_lr_rot / pose_lr_trans): a "
                             "captured graph bakes the camera in")
        for kind in COLOR_SETS:
            if isinstance(self.color_set, kind) or getattr(self.config, kind.rate_field) > 0:
                raise ValueError(f"capture_step_graphs does not combine with {kind.what} ({kind.rate_field}): the captured "
                                 "step has no launches for it")
        if self.mcmc is not None or mcmc_configured(self.config):
            raise ValueError("capture_step_graphs does not combine with the MCMC strategy (enable_mcmc / opacity_reg, scale_reg, "
                             "mcmc_noise_lr): the captured step is the fused one and has no noise draw")
        if not opt.can_fuse_with_backward(deg):
            raise RuntimeError("step graphs need the fused K8+K9 path (dense SH at its full degree 1 or 3)")
        p = self.params
        need = 0
        for v in views:
            v.valid_count()
            b = ops.IntersectBudget()
            ops.project_bin_sort(self.tuned(v.cam), p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, b)
            need = max(need, b.last_need)   # capacity under the per-XCD split, not the plain pair count
        self.budget = ops.IntersectBudget(capacity=int(need * headroom) + 4096, sync=False)
        self.budget.sticky_word(p.flat.device)   # allocated eagerly, outside the captured region
        opt.use_device_bias_corr = True
        opt.upload_bias_corr()
        torch.cuda.synchronize()
        self._graphs, pool = {}, None
        for v in views:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                self.forward_backward(v, fuse_adam=True, begin_step=False)
            pool = (pool or g.pool()) if share_pool else None
            self._graphs[id(v)] = (g, self.last, deg, p.N)
        opt.use_device_bias_corr = False   # only the captured launches read the device scalars

    def drop_step_graphs(self) -> None:
        self._graphs = {}
        self.optimizer.use_device_bias_corr = False

    def train_step(self, view: View, dp=None, next_view: Optional[View] = None) -> None:
        """One optimizer iteration on one view (per rank).  ``dp``: a parallel.GradSync or None.
        ``next_view``: the view of the FOLLOWING train_step call, if the caller knows it (single
        process, fused optimizer): the optimizer kernel then also evaluates the colours the updated
        Gaussians show to that camera, and the following step's K1 skips the SH rows (colour
        prefetch; same results bit for bit).  The caller promises not to modify the parameters
        between the two calls except through this class."""
        distributed = dp is not None and dp.active
        opt, density = self.optimizer, self.density
        pose_on, color_row, next_view = self._begin_refiners(view, next_view, distributed)
        full_view = view    # what the speculative budget replays (the schedule is applied again on the replay)
        view, next_view = self._apply_schedule(view, next_view)
        deg = self.active_sh_degree()
        pre, self._prefetch_ready = self._prefetch_ready, None
        if self._graphs and not distributed and density is None and self._replay_graph(view, deg):
            return
        mcmc = self.mcmc
        if mcmc is None and mcmc_configured(self.config):
            raise ValueError("opacity_reg / scale_reg / mcmc_noise_lr are set but the MCMC strategy is not enabled: call "
                             "model.enable_mcmc(cfg) before the first train_step")
        if mcmc is not None and distributed:
            raise ValueError("the MCMC strategy (enable_mcmc) is not supported in data-parallel steps (dp.active)")
        # MCMC mode: the unfused backward leaves the gradient in params.grad for the regulariser + Adam + noise launch; no
        # prefetch is armed (the noise moves the means after the optimizer)
        fuse = (not distributed) and mcmc is None and self.fuse_adam and opt.can_fuse_with_backward(deg)
        factored = distributed and self.dp_factored_sh and opt.can_gather_sh()
        if self.budget.speculative and distributed and not factored:
            raise RuntimeError("the speculative intersection budget does not combine with the dense (flat all-reduce) "
                               "data-parallel exchange")
        self._dp = dp if distributed else None
        block = self._exchange_buffers(dp) if factored else None
        # prefetched by the previous step: colours (+ front) from the fused optimizer kernel, or the front alone from
        # the geometry Adam of a data-parallel step
        colors = pre if (pre is not None and (fuse or (factored and pre.front_issued and not pre.colors_valid))
                         and pre.matches(self.tuned(view.cam), self.params.N, deg)) else None
        arm = self._arm_prefetch(next_view, deg, fuse, factored, in_use=colors if fuse else pre)
        self.forward_backward(view, want_v_xy=density is not None and mcmc is None, fuse_adam=fuse, color_block=block,
                              colors=colors, prefetch=arm if fuse else None,
                              next_front=arm.front if arm is not None else None, pose_grad=pose_on, color_row=color_row)
        self._prefetch_ready = arm
        if pose_on:     # taken at the (possibly downscaled) camera, applied to the full-resolution view's pose
            self.pose_refiner.submit(full_view, self.last["pose_grad"])
        if density is not None and not factored:
            # a frame that overflowed its intersection buffer (sync-free budget) rendered nothing and will be
            # replayed: it must not count as a view (guard = its status word, evaluated on the device)
            density.accumulate(self.last["v_xy"], self.last["radii"], view.cam.W, view.cam.H, guard=self.last["guard"],
                               view_key=id(full_view))
        if factored:
            self._factored_tail(dp, view, deg, arm)
        elif distributed:
            dp.reduce_and_step(self.params.grad, opt.step_range, opt.begin_step)
        elif mcmc is not None:
            self._mcmc_step(self.last["guard"])
        elif not fuse:
            opt.step(guard=self.last["guard"])
        self.step += 1
        if self.budget.speculative:
            self._speculative_track(full_view, distributed)
        elif self.budget.sync and distributed and getattr(dp, "peer", None) is not None:
            # synchronous budget: no guard words exist, so the error word is read every step (this mode syncs per step anyway).  A pre-sized
            # sync-free budget (bench.py) neither syncs nor polls: its caller checks the transport at its own sync point (GradSync.check_transport)
            dp.peer.raise_if(int(dp.peer.err_word.item()))
        if density is not None and density.due(self.step) and self._refined_at != self.step:
            self._refine(dp)

    def _begin_refiners(self, view: View, next_view: Optional[View], distributed: bool):
        """Checks and pending updates of the pose refiner and the colour set -> (pose_on, color_row or None, next_view or None)."""
        ref, pose_on = self.pose_refiner, False
        if ref is None and (self.config.pose_lr_rot > 0 or self.config.pose_lr_trans > 0):
            raise ValueError("pose_lr_rot / pose_lr_trans are set but no view is registered for refinement: call "
                             "model.enable_pose_refinement(training_views) before the first train_step")
        if ref is not None:
            if distributed:
                raise ValueError("pose refinement (pose_lr_rot / pose_lr_trans) is not supported in data-parallel steps (dp.active)")
            if next_view is view:      # its gradient is produced in this very step: nothing can be built ahead for it
                next_view = None
            # pending updates land before the view is used -- and before next_cam is armed, so that the prefetch is
            # built for the pose the view will really have (cameras are recognised by identity)
            ref.apply_pending(view, self)
            if next_view is not None:
                ref.apply_pending(next_view, self)
            pose_on = ref.owns(view) and self.step >= self.config.pose_start_step
        cs, color_row = self.color_set, None
        for kind in COLOR_SETS:
            if getattr(self.config, kind.rate_field) > 0 and not isinstance(cs, kind):
                raise ValueError(f"{kind.rate_field} is set but no view is registered for {kind.what}: call "
                                 f"model.enable_{kind.name}(training_views) before the first train_step")
        if cs is not None:
            if distributed:
                raise ValueError(f"{cs.what} ({cs.rate_field}) cannot be used in data-parallel steps (dp.active)")
            if cs.owns(view) and self.step >= getattr(self.config, cs.start_field):
                color_row = cs.row(view)    # of the full-resolution view: its downscaled forms step the same row
        return pose_on, color_row, next_view

    def _apply_schedule(self, view: View, next_view: Optional[View]):
        """The recent cameras, the learning rate of the means, the coarse-to-fine level -> (view, next_view) at their levels."""
        if self.config.balance_long_runs and self.config.spatial_sort:
            # the cameras of the last steps (full resolution), for the next spatial_sort (host-side bookkeeping only)
            rc = self._recent_cams
            rc[id(view.cam)] = view.cam
            rc.move_to_end(id(view.cam))
            if len(rc) > 16:
                rc.popitem(last=False)
        self.optimizer.lrs["means"] = self.config.lr_means_at(self.step)   # scheduled position learning rate
        if self.config.num_downscales > 0:   # coarse-to-fine: this step (and the announced next one) at their resolutions
            d = self.config.downscale_factor(self.step)
            if self._last_downscale not in (None, d) and self._pending is not None:
                # a new resolution level: the lists get ~4x longer -- learn the list bound again instead of voiding a frame
                self._seen_longest, self._good_frames = 0, 0
                self.budget.max_list_hint = -1
            self._last_downscale = d
            view = view.downscaled(d)
            if next_view is not None:
                next_view = next_view.downscaled(self.config.downscale_factor(self.step + 1))
        return view, next_view

    def _replay_graph(self, view: View, deg: int) -> bool:
        """Replay the graph captured for ``view`` -> True = the step is done.  A stale graph (SH degree, N) drops them all."""
        entry = self._graphs.get(id(view))
        if entry is None:
            return False
        if entry[2] != deg or entry[3] != self.params.N:
            self.drop_step_graphs()
            return False
        self.optimizer.begin_step()
        self.optimizer.upload_bias_corr()
        entry[0].replay()
        self.last = entry[1]
        self.step += 1
        return True

    def _exchange_buffers(self, dp):
        """-> (rows, blocks) of the factored exchange: the rank's colour-gradient blocks, one per row chunk, [3 rows + 4] each
        (colour gradients | camera position | overflow flag); ``_color_blocks_all``: their images [world, 3 rows + 4]."""
        rows = dp.color_chunk_rows(self.params.N)
        n = 3 * self.params.N + 4 * len(rows)
        if (self._color_block is None or self._color_block.numel() != n or self._color_all.numel() != n * dp.world
                or self._color_rows != rows):
            dev = self.params.flat.device
            self._color_block = torch.zeros(n, dtype=torch.float32, device=dev)
            self._color_all = torch.zeros(dp.world * n, dtype=torch.float32, device=dev)
            self._color_rows, self._color_blocks, self._color_blocks_all, off = rows, [], [], 0
            for b, e in rows:
                m = 3 * (e - b) + 4
                self._color_blocks.append(self._color_block[off:off + m])
                self._color_blocks_all.append(self._color_all[dp.world * off:dp.world * (off + m)].view(dp.world, m))
                off += m
        return rows, self._color_blocks

    def _arm_prefetch(self, next_view: Optional[View], deg: int, fuse: bool, factored: bool, in_use):
        """-> the ColorPrefetch armed for the next view (its K1 runs inside this step's last optimizer kernel, under the rule its own step
        will run K8 with) or None.  Fused: colours + front; factored data parallel: the front alone.  Never the buffer ``in_use``."""
        if next_view is None or not (fuse or (factored and self.front_prefetch)) or self.active_sh_degree(self.step + 1) != deg:
            return None
        next_cam = self.tuned(next_view.cam)
        N, dev, bufs = self.params.N, self.params.flat.device, self._prefetch_bufs
        if bufs is None or bufs[0].N != N or bufs[0].colors.device != dev:
            bufs = self._prefetch_bufs = [ops.ColorPrefetch(N, dev), ops.ColorPrefetch(N, dev)]
        front = None
        if self.front_prefetch and not (fuse and torch.cuda.is_current_stream_capturing()):
            front = ops.FrontBuffers(next_cam, N, self.budget.initial(N), self.density is not None, dev)
            # direct bins (fused single-process step only): sized by the budget's list bound as it stands NOW -- the buffers
            # are per frame, so the bins follow a hint the trainer re-learns; no bound, or bins over the ceiling: fill pass
            if fuse and self.front_bins:
                front.attach_bins(self.budget.list_hint())
        return (bufs[1] if in_use is bufs[0] else bufs[0]).arm(next_cam, deg, front, self.budget, colors_valid=fuse)

    def _factored_tail(self, dp, view: View, deg: int, arm) -> None:
        """Factored data-parallel step after K7: agreed verdict, pipelined exchange with K8 and the Adam forms, statistics."""
        opt, density, rows, dguard = self.optimizer, self.density, self._color_rows, None
        if self.budget.speculative:   # agree the overflow verdict across ranks before anything touches the model
            if self._dp_status is None:
                self._dp_status = torch.zeros(2, dtype=torch.int32, device=self.params.flat.device)
            # a peer-exchange wait that times out raises both words: this step and every later one are voided.  Set every
            # step: a refinement replaces the budget, and with it the sticky word the transport would otherwise keep pointing at
            dp.set_poison_words(self.budget.sticky_word(self.params.flat.device), self._dp_status)
            dguard = self._dp_status
        # the whole tail (SH Adam of every chunk + geometry Adam + the next view's K1) as ONE launch behind the
        # geometry all-reduce, where that is a gain (GradSync.fused_tail: by world size -- on a node the chunked SH
        # Adam hides under the transfers, which the fused launch cannot)
        fused_tail = arm is not None and len(rows) <= 8 and opt.p.K >= 4 and self.params.N > 0 and dp.fused_tail()
        def step_sh_chunk(c, allc, scale):
            if c == 0 and dguard is not None:   # every chunk block of a rank carries the frame's flag
                ops.dp_agree_overflow(dp.world, rows[0][1] - rows[0][0], allc, dguard, self.budget.sticky)
            if not fused_tail:
                opt.step_sh_gathered(dp.world, deg, allc, scale, guard=dguard, rows=rows[c])

        if fused_tail:
            step_geom = lambda b, e, scale: opt.step_sh_gathered_geom_and_project_next(
                dp.world, deg, rows, self._color_blocks_all, scale, dguard, arm)
        elif arm is not None:
            step_geom = lambda b, e, scale: opt.step_geom_and_project_next(deg, scale, dguard, arm)
        else:
            step_geom = lambda b, e, scale: opt.step_range(b, e, scale, guard=dguard)
        dp.pipelined_color_exchange_and_step(
            self.params.grad[:opt.geom_end()], self._color_blocks, self._color_blocks_all, self._backward_chunk,
            step_sh_chunk, step_geom, opt.begin_step)
        self._backward_chunk = None
        if density is not None:   # v_xy exists once the K8 chunks are enqueued
            # guarded by the AGREED verdict (written by chunk 0's dp_agree_overflow, enqueued above), not by this
            # rank's own status word: if another rank's frame overflowed, the step is voided on every rank and
            # replayed, and this rank's (valid) frame must not be counted twice
            # (data parallel: every rank sees its own views; the statistics are summed over the ranks at the
            # refinement, the identities are not -- the window counts as complete by its length, as for anonymous views)
            density.accumulate(self.last["v_xy"], self.last["radii"], view.cam.W, view.cam.H,
                               guard=dguard if dguard is not None else self.last["guard"])

    def _refine(self, dp) -> None:
        """The refinement that is due, a budget for the new N; what was built for the old rows goes; the re-sort counter."""
        if self.budget.speculative:
            # barrier: settle every pending overflow verdict first (a drain that finds one replays the
            # affected steps -- possibly including this one, whose replay then refines; `_refined_at`
            # keeps the outer call from refining a second time)
            self.flush()
            if self._refined_at == self.step:
                return
        n_before = self.params.N
        self.params, self.optimizer, self.last_refine = self.density.refine(self.params, self.optimizer, self.step, dp)
        self._refined_at = self.step
        if self.budget.speculative:
            # the intersection count follows N (capacity_after_refine); a wrong guess only costs a replay
            cap = ops.capacity_after_refine(self._seen_need, self.budget.capacity, n_before, self.params.N)
            self._seen_need = self._seen_longest = self._good_frames = 0     # the lists change with the Gaussians: learn the bound again
            self.budget = ops.IntersectBudget(capacity=cap, sync=False, speculative=True)
        else:
            self.budget = ops.IntersectBudget()  # the intersection count changes with N
        self._prefetch_ready = None
        self._graphs = {}
        if self.config.spatial_sort:
            # refine() puts every spawned row directly behind its parent, so the buffer stays spatially
            # ordered; the full re-sort (argsort + gathers of parameters and both moment buffers) only
            # corrects the slow drift of the means, every `resort_every_refines` refinements
            self._refines_since_sort += 1
            if self._refines_since_sort >= self.config.resort_every_refines:
                self.spatial_sort()

    # -- checkpoint -----------------------------------------------------------------------------
    def state_dict(self):
        sd = dict(flat=self.params.flat, N=self.params.N, K=self.params.K, step=self.step,
                  optim=self.optimizer.state_dict(), config=dataclasses.asdict(self.config))
        if self.pose_refiner is not None:   # only then: checkpoints of runs without refinement keep their keys
            sd["pose"] = self.pose_refiner.state_dict(self)
        if self.color_set is not None:      # likewise
            sd[self.color_set.name] = self.color_set.state_dict()
        if self.mcmc is not None:           # likewise: the noise stream goes on where it stopped
            sd["mcmc"] = dict(generator=self._mcmc_gen.get_state())
        return sd

    def load_state_dict(self, sd):
        """Restores parameters, Adam state and the step counter.  A checkpoint written after
        densification holds a different number of Gaussians: the flat stores are then re-allocated
        at the checkpoint's size (same SH storage degree required)."""
        if sd["K"] != self.params.K:
            raise ValueError(f"checkpoint stores {sd['K']} SH bases per Gaussian, the model {self.params.K}")
        if sd["N"] != self.params.N:
            dev = self.params.flat.device
            self.params = GaussianParams.allocate(sd["N"], sd["K"], dev)
            self.optimizer = FusedAdam(self.params, self.config.lrs())
            self.budget = ops.IntersectBudget()
            self._color_block = self._color_all = None
            self._graphs = {}
            if self.density is not None:
                self.density.reset_stats(sd["N"], dev)
        self.params.flat.copy_(sd["flat"])
        self._prefetch_ready = None
        self.step = sd["step"]
        self.optimizer.load_state_dict(sd["optim"])
        if self.pose_refiner is not None and sd.get("pose") is not None:
            self.pose_refiner.load_state_dict(sd["pose"], self)
        # a model WITHOUT a set ignores the key on purpose: evaluation and export load a corrected run's checkpoint
        # and render every view uncorrected (held-out views have no row); a set of another size is refused by the set
        cs = self.color_set
        if cs is not None and sd.get(cs.name) is not None:
            cs.load_state_dict(sd[cs.name])
        if self.mcmc is not None and sd.get("mcmc") is not None:
            self._mcmc_gen.set_state(sd["mcmc"]["generator"].cpu())


class _SSIM(torch.autograd.Function):
    """Mean SSIM through the K10 kernel, differentiable w.r.t. the rendered image."""

    @staticmethod
    def forward(ctx, img, gt):
        H, W = img.shape[:2]
        tot, v = ops.ssim_fwd_bwd(img.contiguous(), gt.contiguous(), weight=1.0 / (3 * H * W))
        ctx.save_for_backward(v)
        return tot / (3 * H * W)

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        return v * g, None
