"""Fixed-budget MCMC densification (3DGS-MCMC, Kheradmand et al., NeurIPS 2024; gsplat's ``MCMCStrategy``).

The alternative to ``densify.DensityController``: a fixed cap on the number of Gaussians, no gradient thresholds, no
opacity resets, no cull.  Two parts:

* every step (``model.train_step`` in MCMC mode, one HIP launch: ``ops.mcmc_adam_geom``): L1 regularisers on opacity and
  scale push unused Gaussians towards death, and opacity-gated, covariance-shaped noise moves the means after the
  optimizer step;
* every ``refine_every`` steps (``MCMCController.refine``, this module): dead Gaussians (opacity <= ``min_opacity``) are
  RELOCATED onto live ones drawn in proportion to their opacity, then the set GROWS by ``grow_factor`` up to ``cap_max``
  with parents drawn the same way.  A parent drawn c times becomes c + 1 Gaussians at its place whose opacities and
  scales (``ops.mcmc_relocate``, gsplat's ``compute_relocation``) leave the rendered result unchanged.

Each phase is ONE gather per tensor with the ``cnt / first / src`` construction of ``densify.py``: children sit directly
behind their parent, so a Morton-ordered buffer stays ordered.  The draws are deterministic, in the spirit of the split
sampler there: inverse CDF over ``cumsum(o.double())`` with uniforms from a CPU generator seeded from (seed, step, phase),
``searchsorted(right=True)`` -- a zero-weight row is never drawn.

One deliberate difference from gsplat: gsplat zeroes the moments of the sampled parents only and leaves the STALE moments
of a relocated dead row in place; here every new row (relocated or grown) starts with zero moments, which is this
project's convention (densify.py), and so do the parents a relocation lands on; parents of the growth phase keep theirs.

Not supported: data-parallel runs (the replicas would have to agree on the draws and on the noise stream).
"""
from __future__ import annotations

import dataclasses

import torch

from . import ops
from .optim import FusedAdam, GaussianParams


@dataclasses.dataclass
class MCMCConfig:
    cap_max: int = 1_000_000
    refine_every: int = 100
    warmup_length: int = 500
    stop_at: int = 25_000          # the controller stops here; regularisers and noise run to the end of training
    min_opacity: float = 0.005
    grow_factor: float = 1.05
    # the per-step part (TgsMcmcSpec, include/tgs.h)
    opacity_reg: float = 0.01
    scale_reg: float = 0.01
    noise_lr: float = 5e5
    gate_k: float = 100.0
    gate_o0: float = 0.005
    seed: int = 0                  # of the draws here and of the model's noise generator
    num_train_data: int = 0        # read by the speculative budget's list-length hint, as DensifyConfig's

    def spec(self):
        return ops.mcmc_spec(self.opacity_reg, self.scale_reg, self.noise_lr, self.gate_k, self.gate_o0)


def sample_by_opacity(weights: torch.Tensor, n: int, seed: int) -> torch.Tensor:
    """n row indices drawn with replacement with probability proportional to ``weights`` (>= 0, not all 0): inverse CDF
    over the fp64 running sum, uniforms from a CPU generator seeded with ``seed``.  A zero-weight row is never drawn."""
    cdf = torch.cumsum(weights.double(), 0)
    total = cdf[-1]
    g = torch.Generator(device="cpu").manual_seed(seed)
    u = torch.rand(n, generator=g, dtype=torch.float64).to(weights.device) * total
    u = torch.minimum(u, torch.nextafter(total, torch.zeros_like(total)))      # u < total: never past the last positive row
    return torch.searchsorted(cdf, u, right=True).clamp_(max=weights.numel() - 1)


class MCMCController:
    """Same surface as ``densify.DensityController`` (due, accumulate, reset_stats, refine), so the model's refinement
    barrier and ``spatial_sort`` work unchanged; it keeps no per-step statistics."""

    def __init__(self, cfg: MCMCConfig, n: int, device):
        self.cfg = cfg
        self.reset_stats(n, device)

    def reset_stats(self, n: int, device):
        # the three per-row fields spatial_sort permutes along with the rows; nothing reads their values
        self.grad_norm_sum = torch.zeros(n, device=device)
        self.vis_count = torch.zeros(n, device=device)
        self.max_radius = torch.zeros(n, device=device)

    def accumulate(self, v_xy=None, radii=None, W: int = 0, H: int = 0, guard=None, view_key=None):
        """Nothing: the strategy has no gradient thresholds."""

    def due(self, step: int) -> bool:
        c = self.cfg
        return c.warmup_length <= step < c.stop_at and step % c.refine_every == 0 and step > 0

    def _seed(self, step: int, phase: int) -> int:
        return (self.cfg.seed * 2_000_003 + 1_000_003 * (step + 1) + phase) % (2 ** 63 - 1)

    @staticmethod
    def _expand(cur, mom, cnt, draws, min_opacity: float):
        """One gather per tensor: old row i -> cnt[i] consecutive rows; the rows of a run whose parent was drawn
        (``draws`` > 0) take the relocation values.  -> (new tensors, new moments, src, within)."""
        N, dev = cnt.numel(), cnt.device
        first = torch.cumsum(cnt, 0) - cnt
        n_new = int(cnt.sum().item())
        src = torch.repeat_interleave(torch.arange(N, device=dev), cnt, output_size=n_new)    # new row -> old row
        within = torch.arange(n_new, device=dev) - first[src]
        new = {k: v[src] for k, v in cur.items()}
        m_new = {k: (m[src], v[src]) for k, (m, v) in mom.items()}
        ratio = (draws[src] + 1).to(torch.int32).contiguous()
        ops.mcmc_relocate(ratio, new["opac_logit"], new["log_scales"], min_opacity)
        return new, m_new, src, within

    @torch.no_grad()
    def refine(self, params: GaussianParams, optimizer: FusedAdam, step: int, dp=None):
        """Relocate, then grow.  Returns (new GaussianParams, new FusedAdam, info dict)."""
        if dp is not None and getattr(dp, "active", False):
            raise ValueError("the MCMC strategy is not supported in data-parallel runs (dp.active): the replicas would have "
                             "to agree on the draws")
        c = self.cfg
        N, K, dev = params.N, params.K, params.flat.device
        names = GaussianParams.NAMES
        cur = {k: getattr(params, k) for k in names}
        mom = {k: (GaussianParams.views_of(optimizer.exp_avg, N, K)[k], GaussianParams.views_of(optimizer.exp_avg_sq, N, K)[k])
               for k in names}
        changed = False
        # -- relocate: dead rows vanish, each one reappears behind a live parent drawn by opacity; N is unchanged
        opac = torch.sigmoid(cur["opac_logit"])
        dead = opac <= c.min_opacity
        n_dead = int(dead.sum().item())
        relocated = 0
        if 0 < n_dead < N:
            alive = ~dead
            idx = sample_by_opacity(torch.where(alive, opac, torch.zeros_like(opac)), n_dead, self._seed(step, 0))
            draws = torch.bincount(idx, minlength=N)
            cur, mom, src, _ = self._expand(cur, mom, alive.long() * (1 + draws), draws, c.min_opacity)
            hit = draws[src] > 0                        # parents that were drawn and all their children
            for k in names:
                mom[k][0][hit] = 0
                mom[k][1][hit] = 0
            relocated, changed = n_dead, True
        # -- grow: by grow_factor up to the cap, parents drawn from ALL rows by their opacity after the relocation
        n_add = max(0, min(c.cap_max, int(c.grow_factor * N)) - N)
        if n_add > 0 and n_dead < N:                    # (nothing alive: nothing worth multiplying; the refinement is a no-op)
            idx = sample_by_opacity(torch.sigmoid(cur["opac_logit"]), n_add, self._seed(step, 1))
            draws = torch.bincount(idx, minlength=N)
            cur, mom, _, within = self._expand(cur, mom, 1 + draws, draws, c.min_opacity)
            child = within >= 1                         # children start at zero; parents keep their moments
            for k in names:
                mom[k][0][child] = 0
                mom[k][1][child] = 0
            changed = True
        else:
            n_add = 0
        info = dict(before=N, after=N + n_add, relocated=relocated, added=n_add, dead=n_dead)
        if not changed:
            return params, optimizer, info
        new_params = GaussianParams.from_tensors(*[cur[k] for k in names])
        new_opt = FusedAdam(new_params, optimizer.lrs, optimizer.betas, optimizer.eps)
        new_opt.t = optimizer.t
        mv = GaussianParams.views_of(new_opt.exp_avg, new_params.N, K)
        vv = GaussianParams.views_of(new_opt.exp_avg_sq, new_params.N, K)
        for k in names:
            mv[k].copy_(mom[k][0])
            vv[k].copy_(mom[k][1])
        self.reset_stats(new_params.N, dev)
        return new_params, new_opt, info
