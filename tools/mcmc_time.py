"""Developer tool: what does a train step cost in MCMC mode (touch_gs_amd/mcmc.py)?

Part 1, kernels.  For 300 k and 1 M Gaussians (K = 1: only the geometry segments are stepped), in the same process and
interleaved,

    copy             torch's device-to-device copy of 1 GiB (the method of tools/copy_ceiling.py): the bandwidth ceiling
    adam_geom        tgs_adam_step on the geometry range [0, start of sh): 28 B per element, 11 elements per Gaussian
    mcmc_adam_geom   tgs_mcmc_adam_geom with both regularisers and a noise buffer: the same + 12 B of noise read and the
                     second 12 B store of the means per Gaussian
    randn            torch.randn(N, 3) from a device generator: the draw an MCMC step adds

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept.  Every
call of a repeat works on its own optimizer state out of a ring larger than the 256 MiB last-level cache.

Part 2, the step.  Object-centric 720p (the generator of tools/host_vs_gpu.py) and cfg3 (1 M Gaussians, 1080p): four models
from the same start, interleaved, 5 repeats of 60 steps per model after 60 warm-up steps:

    fused            the default step (fused K8+Adam with colour / front prefetch)
    unfused          model.fuse_adam = False: K8 into params.grad, then K9 -- the yardstick, code the strategy does not touch
    mcmc             enable_mcmc with the defaults (regularisers 0.01, noise_lr 5e5); no refinement inside the window
    mcmc_still       the same launches with noise_lr 1e-30: the scene does not move, so the frame's lists stay those of the
                     other models (the noise of `mcmc` changes the scene, and with it K1...K8's work)

and, per model, the host's wall time to enqueue a step into an idle GPU (the method of tools/host_vs_gpu.py).

Part 3: the worst error of tgs_mcmc_relocate over the grid of tests/test_gpu_mcmc.py, in units of its bound.

    python tools/mcmc_time.py [--out profiles/mcmc_time.json] [--skip-cfg3-step]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from depth_corr_time import LAUNCHES, REPEATS, STEP_REPEATS, STEP_WARMUP, STEPS, interleaved
from depth_stats_time import FRAMES

RING_BYTES = 768 << 20
LRS = dict(means=1.6e-4, log_scales=5e-3, quats=1e-3, opac_logit=5e-2, sh_dc=2.5e-3, sh_rest=1.25e-4)


def time_kernels(N, dev, copy_pair):
    from touch_gs_amd import ops
    from touch_gs_amd.optim import FusedAdam, GaussianParams, layout
    K = 1
    total = layout(N, K)["total"]
    per_set = 4 * 4 * total + 12 * N
    ring = max(RING_BYTES // per_set, 2)
    g = torch.Generator().manual_seed(1)
    sets = []
    for _ in range(ring):
        gp = GaussianParams.from_tensors(torch.randn(N, 3, generator=g).to(dev), (torch.rand(N, 3, generator=g) * 3 - 6).to(dev),
                                         torch.randn(N, 4, generator=g).to(dev), (torch.rand(N, generator=g) * 8 - 4).to(dev),
                                         torch.zeros(N, K, 3, device=dev))
        gp.grad.copy_(torch.randn(total, generator=g).to(dev) * 1e-4)
        opt = FusedAdam(gp, LRS)
        opt.t = 1000
        sets.append((opt, torch.randn(N, 3, generator=g).to(dev)))
    spec = ops.mcmc_spec()
    gen = torch.Generator(device=dev).manual_seed(0)
    ge = sets[0][0].geom_end()
    a, b = copy_pair

    def adam():
        for i in range(LAUNCHES):
            sets[i % ring][0].step_range(0, ge)
        return LAUNCHES

    def mcmc():
        for i in range(LAUNCHES):
            opt, nz = sets[i % ring]
            ops.mcmc_adam_geom(opt, spec, nz)
        return LAUNCHES

    def randn():
        for _ in range(LAUNCHES):
            torch.randn(N, 3, generator=gen, device=dev)
        return LAUNCHES

    def copy():
        for _ in range(LAUNCHES):
            b.copy_(a)
        return LAUNCHES

    times = interleaved({"copy": copy, "adam_geom": adam, "mcmc_adam_geom": mcmc, "randn": randn}, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    copy_tbps = 2 * a.numel() * 4 / (med["copy"] * 1e-6) / 1e12
    bytes_of = {"adam_geom": 28 * ge, "mcmc_adam_geom": 28 * 11 * N + 24 * N}
    tbps = {k: n / (med[k] * 1e-6) / 1e12 for k, n in bytes_of.items()}
    finite = all(bool(torch.isfinite(s[0].p.flat).all()) for s in sets)
    res = dict(gaussians=N, ring_sets=ring, ring_mib=ring * per_set >> 20, state_finite_after=finite,
               us_median={k: round(v, 2) for k, v in med.items()}, us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               copy_ceiling_TBps=round(copy_tbps, 3), bytes=bytes_of, achieved_TBps={k: round(v, 3) for k, v in tbps.items()},
               fraction_of_copy_ceiling={k: round(v / copy_tbps, 3) for k, v in tbps.items()},
               us_at_copy_ceiling={k: round(n / (copy_tbps * 1e12) * 1e6, 2) for k, n in bytes_of.items()},
               mcmc_minus_adam_us=round(med["mcmc_adam_geom"] - med["adam_geom"], 2))
    print("kernels", json.dumps(res), flush=True)
    return res


def time_step(spec, dev, deg=3, nv=8):
    from touch_gs_amd.mcmc import MCMCConfig
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_views, synthetic_gaussians
    N, W, H = spec["N"], spec["W"], spec["H"]
    P, _ = synthetic_gaussians(N, W, H, deg, 78, clustered=spec["clustered"])
    views, _ = make_views(N, W, H, deg, 77, dev, nv, clustered=spec["clustered"])
    models = {}
    for name in ("fused", "unfused", "mcmc", "mcmc_still"):
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        if name == "unfused":
            m.fuse_adam = False
        elif name.startswith("mcmc"):
            m.enable_mcmc(MCMCConfig(warmup_length=10 ** 9, noise_lr=5e5 if name == "mcmc" else 1e-30))
        models[name] = m

    def steps(m, n):
        def run():
            for i in range(n):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return n
        return run

    variants = {name: steps(m, STEPS) for name, m in models.items()}
    for m in models.values():
        steps(m, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    # the host's share: wall time to ENQUEUE a burst of 40 steps into an idle GPU, no verdict polling inside the burst (the
    # method of tools/host_vs_gpu.py).  Where it is close to the step time the loop is host-bound and extra launches show in full
    import time
    host = {}
    for k, m in models.items():
        m.flush()
        torch.cuda.synchronize()
        keep, m._max_in_flight = m._max_in_flight, 10 ** 6
        t0 = time.perf_counter()
        steps(m, 40)()
        host[k] = round((time.perf_counter() - t0) / 40 * 1e6, 1)
        torch.cuda.synchronize()
        m._max_in_flight = keep
        m.flush()
    res = dict(label=spec["label"] + f", {nv} views, speculative budget", gaussians=N, width=W, height=H,
               us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               mcmc_over_unfused=round(med["mcmc"] / med["unfused"], 4), mcmc_still_over_unfused=round(med["mcmc_still"] / med["unfused"], 4),
               mcmc_over_fused=round(med["mcmc"] / med["fused"], 4), unfused_over_fused=round(med["unfused"] / med["fused"], 4),
               host_enqueue_us_per_step_burst40=host,
               replays={k: getattr(m, "speculative_replays", 0) for k, m in models.items()},
               intersections_last_frame={k: int(m.budget.last_status4[0]) for k, m in models.items()},
               finite={k: bool(torch.isfinite(m.params.flat).all()) for k, m in models.items()})
    print("step", json.dumps(res), flush=True)
    return res


def relocation_error(dev):
    from tests import mcmc_ref as MR
    from touch_gs_amd import ops
    l, r, new_l, dls = MR.relocation_grid(0.005, (52, 1000))
    ls0 = np.tile(np.asarray([-3.0, 0.5, -7.25], np.float32), (len(l), 1))
    ol, ls = torch.from_numpy(l.copy()).to(dev), torch.from_numpy(ls0.copy()).to(dev)
    ops.mcmc_relocate(torch.from_numpy(r.copy()).to(dev), ol, ls, 0.005)
    ol, ls = ol.cpu().numpy().astype(np.float64), ls.cpu().numpy().astype(np.float64)
    m = r > 1
    ref_ls = ls0.astype(np.float64) + dls[:, None]
    e_l = (np.abs(ol - new_l) / (2.0 ** -23 * np.abs(new_l) + 2.0 ** -40))[m].max()
    e_s = (np.abs(ls - ref_ls) / (2.0 ** -23 * np.abs(ref_ls) + 2.0 ** -40))[m].max()
    return dict(rows=int(m.sum()), bound="2^-23 |ref| + 2^-40", worst_error_over_bound_logit=round(float(e_l), 4),
                worst_error_over_bound_log_scale=round(float(e_s), 4))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "mcmc_time.json"))
    ap.add_argument("--skip-cfg3-step", action="store_true", help="time only the 720p step (cfg3 builds 1 M Gaussians)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/mcmc_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/mcmc_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up, the calls of a repeat rotating through a ring of optimizer states of {RING_BYTES >> 20} MiB; "
                      f"step: device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the four models after "
                      f"{STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="copy: torch's device-to-device copy of 1 GiB in the same process (read + write bytes per second).  step: "
                         "the unfused step (model.fuse_adam = False), which the strategy leaves as it was",
               kernels={}, step={})
    n = (1 << 30) // 4
    pair = (torch.empty(n, device=dev).normal_(), torch.empty(n, device=dev))
    for N in (300_000, 1_000_000):
        out["kernels"][str(N)] = time_kernels(N, dev, pair)
        torch.cuda.empty_cache()
    del pair
    torch.cuda.empty_cache()
    out["relocation"] = relocation_error(dev)
    for name in ("object720",) if a.skip_cfg3_step else ("object720", "cfg3"):
        out["step"][name] = time_step(FRAMES[name], dev)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
