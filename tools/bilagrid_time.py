"""Developer tool: what do per-view bilateral grids (tgs_bilagrid_fwd / tgs_bilagrid_bwd) cost?

Part 1, kernels.  The method of tools/exposure_time.py: at 720p and 1080p, on random images, in the same process and
interleaved,

    copy                  torch's device-to-device copy of 1 GiB: the bandwidth ceiling
    exposure_fwd / _bwd   the exposure op: THE YARDSTICK, its pixel bytes are those of the grid's kernels
    bilagrid_fwd          k_bg_fwd: 12 B read + 12 B written per pixel, the grid from L2
    bilagrid_bwd          k_bg_cells + k_bg_fold + k_bg_step, gradient only: 36 B read + 12 B written per pixel
    bilagrid_bwd_adam     the same with a state row and tv_weight 10, no gradient written: the launches of a train step
    bilagrid_bwd_1x1      tgs_bilagrid_bwd on a 1 x 1 image: the floor of its three launches (fold and step included)

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept, every
call of a repeat on its own set of images out of a ring larger than the last-level cache.

Part 2, the step.  The train steps of tools/exposure_time.py (object-centric 720p, and cfg3 at 1080p) with bilagrid_lr 0
and 2e-3, two models from the same start, interleaved.  The run with the rate 0 issues exactly the launches of a build
without the feature.

    python tools/bilagrid_time.py [--out profiles/bilagrid_time.json] [--skip-step] [--skip-cfg3-step]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from depth_corr_time import LAUNCHES, REPEATS, STEP_REPEATS, STEP_WARMUP, STEPS, interleaved
from depth_stats_time import FRAMES
from exposure_time import RING_BYTES, SIZES

SHAPE = (16, 16, 8)


def time_kernels(name, W, H, dev, copy_pair):
    from touch_gs_amd import _lib, ops
    from touch_gs_amd.bilagrid import identity_grid
    per_set = 4 * 12 * W * H                      # rgb, gt, v_img and the written image
    ring = max(RING_BYTES // per_set, 2)
    g = torch.Generator().manual_seed(1)
    sets = []
    for _ in range(ring):
        rgb, gt = torch.rand(H, W, 3, generator=g).to(dev), torch.rand(H, W, 3, generator=g).to(dev)
        sets.append((rgb, gt, (torch.randn(H, W, 3, generator=g) * 1e-6).to(dev), torch.empty(H, W, 3, device=dev)))
    n, S = ops.bilagrid_sizes(W, H, SHAPE)
    grid = (torch.from_numpy(identity_grid(SHAPE)).reshape(-1) + 0.05 * torch.randn(n, generator=g)).to(dev)
    state = torch.zeros(3 * n + _lib.BILAGRID_TAIL, device=dev)
    state[:n], state[3 * n + 1], state[3 * n + 2] = grid, 1.0, 1.0
    P = _lib.load().tgs_bilagrid_num_partials(W, H, *SHAPE)
    res8, scratch, grad = torch.empty(_lib.BILAGRID_OUT, device=dev), torch.empty(S, device=dev), torch.empty(2, n, device=dev)
    adam = dict(lr=1e-6, betas=(0.9, 0.999), eps=1e-15)
    E = torch.tensor([[1.1, 0.02, -0.01, 0.01], [0.0, 0.95, 0.01, -0.02], [0.01, 0.0, 1.05, 0.0]], device=dev)
    PE = _lib.load().tgs_exposure_num_partials(W, H)
    eout = (torch.empty(_lib.EXPO_OUT, device=dev), torch.empty(PE, _lib.EXPO_OUT, device=dev))
    l1w = 0.8 / (3 * W * H)
    one = torch.rand(1, 1, 3, device=dev)
    a, b = copy_pair

    def each(fn):
        def run():
            for i in range(LAUNCHES):
                fn(sets[i % ring])
            return LAUNCHES
        return run

    def copy():
        for _ in range(LAUNCHES):
            b.copy_(a)
        return LAUNCHES

    variants = {
        "copy": copy,
        "exposure_fwd": each(lambda s: ops.exposure_fwd(s[0], E, out=s[3])),
        "exposure_bwd": each(lambda s: ops.exposure_bwd(s[0], E, gt=s[1], l1_weight=l1w, v_img=s[2], out=eout)),
        "bilagrid_fwd": each(lambda s: ops.bilagrid_fwd(s[0], grid, SHAPE, out=s[3])),
        "bilagrid_bwd": each(lambda s: ops.bilagrid_bwd(s[0], grid, SHAPE, gt=s[1], l1_weight=l1w, v_img=s[2],
                                                        out=(res8, scratch, s[3], grad))),
        "bilagrid_bwd_adam": each(lambda s: ops.bilagrid_bwd(s[0], state, SHAPE, gt=s[1], l1_weight=l1w, v_img=s[2], tv_weight=10.0,
                                                             state=state, adam=adam, want_grad=False, out=(res8, scratch, s[3]))),
        "bilagrid_bwd_1x1": each(lambda s: ops.bilagrid_bwd(one, grid, SHAPE, gt=one, l1_weight=1.0, v_img=one,
                                                            out=(res8, scratch))),
    }
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    copy_tbps = 2 * a.numel() * 4 / (med["copy"] * 1e-6) / 1e12
    R = int(_lib.load().tgs_bilagrid_row_floats(SHAPE[2]))
    bytes_of = {"exposure_fwd": 24 * W * H, "exposure_bwd": 48 * W * H + 128 * PE, "bilagrid_fwd": 24 * W * H + 4 * n,
                "bilagrid_bwd": 48 * W * H + 8 * P * R + 4 * n * 4}
    tbps = {k: v / (med[k] * 1e-6) / 1e12 for k, v in bytes_of.items()}
    res = dict(width=W, height=H, grid=list(SHAPE), workgroups=P, row_floats=R, ring_sets=ring, ring_mib=ring * per_set >> 20,
               us_median={k: round(v, 2) for k, v in med.items()}, us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               copy_ceiling_TBps=round(copy_tbps, 3), bytes=bytes_of, achieved_TBps={k: round(v, 3) for k, v in tbps.items()},
               us_at_copy_ceiling={k: round(v / (copy_tbps * 1e12) * 1e6, 2) for k, v in bytes_of.items()},
               bwd_over_exposure_bwd=round(med["bilagrid_bwd"] / med["exposure_bwd"], 2),
               bwd_adam_over_exposure_bwd=round(med["bilagrid_bwd_adam"] / med["exposure_bwd"], 2),
               fwd_over_exposure_fwd=round(med["bilagrid_fwd"] / med["exposure_fwd"], 2),
               us_cells_by_difference=round(med["bilagrid_bwd"] - med["bilagrid_bwd_1x1"], 2))
    print(name, json.dumps(res), flush=True)
    return res


def time_step(spec, dev, deg=3, nv=8):
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_views, synthetic_gaussians
    N, W, H = spec["N"], spec["W"], spec["H"]
    P, _ = synthetic_gaussians(N, W, H, deg, 78, clustered=spec["clustered"])
    views, _ = make_views(N, W, H, deg, 77, dev, nv, clustered=spec["clustered"])
    models = {}
    for on in (False, True):
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        kw = dict(bilagrid_lr=2e-3, bilagrid_shape=SHAPE) if on else {}
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True, **kw), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        m.enable_bilagrid(views)
        models[on] = m

    def steps(m, k):
        def run():
            for i in range(k):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return k
        return run

    variants = {f"bilagrid_{'on' if on else 'off'}": steps(m, STEPS) for on, m in models.items()}
    for m in models.values():
        steps(m, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    off, on = med["bilagrid_off"], med["bilagrid_on"]
    bs = models[True].bilagrid_set
    res = dict(label=spec["label"] + f", {nv} views, fused optimizer, speculative budget", gaussians=N, width=W, height=H,
               us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               added_us_per_step=round(on - off, 1), added_fraction=round(on / off - 1, 4),
               off_repeat_spread_us=round(max(times["bilagrid_off"]) - min(times["bilagrid_off"]), 1),
               note="with the rate 0 the SSIM pass is band-pipelined with K7; with a grid it runs in sequence (as under exposure_lr)",
               replays={("on" if k else "off"): getattr(m, "speculative_replays", 0) for k, m in models.items()},
               row_steps=[int(x) for x in bs.state[:, 3 * bs.n].cpu().tolist()])
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "bilagrid_time.json"))
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-cfg3-step", action="store_true", help="time only the 720p step (cfg3 builds 1 M Gaussians)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bilagrid_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/bilagrid_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up, the calls of a repeat rotating through a ring of image sets of {RING_BYTES >> 20} MiB; step: "
                      f"device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the two models after "
                      f"{STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="kernels: exposure_fwd / exposure_bwd of the same process (the same pixel bytes), and torch's device-to-device "
                         "copy of 1 GiB.  step: the same step with bilagrid_lr = 0, which issues no launch of the feature",
               not_measured="the step of the parent commit in the same session (with the rate 0 no code of the feature runs)",
               kernels={}, step={})
    k = (1 << 30) // 4
    pair = (torch.empty(k, device=dev).normal_(), torch.empty(k, device=dev))
    for name, (W, H) in SIZES.items():
        out["kernels"][name] = time_kernels(name, W, H, dev, pair)
        torch.cuda.empty_cache()
    del pair
    torch.cuda.empty_cache()
    if not a.skip_step:
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
