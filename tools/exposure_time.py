"""Developer tool: what does per-view exposure compensation (tgs_exposure_fwd / tgs_exposure_bwd) cost?

Part 1, kernels.  At 720p and 1080p, on random images (the kernels' work does not depend on the image content), it times,
in the same process and interleaved,

    copy                  torch's device-to-device copy of 1 GiB (the method of tools/copy_ceiling.py): the bandwidth ceiling
    exposure_fwd          k_expo_fwd: 12 B read + 12 B written per pixel
    exposure_bwd          k_expo_bwd_tiles + k_expo_fold, gradient only: 36 B read + 12 B written per pixel
    exposure_bwd_adam     the same with a state row: the fold also steps the 12 entries
    exposure_bwd_1x1      tgs_exposure_bwd on a 1 x 1 image: the floor of its two launches

with device events: 5 repeats of 20 back-to-back calls each after a warm-up, median of the repeats, all repeats kept.
Every call of a repeat works on its own set of images out of a ring larger than the 256 MiB last-level cache, so that the
bytes come from HBM as they do in a train step, where a frame's images are produced by other kernels.

Part 2, the step.  The train steps of tools/pose_refine_time.py (object-centric 720p, and cfg3 at 1080p) with exposure_lr 0
and 0.01, two models from the same start, interleaved: 5 repeats of 60 steps per model.  The run with the rate 0 issues
exactly the launches of a build without the feature.

    python tools/exposure_time.py [--out profiles/exposure_time.json] [--skip-step]
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

SIZES = {"720p": (1280, 720), "1080p": (1920, 1080)}
RING_BYTES = 768 << 20


def time_kernels(name, W, H, dev, copy_pair):
    from touch_gs_amd import _lib, ops
    per_set = 4 * 12 * W * H                      # rgb, gt, v_img and the written image
    ring = max(RING_BYTES // per_set, 2)
    g = torch.Generator().manual_seed(1)
    sets = []
    for _ in range(ring):
        rgb, gt = torch.rand(H, W, 3, generator=g).to(dev), torch.rand(H, W, 3, generator=g).to(dev)
        sets.append((rgb, gt, (torch.randn(H, W, 3, generator=g) * 1e-6).to(dev), torch.empty(H, W, 3, device=dev)))
    E = torch.tensor([[1.1, 0.02, -0.01, 0.01], [0.0, 0.95, 0.01, -0.02], [0.01, 0.0, 1.05, 0.0]], device=dev)
    state = torch.zeros(_lib.EXPO_STATE, device=dev)
    state[:12], state[37], state[38] = E.reshape(-1), 1.0, 1.0
    P = _lib.load().tgs_exposure_num_partials(W, H)
    out = (torch.empty(_lib.EXPO_OUT, device=dev), torch.empty(P, _lib.EXPO_OUT, device=dev))
    adam = dict(lr=1e-6, betas=(0.9, 0.999), eps=1e-15, l2=0.0)
    l1w = 0.8 / (3 * W * H)
    one = torch.rand(1, 1, 3, device=dev)
    a, b = copy_pair

    def fwd():
        for i in range(LAUNCHES):
            s = sets[i % ring]
            ops.exposure_fwd(s[0], E, out=s[3])
        return LAUNCHES

    def bwd(st):
        def run():
            for i in range(LAUNCHES):
                s = sets[i % ring]
                ops.exposure_bwd(s[0], E if st is None else st, gt=s[1], l1_weight=l1w, v_img=s[2], state=st, adam=adam, out=out)
            return LAUNCHES
        return run

    def bwd_1x1():
        for _ in range(LAUNCHES):
            ops.exposure_bwd(one, E, gt=one, l1_weight=1.0, v_img=one, out=out)
        return LAUNCHES

    def copy():
        for _ in range(LAUNCHES):
            b.copy_(a)
        return LAUNCHES

    variants = {"copy": copy, "exposure_fwd": fwd, "exposure_bwd": bwd(None), "exposure_bwd_adam": bwd(state),
                "exposure_bwd_1x1": bwd_1x1}
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    copy_tbps = 2 * a.numel() * 4 / (med["copy"] * 1e-6) / 1e12
    bytes_of = {"exposure_fwd": 24 * W * H, "exposure_bwd": 48 * W * H + 128 * P, "exposure_bwd_adam": 48 * W * H + 128 * P}
    tbps = {k: n / (med[k] * 1e-6) / 1e12 for k, n in bytes_of.items()}
    res = dict(width=W, height=H, workgroups=P, ring_sets=ring, ring_mib=ring * per_set >> 20,
               note="exposure_bwd allocates v_rgb per call through the caching allocator: the written image is not one of the ring's",
               us_median={k: round(v, 2) for k, v in med.items()}, us_all={k: [round(x, 2) for x in v] for k, v in times.items()},
               copy_ceiling_TBps=round(copy_tbps, 3), bytes=bytes_of, achieved_TBps={k: round(v, 3) for k, v in tbps.items()},
               fraction_of_copy_ceiling={k: round(v / copy_tbps, 3) for k, v in tbps.items()},
               us_at_copy_ceiling={k: round(n / (copy_tbps * 1e12) * 1e6, 2) for k, n in bytes_of.items()},
               us_tiles_by_difference=round(med["exposure_bwd"] - med["exposure_bwd_1x1"], 2),
               us_adam_by_difference=round(med["exposure_bwd_adam"] - med["exposure_bwd"], 2))
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
        kw = dict(exposure_lr=1e-2) if on else {}
        m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2, spatial_sort=True, **kw), params)
        m.spatial_sort()
        m.enable_speculative_budget()
        m.enable_exposure(views)
        models[on] = m

    def steps(m, n):
        def run():
            for i in range(n):
                m.train_step(views[i % nv], next_view=views[(i + 1) % nv])
            return n
        return run

    variants = {f"exposure_{'on' if on else 'off'}": steps(m, STEPS) for on, m in models.items()}
    for m in models.values():
        steps(m, STEP_WARMUP)()
        m.flush()
    times = interleaved(variants, STEP_REPEATS, lambda f: None)
    for m in models.values():
        m.flush()
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    off, on = med["exposure_off"], med["exposure_on"]
    es = models[True].exposure_set
    res = dict(label=spec["label"] + f", {nv} views, fused optimizer, speculative budget", gaussians=N, width=W, height=H,
               us_per_step_median={k: round(v, 1) for k, v in med.items()},
               us_per_step_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               added_us_per_step=round(on - off, 1), added_fraction=round(on / off - 1, 4),
               replays={("on" if k else "off"): getattr(m, "speculative_replays", 0) for k, m in models.items()},
               row_steps=[int(x) for x in es.state[:, 36].cpu().tolist()],
               mean_gain=round(float(es.state[:, [0, 5, 10]].mean()), 5))
    print("step", json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "exposure_time.json"))
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-cfg3-step", action="store_true", help="time only the 720p step (cfg3 builds 1 M Gaussians)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/exposure_time.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    out = dict(tool="tools/exposure_time.py", device=torch.cuda.get_device_name(0),
               method=f"kernels: device events around {LAUNCHES} back-to-back calls, {REPEATS} repeats interleaved over the variants "
                      f"after a warm-up, the calls of a repeat rotating through a ring of image sets of {RING_BYTES >> 20} MiB; step: "
                      f"device events around {STEPS} train steps, {STEP_REPEATS} repeats interleaved over the two models after "
                      f"{STEP_WARMUP} warm-up steps; medians of the repeats, all repeats kept; microseconds",
               yardstick="copy: torch's device-to-device copy of 1 GiB in the same process (read + write bytes per second).  step: "
                         "the same step with exposure_lr = 0, which issues no launch of the feature",
               kernels={}, step={})
    n = (1 << 30) // 4
    pair = (torch.empty(n, device=dev).normal_(), torch.empty(n, device=dev))
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
