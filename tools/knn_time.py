"""Developer tool: what does the exact k-NN cost against what it replaces (csrc/knn.hip)?

Initial scales.  The cloud train.init_params builds -- half a dense touched object (a noisy spherical shell of radius 0.1),
half a uniform fill of [-1, 1]^3 -- at N = 100 k and N = 1 M:

    init_<N>_torch   the parent's expression: blocked torch.cdist + topk(4), N^2 distances            (one run at 1 M)
    init_<N>_hip     train.knn_scale_hip = ops.knn(k = 3) + sqrt + mean; the stages by device events:
                     bounds (amin / amax + the host read), keys, sort (torch.sort + the int32 cast), build, query

Surface metrics.  Two clouds of 300 k points on a sphere of radius 0.2 m (what a 256^3 extraction of it yields):

    surface_ckdtree  tsdf.surface_metrics on the host (two scipy cKDTree queries, fp64; wall clock)
    surface_hip      tsdf.surface_metrics(device=...) (wall clock, uploads and downloads included) and the two ops.knn(k = 1)
                     calls alone by device events

Every step is a CHILD process of its own under its own time limit; the first step that fails, faults or runs out of time
ends the tool, and nothing more is started on the device.  Repeats after a warm-up, medians, all repeats kept.  No bar is
asserted; the ratios are the finding.

    python tools/knn_time.py [--out profiles/knn_time.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 5
STAGES = ("bounds", "keys", "sort", "build", "query")
# step -> time limit in seconds
STEPS = {"init_100000_hip": 120, "init_100000_torch": 180, "init_1000000_hip": 180, "init_1000000_torch": 420,
         "surface_hip": 180, "surface_ckdtree": 300}


def init_cloud(n, dev):
    """The means of train.init_params for a touch cloud of n / 2 points and a fill of n / 2 (seeds first, then the fill)."""
    import numpy as np
    import torch
    rng = np.random.default_rng(0)
    m = n // 2
    v = rng.normal(size=(m, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    shell = (v * (0.1 + 0.002 * rng.normal(size=(m, 1))) + [0.1, -0.05, 0.2]).astype(np.float32)
    g = torch.Generator().manual_seed(0)
    fill = (torch.rand(n - m, 3, generator=g) - 0.5) * 2
    return torch.cat([torch.from_numpy(shell), fill]).to(dev).contiguous()


def torch_scales(md):
    """The parent's expression (touch_gs_amd/train.py, knn="torch"), verbatim."""
    import torch
    N = md.shape[0]
    blk = max(64, min(4096, (1 << 28) // max(N, 1)))
    kd = torch.empty(N, device=md.device)
    for b in range(0, N, blk):
        d = torch.cdist(md[b:b + blk], md)
        kd[b:b + blk] = d.topk(4, largest=False).values[:, 1:].mean(1).clamp_min(1e-5)
    return kd


def timed(f, repeats):
    import torch
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def step_init(n, how):
    import torch
    from touch_gs_amd import ops
    from touch_gs_amd.train import knn_scale_hip
    dev = torch.device("cuda:0")
    md = init_cloud(n, dev)
    if how == "torch":
        repeats = 1 if n > 200000 else 3
        if n <= 200000:
            torch_scales(md)
        ms = timed(lambda: torch_scales(md), repeats)
        kd = torch_scales(md) if n <= 200000 else None
        res = dict(ms_all=[round(x, 2) for x in ms], ms_median=round(statistics.median(ms), 2), repeats=repeats,
                   warm_up=n <= 200000)
        if kd is not None:
            hip = knn_scale_hip(md)
            rel = ((hip - kd).abs() / kd)
            res["hip_vs_torch_scales"] = dict(max_rel=float(rel.max()), median_rel=float(rel.median()))
        return res
    knn_scale_hip(md)
    torch.cuda.synchronize()
    ms = timed(lambda: knn_scale_hip(md), REPEATS)
    stages = {s: [] for s in STAGES}
    for _ in range(REPEATS):
        ev = {}
        ops.knn(md, 3, timing=ev)
        torch.cuda.synchronize()
        prev = "start"
        for s in STAGES:
            stages[s].append(ev[prev].elapsed_time(ev[s]))
            prev = s
    return dict(ms_all=[round(x, 3) for x in ms], ms_median=round(statistics.median(ms), 3), repeats=REPEATS,
                stage_ms_median={s: round(statistics.median(v), 3) for s, v in stages.items()},
                stage_ms_all={s: [round(x, 3) for x in v] for s, v in stages.items()},
                boxes=(n + 255) // 256)


def surface_clouds(n=300000):
    import numpy as np
    rng = np.random.default_rng(1)

    def sphere(noise):
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return v * (0.2 + noise * rng.normal(size=(n, 1))) + [0.3, -0.2, 1.0]
    return sphere(0.001), sphere(0.0)


def step_surface(how):
    import torch
    from touch_gs_amd import ops
    from touch_gs_amd.tsdf import surface_metrics
    p, g = surface_clouds()
    tau = 2 * 0.6 / 256
    if how == "ckdtree":
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            m = surface_metrics(p, g, tau)
            wall.append((time.perf_counter() - t0) * 1e3)
        return dict(wall_ms_all=[round(x, 1) for x in wall], wall_ms_median=round(statistics.median(wall), 1), metrics=m,
                    points=[len(p), len(g)])
    dev = torch.device("cuda:0")
    surface_metrics(p, g, tau, device=dev)
    wall = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        m = surface_metrics(p, g, tau, device=dev)
        wall.append((time.perf_counter() - t0) * 1e3)
    tp, tg = (torch.from_numpy(x.astype("float32")).to(dev) for x in (p, g))

    def both():
        ops.knn(tg, 1, queries=tp)
        ops.knn(tp, 1, queries=tg)
    ms = timed(both, REPEATS)
    return dict(wall_ms_all=[round(x, 1) for x in wall], wall_ms_median=round(statistics.median(wall), 1),
                two_knn_ms_all=[round(x, 3) for x in ms], two_knn_ms_median=round(statistics.median(ms), 3), metrics=m,
                points=[len(p), len(g)])


def run_step(name):
    parts = name.split("_")
    return step_init(int(parts[1]), parts[2]) if parts[0] == "init" else step_surface(parts[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "knn_time.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    a = ap.parse_args()
    if a.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("tools/knn_time.py needs the GPU: there is nothing to time without it")
        print("KNN_TIME_RESULT " + json.dumps(dict(run_step(a.step), device=torch.cuda.get_device_name(0))), flush=True)
        return
    res = {}                                                         # (this process never opens the device: the children do)
    for name, limit in STEPS.items():
        print(f"step {name} (limit {limit} s)", flush=True)
        try:
            cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], cwd=ROOT, timeout=limit,
                                stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {name} ran past its limit of {limit} s: stopping, nothing more is started")
        line = [l for l in cp.stdout.splitlines() if l.startswith("KNN_TIME_RESULT ")]
        if cp.returncode != 0 or not line:
            print(cp.stdout[-4000:])
            raise SystemExit(f"step {name} ended with status {cp.returncode}: stopping, nothing more is started")
        res[name] = json.loads(line[-1][len("KNN_TIME_RESULT "):])
        if name != "init_100000_hip":
            res[name].pop("device")
        print(json.dumps(res[name]), flush=True)
    ratio = {f"init_{n}": round(res[f"init_{n}_torch"]["ms_median"] / res[f"init_{n}_hip"]["ms_median"], 2) for n in (100000, 1000000)}
    ratio["surface_wall"] = round(res["surface_ckdtree"]["wall_ms_median"] / res["surface_hip"]["wall_ms_median"], 2)
    out = dict(tool="tools/knn_time.py", device=res["init_100000_hip"].pop("device"),
               method=f"every step in a child process of its own under a time limit; device events around whole calls (ms), "
                      f"{REPEATS} repeats after a warm-up (torch path: 3 at 100 k, ONE run without warm-up at 1 M), medians, all "
                      "repeats kept; stages of ops.knn by events recorded inside it; surface metrics by the host clock "
                      "(uploads and downloads included) and the two k = 1 queries alone by events",
               cloud="init: n/2 points on a noisy spherical shell of radius 0.1 + n/2 uniform in [-1,1]^3 (init_params' layout); "
                     "surface: 2 x 300 000 points on a sphere of radius 0.2",
               steps=res, torch_over_hip=ratio)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
