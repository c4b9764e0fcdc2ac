"""Developer tool: what do the TSDF fusion and the crossing extraction cost (csrc/tsdf.hip)?

One 256^3 grid (0.6 m cube, trunc 4 voxels) around a sphere of radius 0.2 m, 1280 x 720 depth / weight / colour images of it
from eight cameras on an orbit (analytic, made on the device).  Timed with device events, in one process and interleaved:

    hip_1view            tgs_tsdf_integrate, one view per launch, S + Wt + C          (40 B per voxel and launch)
    hip_8views           eight views per launch                                       (40 B per voxel and launch, 5 B per voxel-view)
    hip_1view_nocolor    C = NULL                                                     (16 B per voxel and launch)
    hip_8views_nocolor
    torch_1view          a plain torch statement of the same update of one view, written for this tool (an independent
    torch_1view_nocolor  implementation, not the code under test): about ten voxel-sized temporaries per view
    extract              tgs_tsdf_extract_count + torch.cumsum + one host read + tgs_tsdf_extract_points on the fused grid

5 repeats after a warm-up, medians, all repeats kept.  The streaming bound of a launch is voxels x bytes read and written
/ the copy ceiling, which the tool measures the way tools/copy_ceiling.py does (a 1 GiB device-to-device copy, read + write
bytes per second).  The HIP and the torch state after the same eight views are compared: the share of voxels where some view
was decided differently (a pixel edge or the -trunc cut: torch forms p with a matrix product) and the largest differences
elsewhere.  No bar is asserted.

    python tools/tsdf_time.py [--out profiles/tsdf_time.json] [--resolution 256]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from depth_corr_time import interleaved

REPEATS = 5
W, H, FX = 1280, 720, 900.0
RADIUS, SIDE = 0.2, 0.6


def look_at(pos, up=(0.0, 0.0, 1.0)):
    pos, up = np.asarray(pos, dtype=np.float64), np.asarray(up, dtype=np.float64)
    z = -pos / np.linalg.norm(pos)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, :3] = np.stack([x, np.cross(z, x), z])
    m[:3, 3] = -m[:3, :3] @ pos
    return m


def make_views(dev, n=8):
    """Cameras on an orbit of radius 1 m, analytic camera-space z of the sphere (0 where missed), weights, colours."""
    from touch_gs_amd import Camera
    g = torch.Generator().manual_seed(0)
    cams, depths, weights, rgbs = [], [], [], []
    us, vs = torch.meshgrid(torch.arange(W, dtype=torch.float64) + 0.5, torch.arange(H, dtype=torch.float64) + 0.5, indexing="xy")
    for k in range(n):
        a = 2 * np.pi * k / n
        m = look_at((np.cos(a), np.sin(a), 0.4))
        cam = Camera(m, FX, FX, W / 2, H / 2, W, H)
        d = torch.stack([(us - cam.cx) / FX, (vs - cam.cy) / FX, torch.ones_like(us)], -1)
        cc = torch.from_numpy(m[:3, 3].copy())                     # the sphere's centre (the world origin) in the camera
        b, dd = d @ cc, (d * d).sum(-1)
        disc = b * b - dd * (cc @ cc - RADIUS * RADIUS)
        z = torch.where(disc > 0, (b - disc.clamp(min=0).sqrt()) / dd, torch.zeros_like(b))
        cams.append(cam)
        depths.append(z.float().to(dev).contiguous())
        weights.append((0.1 + torch.rand(H, W, generator=g)).to(dev).contiguous())
        rgbs.append(torch.rand(H, W, 3, generator=g).to(dev).contiguous())
    return cams, depths, weights, rgbs


def torch_integrate(S, Wt, Cc, centres, origin, vox, trunc, cam, depth, weight, rgb):
    """The update of include/tgs.h for one view in plain torch, in place."""
    vm = np.asarray(cam.viewmat, dtype=np.float64)
    R = torch.tensor(vm[:3, :3], dtype=torch.float32, device=S.device)
    t = torch.tensor(vm[:3, :3] @ origin + vm[:3, 3], dtype=torch.float32, device=S.device)
    p = centres @ R.T + t
    z = p[:, 2]
    fu = torch.floor(cam.fx * p[:, 0] / z + cam.cx + (0.5 - cam.pix_center))
    fv = torch.floor(cam.fy * p[:, 1] / z + cam.cy + (0.5 - cam.pix_center))
    ok = (z > cam.near) & (fu >= 0) & (fu < cam.W) & (fv >= 0) & (fv < cam.H)
    pix = torch.where(ok, fv * cam.W + fu, torch.zeros_like(fu)).long()
    D = depth.view(-1)[pix]
    w = weight.view(-1)[pix]
    sdf = D - z
    ok &= torch.isfinite(D) & (D > 0) & torch.isfinite(w) & (w > 0) & ~(sdf < -trunc)
    w = torch.where(ok, w, torch.zeros_like(w))
    S += w * torch.clamp(sdf / trunc, max=1.0).nan_to_num(0.0, 0.0, 0.0)
    Wt += w
    if Cc is not None:
        Cc += w[:, None] * rgb.view(-1, 3)[pix]


def copy_ceiling(dev):
    a = torch.empty(1024 * 1024 * 1024 // 4, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(5):
        b.copy_(a)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        b.copy_(a)
    e.record()
    torch.cuda.synchronize()
    return 2 * a.numel() * 4 / (s.elapsed_time(e) / 20 * 1e-3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "tsdf_time.json"))
    ap.add_argument("--resolution", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tsdf_time.py needs the GPU: there is nothing to time without it")
    from touch_gs_amd.tsdf import TsdfVolume
    dev = torch.device("cuda:0")
    n = a.resolution
    vox = SIDE / n
    origin = np.full(3, -SIDE / 2)
    ceiling = copy_ceiling(dev)
    torch.cuda.empty_cache()
    cams, depths, weights, rgbs = make_views(dev)
    vols = {c: TsdfVolume(origin, vox, (n, n, n), 4 * vox, dev, color=c) for c in (True, False)}
    V = vols[True].num_voxels
    lin = torch.arange(V, device=dev)
    centres = torch.stack([((lin % n).float() + 0.5) * vox, (((lin // n) % n).float() + 0.5) * vox,
                           ((lin // (n * n)).float() + 0.5) * vox], -1).contiguous()
    tstate = {c: (torch.zeros(V, device=dev), torch.zeros(V, device=dev), torch.zeros(V, 3, device=dev) if c else None)
              for c in (True, False)}

    # agreement first: the same eight views through both, from zero
    vols[True].integrate(cams, depths, weights, rgbs)
    for k in range(8):
        torch_integrate(*tstate[True], centres, origin, vox, 4 * vox, cams[k], depths[k], weights[k], rgbs[k])
    torch.cuda.synchronize()
    Wt = vols[True].Wt
    scale = float(Wt.max())
    # a voxel-view decided differently (a pixel edge, the -trunc cut: torch forms p with a matrix product) moves Wt by a weight
    other = (Wt - tstate[True][1]).abs() > 1e-4 * Wt.clamp(min=1.0)
    same = ~other
    agree = dict(voxels_decided_differently=int(other.sum()), share_decided_differently=round(float(other.float().mean()), 6),
                 max_abs_S_elsewhere=float((vols[True].S - tstate[True][0])[same].abs().max()),
                 max_abs_Wt_elsewhere=float((Wt - tstate[True][1])[same].abs().max()),
                 updated_voxels=int((Wt > 0).sum()), updated_share=round(float((Wt > 0).float().mean()), 4),
                 decisions_differ=int(((Wt > 0) != (tstate[True][1] > 0)).sum()),
                 max_abs_S=float((vols[True].S - tstate[True][0]).abs().max()), max_abs_Wt=float((Wt - tstate[True][1]).abs().max()),
                 max_abs_C=float((vols[True].C - tstate[True][2]).abs().max()), largest_Wt=scale)

    def hip(color, per_launch):
        v = vols[color]

        def run():
            for i0 in range(0, 8, per_launch):
                s = slice(i0, i0 + per_launch)
                v.integrate(cams[s], depths[s], weights[s], rgbs[s] if color else None)
            return 8 // per_launch                                      # launches
        return run

    def tor(color):
        def run():
            torch_integrate(*tstate[color], centres, origin, vox, 4 * vox, cams[0], depths[0], weights[0], rgbs[0])
            return 1
        return run

    def extract():
        vols[True].extract_local(0.5)
        return 1

    variants = {"hip_1view": hip(True, 1), "hip_8views": hip(True, 8), "hip_1view_nocolor": hip(False, 1),
                "hip_8views_nocolor": hip(False, 8), "torch_1view": tor(True), "torch_1view_nocolor": tor(False), "extract": extract}
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    bytes_per_launch = {"hip_1view": 40 * V, "hip_8views": 40 * V, "hip_1view_nocolor": 16 * V, "hip_8views_nocolor": 16 * V}
    bound = {k: b / ceiling * 1e6 for k, b in bytes_per_launch.items()}
    crossings = int(vols[True].extract_local(0.5)["edge_id"].numel())
    out = dict(tool="tools/tsdf_time.py", device=torch.cuda.get_device_name(0),
               method=f"device events around each variant's calls, {REPEATS} repeats interleaved over the variants after a warm-up; "
                      "medians of the repeats, all repeats kept; microseconds PER LAUNCH (hip_*), per view (torch_*), per "
                      "extraction (count + cumsum + host read + points)",
               grid=dict(dims=[n, n, n], voxels=V, voxel_size=vox, trunc=4 * vox), image=[W, H], views=8,
               copy_ceiling_TBps=round(ceiling / 1e12, 3), agreement_hip_vs_torch=agree, crossings=crossings,
               us_median={k: round(v, 1) for k, v in med.items()}, us_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               streaming_bound_us={k: round(v, 1) for k, v in bound.items()},
               ratio_to_streaming_bound={k: round(med[k] / bound[k], 3) for k in bound},
               us_per_view=dict(hip_1view=round(med["hip_1view"], 1), hip_8views=round(med["hip_8views"] / 8, 1),
                                      hip_1view_nocolor=round(med["hip_1view_nocolor"], 1),
                                      hip_8views_nocolor=round(med["hip_8views_nocolor"] / 8, 1),
                                      torch_1view=round(med["torch_1view"], 1), torch_1view_nocolor=round(med["torch_1view_nocolor"], 1)),
               torch_over_hip=dict(one_view=round(med["torch_1view"] / med["hip_1view"], 2),
                                   one_view_nocolor=round(med["torch_1view_nocolor"] / med["hip_1view_nocolor"], 2),
                                   per_view_against_8_per_launch=round(med["torch_1view"] / (med["hip_8views"] / 8), 2),
                                   per_view_against_8_per_launch_nocolor=round(med["torch_1view_nocolor"] / (med["hip_8views_nocolor"] / 8), 2)))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
