"""Developer tool: what does the triangle-mesh extraction cost (csrc/tsdf.hip: tgs_tsdf_mesh_count, tgs_tsdf_mesh_emit; DESIGN
5.1l)?

The 256^3 sphere grid of tools/tsdf_time.py after its eight views.  Timed with device events, in one process and interleaved:

    count        tgs_tsdf_mesh_count: three launches (flags, ntri, vmask)
    prefix       the popcount lookup, the two torch.cumsum, the exclusive offsets and the ONE host read of the two totals
    emit         tgs_tsdf_mesh_emit into preallocated outputs
    mesh         TsdfVolume.extract_mesh_local: all of the above plus its allocations
    points       TsdfVolume.extract_local: the existing point extraction (count + cumsum + host read + points)

5 repeats after a warm-up, medians, all repeats kept.  The streaming bound of a pass is the bytes it reads and writes as
built / the copy ceiling (a 1 GiB device-to-device copy, read + write bytes per second, as tools/tsdf_time.py measures it):

    count   S, Wt in (8 B), flags out and in twice (3 B), ntri out and in (2 B), vmask out (1 B)         = 14 B per voxel
    emit    vmask, flags in (2 B per voxel; the corner bytes of a cell come from the same lines)
            + 44 B per vertex (point, normal, colour, key) + 12 B per face out; the S / Wt / C / offset reads at the surface
            voxels are not counted
No bar is asserted.

    python tools/tsdf_mesh_time.py [--out profiles/tsdf_mesh_time.json] [--resolution 256]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from depth_corr_time import interleaved
from tsdf_time import SIDE, copy_ceiling, make_views

REPEATS = 5
W_MIN = 0.5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "tsdf_mesh_time.json"))
    ap.add_argument("--resolution", type=int, default=256)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/tsdf_mesh_time.py needs the GPU: there is nothing to time without it")
    from touch_gs_amd import _lib
    from touch_gs_amd.tsdf import TsdfVolume, mesh_stats
    lib = _lib.load()
    dev = torch.device("cuda:0")
    n = a.resolution
    vox = SIDE / n
    ceiling = copy_ceiling(dev)
    torch.cuda.empty_cache()
    vol = TsdfVolume(np.full(3, -SIDE / 2), vox, (n, n, n), 4 * vox, dev, color=True)
    vol.integrate(*make_views(dev))
    V = vol.num_voxels
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    grid = (n, n, n, C.c_float(vox), _lib.ptr(vol.S), _lib.ptr(vol.Wt))
    vmask, ntri, flags = (torch.empty(V, dtype=torch.uint8, device=dev) for _ in range(3))
    popcount = torch.tensor([bin(m).count("1") for m in range(256)], dtype=torch.int64, device=dev)
    st = {}

    def count():
        _lib.check(lib.tgs_tsdf_mesh_count(*grid, C.c_float(W_MIN), _lib.ptr(vmask), _lib.ptr(ntri), _lib.ptr(flags), stream))
        return 1

    def prefix():
        nvert = popcount[vmask.long()]
        v_incl, t_incl = torch.cumsum(nvert, 0, dtype=torch.int64), torch.cumsum(ntri, 0, dtype=torch.int64)
        st["voff"], st["toff"] = (v_incl - nvert).contiguous(), (t_incl - ntri).contiguous()
        st["n_v"], st["n_f"] = (int(x) for x in torch.stack([v_incl[-1], t_incl[-1]]).tolist())
        return 1

    count()
    prefix()
    n_v, n_f = st["n_v"], st["n_f"]
    points, normals, colors = (torch.empty(n_v, 3, dtype=torch.float32, device=dev) for _ in range(3))
    key = torch.empty(n_v, dtype=torch.int64, device=dev)
    faces = torch.empty(n_f, 3, dtype=torch.int32, device=dev)

    def emit():
        _lib.check(lib.tgs_tsdf_mesh_emit(*grid, _lib.ptr(vol.C), C.c_float(W_MIN), _lib.ptr(flags), _lib.ptr(vmask), _lib.ptr(st["voff"]),
                                          _lib.ptr(st["toff"]), _lib.ptr(points), _lib.ptr(normals), _lib.ptr(colors), _lib.ptr(key),
                                          _lib.ptr(faces), stream))
        return 1

    def mesh():
        vol.extract_mesh_local(W_MIN)
        return 1

    def pts():
        vol.extract_local(W_MIN)
        return 1

    variants = {"count": count, "prefix": prefix, "emit": emit, "mesh": mesh, "points": pts}
    times = interleaved(variants, REPEATS, lambda f: f())
    med = {k: statistics.median(v) for k, v in times.items()}
    loc = vol.extract_mesh_local(W_MIN)
    same = all(torch.equal(x, y) for x, y in ((loc["points"], points), (loc["normals"], normals), (loc["colors"], colors),
                                                (loc["edge_key"], key), (loc["faces"], faces)))
    crossings = int(vol.extract_local(W_MIN)["edge_id"].numel())
    stats = mesh_stats(loc["points"].cpu().numpy().astype(np.float64), loc["faces"].cpu().numpy())
    nbytes = dict(count=14 * V, emit=2 * V + 44 * n_v + 12 * n_f)
    bound = {k: b / ceiling * 1e6 for k, b in nbytes.items()}
    out = dict(tool="tools/tsdf_mesh_time.py", device=torch.cuda.get_device_name(0),
               method=f"device events around each variant's calls, {REPEATS} repeats interleaved over the variants after a warm-up; "
                      "medians of the repeats, all repeats kept; microseconds per call",
               grid=dict(dims=[n, n, n], voxels=V, voxel_size=vox, trunc=4 * vox), views=8, w_min=W_MIN,
               copy_ceiling_TBps=round(ceiling / 1e12, 3), vertices=n_v, faces=n_f, crossings_of_the_point_extraction=crossings,
               mesh_stats=stats, phases_equal_the_public_path=bool(same),
               us_median={k: round(v, 1) for k, v in med.items()}, us_all={k: [round(x, 1) for x in v] for k, v in times.items()},
               bytes_as_built=nbytes, streaming_bound_us={k: round(v, 1) for k, v in bound.items()},
               ratio_to_streaming_bound={k: round(med[k] / bound[k], 3) for k in bound},
               mesh_over_points=round(med["mesh"] / med["points"], 3))
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
