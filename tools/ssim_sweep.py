"""SSIM forward + backward alone at 1080p, 720p, 800x800 and 2160p: the two kernels (form 0), the one-pass kernel on the
two-kernel grid (form 2, what the default picks from 1080p on) and on its own 54-column grid (form 1), alternated in ONE
process through tgs_set_ssim_form so that clock and box state are shared.
   python tools/ssim_sweep.py            (median and minimum of 6 x 15 calls per form, HIP events, us)"""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from touch_gs_amd import ops, _lib
lib = _lib.load()
dev = torch.device("cuda:0")
for W, H in ((1920, 1080), (1280, 720), (800, 800), (3840, 2160)):
    a = torch.rand(H, W, 3, device=dev); b = torch.rand(H, W, 3, device=dev)
    ts = {0: [], 2: [], 1: []}
    for rnd in range(6):
        for f in ts:
            lib.tgs_set_ssim_form(f)
            for _ in range(3):
                ops.ssim_fwd_bwd(a, b, -0.2 / (3 * H * W), reduce=False)
            for _ in range(15):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); ops.ssim_fwd_bwd(a, b, -0.2 / (3 * H * W), reduce=False); e1.record()
                torch.cuda.synchronize(); ts[f].append(e0.elapsed_time(e1) * 1e3)
    print(f"{W}x{H}", json.dumps({f"form{f}": dict(median_us=round(sorted(v)[len(v) // 2], 1), min_us=round(min(v), 1))
                                   for f, v in ts.items()}), flush=True)
