"""The one-pass SSIM kernel (csrc/imgloss.hip: k_ssim_fused, adjoint rows in a two-row LDS ring) against the two-kernel path
run in the same process (tgs_set_ssim_form), bit for bit, and against the fp64 reference of tests/ssim_ref.py under the
bounds of tests/test_gpu_ssim_oracle.py (4 sum(u) for sums of the map, 4x the fp32 floor for the gradient; helpers and
bounds are imported from there, nothing is restated).

Forms (include/tgs.h): 0 = k_ssim_fwd + k_ssim_bwd, 2 = one pass on the grid of form 0 -- 64-column strips, the forward
launch's segments --, which is what the default picks from 1080p on; 1 = one pass on 54-column strips (TGS_SSIM_FUSED=1).
Form 2 must give the bits of form 0 in v_img AND in every entry of block_partials (so in any sum of them); form 1 gives
the bits of v_img and sums that differ by fp32 summation order, as tests/test_gpu_parity.py already allows.

Sizes: the smallest at which the strip logic can go wrong.  Small images take 12-row segments (2 blocks), so 11 / 12 / 13
rows are one segment -1 / 0 / +1; a smaller n_partials escalates to the 23- and 34-row segments of the large sizes.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import test_gpu_ssim_oracle as T

pytestmark = pytest.mark.gpu

TWO_KERNELS, OWN_GRID, ONE_PASS = 0, 1, 2
REGIMES = ("uniform", "white_vs_grey")         # noise, flat constant

# (W, H, n_partials or None = one per 16x16 tile)
SIZES = [(1, 1, None), (11, 11, None),
         (63, 12, None), (64, 12, None), (65, 12, None),       # one 64-column strip -1 / 0 / +1, one 12-row segment
         (129, 13, None),                                      # two strips + 1 column, one segment + 1 row
         (64, 11, None), (64, 13, None),                       # one segment -1 / +1 row
         (53, 14, None), (55, 13, None), (109, 12, None),      # the 54-column strips of form 1: -1 / +1, two + 1
         (129, 68, 6),                                         # 3 strips x 2 segments of 34 rows (4 blocks, as at 1080p)
         (70, 47, 6)]                                          # 23-row segments (3 blocks): 2 full + 1 row
RAGGED = (637, 395, None)                                      # 10 strips (last 61 columns), 33 segments (last 11 rows)
# the ragged size runs on noise only: its fp64 reference is the slow part of the file
CASES = [(r, *s) for s in SIZES for r in REGIMES] + [("uniform", *RAGGED)]


@pytest.fixture
def form(dev):
    """-> set(form); the process-wide setting is put back afterwards."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    before = lib.tgs_set_ssim_form(-1)
    yield lib.tgs_set_ssim_form
    lib.tgs_set_ssim_form(before)


def run(dev, c, n_p=None, rows=None, grad=True):
    """One call -> (block_partials Buf, v_img Buf or None, scratch Buf or None); sentinels checked by T.call."""
    img, gt = T.on_dev(c, dev)
    n_def = T.default_partials(c.W, c.H)
    bp = T.Buf(n_def, dev)
    v, sc = (T.Buf(3 * c.H * c.W, dev), T.Buf(9 * c.H * c.W, dev)) if grad else (None, None)
    if rows is None and n_p is None:
        assert T.call(c.W, c.H, img, gt, c.weight, bp, v, sc) == 0
    else:
        assert T.call(c.W, c.H, img, gt, c.weight, bp, v, sc, rows=rows or (0, c.H, 0, c.H), n_partials=n_p) == 0
    return bp, v, sc


@pytest.mark.parametrize("regime,W,H,n_p", CASES)
def test_one_pass_bits(dev, form, regime, W, H, n_p):
    c = T.case(regime, W, H)
    n_eff = T.default_partials(W, H) if n_p is None else n_p
    assert form(TWO_KERNELS) == TWO_KERNELS
    bp0, v0, sc0 = run(dev, c, n_p)
    assert not sc0.untouched(), "form 0 did not fill the adjoint planes"
    nblk, nwg = T.two_kernel_segments(W, H, n_eff)
    T.assert_partials(bp0, n_eff, nwg, counted=regime == "uniform")

    assert form(ONE_PASS) == ONE_PASS
    bp2, v2, sc2 = run(dev, c, n_p)
    assert sc2.untouched(), "the one-pass kernel did not run (scratch was written)"
    assert torch.equal(v2.bits, v0.bits), "v_img differs from the two-kernel path"
    assert torch.equal(bp2.bits, bp0.bits), "block_partials differ from the two-kernel path"
    assert T.partial_sum(bp2, n_eff) == T.partial_sum(bp0, n_eff)
    assert float(bp2.body(n_eff).sum()) == float(bp0.body(n_eff).sum())          # the fp32 sum the train step takes

    assert form(OWN_GRID) == OWN_GRID
    bp1, v1, sc1 = run(dev, c, n_p)
    assert sc1.untouched()
    assert torch.equal(v1.bits, v0.bits), "v_img of the 54-column form differs"
    T.assert_partials(bp1, n_eff, T.fused_segments(W, H, n_eff)[1], counted=regime == "uniform")

    g, s, s1 = T.grad_figures(c, v2.body()), T.sum_figures(c, T.partial_sum(bp2, n_eff)), T.sum_figures(c, T.partial_sum(bp1, n_eff))
    print(json.dumps(dict(test="one_pass_bits", regime=regime, W=W, H=H, nblk=nblk, nwg=nwg, grad=g, sum=s, sum_own_grid=s1)))
    T.assert_sum(c, s, whole_image=True)
    T.assert_sum(c, s1, whole_image=True)
    T.assert_grad(c, g)


# y0, y1, count_y0, count_y1 at (100, 70): split at interior rows (the bands partition the image as ops.band_rows makes
# them: overlapping forward rows, disjoint count ranges), a count strictly inside, an empty count, one-row bands at the edges
BANDS = [(0, 32, 0, 16), (16, 64, 16, 48), (48, 70, 48, 70), (0, 37, 0, 37), (37, 70, 37, 70),
         (10, 50, 20, 30), (10, 50, 30, 30), (0, 1, 0, 1), (69, 70, 69, 70), (3, 9, 4, 8)]


@pytest.mark.parametrize("regime", REGIMES)
def test_one_pass_bands(dev, form, regime):
    """Every band: v_img rows inside = the two-kernel path's band = the whole image, rows outside untouched, the band's
    block_partials bit-identical to the two-kernel path's, its sum against the reference.  The empty band and the
    forward-only call run the kernels they always ran (k_ssim_zero_partials, k_ssim_fwd)."""
    W, H = 100, 70
    c = T.case(regime, W, H)
    n_p, row = T.default_partials(W, H), 3 * W
    form(TWO_KERNELS)
    _, v_whole, _ = run(dev, c)
    ref_bands = [run(dev, c, rows=b) for b in BANDS]
    ref_fwd = [run(dev, c, rows=b, grad=False) for b in BANDS]
    ref_empty = run(dev, c, rows=(20, 20, 20, 20))
    for f in (ONE_PASS, OWN_GRID):
        assert form(f) == f
        _, vw, _ = run(dev, c)
        assert torch.equal(vw.bits, v_whole.bits)
        worst = 0.0
        for b, (bp0, v0, _), (bpf0, _, _) in zip(BANDS, ref_bands, ref_fwd):
            y0, y1, c0, c1 = b
            bp, v, sc = run(dev, c, rows=b)
            tag = (regime, f, b)
            assert sc.untouched(), tag
            assert v.untouched(0, y0 * row) and v.untouched(y1 * row), ("v_img written outside the band", tag)
            assert torch.equal(v.bits, v0.bits), ("band differs from the two-kernel path", tag)
            assert torch.equal(v.bits[y0 * row:y1 * row], v_whole.bits[y0 * row:y1 * row]), ("band differs from the whole image", tag)
            assert bool(torch.isfinite(bp.body()).all()) and bp.untouched(n_p), tag
            if f == ONE_PASS:
                assert torch.equal(bp.bits, bp0.bits), ("band sums differ from the two-kernel path", tag)
            if c0 == c1:
                assert bool((bp.bits[:n_p] == 0).all()), ("empty count range: partials not all +0", tag)
            s = T.sum_figures(c, T.partial_sum(bp), c0, c1)
            worst = max(worst, s["over_sum_u"])
            assert s["err"] <= T.SUM_UNITS * s["sum_u"], (tag, s)
            bpf, _, _ = run(dev, c, rows=b, grad=False)                      # forward only: the same kernel in every form
            assert torch.equal(bpf.bits, bpf0.bits), ("forward-only sums differ", tag)
        bp, v, sc = run(dev, c, rows=(20, 20, 20, 20))                         # an empty band
        assert v.untouched() and torch.equal(bp.bits, ref_empty[0].bits) and bool((bp.bits[:n_p] == 0).all())
        print(json.dumps(dict(test="one_pass_bands", regime=regime, form=f, worst_over_sum_u=worst)))


def test_default_picks_by_size(dev, form):
    """Form 3 (the default): below 1080p the two kernels (scratch is written), from 1080p on one pass (scratch is not) --
    and both give the bits of the other form at that size.  No reference here: the bits are pinned above."""
    for (W, H), one_pass in (((1280, 720), False), ((1920, 1080), True)):
        g = torch.Generator().manual_seed(W)
        img, gt = torch.rand(H, W, 3, generator=g).to(dev), torch.rand(H, W, 3, generator=g).to(dev)
        out = {}
        for f in (3, ONE_PASS if not one_pass else TWO_KERNELS):
            assert form(f) == f
            bp, v, sc = T.Buf(T.default_partials(W, H), dev), T.Buf(3 * H * W, dev), T.Buf(9 * H * W, dev)
            assert T.call(W, H, img, gt, -0.2 / (3 * H * W), bp, v, sc) == 0
            out[f] = (bp.bits.clone(), v.bits.clone(), sc.untouched())
        other = ONE_PASS if not one_pass else TWO_KERNELS
        assert out[3][2] == one_pass and out[other][2] == (not one_pass), (W, H)
        assert torch.equal(out[3][0], out[other][0]) and torch.equal(out[3][1], out[other][1]), (W, H)


_WORKER = r'''
import sys, types, torch
sys.path.insert(0, sys.argv[1])
from tests import ssim_ref as R, test_gpu_ssim_oracle as T
dev = torch.device("cuda:0")
out = {}
for regime in ("uniform", "white_vs_grey"):
    for W, H in ((129, 37), (109, 27)):
        img, gt = R.inputs(regime, W, H)
        c = types.SimpleNamespace(W=W, H=H, img=img, gt=gt, weight=-0.2 / (3 * H * W))
        bp, v, sc = T.whole(dev, c)
        k = f"{regime}/{W}x{H}"
        out[k + "/v"], out[k + "/bp"], out[k + "/scratch_untouched"] = v.bits[:v.n].cpu(), bp.bits[:bp.n].cpu(), sc.untouched()
torch.save(out, sys.argv[2])
'''


def test_override_reaches_both_kernels(dev, tmp_path):
    """TGS_SSIM_FUSED=0 and =1, each in its own process (the variable is read once): the same v_img bits, scratch written
    by the first and untouched by the second, sums within the summation-order bound (a thread adds at most 37 values, the
    wave reduction 6 more, the workgroup 3, each rounding at most 2^-24 of the running sum; the strips of form 1 are 54
    columns wide, so its workgroup sums are other sums)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for fused in ("0", "1"):
        f = str(tmp_path / f"ssim_{fused}.pt")
        env = {k: v for k, v in os.environ.items() if k not in ("TGS_SSIM_FUSED", "TGS_SSIM_NBLK")}
        env["TGS_SSIM_FUSED"] = fused
        r = subprocess.run([sys.executable, "-c", _WORKER, root, f], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (fused, r.returncode, r.stderr[-2000:])
        res[fused] = torch.load(f)
    for k in [k for k in res["0"] if k.endswith("/v")]:
        base = k[:-2]
        assert res["0"][base + "/scratch_untouched"] is False and res["1"][base + "/scratch_untouched"] is True, base
        assert torch.equal(res["0"][k], res["1"][k]), base
        s0, s1 = (float(res[f][base + "/bp"].view(torch.float32).double().sum()) for f in ("0", "1"))
        regime, size = base.split("/")
        sabs = float(T.case(regime, *map(int, size.split("x"))).ref.map.abs().sum())
        assert abs(s0 - s1) <= 2 * (37 + 9) * 2.0 ** -24 * sabs, (base, s0, s1)
