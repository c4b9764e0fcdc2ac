"""K10 (csrc/imgloss.hip: k_ssim_fwd / k_ssim_bwd / k_ssim_fused) against the fp64 reference of tests/ssim_ref.py: input
regimes from noise to constant images, every edge of the strip / segment / band geometry, every segment length, the map
row by row, the bands of the pipelined step, the forward-only (eval) path and the code paths the environment selects.

The library is called directly (touch_gs_amd._lib) so that the buffers can be prepared: block_partials and v_img are
prefilled with NaN, and v_img, scratch and block_partials are 64 floats longer than the contract asks, with a sentinel
in the tail that must be bit-unchanged after every call.

Bounds (none of them fitted to a kernel; tests/ssim_ref.py defines the unit, tests/test_cpu_ssim_ref.py measures the floor):
  sums of the map      |sum_hip - sum_ref| <= 4 sum(u) over the counted pixels (image, band or row), u = the conditioning
                       unit of the map; on ``uniform`` and ``smooth`` also the older |d mean| < 1e-5
  gradient             max|v_hip - v_ref| <= 4 F_max and ||v_hip - v_ref||_2 <= 4 F_l2, where F = the larger error of the
                       two fp32 evaluations of the reference on the same input (computed at run time); on ``uniform`` and
                       ``smooth`` also the older max < 1e-4 max|v_ref|
  bit identity         bands against the whole-image call, every segment length against the first, untouched memory
                       against its prefill

Measured on an MI355X (the figures every test prints as JSON; the bounds are 4 in the first three columns):

  a. regimes, worst of (100, 70) and (130, 40)
     regime          max err / F_max   l2 err / F_l2   |d sum| / sum(u)   |d mean|
     uniform              0.37             0.37            0.006           8.0e-9
     smooth               0.28             0.32            0.004           4.6e-8
     converged            0.42             0.36            0.006           2.9e-7
     flat_bright          0.29             0.27            0.004           1.4e-6
     white_vs_grey        0.50             0.34            0.14            5.5e-5   (systematic: every pixel rounds alike)
     white                1.00             1.01            0               5.8e-9
     black                0                0               0.20            1.1e-7   (map = C1 C2 rcp(C1) rcp(C2), not 1)
     identical            1.34             1.19            0               0
     mixed                0.38             0.19            0.13            2.3e-5   (systematic, the flat half)
     F_max / |weight| runs from 1.0e-5 (uniform) over 1.3e-3 (white_vs_grey) to 9.8e-3 (mixed): on flat inputs the
     gradient's fp32 error is a thousand times the one on noise, in the kernel and in both CPU evaluations alike.
  b. edge geometry   max err / F_max 0.29 .. 0.66, |d sum| / sum(u) <= 0.067; (1, 1): 3.07 -- three values, so the
                     floor itself is a sample of three
  c. segments        2, 3, 4, 5, 6, 9, 16 blocks: v_img identical, sums within 0.003 of the summation-order bound
  d. per row         worst row 0.065 sum(u) (uniform), 0.27 sum(u) (mixed); the same both ways
  e. bands           worst band 0.032 sum(u) (uniform), 0.17 sum(u) (mixed)
  f. env paths       all four: max err / F_max 1.00, l2 err / F_l2 1.16 (identical), sums <= 0.30 sum(u), bands <= 0.28 sum(u)
  g. eval path       0.018 sum(u) (uniform), 0.13 sum(u) (mixed)
"""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from tests import ssim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
NAN_BITS = 0x7FC00000            # the prefill
SENT_BITS = 0x4B3C614E           # the tail (12345678.0f)
SUM_UNITS, GRAD_FLOORS = 4.0, 4.0


# ---------------------------------------------------------------------------------------------
# buffers, calls, references
# ---------------------------------------------------------------------------------------------
class Buf:
    """``n`` floats of NaN followed by PAD floats of the sentinel."""

    def __init__(self, n, dev):
        self.n = n
        self.bits = torch.full((n + PAD,), NAN_BITS, dtype=torch.int32, device=dev)
        self.bits[n:] = SENT_BITS
        self.f = self.bits.view(torch.float32)

    def tail_ok(self):
        return bool((self.bits[self.n:] == SENT_BITS).all())

    def untouched(self, lo=0, hi=None):
        return bool((self.bits[lo:self.n if hi is None else hi] == NAN_BITS).all())

    def body(self, n=None):
        return self.f[:self.n if n is None else n]


def default_partials(W, H):
    return ((W + 15) // 16) * ((H + 15) // 16)


def call(W, H, img, gt, weight, bp, v=None, scratch=None, rows=None, n_partials=None):
    """tgs_ssim_fwd_bwd (rows None) or tgs_ssim_fwd_bwd_rows -> status; every sentinel checked."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    p = lambda b: None if b is None else b.f.data_ptr()
    if rows is None:
        assert n_partials is None
        rc = lib.tgs_ssim_fwd_bwd(W, H, img.data_ptr(), gt.data_ptr(), C.c_float(weight), p(bp), p(v), p(scratch), None)
    else:
        n_partials = default_partials(W, H) if n_partials is None else n_partials
        rc = lib.tgs_ssim_fwd_bwd_rows(W, H, img.data_ptr(), gt.data_ptr(), C.c_float(weight), p(bp), n_partials, p(v), p(scratch),
                                       *rows, None)
    torch.cuda.synchronize()
    for name, b in (("block_partials", bp), ("v_img", v), ("scratch", scratch)):
        assert b is None or b.tail_ok(), f"{name}: the sentinel behind the buffer was overwritten"
    return rc


@functools.lru_cache(maxsize=None)
def case(regime, W, H):
    """Inputs, fp64 reference and fp32 floor of one (regime, size): computed once, shared, never modified."""
    img, gt = R.inputs(regime, W, H)
    weight = -0.2 / (3 * H * W)
    ref = R.ssim_ref(img, gt, weight)
    fl = R.fp32_floor(img, gt, weight, ref)
    return types.SimpleNamespace(regime=regime, W=W, H=H, img=img, gt=gt, weight=weight, ref=ref, f_max=fl.f_max, f_l2=fl.f_l2)


def on_dev(c, dev):
    return c.img.to(dev).contiguous(), c.gt.to(dev).contiguous()


def whole(dev, c):
    """The whole-image gradient call -> (block_partials Buf, v_img Buf, scratch Buf)."""
    img, gt = on_dev(c, dev)
    bp, v, sc = Buf(default_partials(c.W, c.H), dev), Buf(3 * c.H * c.W, dev), Buf(9 * c.H * c.W, dev)
    assert call(c.W, c.H, img, gt, c.weight, bp, v, sc) == 0
    return bp, v, sc


def ratio(err, unit):
    return 0.0 if err == 0 else (err / unit if unit > 0 else float("inf"))


def grad_figures(c, v_hip):
    """v_hip [H,W,3] (any device) -> figures of the gradient comparison."""
    d = v_hip.detach().cpu().double().reshape(c.H, c.W, 3) - c.ref.v_img
    e_max, e_l2 = float(d.abs().max()), float(d.norm())
    return dict(e_max=e_max, e_l2=e_l2, max_over_F=ratio(e_max, c.f_max), l2_over_F=ratio(e_l2, c.f_l2),
                max_over_vmax=ratio(e_max, float(c.ref.v_img.abs().max())))


def assert_grad(c, fig):
    assert fig["e_max"] <= GRAD_FLOORS * c.f_max, (c.regime, c.W, c.H, fig, c.f_max)
    assert fig["e_l2"] <= GRAD_FLOORS * c.f_l2, (c.regime, c.W, c.H, fig, c.f_l2)
    if c.regime in ("uniform", "smooth"):
        assert fig["e_max"] < 1e-4 * float(c.ref.v_img.abs().max()), (c.regime, c.W, c.H, fig)


def sum_figures(c, s_hip, c0=0, c1=None):
    c1 = c.H if c1 is None else c1
    s_ref, s_u = float(R.row_sums(c.ref.map, c0, c1).sum()), float(R.row_sums(c.ref.unit, c0, c1).sum())
    err = abs(float(s_hip) - s_ref)
    return dict(err=err, sum_u=s_u, over_sum_u=ratio(err, s_u), d_mean=err / (3.0 * c.W * max(c1 - c0, 1)))


def assert_sum(c, fig, whole_image=False):
    assert fig["err"] <= SUM_UNITS * fig["sum_u"], (c.regime, c.W, c.H, fig)
    if whole_image and c.regime in ("uniform", "smooth"):
        assert fig["d_mean"] < 1e-5, (c.regime, c.W, c.H, fig)


def partial_sum(bp, n=None):
    return float(bp.body(n).double().sum())


def two_kernel_segments(W, rows, n_partials, env_nblk=0):
    """ssim_impl's choice for the two-kernel path -> (blocks per segment, workgroups of the forward launch)."""
    sx = (W + 63) // 64
    wgs = lambda nb: sx * -(-rows // (11 * nb - 10))
    nblk = 4
    while nblk > 2 and wgs(nblk) < 3 * 256:
        nblk -= 1
    if env_nblk:
        nblk = max(2, min(16, env_nblk))
    while nblk < 16 and wgs(nblk) > n_partials:
        nblk += 1
    return nblk, wgs(nblk)


def fused_segments(W, rows, n_partials, env_nblk=0):
    """The same for the one-pass kernel (54 output columns, 11 nblk - 20 rows)."""
    fx = (W + 53) // 54
    wgs = lambda nb: fx * -(-rows // (11 * nb - 20))
    nblk = 7
    while nblk > 3 and wgs(nblk) < 600:
        nblk -= 1
    if env_nblk:
        nblk = max(3, min(16, env_nblk))
    while nblk < 16 and wgs(nblk) > n_partials:
        nblk += 1
    return nblk, wgs(nblk)


def assert_partials(bp, n_partials, nwg, counted=True):
    """First entries = workgroup sums (finite; on a counted noise image none of them is 0), the rest exactly zero, and
    nothing behind n_partials touched."""
    body = bp.body(n_partials)
    assert bool(torch.isfinite(body).all()), "block_partials: an entry in [0, n_partials) was not written"
    assert nwg <= n_partials
    assert bool((bp.bits[nwg:n_partials] == 0).all()), "block_partials: entries behind the workgroup sums are not +0"
    if counted:
        assert bool((body[:nwg] != 0).all()), "fewer workgroup sums than the launch geometry says"
    assert bp.untouched(n_partials), "block_partials written behind n_partials"


# ---------------------------------------------------------------------------------------------
# a. regimes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(100, 70), (130, 40)])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_regimes(dev, regime, W, H):
    """All nine regimes, whole-image call: the sum in units of sum(u), the gradient in units of the fp32 floor.
    (130, 40): three strips, the last two columns wide, four 12-row segments."""
    c = case(regime, W, H)
    bp, v, _ = whole(dev, c)
    assert bool(torch.isfinite(v.body()).all()) and bool(torch.isfinite(bp.body()).all())
    g, s = grad_figures(c, v.body()), sum_figures(c, partial_sum(bp))
    print(json.dumps(dict(test="regimes", regime=regime, W=W, H=H, grad=g, sum=s, f_max_over_w=c.f_max / abs(c.weight))))
    assert_sum(c, s, whole_image=True)
    assert_grad(c, g)


# ---------------------------------------------------------------------------------------------
# b. edge geometry
# ---------------------------------------------------------------------------------------------
EDGE_SIZES = [(1, 1), (3, 40), (40, 3), (10, 10), (11, 11),            # smaller than the window
              (64, 12), (65, 13), (63, 24), (128, 25), (129, 37),     # strip and segment edges of the two kernels
              (16, 100),                                              # fewer partials than 12-row segments: nblk escalates
              (54, 13), (55, 14), (108, 26), (109, 27)]               # the one-pass kernel's 54-column / 13-row edges


@pytest.mark.parametrize("W,H", EDGE_SIZES)
def test_edge_geometry(dev, W, H):
    c = case("uniform", W, H)
    bp, v, _ = whole(dev, c)
    assert bool(torch.isfinite(v.body()).all()), "v_img: a pixel was not written"
    n_p = default_partials(W, H)
    nblk, nwg = two_kernel_segments(W, H, n_p)
    g, s = grad_figures(c, v.body()), sum_figures(c, partial_sum(bp))
    print(json.dumps(dict(test="edge_geometry", W=W, H=H, nblk=nblk, nwg=nwg, grad=g, sum=s)))
    assert_partials(bp, n_p, nwg)
    assert_sum(c, s, whole_image=True)
    assert_grad(c, g)
    if (W, H) == (16, 100):
        assert nblk == 3          # 9 segments of 12 rows do not fit 7 partials: escalated inside the whole-image call


# ---------------------------------------------------------------------------------------------
# c. every segment length
# ---------------------------------------------------------------------------------------------
def test_every_segment_length(dev):
    """(70, 166): n_partials from the default down to 2 escalates from 2 to 16 blocks per segment (12 .. 166 rows; 7, 8 and
    10 .. 15 blocks give no fewer workgroups than 6 resp. 9 at this height and are passed over).  v_img is
    bit-identical throughout; the sums differ by summation order only: a thread adds at most 166 values, the wave
    reduction 6 more, the workgroup 3, each rounding at most 2^-24 of the running sum, so two sums lie within
    2 (166 + 9) 2^-24 sum|map| of each other.  n_partials = 1 is an error that touches nothing."""
    W, H = 70, 166
    c = case("uniform", W, H)
    img, gt = on_dev(c, dev)
    n_def = default_partials(W, H)
    order_bound = 2 * (166 + 9) * 2.0 ** -24 * float(c.ref.map.abs().sum())
    first_v = first_sum = None
    seen, worst = set(), 0.0
    for n_p in range(n_def, 1, -1):
        bp, v, sc = Buf(n_def, dev), Buf(3 * H * W, dev), Buf(9 * H * W, dev)
        assert call(W, H, img, gt, c.weight, bp, v, sc, rows=(0, H, 0, H), n_partials=n_p) == 0, n_p
        nblk, nwg = two_kernel_segments(W, H, n_p)
        seen.add(nblk)
        assert_partials(bp, n_p, nwg)
        tot = partial_sum(bp, n_p)
        if first_v is None:
            first_v, first_sum = v.bits.clone(), tot
            g, s = grad_figures(c, v.body()), sum_figures(c, tot)
            print(json.dumps(dict(test="every_segment_length", grad=g, sum=s)))
            assert_sum(c, s, whole_image=True)
            assert_grad(c, g)
        assert torch.equal(v.bits, first_v), f"v_img differs with {nblk} blocks per segment (n_partials {n_p})"
        worst = max(worst, abs(tot - first_sum))
        assert abs(tot - first_sum) <= order_bound, (n_p, nblk, tot, first_sum, order_bound)
    print(json.dumps(dict(test="every_segment_length", nblk=sorted(seen), worst_sum_diff_over_bound=worst / order_bound)))
    assert {2, 3, 4, 5, 6, 9, 16} <= seen and min(seen) == 2 and max(seen) == 16
    bp, v, sc = Buf(n_def, dev), Buf(3 * H * W, dev), Buf(9 * H * W, dev)
    assert call(W, H, img, gt, c.weight, bp, v, sc, rows=(0, H, 0, H), n_partials=1) != 0
    assert v.untouched() and bp.untouched()


# ---------------------------------------------------------------------------------------------
# d. the map row by row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["uniform", "mixed"])
def test_per_row_forward(dev, regime):
    """(70, 40): the sum of every single row of the map -- as a one-row forward-only band, and as a one-row count range
    inside a gradient call over the whole image -- against the reference's row sum, in units of that row's sum(u)."""
    W, H = 70, 40
    c = case(regime, W, H)
    img, gt = on_dev(c, dev)
    n_p = default_partials(W, H)
    worst = {}
    for mode in ("forward_only", "count_range"):
        figs = []
        v0 = None
        for y in range(H):
            bp = Buf(n_p, dev)
            if mode == "forward_only":
                assert call(W, H, img, gt, c.weight, bp, rows=(y, y + 1, y, y + 1)) == 0
            else:
                v, sc = Buf(3 * H * W, dev), Buf(9 * H * W, dev)
                assert call(W, H, img, gt, c.weight, bp, v, sc, rows=(0, H, y, y + 1)) == 0
                v0 = v.bits.clone() if v0 is None else v0
                assert torch.equal(v.bits, v0), y
            assert bool(torch.isfinite(bp.body()).all()) and bp.tail_ok()
            figs.append(sum_figures(c, partial_sum(bp), y, y + 1))
        worst[mode] = max(f["over_sum_u"] for f in figs)
        print(json.dumps(dict(test="per_row_forward", regime=regime, mode=mode, worst_over_sum_u=worst[mode],
                              rows_over_1=[y for y, f in enumerate(figs) if f["over_sum_u"] > 1])))
        for y, f in enumerate(figs):
            assert f["err"] <= SUM_UNITS * f["sum_u"], (regime, mode, y, f)


# ---------------------------------------------------------------------------------------------
# e. bands
# ---------------------------------------------------------------------------------------------
BANDS = [(0, 32, 0, 16), (16, 64, 16, 48), (48, 70, 48, 70),      # overlapping, as ops.band_rows makes them
         (10, 50, 20, 30),                                        # count strictly inside
         (10, 50, 30, 30),                                        # empty count
         (0, 1, 0, 1), (35, 36, 35, 36), (69, 70, 69, 70),        # one-row bands
         (0, 3, 0, 3), (0, 3, 1, 2), (67, 70, 67, 70), (67, 70, 68, 70)]   # ends within 5 rows of the top / bottom


@pytest.mark.parametrize("regime", ["uniform", "mixed"])
def test_bands(dev, regime):
    """(100, 70): v_img rows inside the band bit-identical to the whole-image call, rows outside still the NaN prefill,
    the band's sum against the reference over its count range; with a gradient buffer and forward-only."""
    W, H = 100, 70
    c = case(regime, W, H)
    img, gt = on_dev(c, dev)
    n_p = default_partials(W, H)
    _, v_whole, _ = whole(dev, c)
    assert_grad(c, grad_figures(c, v_whole.body()))
    row = 3 * W
    worst = 0.0
    for forward_only in (False, True):
        for (y0, y1, c0, c1) in BANDS:
            bp = Buf(n_p, dev)
            v, sc = (None, None) if forward_only else (Buf(3 * H * W, dev), Buf(9 * H * W, dev))
            assert call(W, H, img, gt, c.weight, bp, v, sc, rows=(y0, y1, c0, c1)) == 0
            tag = (regime, forward_only, y0, y1, c0, c1)
            if v is not None:
                assert v.untouched(0, y0 * row) and v.untouched(y1 * row), ("v_img written outside the band", tag)
                assert torch.equal(v.bits[y0 * row:y1 * row], v_whole.bits[y0 * row:y1 * row]), ("band differs from the whole image", tag)
            assert bool(torch.isfinite(bp.body()).all()), tag
            if c0 == c1:
                assert bool((bp.bits[:n_p] == 0).all()), ("empty count range: partials not all +0", tag)
            f = sum_figures(c, partial_sum(bp), c0, c1)
            worst = max(worst, f["over_sum_u"])
            assert f["err"] <= SUM_UNITS * f["sum_u"], (tag, f)
    print(json.dumps(dict(test="bands", regime=regime, worst_over_sum_u=worst)))
    # an empty band with a gradient buffer: v_img untouched, partials zero
    bp, v, sc = Buf(n_p, dev), Buf(3 * H * W, dev), Buf(9 * H * W, dev)
    assert call(W, H, img, gt, c.weight, bp, v, sc, rows=(20, 20, 20, 20)) == 0
    assert v.untouched() and bool((bp.bits[:n_p] == 0).all())


def test_empty_forward_only_band_zeroes_the_partials(dev):
    """v_img = NULL and y0 == y1: no row to produce, and the contract still says "workgroup sums, the rest zero" -- the
    caller sums the buffer."""
    W, H = 100, 70
    c = case("uniform", W, H)
    img, gt = on_dev(c, dev)
    n_p = default_partials(W, H)
    for y in (0, 20, H):
        bp = Buf(n_p, dev)
        assert call(W, H, img, gt, c.weight, bp, rows=(y, y, y, y)) == 0
        assert bool((bp.bits[:n_p] == 0).all()), (y, "block_partials not zeroed")
        # fewer partials than the buffer holds: only [0, n_partials) is the call's to write
        bp = Buf(n_p, dev)
        assert call(W, H, img, gt, c.weight, bp, rows=(y, y, y, y), n_partials=3) == 0
        assert bool((bp.bits[:3] == 0).all()) and bp.untouched(3)


# ---------------------------------------------------------------------------------------------
# f. the code paths the environment selects (read once per process: worker processes)
# ---------------------------------------------------------------------------------------------
FUSED_EDGE_SIZES = [(54, 13), (55, 14), (108, 26), (109, 27)]
WORKER_ENVS = [dict(TGS_SSIM_FUSED="1"), dict(TGS_SSIM_NBLK="3"), dict(TGS_SSIM_NBLK="4"), dict(TGS_SSIM_FUSED="1", TGS_SSIM_NBLK="5")]


def worker_cases():
    return [(r, 130, 40) for r in R.REGIMES] + [("uniform", W, H) for W, H in FUSED_EDGE_SIZES]


def worker_band(H):
    y0, y1 = H // 4, H - H // 5
    return y0, y1, y0 + 1, y1 - 2


def worker_main(out_path):
    """Runs in its own process: whole-image call and one band call per case, everything dumped for the parent."""
    dev = torch.device("cuda:0")
    out = {}
    for regime, W, H in worker_cases():
        img, gt = R.inputs(regime, W, H)
        c = types.SimpleNamespace(W=W, H=H, img=img, gt=gt, weight=-0.2 / (3 * H * W))
        bp, v, sc = whole(dev, c)
        k = f"{regime}/{W}x{H}"
        out[k + "/v"], out[k + "/bp"] = v.bits[:v.n].cpu(), bp.bits[:bp.n].cpu()
        out[k + "/scratch_untouched"] = sc.untouched()
        a, b = on_dev(c, dev)
        bpb, vb, scb = Buf(bp.n, dev), Buf(v.n, dev), Buf(sc.n, dev)
        assert call(W, H, a, b, c.weight, bpb, vb, scb, rows=worker_band(H)) == 0
        out[k + "/vb"], out[k + "/bpb"] = vb.bits[:vb.n].cpu(), bpb.bits[:bpb.n].cpu()
    torch.save(out, out_path)


def test_env_selected_paths(dev, tmp_path):
    """TGS_SSIM_FUSED=1 (the one-pass kernel), TGS_SSIM_NBLK=3 / 4 (23- and 34-row segments) and the two together, each in
    its own process, one after another: the regimes at (130, 40) and the one-pass kernel's edge sizes, whole image and one
    band, under the tolerances of the default path."""
    code = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_ssim_oracle as T; T.worker_main(sys.argv[2])"
    summary = []
    for i, extra in enumerate(WORKER_ENVS):
        f = str(tmp_path / f"worker_{i}.pt")
        env = {k: v for k, v in os.environ.items() if k not in ("TGS_SSIM_FUSED", "TGS_SSIM_NBLK")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", code, ROOT, f], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (extra, r.returncode, r.stderr[-2000:])
        res = torch.load(f)
        fused, env_nblk = "TGS_SSIM_FUSED" in extra, int(extra.get("TGS_SSIM_NBLK", 0))
        worst = dict(max_over_F=0.0, l2_over_F=0.0, over_sum_u=0.0, band_over_sum_u=0.0)
        for regime, W, H in worker_cases():
            c = case(regime, W, H)
            k = f"{regime}/{W}x{H}"
            tag = (extra, k)
            v_bits, bp_bits = res[k + "/v"], res[k + "/bp"]
            v, bp = v_bits.view(torch.float32), bp_bits.view(torch.float32)
            # the variable took effect: the one-pass kernel does not touch scratch, the two kernels fill it
            assert res[k + "/scratch_untouched"] == fused, tag
            assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(bp).all()), tag
            n_p = default_partials(W, H)
            nblk, nwg = (fused_segments if fused else two_kernel_segments)(W, H, n_p, env_nblk)
            assert bool((bp_bits[nwg:] == 0).all()), tag
            if regime == "uniform":
                assert bool((bp[:nwg] != 0).all()), (tag, nblk, nwg)
            g, s = grad_figures(c, v), sum_figures(c, float(bp.double().sum()))
            # the band: inside = the whole image's bits, outside = the prefill, its sum against the reference
            y0, y1, c0, c1 = worker_band(H)
            vb, row = res[k + "/vb"], 3 * W
            assert bool((vb[:y0 * row] == NAN_BITS).all()) and bool((vb[y1 * row:] == NAN_BITS).all()), tag
            assert torch.equal(vb[y0 * row:y1 * row], v_bits[y0 * row:y1 * row]), tag
            bpb = res[k + "/bpb"].view(torch.float32)
            assert bool(torch.isfinite(bpb).all()), tag
            sb = sum_figures(c, float(bpb.double().sum()), c0, c1)
            for key, val in (("max_over_F", g["max_over_F"]), ("l2_over_F", g["l2_over_F"]), ("over_sum_u", s["over_sum_u"]),
                             ("band_over_sum_u", sb["over_sum_u"])):
                worst[key] = max(worst[key], val)
            assert_sum(c, s, whole_image=True)
            assert_grad(c, g)
            assert sb["err"] <= SUM_UNITS * sb["sum_u"], (tag, sb)
        summary.append(dict(env=extra, **worst))
    print(json.dumps(dict(test="env_selected_paths", workers=summary)))


# ---------------------------------------------------------------------------------------------
# g. the eval path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["uniform", "mixed"])
def test_eval_path(dev, regime):
    """ops.ssim_fwd_bwd(want_grad=False), as the model's eval metrics call it."""
    from touch_gs_amd import ops
    c = case(regime, 100, 70)
    img, gt = on_dev(c, dev)
    tot, v = ops.ssim_fwd_bwd(img, gt, want_grad=False)
    assert v is None
    s = sum_figures(c, float(tot.double().item()))
    print(json.dumps(dict(test="eval_path", regime=regime, sum=s)))
    assert_sum(c, s, whole_image=True)
