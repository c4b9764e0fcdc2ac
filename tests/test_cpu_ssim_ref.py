"""The fp64 SSIM reference of the K10 tests (tests/ssim_ref.py) against the oracle's SSIM and its autograd, and the fp32
floor -- the same formulas evaluated in fp32 on the CPU, separably and as one 121-tap convolution -- against the
conditioning unit the GPU tests bound the map with.  No GPU."""
import pytest
import torch

from oracle import torch_oracle as O
from tests import ssim_ref as R

SIZES = [(100, 70), (5, 5), (1, 1), (11, 3)]


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("W,H", SIZES)
def test_reference_equals_oracle_and_its_autograd(regime, W, H):
    """Explicit formulas against O.ssim / autograd, 1e-12 relative: the mean relative to itself, v_img relative to the
    largest un-cancelled term sum of the image (``mass``; on ``identical``, ``white`` and ``black`` the gradient itself is
    zero up to rounding, so it cannot be its own scale)."""
    img, gt = R.inputs(regime, W, H)
    assert img.shape == (H, W, 3) and img.dtype == torch.float32 and 0 <= float(img.min()) and float(img.max()) <= 1
    assert gt.shape == (H, W, 3) and gt.dtype == torch.float32 and 0 <= float(gt.min()) and float(gt.max()) <= 1
    weight = -0.2 / (3 * H * W)
    ref = R.ssim_ref(img, gt, weight)
    a = img.double().requires_grad_(True)
    s = O.ssim(a, gt.double())
    (weight * 3 * H * W * s).backward()
    assert abs(float(ref.map.mean()) - float(s.detach())) <= 1e-12 * abs(float(s.detach()))
    assert float((ref.v_img - a.grad).abs().max()) <= 1e-12 * float(ref.mass.max())
    assert bool((ref.unit >= 2.0 ** -21).all()) and bool(torch.isfinite(ref.unit).all())
    # both forms of the fp64 evaluation are the same reference: per pixel within the unit scaled to fp64's rounding
    alt = R.ssim_ref(img, gt, weight, separable=False)
    assert bool(((alt.map - ref.map).abs() <= 8 * 2.0 ** -29 * ref.unit).all())
    assert float((alt.v_img - ref.v_img).abs().max()) <= 1e-12 * float(ref.mass.max())


def test_regimes_are_what_they_say():
    W, H = 100, 70
    img, gt = R.inputs("white_vs_grey", W, H)
    assert bool((img == 1).all()) and bool((gt == torch.tensor(0.95).float()).all())
    for name, v in (("white", 1.0), ("black", 0.0)):
        img, gt = R.inputs(name, W, H)
        assert bool((img == v).all()) and bool((gt == v).all())
    img, gt = R.inputs("identical", W, H)
    assert torch.equal(img, gt) and float(img.std()) > 0.2
    img, gt = R.inputs("mixed", W, H)
    assert bool((gt[:, W // 2:] == torch.tensor(0.95).float()).logical_or(gt[:, W // 2:] == 1).all())
    for v in (0.0, 1.0):
        assert int(((img == v) & (gt == v)).sum()) >= 3 * (H // 4) * 2 * (W // 8)
    img, gt = R.inputs("flat_bright", W, H)
    assert not torch.equal(img, gt) and float((img - 0.95).abs().max()) < 1e-2 and float((gt - 0.95).abs().max()) < 1e-2
    img, gt = R.inputs("converged", W, H)
    assert 0 < float((img - gt).abs().max()) < 1e-2 and float(gt.std()) > 0.05
    for name in R.REGIMES:                      # fixed seeds
        a, b = R.inputs(name, 33, 17), R.inputs(name, 33, 17)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# Margins over the measured floor of the two fp32 evaluations (not fitted to any kernel).  Measured with this reference at
# (100, 70) over the nine regimes: per pixel at most 1.62 u (separable, smooth) and 4.86 u (121-tap, smooth); per row at
# most 0.34 sum(u) (separable) and 1.88 sum(u) (121-tap), both on white_vs_grey, where every pixel of a row rounds alike.
PIXEL_UNITS, ROW_UNITS = 8.0, 4.0


@pytest.mark.parametrize("separable", [True, False])
@pytest.mark.parametrize("regime", R.REGIMES)
def test_fp32_floor_stays_inside_the_unit(regime, separable):
    W, H = 100, 70
    img, gt = R.inputs(regime, W, H)
    ref = R.ssim_ref(img, gt)
    f32 = R.ssim_ref(img, gt, dtype=torch.float32, separable=separable)
    assert f32.map.dtype == torch.float32 and f32.v_img.dtype == torch.float32
    d = (f32.map.double() - ref.map).abs()
    per_pixel = float((d / ref.unit).max())
    per_row = float(((R.row_sums(f32.map) - R.row_sums(ref.map)).abs() / R.row_sums(ref.unit)).max())
    print({"regime": regime, "separable": separable, "per_pixel_u": round(per_pixel, 3), "per_row_sum_u": round(per_row, 3)})
    assert per_pixel <= PIXEL_UNITS, per_pixel
    assert per_row <= ROW_UNITS, per_row


def test_row_sums_and_floor_helpers():
    img, gt = R.inputs("uniform", 40, 30)
    w = -0.2 / (3 * 30 * 40)
    ref = R.ssim_ref(img, gt, w)
    assert R.row_sums(ref.map).shape == (30,) and R.row_sums(ref.map, 4, 9).shape == (5,) and R.row_sums(ref.map, 7, 7).numel() == 0
    assert abs(float(R.row_sums(ref.map).sum()) - float(ref.map.sum())) < 1e-9
    assert torch.equal(R.row_sums(ref.map, 4, 9), R.row_sums(ref.map)[4:9])
    fl = R.fp32_floor(img, gt, w, ref)
    assert 0 < fl.f_max <= fl.f_l2 and fl.f_max < 1e-4 * float(ref.v_img.abs().max())
    # the gradient is linear in the weight
    assert torch.allclose(R.ssim_ref(img, gt, 2 * w).v_img, 2 * ref.v_img, rtol=1e-14, atol=0)
