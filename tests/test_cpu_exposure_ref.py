"""The exposure reference (tests/exposure_ref.py) against torch autograd in fp64, the properties of the two input builders, the
fp32 floors that set the bars of tests/test_gpu_exposure.py, the fp64 recovery loop, and the ABI of the three calls.  CPU only.

Floors (fp32 pairwise evaluation against fp64, units of 2^-24 mass; printed by test_floors): DESIGN.md section 5.1n.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import exposure_ref as XR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (7, 3), (33, 17), (160, 120))


@pytest.mark.parametrize("build", [XR.dyadic_case, XR.generic_case])
@pytest.mark.parametrize("W,H", SHAPES[:3])
def test_reference_equals_autograd(build, W, H):
    """L = <U, C'> + l1_weight sum |C' - gt| with C' = A C + b: autograd's gradients for C and E are v_rgb and G with
    v_img = U (torch's |.| has gradient 0 at 0: the sign(0) = 0 of the kernels), and L's second term is the L1 value."""
    case = build(W, H)
    C = torch.from_numpy(case.C.astype(np.float64)).requires_grad_(True)
    E = torch.from_numpy(case.E.astype(np.float64)).requires_grad_(True)
    U, gt = torch.from_numpy(case.v_img.astype(np.float64)), torch.from_numpy(case.gt.astype(np.float64))
    cp = C @ E[:, :3].T + E[:, 3]
    l1 = case.l1_weight * (cp - gt).abs().sum()
    ((U * cp).sum() + l1).backward()
    r = XR.bwd(case.C, case.E, case.gt, case.l1_weight, case.v_img)
    np.testing.assert_allclose(r.cprime.reshape(H, W, 3), cp.detach().numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(r.v_rgb.reshape(H, W, 3), C.grad.numpy(), rtol=1e-12, atol=1e-16)
    assert XR.err_units(r.G, E.grad.numpy(), r.mass) < 1e-6      # (2^-24 units: fp64 agreement to 1e-14 of the mass)
    assert abs(float(r.l1) - float(l1.detach())) <= 1e-13 * float(l1.detach()) + 1e-300
    assert r.count == W * H and XR.out32(r)[26] == W * H


@pytest.mark.parametrize("W,H", SHAPES)
def test_dyadic_builder(W, H):
    """C' is exact in fp32 in any order (so `==` is a fair check of the forward) and about 5 % of the entries tie."""
    case = XR.dyadic_case(W, H)
    assert (case.C >= 0).all() and (case.C < 1).all() and (case.C * 1024 == np.round(case.C * 1024)).all()
    assert (np.abs(case.E[:, :3]) <= 2).all() and (case.E[:, :3] * 64 == np.round(case.E[:, :3] * 64)).all()
    assert (case.E[:, 3] * 1024 == np.round(case.E[:, 3] * 1024)).all()
    c64, c32 = XR.apply(case.C, case.E), XR.apply(case.C, case.E, np.float32)
    assert np.array_equal(c64, c32.astype(np.float64))
    assert (c64 * 65536 == np.round(c64 * 65536)).all() and np.abs(c64).max() < 8     # 3 + 16 bits
    d = c64.reshape(H, W, 3) - case.gt.astype(np.float64)
    assert np.array_equal(d == 0, case.tie)
    nz = np.abs(d[~case.tie])
    assert nz.size == 0 or (nz.min() >= 2.0 ** -8 and nz.max() <= 0.5)
    if W * H >= 500:
        assert 0.03 < case.tie.mean() < 0.07


@pytest.mark.parametrize("W,H", SHAPES)
def test_generic_builder(W, H):
    """|C'_ref - gt| stays above 1e-3 - roundings, and the fp32 C' decides every sign as the reference does."""
    case = XR.generic_case(W, H)
    c64, c32 = XR.apply(case.C, case.E), XR.apply(case.C, case.E, np.float32)
    gt = case.gt.reshape(-1, 3).astype(np.float64)
    assert np.abs(c64 - gt).min() >= 1e-3 - 1e-6
    assert np.array_equal(np.sign(c64 - gt), np.sign(c32.astype(np.float64) - gt))
    assert np.abs(c32 - c64).max() <= 4 * XR.EPS32 * XR.fwd_mass(case.C, case.E).max()


def test_floors():
    print()
    for build in (XR.dyadic_case, XR.generic_case):
        for W, H in SHAPES + ((2047, 1), (2048, 1), (2049, 1), (6149, 1)):
            fg, fl = XR.floor(build(W, H))
            print(f"FLOOR {build.__name__:13s} {W:5d} x {H:3d}  G {fg:6.3f}  L1 {fl:6.3f}  (units of 2^-24 mass)")
            assert fg < 8 and fl < 8, "the fp32 pairwise evaluation itself is off: the reference or the masses are wrong"


def test_row_step_is_adam():
    """adam_row_step is torch.optim.Adam on the 12 entries with the L2 pull added to the gradient."""
    rng = np.random.default_rng(5)
    row = XR.new_row()
    E = torch.from_numpy(XR.IDENTITY.astype(np.float64).reshape(-1).copy()).requires_grad_(True)
    opt = torch.optim.Adam([E], lr=float(np.float32(0.01)), betas=(float(np.float32(0.9)), float(np.float32(0.999))),
                           eps=float(np.float32(1e-15)))
    l2 = float(np.float32(0.1))
    for t in range(1, 6):
        G = rng.standard_normal(12)
        E.grad = torch.from_numpy(G + l2 * (E.detach().numpy() - XR.IDENTITY.reshape(-1)))
        opt.step()
        row = XR.adam_row_step(row, G, 0.01, l2=0.1)
        np.testing.assert_allclose(row[:12], E.detach().numpy(), rtol=1e-12, atol=1e-15)
        assert row[36] == t and abs(row[37] - float(np.float32(0.9)) ** t) < 1e-15 and (row[39:] == 0).all()


def test_reference_recovers():
    """The fp64 loop of the GPU recovery test ends below 10 % of its initial L1 (otherwise raise the step count)."""
    C, gt, w = XR.recover_inputs()
    first, last, row = XR.recovery_loop(XR.ref_grad_fn(C, gt, w))
    print(f"\nRECOVER reference: L1 {first:.6f} -> {last:.6f} after {XR.RECOVER['steps']} steps; E =\n{row[:12].reshape(3, 4)}")
    assert last < 0.1 * first


def test_abi_declares_the_calls():
    from touch_gs_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert "#define TGS_VERSION 320" in hdr
    assert int(re.search(r"#define TGS_EXPO_OUT\s+(\d+)", hdr).group(1)) == _lib.EXPO_OUT == 32
    assert int(re.search(r"#define TGS_EXPO_STATE\s+(\d+)", hdr).group(1)) == _lib.EXPO_STATE == 48
    for name, nargs in (("tgs_exposure_num_partials", 2), ("tgs_exposure_fwd", 6), ("tgs_exposure_bwd", 18)):
        assert re.search(r"\bint " + name + r"\(", hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs
    src = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "exposure.hip")).read()
    m = re.search(r"EXPO_THREADS = (\d+);\s*\n\s*constexpr int EXPO_ROUNDS = (\d+);", src)
    assert int(m.group(1)) * 4 * int(m.group(2)) == _lib.EXPO_CHUNK
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)      # comments may speak of atomics; the code has none
    assert "atomic" not in code.lower()
