"""Per-view exposure compensation on the GPU (csrc/exposure.hip: k_expo_fwd, k_expo_bwd_tiles, k_expo_fold; ops.exposure_fwd,
ops.exposure_bwd, ops.apply_exposure) against tests/exposure_ref.py.

Units: error of G in 2^-24 x mass with the mass from the reference; bar = 4 x the fp32 floor of the same case
(tests/exposure_ref.floor, printed by tests/test_cpu_exposure_ref.py::test_floors), never below 4 units.  Every figure is
printed before it is asserted (pytest -s); the floors and the measured figures are in DESIGN.md section 5.1n.

Every output is NaN-prefilled and a sentinel row sits behind the scratch.  out[24] is the valid flag and is 1 on every
frame without a raised guard -- also where neither gt nor v_img is given, where all OTHER entries of out[0..25] are 0.
"""
import types

import numpy as np
import pytest
import torch

from tests import adam_ref as AR
from tests import exposure_ref as XR

pytestmark = pytest.mark.gpu

E32 = 2.0 ** -24


def _chunk():
    from touch_gs_amd import _lib
    return _lib.EXPO_CHUNK


def _shapes():
    c = _chunk()
    return [(1, 1), (7, 3), (33, 17), (c - 1, 1), (c, 1), (c + 1, 1), (3 * c + 5, 1), (160, 120)]


SHAPE_IDS = ["1x1", "7x3", "33x17", "chunk-1", "chunk", "chunk+1", "3chunk+5", "160x120"]


def _note(name, key, value, bar):
    print(f"FIG {name:26s} {key:14s} measured {value:10.3f}  bar {bar:10.3f}")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)


def _with(case, **kw):
    """A copy of a case with some images replaced or dropped (None): floors and bars are those of the copy."""
    return types.SimpleNamespace(**{**vars(case), **kw})


def _fwd(case, dev, E=None):
    from touch_gs_amd import ops
    out = torch.full((case.H, case.W, 3), float("nan"), dtype=torch.float32, device=dev)
    got = ops.exposure_fwd(_t(case.C, dev), _t(case.E if E is None else E, dev), out=out)
    assert got is out
    return out.cpu().numpy()


def _bwd(case, dev, guard=None, state=None, adam=None, expo=None):
    """ops.exposure_bwd into NaN-filled outputs with one sentinel row behind the scratch -> (out [32] fp64, v_rgb fp32)."""
    from touch_gs_amd import _lib, ops
    P = _lib.load().tgs_exposure_num_partials(case.W, case.H)
    assert P == -(-case.W * case.H // _lib.EXPO_CHUNK)
    res = torch.full((_lib.EXPO_OUT,), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.full((P + 1, _lib.EXPO_OUT), float("nan"), dtype=torch.float32, device=dev)
    got, v_rgb = ops.exposure_bwd(_t(case.C, dev), _t(case.E, dev) if expo is None else expo, gt=_t(case.gt, dev),
                                  l1_weight=case.l1_weight, v_img=_t(case.v_img, dev), guard=guard, state=state, adam=adam,
                                  out=(res, scratch))
    assert got is res
    assert torch.isnan(scratch[P]).all(), "k_expo_bwd_tiles wrote behind its last row"
    if guard is None or not bool(guard[1]):
        assert not torch.isnan(scratch[:P]).any()
    return res.cpu().double().numpy(), v_rgb.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", _shapes(), ids=SHAPE_IDS)
def test_forward(dev, W, H):
    case = XR.dyadic_case(W, H)
    got = _fwd(case, dev)
    assert np.array_equal(got.astype(np.float64).reshape(-1, 3), XR.apply(case.C, case.E)), "dyadic inputs: C' is exact"
    case = XR.generic_case(W, H)
    got = _fwd(case, dev).astype(np.float64).reshape(-1, 3)
    e = float((np.abs(got - XR.apply(case.C, case.E)) / (E32 * XR.fwd_mass(case.C, case.E))).max())
    _note(f"fwd generic {W}x{H}", "roundings", e, 4)
    assert e <= 4
    assert np.array_equal(_fwd(case, dev, E=XR.IDENTITY), case.C), "identity E: C' == C"


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
def _check_bwd(label, case, out, v_rgb, ref):
    assert not np.isnan(out).any() and not np.isnan(v_rgb).any()
    assert out[24] == 1.0 and out[26] == case.W * case.H and (out[27:] == 0).all()
    e = np.abs(v_rgb.astype(np.float64).reshape(-1, 3) - ref.v_rgb)
    assert (e[ref.v_mass == 0] == 0).all()
    ev = float(np.where(ref.v_mass > 0, e / np.maximum(E32 * ref.v_mass, 1e-300), 0).max())
    _note(label, "v_rgb roundings", ev, 6)
    assert ev <= 6
    mass = ref.mass.reshape(-1).astype(np.float64)
    rel = np.abs(out[12:24] - mass) / np.where(mass > 0, mass, 1.0)
    _note(label, "mass rel", float(rel.max()), 1e-5)
    assert (rel <= 1e-5).all() and (out[12:24][mass == 0] == 0).all()
    bar_g, bar_l = XR.bar(case)
    eg = XR.err_units(out[:12], ref.G, ref.mass)
    _note(label, "G units", eg, bar_g)
    assert eg <= bar_g, (label, eg, bar_g)
    el = XR.err_units([out[25]], [ref.l1], [ref.l1])
    _note(label, "L1 units", el, bar_l)
    assert el <= bar_l, (label, el, bar_l)


@pytest.mark.parametrize("build", [XR.dyadic_case, XR.generic_case], ids=["dyadic", "generic"])
@pytest.mark.parametrize("W,H", _shapes(), ids=SHAPE_IDS)
def test_backward(dev, build, W, H):
    case = build(W, H)
    out, v_rgb = _bwd(case, dev)
    _check_bwd(f"bwd {build.__name__[:3]} {W}x{H}", case, out, v_rgb, XR.bwd(case.C, case.E, case.gt, case.l1_weight, case.v_img))
    again, v_again = _bwd(case, dev)
    assert np.array_equal(out, again) and np.array_equal(v_rgb, v_again), "the same inputs give the same bits"


def test_exact_ties_contribute_nothing(dev):
    """Dyadic builder, L1 only: C' - gt is exact, so the L1 value is the sum over the non-tie entries and a pixel whose three
    entries tie has v_rgb exactly 0; with every entry tied the whole gradient is exactly 0."""
    case = _with(XR.dyadic_case(33, 17), v_img=None)
    out, v_rgb = _bwd(case, dev)
    ref = XR.bwd(case.C, case.E, case.gt, case.l1_weight, None)
    assert (ref.vprime.reshape(17, 33, 3)[case.tie] == 0).all() and case.tie.any()
    _check_bwd("bwd ties 33x17", case, out, v_rgb, ref)
    case.gt = XR.apply(case.C, case.E).astype(np.float32).reshape(17, 33, 3)
    out, v_rgb = _bwd(case, dev)
    assert (np.delete(out, [24, 26]) == 0).all() and (v_rgb == 0).all()


@pytest.mark.parametrize("W,H", [(33, 17), (_chunk() + 1, 1)], ids=["33x17", "chunk+1"])
def test_absent_images(dev, W, H):
    full = XR.generic_case(W, H)
    case = _with(full, v_img=None)
    out, v_rgb = _bwd(case, dev)
    _check_bwd(f"bwd no v_img {W}x{H}", case, out, v_rgb, XR.bwd(case.C, case.E, case.gt, case.l1_weight, None))
    case = _with(full, gt=None)
    out, v_rgb = _bwd(case, dev)
    _check_bwd(f"bwd no gt {W}x{H}", case, out, v_rgb, XR.bwd(case.C, case.E, None, case.l1_weight, case.v_img))
    assert out[25] == 0
    out, v_rgb = _bwd(_with(full, gt=None, v_img=None), dev)
    assert (out[:24] == 0).all() and out[24] == 1 and out[25] == 0 and out[26] == W * H and (v_rgb == 0).all()


def test_guard(dev):
    """An overflow status word: out all zero, [24] = 0, and a given state row keeps every bit."""
    case = XR.generic_case(33, 17)
    row = torch.from_numpy(XR.new_row(np.float32)).to(dev)
    row[:36] = torch.randn(36, device=dev)
    row[24:36] = row[24:36].abs()
    row[36:39] = torch.tensor([3.0, 0.9 ** 3, 0.999 ** 3], device=dev)
    keep = row.clone()
    adam = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15, l2=0.1)
    out, _ = _bwd(case, dev, guard=torch.tensor([0, 1], dtype=torch.int32, device=dev), state=row, adam=adam, expo=row)
    assert (out == 0).all()
    assert torch.equal(row.view(torch.int32), keep.view(torch.int32))
    out, _ = _bwd(case, dev, guard=torch.zeros(2, dtype=torch.int32, device=dev), state=row, adam=adam, expo=row)
    assert out[24] == 1 and float(row[36]) == 4 and not torch.equal(row[:12], keep[:12])


# ---------------------------------------------------------------------------------------------
# Adam on the row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2", [0.0, 0.1])
def test_adam_row(dev, l2):
    """One row stepped 10 times; the upstream image is rescaled from step to step so that |g| spans 1e-8 ... 1e2.  Each step
    against tests/adam_ref: the gradient is the kernel's own out[0..11] plus the L2 term in fp64, known to
    dg = 2 x 2^-24 (|G| + |l2 (E - I)|) (the product and the add of the kernel); bound (c) takes the bias corrections from
    the kernel's own running products."""
    from touch_gs_amd import _lib
    case = _with(XR.generic_case(33, 17, seed=3), gt=None)
    base = case.v_img / np.abs(case.v_img).max()
    lr, betas, eps = 1e-2, (0.9, 0.999), 1e-15
    adam = dict(lr=lr, betas=betas, eps=eps, l2=l2)
    state = torch.zeros(2, _lib.EXPO_STATE, dtype=torch.float32, device=dev)
    state[0] = torch.from_numpy(XR.new_row(np.float32)).to(dev)
    state[1] = torch.from_numpy(XR.new_row(np.float32)).to(dev) + 0.25
    other = state[1].clone()
    b1, b2, ident = AR.f32(betas[0]), AR.f32(betas[1]), XR.IDENTITY.reshape(-1).astype(np.float64)
    gmin, gmax, worst = np.inf, 0.0, {}
    for t in range(1, 11):
        case.v_img = (base * 10.0 ** (-9.5 + 11 * (t - 1) / 9)).astype(np.float32)
        before = state[0].cpu().numpy()
        out, _ = _bwd(case, dev, state=state[0], adam=adam, expo=state[0])
        after = state[0].cpu().numpy()
        ref = XR.bwd(case.C, before[:12], None, 0.0, case.v_img)
        assert XR.err_units(out[:12], ref.G, ref.mass) <= XR.bar(_with(case, E=before[:12].reshape(3, 4)))[0]
        pull = AR.f32(l2) * (before[:12].astype(np.float64) - ident)
        g = out[:12] + pull
        dg = 2 * E32 * (np.abs(out[:12]) + np.abs(pull))
        gmin, gmax = min(gmin, np.abs(g).min()), max(gmax, np.abs(g).max())
        assert after[36] == t
        for k, beta in ((37, b1), (38, b2)):
            assert abs(float(after[k]) - beta ** t) <= (t + 1) * E32 * beta ** t, (t, k, after[k])
        assert (after[39:] == 0).all()
        f = np.float32
        spec = AR.AdamConsts(b1, b2, AR.f32(eps), float(f(1) - after[37]), float(f(1) - after[38]))
        r = AR.check_step((before[:12], before[12:24], before[24:36]), (after[:12], after[12:24], after[24:36]), g, dg,
                          np.float32(lr), spec, label=f"step {t} ")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"FIG adam row l2={l2}: |g| from {gmin:.2e} to {gmax:.2e}; worst ratios (units of 2^-24; bars m 4, v 8, p 16): {worst}")
    assert gmin <= 1e-8 and gmax >= 1e2, "the gradients do not span the range the test is about"
    assert torch.equal(state[1].view(torch.int32), other.view(torch.int32)), "the neighbouring row was touched"


# ---------------------------------------------------------------------------------------------
# seam with K7
# ---------------------------------------------------------------------------------------------
def test_seam_with_k7(dev):
    """Identity E on a built scene: K7 fed with exposure_bwd's v_rgb and no gt_rgb gives the partials, bit for bit, of K7 fed
    with SSIM's gradient and its own fused L1 term -- sign(0) (ties are planted) and the l1_weight convention are K7's --
    and out[25] is the sum of K7's tile_loss[:, 0]."""
    from tests.test_gpu_pose_grad import _model, _random_supervision
    from touch_gs_amd import ops
    N, W, H, deg = 300, 64, 48, 3
    model, P, c, V, cam, View = _model(dev, N, W, H, deg, 7)
    p = model.params
    splats, radii, group_base, tile_start, sorted_gid, status = ops.project_bin_sort(
        cam, p.means, p.log_scales, p.quats, p.opac_logit, p.sh, deg, model.budget)
    rgb, depth_acc, fT, _ = ops.rasterize_fwd(cam, splats, sorted_gid, tile_start)
    gt = _random_supervision(H, W)[0].float().to(dev)
    tie = torch.rand(H, W, 3, device=dev) < 0.05
    gt = torch.where(tie, rgb, gt).contiguous()
    l1w = 0.8 / (3 * H * W)
    _, v_ssim = ops.ssim_fwd_bwd(rgb, gt, weight=-0.2 / (3 * H * W), reduce=False)
    args = (cam, splats, group_base, sorted_gid, tile_start, rgb, depth_acc, fT)
    nan = lambda: torch.full((sorted_gid.shape[0], 12), float("nan"), dtype=torch.float32, device=dev)
    want, tile_loss = ops.rasterize_bwd(*args, v_rgb=v_ssim, loss=dict(gt_rgb=gt, l1_weight=l1w), want_tile_loss=True, partials=nan())
    ident = torch.from_numpy(XR.IDENTITY).to(dev)
    out, v_rgb = ops.exposure_bwd(rgb, ident, gt=gt, l1_weight=l1w, v_img=v_ssim)
    got, tl0 = ops.rasterize_bwd(*args, v_rgb=v_rgb, loss=dict(gt_rgb=None, l1_weight=0.0), want_tile_loss=True, partials=nan())
    # K7 writes a record per (tile, Gaussian) pair it walks: at most status[0] of them (pairs behind a tile's stop stay unwritten)
    written = ~torch.isnan(want).any(dim=1)
    print(f"FIG seam: {int(written.sum())} of {int(status[0])} partial records written")
    assert 0 < int(written.sum()) <= int(status[0])
    assert torch.isfinite(want[written]).all() and torch.equal(written, ~torch.isnan(got).any(dim=1))
    assert (want[written] != 0).any(dim=1).float().mean() > 0.5, "K7 wrote next to no gradient"
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (tl0[:, 0] == 0).all()
    case = XR._case(W, H, rgb.cpu().numpy(), XR.IDENTITY, gt.cpu().numpy(), v_ssim.cpu().numpy(), l1w)
    k7 = float(tile_loss[:, 0].double().sum())
    e, bar = abs(float(out[25]) - k7) / (E32 * k7), XR.bar(case)[1]
    _note("seam", "L1 vs K7 units", e, bar)
    assert e <= bar
    ref = XR.bwd(case.C, case.E, case.gt, case.l1_weight, None)
    assert XR.err_units([float(out[25])], [ref.l1], [ref.l1]) <= XR.bar(case)[1]


# ---------------------------------------------------------------------------------------------
# recovery, autograd
# ---------------------------------------------------------------------------------------------
def test_recovery(dev):
    """gt = A* C + b*, L1 only, 300 fwd / bwd steps at lr 0.01 from the identity; the final L1 against the fp64 reference
    running the same loop (tests/test_cpu_exposure_ref.py checks that IT ends below 10 % of its initial L1)."""
    from touch_gs_amd import ops
    C, gt, w = XR.recover_inputs()
    first_ref, last_ref, row_ref = XR.recovery_loop(XR.ref_grad_fn(C, gt, w))
    Cd, gd = _t(C, dev), _t(gt, dev)
    row = torch.from_numpy(XR.new_row(np.float32)).to(dev)
    adam = dict(lr=XR.RECOVER["lr"], betas=(0.9, 0.999), eps=1e-15, l2=0.0)
    for _ in range(XR.RECOVER["steps"]):
        ops.exposure_fwd(Cd, row)                      # (the image an SSIM term would read; the backward recomputes it)
        ops.exposure_bwd(Cd, row, gt=gd, l1_weight=w, state=row, adam=adam)
    assert float(row[36]) == XR.RECOVER["steps"]
    last = float(ops.exposure_bwd(Cd, row, gt=gd, l1_weight=w)[0][25])
    print(f"FIG recovery: initial L1 {first_ref:.6f}; reference ends {last_ref:.6f}; GPU ends {last:.6f}; "
          f"|E - E_ref| max {np.abs(row[:12].cpu().numpy() - row_ref[:12]).max():.2e}")
    assert last <= 1.5 * last_ref + 1e-6


def test_apply_exposure_autograd(dev):
    from touch_gs_amd import ops
    case = XR.generic_case(33, 17)
    C = _t(case.C, dev).requires_grad_(True)
    E = _t(case.E, dev).requires_grad_(True)
    cp = ops.apply_exposure(C, E)
    assert np.abs(cp.detach().cpu().double().numpy().reshape(-1, 3) - XR.apply(case.C, case.E)).max() <= \
        4 * E32 * XR.fwd_mass(case.C, case.E).max()
    (cp * _t(case.v_img, dev)).sum().backward()
    ref = XR.bwd(case.C, case.E, None, 0.0, case.v_img)
    assert E.grad.shape == (3, 4) and C.grad.shape == (17, 33, 3)
    e = XR.err_units(E.grad.cpu().numpy(), ref.G, ref.mass)
    _note("autograd 33x17", "G units", e, XR.bar(case)[0])
    assert e <= XR.bar(case)[0]
    ev = np.abs(C.grad.cpu().double().numpy().reshape(-1, 3) - ref.v_rgb) / (E32 * ref.v_mass)
    assert ev.max() <= 6
