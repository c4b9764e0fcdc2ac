"""Per-view bilateral grids on the GPU (csrc/bilagrid.hip: k_bg_fwd, k_bg_cells, k_bg_fold, k_bg_step; ops.bilagrid_fwd,
ops.bilagrid_bwd, ops.apply_bilagrid) against tests/bilagrid_ref.py.

Units: errors in 2^-24 x mass with the mass from the reference; bar = 4 x the fp32 floor of the same case
(tests/bilagrid_ref.floors, printed by tests/test_cpu_bilagrid.py::test_floors), never below 4 units.  Every figure is
printed before it is asserted (pytest -s); the floors and the measured figures are in DESIGN.md section 5.1q.

Every output is NaN-prefilled and a sentinel row sits behind the scratch.  out[0] is the valid flag and is 1 on every frame
without a raised guard -- also where neither gt nor v_img is given, where the L1 value and every gradient are 0.
"""
import functools
import types

import numpy as np
import pytest
import torch

from tests import adam_ref as AR
from tests import bilagrid_ref as BR

pytestmark = pytest.mark.gpu

E32 = 2.0 ** -24
GRIDS = [(16, 16, 8), (2, 2, 2), (5, 3, 4)]
GRID_IDS = ["16x16x8", "2x2x2", "5x3x4"]


def _chunk():
    from touch_gs_amd import _lib
    return _lib.BILAGRID_CHUNK


def _shapes():
    c = _chunk()
    return [(1, 1), (7, 3), (33, 17), (c - 1, 1), (c, 1), (c + 1, 1), (3 * c + 5, 1), (160, 120)]


SHAPE_IDS = ["1x1", "7x3", "33x17", "chunk-1", "chunk", "chunk+1", "3chunk+5", "160x120"]


def _note(name, key, value, bar):
    print(f"FIG {name:34s} {key:16s} measured {value:10.3f}  bar {bar:10.3f}")


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)


def _with(case, **kw):
    """A copy of a case with some images replaced or dropped (None): floors and bars are those of the copy."""
    return types.SimpleNamespace(**{**vars(case), **kw})


@functools.lru_cache(maxsize=None)
def _ref(W, H, shape):
    """The case, its fp64 reference and its bars: computed once, shared by the tests, never changed."""
    case = BR.make_case(W, H, shape)
    return case, BR.case_bwd(case), BR.bars(case), BR.tv(case.grid)[0]


def _fwd(case, dev, grid=None):
    from touch_gs_amd import ops
    out = torch.full((case.H, case.W, 3), float("nan"), dtype=torch.float32, device=dev)
    got = ops.bilagrid_fwd(_t(case.C, dev), _t(case.grid if grid is None else grid, dev), case.shape, out=out)
    assert got is out
    return out.cpu().numpy()


def _bwd(case, dev, guard=None, state=None, adam=None, grid=None, tv_weight=0.0):
    """ops.bilagrid_bwd into NaN-filled outputs with one sentinel row behind the scratch
    -> (out [8] fp64, v_rgb fp32 [H,W,3], grad fp64 [2,n])."""
    from touch_gs_amd import _lib, ops
    lib = _lib.load()
    GW, GH, L = case.shape
    n, S = ops.bilagrid_sizes(case.W, case.H, case.shape)
    P, R = lib.tgs_bilagrid_num_partials(case.W, case.H, GW, GH, L), lib.tgs_bilagrid_row_floats(L)
    assert n == BR.n_entries(case.shape) and S == P * R + n + -(-n // 256) + 4 and S == lib.tgs_bilagrid_scratch_floats(case.W, case.H, GW, GH, L)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=dev)
    res, scratch, v_rgb, grad = nan(_lib.BILAGRID_OUT), nan(S + R), nan(case.H, case.W, 3), nan(2, n)
    got = ops.bilagrid_bwd(_t(case.C, dev), _t(case.grid, dev) if grid is None else grid, case.shape, gt=_t(case.gt, dev),
                           l1_weight=case.l1_weight, v_img=_t(case.v_img, dev), tv_weight=tv_weight, guard=guard, state=state,
                           adam=adam, out=(res, scratch, v_rgb, grad))
    assert got[0] is res and got[1] is v_rgb and got[2] is grad
    assert torch.isnan(scratch[S:]).all(), "a kernel wrote behind the scratch"
    assert not torch.isnan(v_rgb).any(), "v_rgb is written on every frame"
    if guard is None or not bool(guard[1]):
        assert not torch.isnan(scratch[:S - 4]).any() and not torch.isnan(grad).any()
    return res.cpu().double().numpy(), v_rgb.cpu().numpy(), grad.cpu().double().numpy()


# ---------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("W,H", _shapes(), ids=SHAPE_IDS)
def test_forward(dev, W, H, shape):
    case, ref, bars, _ = _ref(W, H, shape)
    got = _fwd(case, dev).astype(np.float64).reshape(-1, 3)
    e = BR.err_units(got, ref.cprime, BR.fwd_mass(case.C, case.grid, shape, W, H))
    _note(f"fwd {W}x{H} {shape}", "units", e, bars["fwd"])
    assert e <= bars["fwd"]
    assert np.array_equal(_fwd(case, dev, grid=BR.identity_grid(shape)), case.C), "identity grid: C' == C"


# ---------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------
def _check_bwd(label, case, got, ref, bars, tv_ref):
    out, v_rgb, grad = got
    assert not np.isnan(out).any()
    assert out[0] == 1.0 and out[2] == case.W * case.H == ref.count and (out[4:] == 0).all()
    ev = BR.err_units(v_rgb, ref.v_rgb, ref.v_mass)
    _note(label, "v_rgb units", ev, bars["v_rgb"])
    assert ev <= bars["v_rgb"]
    G, M = grad
    assert (G[~ref.touched] == 0).all() and (M[~ref.touched] == 0).all(), "a vertex no pixel reaches holds a gradient"
    mass = ref.mass.astype(np.float64)
    rel = float((np.abs(M - mass) / np.where(mass > 0, mass, 1.0)).max())
    _note(label, "mass rel", rel, 1e-5)
    assert rel <= 1e-5 and (M[mass == 0] == 0).all()
    eg = BR.err_units(G, ref.G, ref.mass)
    _note(label, "G units", eg, bars["G"])
    assert eg <= bars["G"], (label, eg, bars["G"])
    el = BR.err_units([out[1]], [ref.l1], [ref.l1])
    _note(label, "L1 units", el, bars["l1"])
    assert el <= bars["l1"], (label, el, bars["l1"])
    et = BR.err_units([out[3]], [tv_ref], [tv_ref])
    _note(label, "TV units", et, bars["tv"])
    assert et <= bars["tv"], (label, et, bars["tv"])


@pytest.mark.parametrize("shape", GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("W,H", _shapes(), ids=SHAPE_IDS)
def test_backward(dev, W, H, shape):
    case, ref, bars, tv_ref = _ref(W, H, shape)
    got = _bwd(case, dev)
    _check_bwd(f"bwd {W}x{H} {shape}", case, got, ref, bars, tv_ref)
    again = _bwd(case, dev)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "the same inputs give the same bits"
    if (W, H, shape) == (7, 3, (16, 16, 8)):
        assert not ref.touched.all(), "7 x 3 under 16 x 16 is to have empty cells"


@pytest.mark.parametrize("W,H,shape", [(33, 17, (5, 3, 4)), (_chunk() + 1, 1, (2, 2, 2))], ids=["33x17", "chunk+1"])
def test_absent_images(dev, W, H, shape):
    full = _ref(W, H, shape)[0]
    tv_ref = BR.tv(full.grid)[0]
    for label, case in (("no v_img", _with(full, v_img=None)), ("no gt", _with(full, gt=None))):
        got = _bwd(case, dev)
        _check_bwd(f"bwd {label} {W}x{H}", case, got, BR.case_bwd(case), BR.bars(case), tv_ref)
        if case.gt is None:
            assert got[0][1] == 0
    out, v_rgb, grad = _bwd(_with(full, gt=None, v_img=None), dev)
    assert out[0] == 1 and out[1] == 0 and out[2] == W * H and (v_rgb == 0).all() and (grad == 0).all()
    assert BR.err_units([out[3]], [tv_ref], [tv_ref]) <= _ref(W, H, shape)[2]["tv"]


def test_ties_contribute_nothing(dev):
    """gt planted from the GPU forward's own output on 5 % of the entries: the backward recomputes C' with the forward's
    bits, so those entries contribute exactly nothing (the reference is given the tie mask); with every entry tied and no
    upstream image the whole gradient is exactly 0."""
    W, H, shape = 33, 17, (5, 3, 4)
    base = _ref(W, H, shape)[0]
    cp = _fwd(base, dev)
    tie = np.random.default_rng(9).random((H, W, 3)) < 0.05
    case = _with(base, gt=np.where(tie, cp, base.gt).astype(np.float32), v_img=None, tie=tie)
    ref = BR.case_bwd(case)
    assert tie.any() and (ref.vprime.reshape(H, W, 3)[tie] == 0).all() and (ref.vprime != 0).any()
    _check_bwd("bwd ties 33x17", case, _bwd(case, dev), ref, BR.bars(case), BR.tv(case.grid)[0])
    out, v_rgb, grad = _bwd(_with(base, gt=cp, v_img=None), dev)
    assert out[0] == 1 and out[1] == 0 and (grad == 0).all() and (v_rgb == 0).all()


def _rows(dev, shape, k=3):
    """k state rows with random contents (positive second moments, t = 3)."""
    from touch_gs_amd import _lib
    n = BR.n_entries(shape)
    state = torch.zeros(k, 3 * n + _lib.BILAGRID_TAIL, dtype=torch.float32, device=dev)
    for i in range(k):
        state[i] = torch.from_numpy(BR.new_row(shape, np.float32)).to(dev)
    state[:, :3 * n] += 0.1 * torch.randn(k, 3 * n, device=dev)
    state[:, 2 * n:3 * n] = state[:, 2 * n:3 * n].abs()
    state[:, 3 * n:3 * n + 3] = torch.tensor([3.0, 0.9 ** 3, 0.999 ** 3], device=dev)
    return state, n


def test_guard(dev):
    """An overflow status word: out all zero, and the row and its neighbour rows keep every bit; v_rgb is still written."""
    case = _ref(33, 17, (5, 3, 4))[0]
    state, n = _rows(dev, case.shape)
    keep = state.clone()
    adam = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15)
    out, v_rgb, _ = _bwd(case, dev, guard=torch.tensor([0, 1], dtype=torch.int32, device=dev), state=state[1], adam=adam,
                         grid=state[1], tv_weight=10.0)
    assert (out == 0).all()
    assert torch.equal(state.view(torch.int32), keep.view(torch.int32))
    held = _with(case, grid=keep[1, :n].cpu().numpy().reshape(3, 5, 4, 12))
    ref = BR.case_bwd(held)
    assert BR.err_units(v_rgb, ref.v_rgb, ref.v_mass) <= BR.bars(held)["v_rgb"]
    out, _, _ = _bwd(case, dev, guard=torch.zeros(2, dtype=torch.int32, device=dev), state=state[1], adam=adam, grid=state[1],
                     tv_weight=10.0)
    assert out[0] == 1 and float(state[1, 3 * n]) == 4 and not torch.equal(state[1, :n], keep[1, :n])
    assert torch.equal(state[0].view(torch.int32), keep[0].view(torch.int32))
    assert torch.equal(state[2].view(torch.int32), keep[2].view(torch.int32))


# ---------------------------------------------------------------------------------------------
# Adam and TV on the row
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tv_weight", [0.0, 10.0])
def test_adam_row(dev, tv_weight):
    """One row stepped 10 times; the upstream image is rescaled from step to step so that |G| spans 1e-8 ... 1e2.  Each step
    against tests/adam_ref: the gradient is the kernel's own G plus tv_weight dTV/dg of the grid BEFORE the step in fp64
    (a kernel that stepped in place while reading its neighbours would miss it), known to dg = 2 x 2^-24 (|G| + |tv term|)
    (the rounding of G and of the sum); bound (c) takes the bias corrections from the kernel's own running products."""
    from touch_gs_amd import _lib
    W, H, shape = 33, 17, (5, 3, 4)
    GW, GH, L = shape
    case = _with(_ref(W, H, shape)[0], gt=None)
    base = case.v_img / np.abs(case.v_img).max()
    lr, betas, eps = 1e-2, (0.9, 0.999), 1e-15
    adam = dict(lr=lr, betas=betas, eps=eps)
    n = BR.n_entries(shape)
    state = torch.zeros(3, 3 * n + _lib.BILAGRID_TAIL, dtype=torch.float32, device=dev)
    for i in range(3):
        state[i] = torch.from_numpy(BR.new_row(shape, np.float32)).to(dev)
    state[1, :n] = _t(case.grid.reshape(-1), dev)
    state[0, :3 * n] += 0.25
    state[2, :3 * n] += 0.5
    others = state.clone()
    b1, b2 = AR.f32(betas[0]), AR.f32(betas[1])
    gmin, gmax, worst = np.inf, 0.0, {}
    for t in range(1, 11):
        case.v_img = (base * 10.0 ** (-9.5 + 12 * (t - 1) / 9)).astype(np.float32)
        before = state[1].cpu().numpy()
        out, _, grad = _bwd(case, dev, state=state[1], adam=adam, grid=state[1], tv_weight=tv_weight)
        after = state[1].cpu().numpy()
        grid0 = before[:n].reshape(GH, GW, L, 12)
        ref = BR.bwd(case.C, grid0, shape, W, H, None, 0.0, case.v_img)
        bars = BR.bars(_with(case, grid=grid0))
        assert BR.err_units(grad[0], ref.G, ref.mass) <= bars["G"]
        tv_val, tv_grad = BR.tv(grid0)
        assert BR.err_units([out[3]], [tv_val], [tv_val]) <= bars["tv"]
        pull = AR.f32(tv_weight) * tv_grad.reshape(-1)
        g = grad[0] + pull
        dg = 2 * E32 * (np.abs(grad[0]) + np.abs(pull))
        live = np.abs(grad[0]) > 0
        gmin, gmax = min(gmin, np.abs(grad[0][live]).min()), max(gmax, np.abs(grad[0]).max())
        assert after[3 * n] == t
        for k, beta in ((3 * n + 1, b1), (3 * n + 2, b2)):
            assert abs(float(after[k]) - beta ** t) <= (t + 1) * E32 * beta ** t, (t, k, after[k])
        assert (after[3 * n + 3:] == 0).all()
        f = np.float32
        spec = AR.AdamConsts(b1, b2, AR.f32(eps), float(f(1) - after[3 * n + 1]), float(f(1) - after[3 * n + 2]))
        r = AR.check_step((before[:n], before[n:2 * n], before[2 * n:3 * n]), (after[:n], after[n:2 * n], after[2 * n:3 * n]), g, dg,
                          np.float32(lr), spec, label=f"step {t} ")
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    print(f"FIG adam row tv={tv_weight}: |G| from {gmin:.2e} to {gmax:.2e}; worst ratios (units of 2^-24; bars m 4, v 8, p 16): {worst}")
    assert gmin <= 1e-8 and gmax >= 1e2, "the gradients do not span the range the test is about"
    for i in (0, 2):
        assert torch.equal(state[i].view(torch.int32), others[i].view(torch.int32)), "a neighbouring row was touched"


# ---------------------------------------------------------------------------------------------
# seam with K7
# ---------------------------------------------------------------------------------------------
def test_seam_with_k7(dev):
    """Identity grid on a built scene: A1 - A0 = 0 and A = I, so v_rgb == v' exactly, and K7 fed with bilagrid_bwd's v_rgb and
    no gt_rgb gives the partials, bit for bit, of K7 fed with SSIM's gradient and its own fused L1 term -- sign(0) (ties are
    planted) and the l1_weight convention are K7's -- and out[1] is the sum of K7's tile_loss[:, 0]."""
    from tests.test_gpu_pose_grad import _model, _random_supervision
    from touch_gs_amd import ops
    N, W, H, deg, shape = 300, 64, 48, 3, (16, 16, 8)
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
    ident = torch.from_numpy(BR.identity_grid(shape)).to(dev)
    assert torch.equal(ops.bilagrid_fwd(rgb, ident, shape), rgb)
    out, v_rgb, _ = ops.bilagrid_bwd(rgb, ident, shape, gt=gt, l1_weight=l1w, v_img=v_ssim, tv_weight=0.0)
    got, tl0 = ops.rasterize_bwd(*args, v_rgb=v_rgb, loss=dict(gt_rgb=None, l1_weight=0.0), want_tile_loss=True, partials=nan())
    written = ~torch.isnan(want).any(dim=1)
    print(f"FIG seam: {int(written.sum())} of {int(status[0])} partial records written")
    assert 0 < int(written.sum()) <= int(status[0])
    assert torch.isfinite(want[written]).all() and torch.equal(written, ~torch.isnan(got).any(dim=1))
    assert (want[written] != 0).any(dim=1).float().mean() > 0.5, "K7 wrote next to no gradient"
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert (tl0[:, 0] == 0).all()
    case = types.SimpleNamespace(W=W, H=H, shape=shape, C=rgb.cpu().numpy(), grid=BR.identity_grid(shape), gt=gt.cpu().numpy(),
                                 v_img=v_ssim.cpu().numpy(), l1_weight=float(np.float32(l1w)), tie=tie.cpu().numpy())
    bar = BR.bars(case)["l1"]
    k7 = float(tile_loss[:, 0].double().sum())
    e = abs(float(out[1]) - k7) / (E32 * k7)
    _note("seam", "L1 vs K7 units", e, bar)
    assert e <= bar and float(out[3]) == 0.0
    ref = BR.case_bwd(case)
    assert BR.err_units([float(out[1])], [ref.l1], [ref.l1]) <= bar


# ---------------------------------------------------------------------------------------------
# recovery, autograd
# ---------------------------------------------------------------------------------------------
def test_recovery(dev):
    """gt = C sliced through a fixed smooth grid, L1 only, 300 fwd / bwd steps from the identity; the final L1 against the
    fp64 reference running the same loop (tests/test_cpu_bilagrid.py checks that IT ends below 25 % of its initial L1)."""
    from touch_gs_amd import _lib, ops
    C, gt, w = BR.recover_inputs()
    first_ref, last_ref, row_ref = BR.recovery_loop(BR.ref_grad_fn(C, gt, w))
    shape, n = BR.RECOVER["shape"], BR.n_entries(BR.RECOVER["shape"])
    Cd, gd = _t(C, dev), _t(gt, dev)
    row = torch.from_numpy(BR.new_row(shape, np.float32)).to(dev)
    adam = dict(lr=BR.RECOVER["lr"], betas=(0.9, 0.999), eps=1e-15)
    S = ops.bilagrid_sizes(BR.RECOVER["W"], BR.RECOVER["H"], shape)[1]
    bufs = (torch.empty(_lib.BILAGRID_OUT, device=dev), torch.empty(S, device=dev))
    for _ in range(BR.RECOVER["steps"]):
        ops.bilagrid_fwd(Cd, row, shape)                # (the image an SSIM term would read; the backward recomputes it)
        ops.bilagrid_bwd(Cd, row, shape, gt=gd, l1_weight=w, state=row, adam=adam, want_grad=False, out=bufs)
    assert float(row[3 * n]) == BR.RECOVER["steps"]
    last = float(ops.bilagrid_bwd(Cd, row, shape, gt=gd, l1_weight=w)[0][1])
    print(f"FIG recovery: initial L1 {first_ref:.6f}; reference ends {last_ref:.6f}; GPU ends {last:.6f}; "
          f"|g - g_ref| max {np.abs(row[:n].cpu().numpy() - row_ref[:n]).max():.2e}")
    assert last_ref < 0.25 * first_ref
    assert last <= 1.5 * last_ref + 1e-6


def test_apply_bilagrid_autograd(dev):
    from touch_gs_amd import ops
    W, H, shape = 33, 17, (5, 3, 4)
    case, _, bars, _ = _ref(W, H, shape)
    case = _with(case, gt=None)
    C = _t(case.C, dev).requires_grad_(True)
    g = _t(case.grid, dev).requires_grad_(True)
    cp = ops.apply_bilagrid(C, g)
    ref = BR.case_bwd(case)
    assert BR.err_units(cp.detach().cpu().numpy(), ref.cprime, BR.fwd_mass(case.C, case.grid, shape, W, H)) <= bars["fwd"]
    (cp * _t(case.v_img, dev)).sum().backward()
    assert g.grad.shape == case.grid.shape and C.grad.shape == (H, W, 3)
    b = BR.bars(case)
    e = BR.err_units(g.grad.cpu().numpy(), ref.G, ref.mass)
    _note("autograd 33x17", "G units", e, b["G"])
    assert e <= b["G"]
    ev = BR.err_units(C.grad.cpu().numpy(), ref.v_rgb, ref.v_mass)
    _note("autograd 33x17", "v_rgb units", ev, b["v_rgb"])
    assert ev <= b["v_rgb"]
