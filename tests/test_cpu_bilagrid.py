"""The bilateral-grid reference (tests/bilagrid_ref.py) against torch autograd through F.grid_sample in fp64, the properties of
the input builder, the fp32 floors that set the bars of tests/test_gpu_bilagrid.py, the fp64 recovery loop, the ABI of the
calls, argument validation, and BilagridSet's row layout, schedule and file format.  CPU only.

Floors (fp32 evaluation against fp64, units of 2^-24 mass; printed by test_floors): DESIGN.md section 5.1q.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bilagrid_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = {
    "tgs_bilagrid_num_partials": 5, "tgs_bilagrid_row_floats": 1, "tgs_bilagrid_scratch_floats": 5,
    "tgs_bilagrid_fwd": 9, "tgs_bilagrid_bwd": 22,
}


def test_entry_points_are_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert "#define TGS_VERSION 320" in hdr and lib.tgs_version() == 320
    assert int(re.search(r"#define TGS_BILAGRID_OUT\s+(\d+)", hdr).group(1)) == _lib.BILAGRID_OUT == 8
    assert int(re.search(r"#define TGS_BILAGRID_TAIL\s+(\d+)", hdr).group(1)) == _lib.BILAGRID_TAIL == BR.TAIL == 16
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, nargs in NAMES.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, f"prototype of {name} missing from include/tgs.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert getattr(lib, name) is not None
    src = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "bilagrid.hip")).read()
    m = re.search(r"BG_THREADS = (\d+);\s*\n\s*constexpr int BG_PX = (\d+);", src)
    assert int(m.group(1)) * int(m.group(2)) == _lib.BILAGRID_CHUNK
    body = re.sub(r"//[^\n]*|/\*.*?\*/", "", src, flags=re.S)      # comments may speak of atomics; the code has none
    assert "atomic" not in body.lower() and "fmaf" not in body
    build = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "build.sh")).read()
    assert '[bilagrid]="-ffp-contract=off"' in build and re.search(r'SRCS="[^"]*\bbilagrid\b', build)


def test_size_functions_depend_on_the_five_integers():
    from touch_gs_amd import _lib
    lib = _lib.load()
    ch = _lib.BILAGRID_CHUNK
    assert lib.tgs_bilagrid_row_floats(8) == 4 * 8 * 24 + 8
    assert lib.tgs_bilagrid_row_floats(1) == 0
    # (2,2,2): one cell holds every pixel, hence ceil(W H / chunk) chunks
    for W, H in ((1, 1), (ch, 1), (ch + 1, 1), (3 * ch + 5, 1), (160, 120)):
        assert lib.tgs_bilagrid_num_partials(W, H, 2, 2, 2) == -(-W * H // ch)
    # cells no wider than the chunk: one row per cell, empty cells included (7 x 3 under 16 x 16)
    assert lib.tgs_bilagrid_num_partials(7, 3, 16, 16, 8) == 15 * 15
    P = lib.tgs_bilagrid_num_partials(160, 120, 16, 16, 8)
    n = 16 * 16 * 8 * 12
    assert lib.tgs_bilagrid_scratch_floats(160, 120, 16, 16, 8) == P * (4 * 8 * 24 + 8) + n + -(-n // 256) + 4
    assert lib.tgs_bilagrid_num_partials(160, 120, 1, 16, 8) == 0 and lib.tgs_bilagrid_scratch_floats(0, 1, 2, 2, 2) == 0


def test_argument_validation_launches_nothing():
    """Every refusal comes back before a launch: the pointers handed in are host memory."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.tgs_last_error()
    f = C.c_float

    def fwd(W=4, H=4, GW=2, GH=2, L=2, rgb=p, grid=p, out=p):
        return lib.tgs_bilagrid_fwd(W, H, GW, GH, L, rgb, grid, out, None)

    def bwd(W=4, H=4, GW=2, GH=2, L=2, rgb=p, grid=p, v_rgb=p, scratch=p, out=p, state=None, b1=0.9, b2=0.999):
        return lib.tgs_bilagrid_bwd(W, H, GW, GH, L, rgb, grid, None, f(0), None, f(0), v_rgb, scratch, None, out, None, state,
                                    f(1e-3), f(b1), f(b2), f(1e-15), None)

    for call in (fwd, bwd):
        for kw in (dict(W=0), dict(H=-1), dict(GW=1), dict(GH=1), dict(L=1), dict(L=65), dict(GW=4097), dict(W=1 << 16, H=1 << 16)):
            assert call(**kw) == -1 and b"bad image or grid size" in err(), (call.__name__, kw)
        for kw in (dict(rgb=None), dict(grid=None)):
            assert call(**kw) == -1 and b"null" in err(), (call.__name__, kw)
    assert fwd(out=None) == -1 and b"null" in err()
    for kw in (dict(v_rgb=None), dict(scratch=None), dict(out=None)):
        assert bwd(**kw) == -1 and b"null" in err(), kw
    assert bwd(state=p, b1=1.0) == -1 and b"beta" in err()
    assert bwd(state=p, b2=-0.1) == -1 and b"beta" in err()


# ---------------------------------------------------------------------------------------------
# the reference against torch
# ---------------------------------------------------------------------------------------------
def _torch_slice(C, grid, shape, W, H):
    """C' through F.grid_sample: grid [GH,GW,L,12] -> [1,12,L,GH,GW], align_corners=True, padding_mode='border', guide
    ((px + 0.5) / W, (py + 0.5) / H, luma) mapped to [-1, 1]."""
    GW, GH, L = shape
    vol = grid.permute(3, 2, 0, 1)[None]
    px = (torch.arange(W, dtype=torch.float64) + 0.5) / W
    py = (torch.arange(H, dtype=torch.float64) + 0.5) / H
    wl = torch.tensor([float(np.float32(w)) for w in BR.WL], dtype=torch.float64)
    luma = (C * wl).sum(dim=1)
    guide = torch.stack([px.repeat(H), py.repeat_interleave(W), luma], dim=1) * 2 - 1
    A = F.grid_sample(vol, guide[None, None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A.reshape(12, -1).T.reshape(-1, 3, 4)
    return (A[:, :, :3] * C[:, None, :]).sum(dim=2) + A[:, :, 3]


@pytest.mark.parametrize("W,H,shape", [(33, 17, (5, 3, 4)), (7, 3, (16, 16, 8)), (40, 30, (2, 2, 2))])
def test_reference_equals_grid_sample_autograd(W, H, shape):
    """L = <U, C'> + l1_weight sum |C' - gt|: autograd's gradients for C (the guide included) and for the grid are v_rgb and
    G of the reference in its fp64-guide mode; TV and its gradient against torch's own differences."""
    case = BR.make_case(W, H, shape, seed=1)
    GW, GH, L = shape
    Ct = torch.from_numpy(case.C.reshape(-1, 3).astype(np.float64)).requires_grad_(True)
    g = torch.from_numpy(case.grid.astype(np.float64)).requires_grad_(True)
    U, gt = (torch.from_numpy(a.reshape(-1, 3).astype(np.float64)) for a in (case.v_img, case.gt))
    cp = _torch_slice(Ct, g, shape, W, H)
    l1 = case.l1_weight * (cp - gt).abs().sum()
    ((U * cp).sum() + l1).backward()
    r = BR.case_bwd(case, guide64=True)
    clamped = float((~r.co.inside).mean())
    rel = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))
    figs = dict(fwd=rel(r.cprime, cp.detach().numpy()), v_rgb=rel(r.v_rgb, Ct.grad.numpy()),
                G=rel(r.G, g.grad.numpy().reshape(-1)), l1=abs(float(r.l1) - float(l1.detach())) / float(l1.detach()))
    val, grad = BR.tv(case.grid)
    gg = torch.from_numpy(case.grid.astype(np.float64)).requires_grad_(True)
    tv_t = sum(((gg.narrow(ax, 1, gg.shape[ax] - 1) - gg.narrow(ax, 0, gg.shape[ax] - 1)) ** 2).mean() for ax in (0, 1, 2))
    tv_t.backward()
    figs.update(tv=abs(float(val) - float(tv_t.detach())) / float(tv_t.detach()), tv_grad=rel(grad, gg.grad.numpy()))
    print(f"\nAUTOGRAD {W}x{H} {shape}: clamped {clamped:.3f}; relative differences {figs}")
    assert all(v <= 1e-10 for v in figs.values()), figs
    assert r.count == W * H
    # the fp32 guide moves the result by its own rounding only
    r32g = BR.case_bwd(case)
    assert rel(r32g.cprime, r.cprime) <= 1e-5 and rel(r32g.G, r.G) <= 1e-4


def test_identity_grid_is_exact_in_fp32():
    case = BR.make_case(33, 17, (5, 3, 4))
    got = BR.fwd(case.C, BR.identity_grid(case.shape), case.shape, 33, 17, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, case.C.reshape(-1, 3))


@pytest.mark.parametrize("W,H,shape", [(33, 17, (5, 3, 4)), (160, 120, (16, 16, 8)), (7, 3, (16, 16, 8))])
def test_builder(W, H, shape):
    case = BR.make_case(W, H, shape)
    assert case.C.min() >= -0.2 and case.C.max() <= 1.2
    co = BR.coords(W, H, shape, case.C)
    if W * H >= 400:
        lo, hi = float((co.luma <= 0).mean()), float((co.luma >= 1).mean())
        print(f"\nBUILDER {W}x{H}: clamped below {lo:.3f}, above {hi:.3f}")
        assert lo > 0 and hi > 0
    assert np.abs(case.grid - BR.identity_grid(shape)).max() <= 0.3 + 1e-6
    # smooth: per entry one sinusoid of at most one period along each axis, so a step between vertices is bounded by its slope
    for ax, G in ((0, shape[1]), (1, shape[0]), (2, shape[2])):
        assert np.abs(np.diff(case.grid, axis=ax)).max() <= 0.3 * 2 * np.pi / (G - 1) + 1e-6
    assert co.ix.min() >= 0 and co.ix.max() <= shape[0] - 2 and co.iz.min() >= 0 and co.iz.max() <= shape[2] - 2
    assert (co.fx >= 0).all() and (co.fx <= 1).all() and (co.fz >= 0).all() and (co.fz <= 1).all()
    c64 = BR.fwd(case.C, case.grid, shape, W, H)
    c32 = BR.fwd(case.C, case.grid, shape, W, H, np.float32)
    gt = case.gt.reshape(-1, 3).astype(np.float64)
    assert np.abs(c64 - gt).min() >= 1e-3 - 1e-6
    assert np.array_equal(np.sign(c64 - gt), np.sign(c32.astype(np.float64) - gt))
    if shape == (16, 16, 8) and W == 7:
        r = BR.case_bwd(case)
        assert not r.touched.all() and (r.G[~r.touched] == 0).all() and (r.mass[~r.touched] == 0).all()   # empty cells


def test_floors():
    from touch_gs_amd import _lib
    c = _lib.BILAGRID_CHUNK
    print()
    for shape in ((16, 16, 8), (2, 2, 2), (5, 3, 4)):
        for W, H in ((1, 1), (7, 3), (33, 17), (c - 1, 1), (c + 1, 1), (3 * c + 5, 1), (160, 120)):
            fl = BR.floors(BR.make_case(W, H, shape))
            print(f"FLOOR {str(shape):12s} {W:5d} x {H:3d}  " + "  ".join(f"{k} {v:6.3f}" for k, v in fl.items()) + "  (units of 2^-24 mass)")
            # a sanity bound on the reference, not a bar: the forward's unit sum |A C| + |b| does not hold the cancellation
            # inside a lerp (a = 0.25, b = -0.25 blend to A near 0 with the rounding of 0.25), hence a forward floor of 20
            assert all(v < 64 for v in fl.values()), "the fp32 evaluation itself is off: the reference or the masses are wrong"


def test_row_step_is_adam_with_tv():
    """adam_row_step is torch.optim.Adam on the grid with tv_weight * TV added to the loss."""
    shape = (3, 2, 2)
    GW, GH, L = shape
    n = BR.n_entries(shape)
    rng = np.random.default_rng(5)
    row = BR.new_row(shape)
    row[:n] += 0.1 * rng.standard_normal(n)
    g = torch.from_numpy(row[:n].copy()).requires_grad_(True)
    f = lambda x: float(np.float32(x))
    opt = torch.optim.Adam([g], lr=f(0.01), betas=(f(0.9), f(0.999)), eps=f(1e-15))
    for t in range(1, 6):
        G = rng.standard_normal(n)
        opt.zero_grad()
        gg = g.reshape(GH, GW, L, 12)
        tv_t = sum(((gg.narrow(ax, 1, gg.shape[ax] - 1) - gg.narrow(ax, 0, gg.shape[ax] - 1)) ** 2).mean() for ax in (0, 1, 2))
        (f(10.0) * tv_t + (g * torch.from_numpy(G)).sum()).backward()
        opt.step()
        row = BR.adam_row_step(row, shape, G, 0.01, tv_weight=10.0)
        np.testing.assert_allclose(row[:n], g.detach().numpy(), rtol=1e-10, atol=1e-13)
        assert row[3 * n] == t and abs(row[3 * n + 1] - f(0.9) ** t) < 1e-15 and (row[3 * n + 3:] == 0).all()


def test_reference_recovers():
    """The fp64 loop of the GPU recovery test ends below 25 % of its initial mean |C' - gt|."""
    Cc, gt, w = BR.recover_inputs()
    first, last, row = BR.recovery_loop(BR.ref_grad_fn(Cc, gt, w))
    print(f"\nRECOVER reference: L1 {first:.6f} -> {last:.6f} ({last / first:.3f}) after {BR.RECOVER['steps']} steps")
    assert last < 0.25 * first


# ---------------------------------------------------------------------------------------------
# BilagridSet
# ---------------------------------------------------------------------------------------------
def test_bilagrid_set_row_layout_schedule_and_files(tmp_path):
    from touch_gs_amd import _lib
    from touch_gs_amd.bilagrid import BilagridSet, from_gsplat, identity_grid, load_bilagrids, save_bilagrids, to_gsplat
    views = [object(), object(), object()]
    shape = (5, 3, 4)
    n = 3 * 5 * 4 * 12
    bs = BilagridSet(views, "cpu", lr=2e-3, shape=shape, max_steps=30000)
    assert bs.state.shape == (3, 3 * n + _lib.BILAGRID_TAIL) and bs.n == n
    assert np.array_equal(bs.state.numpy(), np.stack([BR.new_row(shape, np.float32)] * 3))
    assert np.array_equal(identity_grid(shape), BR.identity_grid(shape))
    assert bs.owns(views[1]) and not bs.owns(object()) and bs.row(views[2]).data_ptr() == bs.state[2].data_ptr()
    with pytest.raises(ValueError):
        BilagridSet(views, "cpu", shape=(5, 1, 4))
    # gsplat's schedule: 1 % at step 0, the full rate (times the decay so far) at the end of the warm-up, 1 % at the last step
    assert bs.lr_at(0) == pytest.approx(2e-5)
    assert bs.lr_at(1000) == pytest.approx(2e-3 * 0.01 ** (1000 / 30000))
    assert bs.lr_at(500) == pytest.approx(2e-3 * (0.01 + 0.99 * 0.5) * 0.01 ** (500 / 30000))
    assert bs.lr_at(30000) == pytest.approx(2e-5) and bs.lr_at(40000) == pytest.approx(2e-5)
    assert bs.adam(7) == dict(lr=bs.lr_at(7), betas=(0.9, 0.999), eps=1e-15)
    # files: gsplat's [12, L, GH, GW] per image name
    rng = np.random.default_rng(0)
    bs.state[:, :n] = torch.from_numpy(rng.standard_normal((3, n)).astype(np.float32))
    names = ["a.png", "b.png", "c.png"]
    path = save_bilagrids(str(tmp_path), bs, names)
    with np.load(path) as z:
        assert sorted(z.files) == names and z["b.png"].shape == (12, 4, 3, 5)
        g = bs.grid(views[1])
        assert g.shape == (3, 5, 4, 12)
        for e, l, y, x in ((0, 0, 0, 0), (7, 3, 2, 4), (11, 1, 1, 2)):
            assert z["b.png"][e, l, y, x] == g[y, x, l, e]
    back = load_bilagrids(path)
    assert all(np.array_equal(back[nm], bs.grid(v)) for nm, v in zip(names, views))
    assert np.array_equal(from_gsplat(to_gsplat(g)), g)
    sd = bs.state_dict()
    other = BilagridSet(views, "cpu", shape=shape)
    other.load_state_dict(sd)
    assert torch.equal(other.state, bs.state)
    with pytest.raises(ValueError):
        BilagridSet(views, "cpu", shape=(4, 3, 4)).load_state_dict(sd)
