"""CPU tests of the depth-derived normals and the normal-prior loss (tgs_depth_normal_fwd_bwd): the entry point is
declared, exported and bound within TGS_VERSION 320 and validates its arguments before any launch; the fp64 reference the GPU
tests compare with (tests/depth_normal_ref.py) has the gradient its loss has (central finite differences), gives the
hand-computed values on the gate and degenerate cases, and an fp32 emulation of the kernels' arithmetic stays within 2 units
of the condition numbers the GPU bounds are stated in; the Python surface above the kernel carries the prior through.

What fixes the GPU bounds: over the seven synthetic cases (seed 1, alpha_min 0.5, max_jump 0.1) the straightforward fp32
transcription of the kernels (depth_normal_emulated) differs from the fp64 reference by at most 0.46 kappa_i 2^-24 on a
normal and 0.37 S_j 2^-24 on G.  The GPU bounds are 16 units each: about 35 x the emulation, for contraction, a different
division / square root and a different summation order (kappa >= 2 always, so a few ulp of the normalisation are inside it).
This test holds the emulation under 2 units so that the bound cannot drift."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.depth_normal_ref import (CASES, UNIT, assert_margins, camera, decisions, depth_normal_emulated, depth_normal_ref,
                                    loss_fp64, synthetic)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tgs_depth_normal_fwd_bwd"
_CACHE = {}


def _case(W, H, fx):
    if (W, H, fx) not in _CACHE:
        s = synthetic(W, H, 1, fx)
        assert_margins(s["out_depth"], s["final_T"], 0.5, 0.1)
        ref = depth_normal_ref(s["cam"], s["out_depth"], s["final_T"], s["prior"], s["conf"], 0.5, 0.1, 0.7)
        _CACHE[(W, H, fx)] = (s, ref)
    return _CACHE[(W, H, fx)]


def test_entry_point_is_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "prototype missing from include/tgs.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert len(args) == 15
    assert args[0].startswith("const TgsCamera*") and args[5].startswith("float alpha_min") and args[6].startswith("float max_jump")
    assert args[7].startswith("float weight") and args[13].startswith("int accumulate")
    assert hasattr(lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 15
    assert argtypes[5] is argtypes[6] is argtypes[7] is C.c_float and argtypes[13] is C.c_int
    assert lib.tgs_version() == 320
    # an addition: no struct grew
    assert C.sizeof(_lib.TgsLossSpec) == 3 * 8 + 4 * 4 and C.sizeof(_lib.TgsCamera) == 116 and C.sizeof(_lib.TgsRasterOpts) == 32
    assert os.path.exists(os.path.join(ROOT, "touch_gs_amd", "csrc", "depthnormal.hip"))
    assert re.search(r'SRCS="[^"]*\bdepthnormal\b', open(os.path.join(ROOT, "touch_gs_amd", "csrc", "build.sh")).read())


def test_argument_validation_without_a_device():
    """TGS_E_ARG before any launch; the pointers are never dereferenced."""
    from touch_gs_amd import _lib
    from touch_gs_amd.camera import Camera
    lib = _lib.load()
    fn = getattr(lib, NAME)
    fake = C.c_void_p(0x1000)

    def call(cam="ok", W=64, H=48, fx=50.0, od=fake, fT=fake, prior=fake, conf=fake, amin=0.5, jump=0.1, weight=1.0, tiles=fake,
             stats=fake, acc=0):
        cs = Camera(np.eye(4), fx, 50.0, 32.0, 24.0, W, H).c_struct()
        return fn(C.byref(cs) if cam == "ok" else None, od, fT, prior, conf, C.c_float(amin), C.c_float(jump), C.c_float(weight),
                  tiles, stats, fake, fake, fake, acc, None)

    assert call(cam=None) == -1 and b"camera" in lib.tgs_last_error()
    for kw in (dict(od=None), dict(fT=None), dict(tiles=None), dict(stats=None)):
        assert call(**kw) == -1 and b"null" in lib.tgs_last_error(), (kw, lib.tgs_last_error())
    assert call(prior=None) == -1 and b"conf without a prior" in lib.tgs_last_error()
    for kw in (dict(W=0), dict(H=0), dict(W=-3)):
        assert call(**kw) == -1 and b"image size" in lib.tgs_last_error(), (kw, lib.tgs_last_error())
    for fx in (0.0, -1.0, float("nan"), float("inf")):
        assert call(fx=fx) == -1 and b"intrinsics" in lib.tgs_last_error(), fx
    for amin in (0.0, -0.5, 1.0001, float("nan")):
        assert call(amin=amin) == -1 and b"alpha_min" in lib.tgs_last_error(), amin
    assert call(jump=float("nan")) == -1 and b"max_jump" in lib.tgs_last_error()
    assert call(weight=float("inf")) == -1 and b"weight" in lib.tgs_last_error()
    assert call(acc=2) == -1 and b"accumulate" in lib.tgs_last_error()
    assert call(tiles=C.c_void_p(0x1004)) == -1 and b"aligned" in lib.tgs_last_error()


def test_the_reference_gradient_equals_central_finite_differences():
    """G of the definition against finite differences of L in fp64 on a 24x20 case with every gate engaged: invalid pixels,
    a depth step the jump gate cuts, zero priors, zero weights.  The supervised set and C are held constant, as specified."""
    s = synthetic(24, 20, 4, 30.0)
    ref = depth_normal_ref(s["cam"], s["out_depth"], s["final_T"], s["prior"], s["conf"], 0.5, 0.1, 0.7)
    sup, formed, valid = ref["supervised"], ref["formed"], ref["valid"]
    _, cand_nogate, _ = decisions(s["out_depth"], s["final_T"], 0.5, 0.0)
    assert (~valid).sum() > 5 and (cand_nogate & ~formed).sum() > 5 and (formed & ~sup).sum() > 5 and sup.sum() > 50
    od = s["out_depth"].astype(np.float64)
    a = (np.float32(1) - s["final_T"]).astype(np.float64)
    L = lambda od_, a_: loss_fp64(s["cam"], od_, a_, sup, ref["phat"], ref["c"], 0.7)
    assert abs(L(od, a) - ref["stats"][4]) <= 1e-14
    rng = np.random.default_rng(0)
    fed = np.argwhere(ref["S"] > 0)
    scale = np.abs(ref["v_depth"]).max()
    worst = 0.0
    for iy, ix in fed[rng.choice(len(fed), 40, replace=False)]:
        for img, want in ((0, ref["v_depth"][iy, ix]), (1, ref["v_alpha"][iy, ix])):
            h = 1e-6
            p, q = [od.copy(), a.copy()], [od.copy(), a.copy()]
            p[img][iy, ix] += h
            q[img][iy, ix] -= h
            fd = (L(*p) - L(*q)) / (2 * h)
            worst = max(worst, abs(fd - want) / scale)
    print(f"[depth_normal FD] max |fd - analytic| / max |v_depth| = {worst:.2e}")
    assert worst <= 1e-6
    # a pixel that feeds no supervised centre has no gradient at all
    assert not ref["v_depth"][ref["S"] == 0].any() and not ref["v_alpha"][ref["S"] == 0].any()


def _plane(W=12, H=10, depth=1.5, alpha=1.0):
    cam = camera(W, H, 25.0)
    fT = np.full((H, W), 1.0 - alpha, np.float32)
    od = (np.float32(depth) * (np.float32(1) - fT)).astype(np.float32)
    return cam, od, fT


def test_gates_and_degenerate_cases_against_hand_computed_values():
    W, H = 12, 10
    cam, od, fT = _plane(W, H)
    prior = np.zeros((H, W, 3), np.float32)
    prior[..., 2] = -3.0
    interior = (W - 2) * (H - 2)
    for fn in (depth_normal_ref, depth_normal_emulated):
        # a plane at constant depth: (0, 0, -1) exactly on every interior pixel, loss 0 against that prior, no gradient
        r = fn(cam, od, fT, prior, None, 0.5, 0.1, 0.7)
        n = r["normals"]
        assert r["stats"][0] == interior and r["stats"][1] == interior and r["stats"][2] == interior
        assert (n[1:-1, 1:-1] == np.array([0.0, 0.0, -1.0])).all()
        assert not n[0].any() and not n[-1].any() and not n[:, 0].any() and not n[:, -1].any()
        assert r["stats"][3] == 0 and r["stats"][4] == 0 and not r["G"].any()
        # the opposite prior: 1 - cos = 2 everywhere, loss = 2 weight; the gradient still vanishes (g_n is parallel to n)
        r = fn(cam, od, fT, -prior, None, 0.5, 0.1, 0.7)
        assert abs(r["stats"][3] - 2.0) <= 1e-6 and abs(r["stats"][4] - 1.4) <= 1e-6 and np.abs(r["G"]).max() <= 1e-9
        # no prior, a prior of length 0, conf all 0: formed, but nothing supervised
        for p, c in ((None, None), (np.zeros_like(prior), None), (prior, np.zeros((H, W), np.float32))):
            r = fn(cam, od, fT, p, c, 0.5, 0.1, 0.7)
            assert r["stats"][0] == interior and not r["stats"][1:].any() and not r["G"].any(), (p is None, c is None)
        # alpha below alpha_min everywhere: nothing formed
        cam2, od2, fT2 = _plane(W, H, alpha=0.25)
        r = fn(cam2, od2, fT2, prior, None, 0.5, 0.1, 0.7)
        assert not r["stats"].any() and not r["normals"].any() and not r["G"].any()
        # one invalid pixel takes out itself and its four neighbours
        fT3 = fT.copy()
        fT3[4, 5] = 0.9
        r = fn(cam, od * (1 - fT3), fT3, prior, None, 0.5, 0.1, 0.7)
        assert r["stats"][0] == interior - 5
        assert not r["formed"][4, 4:7].any() and not r["formed"][3:6, 5].any() and r["formed"][3, 4] and r["formed"][5, 6]
        # a depth step of 0.3 between columns 5 and 6 at depth 1.5: |x_r - x_l| = 0.3 > 0.1 * 1.5 on the two columns whose
        # horizontal difference straddles it (and > 0.1 * 1.2); max_jump 0.3 (thresholds 0.45 and 0.36) and max_jump <= 0
        # let them through
        od4 = od.copy()
        od4[:, 6:] = np.float32(1.2)
        r = fn(cam, od4, fT, prior, None, 0.5, 0.1, 0.7)
        assert r["stats"][0] == interior - 2 * (H - 2) and not r["formed"][:, 5:7].any()
        assert (r["normals"][1:-1, 1:5] == np.array([0.0, 0.0, -1.0])).all()
        for jump in (0.3, 0.0, -1.0):
            r = fn(cam, od4, fT, prior, None, 0.5, jump, 0.7)
            assert r["stats"][0] == interior and r["stats"][3] > 0.01
    # an image too small to have an interior pixel
    cam1, od1, fT1 = _plane(2, 7)
    r = depth_normal_ref(cam1, od1, fT1, None, None)
    assert not r["stats"].any()


def test_a_tilted_plane_gives_its_analytic_normal():
    """Depth of the plane n0 . X = d along every ray: z = d / (n0 . r).  The reference's normal is +-n0 facing the camera."""
    W, H = 20, 16
    cam = camera(W, H, 30.0)
    n0 = np.array([0.3, -0.2, -0.933])
    n0 /= np.linalg.norm(n0)
    from tests.depth_normal_ref import _rays
    z = -1.4 / (_rays(cam) @ n0)
    assert z.min() > 0.5
    fT = np.zeros((H, W), np.float32)
    r = depth_normal_ref(cam, z.astype(np.float32), fT, None, None, 0.5, 0.0)
    err = np.abs(r["normals"][1:-1, 1:-1] - n0).max()
    assert r["stats"][0] == (W - 2) * (H - 2) and err <= 2e-5, err     # (fp32 storage of the depth, times kappa)


@pytest.mark.parametrize("W,H,fx", CASES)
def test_fp32_emulation_stays_within_two_units_of_the_reference(W, H, fx):
    s, ref = _case(W, H, fx)
    emu = depth_normal_emulated(s["cam"], s["out_depth"], s["final_T"], s["prior"], s["conf"], 0.5, 0.1, 0.7)
    assert (emu["formed"] == ref["formed"]).all() and (emu["supervised"] == ref["supervised"]).all()
    f, fed = ref["formed"], ref["S"] > 0
    assert ref["kappa"][f].min() >= 2
    en = (np.abs(emu["normals"].astype(np.float64) - ref["normals"]).max(-1)[f] / (ref["kappa"][f] * UNIT)).max()
    eg = (np.abs(emu["G"].astype(np.float64) - ref["G"])[fed] / (ref["S"][fed] * UNIT)).max()
    print(f"[depth_normal emulation {W}x{H} fx {fx}] formed {int(ref['stats'][0])} of {W * H}, supervised {int(ref['stats'][1])}; "
          f"normals {en:.2f} units of kappa 2^-24, G {eg:.2f} units of S 2^-24 (bound 2; GPU bound 16)")
    assert en <= 2 and eg <= 2
    assert not emu["G"][~fed].any() and not emu["normals"][~f].any()
    assert abs(emu["stats"][2] - ref["stats"][2]) <= 1e-6 * ref["stats"][2]
    assert abs(emu["stats"][4] - ref["stats"][4]) <= 1e-6 * ref["stats"][4]


def test_synthetic_counts_do_not_depend_on_a_rounding():
    """Formed centres and centres cut by the jump gate of the specification's table; the margins hold for every case."""
    table = {(16, 16): (139, 28), (17, 19): (191, 28), (157, 93): (13298, 288), (1280, 720): (880259, 2288)}
    for W, H, fx in CASES:
        s, ref = _case(W, H, fx)
        _, cand_nogate, _ = decisions(s["out_depth"], s["final_T"], 0.5, 0.0)
        formed, cut = int(ref["stats"][0]), int(cand_nogate.sum()) - int(ref["stats"][0])
        assert 0 < ref["stats"][1] < formed and cut > 0
        if (W, H) in table:
            assert (formed, cut) == table[(W, H)], (W, H, formed, cut)


def test_python_surface_carries_the_prior():
    from touch_gs_amd.camera import Camera
    from touch_gs_amd.model import ModelConfig, View
    c = ModelConfig()
    assert (c.normal_prior_mult, c.normal_alpha_min, c.normal_max_jump) == (0.0, 0.5, 0.1)
    H, W = 8, 12
    prior = torch.zeros(H, W, 3)
    prior[..., 0] = torch.arange(W)[None, :].float()
    prior[..., 1] = torch.arange(H)[:, None].float()
    conf = torch.arange(H * W).float().view(H, W)
    v = View(cam=Camera(np.eye(4), 10.0, 10.0, 6.0, 4.0, W, H), rgb=torch.rand(H, W, 3), normal_prior=prior, normal_conf=conf)
    d = v.downscaled(2)
    assert d.normal_prior.shape == (4, 6, 3) and d.normal_conf.shape == (4, 6)
    # nearest neighbour: every value is one of the original's, none is a blend
    assert torch.equal(d.normal_prior[..., 0], prior[::2, ::2, 0]) and torch.equal(d.normal_prior[..., 1], prior[::2, ::2, 1])
    assert torch.equal(d.normal_conf, conf[::2, ::2])
    assert View(cam=v.cam, rgb=v.rgb).downscaled(2).normal_prior is None


def test_normal_maps_are_read_flipped_and_resized_by_nearest_neighbour(tmp_path):
    from PIL import Image
    from touch_gs_amd.dataset import read_normal_map
    H, W = 6, 8
    rng = np.random.default_rng(2)
    n = rng.standard_normal((H, W, 3)).astype(np.float32)
    conf = rng.random((H, W)).astype(np.float32)
    np.save(tmp_path / "a.npy", n)
    np.save(tmp_path / "a_conf.npy", conf)
    got, c = read_normal_map(str(tmp_path / "a"), H, W)
    assert got.dtype == np.float32 and (got == n).all() and (c == conf).all()
    gl, _ = read_normal_map(str(tmp_path / "a"), H, W, "opengl")
    assert (gl == n * np.array([1, -1, -1], np.float32)).all()
    half, ch = read_normal_map(str(tmp_path / "a"), H // 2, W // 2)
    assert (half == n[::2, ::2]).all() and (ch == conf[::2, ::2]).all()      # every value is one of the original's
    # PNG: n = 2 v / 255 - 1, a black pixel is "no prior"; the encoding train.render_views writes
    v = np.zeros((H, W, 3), np.uint8)
    v[..., 2] = 255
    v[0, 0] = 0
    v[1, 1] = (255, 128, 0)
    Image.fromarray(v).save(tmp_path / "b.png")
    png, c = read_normal_map(str(tmp_path / "b"), H, W)
    assert c is None and (png[2, 2] == np.array([-1.0, -1.0, 1.0], np.float32)).all() and not png[0, 0].any()
    assert np.allclose(png[1, 1], [1.0, 2 * 128 / 255 - 1, -1.0], atol=1e-6)
    assert read_normal_map(str(tmp_path / "missing"), H, W) == (None, None)
    np.save(tmp_path / "bad.npy", np.zeros((H, W), np.float32))
    with pytest.raises(ValueError):
        read_normal_map(str(tmp_path / "bad"), H, W)


def test_trainer_and_eval_flags_exist():
    import inspect
    from touch_gs_amd import run_eval, train
    src = inspect.getsource(train.main)
    for flag in ("--normal-dir", "--normal-frame", "--normal-mult", "--normal-max-jump", "--eval-normals"):
        assert f'"{flag}"' in src, flag
    assert "normal_prior_mult=args.normal_mult" in src and "normal_max_jump=args.normal_max_jump" in src
    assert '"--normals"' in inspect.getsource(run_eval.main)
    assert "normals" in inspect.signature(train.evaluate).parameters and "normals" in inspect.signature(train.render_views).parameters
    assert "normals" in inspect.signature(run_eval.eval_run).parameters
