"""CPU tests of the scale-invariant monocular depth loss (tgs_depth_corr_fwd_bwd): the entry point is declared, exported
and bound within TGS_VERSION 320; its argument validation runs before any launch; the fp64 reference the GPU tests compare
with (tests/depth_corr_ref.py) equals torch fp64 autograd of 1 - rho written from the definition, is invariant to an affine
map of the monocular depth, and gives zeros -- never NaN -- on degenerate frames; the Python surface above the kernel
(config, view, dataset, trainer flags) carries the map through."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests.depth_corr_ref import depth_corr_ref, synthetic_images, valid_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tgs_depth_corr_fwd_bwd"


def test_entry_point_is_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "prototype missing from include/tgs.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert len(args) == 12
    assert [a.split()[0] for a in args[:2]] == ["int", "int"] and args[5].startswith("float alpha_min") and args[6].startswith("float weight")
    assert hasattr(lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 12
    assert argtypes[5] is C.c_float and argtypes[6] is C.c_float and argtypes[0] is C.c_int
    assert lib.tgs_version() == 320
    # an addition: no struct grew, TgsLossSpec in particular
    assert C.sizeof(_lib.TgsLossSpec) == 3 * 8 + 4 * 4 and C.sizeof(_lib.TgsCamera) == 116 and C.sizeof(_lib.TgsRasterOpts) == 32
    # built from its own translation unit
    assert os.path.exists(os.path.join(ROOT, "touch_gs_amd", "csrc", "depthcorr.hip"))
    assert re.search(r'SRCS="[^"]*\bdepthcorr\b', open(os.path.join(ROOT, "touch_gs_amd", "csrc", "build.sh")).read())


def test_argument_validation_without_a_device():
    """TGS_E_ARG before any launch: NULL images / buffers, W or H < 1, alpha_min outside (0, 1] (NaN included).  The
    pointers are never dereferenced."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    fake = C.c_void_p(0x1000)

    def call(W=64, H=48, od=fake, fT=fake, mono=fake, amin=0.5, tiles=fake, stats=fake):
        return fn(W, H, od, fT, mono, C.c_float(amin), C.c_float(1.0), tiles, stats, fake, fake, None)

    for kw in (dict(od=None), dict(fT=None), dict(mono=None), dict(tiles=None), dict(stats=None)):
        assert call(**kw) == -1 and b"null" in lib.tgs_last_error(), (kw, lib.tgs_last_error())
    for kw in (dict(W=0), dict(H=0), dict(W=-3), dict(H=-1)):
        assert call(**kw) == -1 and b"image size" in lib.tgs_last_error(), (kw, lib.tgs_last_error())
    for amin in (0.0, -0.5, 1.0001, 2.0, float("nan"), float("inf")):
        assert call(amin=amin) == -1 and b"alpha_min" in lib.tgs_last_error(), (amin, lib.tgs_last_error())


def test_ops_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from touch_gs_amd import ops
    z = torch.zeros(48, 64)
    with pytest.raises(RuntimeError):      # no CPU path
        ops.depth_corr_fwd_bwd(z, z, z)
    with pytest.raises(ValueError):
        ops.depth_corr_fwd_bwd(z, z, torch.zeros(48, 65))
    with pytest.raises(ValueError):
        ops.depth_corr_fwd_bwd(torch.zeros(48, 64, 1), torch.zeros(48, 64, 1), torch.zeros(48, 64, 1))


def _torch_loss(od, fT, mono, alpha_min, weight):
    """weight * (1 - rho) from the definition, fp64 autograd leaves: depth_acc and alpha' = 1 - final_T."""
    valid = torch.from_numpy(valid_mask(fT, mono, alpha_min))
    d = torch.from_numpy(od.astype(np.float64)).requires_grad_(True)
    a = (1.0 - torch.from_numpy(fT.astype(np.float64))).requires_grad_(True)
    y = torch.from_numpy(mono.astype(np.float64))[valid]
    x = (d / torch.clamp(a, min=1e-10))[valid]
    dx, dy = x - x.mean(), y - y.mean()
    rho = (dx * dy).mean() / torch.sqrt((dx * dx).mean() * (dy * dy).mean())
    loss = weight * (1 - rho)
    loss.backward()
    return float(loss.detach()), float(rho.detach()), d.grad.numpy(), a.grad.numpy()


@pytest.mark.parametrize("W,H,rel_noise", [(16, 16, 0.3), (157, 93, 0.1), (157, 93, 1e-3), (320, 208, 0.3)])
def test_reference_gradients_equal_torch_fp64_autograd(W, H, rel_noise):
    od, fT, mono = synthetic_images(W, H, rel_noise, seed=11)
    weight = 0.7
    ref = depth_corr_ref(od, fT, mono, 0.5, weight)
    loss, rho, gd, ga = _torch_loss(od, fT, mono, 0.5, weight)
    assert abs(ref["stats"][6] - rho) <= 1e-12 and abs(ref["stats"][7] - loss) <= 1e-12
    assert ref["stats"][0] == ref["valid"].sum() and 0.5 * W * H < ref["stats"][0] < 0.9 * W * H
    scale = max(np.abs(gd).max(), np.abs(ga).max())
    assert np.abs(ref["v_depth"] - gd).max() <= 1e-10 * scale
    assert np.abs(ref["v_alpha"] - ga).max() <= 1e-10 * scale
    inv = ~ref["valid"]
    assert (ref["v_depth"][inv] == 0).all() and (ref["v_alpha"][inv] == 0).all() and (gd[inv] == 0).all()
    # the gradient scale bounds the gradient itself (it is the sum of the magnitudes of its terms)
    v = ref["valid"]
    assert (np.abs(ref["v_depth"][v]) * ref["alpha"][v] <= ref["scale"][v] * (1 + 1e-12)).all()


def test_reference_loss_is_invariant_to_an_affine_map_of_the_monocular_depth():
    od, fT, mono = synthetic_images(157, 93, 0.1, seed=5)
    base = depth_corr_ref(od, fT, mono, 0.5, 1.0)
    for a, b in ((1.0, 0.0), (3.0, 0.5), (1000.0, 250.0), (0.01, 2.0)):
        m2 = np.where(mono > 0, a * mono.astype(np.float64) + b, 0.0)
        m2_32 = m2.astype(np.float32)
        # the fp32 rounding of the mapped image is an input perturbation of ~6e-8 relative, not part of the invariance
        r = depth_corr_ref(od, fT, m2_32, 0.5, 1.0)
        assert np.array_equal(r["valid"], base["valid"])
        assert abs(r["stats"][7] - base["stats"][7]) <= 1e-6, (a, b)
    for a in (4.0, 0.25):       # exact in fp32: the gradient images do not move either
        r = depth_corr_ref(od, fT, (np.float32(a) * mono).astype(np.float32), 0.5, 1.0)
        assert np.abs(r["v_depth"] - base["v_depth"]).max() <= 1e-10 * np.abs(base["v_depth"]).max()
        assert np.abs(r["v_alpha"] - base["v_alpha"]).max() <= 1e-10 * np.abs(base["v_alpha"]).max()
    neg = depth_corr_ref(od, fT, np.where(mono > 0, 10.0 - mono, 0.0).astype(np.float32), 0.5, 1.0)
    assert abs(neg["stats"][6] + base["stats"][6]) <= 1e-6     # a NEGATIVE scale flips the sign: a > 0 is part of the claim


def test_reference_degenerate_frames_give_zeros_and_no_nan():
    od, fT, mono = synthetic_images(64, 48, 0.1, seed=2)
    one = np.zeros_like(mono)
    ok = np.argwhere(valid_mask(fT, mono, 0.5))[7]
    one[ok[0], ok[1]] = mono[ok[0], ok[1]]
    fT_const = np.where(fT < 0.45, np.float32(0.0), np.float32(1.0)).astype(np.float32)     # alpha 1 or 0: x = 1.25 exactly
    cases = {"no map": (od, fT, np.zeros_like(mono), 0), "one pixel": (od, fT, one, 1),
             "constant depth": (np.float32(1.25) * (1 - fT_const), fT_const, mono, None),
             "constant map": (od, fT, np.where(mono > 0, np.float32(3.0), np.float32(0.0)), None)}
    for name, (d, T, m, n) in cases.items():
        r = depth_corr_ref(d, T, m, 0.5, 0.3)
        assert r["stats"][6] == 0 and r["stats"][7] == 0, name
        assert np.isfinite(r["stats"]).all() and (r["v_depth"] == 0).all() and (r["v_alpha"] == 0).all(), name
        assert r["stats"][0] == (valid_mask(T, m, 0.5).sum() if n is None else n), name


def test_config_view_and_trainer_carry_the_term_and_default_to_off(tmp_path):
    from touch_gs_amd import Camera
    from touch_gs_amd.model import ModelConfig, View
    cfg = ModelConfig()
    assert cfg.mono_depth_mult == 0.0 and cfg.mono_depth_alpha_min == 0.5
    # a checkpoint written before the fields existed records a config without them: they take their defaults
    old = {k: v for k, v in dataclasses.asdict(cfg).items() if not k.startswith("mono_depth")}
    assert ModelConfig(**old) == cfg
    H, W = 12, 20
    mono = torch.arange(H * W, dtype=torch.float32).reshape(H, W)
    v = View(cam=Camera(np.eye(4), 50.0, 50.0, W / 2, H / 2, W, H), rgb=torch.zeros(H, W, 3), mono_depth=mono)
    assert View(cam=v.cam, rgb=v.rgb).mono_depth is None
    half = v.downscaled(2)
    assert half.mono_depth.shape == (H // 2, W // 2)
    assert torch.equal(half.mono_depth, mono[::2, ::2])       # nearest neighbour, like depth: no value is invented
    src = open(os.path.join(ROOT, "touch_gs_amd", "train.py")).read()
    for flag in ("--mono-depth-dir", "--mono-depth-mult", "--mono-depth-alpha-min"):
        assert flag in src


def test_scene_reads_png_and_npy_monocular_maps(tmp_path):
    import json
    from PIL import Image
    from touch_gs_amd.dataset import Scene
    from touch_gs_amd.plumbing import write_png16
    H, W = 24, 32
    root = tmp_path / "scene"
    (root / "imgs").mkdir(parents=True)
    (root / "zoe_depth").mkdir()
    frames = []
    for i in range(5):
        Image.fromarray(np.full((H, W, 3), 40 * i, np.uint8)).save(root / "imgs" / f"{i:04d}.png")
        c2w = np.eye(4)
        c2w[0, 3] = i
        frames.append(dict(file_path=f"imgs/{i:04d}.png", transform_matrix=c2w.tolist()))
    json.dump(dict(fl_x=30.0, fl_y=30.0, cx=W / 2, cy=H / 2, w=W, h=H, frames=frames), open(root / "transforms.json", "w"))
    png = (np.arange(H * W).reshape(H, W) * 7 % 60000).astype(np.uint16)
    write_png16(str(root / "zoe_depth" / "0000.png"), png)
    npy = np.random.default_rng(0).random((H // 2, W // 2)).astype(np.float32) + 0.5     # other size: resized to the image
    np.save(root / "zoe_depth" / "0001.npy", npy)
    s = Scene(str(root), 0.8, "cpu", mono_depth_dir="zoe_depth")
    assert torch.equal(s.views[0].mono_depth, torch.from_numpy(png.astype(np.float32)))      # raw values: no unit conversion
    assert s.views[1].mono_depth.shape == (H, W) and s.views[1].mono_depth.dtype == torch.float32
    assert abs(float(s.views[1].mono_depth.mean()) - float(npy.mean())) < 0.02
    assert s.views[2].mono_depth is None
    assert s.describe()["mono_depth_dir"] == "zoe_depth" and s.describe()["mono_depth_views"] == 2
    assert all(v.mono_depth is None for v in Scene(str(root), 0.8, "cpu").views)
