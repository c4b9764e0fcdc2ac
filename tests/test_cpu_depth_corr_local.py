"""CPU tests of the patch-wise (local) Pearson term for raw monocular depth (tgs_depth_corr_local_fwd_bwd): the
entry point is declared, exported and bound within TGS_VERSION 320 beside the unchanged global one; its argument validation
runs before any launch; the fp64 reference the GPU tests compare with (tests/depth_corr_local_ref.py) equals torch fp64
autograd of the written-out definition with the gates held fixed, and rho_bar and every rho_p are invariant under a DIFFERENT
positive affine map of the monocular depth in every patch, which the global rho is not; config, trainer flags and checkpoint
defaults carry the fields, and off is the default."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from tests.depth_corr_local_ref import depth_corr_local_ref, min_count_of, patch_grid
from tests.depth_corr_ref import synthetic_images, valid_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tgs_depth_corr_local_fwd_bwd"
OLD = "tgs_depth_corr_fwd_bwd"


def _prototype_args(txt, name):
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, f"prototype of {name} missing from include/tgs.h"
    return [a.strip() for a in " ".join(m.group(1).split()).split(",")]


def test_entry_point_is_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    args = _prototype_args(txt, NAME)
    assert len(args) == 19
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names == ["W", "H", "out_depth", "final_T", "mono", "alpha_min", "weight_global", "weight_local", "patch_tiles",
                     "off_x", "off_y", "min_count", "min_var_ratio", "tile_moments", "patch_stats", "stats", "v_depth",
                     "v_alpha", "stream"]
    assert hasattr(lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 19
    assert [argtypes[i] for i in (5, 6, 7, 12)] == [C.c_float] * 4
    assert [argtypes[i] for i in (0, 1, 8, 9, 10, 11)] == [C.c_int] * 6
    assert lib.tgs_version() == 320
    assert C.sizeof(_lib.TgsLossSpec) == 3 * 8 + 4 * 4 and C.sizeof(_lib.TgsCamera) == 116 and C.sizeof(_lib.TgsRasterOpts) == 32
    # the existing entry point keeps its 12 arguments
    assert len(_prototype_args(txt, OLD)) == 12 and len(_lib.SIGNATURES[OLD][1]) == 12


GOOD = dict(W=64, H=48, od=0x1000, fT=0x1000, mono=0x1000, amin=0.5, k=2, ox=0, oy=0, min_count=2, ratio=1e-3, tiles=0x1000,
            patches=0x1000, stats=0x1000)
BAD = [
    (dict(od=None), b"null"), (dict(fT=None), b"null"), (dict(mono=None), b"null"), (dict(tiles=None), b"null"),
    (dict(patches=None), b"null"), (dict(stats=None), b"null"),
    (dict(W=0), b"image size"), (dict(H=0), b"image size"), (dict(W=-3), b"image size"),
    (dict(amin=0.0), b"alpha_min"), (dict(amin=1.0001), b"alpha_min"), (dict(amin=float("nan")), b"alpha_min"),
    (dict(k=0), b"patch_tiles"), (dict(k=17), b"patch_tiles"), (dict(k=-1), b"patch_tiles"),
    (dict(ox=2), b"offset"), (dict(oy=2), b"offset"), (dict(ox=-1), b"offset"), (dict(oy=-1), b"offset"),
    (dict(min_count=1), b"min_count"), (dict(min_count=0), b"min_count"), (dict(min_count=-5), b"min_count"),
    (dict(ratio=-1e-3), b"min_var_ratio"), (dict(ratio=float("nan")), b"min_var_ratio"), (dict(ratio=float("inf")), b"min_var_ratio"),
    (dict(tiles=0x1004), b"aligned"), (dict(patches=0x1008), b"aligned"), (dict(stats=0x100c), b"aligned"),
]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{list(k)[0]}={list(k.values())[0]}" for k, _ in BAD])
def test_argument_validation_without_a_device(kw, word):
    """TGS_E_ARG before any launch, one case per rule; the fake pointers are never dereferenced."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    a = dict(GOOD, **kw)
    p = lambda v: None if v is None else C.c_void_p(v)
    rc = getattr(lib, NAME)(a["W"], a["H"], p(a["od"]), p(a["fT"]), p(a["mono"]), C.c_float(a["amin"]), C.c_float(1.0),
                            C.c_float(1.0), a["k"], a["ox"], a["oy"], a["min_count"], C.c_float(a["ratio"]), p(a["tiles"]),
                            p(a["patches"]), p(a["stats"]), C.c_void_p(0x1000), C.c_void_p(0x1000), None)
    assert rc == -1 and word in lib.tgs_last_error(), (kw, lib.tgs_last_error())


def test_ops_wrapper_refuses_cpu_tensors_wrong_shapes_and_bad_grids():
    from touch_gs_amd import ops
    z = torch.zeros(48, 64)
    with pytest.raises(RuntimeError):      # no CPU path
        ops.depth_corr_local_fwd_bwd(z, z, z)
    with pytest.raises(ValueError):
        ops.depth_corr_local_fwd_bwd(z, z, torch.zeros(48, 65))
    with pytest.raises(ValueError):
        ops.depth_corr_local_fwd_bwd(z, z, z, patch_tiles=17)
    with pytest.raises(ValueError):
        ops.depth_corr_local_fwd_bwd(z, z, z, patch_tiles=2, offset=(2, 0))
    assert ops.depth_corr_patch_min_count(8, 0.25) == 4096 == min_count_of(8, 0.25)
    assert ops.depth_corr_patch_min_count(1, 0.001) == 2 and ops.depth_corr_patch_min_count(2, 0.3) == 308


def _torch_loss(od, fT, mono, alpha_min, wg, wl, pid, active):
    """wg (1 - rho) + wl (1 - mean of rho_p over ``active``) from the definition; fp64 autograd leaves depth_acc and
    alpha' = 1 - final_T; the set of active patches is given (the gates are constants)."""
    valid = torch.from_numpy(valid_mask(fT, mono, alpha_min))
    d = torch.from_numpy(od.astype(np.float64)).requires_grad_(True)
    a = (1.0 - torch.from_numpy(fT.astype(np.float64))).requires_grad_(True)
    y = torch.from_numpy(mono.astype(np.float64))
    x = d / torch.clamp(a, min=1e-10)
    pid = torch.from_numpy(pid)

    def rho_of(sel):
        xs, ys = x[sel], y[sel]
        dx, dy = xs - xs.mean(), ys - ys.mean()
        return (dx * dy).mean() / torch.sqrt((dx * dx).mean() * (dy * dy).mean())
    rho = rho_of(valid)
    rhos = [rho_of(valid & (pid == int(p))) for p in np.flatnonzero(active)]
    rho_bar = sum(rhos) / len(rhos)
    loss = wg * (1 - rho) + wl * (1 - rho_bar)
    loss.backward()
    return float(loss.detach()), float(rho_bar.detach()), d.grad.numpy(), a.grad.numpy()


@pytest.mark.parametrize("off", [(0, 0), (1, 1)])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("W,H", [(48, 32), (157, 93)])
def test_reference_gradients_equal_torch_fp64_autograd(W, H, k, off):
    if off[0] >= k:
        off = (0, 0)        # (k = 1 has the one alignment)
    od, fT, mono = synthetic_images(W, H, 0.1, seed=11)
    wg, wl = 0.7, 0.4
    ref = depth_corr_local_ref(od, fT, mono, 0.5, wg, wl, k, off, min_count_of(k, 0.25), 1e-3)
    assert ref["active"].sum() >= 2 and ref["stats"][9] == ref["active"].sum()
    assert ref["n"].sum() == ref["valid"].sum()            # every valid pixel is in exactly one patch
    loss, rho_bar, gd, ga = _torch_loss(od, fT, mono, 0.5, wg, wl, ref["pid"], ref["active"])
    assert abs(ref["stats"][10] - rho_bar) <= 1e-12 and abs(ref["stats"][12] - loss) <= 1e-12
    scale = max(np.abs(gd).max(), np.abs(ga).max())
    assert np.abs(ref["v_depth"] - gd).max() <= 1e-10 * scale
    assert np.abs(ref["v_alpha"] - ga).max() <= 1e-10 * scale
    inv = ~ref["valid"]
    assert (ref["v_depth"][inv] == 0).all() and (ref["v_alpha"][inv] == 0).all()
    v = ref["valid"]
    assert (np.abs(ref["v_depth"][v]) * ref["alpha"][v] <= ref["scale"][v] * (1 + 1e-12)).all()


def test_local_correlation_is_invariant_to_a_different_affine_map_in_every_patch_and_the_global_one_is_not():
    W, H, k, off = 157, 93, 2, (1, 1)
    od, fT, mono = synthetic_images(W, H, 0.1, seed=5)
    mc = min_count_of(k, 0.25)
    # min_var_ratio 0: the variance gate compares with the GLOBAL variance of the map, which a per-patch map changes
    base = depth_corr_local_ref(od, fT, mono, 0.5, 1.0, 1.0, k, off, mc, 0.0)
    PW, PH, pid = patch_grid(W, H, k, off)
    rng = np.random.default_rng(0)
    a, b = rng.uniform(0.5, 20.0, PW * PH), rng.uniform(0.0, 5.0, PW * PH)
    m2 = np.where(mono > 0, a[pid] * mono.astype(np.float64) + b[pid], 0.0).astype(np.float32)
    r = depth_corr_local_ref(od, fT, m2, 0.5, 1.0, 1.0, k, off, mc, 0.0)
    assert np.array_equal(r["valid"], base["valid"]) and np.array_equal(r["active"], base["active"]) and base["active"].sum() >= 6
    # (the fp32 rounding of the mapped image is an input perturbation of ~6e-8 relative, not part of the invariance)
    assert np.abs(r["rho"] - base["rho"]).max() <= 1e-6
    assert abs(r["stats"][10] - base["stats"][10]) <= 1e-6
    assert abs(r["stats"][6] - base["stats"][6]) > 0.05          # the global rho moved


def test_reference_gates_and_degenerate_frames():
    W, H, k = 64, 48, 2
    od, fT, mono = synthetic_images(W, H, 0.1, seed=2)
    full = depth_corr_local_ref(od, fT, mono, 0.5, 0.3, 0.2, k, (0, 0), 2, 0.0)
    assert full["active"].all() and full["stats"][8] == full["stats"][9] == 4
    # a count no patch reaches: nothing counted, local loss 0, the gradient is the global one
    none = depth_corr_local_ref(od, fT, mono, 0.5, 0.3, 0.2, k, (0, 0), 32 * 32 + 1, 0.0)
    glob = depth_corr_local_ref(od, fT, mono, 0.5, 0.3, 0.0, k, (0, 0), 2, 0.0)
    assert none["stats"][8] == none["stats"][9] == none["stats"][10] == none["stats"][11] == 0
    assert none["stats"][12] == none["stats"][7] and np.array_equal(none["v_depth"], glob["v_depth"])
    # a ratio no patch reaches
    flat = depth_corr_local_ref(od, fT, mono, 0.5, 0.3, 0.2, k, (0, 0), 2, 100.0)
    assert flat["stats"][8] == 4 and flat["stats"][9] == 0 and flat["stats"][11] == 0
    # a degenerate frame has no active patch
    z = depth_corr_local_ref(od, fT, np.zeros_like(mono), 0.5, 0.3, 0.2, k, (0, 0), 2, 0.0)
    assert not z["stats"].any() and not z["v_depth"].any() and not z["v_alpha"].any()


def test_config_trainer_and_checkpoint_defaults_carry_the_term_and_default_to_off():
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    cfg = ModelConfig()
    assert cfg.mono_depth_local_mult == 0.0 and cfg.mono_depth_patch_tiles == 8
    assert cfg.mono_depth_patch_min_fill == 0.25 and cfg.mono_depth_patch_min_var == 1e-3
    # a checkpoint written before the fields existed records a config without them: they take their defaults
    new = ("mono_depth_local_mult", "mono_depth_patch_tiles", "mono_depth_patch_min_fill", "mono_depth_patch_min_var")
    old = {k: v for k, v in dataclasses.asdict(cfg).items() if k not in new}
    assert len(old) == len(dataclasses.asdict(cfg)) - 4 and ModelConfig(**old) == cfg
    # the offset rule: off_x = step % k, off_y = (step // k) % k -- every alignment once in k^2 steps
    offs = [DepthGaussianSplattingModel.patch_offset(type("M", (), dict(config=ModelConfig(mono_depth_patch_tiles=3), step=s))())
            for s in range(9)]
    assert offs == [(s % 3, (s // 3) % 3) for s in range(9)] and len(set(offs)) == 9
    src = open(os.path.join(ROOT, "touch_gs_amd", "train.py")).read()
    for flag in ("--mono-depth-local-mult", "--mono-depth-patch-tiles", "--mono-depth-patch-min-fill", "--mono-depth-patch-min-var"):
        assert flag in src
    for field in new:
        assert re.search(field + r"=args\." + field, src), field
    assert "args.mono_depth_local_mult > 0" in src          # without a map: the same SystemExit as the global term
