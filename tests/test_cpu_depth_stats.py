"""CPU tests of the depth-statistics pass (tgs_rasterize_depth_stats): the entry point is declared, exported and bound
within TGS_VERSION 320; its argument validation runs before any launch; the fp64 reference the GPU tests compare with
(tests/depth_stats_ref.py) agrees with the untouched oracle where the two overlap; the rendered variance goes to disk in
the format of the pipeline's uncertainty maps."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests.depth_stats_ref import clear_pixels, depth_stats_ref_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tgs_rasterize_depth_stats"


def test_entry_point_is_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "prototype missing from include/tgs.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert len(args) == 14
    assert hasattr(lib, NAME)
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 14
    assert argtypes[0] == C.POINTER(_lib.TgsCamera) and argtypes[4] is C.c_int64
    assert argtypes[12] == C.POINTER(_lib.TgsRasterOpts)
    assert lib.tgs_version() == 320
    # additions only: the structs the entry point takes kept their sizes
    assert C.sizeof(_lib.TgsCamera) == 116 and C.sizeof(_lib.TgsRasterOpts) == 32


def _cam(W, H):
    from touch_gs_amd import _lib
    cam = _lib.TgsCamera()
    cam.W, cam.H, cam.fx, cam.fy, cam.cx, cam.cy = W, H, 300.0, 300.0, W / 2, H / 2
    for i in (0, 5, 10, 15):
        cam.viewmat[i] = 1.0
    return cam


def test_argument_validation_without_a_device():
    """TGS_E_ARG before any launch: a tile_start buffer shorter than tgs_tile_start_len, a NULL out_depth, an image side
    above 4080 px, a bad camera.  (The pointers are never dereferenced.)"""
    from touch_gs_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    W, H = 320, 208
    T = lib.tgs_num_tiles(W, H)
    need = lib.tgs_tile_start_len(W, H)
    cam = _cam(W, H)
    fake = C.c_void_p(0x1000)
    call = lambda cam, tlen, out_depth=fake: fn(C.byref(cam), fake, fake, fake, tlen, None, out_depth, fake, None,
                                                fake, fake, None, None, None)
    for short in (0, T + 1, need - 1):
        assert call(cam, short) == -1 and b"tgs_tile_start_len" in lib.tgs_last_error(), lib.tgs_last_error()
    assert call(cam, need, None) == -1 and b"null" in lib.tgs_last_error()
    for w, h in ((4081, 64), (64, 4096), (5000, 5000)):
        big = _cam(w, h)
        assert call(big, lib.tgs_tile_start_len(w, h)) == -1 and b"4080" in lib.tgs_last_error(), lib.tgs_last_error()
    assert call(_lib.TgsCamera(), need) == -1 and b"camera" in lib.tgs_last_error()


def test_ops_wrapper_refuses_cpu_tensors_and_wrong_shapes():
    from touch_gs_amd import Camera, ops
    cam = Camera(np.eye(4), 100.0, 100.0, 32.0, 24.0, 64, 48)
    T = cam.num_tiles
    ts = torch.zeros(T + 513, dtype=torch.int32)[:T + 1]
    z = torch.zeros(48, 64)
    with pytest.raises(RuntimeError):      # no CPU path
        ops.rasterize_depth_stats(cam, torch.zeros(4, 12), torch.zeros(4, dtype=torch.int32), ts, z, z)
    with pytest.raises(ValueError):        # a copy of tile_start has lost the scratch behind the starts
        ops.rasterize_depth_stats(cam, torch.zeros(4, 12), torch.zeros(4, dtype=torch.int32), ts.clone(), z, z)
    with pytest.raises(ValueError):
        ops.rasterize_depth_stats(cam, torch.zeros(4, 12), torch.zeros(4, dtype=torch.int32), ts, z[:10], z)


@pytest.mark.parametrize("N,W,H,seed,view", [(2000, 128, 96, 1, 0), (640, 157, 93, 4, 0), (1500, 100, 70, 5, 3)])
def test_reference_agrees_with_the_oracle_blend(N, W, H, seed, view):
    """The new reference's alpha and expected depth are the oracle's ``depth_acc / alpha`` to 1e-12; its variance is
    non-negative and equals the moment form where that form is well conditioned; the median obeys its definition."""
    P, c = O.synthetic_scene(N, W, H, 1, seed)
    cam = O.Camera(viewmat=O.orbit_viewmat(view, 8), **c, bg=(0.1, 0.2, 0.3))
    ref, out, pr, gid, ts = depth_stats_ref_scene(P, cam, 1)
    alpha = out["alpha"].numpy()
    assert np.abs(ref["alpha"] - alpha).max() <= 1e-12
    dhat = (out["depth_acc"] / torch.clamp(out["alpha"], min=1e-10)).numpy()
    assert np.abs(ref["dhat"] - dhat).max() <= 1e-12 * max(1.0, np.abs(dhat).max())
    assert (ref["var"] >= 0).all() and (ref["var"][alpha == 0] == 0).all()
    # the spread of depths along a ray is bounded by the scene's depth range
    d = pr["depth"][pr["valid"]].numpy()
    assert ref["var"].max() <= (d.max() - d.min()) ** 2
    has = ref["median_gid"] >= 0
    clear = clear_pixels(out, ref)
    assert clear.mean() >= 0.99, clear.mean()
    assert np.array_equal(has[clear], (alpha >= 0.5)[clear])        # a median exists <=> transmittance reaches 1/2
    assert (ref["median_depth"][~has] == 0).all()
    assert np.array_equal(ref["median_depth"][has], pr["depth"].numpy()[ref["median_gid"][has]])
    # every median is a member of its pixel's tile list
    TW = cam.tiles[0]
    ys, xs = np.nonzero(has)
    for y, x in list(zip(ys, xs))[::37]:
        t = (y // 16) * TW + x // 16
        assert ref["median_gid"][y, x] in gid[ts[t]:ts[t + 1]]


def test_variance_moment_form_cancels():
    """Why the pass accumulates sum w (d - Dhat)^2 and not sum w d^2 / alpha - Dhat^2: on a plain synthetic scene the
    second form cancels by a factor of several hundred on pixels of substantial coverage (alpha > 0.05) -- of fp32's seven
    digits fewer than five are left, against the four the variance is held to.  Measured here in fp64, where both forms
    can still be compared."""
    P, c = O.synthetic_scene(2000, 128, 96, 0, 1)
    cam = O.Camera(viewmat=O.orbit_viewmat(0, 8), **c)
    ref, out, pr, gid, ts = depth_stats_ref_scene(P, cam, 0)
    m = (ref["alpha"] > 0.05) & (ref["var"] > 0)
    ratio = (ref["var"][m] + ref["dhat"][m] ** 2) / ref["var"][m]        # = sum w d^2 / alpha over the variance
    assert ratio.max() > 3e2, ratio.max()


def test_uncertainty_png_round_trips_through_the_dataset_reader(tmp_path):
    """Variance (scene units squared) -> m^2 -> clip [0, 10] -> x 1000 -> uint16, written with write_png16 and read with
    read_png16 / from_uint16_mm: within one quantum (1e-3 m^2) of the clipped map, never above it (truncation)."""
    from touch_gs_amd.plumbing import from_uint16_mm, read_png16, write_png16
    from touch_gs_amd.train import uncertainty_png
    g = torch.Generator().manual_seed(3)
    scale = 0.37
    var_m2 = torch.cat([torch.rand(40, 50, generator=g, dtype=torch.float64) * 12.0,       # some above the clip
                        torch.rand(40, 50, generator=g, dtype=torch.float64) * 1e-2,
                        torch.zeros(1, 50, dtype=torch.float64)])
    img = uncertainty_png((var_m2 * scale ** 2).float(), scale)
    assert img.dtype == np.uint16 and img.shape == (81, 50) and img.max() == 10000
    path = str(tmp_path / "u.png")
    write_png16(path, img)
    back = from_uint16_mm(read_png16(path))
    want = np.clip(var_m2.numpy(), 0.0, 10.0)
    assert np.array_equal(read_png16(path), img)
    assert (np.abs(back - want) <= 1e-3 + 1e-5).all() and (back <= want + 1e-5).all()
    assert (back[-1] == 0).all()


def test_eval_tools_keep_depth_stats_off_by_default():
    from touch_gs_amd import run_eval, train
    import inspect
    assert inspect.signature(train.evaluate).parameters["depth_stats"].default is False
    assert inspect.signature(train.render_views).parameters["depth_stats"].default is False
    assert inspect.signature(run_eval.eval_run).parameters["depth_stats"].default is False
    src = open(os.path.join(ROOT, "touch_gs_amd", "train.py")).read()
    assert '"--eval-depth-stats", action="store_true"' in src
    src = open(os.path.join(ROOT, "touch_gs_amd", "run_eval.py")).read()
    assert '"--depth-stats"' in src and 'action="store_true"' in src
