"""CPU tests of the exact k nearest neighbours (tgs_knn_keys / tgs_knn_build / tgs_knn_query, touch_gs_amd.ops.knn,
touch_gs_amd.simple_knn): the ABI, the argument checks, the fp32 definition's error against fp64 (printed), and the
guard of init_params' default path.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import knn_ref as R
from touch_gs_amd import simple_knn  # noqa: F401  (before the feature the whole file fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "tgs_knn_keys": ["n", "pts", "lo", "hi", "keys", "stream"],
    "tgs_knn_build": ["n", "pts", "order", "sorted_pts", "boxes", "stream"],
    "tgs_knn_query": ["n_q", "queries", "q_order", "n_ref", "sorted_pts", "boxes", "k", "exclude_self", "dist2", "idx", "stream"],
}


def test_entry_points_are_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, want in NAMES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, f"prototype of {name} missing from include/tgs.h"
        assert [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")] == want
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(want) and hasattr(lib, name)
    assert lib.tgs_version() == 320
    assert int(re.search(r"#define\s+TGS_KNN_MAX_K\s+(\d+)", txt).group(1)) == _lib.KNN_MAX_K == 16
    assert int(re.search(r"#define\s+TGS_KNN_BOX\s+(\d+)", txt).group(1)) == _lib.KNN_BOX
    build = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "build.sh")).read()
    assert "knn" in build.split('SRCS="')[1].split('"')[0].split()
    assert '[knn]="-ffp-contract=off"' in build


def test_argument_validation_launches_nothing():
    """Every refusal comes back before a launch: the pointers handed in are host memory."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    f3 = lambda *v: (C.c_float * 3)(*v)
    err = lambda: lib.tgs_last_error()
    lo, hi = f3(0, 0, 0), f3(1, 1, 1)

    keys = lambda **kw: lib.tgs_knn_keys(kw.get("n", 8), kw.get("pts", p), kw.get("lo", lo), kw.get("hi", hi), kw.get("keys", p), None)
    assert keys(n=0) == -1 and b"n < 1" in err()
    assert keys(n=-5) == -1
    assert keys(pts=None) == -1 and b"null" in err()
    assert keys(keys=None) == -1 and keys(lo=None) == -1 and keys(hi=None) == -1 and b"null" in err()
    assert keys(lo=f3(0, float("nan"), 0)) == -1 and b"non-finite" in err()
    assert keys(hi=f3(float("inf"), 1, 1)) == -1 and b"non-finite" in err()
    assert keys(lo=f3(0, 2, 0)) == -1 and b"inverted" in err()

    build = lambda **kw: lib.tgs_knn_build(kw.get("n", 8), kw.get("pts", p), kw.get("order", p), kw.get("sorted_pts", p),
                                           kw.get("boxes", p), None)
    assert build(n=0) == -1 and b"n < 1" in err()
    assert build(n=1 << 30) == -1 and b"index" in err()
    assert build(pts=None) == -1 and build(order=None) == -1 and build(sorted_pts=None) == -1 and build(boxes=None) == -1
    assert b"null" in err()

    def query(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return lib.tgs_knn_query(g("n_q", 8), g("queries", p), g("q_order", None), g("n_ref", 8), g("sorted_pts", p), g("boxes", p),
                                 g("k", 3), g("exclude_self", 0), g("dist2", p), g("idx", p), None)
    assert query(n_q=0) == -1 and query(n_ref=0) == -1 and query(n_q=-1) == -1 and b"< 1" in err()
    assert query(k=0) == -1 and query(k=17) == -1 and query(k=-2) == -1 and b"k outside" in err()
    assert query(queries=None) == -1 and query(sorted_pts=None) == -1 and query(boxes=None) == -1 and b"null" in err()
    assert query(dist2=None) == -1 and query(idx=None) == -1 and b"null" in err()
    assert query(exclude_self=1, n_q=8, n_ref=9) == -1 and b"exclude_self" in err()
    assert query(n_ref=1 << 30) == -1 and b"index" in err()


def test_ops_knn_refuses_bad_input_before_the_library():
    from touch_gs_amd import ops
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError):
        ops.knn(x, 0)
    with pytest.raises(ValueError):
        ops.knn(x, 17)
    with pytest.raises(ValueError):
        ops.knn(torch.zeros(5, 2), 3)
    with pytest.raises(ValueError):
        ops.knn(x.double(), 3)
    with pytest.raises(RuntimeError):
        ops.knn(x, 3)                                  # a host tensor: there is no CPU path
    assert "non-finite" in inspect.getsource(ops._knn_bounds)


@pytest.mark.parametrize("name", ["uniform", "mix", "planar", "collinear", "refs777"])
def test_fp32_definition_against_fp64(name):
    """Per rank |d2_32 - d2_64| <= 8 * 2^-24 * d2_64: three correctly rounded differences, three products and two sums of
    non-negative terms stay under 6 ulp (an order statistic of values that are each within a relative bound is within it).
    Measured largest ratios to 2^-24 * d2_64: uniform 3.37, mix 3.29, planar 2.82, collinear 2.61, refs777 3.34."""
    d32, _ = R.reference(name, 16, "float32")
    d64, _ = R.reference(name, 16, "float64")
    assert d32.dtype == np.float32 and d64.dtype == np.float64 and (d64 > 0).all()
    ratio = np.abs(d32.astype(np.float64) - d64) / (2.0 ** -24 * d64)
    print(f"{name}: largest |d2_32 - d2_64| = {ratio.max():.3f} x 2^-24 d2_64 (bound 8)")
    assert ratio.max() <= 8.0


def test_reference_orders_ties_by_index_and_excludes_by_index():
    d, i = R.knn(R.fixture("same300"), 16)
    assert not d.any()
    want = np.array([[j for j in range(17) if j != q][:16] for q in range(300)])
    assert np.array_equal(i, want)
    d, i = R.knn(R.fixture("n3"), 3)
    assert np.isinf(d[:, 2]).all() and (i[:, 2] == -1).all() and np.isfinite(d[:, :2]).all() and (i[:, :2] >= 0).all()
    d, i = R.knn(R.fixture("n1"), 3)
    assert np.isinf(d).all() and (i == -1).all()
    d, i = R.knn(R.fixture("lattice"), 8)
    assert (d[:, :3] == 1).all() and (np.diff(d, axis=1) >= 0).all()
    ties = np.diff(d, axis=1) == 0
    assert (np.diff(i, axis=1)[ties] > 0).all()
    # the two-set form keeps a reference at distance 0
    d, i = R.knn(R.fixture("n4"), 2, queries=R.fixture("n4"))
    assert not d[:, 0].any() and np.array_equal(i[:, 0], np.arange(4))


def test_init_params_default_is_todays_expression_bit_for_bit():
    """knn="torch", and no keyword at all, give the scales of the expression init_params has always used."""
    from touch_gs_amd.train import init_params
    pts, cols = R.init_cloud(700, seed=5)
    seed_points = (torch.from_numpy(pts), torch.from_numpy(cols))
    n, K = 1000, 4
    for kw in (dict(), dict(knn="torch")):
        params = init_params(n, K, "cpu", seed_points, extent=1.0, seed=3, seed_fraction=0.5, **kw)
        md = params.means
        N = md.shape[0]
        assert N == n
        blk = max(64, min(4096, (1 << 28) // max(N, 1)))
        kd = torch.empty(N, device=md.device)
        for b in range(0, N, blk):
            d = torch.cdist(md[b:b + blk], md)
            kd[b:b + blk] = d.topk(4, largest=False).values[:, 1:].mean(1).clamp_min(1e-5)
        assert torch.equal(params.log_scales, torch.log(kd.cpu())[:, None].repeat(1, 3))
    with pytest.raises(ValueError):
        init_params(n, K, "cpu", seed_points, knn="kdtree")
    src = inspect.getsource(__import__("touch_gs_amd.train", fromlist=["main"]).main)
    assert '"--init-knn"' in src and 'choices=("torch", "hip")' in src


def test_cli_flags_and_shim():
    from touch_gs_amd import export, run_eval, tsdf
    assert '"--metrics-device"' in inspect.getsource(export.main) and '"--metrics-device"' in inspect.getsource(run_eval.main)
    assert inspect.signature(tsdf.surface_metrics).parameters["device"].default is None
    assert inspect.signature(export.export_tsdf).parameters["metrics_device"].default is None
    assert callable(simple_knn.distCUDA2)
