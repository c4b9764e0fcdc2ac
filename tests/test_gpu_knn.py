"""The exact k-NN kernels (csrc/knn.hip through touch_gs_amd.ops.knn) against the brute-force reference tests/knn_ref.py:
dist2 AND idx are compared for EQUALITY with the fp32 reference -- no tolerance, no case left out -- on clouds chosen for what
can go wrong: one box and several, a last partial box, a dense object in a sparse fill, duplicates (distance 0, self excluded
by index, ties by index), one key for the whole cloud, a lattice of exact ties, clouds flat on one or two axes, fewer points
than k, queries outside the references' bounds.  Then the three consumers: distCUDA2, init_params(knn="hip"), surface_metrics."""
import numpy as np
import pytest
import torch

import knn_ref as R
from touch_gs_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = [1, 3, 8, 16]
BOX = _lib.KNN_BOX


def _run(points, k, queries=None, **kw):
    tq = None if queries is None else torch.from_numpy(queries).to(DEV)
    d, i = ops.knn(torch.from_numpy(points).to(DEV), k, queries=tq, **kw)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == i.shape == (len(points if queries is None else queries), k)
    return d.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    bad = np.nonzero((gd.view(np.int32) != wd.view(np.int32)).any(1) | (gi != wi).any(1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} rows differ, first {bad[0]}: got {gd[bad[0]]} {gi[bad[0]]}, want {wd[bad[0]]} {wi[bad[0]]}"


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ["uniform", "mix", "dup4", "same300", "lattice", "planar", "collinear"])
def test_self_query_equals_the_reference(name, k):
    """Fixtures 1 - 5 (the reference is computed once at k = 16; its first k columns are the reference at k)."""
    wd, wi = R.reference(name, 16)
    _same(_run(R.fixture(name), k), (np.ascontiguousarray(wd[:, :k]), wi[:, :k]), f"{name} k={k}")


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fewer_points_than_k(n):
    """Fixture 6a: n - 1 neighbours exist; the slots behind them are +inf / -1."""
    got = _run(R.fixture(f"n{n}"), 3)
    _same(got, R.knn(R.fixture(f"n{n}"), 3), f"n={n}")
    m = min(n - 1, 3)
    assert np.isinf(got[0][:, m:]).all() and (got[1][:, m:] == -1).all() and np.isfinite(got[0][:, :m]).all()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", [BOX - 1, BOX, BOX + 1, 2 * BOX + 1])
def test_box_boundaries(n, k):
    """Fixture 6b: one box short of full, exactly full, a second box of one point, a third of one point."""
    wd, wi = R.reference(f"n{n}", 16)
    _same(_run(R.fixture(f"n{n}"), k), (np.ascontiguousarray(wd[:, :k]), wi[:, :k]), f"n={n} k={k}")


@pytest.mark.parametrize("k", KS)
def test_two_sets_with_and_without_query_order(k):
    """Fixture 7: 777 references in the unit cube, 1 000 queries of which a third lie far outside; served in Morton order
    (q_order given) and in their own order (q_order NULL): the same bits."""
    ref, q = R.fixture("refs777"), R.fixture("queries1000")
    lo, hi = ref.min(0), ref.max(0)
    outside = ((q < lo - 1) | (q > hi + 1)).any(1)
    assert 300 <= outside.sum() <= 400
    want = R.knn(ref, k, queries=q)
    assert (want[1] >= 0).all()
    a = _run(ref, k, queries=q)
    b = _run(ref, k, queries=q, sort_queries=False)
    _same(a, want, f"two sets, Morton order, k={k}")
    _same(b, want, f"two sets, own order, k={k}")


@pytest.mark.parametrize("k", KS)
def test_rows_shuffled(k):
    """Fixture 8: the cloud in another order: per point the same dist2 bits, and -- fixture 1 has no ties, asserted on the
    reference -- the same neighbours."""
    pts = R.fixture("uniform")
    d17, i17 = R.reference("uniform", 17)
    assert (np.diff(d17, axis=1) > 0).all()                        # no ties up to the first neighbour left out
    perm = np.random.default_rng(11).permutation(len(pts))         # row j of the shuffled cloud is point perm[j]
    gd, gi = _run(np.ascontiguousarray(pts[perm]), k)
    wd, wi = d17, i17
    _same((gd, perm[gi].astype(np.int32)), (np.ascontiguousarray(wd[perm, :k]), wi[perm, :k]), f"shuffled k={k}")


def test_two_runs_are_bit_identical():
    """Fixture 9."""
    for name in ("mix", "dup4"):
        a, b = _run(R.fixture(name), 16), _run(R.fixture(name), 16)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_non_finite_coordinates_are_refused():
    p = torch.from_numpy(R.fixture("n257")).to(DEV).clone()
    for bad in (float("nan"), float("inf")):
        x = p.clone()
        x[100, 1] = bad
        with pytest.raises(ValueError):
            ops.knn(x, 3)
        with pytest.raises(ValueError):
            ops.knn(p, 3, queries=x)


def test_distCUDA2_equals_the_reference_mean_of_three():
    """Fixture 10: squared, not clamped -- INRIA's semantics."""
    from touch_gs_amd.simple_knn import distCUDA2
    for name in ("mix", "dup4"):
        got = distCUDA2(torch.from_numpy(R.fixture(name)).to(DEV))
        want = R.dist_mean3(R.fixture(name))
        assert got.shape == (len(want),) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), name
    assert (R.dist_mean3(R.fixture("dup4")) == 0).all()             # three copies at distance 0: nothing is clamped


def test_init_params_hip_scales_against_fp64():
    """Fixture 11: scale = mean(sqrt(dist2[:, :3]), 1) against the fp64 brute force to 4 * 2^-24 relative: d2 is within
    8 * 2^-24 (tests/test_cpu_knn.py), the root halves that, root and mean add under 2 ulp.  The log-scales are the log of
    exactly those scales.  Measured on an MI355X: largest relative error 3.07 x 2^-24."""
    from touch_gs_amd.train import init_params, knn_scale_hip
    pts, cols = R.init_cloud(2500, seed=2)
    params = init_params(4000, 4, DEV, (torch.from_numpy(pts), torch.from_numpy(cols)), extent=1.0, seed=1, knn="hip")
    assert params.means.shape == (4000, 3)
    kd = knn_scale_hip(params.means.contiguous())
    assert torch.equal(params.log_scales.cpu(), torch.log(kd.cpu())[:, None].repeat(1, 3))
    d64, _ = R.knn(params.means.cpu().numpy(), 3, dtype=np.float64)
    want = np.sqrt(d64).mean(1)
    assert want.min() > 1e-5                                          # the clamp is idle on this cloud
    rel = np.abs(kd.cpu().numpy().astype(np.float64) - want) / want
    print(f"init scales: largest relative error {rel.max() / 2.0 ** -24:.3f} x 2^-24 (bound 4); scales {want.min():.2e} .. {want.max():.2e}")
    assert rel.max() <= 4 * 2.0 ** -24
    # the dense object's scales are its own spacing, not the fill's
    assert np.median(want[:2000]) < 0.2 * np.median(want[2000:])


def _sphere(rng, n, centre, radius, noise):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return centre + v * (radius + noise * rng.normal(size=(n, 1)))


def test_surface_metrics_on_the_device_against_ckdtree():
    """Fixture 12: two 20 000-point clouds of a sphere far from the origin.  Chamfer within 4 * 2^-24 * max |centred
    coordinate| (the fp32 rounding of two points) + 1e-6 * chamfer (the d2 bound through the root); precision and recall
    EQUAL, with tau placed where no fp64 distance lies within that bound of it (asserted on the reference).  Measured on an
    MI355X: |chamfer difference| 4.3e-11 of a bound of 2.6e-7; tau clear of every distance by 3.4e-6."""
    from scipy.spatial import cKDTree
    from touch_gs_amd.tsdf import surface_metrics
    rng = np.random.default_rng(4)
    centre = np.array([50.0, -30.0, 20.0])
    p = _sphere(rng, 20000, centre, 1.0, 0.004)
    g = _sphere(rng, 20000, centre, 1.0, 0.0)
    d_all = np.sort(np.concatenate([cKDTree(g).query(p)[0], cKDTree(p).query(g)[0]]))
    c = np.concatenate([p, g]).mean(0)
    chamfer = 0.5 * (cKDTree(g).query(p)[0].mean() + cKDTree(p).query(g)[0].mean())
    bound = 4 * 2.0 ** -24 * np.abs(np.concatenate([p, g]) - c).max() + 1e-6 * chamfer
    mid = d_all[len(d_all) // 4: 3 * len(d_all) // 4]
    j = int(np.argmax(np.diff(mid)))
    tau = 0.5 * (mid[j] + mid[j + 1])                                 # the widest gap of the middle half
    assert np.abs(d_all - tau).min() > bound, "the fixture must keep every distance clear of tau"
    host = surface_metrics(p, g, tau)
    dev = surface_metrics(p, g, tau, device=DEV)
    print(f"chamfer host {host['chamfer']:.9e} device {dev['chamfer']:.9e} |diff| {abs(host['chamfer'] - dev['chamfer']):.3e} "
          f"(bound {bound:.3e}); tau {tau:.6e} clear by {np.abs(d_all - tau).min():.3e}; precision {host['precision']:.4f} "
          f"recall {host['recall']:.4f}")
    assert 0.05 < host["precision"] < 0.95 and 0.05 < host["recall"] < 0.95
    assert abs(host["chamfer"] - dev["chamfer"]) <= bound
    assert dev["precision"] == host["precision"] and dev["recall"] == host["recall"] and dev["fscore"] == host["fscore"]
    assert dev["n_points"] == host["n_points"] and dev["n_gt"] == host["n_gt"]
