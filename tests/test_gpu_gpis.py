"""GPU tests of tgs_gpis_render (csrc/gpis.hip) through ``GPIS.render_depth(backend="hip")``: status, depth,
variance and normal against the fp64 NumPy reference (tests/gpis_ref.py: the classification of clear / unclear rays and the
bars), the edge cases, determinism, and the capture end to end.

The fp32 NumPy emulation of the kernel's arithmetic on this fixture (n = 600; tests/test_cpu_gpis.py): depth 2.3e-6 m,
variance 8.4e-5 at variances up to 0.2 (case centre) and 2.2e-6 under max_var = 0.01, normal 0.0050 degrees, 0 / 0 / 1
status differences (unclear rays).

Measured on the MI355X (each test prints its own figures next to the bars; the table is in DESIGN 5.1j): status differences
0 in every case; depth on clear rays 1.18e-6 ... 1.59e-6 m (bar 5e-5), on the other common hits up to 3.40e-6 m (bar 1e-3);
variance 4.78e-5 (centre, variances up to 0.2), 1.75e-5 (unaligned), 2.32e-5 (small_odd), 1.8e-6 ... 2.0e-6 under max_var
(bar 2.5e-4); normal 0.0009 ... 0.0027 degrees (bar 0.05); capture: 100 % of 480 touched pixels within 1 count (bar 99 %).
"""
import os

import numpy as np
import pytest

import gpis_ref as G

pytestmark = pytest.mark.gpu


def _render(name, dev, **kw):
    import torch
    with torch.cuda.device(dev):
        return G.case_fit(name).render_depth(**G.render_kwargs(name), backend="hip", **kw)


@pytest.mark.parametrize("name", ["centre", "centre_max_var", "unaligned", "unaligned_max_var", "centre_stride2", "moved",
                                  "small_odd", "one_pixel"])
def test_render_against_the_fp64_reference(name, dev):
    """centre / centre_max_var: 64 x 64, fx 120; unaligned: 37 x 29, fx 70, principal point (17.3, 15.9), the region clipped
    by the image; centre_stride2; moved: the world translated by (3, -2, 5) m, the camera rotated about two axes (the
    re-centring; same bars); small_odd: n = 163, n_p = 41 (no multiple of 64, 16 or 4); one_pixel: a region of one pixel."""
    gp = G.case_fit(name)
    if name == "small_odd":
        assert len(gp.X) % 4 and len(gp.X) % 16 and len(gp.P) % 64
    else:
        assert len(gp.X) % 64 and len(gp.P) % 64
    ref = G.images(name)
    depth, var, normal = _render(name, dev, return_normals=True)
    assert depth.shape == ref["depth"].shape and normal.shape == ref["normal"].shape
    fig = G.compare(ref, depth, var, normal)
    print(G.report(name, fig))
    assert fig["unclear_share"] <= G.BAR_UNCLEAR_SHARE
    G.check(fig)
    # without normals: the same depth and variance bits
    d2, v2 = _render(name, dev)
    assert d2.tobytes() == depth.tobytes() and v2.tobytes() == var.tobytes()


def test_two_calls_give_identical_bits(dev):
    a = _render("centre_max_var", dev, return_normals=True)
    b = _render("centre_max_var", dev, return_normals=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_all_points_behind_the_camera_launch_nothing(dev, monkeypatch):
    gp = G.case_fit("centre")
    kw = G.render_kwargs("centre")
    kw["c2w_opengl"] = np.diag([-1.0, 1.0, -1.0, 1.0])      # looking away from the cap
    monkeypatch.setattr(type(gp), "_render_hip", lambda *a, **k: pytest.fail("a launch for a view that sees no touched point"))
    depth, var, normal = gp.render_depth(**kw, backend="hip", return_normals=True)
    assert np.isnan(depth).all() and np.isnan(var).all() and not normal.any()
    assert depth.shape == (kw["H"], kw["W"]) and normal.shape == (kw["H"], kw["W"], 3)


def test_march_without_variance(dev):
    """Kinv = NULL: two launches, var untouched by any crossing; depth = the full call's wherever that one's variance
    cut nothing (no max_var)."""
    import torch
    name = "unaligned"
    gp, kw = G.case_fit(name), G.render_kwargs(name)
    vs = G.view_setup(gp, kw["c2w_opengl"], kw["fx"], kw["fy"], kw["cx"], kw["cy"], kw["W"], kw["H"], kw["near"], kw["far"], kw["n_steps"])
    with torch.cuda.device(dev):
        d, v, n = gp._render_hip(vs["R"], vs["t"], kw["fx"], kw["fy"], kw["cx"], kw["cy"], kw["W"], kw["H"], vs["roi"], 1,
                                 vs["zgrid"][0], vs["zgrid"][-1], kw["n_steps"], None, 0.0, want_var=False, want_normals=False)
        torch.cuda.synchronize()
    full, _ = _render(name, dev)
    assert v is None and n is None
    assert d.cpu().numpy().astype(np.float64).tobytes() == full.tobytes()


def test_capture_end_to_end(dev, tmp_path):
    """write_raw_capture with the defaults and with gpis_backend="hip" at the same stride: after gpis_npy_to_mm the uint16
    maps differ by at most 1 count on at least 99 % of the touched pixels; the normals_gpis files load through
    dataset.Scene(normal_dir=)."""
    import torch
    from touch_gs_amd.analytic_scene import write_raw_capture
    from touch_gs_amd.dataset import read_normal_map
    from touch_gs_amd.plumbing import gpis_npy_to_mm
    kw = dict(n_views=2, n_touches=4, W=160, H=90, seed=3, gpis_max_points=150)
    a, b = str(tmp_path / "numpy"), str(tmp_path / "hip")
    write_raw_capture(a, device="cpu", **kw)
    with torch.cuda.device(dev):
        write_raw_capture(b, device="cpu", gpis_backend="hip", gpis_normals=True, **kw)
    touched = 0
    for i in range(2):
        maps = []
        for root in (a, b):
            d = np.load(os.path.join(root, "gpis_depth", f"Image{i:03d}.npy"))
            v = np.load(os.path.join(root, "gpis_var", f"Image{i:03d}.npy"))
            assert d.shape == (90, 160)
            maps.append(gpis_npy_to_mm(d, v))
        (d0, v0), (d1, v1) = maps
        on = (d0 > 0) | (d1 > 0)
        touched += int(on.sum())
        if on.any():
            close = (np.abs(d0.astype(np.int64) - d1.astype(np.int64)) <= 1) & (np.abs(v0.astype(np.int64) - v1.astype(np.int64)) <= 1)
            share = close[on].mean()
            print(f"view {i}: {on.sum()} touched pixels, {share:.4%} within 1 count (bar 99 %)")
            assert share >= 0.99
        n, conf = read_normal_map(os.path.join(b, "normals_gpis", f"{i:03d}"), 90, 160)
        assert n.shape == (90, 160, 3) and conf.shape == (90, 160) and n.dtype == np.float32
        hit = np.isfinite(np.load(os.path.join(b, "gpis_depth", f"Image{i:03d}.npy")))
        assert not n[~hit].any() and not conf[~hit].any()
        if hit.any():
            assert np.allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-5) and (conf[hit] >= 0).all() and (conf[hit] <= 0.9 + 1e-6).all()
    assert touched > 50
    assert not os.path.exists(os.path.join(a, "normals_gpis"))
    from touch_gs_amd.dataset import Scene
    scene = Scene(b, train_split_fraction=0.5, device="cpu", real_world=False, normal_dir="normals_gpis")
    assert len(scene.views) == 2
    for i, view in enumerate(scene.views):
        n, _ = read_normal_map(os.path.join(b, "normals_gpis", f"{i:03d}"), 90, 160)
        assert view.normal_prior is not None and view.normal_conf is not None
        assert np.array_equal(view.normal_prior.numpy(), n) and tuple(view.normal_conf.shape) == (90, 160)
