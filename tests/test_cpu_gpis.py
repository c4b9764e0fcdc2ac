"""CPU tests of the GPIS render feature (tgs_gpis_render): the NumPy definitions the kernel is held to, the
reference's own classification, the fp32 emulation against the bars, and the unchanged default path.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gpis_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tgs_gpis_render"


def test_entry_point_is_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "prototype missing from include/tgs.h"
    names = [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
    assert names == ["n", "X", "n_p", "P", "N", "Kinv", "l", "sf2", "prior", "view", "depth", "var", "normal", "hits", "stream"]
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == 15 and argtypes[9] == C.POINTER(_lib.TgsGpisView)
    assert hasattr(lib, NAME) and lib.tgs_version() == 320
    # the struct's fields, in the header's order
    body = re.search(r"typedef struct TgsGpisView \{(.*?)\} TgsGpisView;", txt, flags=re.S).group(1)
    fields = [f.strip().split("[")[0] for decl in re.findall(r"(?:float|int32_t)\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [f[0] for f in _lib.TgsGpisView._fields_]
    assert C.sizeof(_lib.TgsGpisView) == 4 * (9 + 3 + 4 + 2 + 5 + 2 + 1 + 2)


def test_argument_validation_launches_nothing():
    from touch_gs_amd import _lib
    lib = _lib.load()
    v = _lib.TgsGpisView()
    v.fx = v.fy = 100.0
    v.W = v.H = 8
    v.u1 = v.v1 = 7
    v.stride, v.n_steps, v.dz, v.max_var = 1, 16, 0.01, -1.0
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    call = lambda **kw: lib.tgs_gpis_render(kw.get("n", 4), kw.get("X", p), 4, p, p, kw.get("Kinv"), C.c_float(kw.get("l", 0.04)),
                                            C.c_float(1.0), C.c_float(0.01), C.byref(v), kw.get("depth", p), p, None, p, None)
    assert call(n=0) < 0 and b"no points" in lib.tgs_last_error()
    assert call(X=None) < 0
    assert call(l=0.0) < 0
    assert call(depth=None) < 0
    v.n_steps = 513
    assert call() < 0 and b"n_steps" in lib.tgs_last_error()
    v.n_steps, v.u1 = 16, 8
    assert call() < 0 and b"region" in lib.tgs_last_error()
    v.u1, v.max_var = 7, 0.01
    assert call() < 0 and b"max_var without Kinv" in lib.tgs_last_error()


def test_gradient_matches_a_central_difference_of_predict():
    """1e-6 of the largest gradient (measured: 2.4e-8 with the n = 1600 fit, 3e-8 here)."""
    gp = G.sphere_fit()
    rng = np.random.default_rng(1)
    Q = gp.P[rng.choice(len(gp.P), 40, replace=False)] + rng.normal(size=(40, 3)) * 0.01
    Q = np.concatenate([Q, gp.P[:5] + np.array([0.0, 0.0, 0.2])])      # far from every touch: the prior's blend dominates
    g = gp.gradient_at(Q)
    h = 1e-6
    fd = np.empty_like(g)
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        fd[:, a] = (gp.predict(Q + e, want_var=False)[0] - gp.predict(Q - e, want_var=False)[0]) / (2 * h)
    scale = np.linalg.norm(g, axis=1).max()
    err = np.abs(g - fd).max() / scale
    print(f"gradient_at against a central difference: {err:.2e} of the largest gradient {scale:.3f} (bar 1e-6)")
    assert err <= 1e-6
    n = gp.normal_at(Q)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-12)
    assert np.allclose(n, g / np.linalg.norm(g, axis=1, keepdims=True), atol=1e-15)


def test_normals_of_the_sphere():
    """Against the analytic sphere on the core rays of test_gpis_sphere: within 10 degrees (measured with that test's own
    fit, n = 1600: mean 1.4, max 3.8 degrees)."""
    from touch_gs_amd.gpis import GPIS, estimate_outward_normals
    rng = np.random.default_rng(0)
    pts, _ = G.sphere_points()
    g = GPIS(length_scale=0.04, offset=0.01).fit(pts, estimate_outward_normals(pts, np.zeros_like(pts)), max_points=400, rng=rng)
    W = H = 64
    fx = fy = 120.0
    depth, var, normals = g.render_depth(np.eye(4), fx, fy, W / 2, H / 2, W, H, near=0.05, far=1.0, n_steps=64, return_normals=True)
    ok = np.isfinite(depth)
    us, vs = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    core = ok & (np.hypot(us - W / 2, vs - H / 2) < 10)
    assert core.sum() > 100
    d = np.stack([(us - W / 2) / fx, (vs - H / 2) / fy, np.ones_like(us)], -1)
    hit = d[core] * depth[core][:, None]                    # OpenCV camera axes; the sphere's centre is (0, 0, 0.5)
    true = hit - np.array([0.0, 0.0, 0.5])
    true /= np.linalg.norm(true, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip((normals[core] * true).sum(1), -1, 1)))
    print(f"GPIS normals against the sphere's on {core.sum()} core rays: mean {ang.mean():.2f}, max {ang.max():.2f} degrees (bar 10)")
    assert ang.max() < 10.0
    assert (normals[core][:, 2] < 0).all()                  # outward = towards the camera
    assert np.array_equal(normals[~ok], np.zeros_like(normals[~ok]))
    assert np.allclose(np.linalg.norm(normals[ok], axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("name", ["centre", "centre_max_var", "unaligned"])
def test_default_path_is_the_parent_body_and_the_reference_restates_it(name):
    gp = G.case_fit(name)
    kw = G.render_kwargs(name)
    d0, v0 = G.render_depth_parent(gp, **kw)
    d1, v1 = gp.render_depth(**kw)
    assert d1.tobytes() == d0.tobytes() and v1.tobytes() == v0.tobytes()
    d2, v2, n2 = gp.render_depth(**kw, return_normals=True)
    assert d2.tobytes() == d0.tobytes() and v2.tobytes() == v0.tobytes()
    hit = np.isfinite(d0)
    assert hit.any() and not n2[~hit].any()
    ref = G.images(name)
    assert ref["depth"].tobytes() == d0.tobytes() and ref["var"].tobytes() == v0.tobytes()
    assert np.array_equal(ref["normal"], n2)
    with pytest.raises(ValueError):
        gp.render_depth(**kw, backend="cuda")


def test_reference_images_of_the_strided_case():
    """The stride-2 reference is cut from the stride-1 march (another batch shape of the same arithmetic)."""
    name = "centre_stride2"
    d0, v0 = G.render_depth_parent(G.case_fit(name), **G.render_kwargs(name))
    ref = G.images(name)
    assert np.array_equal(np.isfinite(ref["depth"]), np.isfinite(d0))
    hit = np.isfinite(d0)
    assert np.abs(ref["depth"][hit] - d0[hit]).max() < 1e-12 and np.abs(ref["var"][hit] - v0[hit]).max() < 1e-12
    assert ref["region"].sum() == 32 * 32 and not ref["region"][1::2].any() and not ref["region"][:, 1::2].any()


@pytest.mark.parametrize("name", list(G.CASES))
def test_clear_share_of_the_reference(name):
    """At most 10 % of the region's rays are unclear (measured: 4.5 % centre, 5.7 % unaligned, 4.5 % moved)."""
    ref = G.images(name)
    share = (ref["unclear"] & ref["region"]).sum() / ref["region"].sum()
    print(f"{name}: unclear share {share:.3%} of {ref['region'].sum()} rays (bar {G.BAR_UNCLEAR_SHARE:.0%})")
    assert share <= G.BAR_UNCLEAR_SHARE
    assert np.isfinite(ref["depth"]).sum() > 0.3 * ref["region"].sum()


@pytest.mark.parametrize("name", ["centre", "unaligned_max_var", "moved"])
def test_fp32_emulation_stays_inside_every_bar(name):
    """The kernel's arithmetic in NumPy fp32 (centred coordinates, differences, fp32 exponentials) against the fp64
    reference, summed as the kernel sums (fp32 over 8 points, fp64 across).  Measured: depth 2.3e-6 m on clear rays (bar
    5e-5) and 5.7e-6 m on the others, variance 8.4e-5 at variances up to 0.2 (centre) and 2.2e-6 under max_var (bar 2.5e-4),
    normal 0.0050 degrees (bar 0.05), status differences 0 / 0 / 1 unclear ray of 4096."""
    em = G.emulate(name)
    fig = G.compare(G.images(name), em["depth"], em["var"], em["normal"])
    print(G.report(name, fig))
    G.check(fig)
