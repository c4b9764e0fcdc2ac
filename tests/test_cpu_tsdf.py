"""CPU tests of the TSDF export (tgs_tsdf_integrate / tgs_tsdf_extract_count / tgs_tsdf_extract_points, touch_gs_amd.tsdf,
touch_gs_amd.export): the ABI, the argument checks, the NumPy definition against analytic facts, the fixtures'
clear shares, the fp32 emulation's floors (printed; the GPU bars of tests/test_gpu_tsdf.py are 4 x them), the file formats
and the metrics.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tsdf_ref as T
from touch_gs_amd import export, tsdf  # noqa: F401  (before the feature the whole file fails here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "tgs_tsdf_integrate": ["nx", "ny", "nz", "vox", "trunc", "S", "Wt", "C", "n_views", "views", "stream"],
    "tgs_tsdf_extract_count": ["nx", "ny", "nz", "vox", "S", "Wt", "w_min", "counts", "stream"],
    "tgs_tsdf_extract_points": ["nx", "ny", "nz", "vox", "S", "Wt", "C", "w_min", "offsets", "points", "normals", "colors",
                                "edge_id", "stream"],
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
    assert _lib.SIGNATURES["tgs_tsdf_integrate"][1][9] == C.POINTER(_lib.TgsTsdfView)
    assert lib.tgs_version() == 320
    body = re.search(r"typedef struct TgsTsdfView \{(.*?)\} TgsTsdfView;", txt, flags=re.S).group(1)
    fields = [f.strip().split("[")[0].lstrip("* ") for decl in re.findall(r"(?:const float\*|float|int32_t)\s+([^;]+);", body)
              for f in decl.split(",")]
    assert fields == [f[0] for f in _lib.TgsTsdfView._fields_]
    assert C.sizeof(_lib.TgsTsdfView) == 4 * (9 + 3 + 4 + 2 + 2) + 3 * 8
    assert "tsdf" in open(os.path.join(ROOT, "touch_gs_amd", "csrc", "build.sh")).read().split('SRCS="')[1].split('"')[0].split()


def test_argument_validation_launches_nothing():
    """Every refusal comes back before a launch: the pointers handed in are host memory."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    view = _lib.TgsTsdfView()
    view.fx = view.fy = 60.0
    view.W, view.H, view.near_plane, view.pix_center, view.depth = 8, 8, 0.01, 0.5, p.value
    views = (_lib.TgsTsdfView * 1)(view)
    err = lambda: lib.tgs_last_error()

    def integ(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return lib.tgs_tsdf_integrate(g("nx", 4), 4, 4, C.c_float(g("vox", 0.1)), C.c_float(g("trunc", 0.3)), g("S", p), g("Wt", p),
                                      None, g("n", 1), g("views", views), None)
    assert integ(n=0) < 0 and b"n_views" in err()
    assert integ(n=9) < 0 and b"n_views" in err()
    assert integ(nx=0) < 0 and b"dims" in err()
    assert integ(nx=-3) < 0
    assert integ(vox=0.0) < 0 and b"voxel size" in err()
    assert integ(trunc=0.0) < 0 and b"truncation" in err()
    assert integ(trunc=float("nan")) < 0
    assert integ(S=None) < 0 and integ(Wt=None) < 0 and b"null" in err()
    assert integ(views=None) < 0
    assert integ(nx=1 << 29) < 0 and b"index" in err()          # 2^29 * 16 voxels
    views[0].depth = None
    assert integ() < 0 and b"depth" in err()
    views[0].depth, views[0].W = p.value, 0
    assert integ() < 0 and b"image size" in err()
    views[0].W, views[0].near_plane = 8, 0.0
    assert integ() < 0 and b"near" in err()

    count = lambda **kw: lib.tgs_tsdf_extract_count(4, 4, kw.get("nz", 4), C.c_float(0.1), kw.get("S", p), p,
                                                     C.c_float(kw.get("w_min", 0.5)), kw.get("counts", p), None)
    assert count(w_min=0.0) < 0 and b"w_min" in err()
    assert count(w_min=-1.0) < 0 and count(nz=0) < 0 and count(S=None) < 0 and count(counts=None) < 0
    points = lambda **kw: lib.tgs_tsdf_extract_points(4, 4, 4, C.c_float(kw.get("vox", 0.1)), p, p, kw.get("C"), C.c_float(kw.get("w_min", 0.5)),
                                                       kw.get("offsets", p), kw.get("points", p), kw.get("normals", p),
                                                       kw.get("colors"), None, None)
    assert points(w_min=0.0) < 0 and points(vox=-1.0) < 0
    assert points(offsets=None) < 0 and points(points=None) < 0 and points(normals=None) < 0
    assert points(colors=p) < 0 and b"colors without C" in err()


def test_reference_meets_the_analytic_sphere():
    """On `sphere` every extracted point lies within one voxel of the sphere, and the normals point outward along the radius:
    measured max distance 0.893 vox; angle to the radial direction mean 8.5, median 4.0, 90th percentile 19 degrees, max 110
    degrees -- the far tail are the crossings at the three views' silhouettes, where free space (d = 1) meets the sphere's
    shadow and no surface was seen."""
    grid, _ = T.fixture("sphere")
    st, ex = T.reference("sphere")
    assert abs((st["updates"] > 0).mean() - 0.194) < 1e-3 and len(ex["edge_id"]) == 858 and len(st["S"]) == 24679
    p = ex["points"] + np.asarray(grid["origin"])
    rad = p - np.asarray(T.SPHERE_C)
    r = np.linalg.norm(rad, axis=1)
    dist = np.abs(r - T.SPHERE_R) / grid["vox"]
    ang = np.degrees(np.arccos(np.clip((ex["normals"] * rad / r[:, None]).sum(1), -1, 1)))
    print(f"sphere: {len(p)} points, distance to the sphere max {dist.max():.3f} vox; normal against the radius: mean {ang.mean():.2f}, "
          f"median {np.median(ang):.2f}, 90 % {np.quantile(ang, 0.9):.2f}, max {ang.max():.2f} degrees")
    assert dist.max() <= 1.0
    assert np.allclose(np.linalg.norm(ex["normals"], axis=1), 1.0, atol=1e-12)
    assert np.median(ang) < 10.0 and np.quantile(ang, 0.9) < 30.0 and ang.mean() < 15.0
    # counts, offsets and the order
    assert ex["counts"].sum() == len(ex["edge_id"]) and ex["counts"].max() <= 3 and (np.diff(ex["edge_id"]) > 0).all()
    assert ((ex["t"] >= 0) & (ex["t"] <= 1)).all()
    # the clamp: free space in front of the sphere holds exactly d = 1
    f = st["S"] / np.where(st["Wt"] > 0, st["Wt"], 1)
    assert f.max() == 1.0 and f.min() >= -1.0


def test_reference_carves_free_space_in_front_of_the_plane():
    st, ex = T.reference("plane_behind")
    f = st["S"] / np.where(st["Wt"] > 0, st["Wt"], 1)
    assert (st["updates"] > 0).mean() > 0.8 and (f[st["updates"] > 0] == 1.0).mean() > 0.4
    assert len(ex["edge_id"]) > len(T.reference("sphere")[1]["edge_id"])


def test_reference_skips_what_the_header_skips():
    """Zero and NaN weights, zero depths and cameras that see none of the grid leave no trace."""
    st, _ = T.reference("behind")
    assert not st["S"].any() and not st["Wt"].any() and not st["C"].any() and not st["updates"].any()
    st, _ = T.reference("weights_rgb")
    assert np.isfinite(st["S"]).all() and np.isfinite(st["Wt"]).all() and np.isfinite(st["C"]).all()
    grid, views = T.fixture("weights_rgb")
    assert any(np.isnan(v["weight"]).any() for v in views) and all((v["weight"] == 0).any() for v in views)


def test_reference_continues_and_batches():
    grid, views = T.fixture("eight")
    whole, _ = T.reference("eight")
    part = T.integrate(grid, views[3:], state=T.integrate(grid, views[:3]))
    for k in ("S", "Wt", "C", "U"):
        assert part[k].tobytes() == whole[k].tobytes()


@pytest.mark.parametrize("name", T.ALL)
def test_unclear_share_of_the_fixture(name):
    """At most 3 % of a fixture's voxels are unclear (measured: 1.24 % on the three-camera grids, 1.22 % aligned, 0 and
    1.5 % on the thin ones, 0.04 % behind, 2.1 % with eight views), and at most 3 % of its reference crossings have an end
    that is not sign-clear (measured: none)."""
    st, ex = T.reference(name)
    share = st["unclear"].mean()
    weak = (~ex["sign_clear"]).mean() if len(ex["edge_id"]) else 0.0
    print(f"{name}: {len(st['S'])} voxels, {(st['updates'] > 0).mean():.1%} updated, unclear {share:.3%} (cap {T.CAP_UNCLEAR:.0%}); "
          f"{len(ex['edge_id'])} crossings, not sign-clear {weak:.3%}")
    assert share <= T.CAP_UNCLEAR and weak <= T.CAP_UNCLEAR


@pytest.mark.parametrize("name", T.ALL)
def test_fp32_emulation_gives_the_floors(name):
    """The header's arithmetic in NumPy fp32 against fp64, in the units of tests/tsdf_ref.py.  Measured floors (largest over
    the fixtures): S 1.41, Wt 2.71, C 3.11 (all three on `eight`), t and point 0.51, normal 0.18, colour 0.73; the fp32 and
    fp64 decisions (pixel chosen, update or not) differ on 0 voxels of every fixture.  FLOORS holds them, rounded up in the third digit."""
    st, ex = T.reference(name)
    em, eex = T.emulation(name)
    fig = T.state_errors(st, em["S"], em["Wt"], em["C"])
    cf = T.crossing_errors(ex, eex)
    differ = int((st["updates"] != em["updates"]).sum())
    print(f"{name}: S {fig['S']:.3f} Wt {fig['Wt']:.3f} C {fig.get('C', 0):.3f} units on {fig['clear']} clear voxels; decisions differ on "
          f"{differ}; crossings {cf['common']} common, t {cf.get('t', 0):.3f} point {cf.get('point', 0):.3f} normal "
          f"{cf.get('normal', 0):.3f} ({cf.get('normal_abs_deg', 0):.2e} deg) colour {cf.get('color', 0):.3f} units")
    assert differ == 0 and fig["nonfinite"] == 0
    assert fig["S"] <= T.FLOORS["S"] and fig["Wt"] <= T.FLOORS["Wt"] and fig.get("C", 0) <= T.FLOORS["C"]
    assert cf["missing_clear"] == 0 and cf["extra_clear"] == 0 and len(cf["extra"]) == 0
    for k in ("t", "point", "normal", "color"):
        assert cf.get(k, 0) <= T.FLOORS[k], k
    assert cf.get("normal_zero_mismatch", 0) == 0


def test_world_offset_changes_no_rounded_view():
    """A grid and its cameras moved by (300, -200, 500) m hand the device the same fp32 R and t'."""
    grid, views = T.fixture("eight")
    off = np.array([300.0, -200.0, 500.0])
    for vw in views:
        R0, t0 = T.recentre(vw, grid["origin"])
        moved = dict(vw, t=vw["t"] - vw["R"] @ off)
        R1, t1 = T.recentre(moved, np.asarray(grid["origin"]) + off)
        assert np.array_equal(R0.astype(np.float32), R1.astype(np.float32)) and np.array_equal(t0.astype(np.float32), t1.astype(np.float32))
        assert np.abs(t1 - t0).max() < 1e-12


# ----------------------------------------------------------------------------------------------------------------------
# host code: grid, images, files, metrics
# ----------------------------------------------------------------------------------------------------------------------
def test_grid_for_bounds():
    from touch_gs_amd.tsdf import grid_for_bounds
    lo, vox, dims = grid_for_bounds(([0.0, -1.0, 2.0], [1.0, 1.0, 2.5]), resolution=64)
    assert vox == 2.0 / 64 and dims == (32, 64, 16) and np.array_equal(lo, [0.0, -1.0, 2.0])
    _, vox, dims = grid_for_bounds(([0, 0, 0], [1.0, 0.55, 0.1]), resolution=None, voxel_size=0.1)
    assert vox == 0.1 and dims == (10, 6, 1)
    with pytest.raises(ValueError):
        grid_for_bounds(([0, 0, 0], [1, 0, 1]))


def test_fusion_images_gate_and_weight():
    import torch
    from touch_gs_amd.tsdf import fusion_images
    H, W = 6, 8
    exp = torch.full((H, W), 2.0)
    exp[:, 4:] = 3.0                                   # a step of 50 % between columns 3 and 4
    med = exp + 0.0625
    gid = torch.zeros(H, W, dtype=torch.int32)
    gid[0, 0] = -1                                     # no median there: the expected depth
    alpha = torch.ones(H, W)
    alpha[5, 7] = 0.4
    var = torch.full((H, W), 0.03)
    out = dict(alpha=alpha, depth=exp[..., None], median_depth=med[..., None], median_gid=gid, depth_var=var[..., None])
    d, w = fusion_images(out, "median", "inverse_variance", alpha_min=0.5, max_jump=0.1, var_floor=0.01)
    assert d[0, 0] == 2.0 and d[1, 1] == 2.0625 and d[2, 6] == 3.0625
    assert not d[:, 3:5].any() and d[:, :3].all() and d[:-1, 5:].all()      # the gate takes the two columns at the step
    assert d[5, 7] == 0.0
    assert torch.allclose(w, torch.full((H, W), 0.25)) and d.dtype == torch.float32 and d.is_contiguous()
    d2, w2 = fusion_images(out, "expected", "uniform", alpha_min=0.5, max_jump=0.0)
    assert w2 is None and d2[0, 3] == 2.0 and d2[0, 4] == 3.0 and d2[5, 7] == 0.0
    with pytest.raises(ValueError):
        fusion_images(out, "mean")


read_ply = T.read_ply


def test_write_ply_round_trip(tmp_path):
    from touch_gs_amd.tsdf import write_ply
    rng = np.random.default_rng(0)
    p, n, c = rng.normal(size=(17, 3)), rng.normal(size=(17, 3)).astype(np.float32), rng.random((17, 3))
    write_ply(str(tmp_path / "a.ply"), p, n, c)
    names, rec = read_ply(tmp_path / "a.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1), p.astype(np.float32))
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], -1), n)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], -1), np.rint(c * 255).astype(np.uint8))
    write_ply(str(tmp_path / "b.ply"), p[:0])
    names, rec = read_ply(tmp_path / "b.ply")
    assert names == ["x", "y", "z"] and len(rec) == 0


def test_gaussian_ply_layout(tmp_path):
    """Three Gaussians with distinct values everywhere: the INRIA column order, f_rest channel-major."""
    from touch_gs_amd.export import write_gaussian_ply
    N, K = 3, 4
    means = np.arange(9, dtype=np.float32).reshape(N, 3) + 0.5
    sh = (100 + np.arange(N * K * 3, dtype=np.float32)).reshape(N, K, 3)
    opac = np.array([-1.0, 0.25, 2.0], np.float32)
    ls = -np.arange(1, 10, dtype=np.float32).reshape(N, 3)
    q = (200 + np.arange(12, dtype=np.float32)).reshape(N, 4)
    write_gaussian_ply(str(tmp_path / "point_cloud.ply"), means, sh, opac, ls, q)
    names, rec = read_ply(tmp_path / "point_cloud.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(9)] \
        + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    for g in range(N):
        assert [rec[k][g] for k in ("x", "y", "z")] == list(means[g]) and not any(rec[k][g] for k in ("nx", "ny", "nz"))
        assert [rec[f"f_dc_{c}"][g] for c in range(3)] == list(sh[g, 0])
        for c in range(3):
            for k in range(1, K):
                assert rec[f"f_rest_{c * (K - 1) + (k - 1)}"][g] == sh[g, k, c]
        assert rec["opacity"][g] == opac[g]
        assert [rec[f"scale_{i}"][g] for i in range(3)] == list(ls[g]) and [rec[f"rot_{i}"][g] for i in range(4)] == list(q[g])


def test_surface_metrics_against_brute_force():
    from touch_gs_amd.tsdf import surface_metrics
    rng = np.random.default_rng(3)
    p, g = rng.normal(size=(50, 3)), rng.normal(size=(50, 3)) + 0.1
    tau = 0.4
    d = np.linalg.norm(p[:, None] - g[None], axis=2)
    d_pg, d_gp = d.min(1), d.min(0)
    prec, rec = (d_pg <= tau).mean(), (d_gp <= tau).mean()
    m = surface_metrics(p, g, tau)
    assert abs(m["chamfer"] - 0.5 * (d_pg.mean() + d_gp.mean())) < 1e-12
    assert m["precision"] == prec and m["recall"] == rec and abs(m["fscore"] - 2 * prec * rec / (prec + rec)) < 1e-12
    assert 0 < prec < 1 and 0 < rec < 1
    same = surface_metrics(p, p, 1e-9)
    assert same["chamfer"] == 0 and same["fscore"] == 1.0
    assert surface_metrics(p[:0], g, tau)["fscore"] == 0.0


def test_frames_round_trip_and_cli_flags():
    import inspect
    from types import SimpleNamespace
    from touch_gs_amd import export, run_eval
    scene = SimpleNamespace(scale=2.5, _centre=np.array([0.3, -0.2, 1.0]))
    p = np.array([[0.1, 0.2, 0.3], [-1.0, 4.0, 0.5]])
    assert np.allclose(export.to_model_frame(export.to_capture_frame(p, scene), scene), p, atol=1e-15)
    assert np.allclose(export.to_model_frame(scene._centre, scene), 0)
    src = inspect.getsource(export.main)
    for flag in ("--run", "--output-dir", "--resolution", "--voxel-size", "--bounds", "--depth", "--weight", "--views"):
        assert f'"{flag}"' in src, flag
    assert '"--surface"' in inspect.getsource(run_eval.main) and "surface" in inspect.signature(run_eval.eval_run).parameters
