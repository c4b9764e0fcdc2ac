"""CPU tests of the TSDF triangle mesh (tgs_tsdf_mesh_count / tgs_tsdf_mesh_emit, TsdfVolume.extract_mesh, tsdf.mesh_stats,
export tsdf --mesh): the ABI and the argument checks, the case table in csrc/tsdf.hip against the one the
reference generates, the properties of the fp64 reference tests/tsdf_mesh_ref.py on the analytic states, its agreement with
the point extraction of tests/tsdf_ref.py, the fp32 emulation's floors on all seven edge classes (printed; the GPU bars of
tests/test_gpu_tsdf_mesh.py are 4 x them), the PLY faces and the mesh statistics.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import tsdf_mesh_ref as M
import tsdf_ref as T

TGS_E_ARG = -1          # include/tgs.h
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {
    "tgs_tsdf_mesh_count": ["nx", "ny", "nz", "vox", "S", "Wt", "w_min", "vmask", "ntri", "flags", "stream"],
    "tgs_tsdf_mesh_emit": ["nx", "ny", "nz", "vox", "S", "Wt", "C", "w_min", "flags", "vmask", "vert_offsets", "tri_offsets",
                           "points", "normals", "colors", "edge_key", "faces", "stream"],
}


def test_entry_points_are_declared_exported_and_bound_within_version_320():
    from touch_gs_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert re.search(r"#define\s+TGS_VERSION\s+320\b", txt) and lib.tgs_version() == 320
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, want in NAMES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, f"prototype of {name} missing from include/tgs.h"
        assert [a.split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")] == want
        res, argtypes = _lib.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == len(want) and hasattr(lib, name)


def test_argument_validation_launches_nothing():
    """Every refusal comes back before a launch: the pointers handed in are host memory."""
    from touch_gs_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    p = C.cast(buf, C.c_void_p)
    err = lambda: lib.tgs_last_error()

    def count(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return lib.tgs_tsdf_mesh_count(g("nx", 4), 4, g("nz", 4), C.c_float(g("vox", 0.1)), g("S", p), g("Wt", p),
                                       C.c_float(g("w_min", 0.5)), g("vmask", p), g("ntri", p), g("flags", p), None)
    assert count(w_min=0.0) == TGS_E_ARG and b"w_min" in err()
    assert count(w_min=-1.0) < 0 and count(w_min=float("nan")) < 0
    assert count(nx=0) == TGS_E_ARG and b"dims" in err()
    assert count(nz=-2) < 0 and count(vox=0.0) < 0 and b"voxel size" in err()
    assert count(nx=1 << 29) < 0 and b"index" in err()
    assert count(S=None) < 0 and b"null" in err()
    assert count(Wt=None) < 0 and count(vmask=None) < 0 and count(ntri=None) < 0
    assert count(flags=None) == TGS_E_ARG and b"null" in err()

    def emit(**kw):
        g = lambda k, d: kw[k] if k in kw else d
        return lib.tgs_tsdf_mesh_emit(g("nx", 4), 4, 4, C.c_float(g("vox", 0.1)), g("S", p), g("Wt", p), g("C", None),
                                      C.c_float(g("w_min", 0.5)), g("flags", p), g("vmask", p), g("vert_offsets", p),
                                      g("tri_offsets", p), g("points", p), g("normals", p), g("colors", None), g("edge_key", None),
                                      g("faces", p), None)
    assert emit(w_min=0.0) == TGS_E_ARG and b"w_min" in err()
    assert emit(nx=0) < 0 and emit(vox=-1.0) < 0 and emit(nx=1 << 29) < 0
    for k in ("S", "Wt", "flags", "vmask", "vert_offsets", "tri_offsets", "points", "normals", "faces"):
        assert emit(**{k: None}) == TGS_E_ARG and b"null" in err(), k
    assert emit(colors=p) == TGS_E_ARG and b"colors without C" in err()


def test_case_table_in_the_kernel_source_is_the_generated_one():
    src = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "tsdf.hip")).read()
    m = re.search(r"// TSDF_TET_CASES begin\n(.*?)\n// TSDF_TET_CASES end", src, flags=re.S)
    assert m, "the marker comments around the case table are missing"
    assert m.group(1) == M.case_table_text()
    # what the table must be, whatever generated it: 1 or 3 inside -> one triangle of the three cut edges, 2 -> two that
    # share the diagonal, the complement case = the same triangles reversed, odd = even mirrored
    even, odd = M.case_table()
    for case in range(16):
        cut = {n for n, (p, q) in enumerate(M.TET_EDGES) if (case >> p & 1) != (case >> q & 1)}
        tris = even[case]
        assert len(tris) == {0: 0, 3: 1, 4: 2}[len(cut)] and {e for t in tris for e in t} == cut
        assert all(len(set(t)) == 3 for t in tris)
        if len(tris) == 2:
            assert len(set(tris[0]) & set(tris[1])) == 2
        rev = lambda ts: sorted(tuple(sorted((t[0], t[2], t[1]))) for t in ts)
        assert sorted(tuple(sorted(t)) for t in odd[case]) == rev(tris)
        cyc = lambda t: {(t[0], t[1]), (t[1], t[2]), (t[2], t[0])}
        assert all(cyc(o) == {(b, a) for a, b in cyc(e)} for e, o in zip(tris, odd[case]))
    assert [M.parity(p) for p in M.PERMS] == [0, 1, 1, 0, 0, 1]


def test_packed_tables_in_the_kernel_source_are_the_definition():
    """The small tables the kernels carry as hex digits, against OFFSETS, PERMS and TET_EDGES of the reference."""
    src = open(os.path.join(ROOT, "touch_gs_amd", "csrc", "tsdf.hip")).read()
    const = lambda name: int(re.search(name + r" = (0x[0-9a-fA-F]+)u", src).group(1), 16)
    digit = lambda word, n: word >> 4 * n & 0xF
    bits = lambda d: d[0] + 2 * d[1] + 4 * d[2]
    for e, d in enumerate(M.OFFSETS):
        assert digit(const("TSDF_CLASS_BITS"), e) == bits(d) and digit(const("TSDF_BITS_CLASS"), bits(d)) == e
    for n, (p, q) in enumerate(M.TET_EDGES):
        assert (digit(const("TSDF_EDGE_P"), n), digit(const("TSDF_EDGE_Q"), n)) == (p, q)
    corners = [int(x, 16) for x in re.search(r"constexpr unsigned c\[6\] = \{(.*?)\};", src).group(1).replace("u", "").split(",")]
    for n, perm in enumerate(M.PERMS):
        assert [digit(corners[n], q) for q in range(4)] == [bits(c) for c in M.tet_corners(perm)]
        assert const("TSDF_TET_ODD") >> n & 1 == M.parity(perm)


def _mesh64(name):
    grid, st = M.analytic(name)
    return grid, st, M.extract_mesh(grid, st["S"], st["Wt"], st["C"], T.W_MIN)


def _ball_geometry(name):
    spec = M.BALLS[name]
    (ctr, r), = spec["balls"]
    return np.asarray(ctr) * M.AVOX, r * M.AVOX


def test_ball_is_a_closed_outward_sphere():
    grid, st, ex = _mesh64("ball")
    nv, vox = len(ex["edge_key"]), grid["vox"]
    top = M.topology(ex["faces"], nv)
    print(f"ball: {nv} vertices, {len(ex['faces'])} faces, {top['edges']} edges, chi {top['chi']}")
    assert top["boundary"] == 0 and top["nonmanifold"] == 0 and top["components"] == 1 and top["chi"] == 2
    assert set(ex["cls"].tolist()) == set(range(7))                          # every edge class carries vertices
    assert ex["ntri"].sum() == len(ex["faces"]) and ex["ntri"].max() <= 12 and ex["faces"].max() == nv - 1
    ctr, r = _ball_geometry("ball")
    fn = M.face_normals(ex["points"], ex["faces"])
    keep = np.linalg.norm(fn, axis=1) > 0
    radial = ex["points"][ex["faces"]].mean(1) - ctr
    assert ((fn * radial).sum(1)[keep] > 0).all()
    for q in range(3):
        assert ((fn * ex["normals"][ex["faces"][:, q]]).sum(1)[keep] > 0).all()
    dist = np.abs(np.linalg.norm(ex["points"] - ctr, axis=1) - r)
    vol = M.signed_volume(ex["points"], ex["faces"])
    ball = lambda rad: 4.0 / 3.0 * np.pi * rad ** 3
    print(f"ball: farthest vertex {dist.max() / vox:.3f} vox from the sphere; volume {vol:.6e} against {ball(r):.6e}")
    assert dist.max() <= np.sqrt(3.0) * vox
    assert ball(r - np.sqrt(3.0) * vox) <= vol <= ball(r + np.sqrt(3.0) * vox)
    assert ((ex["t"] >= 0) & (ex["t"] <= 1)).all() and (np.diff(ex["edge_key"]) > 0).all()
    # the surface stays two voxels from the border: every voxel within sqrt(3) vox of it
    i, j, k = T.voxel_indices(grid["dims"])
    near = ex["vmask"] != 0
    for idx, n in zip((i, j, k), grid["dims"]):
        assert idx[near].min() >= 2 and idx[near].max() <= n - 3


def test_two_balls_are_two_closed_components():
    grid, st, ex = _mesh64("two_balls")
    top = M.topology(ex["faces"], len(ex["edge_key"]))
    assert top["boundary"] == 0 and top["nonmanifold"] == 0 and top["components"] == 2 and top["chi"] == 4


def test_half_valid_ball_has_a_boundary_at_the_inactive_cells_only():
    grid, st, ex = _mesh64("ball_half_valid")
    nx, ny, nz = grid["dims"]
    top = M.topology(ex["faces"], len(ex["edge_key"]))
    print(f"ball_half_valid: {top['boundary']} boundary edges, most faces on an edge {top['edge_faces']}")
    assert top["boundary"] > 0 and top["edge_faces"] <= 2 and top["nonmanifold"] == 0 and top["components"] == 1
    active = ex["active"]
    for cell in np.unique(ex["face_cell"][top["boundary_faces"]]).tolist():
        i, j, k = cell % nx, (cell // nx) % ny, cell // (nx * ny)
        lonely = False
        for di, dj, dk in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            a, b, c = i + di, j + dj, k + dk
            inside = 0 <= a < nx - 1 and 0 <= b < ny - 1 and 0 <= c < nz - 1
            lonely |= not inside or not active[a + nx * (b + ny * c)]
        assert lonely, cell
    # no vertex beyond the plane, and none that no face references (extract_mesh asserts the latter itself)
    assert (T.voxel_indices(grid["dims"])[0][ex["b"]] < M.BALLS["ball_half_valid"]["invalid_from_i"]).all()


def test_ball_on_voxel_centres_keeps_its_degenerate_faces():
    grid, st, ex = _mesh64("ball_on_centres")
    valid = st["Wt"] >= T.W_MIN
    assert ((st["S"] == 0) & valid).sum() >= 6                                # f == 0 exactly at several centres
    fn = M.face_normals(ex["points"], ex["faces"])
    deg = int((np.linalg.norm(fn, axis=1) == 0).sum())
    top = M.topology(ex["faces"], len(ex["edge_key"]))
    print(f"ball_on_centres: {int(((st['S'] == 0) & valid).sum())} centres with f == 0, {deg} degenerate faces of {len(fn)}")
    assert deg > 0 and (ex["t"] == 0).any() | (ex["t"] == 1).any()
    assert top["boundary"] == 0 and top["nonmanifold"] == 0 and top["components"] == 1 and top["chi"] == 2
    # f == 0 counts as outside: no vertex has its inside end there
    inside_end = np.where(st["S"][ex["a"]] < 0, ex["a"], ex["b"])
    assert (st["S"][inside_end] < 0).all()


@pytest.mark.parametrize("corner", range(8))
def test_single_cell_with_one_corner_inside(corner):
    """The inside corner c meets the Kuhn edges to every u <= c or u >= c: 7 for 000 and 111, 4 for the others; every
    tetrahedron that holds c gives the one triangle of a one-inside case."""
    grid, st = M.analytic("single_cell")
    S = np.full(8, 0.5)
    S[corner] = -0.5
    if corner == 0:
        assert np.array_equal(S, st["S"])
    ex = M.extract_mesh(grid, S, st["Wt"], st["C"], T.W_MIN)
    bits = [corner & 1, corner >> 1 & 1, corner >> 2 & 1]
    want_v = sum(1 for u in M.CORNERS if tuple(u) != tuple(bits) and (all(a <= b for a, b in zip(u, bits)) or all(a >= b for a, b in zip(u, bits))))
    want_f = 0
    for perm in M.PERMS:
        tc = M.tet_corners(perm)
        if tuple(bits) in tc:
            want_f += len(M.case_table()[M.parity(perm)][1 << tc.index(tuple(bits))])
    assert want_v == (7 if corner in (0, 7) else 4) and want_f == (6 if corner in (0, 7) else 2)
    assert len(ex["edge_key"]) == want_v and len(ex["faces"]) == want_f and ex["ntri"][0] == want_f and not ex["ntri"][1:].any()
    # outward: away from the inside corner
    c = (np.asarray(bits) + 0.5) * grid["vox"]
    fn = M.face_normals(ex["points"], ex["faces"])
    assert ((fn * (ex["points"][ex["faces"]].mean(1) - c)).sum(1) > 0).all()


@pytest.mark.parametrize("name", ["thin_z", "thin_x"])
def test_grids_without_cells_are_empty(name):
    ex = M.reference32(name)
    assert len(ex["edge_key"]) == 0 and ex["faces"].shape == (0, 3) and not ex["vmask"].any() and not ex["ntri"].any()
    assert len(T.reference(name)[1]["edge_id"]) == 1                         # (the point extraction does find a crossing there)


@pytest.mark.parametrize("name", T.ALL)
def test_axis_vertices_are_crossings_of_the_point_extraction(name):
    """Classes 0 ... 2 are the edges that edge_id = 3 a + axis names: a subset of tsdf_ref.extract's crossings (an edge outside
    every active cell has a crossing and no vertex), with equal t, point, normal and colour."""
    grid, _ = T.fixture(name)
    st, ex = T.reference(name)
    me = M.extract_mesh(grid, st["S"], st["Wt"], st["C"], T.W_MIN)
    axis = me["cls"] < 3
    eid = 3 * me["a"][axis] + me["cls"][axis]
    pos = np.searchsorted(ex["edge_id"], eid)
    assert (pos < max(len(ex["edge_id"]), 1)).all() and np.array_equal(ex["edge_id"][pos], eid)
    print(f"{name}: {int(axis.sum())} axis-edge vertices of {len(ex['edge_id'])} crossings; {int((~axis).sum())} on diagonals")
    for k in ("t", "points", "normals", "colors"):
        assert np.array_equal(me[k][axis], ex[k][pos]), k
    assert name in ("thin_z", "thin_x", "behind") or (axis.sum() > 100 and (~axis).sum() > 100)


def test_fp32_emulation_gives_the_floors(capsys):
    """The definition in NumPy fp32 against fp64 ON THE SAME fp32-rounded state, all seven edge classes, in the units of
    tests/tsdf_ref.py.  Validity and signs are then equal by construction: the topology arrays must be EQUAL.  Measured
    (largest over tsdf_ref.ALL and the analytic states): t and point 0.5454 (two_balls), normal 0.0799 (ball), colour 0.5336
    (eight).  t and point exceed tsdf_ref.FLOORS (0.511), so tsdf_mesh_ref.FLOORS holds the mesh's own, rounded up in the
    third digit."""
    worst = dict(t=0.0, point=0.0, normal=0.0, color=0.0)
    for name in T.ALL + M.ANALYTIC:
        ref, emu = M.reference32(name), M.emulation32(name)
        for k in ("vmask", "ntri", "edge_key", "faces"):
            assert np.array_equal(ref[k], emu[k]), (name, k)
        fig = M.vertex_errors(ref, emu)
        print(f"{name}: {fig['n']} vertices, {len(ref['faces'])} faces; t {fig['t']:.4f} point {fig['point']:.4f} normal "
              f"{fig['normal']:.4f} ({fig['normal_abs_deg']:.2e} deg) colour {fig['color']:.4f} units")
        assert fig["normal_zero_mismatch"] == 0
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    print("floors: " + ", ".join(f"{k} {v:.4f} (held to {M.FLOORS[k]})" for k, v in worst.items()))
    for k in worst:
        assert worst[k] <= M.FLOORS[k], k
    assert any(worst[k] > T.FLOORS[k] for k in worst), "within tsdf_ref.FLOORS: the mesh needs no floors of its own"
    assert M.BARS == {k: 4.0 * v for k, v in M.FLOORS.items()}


# ----------------------------------------------------------------------------------------------------------------------
# host code: files and statistics
# ----------------------------------------------------------------------------------------------------------------------
def test_write_ply_with_faces_and_without(tmp_path):
    from touch_gs_amd.tsdf import write_ply
    rng = np.random.default_rng(0)
    p, n, c = rng.normal(size=(5, 3)), rng.normal(size=(5, 3)).astype(np.float32), rng.random((5, 3))
    faces = np.array([[0, 1, 2], [2, 1, 3], [4, 0, 3]], np.int32)
    write_ply(str(tmp_path / "m.ply"), p, n, c, faces)
    names, rec, got = M.read_ply_mesh(tmp_path / "m.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and got.dtype == np.int32 and np.array_equal(got, faces)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1), p.astype(np.float32))
    head = open(tmp_path / "m.ply", "rb").read().split(b"end_header\n")[0].decode()
    assert "element face 3\nproperty list uchar int vertex_indices\n" in head
    # without faces: the bytes of the point-cloud writer as it was
    write_ply(str(tmp_path / "a.ply"), p, n, c)
    rec = np.empty(5, dtype=[(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz")] + [(k, "u1") for k in ("red", "green", "blue")])
    for q, k in enumerate(("x", "y", "z")):
        rec[k], rec["n" + k] = p[:, q], n[:, q]
    for q, k in enumerate(("red", "green", "blue")):
        rec[k] = np.rint(c[:, q] * 255)
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\n" + "".join(f"property float {k}\n" for k in rec.dtype.names[:6])
            + "".join(f"property uchar {k}\n" for k in rec.dtype.names[6:]) + "end_header\n").encode("ascii") + rec.tobytes()
    assert open(tmp_path / "a.ply", "rb").read() == want
    names, rec2 = T.read_ply(tmp_path / "a.ply")
    assert len(rec2) == 5
    write_ply(str(tmp_path / "e.ply"), p[:0], faces=np.zeros((0, 3), np.int32))
    assert M.read_ply_mesh(tmp_path / "e.ply")[2].shape == (0, 3)


def test_mesh_stats():
    from touch_gs_amd.tsdf import mesh_stats
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64) + np.array([300.0, -200.0, 500.0])
    f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])                 # outward
    s = mesh_stats(v, f)
    assert s["n_vertices"] == 4 and s["n_faces"] == 4 and s["boundary_edges"] == 0 and s["nonmanifold_edges"] == 0
    assert s["components"] == 1 and s["degenerate_faces"] == 0
    assert abs(s["volume"] - 1.0 / 6.0) < 1e-12 and abs(s["area"] - (1.5 + np.sqrt(3.0) / 2.0)) < 1e-12
    assert mesh_stats(v, f[:, ::-1])["volume"] < 0
    s = mesh_stats(v, f[:3])                                                  # open: the three edges of the missing face
    assert s["boundary_edges"] == 3 and s["nonmanifold_edges"] == 0
    s = mesh_stats(v, np.concatenate([f, f[:1]]))                             # a face twice: three edges with three faces
    assert s["nonmanifold_edges"] == 3
    s = mesh_stats(v, np.concatenate([f[:3], f[3:, ::-1]]))                   # one face flipped: its edges run the same way twice
    assert s["nonmanifold_edges"] == 3 and s["boundary_edges"] == 0
    s = mesh_stats(np.concatenate([v, v + 5.0, v[:1]]), np.concatenate([f, f + 4, [[0, 8, 1]]]))
    assert s["components"] == 2 and s["degenerate_faces"] == 1 and s["n_vertices"] == 9
    assert mesh_stats(v[:0], np.zeros((0, 3), np.int64)) == dict(n_vertices=0, n_faces=0, boundary_edges=0, nonmanifold_edges=0,
                                                                   components=0, area=0.0, volume=0.0, degenerate_faces=0)
    # against the reference's checker, on meshes of the definition
    for name in ("ball", "ball_half_valid", "two_balls", "ball_on_centres"):
        grid, st, ex = _mesh64(name)
        s, top = mesh_stats(ex["points"], ex["faces"]), M.topology(ex["faces"], len(ex["edge_key"]))
        assert (s["boundary_edges"], s["nonmanifold_edges"], s["components"]) == (top["boundary"], top["nonmanifold"], top["components"])
        # (mesh_stats centres the vertices first: the same number where the mesh is closed, a choice of origin where not)
        assert abs(s["volume"] - M.signed_volume(ex["points"] - ex["points"].mean(0), ex["faces"])) < 1e-12
        assert top["boundary"] or abs(s["volume"] - M.signed_volume(ex["points"], ex["faces"])) < 1e-12
        assert s["degenerate_faces"] == int((np.linalg.norm(M.face_normals(ex["points"], ex["faces"]), axis=1) == 0).sum())


def test_cli_flag_and_python_api_exist():
    from touch_gs_amd import export, tsdf
    assert '"--mesh"' in inspect.getsource(export.main) and "mesh" in inspect.signature(export.export_tsdf).parameters
    assert inspect.signature(export.export_tsdf).parameters["mesh"].default is False
    assert list(inspect.signature(tsdf.TsdfVolume.extract_mesh_local).parameters) == ["self", "w_min", "want_colors"]
    assert list(inspect.signature(tsdf.TsdfVolume.extract_mesh).parameters) == ["self", "w_min"]
    assert list(inspect.signature(tsdf.write_ply).parameters) == ["path", "points", "normals", "colors", "faces"]
