"""GPU tests of the TSDF triangle mesh (csrc/tsdf.hip: tgs_tsdf_mesh_count, tgs_tsdf_mesh_emit; TsdfVolume.extract_mesh_local /
extract_mesh, tsdf.mesh_stats, export tsdf --mesh) against the NumPy definition tests/tsdf_mesh_ref.py.

The pin: the fp64 reference state of every tsdf_ref fixture and every analytic state, rounded to fp32 and copied into a
TsdfVolume.  Validity and signs are then the reference's by construction, so vmask, ntri, edge_key and faces must be EQUAL
-- no exclusions, no cap -- and t, points, normal angles and colours lie within tsdf_mesh_ref.BARS = 4 x the fp32 emulation's
floors (t and point 2.184, normal 0.320, colour 2.136 units; units: tests/tsdf_ref.py, floors: tests/test_cpu_tsdf_mesh.py).
Then the GPU's own integrated state against the fp32 emulation (topology equal, axis-edge vertices bit-identical to the rows
of extract_local), determinism, a world offset, colour on and off, the empty cases, a Gaussian model and the command line.
Every buffer a kernel writes sits inside odd sentinel padding that is checked after the calls.  The pin writes its measured
worst case per quantity to $TGS_REPORT_DIR/tsdf_mesh_report.json (where that is set); the figures are in DESIGN 5.1l.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tsdf_mesh_ref as M
import tsdf_ref as T

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
REPORT = {}
REPORT_DIR = os.environ.get("TGS_REPORT_DIR")        # where the pin leaves tsdf_mesh_report.json; unset: the figures are printed only


def _padded(n, dev, pad, body, dtype=None):
    """(whole buffer, the n-element body inside it): `pad` sentinel elements on either side."""
    import torch
    dtype = dtype or torch.float32
    sent = SENTINEL if dtype.is_floating_point else 123
    buf = torch.full((n + 2 * pad,), sent, dtype=dtype, device=dev)
    buf[pad:pad + n] = body
    return buf, buf[pad:pad + n]


def _pads_intact(buf, n, pad):
    sent = SENTINEL if buf.dtype.is_floating_point else 123
    return bool((buf[:pad] == sent).all()) and bool((buf[pad + n:] == sent).all())


class Volume:
    """A TsdfVolume whose state lives inside sentinel padding (odd pads: addresses that are no multiple of 8 or 16 bytes)."""

    def __init__(self, grid, dev, pad=61, color=True, origin=None):
        from touch_gs_amd.tsdf import TsdfVolume
        self.grid, self.pad, self.dev = grid, pad, dev
        self.vol = TsdfVolume(grid["origin"] if origin is None else origin, grid["vox"], grid["dims"], grid["trunc"], dev, color=color)
        V = self.V = self.vol.num_voxels
        self.bufS, self.vol.S = _padded(V, dev, pad, 0.0)
        self.bufW, self.vol.Wt = _padded(V, dev, pad, 0.0)
        self.bufC = None
        if color:
            self.bufC, body = _padded(3 * V, dev, pad, 0.0)
            self.vol.C = body.view(V, 3)

    def load(self, S, Wt, Cc):
        import torch
        self.vol.S.copy_(torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)))
        self.vol.Wt.copy_(torch.from_numpy(np.ascontiguousarray(Wt, dtype=np.float32)))
        if self.vol.C is not None:
            self.vol.C.copy_(torch.from_numpy(np.ascontiguousarray(Cc, dtype=np.float32)))
        return self

    def integrate(self, views, offset=None):
        import torch
        from touch_gs_amd import Camera
        cams, depths, weights, rgbs = [], [], [], []
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
        for vw in views:
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = vw["R"], vw["t"] if offset is None else vw["t"] - vw["R"] @ offset
            cams.append(Camera(m, vw["fx"], vw["fy"], vw["cx"], vw["cy"], vw["W"], vw["H"], near=vw["near"], pix_center=vw["pix_center"]))
            depths.append(up(vw["depth"]))
            weights.append(up(vw.get("weight")))
            rgbs.append(None if self.vol.C is None else up(vw.get("rgb")))
        self.vol.integrate(cams, depths, weights, rgbs)
        torch.cuda.synchronize(self.dev)
        return self

    def state(self):
        return (self.vol.S.cpu().numpy(), self.vol.Wt.cpu().numpy(), None if self.vol.C is None else self.vol.C.cpu().numpy())

    def pads_intact(self):
        return _pads_intact(self.bufS, self.V, self.pad) and _pads_intact(self.bufW, self.V, self.pad) and \
            (self.bufC is None or _pads_intact(self.bufC, 3 * self.V, self.pad))

    def mesh(self, w_min=T.W_MIN, pad=63, want_edge_key=True):
        """The two calls on prefilled, sentinel-padded outputs -> host arrays, whether the padding survived, and whether the
        emit was needed."""
        import torch
        from touch_gs_amd import _lib
        lib = _lib.load()
        v, dev, V = self.vol, self.dev, self.V
        nx, ny, nz = v.dims
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        u8 = torch.uint8
        (bufM, vmask), (bufT, ntri), (bufF, flags) = (_padded(V, dev, pad, 200, u8) for _ in range(3))
        with torch.cuda.device(dev):
            _lib.check(lib.tgs_tsdf_mesh_count(nx, ny, nz, C.c_float(v.voxel_size), _lib.ptr(v.S), _lib.ptr(v.Wt), C.c_float(w_min),
                                               _lib.ptr(vmask), _lib.ptr(ntri), _lib.ptr(flags), stream))
            hm, ht = vmask.cpu().numpy(), ntri.cpu().numpy()
            nvert = np.array([bin(m).count("1") for m in range(256)])[hm]
            n_v, n_f = int(nvert.sum()), int(ht.sum())
            voff = torch.from_numpy(np.cumsum(nvert) - nvert).to(dev)
            toff = torch.from_numpy(np.cumsum(ht.astype(np.int64)) - ht).to(dev)
            nan = float("nan")
            bufP, points = _padded(3 * n_v, dev, pad, nan)
            bufN, normals = _padded(3 * n_v, dev, pad, nan)
            bufCo, colors = _padded(3 * n_v, dev, pad, nan)
            bufK, key = _padded(n_v, dev, pad, -1, torch.int64)
            bufFa, faces = _padded(3 * n_f, dev, pad, -1, torch.int32)
            if v.C is None:
                colors = None
            if n_v:
                _lib.check(lib.tgs_tsdf_mesh_emit(nx, ny, nz, C.c_float(v.voxel_size), _lib.ptr(v.S), _lib.ptr(v.Wt), _lib.ptr(v.C),
                                                  C.c_float(w_min), _lib.ptr(flags), _lib.ptr(vmask), _lib.ptr(voff), _lib.ptr(toff),
                                                  _lib.ptr(points), _lib.ptr(normals), _lib.ptr(colors),
                                                  _lib.ptr(key) if want_edge_key else None, _lib.ptr(faces), stream))
            torch.cuda.synchronize(dev)
        intact = all(_pads_intact(b, V, pad) for b in (bufM, bufT, bufF)) and all(_pads_intact(b, 3 * n_v, pad) for b in (bufP, bufN, bufCo)) \
            and _pads_intact(bufK, n_v, pad) and _pads_intact(bufFa, 3 * n_f, pad) and self.pads_intact()
        return dict(vmask=hm, ntri=ht, edge_key=key.cpu().numpy(), points=points.cpu().numpy().reshape(n_v, 3),
                    normals=normals.cpu().numpy().reshape(n_v, 3), colors=None if colors is None else colors.cpu().numpy().reshape(n_v, 3),
                    faces=faces.cpu().numpy().reshape(n_f, 3), intact=intact)


def _local(vol, w_min=T.W_MIN, **kw):
    import torch
    loc = vol.extract_mesh_local(w_min, **kw)
    torch.cuda.synchronize(vol.device)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in loc.items()}


def _assert_topology_equal(name, ref, got):
    for k in ("vmask", "ntri", "edge_key", "faces"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (name, k)
    assert got["faces"].dtype == np.int32 and got["vmask"].dtype == np.uint8 and got["ntri"].dtype == np.uint8
    assert np.isfinite(got["points"]).all() and np.isfinite(got["normals"]).all()        # no prefilled NaN left in a row
    assert got["colors"] is None or np.isfinite(got["colors"]).all()


@pytest.mark.parametrize("name,pad", [(n, 61 + 2 * (q % 2)) for q, n in enumerate(T.ALL + M.ANALYTIC)])
def test_pin_against_the_fp64_reference_on_the_same_fp32_state(name, pad, dev):
    grid, S, Wt, Cc, _, _ = M.state32(name)
    ref = M.reference32(name)
    vol = Volume(grid, dev, pad).load(S, Wt, Cc)
    got = vol.mesh(pad=pad + 2)
    assert got["intact"]
    _assert_topology_equal(name, ref, got)
    fig = M.vertex_errors(ref, got)
    print(f"{name}: {fig['n']} vertices, {len(ref['faces'])} faces equal; t {fig['t']:.3f} (bar {M.BARS['t']:.3f}) point {fig['point']:.3f} "
          f"({M.BARS['point']:.3f}) normal {fig['normal']:.3f} ({M.BARS['normal']:.3f}; {fig['normal_abs_deg']:.2e} deg) colour "
          f"{fig['color']:.3f} ({M.BARS['color']:.3f}) units")
    REPORT[name] = dict(vertices=fig["n"], faces=int(len(ref["faces"])), **{k: fig[k] for k in ("t", "point", "normal", "color", "normal_abs_deg")})
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "tsdf_mesh_report.json"), "w") as f:
            worst = {k: max(r[k] for r in REPORT.values()) for k in ("t", "point", "normal", "color")}
            json.dump(dict(bars=M.BARS, floors=M.FLOORS, worst=worst, states=REPORT), f, indent=2)
    for k in ("t", "point", "normal", "color"):
        assert fig[k] <= M.BARS[k], k
    assert fig["normal_zero_mismatch"] == 0
    # the public path gives the same arrays
    loc = _local(vol.vol)
    for k in ("vmask", "ntri", "edge_key", "faces", "points", "normals", "colors"):
        assert loc[k].tobytes() == got[k].tobytes(), k
    world = vol.vol.extract_mesh(T.W_MIN)
    assert world["vertices"].dtype == np.float64 and world["faces"].dtype == np.int32
    assert np.array_equal(world["vertices"], got["points"].astype(np.float64).reshape(-1, 3) + np.asarray(grid["origin"]))
    assert np.array_equal(world["faces"], got["faces"]) and np.array_equal(world["edge_key"], got["edge_key"])


@pytest.mark.parametrize("name", T.ALL)
def test_integrated_state_end_to_end(name, dev):
    """The existing kernel's own state: its mesh equals the fp32 emulation's on the downloaded arrays in every topology
    array, and the vertices on axis edges are, bit for bit, the rows of extract_local with the same edge (one device function
    forms both)."""
    grid, views = T.fixture(name)
    vol = Volume(grid, dev, 63).integrate(views)
    S, Wt, Cc = vol.state()
    emu = M.extract_mesh(grid, S, Wt, Cc, T.W_MIN, dtype=np.float32)
    got = vol.mesh()
    assert got["intact"]
    _assert_topology_equal(name, emu, got)
    import torch
    pts = vol.vol.extract_local(T.W_MIN)
    torch.cuda.synchronize(dev)
    eid = pts["edge_id"].cpu().numpy()
    cls, a = got["edge_key"] % 7, got["edge_key"] // 7
    axis = cls < 3
    pos = np.searchsorted(eid, 3 * a[axis] + cls[axis])
    assert (pos < max(len(eid), 1)).all() and np.array_equal(eid[pos], 3 * a[axis] + cls[axis])
    for k in ("points", "normals", "colors"):
        assert pts[k].cpu().numpy()[pos].tobytes() == got[k][axis].tobytes(), k
    print(f"{name}: {len(cls)} vertices ({int(axis.sum())} on axis edges, bit-identical to the point rows), {len(got['faces'])} faces")


def test_two_extractions_give_the_same_bytes(dev):
    grid, views = T.fixture("eight")
    vol = Volume(grid, dev).integrate(views)
    a, b, c = vol.mesh(), vol.mesh(), _local(vol.vol)
    for k in ("vmask", "ntri", "edge_key", "faces", "points", "normals", "colors"):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k
    assert a["intact"] and b["intact"] and len(a["faces"]) > 1000


def test_world_offset_gives_the_same_grid_local_bits(dev):
    grid, views = T.fixture("eight")
    off = np.array([300.0, -200.0, 500.0])
    here = Volume(grid, dev).integrate(views)
    there = Volume(grid, dev, origin=np.asarray(grid["origin"]) + off).integrate(views, offset=off)
    a, b = _local(here.vol), _local(there.vol)
    for k in ("vmask", "ntri", "edge_key", "faces", "points", "normals", "colors"):
        assert a[k].tobytes() == b[k].tobytes(), k
    va, vb = here.vol.extract_mesh(T.W_MIN)["vertices"], there.vol.extract_mesh(T.W_MIN)["vertices"]
    assert len(va) > 1000 and np.abs((vb - off) - va).max() < 1e-10


def test_colour_changes_nothing_else(dev):
    grid, S, Wt, Cc, _, _ = M.state32("eight")
    with_c = Volume(grid, dev).load(S, Wt, Cc)
    without = Volume(grid, dev, color=False).load(S, Wt, None)
    a, b = with_c.mesh(), without.mesh(want_edge_key=False)
    assert a["intact"] and b["intact"] and b["colors"] is None and a["colors"] is not None
    for k in ("vmask", "ntri", "faces", "points", "normals"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (b["edge_key"] == -1).all() and len(b["edge_key"]) == len(a["edge_key"])          # edge_key = NULL: rows left alone
    c = _local(with_c.vol, want_colors=False)
    assert c["colors"] is None and c["points"].tobytes() == a["points"].tobytes() and c["faces"].tobytes() == a["faces"].tobytes()
    with pytest.raises(ValueError):
        without.vol.extract_mesh_local(T.W_MIN, want_colors=True)


@pytest.mark.parametrize("case", ["thin_x", "thin_z", "flat_y", "all_invalid"])
def test_empty_cases_launch_no_emit(case, dev, monkeypatch):
    from touch_gs_amd import _lib
    if case == "all_invalid":
        grid, S, Wt, Cc, _, _ = M.state32("ball")
        Wt = np.zeros_like(Wt)
    elif case == "flat_y":
        grid = dict(dims=(9, 1, 7), vox=M.AVOX, origin=(0.0, 0.0, 0.0), trunc=3 * M.AVOX)
        i = T.voxel_indices(grid["dims"])[0]
        S, Wt, Cc = np.where(i < 4, -0.5, 0.5), np.ones(63), np.full((63, 3), 0.5)
    else:
        grid, S, Wt, Cc, _, _ = M.state32(case)
    vol = Volume(grid, dev).load(S, Wt, Cc)
    lib = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(lib, name)
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    loc = _local(vol.vol)
    world = vol.vol.extract_mesh(T.W_MIN)
    assert calls == ["tgs_tsdf_mesh_count", "tgs_tsdf_mesh_count"]
    assert loc["points"].shape == (0, 3) and loc["normals"].shape == (0, 3) and loc["colors"].shape == (0, 3)
    assert loc["faces"].shape == (0, 3) and loc["faces"].dtype == np.int32 and loc["edge_key"].shape == (0,)
    assert not loc["vmask"].any() and not loc["ntri"].any() and vol.pads_intact()
    assert world["vertices"].shape == (0, 3) and world["vertices"].dtype == np.float64 and world["faces"].shape == (0, 3)


def _sphere_model(dev, n=4000, seed=0):
    """The 4 k-Gaussian sphere of tests/test_gpu_tsdf.py::test_model_end_to_end."""
    import torch
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    means = torch.from_numpy((np.asarray(T.SPHERE_C) + T.SPHERE_R * d).astype(np.float32))
    log_scales = torch.full((n, 3), float(np.log(0.005)))
    quats = torch.zeros(n, 4)
    quats[:, 0] = 1.0
    opac = torch.full((n,), 6.0)
    sh = torch.from_numpy(((0.5 + 0.4 * d) - 0.5) / 0.28209479177387814).float()[:, None, :].contiguous()
    params = GaussianParams.from_tensors(*[t.to(dev) for t in (means, log_scales, quats, opac, sh)])
    return DepthGaussianSplattingModel(ModelConfig(sh_degree=0, sh_degree_interval=0), params)


def test_model_end_to_end(dev):
    import torch
    from touch_gs_amd import Camera, tsdf
    model = _sphere_model(dev)
    img = dict(W=96, H=72, fx=110.0, fy=110.0, cx=47.6, cy=36.2)
    cams = []
    for pos in T.CAM_POS + [(-0.5, -0.1, 0.2), (0.1, 0.5, -0.25), (-0.05, -0.2, -0.5)]:
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = T.look_at(pos, target=T.SPHERE_C)
        cams.append(Camera(m, **img))
    c = np.asarray(T.SPHERE_C)
    with torch.cuda.device(dev):
        vol = tsdf.fuse_model(model, cams, (c - 0.15, c + 0.15), resolution=24, trunc_voxels=3)
        mesh = vol.extract_mesh(T.W_MIN)
        torch.cuda.synchronize()
    stats = tsdf.mesh_stats(mesh["vertices"], mesh["faces"])
    print(f"model: {stats}")
    assert stats["nonmanifold_edges"] == 0 and stats["n_vertices"] > 300 and stats["n_faces"] > 600
    assert mesh["faces"].min() >= 0 and mesh["faces"].max() < stats["n_vertices"]
    grid = dict(dims=vol.dims, vox=vol.voxel_size, origin=vol.origin, trunc=vol.trunc)
    emu = M.extract_mesh(grid, vol.S.cpu().numpy(), vol.Wt.cpu().numpy(), vol.C.cpu().numpy(), T.W_MIN, dtype=np.float32)
    assert np.array_equal(mesh["faces"], emu["faces"]) and np.array_equal(mesh["edge_key"], emu["edge_key"])
    # outward, next to the sphere
    fn = M.face_normals(mesh["vertices"], mesh["faces"])
    radial = mesh["vertices"][mesh["faces"]].mean(1) - c
    assert np.median((fn * radial).sum(1) / np.maximum(np.linalg.norm(fn, axis=1) * np.linalg.norm(radial, axis=1), 1e-300)) > 0.9


def test_command_line_writes_the_mesh(dev, tmp_path):
    """The tiny capture and ten-step run of tests/test_gpu_tsdf.py's command-line test, its Gaussians put on the touch cloud:
    `export tsdf --mesh` writes mesh.ply with the vertices and faces of extract_mesh and the mesh block = mesh_stats; without
    the flag there is no mesh.ply and no mesh key."""
    import torch
    from touch_gs_amd import export, train, tsdf
    from touch_gs_amd.analytic_scene import prepare_capture, write_raw_capture
    from touch_gs_amd.dataset import Scene
    from touch_gs_amd.optim import GaussianParams
    root = str(tmp_path / "capture")
    write_raw_capture(root, n_views=2, n_touches=4, W=160, H=90, seed=3, gpis_max_points=150, device="cpu")
    prepare_capture(root, 0.5)
    with torch.cuda.device(dev):
        run = train.main(["--data", root, "--train-split-fraction", "0.5", "--max-num-iterations", "10", "--steps-per-eval", "10",
                          "--steps-per-save", "10", "--sh-degree", "1", "--num-gaussians", "2000", "--output-dir", str(tmp_path / "out")])
        scene = Scene(root, 0.5, "cpu")
        ckpt = [os.path.join(run, f) for f in sorted(os.listdir(run)) if f.endswith(".ckpt")][-1]
        sd = torch.load(ckpt, map_location="cpu")
        par = GaussianParams.views_of(sd["flat"], sd["N"], sd["K"])
        touch = np.load(os.path.join(root, "points_touch.npy")).astype(np.float64)
        rng = np.random.default_rng(0)
        on = touch[rng.integers(0, len(touch), sd["N"])] + rng.normal(size=(sd["N"], 3)) * 0.001
        par["means"].copy_(torch.from_numpy(((on - scene._centre) * scene.scale).astype(np.float32)))
        par["log_scales"].fill_(float(np.log(0.003 * scene.scale)))
        par["opac_logit"].fill_(6.0)
        torch.save(sd, ckpt)
        args = ["tsdf", "--run", run, "--resolution", "24", "--views", "all", "--depth", "expected", "--weight", "uniform"]
        plain = export.main(args + ["--output-dir", str(tmp_path / "plain")])
        info = export.main(args + ["--output-dir", str(tmp_path / "mesh"), "--mesh"])
        vol = tsdf.TsdfVolume.load(str(tmp_path / "mesh" / "tsdf.npz"), dev)
        mesh = vol.extract_mesh(0.5)
    assert sorted(os.listdir(tmp_path / "plain")) == ["export.json", "surface.ply", "tsdf.npz"] and "mesh" not in plain
    assert "mesh" not in json.load(open(tmp_path / "plain" / "export.json"))
    assert sorted(os.listdir(tmp_path / "mesh")) == ["export.json", "mesh.ply", "surface.ply", "tsdf.npz"]
    on_disk = json.load(open(tmp_path / "mesh" / "export.json"))
    assert set(on_disk) == set(json.load(open(tmp_path / "plain" / "export.json"))) | {"mesh"}
    assert open(tmp_path / "mesh" / "surface.ply", "rb").read() == open(tmp_path / "plain" / "surface.ply", "rb").read()
    names, rec, faces = M.read_ply_mesh(tmp_path / "mesh" / "mesh.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    verts = export.to_capture_frame(mesh["vertices"], scene)
    assert len(rec) == len(verts) > 50 and np.array_equal(faces, mesh["faces"]) and len(faces) > 100
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1), verts.astype(np.float32))
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], -1), mesh["normals"])
    stats = tsdf.mesh_stats(verts, mesh["faces"])
    block = dict(on_disk["mesh"])
    seconds = block.pop("seconds")
    assert block == stats == {k: v for k, v in info["mesh"].items() if k != "seconds"} and set(seconds) == {"extract", "write"}
    assert stats["nonmanifold_edges"] == 0 and stats["n_faces"] == len(faces)
    print(f"cli: {stats}")
