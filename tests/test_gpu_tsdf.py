"""GPU tests of the TSDF fusion and extraction (csrc/tsdf.hip: tgs_tsdf_integrate, tgs_tsdf_extract_count,
tgs_tsdf_extract_points; touch_gs_amd.tsdf, touch_gs_amd.export) against the fp64 NumPy definition
tests/tsdf_ref.py on its tiny fixtures: every clear voxel's S, Wt and C, the crossings as sets by edge_id, t, points, normals
and colours on the common crossings, the bytes under batching, repetition, missing optional inputs and a world offset, a
Gaussian model fused end to end, and the command line.

Units: tests/tsdf_ref.py.  Floors = the fp32 NumPy emulation of the header's arithmetic against fp64 (tests/test_cpu_tsdf.py
prints them): S 1.41, Wt 2.71, C 3.11, t 0.51, point 0.51, normal 0.18, colour 0.73 units, 0 differing decisions.  Bars =
4 x the floors (tsdf_ref.BARS): S 5.64, Wt 10.84, C 12.44, t 2.04, point 2.04, normal 0.73, colour 2.93 units.
Unclear voxels (within 1e-3 px of a pixel edge, 1e-4 of the near plane or 1e-5 of -trunc in some view; at most 3 % of a
fixture) are counted and printed, not asserted.

Measured on the MI355X (each test prints its figures next to the bars; the table is in DESIGN 5.1k): the kernel is built
without contraction and gives the emulation's figures to every printed digit -- worst fixture S 1.41, Wt 2.70, C 3.11 (eight),
t and point 0.51 (weights_rgb), normal 0.18 (plane_behind), colour 0.73 (eight); crossing sets equal in every fixture (858 /
2243 / 1606 / 245 / 1 / 1 / 0 / 2289), no crossing with an end that is not sign-clear; unclear voxels 0 - 2.25 %, of which 1
differs (eight).  The Gaussian sphere: S 1.26, Wt 1.88, C 1.88, t 0.47, normal 0.10, colour 0.70 units; 1812 points at a median
of 8.0 mm from the sphere, voxel 12.5 mm, median render error 5.0 mm.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tsdf_ref as T

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


def _padded(n, dev, pad, body, dtype=None):
    """(whole buffer, the n-element body inside it): `pad` sentinel elements on either side."""
    import torch
    dtype = dtype or torch.float32
    sent = SENTINEL if dtype.is_floating_point else 12345
    buf = torch.full((n + 2 * pad,), sent, dtype=dtype, device=dev)
    buf[pad:pad + n] = body
    return buf, buf[pad:pad + n]


def _pads_intact(buf, n, pad):
    sent = SENTINEL if buf.dtype.is_floating_point else 12345
    return bool((buf[:pad] == sent).all()) and bool((buf[pad + n:] == sent).all())


class Volume:
    """A TsdfVolume whose state lives inside sentinel padding; pad = 61 or 62 floats puts S, Wt and C at addresses that are
    no multiple of 16 (or 8) bytes -- the kernel has one path, 4 bytes per lane, and must not care."""

    def __init__(self, grid, dev, pad=64, color=True, origin=None):
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

    def integrate(self, views, offset=None, drop=()):
        import torch
        from touch_gs_amd import Camera
        cams, depths, weights, rgbs = [], [], [], []
        for vw in views:
            m = np.eye(4)
            m[:3, :3], m[:3, 3] = vw["R"], vw["t"] if offset is None else vw["t"] - vw["R"] @ offset
            cams.append(Camera(m, vw["fx"], vw["fy"], vw["cx"], vw["cy"], vw["W"], vw["H"], near=vw["near"], pix_center=vw["pix_center"]))
            up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.dev)
            depths.append(up(vw["depth"]))
            weights.append(None if "weight" in drop else up(vw.get("weight")))
            rgbs.append(None if "rgb" in drop or self.vol.C is None else up(vw.get("rgb")))
        self.vol.integrate(cams, depths, weights, rgbs)
        torch.cuda.synchronize(self.dev)
        return self

    def state(self):
        return (self.vol.S.cpu().numpy(), self.vol.Wt.cpu().numpy(), None if self.vol.C is None else self.vol.C.cpu().numpy())

    def pads_intact(self):
        return _pads_intact(self.bufS, self.V, self.pad) and _pads_intact(self.bufW, self.V, self.pad) and \
            (self.bufC is None or _pads_intact(self.bufC, 3 * self.V, self.pad))

    def extract(self, w_min=T.W_MIN, pad=64, want_edge_id=True):
        """The two extraction calls on NaN-prefilled, sentinel-padded outputs -> host arrays + whether the padding survived."""
        import torch
        from touch_gs_amd import _lib
        lib = _lib.load()
        v, dev = self.vol, self.dev
        nx, ny, nz = v.dims
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        bufN, counts = _padded(self.V, dev, pad, -7, torch.int32)
        with torch.cuda.device(dev):
            _lib.check(lib.tgs_tsdf_extract_count(nx, ny, nz, C.c_float(v.voxel_size), _lib.ptr(v.S), _lib.ptr(v.Wt), C.c_float(w_min),
                                                  _lib.ptr(counts), stream))
            offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()
            total = int(counts.sum().item())
            nan = float("nan")
            bufP, points = _padded(3 * total, dev, pad, nan)
            bufNr, normals = _padded(3 * total, dev, pad, nan)
            bufCo, colors = _padded(3 * total, dev, pad, nan)
            bufE, eid = _padded(total, dev, pad, -1, torch.int64)
            if v.C is None:
                colors = None
            if total:
                _lib.check(lib.tgs_tsdf_extract_points(nx, ny, nz, C.c_float(v.voxel_size), _lib.ptr(v.S), _lib.ptr(v.Wt), _lib.ptr(v.C),
                                                       C.c_float(w_min), _lib.ptr(offsets), _lib.ptr(points), _lib.ptr(normals),
                                                       _lib.ptr(colors), _lib.ptr(eid) if want_edge_id else None, stream))
            torch.cuda.synchronize(dev)
        intact = _pads_intact(bufN, self.V, pad) and _pads_intact(bufP, 3 * total, pad) and _pads_intact(bufNr, 3 * total, pad) \
            and _pads_intact(bufCo, 3 * total, pad) and _pads_intact(bufE, total, pad) and self.pads_intact()
        return dict(counts=counts.cpu().numpy(), edge_id=eid.cpu().numpy(), points=points.cpu().numpy().reshape(total, 3),
                    normals=normals.cpu().numpy().reshape(total, 3),
                    colors=None if colors is None else colors.cpu().numpy().reshape(total, 3), intact=intact)


def _check_state(name, ref, S, Wt, Cc):
    fig = T.state_errors(ref, S, Wt, Cc)
    print(f"{name}: S {fig['S']:.3f} (bar {T.BARS['S']:.2f}) Wt {fig['Wt']:.3f} (bar {T.BARS['Wt']:.2f}) C {fig.get('C', 0):.3f} (bar "
          f"{T.BARS['C']:.2f}) units on {fig['clear']} clear voxels; {fig['unclear']} unclear ({fig['unclear_share']:.2%}), of which "
          f"{fig['unclear_differ']} differ")
    assert fig["nonfinite"] == 0 and fig["unclear_share"] <= T.CAP_UNCLEAR
    assert fig["S"] <= T.BARS["S"] and fig["Wt"] <= T.BARS["Wt"] and fig.get("C", 0) <= T.BARS["C"]
    return fig


def _check_crossings(name, ex, got):
    """The set rules and the bars on the common crossings."""
    total = len(got["edge_id"])
    assert got["counts"].min() >= 0 and got["counts"].max() <= 3 and got["counts"].sum() == total
    assert (np.diff(got["edge_id"]) > 0).all()                                       # rows in edge_id order
    offs = np.cumsum(got["counts"]) - got["counts"]
    assert np.array_equal(got["edge_id"] // 3, np.repeat(np.arange(len(offs)), got["counts"]))
    assert np.isfinite(got["points"]).all() and np.isfinite(got["normals"]).all()   # no prefilled NaN left in a row
    assert got["colors"] is None or np.isfinite(got["colors"]).all()
    cf = T.crossing_errors(ex, got)
    sc = dict(zip(ex["edge_id"].tolist(), ex["sign_clear"].tolist()))
    print(f"{name}: crossings {cf['got']} against {cf['ref']} of the reference ({cf['not_sign_clear_share']:.2%} not sign-clear), "
          f"{cf['common']} common, missing {cf['missing_clear']} clear + {cf['missing_unclear']} unclear, extra {len(cf['extra'])} (clear {cf['extra_clear']}); "
          f"t {cf.get('t', 0):.3f} (bar {T.BARS['t']:.2f}) point {cf.get('point', 0):.3f} ({T.BARS['point']:.2f}) normal "
          f"{cf.get('normal', 0):.3f} ({T.BARS['normal']:.2f}; {cf.get('normal_abs_deg', 0):.2e} deg) colour {cf.get('color', 0):.3f} "
          f"({T.BARS['color']:.2f}) units")
    assert cf["not_sign_clear_share"] <= T.CAP_UNCLEAR
    assert cf["missing_clear"] == 0                  # every reference crossing with both ends sign-clear is present
    assert cf["extra_clear"] == 0, "a GPU crossing that the reference does not have, with both ends sign-clear"
    assert all(not sc[e] for e in np.setdiff1d(ex["edge_id"], got["edge_id"]).tolist())
    for k in ("t", "point", "normal", "color"):
        assert cf.get(k, 0) <= T.BARS[k], k
    assert cf.get("normal_zero_mismatch", 0) == 0
    return cf


@pytest.mark.parametrize("name,pad", [(n, 64) for n in T.FIXTURES] + [("weights_rgb", 61), ("thin_x", 61), ("aligned", 62)])
def test_fixture_against_the_fp64_reference(name, pad, dev):
    """sphere: 37 x 29 x 23 (no multiple of 4 or 64 anywhere), three cameras; plane_behind: free-space carving, a depth
    discontinuity, the clamp d = 1; weights_rgb: weights in [0, 2] with zeros and a NaN, random colours; aligned: 64 x 8 x 4;
    thin_z 1 x 1 x 5 and thin_x 130 x 1 x 1: the row tail, single voxels; behind: nothing changes.  pad 61 / 62: the state
    arrays at addresses that are no multiple of 16 bytes."""
    grid, views = T.fixture(name)
    ref, ex = T.reference(name)
    vol = Volume(grid, dev, pad).integrate(views)
    S, Wt, Cc = vol.state()
    assert vol.pads_intact()
    _check_state(name, ref, S, Wt, Cc)
    if name == "behind":
        assert not S.any() and not Wt.any() and not Cc.any()
        used = Volume(grid, dev, pad).integrate(T.fixture("weights_rgb")[1])
        before = [a.tobytes() for a in used.state()]
        assert [a.tobytes() for a in used.integrate(views).state()] == before
    got = vol.extract()
    assert got["intact"]
    _check_crossings(name, ex, got)
    # the public path gives the same rows
    loc = vol.vol.extract_local(T.W_MIN)
    assert loc["edge_id"].cpu().numpy().tobytes() == got["edge_id"].tobytes()
    assert loc["points"].cpu().numpy().tobytes() == got["points"].tobytes()
    assert loc["normals"].cpu().numpy().tobytes() == got["normals"].tobytes()
    world = vol.vol.extract_points(T.W_MIN)
    assert world["points"].dtype == np.float64
    assert np.array_equal(world["points"], got["points"].astype(np.float64) + np.asarray(grid["origin"]))
    f = vol.vol.tsdf(T.W_MIN).cpu().numpy().reshape(-1)
    assert np.array_equal(np.isnan(f), ~(Wt >= T.W_MIN)) and np.array_equal(f[Wt >= T.W_MIN], (S / np.where(Wt > 0, Wt, 1))[Wt >= T.W_MIN])


def test_batching_is_invisible_in_the_bits(dev):
    """Eight views in one call, in eight calls and as 3 + 5; twice the same call."""
    grid, views = T.fixture("eight")
    whole = Volume(grid, dev).integrate(views)
    again = Volume(grid, dev).integrate(views)
    single = Volume(grid, dev)
    for vw in views:
        single.integrate([vw])
    split = Volume(grid, dev).integrate(views[:3]).integrate(views[3:])
    want = [a.tobytes() for a in whole.state()]
    for other in (again, single, split):
        assert [a.tobytes() for a in other.state()] == want and other.pads_intact()
    a, b = whole.extract(), again.extract()
    for k in ("counts", "edge_id", "points", "normals", "colors"):
        assert a[k].tobytes() == b[k].tobytes()
    assert whole.vol.views_integrated == 8 and split.vol.views_integrated == 8


def test_second_integrate_continues_the_reference(dev):
    grid, views = T.fixture("eight")
    ref, ex = T.reference("eight")
    vol = Volume(grid, dev, pad=61).integrate(views[:3])
    _check_state("eight[:3]", T.integrate(grid, views[:3]), *vol.state())
    vol.integrate(views[3:])
    _check_state("eight", ref, *vol.state())
    got = vol.extract()
    assert got["intact"]
    _check_crossings("eight", ex, got)


def test_missing_optional_inputs_leave_the_rest_bit_identical(dev):
    grid, views = T.fixture("eight")
    full = Volume(grid, dev).integrate(views)
    S, Wt, Cc = full.state()
    s2, w2, c2 = Volume(grid, dev, color=False).integrate(views).state()             # C = NULL
    assert c2 is None and s2.tobytes() == S.tobytes() and w2.tobytes() == Wt.tobytes()
    s3, w3, c3 = Volume(grid, dev).integrate(views, drop=("rgb",)).state()           # rgb = NULL: no colour, the rest alike
    assert s3.tobytes() == S.tobytes() and w3.tobytes() == Wt.tobytes() and not c3.any()
    # weight = NULL is the weight image of ones
    ones = [dict(vw, weight=np.ones((vw["H"], vw["W"]), np.float32)) for vw in views]
    a, b = Volume(grid, dev).integrate(ones).state(), Volume(grid, dev).integrate(views, drop=("weight",)).state()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # the extraction with colors = NULL and edge_id = NULL writes the same points and normals, and leaves the id rows alone
    nc = Volume(grid, dev, color=False).integrate(views).extract(want_edge_id=False)
    wc = full.extract()
    assert nc["colors"] is None and nc["points"].tobytes() == wc["points"].tobytes() and nc["normals"].tobytes() == wc["normals"].tobytes()
    assert nc["intact"] and (nc["edge_id"] == -1).all() and len(nc["edge_id"]) == len(wc["edge_id"])


def test_world_offset_gives_the_same_grid_local_bits(dev):
    """The grid and the cameras moved by (300, -200, 500) m: the same fp32 R and t' reach the device
    (tests/test_cpu_tsdf.py::test_world_offset_changes_no_rounded_view), so the same bits come back."""
    grid, views = T.fixture("eight")
    off = np.array([300.0, -200.0, 500.0])
    here = Volume(grid, dev).integrate(views)
    there = Volume(grid, dev, origin=np.asarray(grid["origin"]) + off).integrate(views, offset=off)
    assert [a.tobytes() for a in here.state()] == [a.tobytes() for a in there.state()]
    a, b = here.vol.extract_local(T.W_MIN), there.vol.extract_local(T.W_MIN)
    assert a["points"].cpu().numpy().tobytes() == b["points"].cpu().numpy().tobytes()
    pa, pb = here.vol.extract_points(T.W_MIN)["points"], there.vol.extract_points(T.W_MIN)["points"]
    assert np.abs((pb - off) - pa).max() < 1e-10


def test_save_load_round_trip(dev, tmp_path):
    from touch_gs_amd.tsdf import TsdfVolume
    grid, views = T.fixture("weights_rgb")
    vol = Volume(grid, dev).integrate(views).vol
    vol.save(str(tmp_path / "tsdf.npz"))
    back = TsdfVolume.load(str(tmp_path / "tsdf.npz"), dev)
    assert back.dims == vol.dims and back.voxel_size == vol.voxel_size and back.trunc == vol.trunc and np.array_equal(back.origin, vol.origin)
    for k in ("S", "Wt", "C"):
        assert getattr(back, k).cpu().numpy().tobytes() == getattr(vol, k).cpu().numpy().tobytes()
    assert back.views_integrated == 3


def test_default_device_spelling(dev, tmp_path):
    """A volume built, and one loaded, with device="cuda" (the constructor's default, no index) takes images that live on
    "cuda:0", continues, and gives the bits of a volume built on the indexed device."""
    import torch
    from touch_gs_amd.tsdf import TsdfVolume
    grid, views = T.fixture("eight")
    want = Volume(grid, dev).integrate(views).state()
    with torch.cuda.device(dev):
        plain = Volume(grid, "cuda")
        assert plain.vol.device == dev and plain.vol.S.device == dev
        plain.integrate(views[:3])
        plain.vol.save(str(tmp_path / "part.npz"))
        back = TsdfVolume.load(str(tmp_path / "part.npz"))                   # default device
        assert back.device == dev and back.views_integrated == 3
        cont = Volume(grid, "cuda")
        cont.vol = back
        cont.bufS = cont.bufW = cont.bufC = None
        cont.integrate(views[3:])
        plain.integrate(views[3:])
    for got in (plain.state(), (back.S.cpu().numpy(), back.Wt.cpu().numpy(), back.C.cpu().numpy())):
        assert [a.tobytes() for a in got] == [a.tobytes() for a in want]
    assert back.views_integrated == 8


def _sphere_model(dev, n=4000, seed=0):
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


def test_model_end_to_end(dev, monkeypatch):
    """About 4 k small opaque Gaussians on the sphere, six 96 x 72 views through fuse_model: the kernel path equals the fp64
    reference FED THE SAME RENDERED IMAGES within the bars, and the extracted points' median distance to the sphere is within
    one voxel plus the median error of those renders against the analytic depth (the surface cannot be better than the depth
    it is fused from)."""
    import torch
    from touch_gs_amd import Camera, tsdf
    model = _sphere_model(dev)
    img = dict(W=96, H=72, fx=110.0, fy=110.0, cx=47.6, cy=36.2)
    cams, poses = [], []
    for pos in T.CAM_POS + [(-0.5, -0.1, 0.2), (0.1, 0.5, -0.25), (-0.05, -0.2, -0.5)]:
        R, t = T.look_at(pos, target=T.SPHERE_C)
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = R, t
        cams.append(Camera(m, **img))
        poses.append((R, t))
    seen = []
    real = tsdf.TsdfVolume.integrate

    def spy(self, cams_, depths, weights=None, rgbs=None):
        seen.append((list(cams_), [d.clone() for d in depths], [None if w is None else w.clone() for w in weights],
                     [None if c is None else c.clone() for c in rgbs]))
        return real(self, cams_, depths, weights, rgbs)
    monkeypatch.setattr(tsdf.TsdfVolume, "integrate", spy)
    c = np.asarray(T.SPHERE_C)
    with torch.cuda.device(dev):
        vol = tsdf.fuse_model(model, cams, (c - 0.15, c + 0.15), resolution=24, trunc_voxels=3)
        torch.cuda.synchronize()
    assert vol.dims == (24, 24, 24) and len(seen) == 1 and len(seen[0][0]) == 6 and vol.views_integrated == 6
    grid = dict(dims=vol.dims, vox=vol.voxel_size, origin=vol.origin, trunc=vol.trunc)
    views, errs = [], []
    for (R, t), cam, d, w, rgb in zip(poses, *seen[0]):
        d = d.cpu().numpy()
        views.append(dict(R=R, t=t, **img, near=cam.near, pix_center=cam.pix_center, depth=d, weight=w.cpu().numpy(), rgb=rgb.cpu().numpy()))
        truth = T.sphere_depth(R, t, **img, centre=T.SPHERE_C, radius=T.SPHERE_R, pix_center=cam.pix_center)
        both = (d > 0) & (truth > 0)
        assert both.sum() > 500
        errs.append(np.abs(d - truth)[both])
    ref = T.integrate(grid, views)
    ex = T.extract(grid, ref["S"], ref["Wt"], ref["C"], T.W_MIN, U=ref["U"], UC=ref["UC"])
    _check_state("model", ref, vol.S.cpu().numpy(), vol.Wt.cpu().numpy(), vol.C.cpu().numpy())
    loc = vol.extract_local(T.W_MIN)
    got = {k: loc[k].cpu().numpy() for k in ("counts", "edge_id", "points", "normals", "colors")}
    _check_crossings("model", ex, got)
    cloud = vol.extract_points(T.W_MIN)
    dist = np.abs(np.linalg.norm(cloud["points"] - c, axis=1) - T.SPHERE_R)
    render_err = float(np.median(np.concatenate(errs)))
    print(f"model: {len(dist)} points, median distance to the sphere {np.median(dist):.5f} m; voxel {vol.voxel_size:.5f} m, median "
          f"error of the rendered depth {render_err:.5f} m")
    assert len(dist) > 300 and np.median(dist) <= vol.voxel_size + render_err
    out = (cloud["points"] - c) / np.linalg.norm(cloud["points"] - c, axis=1, keepdims=True)
    assert np.median((cloud["normals"] * out).sum(1)) > 0.9                          # outward


def test_command_line_writes_the_three_files(dev, tmp_path):
    """A two-view 160 x 90 capture of write_raw_capture and a ten-step run whose checkpoint then gets opaque Gaussians on the
    touch cloud; the two exports: the three files (and point_cloud.ply) load, the grid is the padded box of the touch cloud and
    the points lie next to the touched points IN THE CAPTURE'S FRAME (metres, not the centred and scaled frame of the model)."""
    import torch
    read_ply = T.read_ply
    from touch_gs_amd import export, train
    from touch_gs_amd.analytic_scene import prepare_capture, write_raw_capture
    root = str(tmp_path / "capture")
    write_raw_capture(root, n_views=2, n_touches=4, W=160, H=90, seed=3, gpis_max_points=150, device="cpu")
    prepare_capture(root, 0.5)
    with torch.cuda.device(dev):
        run = train.main(["--data", root, "--train-split-fraction", "0.5", "--max-num-iterations", "10", "--steps-per-eval", "10",
                          "--steps-per-save", "10", "--sh-degree", "1", "--num-gaussians", "2000", "--output-dir", str(tmp_path / "out")])
        # ten steps leave the model translucent (alpha < 0.5 everywhere: an empty surface).  Put its Gaussians, opaque, on
        # the touch cloud -- in the model's centred and scaled frame -- so that the export has a surface to find
        from touch_gs_amd.dataset import Scene
        from touch_gs_amd.optim import GaussianParams
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
        out = str(tmp_path / "export")
        info = export.main(["tsdf", "--run", run, "--output-dir", out, "--resolution", "24", "--views", "all", "--depth", "expected",
                            "--weight", "uniform"])
        ginfo = export.main(["gaussians", "--run", run, "--output-dir", out])
    assert sorted(os.listdir(out)) == ["export.json", "point_cloud.ply", "surface.ply", "tsdf.npz"]
    on_disk = json.load(open(os.path.join(out, "export.json")))
    assert on_disk["counts"] == info["counts"] and on_disk["grid"]["bounds"] == "touch" and info["counts"]["views"] == 2
    assert set(on_disk["seconds"]) >= {"load", "render_and_fuse", "extract", "write"}
    assert {"chamfer", "precision", "recall", "fscore"} <= set(on_disk["surface_metrics"])      # the capture has gt_depth/
    assert abs(on_disk["surface_metrics"]["tau"] - 2 * on_disk["grid"]["voxel_size_m"]) < 1e-12
    names, rec = read_ply(os.path.join(out, "surface.ply"))
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and len(rec) == info["counts"]["points"]
    lo, hi = touch.min(0), touch.max(0)
    pad = 0.2 * (hi - lo)
    g = on_disk["grid"]
    assert np.allclose(g["origin_m"], lo - pad, atol=1e-9) and max(g["dims"]) == 24
    assert abs(g["voxel_size_m"] - (1.4 * (hi - lo)).max() / 24) < 1e-9
    # the points are in the CAPTURE's frame: inside the padded box of the touch cloud and next to the touched points
    # (the scaled frame's origin is the mean camera position, 0.3 m from the object)
    assert len(rec) > 50 and info["counts"]["observed_voxels"] > 0
    p = np.stack([rec["x"], rec["y"], rec["z"]], -1).astype(np.float64)
    top = np.asarray(g["origin_m"]) + np.asarray(g["dims"]) * g["voxel_size_m"]
    assert (p >= np.asarray(g["origin_m"]) - 1e-6).all() and (p <= top + 1e-6).all()
    near = np.sqrt(((p[:, None] - touch[None]) ** 2).sum(2).min(1))
    print(f"cli: {len(p)} points, median distance to the touch cloud {np.median(near):.4f} m, voxel {g['voxel_size_m']:.4f} m; "
          f"surface metrics {on_disk['surface_metrics']}")
    assert np.median(near) < 3 * g["voxel_size_m"]
    n = np.stack([rec["nx"], rec["ny"], rec["nz"]], -1)
    ln = np.linalg.norm(n, axis=1)
    assert (np.abs(ln[ln > 0] - 1) < 1e-5).all()
    from touch_gs_amd.tsdf import TsdfVolume
    back = TsdfVolume.load(os.path.join(out, "tsdf.npz"), dev)
    assert list(back.dims) == g["dims"] and back.views_integrated == 2
    names, rec = read_ply(os.path.join(out, "point_cloud.ply"))
    assert len(rec) == ginfo["gaussians"] and names[:6] == ["x", "y", "z", "nx", "ny", "nz"] and names[-4:] == ["rot_0", "rot_1", "rot_2", "rot_3"]
    assert len([k for k in names if k.startswith("f_rest_")]) == 3 * (ginfo["sh_coefficients"] - 1)
    # the Gaussians too: positions back in metres, log scales shifted by -log(scale), opacities as stored
    assert scene.scale > 1.5
    got = np.stack([rec["x"], rec["y"], rec["z"]], -1).astype(np.float64)
    assert np.abs(got - on).max() < 1e-5
    scales = np.stack([rec[f"scale_{i}"] for i in range(3)], -1)
    assert np.abs(scales - np.log(0.003)).max() < 1e-5
    assert np.array_equal(rec["opacity"], par["opac_logit"].numpy())
