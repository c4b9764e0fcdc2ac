"""GPU tests of the depth-statistics pass (k_raster_depth_stats / tgs_rasterize_depth_stats / ops.rasterize_depth_stats):
median depth and per-pixel depth variance against the fp64 reference of tests/depth_stats_ref.py, evaluated on the fp32
records and the lists the GPU made (the convention of tests/test_gpu_parity.py), and the Python surface above it.

Bars (set by the feature's specification, not tuned):
  * decision-clear pixels: the oracle's margin >= 1e-4 AND min |T' - 1/2| / (1/2) >= 1e-4 over the included entries; at
    most 1 % of the pixels of every scene may be unclear (a condition on the scene, asserted);
  * median: on clear pixels the Gaussian id equals the reference's exactly and id == -1 <=> alpha < 1/2; on EVERY pixel
    the depth is bit-equal to record slot 2 of the id (0 where -1) and the id is a member of the pixel's tile list;
  * variance: on clear pixels |var - ref| <= 1e-4 max(ref, (1e-3 Dhat)^2) -- d - Dhat is rounded at ~6e-8 d, so a
    spread below 0.1 % of the depth cannot be held to four digits in fp32 --, on every pixel var >= 0.

Observed on an MI355X (each test prints its own line: run with -s): unclear share 0.09 - 0.34 % on the seven frames;
variance error over max(ref, (1e-3 Dhat)^2): max 5.3e-5 (object-centric frame, lists up to 1393 entries), q99 <= 3.1e-6,
against the bound 1e-4; median ids exact on every clear pixel.
"""
import types

import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests.depth_stats_ref import clear_pixels, depth_stats_ref
from tests.util import amd_cam, clamp_scene, count_clamped, splat_fields, to_dev

pytestmark = pytest.mark.gpu

VAR_TOL = 1e-4
VAR_FLOOR = 1e-3          # of the expected depth (standard deviation)
CLEAR_TOL = 1e-4
MAX_UNCLEAR = 0.01


def _front(dev, D, acam, deg):
    from touch_gs_amd import ops
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(acam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], deg)
    return sp, gb, ts, sg


def _check_against_reference(label, ocam, sp, ts, sg, depth_acc, var, med, gid):
    """The bars of the module docstring for one frame; prints the observed errors next to the bound."""
    n = int(ts[-1])
    f = splat_fields(sp)
    sgn, tsn = sg[:n].cpu().numpy().astype(np.int64), ts.cpu().numpy().astype(np.int64)
    ref = depth_stats_ref(f["xy"], f["conic"], f["opac"], f["depth"], sgn, tsn, ocam)
    out = O.blend(f["xy"], f["conic"], f["opac"], f["rgb"], f["depth"], sgn, tsn, ocam, want_margin=True)
    clear = clear_pixels(out, ref, CLEAR_TOL)
    unclear = 1.0 - clear.mean()
    var, med, gid = var.cpu().numpy(), med.cpu().numpy(), gid.cpu().numpy().astype(np.int64)
    rec_depth = sp[:, 2].cpu().numpy()
    # variance
    bound = VAR_TOL * np.maximum(ref["var"], (VAR_FLOOR * ref["dhat"]) ** 2)
    err = np.abs(var.astype(np.float64) - ref["var"])
    rel = (err / np.maximum(bound / VAR_TOL, 1e-300))[clear]
    covered = clear & (ref["alpha"] > 0)
    print(f"[depth_stats {label}] pixels {clear.size}  unclear {unclear:.4%} (cap {MAX_UNCLEAR:.0%})  "
          f"variance rel err max {rel.max():.3e} q99 {np.quantile(rel, 0.99):.3e} (bound {VAR_TOL:.0e})  "
          f"with a median {np.mean(gid >= 0):.3f}  covered {covered.mean():.3f}  longest list {int(np.diff(tsn).max())}")
    assert unclear <= MAX_UNCLEAR, unclear
    assert covered.mean() > 0.3                      # (the scene is not mostly background)
    assert (var >= 0).all()
    assert (err[clear] <= bound[clear]).all(), (rel.max(), int((err > bound)[clear].sum()))
    assert (var[ref["alpha"] == 0] == 0).all()
    # median: exact id on clear pixels, and there is one exactly where the transmittance reaches 1/2
    assert np.array_equal(gid[clear], ref["median_gid"][clear]), int((gid != ref["median_gid"])[clear].sum())
    assert np.array_equal((gid == -1)[clear], (ref["alpha"] < 0.5)[clear])
    assert (gid >= 0).mean() > 0.1
    # every pixel: depth bit-equal to the record's slot 2, 0 without a median; id is a member of the pixel's tile list
    has = gid >= 0
    assert gid.min() >= -1 and gid.max() < sp.shape[0]
    assert np.array_equal(med[has].view(np.uint32), rec_depth[gid[has]].view(np.uint32))
    assert (med[~has].view(np.uint32) == 0).all()
    TW = ocam.tiles[0]
    H, W = gid.shape
    tile_of = (np.arange(H)[:, None] // 16) * TW + np.arange(W)[None, :] // 16
    for t in np.unique(tile_of[has]):
        members = sgn[tsn[t]:tsn[t + 1]]
        assert np.isin(gid[(tile_of == t) & has], members).all(), t
    return ref, clear


SCENES = [  # N, W, H, seed, orbit view (0 = identity); the four scenes whose unclear share was checked beforehand + two orbit views
    (2000, 128, 96, 1, 0), (2000, 128, 96, 2, 0), (20000, 320, 240, 3, 0), (640, 157, 93, 4, 0),
    (2000, 128, 96, 1, 3), (640, 157, 93, 4, 1)]


@pytest.mark.parametrize("N,W,H,seed,view", SCENES)
def test_depth_stats_match_the_fp64_reference(dev, N, W, H, seed, view):
    from touch_gs_amd import ops
    deg = 1
    P, c = O.synthetic_scene(N, W, H, deg, seed)
    ocam = O.Camera(viewmat=O.orbit_viewmat(view, 8), **c, bg=(0.1, 0.2, 0.3))
    acam = amd_cam(ocam)
    D = to_dev(P, dev)
    sp, gb, ts, sg = _front(dev, D, acam, deg)
    rgb, depth, fT, _ = ops.rasterize_fwd(acam, sp, sg, ts)
    var, med, gid = ops.rasterize_depth_stats(acam, sp, sg, ts, depth, fT, want_gid=True)
    assert var.shape == med.shape == gid.shape == (H, W) and gid.dtype == torch.int32
    _check_against_reference(f"iid N={N} {W}x{H} seed {seed} view {view}", ocam, sp, ts, sg, depth, var, med, gid)
    # without the ids: same images
    var2, med2, none = ops.rasterize_depth_stats(acam, sp, sg, ts, depth, fT)
    assert none is None and torch.equal(var, var2) and torch.equal(med, med2)


def _clustered(dev, N, W, H, seed, view=1):
    from touch_gs_amd.scene import make_camera, synthetic_gaussians
    P, intr = synthetic_gaussians(N, W, H, 1, seed, clustered=True)
    cam = make_camera(intr, view, 8, bg=(0.1, 0.2, 0.3))
    D = {k: v.to(dev).float().contiguous() for k, v in P.items()}
    ocam = O.Camera(viewmat=torch.from_numpy(np.asarray(cam.viewmat, np.float64).reshape(4, 4)), fx=cam.fx, fy=cam.fy,
                    cx=cam.cx, cy=cam.cy, W=W, H=H, bg=(0.1, 0.2, 0.3))
    return D, cam, ocam


def test_long_lists_of_an_object_centric_frame(dev):
    """Lists above 1024 entries (80 % of the Gaussians inside the central 10 % of a 320x180 image): the default rule walks
    the dense tiles with four quadrant blocks, the rest in 4x4-block form -- same bars."""
    from touch_gs_amd import ops
    D, cam, ocam = _clustered(dev, 20_000, 320, 180, 5)
    sp, gb, ts, sg = _front(dev, D, cam, 1)
    T = cam.num_tiles
    n = (ts[1:T + 1] - ts[:T]).long()
    I = int(n.sum())
    assert int(n.max()) > 1024, int(n.max())
    assert int((n > max(256, (2 * I) >> 12)).sum()) > 0          # the default rule (factor 2, floor 256) splits tiles
    rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts)
    var, med, gid = ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT, want_gid=True)
    _check_against_reference("object-centric N=20000 320x180", ocam, sp, ts, sg, depth, var, med, gid)


def test_outputs_do_not_depend_on_stop_pos_schedule_or_kernel_form(dev):
    """Bit-identical outputs with the forward's stop positions and without; with the tile_order schedule and in spatial
    order; with long tiles split into quadrant blocks (every rule) and unsplit; from a quadrant-form forward
    (k6_blocks=0) and the default one; and from one call to the next."""
    from touch_gs_amd import ops
    for N, W, H in ((30_000, 250, 170), (20_000, 320, 208)):
        D, cam, _ = _clustered(dev, N, W, H, 5)
        sp, gb, ts, sg = _front(dev, D, cam, 1)
        rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts)
        assert fT.stop_pos is not None
        base = ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT, want_gid=True)

        def same(got, why):
            for name, a, b in zip(("depth_var", "median_depth", "median_gid"), base, got):
                assert torch.equal(a, b), (why, name)

        same(ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT, want_gid=True), "run to run")
        fT_plain = fT.clone()                                     # (a copy does not carry .stop_pos)
        assert getattr(fT_plain, "stop_pos", None) is None
        same(ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT_plain, want_gid=True), "stop_pos=None")
        ts_plain = ts[:]                                          # the same buffer without the schedule riding on it
        assert getattr(ts_plain, "tile_order", None) is None and ts.tile_order is not None
        same(ops.rasterize_depth_stats(cam, sp, sg, ts_plain, depth, fT, want_gid=True), "spatial order")
        same(ops.rasterize_depth_stats(cam, sp, sg, ts_plain, depth, fT_plain, want_gid=True), "spatial order, stop_pos=None")
        for rule in (dict(k6_split=0), dict(k6_split=1, k6_split_floor=64, k6_split_heads=4096),
                     dict(k6_split=1, k6_split_floor=128, k6_split_heads=2048)):
            for f in (fT, fT_plain):
                same(ops.rasterize_depth_stats(cam, sp, sg, ts, depth, f, want_gid=True, opts=ops.raster_opts(**rule)), str(rule))
        rgb_q, depth_q, fT_q, _ = ops.rasterize_fwd(cam, sp, sg, ts, opts=ops.raster_opts(k6_blocks=0))
        assert torch.equal(depth_q, depth) and torch.equal(fT_q, fT) and torch.equal(fT_q.stop_pos, fT.stop_pos)
        same(ops.rasterize_depth_stats(cam, sp, sg, ts, depth_q, fT_q, want_gid=True, opts=ops.raster_opts(k6_blocks=0)),
             "quadrant-form forward")


def test_clamped_entries_walk_the_same_in_every_form(dev):
    """Batches with an opacity above 0.99 take the walk's copy WITH the 0.999 clamp (MAYCLAMP = true), which no other
    scene of this module reaches.  On the ragged clamp scene of test_k6_block_form_is_bit_identical the three images are
    bit-identical unsplit and with every tile of the schedule's head in quadrant blocks, with the forward's stop positions
    and without, and from a quadrant-form forward's images; a pixel has a median exactly where it ends with T <= 1/2."""
    from touch_gs_amd import ops
    N, W, H, deg = 3000, 100, 70, 1
    P, ocam = clamp_scene(N, W, H, deg, 79)
    acam = amd_cam(ocam)
    sp, gb, ts, sg = _front(dev, to_dev(P, dev), acam, deg)
    T = acam.num_tiles
    n = int(ts[T])
    assert count_clamped(splat_fields(sp), sg[:n].cpu().numpy(), ts.cpu().numpy(), ocam) > 0
    assert int((ts[1:T + 1] - ts[:T]).max()) > 64                 # (tiles that the floor-64 rule below really splits)
    assert ts.tile_order is not None                              # (no split without the schedule)
    unsplit = ops.raster_opts(k6_split=0)
    split = ops.raster_opts(k6_split=1, k6_split_floor=64, k6_split_heads=4096)
    rgb, depth, fT, _ = ops.rasterize_fwd(acam, sp, sg, ts, opts=unsplit)
    assert fT.stop_pos is not None
    fT_plain = fT.clone()                                         # (a copy does not carry .stop_pos)
    assert getattr(fT_plain, "stop_pos", None) is None
    base = ops.rasterize_depth_stats(acam, sp, sg, ts, depth, fT, want_gid=True, opts=unsplit)

    def same(got, why):
        for name, a, b in zip(("depth_var", "median_depth", "median_gid"), base, got):
            assert torch.equal(a, b), (why, name)

    for name, opts in (("unsplit", unsplit), ("split", split)):
        for f in (fT, fT_plain):
            same(ops.rasterize_depth_stats(acam, sp, sg, ts, depth, f, want_gid=True, opts=opts),
                 (name, "stop_pos" if f is fT else "stop_pos=None"))
    rgb_q, depth_q, fT_q, _ = ops.rasterize_fwd(acam, sp, sg, ts, opts=ops.raster_opts(k6_blocks=0))
    assert torch.equal(depth_q, depth) and torch.equal(fT_q, fT) and torch.equal(fT_q.stop_pos, fT.stop_pos)
    for name, opts in (("unsplit", unsplit), ("split", split)):
        same(ops.rasterize_depth_stats(acam, sp, sg, ts, depth_q, fT_q, want_gid=True, opts=opts), ("quadrant-form forward", name))
    var, med, gid = base
    assert torch.equal(gid >= 0, fT <= 0.5)
    assert bool((gid >= 0).any())
    assert bool((var >= 0).all())


def test_pass_leaves_the_scratch_behind_tile_start_and_the_backward_alone(dev):
    """The words behind the tile starts (walk statistics of the forward, slot counters of the backward) read the same
    before and after the pass, and a backward gives bit-identical partials with and without the pass in between: on
    the same lists (record for record), and on two separately binned frames of which only one ran the pass (there the
    pair ranges of the binning groups are laid out in arbitrary order, so the per-Gaussian sums are compared)."""
    from touch_gs_amd import ops
    D, cam, _ = _clustered(dev, 30_000, 250, 170, 5)
    T = cam.num_tiles
    g = torch.Generator().manual_seed(1)
    v_rgb = torch.rand(cam.H, cam.W, 3, generator=g).to(dev)
    v_depth = torch.rand(cam.H, cam.W, generator=g).to(dev)

    def backward(sp, gb, ts, sg, rgb, depth, fT):
        pt = torch.zeros(sg.shape[0], 12, device=dev)
        p, _ = ops.rasterize_bwd(cam, sp, gb, sg, ts, rgb, depth, fT, v_rgb=v_rgb, v_depth=v_depth, partials=pt)
        return p.clone(), ops.reduce_partials(cam, sp, gb, p).clone()

    reduced = []
    for with_pass in (False, True):
        sp, gb, ts, sg = _front(dev, D, cam, 1)
        rgb, depth, fT, _ = ops.rasterize_fwd(cam, sp, sg, ts)
        if with_pass:
            p_before, _ = backward(sp, gb, ts, sg, rgb, depth, fT)
            words = lambda: torch.as_strided(ts, (512,), (1,), ts.storage_offset() + T + 1).clone()
            before = words()
            assert int(before.abs().sum()) > 0                     # the forward did leave its walk statistics there
            ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT, want_gid=True)
            ops.rasterize_depth_stats(cam, sp, sg, ts, depth, fT.clone())
            assert torch.equal(words(), before)
        p, r = backward(sp, gb, ts, sg, rgb, depth, fT)
        if with_pass:
            assert torch.equal(p, p_before)                        # same lists: record for record
        reduced.append(r)
    assert torch.equal(reduced[0], reduced[1])
    assert float(reduced[0].abs().sum()) > 0


def _model_and_view(dev, N=3000, W=160, H=96, deg=2):
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_view, synthetic_gaussians
    view = make_view(N, W, H, deg, 5, dev)
    P, _ = synthetic_gaussians(N, W, H, deg, 99)
    params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
    model = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, depth_loss_mult=0.2), params)
    g = torch.Generator().manual_seed(2)
    view.gt_depth = (view.depth + 0.01 * torch.randn(H, W, generator=g).to(dev)) * (torch.rand(H, W, generator=g).to(dev) > 0.2)
    view.object_mask = torch.rand(H, W, generator=g).to(dev) > 0.5
    return model, view


TODAYS_KEYS = {"rgb", "depth", "accumulation", "depth_acc", "alpha", "radii"}
NEW_KEYS = {"median_depth", "depth_var", "depth_std", "median_gid"}
NEW_METRICS = {"median_depth_mse", "gt_depth_mse_median", "gt_object_depth_mse_median"}


def test_model_outputs_and_metrics(dev):
    model, view = _model_and_view(dev)
    H, W = view.cam.H, view.cam.W
    with torch.no_grad():
        out0 = model.get_outputs(view.cam)
        out1 = model.get_outputs(view.cam, depth_stats=True)
    assert set(out0) == TODAYS_KEYS
    assert set(out1) == TODAYS_KEYS | NEW_KEYS
    for k in TODAYS_KEYS:
        assert torch.equal(out0[k], out1[k]), k
    assert out1["median_depth"].shape == out1["depth_var"].shape == out1["depth_std"].shape == (H, W, 1)
    assert out1["median_gid"].shape == (H, W) and out1["median_gid"].dtype == torch.int32
    assert torch.equal(out1["depth_std"], torch.sqrt(out1["depth_var"]))
    assert not any(out1[k].requires_grad for k in NEW_KEYS)
    # with gradients enabled the first outputs differentiate as before (bit-identical gradients) and the statistics stay detached
    from touch_gs_amd.model import DepthGaussianSplattingModel
    from touch_gs_amd.optim import GaussianParams
    grads = []
    for stats in (False, True):
        leaves = [getattr(model.params, k).detach().clone().requires_grad_(True) for k in GaussianParams.NAMES]
        p2 = GaussianParams.from_tensors(*[t.detach() for t in leaves])
        for k, t in zip(GaussianParams.NAMES, leaves):
            setattr(p2, k, t)
        m2 = DepthGaussianSplattingModel(model.config, p2)
        out2 = m2.get_outputs(view.cam, depth_stats=True) if stats else m2.get_outputs(view.cam)
        assert out2["rgb"].requires_grad
        if stats:
            assert not any(out2[k].requires_grad for k in NEW_KEYS)
            for k in TODAYS_KEYS | NEW_KEYS:
                assert torch.equal(out2[k].detach(), out1[k]), k
        sum(m2.get_loss_dict(out2, view).values()).backward()
        grads.append([t.grad.clone() for t in leaves])
    for a, b in zip(*grads):
        assert torch.equal(a, b) and float(a.abs().sum()) > 0
    m0, im0 = model.get_image_metrics_and_images(out0, view)
    m1, im1 = model.get_image_metrics_and_images(out1, view)
    assert set(m1) - set(m0) == NEW_METRICS and set(m0) <= set(m1)
    assert all(m1[k] == m0[k] for k in m0)                        # keys that exist today keep their values
    assert set(im1) - set(im0) == {"median_depth", "depth_std"}
    # the definition: the median where there is one, else the expected depth, under the masks of the expected-depth keys
    dm = torch.where(out1["median_gid"] >= 0, out1["median_depth"][..., 0], out1["depth"][..., 0])
    valid = view.gt_depth > 0
    assert m1["median_depth_mse"] == pytest.approx(float(((dm - view.depth)[view.depth > 0] ** 2).mean()), rel=1e-6)
    assert m1["gt_depth_mse_median"] == pytest.approx(float(((dm - view.gt_depth)[valid] ** 2).mean()), rel=1e-6)
    obj = valid & view.object_mask
    assert m1["gt_object_depth_mse_median"] == pytest.approx(float(((dm - view.gt_depth)[obj] ** 2).mean()), rel=1e-6)
    # ops.render: the default call is the 4-tuple, the keyword appends the three tensors
    from touch_gs_amd import ops
    p = model.params
    with torch.no_grad():
        r4 = ops.render(p.means, p.log_scales, p.quats, p.opac_logit, p.sh, view.cam, 2)
        r7 = ops.render(p.means, p.log_scales, p.quats, p.opac_logit, p.sh, view.cam, 2, depth_stats=True)
    assert len(r4) == 4 and len(r7) == 7
    assert all(torch.equal(a, b) for a, b in zip(r4, r7[:4]))
    assert torch.equal(r7[4], out1["depth_var"][..., 0]) and torch.equal(r7[6], out1["median_gid"])


def test_plugin_field_defaults_to_off(dev):
    from touch_gs_amd.nerfstudio_plugin import AutogradGaussians
    from touch_gs_amd.scene import make_view, synthetic_gaussians
    N, W, H, deg = 2000, 128, 80, 1
    view = make_view(N, W, H, deg, 5, dev)
    P, _ = synthetic_gaussians(N, W, H, deg, 99)
    base = dict(sh_degree=deg, ssim_lambda=0.2, depth_loss_mult=0.2, depth_loss_type="DEPTH_UNCERTAINTY_WEIGHTED_LOSS",
                uncertainty_weight=1.0)
    outs = []
    for extra in ({}, dict(output_depth_stats=False), dict(output_depth_stats=True)):
        ag = AutogradGaussians(types.SimpleNamespace(**base, **extra), P["means"], torch.full((N, 3), 0.5), device=dev)
        assert ag.output_depth_stats is bool(extra.get("output_depth_stats", False))
        ag.training = False
        outs.append(ag.render(view.cam))
    assert set(outs[0]) == set(outs[1]) == TODAYS_KEYS
    assert set(outs[2]) == TODAYS_KEYS | NEW_KEYS
    assert torch.equal(outs[0]["rgb"], outs[2]["rgb"]) and torch.equal(outs[0]["depth"], outs[2]["depth"])
    batch = {"image": view.rgb, "depth_image": view.depth[..., None], "uncertainty": view.uncertainty[..., None]}
    m_off, _ = ag.image_metrics_and_images(outs[0], batch)
    m_on, _ = ag.image_metrics_and_images(outs[2], batch)
    assert set(m_on) - set(m_off) == {"median_depth_mse"}            # (no sensor ground truth in a nerfstudio batch)


def test_eval_tools_write_the_metrics_and_the_uncertainty_map(dev, tmp_path):
    """train.evaluate gains the three metrics (the others keep their values); train.render_views writes
    uncertainty/<name>.png in the format of the input maps: read back with the dataset's reader it is within one quantum
    (1e-3 m^2) of the variance in m^2 clipped to [0, 10]."""
    from touch_gs_amd.plumbing import from_uint16_mm, read_png16
    from touch_gs_amd.train import evaluate, render_views
    model, view = _model_and_view(dev)
    r0 = evaluate(model, [view])
    r1 = evaluate(model, [view], depth_stats=True)
    assert set(r1) - set(r0) == NEW_METRICS and all(r1[k] == r0[k] for k in r0)
    scale = 0.5
    plain = tmp_path / "plain"
    render_views(model, [view], str(plain))
    assert sorted(p.name for p in plain.iterdir()) == ["depth", "rgb"]
    full = tmp_path / "full"
    render_views(model, [view], str(full), depth_stats=True, dataparser_scale=scale)
    assert sorted(p.name for p in full.iterdir()) == ["depth", "median_depth", "rgb", "uncertainty"]
    assert np.array_equal(read_png16(str(full / "depth" / "00000.png")), read_png16(str(plain / "depth" / "00000.png")))
    with torch.no_grad():
        out = model.get_outputs(view.cam, sh_degree=model.active_sh_degree(), depth_stats=True)
    want = np.clip(out["depth_var"][..., 0].double().cpu().numpy() / scale ** 2, 0.0, 10.0)
    got = from_uint16_mm(read_png16(str(full / "uncertainty" / "00000.png")))
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-3 + 1e-9
    assert (got > 0).mean() > 0.1                                     # (the map is not empty)
    med = read_png16(str(full / "median_depth" / "00000.png")).astype(np.float64) / 1000.0
    assert np.abs(med - out["median_depth"][..., 0].double().cpu().numpy().clip(0, 65.535)).max() <= 0.5e-3 + 1e-6
