"""GPU tests of the depth-derived normals and the normal-prior loss (csrc/depthnormal.hip / tgs_depth_normal_fwd_bwd /
ops.depth_normal_fwd_bwd / ops.depth_normals / ops.depth_normal_loss) against the fp64 reference of tests/depth_normal_ref.py,
which reads the same fp32 images and makes the same fp32 decisions (validity, jump gate), and of the model paths above it.

Bars (set by the feature's specification, not tuned):
  * formed and supervised counts exact; C and the loss within 1e-6 relative;
  * |n - n_ref|_inf <= 16 kappa_i 2^-24 on EVERY formed centre, exact zeros elsewhere;
  * |v_depth - ref| <= 16 * 2^-24 S_j / alpha_j and |v_alpha - ref| <= 16 * 2^-24 S_j x_j / alpha_j on every pixel with S_j > 0,
    exact +-0 on every pixel with S_j = 0; kappa, S: the condition numbers of tests/depth_normal_ref.py;
  * two calls give identical bits; unaligned views give the bits of aligned images; accumulate = old + value, bit for bit;
  * fused step against autograd: every parameter gradient group within 1e-4 of the group's largest magnitude, the two loss
    values within 1e-6; with the term off nothing changes, bit for bit.
16 units is about 35 x what a CPU emulation of the kernels' fp32 arithmetic shows (0.46 and 0.37 units over the seven cases,
tests/test_cpu_depth_normal.py, which holds the emulation under 2 units).

Each test prints its observed maxima next to the bound (run with -s).  Observed on an MI355X: normals <= 0.46 kappa-units,
v_depth / v_alpha <= 0.37 S-units over the seven synthetic cases, the switches and the rendered frames (the emulation's own
figures), C within 5e-8 relative; fused against autograd <= 7e-9 on gradients of 7e-3 (1e-6 of a group's largest), loss values
equal to eight digits; the 60-step run takes the mean of 1 - cos from 0.81 to 0.05 with the term.
"""
import numpy as np
import pytest
import torch

from tests.depth_normal_ref import CASES, UNIT, assert_margins, decisions, depth_normal_ref, max_errors, synthetic
from tests.util import amd_cam, scene, to_dev

pytestmark = pytest.mark.gpu

UNITS = 16.0
WEIGHT = 0.7
_CACHE = {}


def _acam(cam):
    from touch_gs_amd.camera import Camera
    return Camera(np.eye(4), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["W"], cam["H"], pix_center=cam["pix_center"])


def _inputs(W, H, fx, with_conf=True, max_jump=0.1):
    """Synthetic images + their fp64 reference, computed once per case and never modified."""
    key = (W, H, fx, with_conf, max_jump)
    if key not in _CACHE:
        s = synthetic(W, H, 1, fx)
        assert_margins(s["out_depth"], s["final_T"], 0.5, max_jump)
        conf = s["conf"] if with_conf else None
        _CACHE[key] = (s, depth_normal_ref(s["cam"], s["out_depth"], s["final_T"], s["prior"], conf, 0.5, max_jump, WEIGHT))
    return _CACHE[key]


def _zero_bits(a):
    return (a.view(np.uint32) << 1 == 0).all()


def _check(label, stats, normals, vd, va, ref):
    st = stats.double().cpu().numpy()
    n, vd, va = normals.cpu().numpy(), vd.cpu().numpy(), va.cpu().numpy()
    e = max_errors(n, vd, va, ref)
    r = ref["stats"]
    print(f"[depth_normal {label}] formed {int(st[0])} supervised {int(st[1])}  C rel {abs(st[2] - r[2]) / max(r[2], 1e-300):.1e}  "
          f"loss {st[4]:.7f} (ref {r[4]:.7f})  normals {e.get('normals', 0):.2f} kappa-units  v_depth {e.get('v_depth', 0):.2f}  "
          f"v_alpha {e.get('v_alpha', 0):.2f} S-units  (bound {UNITS:.0f})")
    assert np.isfinite(st).all() and np.isfinite(n).all() and np.isfinite(vd).all() and np.isfinite(va).all()
    assert st[0] == r[0] and st[1] == r[1]
    assert abs(st[2] - r[2]) <= 1e-6 * abs(r[2]) and abs(st[3] - r[3]) <= 1e-6 * abs(r[3]) and abs(st[4] - r[4]) <= 1e-6 * abs(r[4])
    assert not st[5:].any()
    assert e["normals"] <= UNITS                      # every formed centre
    assert _zero_bits(n[~ref["formed"]])              # and exactly 0 elsewhere
    assert e["v_depth"] <= UNITS and e["v_alpha"] <= UNITS      # every pixel that feeds a supervised centre, none left out
    dead = ref["S"] == 0
    assert _zero_bits(vd[dead]) and _zero_bits(va[dead])
    assert np.abs(vd[~dead]).max() > 0
    return e


def _run(ops, dev, s, conf="own", weight_override=None, **kw):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    c = s["conf"] if isinstance(conf, str) else conf
    return ops.depth_normal_fwd_bwd(_acam(s["cam"]), t(s["out_depth"]), t(s["final_T"]), t(s["prior"]), t(c), alpha_min=0.5,
                                    weight=WEIGHT if weight_override is None else weight_override, want_normals=True, **kw)


@pytest.mark.parametrize("W,H,fx", CASES)
def test_synthetic_images_match_the_fp64_reference(dev, W, H, fx):
    from touch_gs_amd import ops
    s, ref = _inputs(W, H, fx)
    stats, normals, vd, va = _run(ops, dev, s, max_jump=0.1)
    assert stats.shape == (8,) and normals.shape == (H, W, 3) and vd.shape == va.shape == (H, W)
    assert ref["stats"][1] > 0.3 * W * H
    _check(f"{W}x{H} fx {fx}", stats, normals, vd, va, ref)


@pytest.mark.parametrize("W,H,fx", [(33, 18, 40.0), (157, 93, 140.0)])
def test_non_default_switches(dev, W, H, fx):
    """conf = None (weights 1), and max_jump = 0: the gate is off and the edge of the lowered box contributes."""
    from touch_gs_amd import ops
    s, ref = _inputs(W, H, fx, with_conf=False)
    _check(f"{W}x{H} conf None", *_run(ops, dev, s, conf=None, max_jump=0.1), ref)
    s, ref0 = _inputs(W, H, fx, max_jump=0.0)
    assert ref0["stats"][0] > _inputs(W, H, fx)[1]["stats"][0]
    _check(f"{W}x{H} max_jump 0", *_run(ops, dev, s, max_jump=0.0), ref0)


def test_unaligned_images_give_the_same_bits(dev):
    """Views at a 4-byte offset into a larger buffer, none 16-byte aligned."""
    from touch_gs_amd import ops
    W, H, fx = 157, 93, 140.0
    s, _ = _inputs(W, H, fx)
    base = _run(ops, dev, s)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
        buf[1:] = torch.from_numpy(a).to(dev).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    cam = _acam(s["cam"])
    vd_buf, va_buf = (torch.zeros(H * W + 1, dtype=torch.float32, device=dev) for _ in range(2))
    got = ops.depth_normal_fwd_bwd(cam, shifted(s["out_depth"]), shifted(s["final_T"]), shifted(s["prior"]), shifted(s["conf"]),
                                   alpha_min=0.5, weight=WEIGHT, want_normals=True)
    for a, b in zip(base, got):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # unaligned outputs as well: accumulate onto zeroed views (0 + value = value; a -0 becomes +0, compare as numbers)
    acc = ops.depth_normal_fwd_bwd(cam, shifted(s["out_depth"]), shifted(s["final_T"]), shifted(s["prior"]), shifted(s["conf"]),
                                   alpha_min=0.5, weight=WEIGHT, accumulate_into=(vd_buf[1:].view(H, W), va_buf[1:].view(H, W)))
    assert torch.equal(acc[2], base[2]) and torch.equal(acc[3], base[3])


def test_two_calls_give_identical_bits_and_the_forward_only_forms_agree(dev):
    from touch_gs_amd import ops
    W, H, fx = 320, 208, 300.0
    s, _ = _inputs(W, H, fx)
    a, b = _run(ops, dev, s), _run(ops, dev, s)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    fwd = _run(ops, dev, s, want_grad=False)
    assert fwd[2] is None and fwd[3] is None
    assert torch.equal(fwd[0].view(torch.int32), a[0].view(torch.int32)) and torch.equal(fwd[1].view(torch.int32), a[1].view(torch.int32))
    t = lambda x: torch.from_numpy(x).to(dev)
    n = ops.depth_normals(_acam(s["cam"]), t(s["out_depth"]), t(s["final_T"]), alpha_min=0.5, max_jump=0.1)
    assert torch.equal(n.view(torch.int32), a[1].view(torch.int32))
    # differentiable through ops.depth_normal_loss: the mean of 1 - cos and its gradient
    d_leaf, a_leaf = t(s["out_depth"]).requires_grad_(True), (1 - t(s["final_T"])).requires_grad_(True)
    loss = ops.depth_normal_loss(_acam(s["cam"]), d_leaf, a_leaf, t(s["prior"]), t(s["conf"]), 0.5, 0.1)
    assert loss.shape == () and float(loss.detach()) == float(a[0][3])
    (3.0 * loss).backward()
    unit = _run(ops, dev, s, max_jump=0.1, weight_override=1.0)      # the images of weight 1, which the Function scales
    assert torch.equal(d_leaf.grad, 3.0 * unit[2]) and torch.equal(a_leaf.grad, 3.0 * unit[3])


def test_accumulate_adds_to_the_pearson_images_bit_for_bit(dev):
    from touch_gs_amd import ops
    W, H, fx = 157, 93, 140.0
    s, _ = _inputs(W, H, fx)
    t = lambda x: torch.from_numpy(x).to(dev)
    mono = t((0.4 * s["out_depth"] / np.maximum(1 - s["final_T"], 1e-3) + 0.1).astype(np.float32) * (s["conf"] > 0))
    _, old_d, old_a = ops.depth_corr_fwd_bwd(t(s["out_depth"]), t(s["final_T"]), mono, 0.5, weight=0.3)
    assert old_d.abs().max() > 0
    stats, _, vd, va = _run(ops, dev, s)
    want_d, want_a = old_d + vd, old_a + va
    st2, _, got_d, got_a = _run(ops, dev, s, accumulate_into=(old_d, old_a))
    assert got_d is old_d and got_a is old_a
    assert torch.equal(got_d.view(torch.int32), want_d.view(torch.int32)) and torch.equal(got_a.view(torch.int32), want_a.view(torch.int32))
    assert torch.equal(stats, st2)
    # one image only: the other is not part of the call
    import ctypes as C
    from touch_gs_amd import _lib
    lib = _lib.load()
    cs = _acam(s["cam"]).c_struct()
    tiles = torch.empty(lib.tgs_num_tiles(W, H), 4, device=dev)
    st3 = torch.empty(8, device=dev)
    only = torch.full((H, W), 7.0, device=dev)
    D, T, P, Cf = t(s["out_depth"]), t(s["final_T"]), t(s["prior"]), t(s["conf"])
    _lib.check(lib.tgs_depth_normal_fwd_bwd(C.byref(cs), D.data_ptr(), T.data_ptr(), P.data_ptr(), Cf.data_ptr(), C.c_float(0.5),
                                            C.c_float(0.1), C.c_float(WEIGHT), tiles.data_ptr(), st3.data_ptr(), None, None,
                                            only.data_ptr(), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(only, va) and torch.equal(st3, stats)


def test_degenerate_frames_give_zeros_and_nothing_non_finite(dev):
    from touch_gs_amd import ops
    W, H, fx = 157, 93, 140.0
    s, _ = _inputs(W, H, fx)
    low = (1.0 - 0.3 * (1.0 - s["final_T"])).astype(np.float32)       # alpha < 0.5 everywhere
    flat_T = np.zeros((H, W), np.float32)
    flat_d = np.full((H, W), 1.25, np.float32)
    head_on = np.zeros((H, W, 3), np.float32)
    head_on[..., 2] = -2.0
    cases = {"no prior": (s["out_depth"], s["final_T"], None, None), "prior of length 0": (s["out_depth"], s["final_T"], np.zeros_like(s["prior"]), s["conf"]),
             "conf all 0": (s["out_depth"], s["final_T"], s["prior"], np.zeros_like(s["conf"])),
             "alpha below alpha_min": (s["out_depth"], low, s["prior"], s["conf"]),
             "constant-depth plane": (flat_d, flat_T, head_on, None)}
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    cam = _acam(s["cam"])
    for name, (d, T, p, c) in cases.items():
        ref = depth_normal_ref(s["cam"], d, T, p, c, 0.5, 0.1, WEIGHT)
        assert ref["stats"][4] == 0 and not ref["G"].any()
        stats, n, vd, va = ops.depth_normal_fwd_bwd(cam, t(d), t(T), t(p), t(c), alpha_min=0.5, max_jump=0.1, weight=WEIGHT,
                                                    want_normals=True)
        st = stats.cpu().numpy()
        print(f"[depth_normal degenerate: {name}] stats {st}")
        assert st[0] == ref["stats"][0] and st[1] == ref["stats"][1], name
        assert st[3] == 0 and st[4] == 0 and np.isfinite(st).all(), name
        assert not vd.any() and not va.any() and torch.isfinite(n).all(), name
        if name == "constant-depth plane":
            assert st[0] == st[1] == (W - 2) * (H - 2)
            assert (n[1:-1, 1:-1].cpu() == torch.tensor([0.0, 0.0, -1.0])).all()      # (0, 0, -1) exactly
        if name == "alpha below alpha_min":
            assert st[0] == 0 and not n.any()


def _rendered(dev, seed):
    from touch_gs_amd import ops
    N, W, H, deg = 20000, 320, 208, 3
    P, ocam = scene(N, W, H, deg, seed)
    acam = amd_cam(ocam)
    D = to_dev(P, dev)
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(acam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], deg)
    rgb, depth_acc, fT, _ = ops.rasterize_fwd(acam, sp, sg, ts)
    return acam, depth_acc, fT


@pytest.mark.parametrize("max_jump", [0.5, 0.1])
@pytest.mark.parametrize("seed", [3, 8])
def test_a_rendered_frame_matches_the_fp64_reference(dev, seed, max_jump):
    """The op on K6's own out_depth / final_T; the prior is the reference's own normals plus noise.

    The jump-gate margin (no ratio within [0.8, 1.25] of the threshold) is asserted at max_jump 0.5.  At the default 0.1 no
    seed has it: of the seeds 1...24 of this scene every frame has 4 100 - 5 700 of its 64 000 ratios inside that band (229 -
    437 at 0.2, none at 0.5 and 1.0), so another seed does not help and the margin is asserted where a rendered frame can
    have it; the gate then is on and cuts nothing, its cutting is pinned by the synthetic cases.  The frames are run at 0.1
    as well, same bars, margin printed and not asserted: kernel and reference make the decision by the same IEEE
    operations on the same bits."""
    from touch_gs_amd import ops
    W, H = 320, 208
    acam, depth_acc, fT = _rendered(dev, seed)
    od, T = depth_acc.cpu().numpy(), fT.cpu().numpy()
    cam = dict(W=W, H=H, fx=float(np.float32(acam.fx)), fy=float(np.float32(acam.fy)), cx=float(np.float32(acam.cx)),
               cy=float(np.float32(acam.cy)), pix_center=float(np.float32(acam.pix_center)))
    # the jump-gate margin on the rendered depth: no decision of the gate depends on a rounding
    _, _, ratio = decisions(od, T, 0.5, max_jump)
    q = ratio[np.isfinite(ratio)]
    near = int(((q >= 0.8) & (q <= 1.25)).sum())
    print(f"[depth_normal rendered seed {seed} max_jump {max_jump}] jump ratios within [0.8, 1.25] of the threshold: "
          f"{near} of {q.size}")
    if max_jump == 0.5:
        assert near == 0
    rng = np.random.default_rng(seed)
    n0 = depth_normal_ref(cam, od, T, None, None, 0.5, max_jump)["normals"]
    prior = ((n0 + 0.2 * rng.standard_normal((H, W, 3))) * (0.5 + rng.random((H, W, 1)))).astype(np.float32)
    conf = np.where(rng.random((H, W)) < 0.1, 0.0, 0.2 + rng.random((H, W))).astype(np.float32)
    ref = depth_normal_ref(cam, od, T, prior, conf, 0.5, max_jump, WEIGHT)
    assert ref["stats"][0] >= 0.2 * W * H           # at least 20 % of the pixels are formed
    got = ops.depth_normal_fwd_bwd(acam, depth_acc, fT, torch.from_numpy(prior).to(dev), torch.from_numpy(conf).to(dev),
                                   alpha_min=0.5, max_jump=max_jump, weight=WEIGHT, want_normals=True)
    _check(f"rendered N=20000 {W}x{H} seed {seed}", *got, ref)


def _model_and_view(dev, mult, with_prior=True, rendered_rgb=False, N=3000, W=160, H=96, deg=3, **cfg_kw):
    """Model + one view whose normal prior is the normals of the model's own depth plus noise, with weights.  ``rendered_rgb``:
    the colour target is the model's own render, so that the L1 term has no gradient and every gradient comes from the prior."""
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    P, cam = scene(N, W, H, deg, 121)
    acam = amd_cam(cam)
    params = GaussianParams.from_tensors(*[P[k].float().to(dev) for k in GaussianParams.NAMES])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        rgb, dacc, alpha, _ = ops.render(params.means, params.log_scales, params.quats, params.opac_logit, params.sh, acam, deg)
    n0 = ops.depth_normals(acam, dacc, 1.0 - alpha, 0.5, 0.1).cpu()
    prior = (n0 + 0.3 * torch.randn(H, W, 3, generator=g)) * (torch.rand(H, W, 1, generator=g) > 0.1)
    conf = 0.2 + torch.rand(H, W, generator=g)
    mono = (2.0 * (dacc / alpha.clamp(min=1e-10)).cpu() + 0.3 + 2.0 * torch.rand(H, W, generator=g)) * (torch.rand(H, W, generator=g) > 0.1)
    target = rgb.contiguous() if rendered_rgb else torch.rand(H, W, 3, generator=g).to(dev)
    view = View(cam=acam, rgb=target, mono_depth=mono.to(dev).contiguous(),
                normal_prior=prior.to(dev).contiguous() if with_prior else None, normal_conf=conf.to(dev) if with_prior else None)
    kw = dict(sh_degree=deg, sh_degree_interval=0, normal_prior_mult=mult)
    kw.update(cfg_kw)
    return DepthGaussianSplattingModel(ModelConfig(**kw), params), view, P


@pytest.mark.parametrize("mono_mult", [0.0, 0.1])
def test_fused_step_equals_the_autograd_path(dev, mono_mult):
    """mono_mult > 0: the Pearson op writes the two images first and this term accumulates onto them."""
    from touch_gs_amd.model import DepthGaussianSplattingModel
    from touch_gs_amd.optim import GaussianParams
    model, view, _ = _model_and_view(dev, 0.3, rendered_rgb=True, ssim_lambda=0.0, mono_depth_mult=mono_mult)
    tl, ss = model.forward_backward(view)
    fused = {k: float(v) for k, v in model.loss_from(tl, ss, view).items()}
    assert "normal_loss" in fused and float(model.last["normal_stats"][1]) > 1000
    assert ("mono_depth_loss" in fused) == (mono_mult > 0)
    fused_grads = {k: model.params.g[k].clone() for k in GaussianParams.NAMES}
    leaves = [getattr(model.params, k).detach().clone().requires_grad_(True) for k in GaussianParams.NAMES]
    p2 = GaussianParams.from_tensors(*[t.detach() for t in leaves])
    for k, t in zip(GaussianParams.NAMES, leaves):
        setattr(p2, k, t)
    m2 = DepthGaussianSplattingModel(model.config, p2)
    ld = m2.get_loss_dict(m2.get_outputs(view.cam), view)
    assert set(ld) == {"main_loss", "normal_loss"} | ({"mono_depth_loss"} if mono_mult > 0 else set())
    sum(ld.values()).backward()
    print(f"[depth_normal fused vs autograd, mono {mono_mult}] normal_loss fused {fused['normal_loss']:.8f} autograd {float(ld['normal_loss'].detach()):.8f}")
    assert abs(float(ld["normal_loss"].detach()) - fused["normal_loss"]) <= 1e-6
    assert fused["normal_loss"] > 1e-4
    # the term reaches every geometric group: against a step without it the gradients differ
    off, view_off, _ = _model_and_view(dev, 0.0, rendered_rgb=True, ssim_lambda=0.0, mono_depth_mult=mono_mult)
    off.forward_backward(view_off)
    for k, t in zip(GaussianParams.NAMES, leaves):
        scale = fused_grads[k].abs().max().item()
        diff = (t.grad - fused_grads[k]).abs().max().item()
        moved = (off.params.g[k] - fused_grads[k]).abs().max().item()
        print(f"[depth_normal fused vs autograd, mono {mono_mult}] {k}: max |grad| {scale:.3e}  max |fused - autograd| {diff:.3e} "
              f"(bound 1e-4 of the former)  max |with - without the term| {moved:.3e}")
        assert diff <= 1e-4 * scale, k
        if k not in ("sh", "sh_dc", "sh_rest"):        # (depth and alpha do not depend on colour)
            assert scale > 0 and moved > 1e-3 * scale, k


def test_switching_the_term_off_changes_nothing(dev):
    """mult = 0 with a prior, mult > 0 without one, and the fields at their defaults: one train_step leaves the three models
    bit-identical, and loss_from has no new key; with the term on the parameters do move."""
    runs = {}
    for name, (mult, with_prior) in {"defaults": (0.0, False), "mult 0": (0.0, True), "no prior": (0.3, False), "on": (0.3, True)}.items():
        model, view, _ = _model_and_view(dev, mult, with_prior)
        if name == "defaults":
            from touch_gs_amd.model import ModelConfig
            assert model.config == ModelConfig(sh_degree=3, sh_degree_interval=0)
        model.train_step(view)
        model.flush()
        keys = set(model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], view))
        runs[name] = (model.params.flat.clone(), keys)
    base, keys = runs["defaults"]
    assert keys == {"main_loss", "depth_loss"}
    for name in ("mult 0", "no prior"):
        assert torch.equal(runs[name][0].view(torch.int32), base.view(torch.int32)), name
        assert runs[name][1] == keys, name
    assert runs["on"][1] == keys | {"normal_loss"}
    assert not torch.equal(runs["on"][0], base)


def test_the_term_optimises_the_angle(dev):
    """5 000 Gaussians at 160x120; prior = the normals of the depth rendered from a target model; start = that model with
    means and scales perturbed; 60 train_steps with normal_prior_mult 0 and on from the same start.  The mean of 1 - cos
    (stats[3], forward-only op, the fixed view) must end below its start with the term on, and below the final value of the
    run without it."""
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_camera, synthetic_gaussians
    N, W, H, deg = 5000, 160, 120, 1
    P, intr = synthetic_gaussians(N, W, H, deg, 77)
    cam = make_camera(intr, 0, 8)
    T = {k: v.to(dev).contiguous() for k, v in P.items()}
    with torch.no_grad():
        rgb, dacc, alpha, _ = ops.render(T["means"], T["log_scales"], T["quats"], T["opac_logit"], T["sh"], cam, deg)
    prior = ops.depth_normals(cam, dacc, 1.0 - alpha, 0.5, 0.1)
    assert (prior.abs().sum(-1) > 0).sum() > 0.2 * W * H
    view = View(cam=cam, rgb=rgb.clamp(0, 1).contiguous(), normal_prior=prior)
    g = torch.Generator().manual_seed(3)
    start = dict(P)
    start["means"] = P["means"] + 0.3 * torch.randn(N, 3, generator=g)
    start["log_scales"] = P["log_scales"] + 0.3 * torch.randn(N, 3, generator=g)

    def mean_one_minus_cos(model):
        with torch.no_grad():
            out = model.get_outputs(cam)
        s = ops.depth_normal_fwd_bwd(cam, out["depth_acc"], 1 - out["alpha"], prior, None, 0.5, 0.1, want_grad=False)[0]
        assert float(s[1]) > 0.1 * W * H
        return float(s[3])

    final = {}
    for mult in (0.0, 0.2):
        params = GaussianParams.from_tensors(*[start[k].to(dev) for k in GaussianParams.NAMES])
        model = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, lr_means=2e-3, lr_means_final=None,
                                                        normal_prior_mult=mult), params)
        first = mean_one_minus_cos(model)
        for _ in range(60):
            model.train_step(view)
        model.flush()
        final[mult] = mean_one_minus_cos(model)
        print(f"[depth_normal optimises] mult {mult}: mean 1 - cos {first:.5f} -> {final[mult]:.5f}")
        assert first > 1e-4        # (there is something to optimise)
    assert final[0.2] < first
    assert final[0.2] < final[0.0]


def test_get_outputs_renders_the_normals_and_eval_reports_the_angle(dev):
    """get_outputs(normals=True) adds the detached normals image of ops.depth_normals and changes no other key's value;
    the eval metric is the weighted mean angle to the prior over the supervised centres."""
    from touch_gs_amd import ops
    model, view, _ = _model_and_view(dev, 0.0)
    with torch.no_grad():
        plain = model.get_outputs(view.cam)
        out = model.get_outputs(view.cam, normals=True)
    assert set(out) == set(plain) | {"normal"} and "normal" not in plain
    for k in plain:
        assert torch.equal(out[k], plain[k]), k
    n = out["normal"]
    assert n.shape == (view.cam.H, view.cam.W, 3) and not n.requires_grad
    assert torch.equal(n, ops.depth_normals(view.cam, out["depth_acc"], 1.0 - out["alpha"], 0.5, 0.1))
    formed = n.abs().sum(-1) > 0
    assert formed.float().mean() > 0.2 and (n[formed].norm(dim=-1) - 1).abs().max() < 1e-5
    # the angle: 0 against the normals themselves, 90 against a perpendicular field, a mix weighted by conf; no key without a prior
    view.normal_prior, view.normal_conf = 2.5 * n, None
    m, images = model.get_image_metrics_and_images(out, view)
    assert m["normal_angle_deg"] < 0.05 and images["normal"].min() >= 0 and images["normal"].max() <= 1
    perp = torch.cross(n, torch.tensor([1.0, 0.0, 0.0], device=dev).expand_as(n), dim=-1)
    ok = perp.norm(dim=-1) > 1e-3
    half = torch.zeros_like(ok)
    half[:, : view.cam.W // 2] = True
    view.normal_prior = torch.where((ok & half)[..., None], perp, n)
    view.normal_conf = torch.where(ok & half, 3.0, 1.0)
    m, _ = model.get_image_metrics_and_images(out, view)
    sup = formed
    want = 90.0 * (3.0 * (sup & ok & half).sum()) / (3.0 * (sup & ok & half).sum() + (sup & ~(ok & half)).sum())
    assert abs(m["normal_angle_deg"] - float(want)) < 0.05
    view.normal_prior = view.normal_conf = None
    m, images = model.get_image_metrics_and_images(out, view)
    assert "normal_angle_deg" not in m and "normal" in images
    assert "normal" not in model.get_image_metrics_and_images(plain, view)[1]
