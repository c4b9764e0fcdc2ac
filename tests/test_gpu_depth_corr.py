"""GPU tests of the scale-invariant monocular depth loss (csrc/depthcorr.hip / tgs_depth_corr_fwd_bwd /
ops.depth_corr_fwd_bwd / ops.depth_correlation) against the fp64 reference of tests/depth_corr_ref.py, which reads the same
fp32 images and makes the same fp32 validity decision, and of the model paths above it.

Bars (set by the feature's specification, not tuned):
  * |rho - rho_ref| <= 1e-5; n exact; means and moments within 1e-5 relative;
  * on EVERY valid pixel |v_depth - ref| <= 1e-5 s_i / alpha_i and |v_alpha - ref| <= 1e-5 s_i x_i / alpha_i, s_i = the
    per-pixel gradient scale of the reference; both images exactly 0 on every invalid pixel;
  * degenerate frames: rho = loss = 0, all-zero images, nothing non-finite; two calls give identical bits;
  * fused step against autograd: every parameter gradient group within 1e-4 of the group's largest magnitude, the two
    loss values within 1e-6; with the term off nothing changes, bit for bit.
1e-5 is 30 x what a CPU emulation of the kernels' arithmetic (fp32 per tile, fp64 fold, fp32 per pixel) shows.

Each test prints its observed maxima next to the bound (run with -s).  Observed on an MI355X: |rho - rho_ref| <= 2.7e-8,
moments <= 1e-7 relative, v_depth / v_alpha <= 5.3e-7 of their scale over the twelve synthetic cases and the two rendered
frames; fused against autograd <= 2.2e-6 of a group's largest gradient, loss values equal to eight digits; the 60-step run
takes 1 - rho from 0.862 to 0.037 with the term and to 0.719 without.
"""
import numpy as np
import pytest
import torch

from tests.depth_corr_ref import depth_corr_ref, max_errors, synthetic_images
from tests.util import amd_cam, scene, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
_CACHE = {}


def _inputs(W, H, rel_noise):
    """Synthetic images + their fp64 reference, computed once per (shape, noise) and never modified."""
    key = (W, H, rel_noise)
    if key not in _CACHE:
        od, fT, mono = synthetic_images(W, H, rel_noise, seed=1)
        _CACHE[key] = (od, fT, mono, depth_corr_ref(od, fT, mono, 0.5, 0.25))
    return _CACHE[key]


def _check(label, stats, vd, va, ref, weight):
    st = stats.double().cpu().numpy()
    vd, va = vd.cpu().numpy(), va.cpu().numpy()
    e = max_errors(st, vd, va, ref)
    print(f"[depth_corr {label}] n {int(st[0])} rho {ref['stats'][6]:.7f}  |rho err| {e['rho']:.2e}  moments rel {e['moments']:.2e}  "
          f"v_depth err / scale {e['v_depth']:.2e}  v_alpha err / scale {e['v_alpha']:.2e}  (bound {TOL:.0e})")
    assert np.isfinite(st).all() and np.isfinite(vd).all() and np.isfinite(va).all()
    assert st[0] == ref["stats"][0]
    assert e["rho"] <= TOL and e["moments"] <= TOL
    assert e["loss"] <= TOL * abs(weight)
    assert e["v_depth"] <= TOL and e["v_alpha"] <= TOL       # every valid pixel, none left out
    inv = ~ref["valid"]
    assert (vd[inv].view(np.uint32) << 1 == 0).all() and (va[inv].view(np.uint32) << 1 == 0).all()   # +-0 exactly
    assert np.abs(vd[ref["valid"]]).max() > 0
    return e


@pytest.mark.parametrize("rel_noise", [0.3, 0.1, 1e-3])
@pytest.mark.parametrize("W,H", [(16, 16), (157, 93), (320, 208), (1280, 720)])
def test_synthetic_images_match_the_fp64_reference(dev, W, H, rel_noise):
    from touch_gs_amd import ops
    od, fT, mono, ref = _inputs(W, H, rel_noise)
    t = lambda a: torch.from_numpy(a).to(dev)
    stats, vd, va = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), alpha_min=0.5, weight=0.25)
    assert stats.shape == (8,) and vd.shape == va.shape == (H, W)
    assert 0.5 * W * H < ref["stats"][0] < 0.9 * W * H
    _check(f"{W}x{H} noise {rel_noise}", stats, vd, va, ref, 0.25)


def test_unaligned_images_take_the_scalar_path_and_give_the_same_bits(dev):
    """Image pointers that are not 16-byte aligned (views into a larger buffer) select the gradient kernel's scalar form."""
    from touch_gs_amd import ops
    W, H = 157, 93
    od, fT, mono, ref = _inputs(W, H, 0.1)
    t = lambda a: torch.from_numpy(a).to(dev)
    base = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), weight=0.25)

    def shifted(a):
        buf = torch.empty(H * W + 1, dtype=torch.float32, device=dev)
        buf[1:] = t(a).reshape(-1)
        v = buf[1:].view(H, W)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    got = ops.depth_corr_fwd_bwd(shifted(od), shifted(fT), shifted(mono), weight=0.25)
    for a, b in zip(base, got):
        assert torch.equal(a, b)


def test_degenerate_frames_give_zeros_and_nothing_non_finite(dev):
    from touch_gs_amd import ops
    W, H = 157, 93
    od, fT, mono, _ = _inputs(W, H, 0.1)
    one = np.zeros_like(mono)
    iy, ix = np.argwhere(depth_corr_ref(od, fT, mono)["valid"])[40]
    one[iy, ix] = mono[iy, ix]
    # constant depth: alpha is 1 or 0 and the depth a dyadic number, so that x = 1.25 exactly and fp32 sums of it are
    # exact (a constant whose multiples round is constant only to within an ulp, and such a frame is not degenerate)
    fT_c = np.where(fT < 0.45, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    od_c = (np.float32(1.25) * (1 - fT_c)).astype(np.float32)
    cases = {"no map": (od, fT, np.zeros_like(mono)), "one valid pixel": (od, fT, one), "constant depth": (od_c, fT_c, mono)}
    t = lambda a: torch.from_numpy(a).to(dev)
    for name, (d, T, m) in cases.items():
        ref = depth_corr_ref(d, T, m, 0.5, 0.3)
        assert ref["stats"][6] == 0 and ref["stats"][7] == 0
        stats, vd, va = ops.depth_corr_fwd_bwd(t(d), t(T), t(m), alpha_min=0.5, weight=0.3)
        st = stats.cpu().numpy()
        print(f"[depth_corr degenerate: {name}] stats {st}")
        assert st[0] == ref["stats"][0], name
        assert st[6] == 0 and st[7] == 0, name
        assert np.isfinite(st).all(), name
        assert not vd.any() and not va.any(), name
        fwd, none_d, none_a = ops.depth_corr_fwd_bwd(t(d), t(T), t(m), alpha_min=0.5, weight=0.3, want_grad=False)
        assert none_d is None and none_a is None and torch.equal(fwd, stats)


def test_two_calls_give_identical_bits_and_forward_only_the_same_stats(dev):
    from touch_gs_amd import _lib, ops
    import ctypes as C
    W, H = 320, 208
    od, fT, mono, _ = _inputs(W, H, 0.1)
    t = lambda a: torch.from_numpy(a).to(dev)
    a = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), weight=0.25)
    b = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), weight=0.25)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    fwd, vd, va = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), weight=0.25, want_grad=False)
    assert vd is None and va is None and torch.equal(fwd.view(torch.int32), a[0].view(torch.int32))
    # the C entry point with one image only: the other buffer is not part of the call, the given one holds the same bits
    lib = _lib.load()
    tiles = torch.empty(lib.tgs_num_tiles(W, H), 8, device=dev)
    stats = torch.empty(8, device=dev)
    only = torch.full((H, W), 7.0, device=dev)
    D, T, M = t(od), t(fT), t(mono)
    _lib.check(lib.tgs_depth_corr_fwd_bwd(W, H, D.data_ptr(), T.data_ptr(), M.data_ptr(), C.c_float(0.5), C.c_float(0.25),
                                          tiles.data_ptr(), stats.data_ptr(), None, only.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(only, a[2]) and torch.equal(stats, a[0])
    # the op is differentiable through ops.depth_correlation: rho and d rho / d (depth_acc, alpha)
    d_leaf, a_leaf = t(od).requires_grad_(True), (1 - t(fT)).requires_grad_(True)
    rho = ops.depth_correlation(d_leaf, a_leaf, t(mono), 0.5)
    assert rho.shape == () and float(rho.detach()) == float(a[0][6])
    (3.0 * rho).backward()
    assert torch.allclose(d_leaf.grad, a[1] * (-3.0 / 0.25), rtol=1e-6, atol=0)
    assert torch.allclose(a_leaf.grad, a[2] * (-3.0 / 0.25), rtol=1e-6, atol=0)


@pytest.mark.parametrize("seed", [3, 8])
def test_a_rendered_frame_matches_the_fp64_reference(dev, seed):
    """The op on K6's own out_depth / final_T: kernel and reference read the same images, so the valid sets coincide and
    no pixel is excluded."""
    from touch_gs_amd import ops
    N, W, H, deg = 20000, 320, 208, 3
    P, ocam = scene(N, W, H, deg, seed)
    acam = amd_cam(ocam)
    D = to_dev(P, dev)
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(acam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], deg)
    rgb, depth_acc, fT, _ = ops.rasterize_fwd(acam, sp, sg, ts)
    od, T = depth_acc.cpu().numpy(), fT.cpu().numpy()
    rng = np.random.default_rng(seed)
    dhat = od.astype(np.float64) / np.maximum(1.0 - T.astype(np.float64), 1e-10)
    mono = (0.37 * dhat + 0.11) * (1 + 0.1 * rng.standard_normal((H, W)))
    mono = np.where(rng.random((H, W)) < 0.1, 0.0, np.maximum(mono, 1e-3)).astype(np.float32)
    ref = depth_corr_ref(od, T, mono, 0.5, 0.2)
    assert ref["stats"][0] > 0.2 * W * H            # (the frame is not mostly background)
    stats, vd, va = ops.depth_corr_fwd_bwd(depth_acc, fT, torch.from_numpy(mono).to(dev), alpha_min=0.5, weight=0.2)
    _check(f"rendered N={N} {W}x{H} seed {seed}", stats, vd, va, ref, 0.2)


def _model_and_view(dev, mult, with_map=True, rendered_rgb=False, N=3000, W=160, H=96, deg=3, **cfg_kw):
    """Model + one view whose monocular map is a noisy affine map of the model's own depth.  ``rendered_rgb``: the colour
    target is the model's own render, so that the L1 term has no gradient and every gradient comes from the mono term."""
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    P, cam = scene(N, W, H, deg, 121)
    acam = amd_cam(cam)
    params = GaussianParams.from_tensors(*[P[k].float().to(dev) for k in GaussianParams.NAMES])
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        rgb, dacc, alpha, _ = ops.render(params.means, params.log_scales, params.quats, params.opac_logit, params.sh, acam, deg)
    dhat = (dacc / alpha.clamp(min=1e-10)).cpu()
    mono = (2.0 * dhat + 0.3 + 2.0 * torch.rand(H, W, generator=g)) * (torch.rand(H, W, generator=g) > 0.1)
    target = rgb.contiguous() if rendered_rgb else torch.rand(H, W, 3, generator=g).to(dev)
    view = View(cam=acam, rgb=target, mono_depth=mono.to(dev).contiguous() if with_map else None)
    kw = dict(sh_degree=deg, sh_degree_interval=0, mono_depth_mult=mult)
    kw.update(cfg_kw)
    return DepthGaussianSplattingModel(ModelConfig(**kw), params), view, P


def test_fused_step_equals_the_autograd_path(dev):
    from touch_gs_amd.model import DepthGaussianSplattingModel
    from touch_gs_amd.optim import GaussianParams
    model, view, _ = _model_and_view(dev, 0.1, rendered_rgb=True, ssim_lambda=0.0)
    tl, ss = model.forward_backward(view)
    fused = {k: float(v) for k, v in model.loss_from(tl, ss, view).items()}
    assert "mono_depth_loss" in fused and float(model.last["mono_stats"][0]) > 1000
    fused_grads = {k: model.params.g[k].clone() for k in GaussianParams.NAMES}
    leaves = [getattr(model.params, k).detach().clone().requires_grad_(True) for k in GaussianParams.NAMES]
    p2 = GaussianParams.from_tensors(*[t.detach() for t in leaves])
    for k, t in zip(GaussianParams.NAMES, leaves):
        setattr(p2, k, t)
    m2 = DepthGaussianSplattingModel(model.config, p2)
    ld = m2.get_loss_dict(m2.get_outputs(view.cam), view)
    assert set(ld) == {"main_loss", "mono_depth_loss"}
    sum(ld.values()).backward()
    print(f"[depth_corr fused vs autograd] mono_depth_loss fused {fused['mono_depth_loss']:.8f} autograd {float(ld['mono_depth_loss']):.8f}")
    assert abs(float(ld["mono_depth_loss"]) - fused["mono_depth_loss"]) <= 1e-6
    assert 0 < fused["mono_depth_loss"] < 0.1
    # the term reaches every group: against a step without it the gradients differ
    off, view_off, _ = _model_and_view(dev, 0.0, rendered_rgb=True, ssim_lambda=0.0)
    off.forward_backward(view_off)
    for k, t in zip(GaussianParams.NAMES, leaves):
        scale = fused_grads[k].abs().max().item()
        diff = (t.grad - fused_grads[k]).abs().max().item()
        moved = (off.params.g[k] - fused_grads[k]).abs().max().item()
        print(f"[depth_corr fused vs autograd] {k}: max |grad| {scale:.3e}  max |fused - autograd| {diff:.3e} (bound 1e-4 of the former)  "
              f"max |with - without the term| {moved:.3e}")
        assert diff <= 1e-4 * scale, k
        if k not in ("sh", "sh_dc", "sh_rest"):        # (depth and alpha do not depend on colour)
            assert scale > 0 and moved > 1e-3 * scale, k


def test_switching_the_term_off_changes_nothing(dev):
    """mult = 0 with a map, mult > 0 without a map, and the fields at their defaults: one train_step leaves the three models
    bit-identical, and loss_from has no new key; with the term on the parameters do move."""
    runs = {}
    for name, (mult, with_map) in {"defaults": (0.0, False), "mult 0": (0.0, True), "no map": (0.2, False), "on": (0.2, True)}.items():
        model, view, _ = _model_and_view(dev, mult, with_map)
        if name == "defaults":
            from touch_gs_amd.model import ModelConfig
            assert model.config == ModelConfig(sh_degree=3, sh_degree_interval=0)
        model.train_step(view)
        model.flush()
        keys = set(model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], view))
        runs[name] = (model.params.flat.clone(), keys)
    base, keys = runs["defaults"]
    assert keys == {"main_loss", "depth_loss"}
    for name in ("mult 0", "no map"):
        assert torch.equal(runs[name][0].view(torch.int32), base.view(torch.int32)), name
        assert runs[name][1] == keys, name
    assert runs["on"][1] == keys | {"mono_depth_loss"}
    assert not torch.equal(runs["on"][0], base)


def test_the_term_optimises_the_correlation(dev):
    """5 000 Gaussians at 160x120; mono = an affine map of the depth rendered from a target model; start = that model with
    means and scales perturbed; 60 train_steps with mono_depth_mult 0 and 0.2 from the same start.  1 - rho (forward-only
    op, the fixed view) must end below its start with the term on, and below the final value of the run without it."""
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
    mono = torch.where(alpha > 0.05, 3.0 * dacc / alpha.clamp(min=1e-10) + 0.7, torch.zeros_like(dacc)).contiguous()
    view = View(cam=cam, rgb=rgb.clamp(0, 1).contiguous(), mono_depth=mono)
    g = torch.Generator().manual_seed(3)
    start = dict(P)
    start["means"] = P["means"] + 0.3 * torch.randn(N, 3, generator=g)
    start["log_scales"] = P["log_scales"] + 0.3 * torch.randn(N, 3, generator=g)

    def one_minus_rho(model):
        with torch.no_grad():
            out = model.get_outputs(cam)
        s, _, _ = ops.depth_corr_fwd_bwd(out["depth_acc"], 1 - out["alpha"], mono, 0.5, want_grad=False)
        assert float(s[0]) > 0.3 * W * H
        return 1.0 - float(s[6])

    final = {}
    for mult in (0.0, 0.2):
        params = GaussianParams.from_tensors(*[start[k].to(dev) for k in GaussianParams.NAMES])
        model = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, lr_means=2e-3, lr_means_final=None,
                                                        mono_depth_mult=mult), params)
        first = one_minus_rho(model)
        for _ in range(60):
            model.train_step(view)
        model.flush()
        final[mult] = one_minus_rho(model)
        print(f"[depth_corr optimises] mult {mult}: 1 - rho {first:.5f} -> {final[mult]:.5f}")
        assert first > 1e-4        # (there is something to optimise)
    assert final[0.2] < first
    assert final[0.2] < final[0.0]
