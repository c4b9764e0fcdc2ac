"""GPU tests of the patch-wise (local) Pearson term for raw monocular depth (csrc/depthcorr.hip: k_dcorr_patches,
k_dcorr_patch_sum, k_dcorr_grad_local / tgs_depth_corr_local_fwd_bwd / ops.depth_corr_local_fwd_bwd /
ops.depth_correlation_local) against the fp64 reference of tests/depth_corr_local_ref.py, which reads the same fp32 images
and makes the same fp32 validity decision, and of the model paths above it.

Bars (set by the feature's specification, not tuned):
  * n_p, stats[8] (patches that pass the count gate), A and every active flag exact; |rho_p - ref|, |rho_bar - ref| and
    |rho - ref| <= 1e-5; stats[0..7] equal to ops.depth_corr_fwd_bwd(weight = weight_global) bit for bit;
  * on EVERY valid pixel |v_depth - ref| <= 1e-5 s_i / alpha_i and |v_alpha - ref| <= 1e-5 s_i x_i / alpha_i, s_i = the
    global scale plus the same scale formed with the patch's statistics and weight_local / A; exactly +-0 on every invalid
    pixel; an inactive patch's pixels carry exactly the global op's gradient;
  * no gate decision of the synthetic cases may lie within 10 % of its threshold (none does: the smallest variance ratio
    of a counted patch is 0.048 against 1e-3); on the rendered frames such patches take the kernel's decision and may
    number at most 5 % of stats[8];
  * fused step against autograd: every gradient group within 1e-4 of its largest magnitude, loss values within 1e-6;
    with the term off nothing changes, bit for bit.
1e-5 is the bar of the global op (tests/test_gpu_depth_corr.py); a CPU emulation of this arithmetic (fp32 per tile, fp64
combine) on the synthetic inputs gives a largest rho_p error of 2.5e-7.

Each test prints its observed maxima next to the bound (run with -s).  Observed on an MI355X over the 61 synthetic cases, the
gate case and the two rendered frames: |rho_p - ref| <= 2.1e-7, |rho_bar - ref| <= 1.1e-7, |rho - ref| <= 3.7e-8, v_depth /
v_alpha <= 1.3e-6 of their scale; no patch of the rendered frames within 10 % of the variance gate (0 of 15, 0 of 20);
fused against autograd <= 2.3e-6 of a group's largest gradient, loss values equal to eight digits; the 60-step run takes
rho_bar from 0.029 to 0.949 with the term and to 0.122 without.
"""
import numpy as np
import pytest
import torch

from tests.depth_corr_local_ref import depth_corr_local_ref, min_count_of
from tests.depth_corr_ref import depth_corr_ref, max_errors, synthetic_images
from tests.test_gpu_depth_corr import _model_and_view
from tests.util import amd_cam, scene, to_dev

pytestmark = pytest.mark.gpu

TOL = 1e-5
WG, WL = 0.25, 0.15
MIN_FILL, MIN_VAR = 0.25, 1e-3
_IMG, _REF = {}, {}


def _images(W, H, rel_noise):
    key = (W, H, rel_noise)
    if key not in _IMG:
        _IMG[key] = synthetic_images(W, H, rel_noise, seed=1)
    return _IMG[key]


def _inputs(W, H, rel_noise, k, off):
    """Synthetic images + their fp64 reference, computed once per case and never modified."""
    key = (W, H, rel_noise, k, off)
    if key not in _REF:
        od, fT, mono = _images(W, H, rel_noise)
        _REF[key] = depth_corr_local_ref(od, fT, mono, 0.5, WG, WL, k, off, min_count_of(k, MIN_FILL), MIN_VAR)
    return _images(W, H, rel_noise) + (_REF[key],)


def _near_gate(ref, min_var=MIN_VAR):
    """Counted patches whose variance ratio lies within +-10 % of the gate."""
    near = lambda r: np.isfinite(r) & (r >= 0.9 * min_var) & (r <= 1.1 * min_var)
    return ref["counted"] & (near(ref["ratio_x"]) | near(ref["ratio_y"]))


def _is_zero(a):
    return (a.view(np.uint32) << 1 == 0)


def _check(label, stats, vd, va, patches, ref, wg=WG, wl=WL):
    st = stats.double().cpu().numpy()
    vd, va = vd.cpu().numpy(), va.cpu().numpy()
    ps = patches.cpu().numpy().reshape(-1, 8)
    P = ref["PW"] * ref["PH"]
    assert st.shape == (16,) and ps.shape == (P, 8) and patches.shape[:2] == (ref["PH"], ref["PW"])     # no patch left out
    assert np.isfinite(st).all() and np.isfinite(vd).all() and np.isfinite(va).all() and np.isfinite(ps).all()
    e = max_errors(st[:8], vd, va, ref)
    act = ref["active"]
    e_rho_p = np.abs(ps[:, 5].astype(np.float64) - ref["rho"]).max()
    e_bar = abs(st[10] - ref["stats"][10])
    print(f"[depth_corr_local {label}] patches {P} counted {int(st[8])} active {int(st[9])}  rho_bar {ref['stats'][10]:.7f}  "
          f"|rho err| {e['rho']:.2e}  |rho_bar err| {e_bar:.2e}  max |rho_p err| {e_rho_p:.2e}  v_depth err / scale {e['v_depth']:.2e}  "
          f"v_alpha err / scale {e['v_alpha']:.2e}  (bound {TOL:.0e})")
    assert np.array_equal(ps[:, 6], ref["n"].astype(np.float32))                # n_p exact
    assert np.array_equal(ps[:, 0] != 0, act) and np.isin(ps[:, 0], (0.0, 1.0)).all()       # every active flag
    assert np.array_equal(ps[:, 7] != 0, ref["counted"])
    assert st[8] == ref["stats"][8] and st[9] == ref["stats"][9] == act.sum()
    assert e["rho"] <= TOL and e_bar <= TOL and e_rho_p <= TOL
    assert abs(st[11] - ref["stats"][11]) <= TOL * abs(wl) and abs(st[12] - ref["stats"][12]) <= TOL * (abs(wg) + abs(wl))
    assert (st[13:] == 0).all()
    assert e["v_depth"] <= TOL and e["v_alpha"] <= TOL       # every valid pixel, none left out
    inv = ~ref["valid"]
    assert _is_zero(vd[inv]).all() and _is_zero(va[inv]).all()   # +-0 exactly
    return e


CASES = [(1, (0, 0)), (2, (0, 0)), (2, (1, 1)), (4, (0, 0)), (4, (3, 1))]


def _run_case(dev, W, H, rel_noise, k, off):
    from touch_gs_amd import ops
    od, fT, mono, ref = _inputs(W, H, rel_noise, k, off)
    assert not _near_gate(ref).any()          # none is allowed here: every gate decision is far from its threshold
    t = lambda a: torch.from_numpy(a).to(dev)
    stats, vd, va, patches = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), 0.5, WG, WL, patch_tiles=k, offset=off,
                                                          min_fill=MIN_FILL, min_var_ratio=MIN_VAR, return_patches=True)
    assert vd.shape == va.shape == (H, W)
    _check(f"{W}x{H} noise {rel_noise} k {k} off {off}", stats, vd, va, patches, ref)
    g_stats, g_vd, g_va = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), alpha_min=0.5, weight=WG)
    assert torch.equal(stats[:8].view(torch.int32), g_stats.view(torch.int32))          # bit for bit
    if ref["stats"][9] == 0:      # no active patch: local loss 0 and the global gradient alone
        assert float(stats[10]) == 0 and float(stats[11]) == 0 and float(stats[12]) == float(stats[7])
        assert torch.equal(vd.view(torch.int32), g_vd.view(torch.int32)) and torch.equal(va.view(torch.int32), g_va.view(torch.int32))
    return ref


@pytest.mark.parametrize("k,off", CASES)
@pytest.mark.parametrize("rel_noise", [0.3, 0.1, 1e-3])
@pytest.mark.parametrize("W,H", [(16, 16), (48, 32), (157, 93), (320, 208)])
def test_synthetic_images_match_the_fp64_reference(dev, W, H, rel_noise, k, off):
    ref = _run_case(dev, W, H, rel_noise, k, off)
    if (W, H) == (16, 16) and k >= 2:
        assert ref["stats"][9] == 0         # one tile cannot fill a quarter of a 32-pixel patch
    if (W, H) == (320, 208):
        assert ref["stats"][9] >= 2


def test_a_720p_image_with_128_pixel_patches(dev):
    ref = _run_case(dev, 1280, 720, 0.1, 8, (5, 2))
    assert ref["stats"][9] >= 20


def test_the_three_gates(dev):
    """157x93, k = 2 (5 x 3 patches of 32 x 32 pixels): patch 0 flat in x (alpha in {0, 1}, depth 1.25: vx = 0 exactly), patch 1
    flat in mono, patch 2 thinned below min_count.  Each is inactive, counted as the rule says, and its pixels carry exactly
    the global gradient; the rest match the reference."""
    from touch_gs_amd import ops
    W, H, k = 157, 93, 2
    od, fT, mono = (a.copy() for a in _images(W, H, 0.1))
    fT[:32, :32] = np.where(fT[:32, :32] < 0.45, np.float32(0.0), np.float32(1.0))
    od[:32, :32] = np.float32(1.25) * (1 - fT[:32, :32])
    mono[:32, 32:64] = np.where(mono[:32, 32:64] > 0, np.float32(3.0), np.float32(0.0))
    thin = mono[:32, 64:96].copy()
    keep = np.zeros(thin.size, bool)
    keep[::11] = True                       # 94 of 1024 pixels keep their map value (before validity): below 256
    mono[:32, 64:96] = np.where(keep.reshape(thin.shape), thin, np.float32(0.0))
    mc = min_count_of(k, MIN_FILL)
    assert mc == 256
    ref = depth_corr_local_ref(od, fT, mono, 0.5, WG, WL, k, (0, 0), mc, MIN_VAR)
    assert ref["n"][0] >= mc and ref["n"][1] >= mc and 2 <= ref["n"][2] < mc
    assert ref["ratio_x"][0] == 0 and ref["ratio_y"][1] == 0
    assert list(ref["counted"][:3]) == [True, True, False] and not ref["active"][:3].any() and ref["active"][3:].all()
    assert not _near_gate(ref).any()
    t = lambda a: torch.from_numpy(a).to(dev)
    stats, vd, va, patches = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), 0.5, WG, WL, patch_tiles=k, offset=(0, 0),
                                                          min_fill=MIN_FILL, min_var_ratio=MIN_VAR, return_patches=True)
    _check("gates", stats, vd, va, patches, ref)
    assert float(stats[8]) == 14 and float(stats[9]) == 12
    _, g_vd, g_va = ops.depth_corr_fwd_bwd(t(od), t(fT), t(mono), alpha_min=0.5, weight=WG)
    off_patches = torch.from_numpy(ref["pid"] < 3).to(dev)
    assert torch.equal(vd[off_patches].view(torch.int32), g_vd[off_patches].view(torch.int32))
    assert torch.equal(va[off_patches].view(torch.int32), g_va[off_patches].view(torch.int32))
    assert not torch.equal(vd[~off_patches], g_vd[~off_patches])


def test_degenerate_frames_give_zeros_identical_bits_and_forward_only_the_same_stats(dev):
    from touch_gs_amd import ops
    W, H, k = 157, 93, 2
    od, fT, mono = _images(W, H, 0.1)
    one = np.zeros_like(mono)
    iy, ix = np.argwhere(depth_corr_ref(od, fT, mono)["valid"])[40]
    one[iy, ix] = mono[iy, ix]
    fT_c = np.where(fT < 0.45, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    od_c = (np.float32(1.25) * (1 - fT_c)).astype(np.float32)
    cases = {"no map": (od, fT, np.zeros_like(mono)), "one valid pixel": (od, fT, one), "constant depth": (od_c, fT_c, mono)}
    t = lambda a: torch.from_numpy(a).to(dev)
    kw = dict(alpha_min=0.5, weight_global=0.3, weight_local=0.2, patch_tiles=k, offset=(1, 0), min_fill=MIN_FILL, min_var_ratio=MIN_VAR)
    for name, (d, T, m) in cases.items():
        ref = depth_corr_local_ref(d, T, m, 0.5, 0.3, 0.2, k, (1, 0), min_count_of(k, MIN_FILL), MIN_VAR)
        assert ref["stats"][9] == 0 and ref["stats"][12] == 0
        a = ops.depth_corr_local_fwd_bwd(t(d), t(T), t(m), return_patches=True, **kw)
        b = ops.depth_corr_local_fwd_bwd(t(d), t(T), t(m), return_patches=True, **kw)
        st = a[0].cpu().numpy()
        print(f"[depth_corr_local degenerate: {name}] stats {st}")
        assert np.isfinite(st).all() and torch.isfinite(a[3]).all(), name
        assert st[0] == ref["stats"][0] and st[8] == ref["stats"][8], name
        assert (st[[6, 7, 9, 10, 11, 12, 13, 14, 15]] == 0).all(), name
        assert not a[1].any() and not a[2].any() and not a[3][..., 0].any(), name
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
        fwd, none_d, none_a = ops.depth_corr_local_fwd_bwd(t(d), t(T), t(m), want_grad=False, **kw)
        assert none_d is None and none_a is None and torch.equal(fwd.view(torch.int32), a[0].view(torch.int32)), name
    # a frame that is not degenerate: two calls, and the forward-only call, give identical bits too
    a = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), return_patches=True, **kw)
    b = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), return_patches=True, **kw)
    assert float(a[0][9]) >= 6
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    fwd, _, _ = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), want_grad=False, **kw)
    assert torch.equal(fwd.view(torch.int32), a[0].view(torch.int32))


@pytest.mark.parametrize("W,H", [(157, 93), (160, 96)])
def test_unaligned_and_odd_width_images_take_the_scalar_form_and_give_the_same_bits(dev, W, H):
    """Image pointers at 4 modulo 16 (views into a larger buffer) select the gradient kernel's scalar form, as an odd W does;
    at W = 160 the aligned call is the vector form, so the two forms are compared with each other."""
    from touch_gs_amd import ops
    od, fT, mono = _images(W, H, 0.1)
    t = lambda a: torch.from_numpy(a).to(dev)
    kw = dict(alpha_min=0.5, weight_global=WG, weight_local=WL, patch_tiles=2, offset=(1, 1), min_fill=MIN_FILL,
              min_var_ratio=MIN_VAR, return_patches=True)
    base = ops.depth_corr_local_fwd_bwd(t(od), t(fT), t(mono), **kw)
    assert float(base[0][9]) >= 4 and all(a.data_ptr() % 16 == 0 for a in base[1:3])

    def shifted(a):
        buf = torch.empty(H * W + 1, dtype=torch.float32, device=dev)
        buf[1:] = t(a).reshape(-1)
        v = buf[1:].view(H, W)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    got = ops.depth_corr_local_fwd_bwd(shifted(od), shifted(fT), shifted(mono), **kw)
    for a, b in zip(base, got):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("seed,off", [(3, (0, 0)), (8, (3, 1))])
def test_a_rendered_frame_matches_the_fp64_reference(dev, seed, off):
    """The op on K6's own out_depth / final_T with k = 4; the map carries a smooth multiplicative distortion on top of the
    affine map and the noise.  A counted patch whose reference variance ratio lies within +-10 % of min_var_ratio takes the
    kernel's own decision in the reference; such patches may number at most 5 % of stats[8]."""
    from touch_gs_amd import ops
    N, W, H, deg, k = 20000, 320, 208, 3, 4
    P, ocam = scene(N, W, H, deg, seed)
    acam = amd_cam(ocam)
    D = to_dev(P, dev)
    sp, radii, gb, ts, sg, st = ops.project_bin_sort(acam, D["means"], D["log_scales"], D["quats"], D["opac_logit"], D["sh"], deg)
    rgb, depth_acc, fT, _ = ops.rasterize_fwd(acam, sp, sg, ts)
    od, T = depth_acc.cpu().numpy(), fT.cpu().numpy()
    rng = np.random.default_rng(seed)
    dhat = od.astype(np.float64) / np.maximum(1.0 - T.astype(np.float64), 1e-10)
    px = np.arange(W)[None, :]
    mono = (0.37 * dhat + 0.11) * (1 + 0.2 * np.sin(px / 40.0)) * (1 + 0.1 * rng.standard_normal((H, W)))
    mono = np.where(rng.random((H, W)) < 0.1, 0.0, np.maximum(mono, 1e-3)).astype(np.float32)
    mc = min_count_of(k, MIN_FILL)
    stats, vd, va, patches = ops.depth_corr_local_fwd_bwd(depth_acc, fT, torch.from_numpy(mono).to(dev), 0.5, 0.2, 0.1,
                                                          patch_tiles=k, offset=off, min_fill=MIN_FILL, min_var_ratio=MIN_VAR,
                                                          return_patches=True)
    ref = depth_corr_local_ref(od, T, mono, 0.5, 0.2, 0.1, k, off, mc, MIN_VAR)
    near = np.flatnonzero(_near_gate(ref))
    counted = float(stats[8])
    print(f"[depth_corr_local rendered seed {seed}] patches within 10 % of the variance gate: {len(near)} of {int(counted)} counted "
          f"(cap 5 %)")
    assert ref["stats"][0] > 0.2 * W * H and counted >= 4
    assert len(near) <= 0.05 * counted
    if len(near):
        flags = patches.cpu().numpy().reshape(-1, 8)[:, 0] != 0
        ref = depth_corr_local_ref(od, T, mono, 0.5, 0.2, 0.1, k, off, mc, MIN_VAR, active_override={int(p): bool(flags[p]) for p in near})
    assert ref["stats"][9] >= 2
    _check(f"rendered N={N} {W}x{H} seed {seed} k {k} off {off}", stats, vd, va, patches, ref, 0.2, 0.1)


LOCAL_CFG = dict(mono_depth_patch_tiles=2, mono_depth_patch_min_fill=0.1)


def test_fused_step_equals_the_autograd_path(dev):
    """All gradient from the local term: the colour target is the model's own render, ssim_lambda 0, global mult 0."""
    from touch_gs_amd.model import DepthGaussianSplattingModel
    from touch_gs_amd.optim import GaussianParams
    model, view, _ = _model_and_view(dev, 0.0, rendered_rgb=True, ssim_lambda=0.0, mono_depth_local_mult=0.1, **LOCAL_CFG)
    model.step = 3                      # offset (1, 1)
    tl, ss = model.forward_backward(view)
    fused = {k: float(v) for k, v in model.loss_from(tl, ss, view).items()}
    assert set(fused) == {"main_loss", "depth_loss", "mono_depth_local_loss"}
    assert model.last["mono_patch_offset"] == (1, 1) and float(model.last["mono_stats"][9]) >= 2
    fused_grads = {k: model.params.g[k].clone() for k in GaussianParams.NAMES}
    leaves = [getattr(model.params, k).detach().clone().requires_grad_(True) for k in GaussianParams.NAMES]
    p2 = GaussianParams.from_tensors(*[t.detach() for t in leaves])
    for k, t in zip(GaussianParams.NAMES, leaves):
        setattr(p2, k, t)
    m2 = DepthGaussianSplattingModel(model.config, p2)
    m2.step = 3
    ld = m2.get_loss_dict(m2.get_outputs(view.cam), view)
    assert set(ld) == {"main_loss", "mono_depth_local_loss"}
    sum(ld.values()).backward()
    ld = {k: v.detach() for k, v in ld.items()}
    print(f"[depth_corr_local fused vs autograd] mono_depth_local_loss fused {fused['mono_depth_local_loss']:.8f} "
          f"autograd {float(ld['mono_depth_local_loss']):.8f}  active patches {int(model.last['mono_stats'][9])}")
    assert abs(float(ld["mono_depth_local_loss"]) - fused["mono_depth_local_loss"]) <= 1e-6
    assert 0 < fused["mono_depth_local_loss"] < 0.1
    off, view_off, _ = _model_and_view(dev, 0.0, rendered_rgb=True, ssim_lambda=0.0)
    off.forward_backward(view_off)
    for k, t in zip(GaussianParams.NAMES, leaves):
        scale = fused_grads[k].abs().max().item()
        diff = (t.grad - fused_grads[k]).abs().max().item()
        moved = (off.params.g[k] - fused_grads[k]).abs().max().item()
        print(f"[depth_corr_local fused vs autograd] {k}: max |grad| {scale:.3e}  max |fused - autograd| {diff:.3e} (bound 1e-4 of the "
              f"former)  max |with - without the term| {moved:.3e}")
        assert diff <= 1e-4 * scale, k
        if k not in ("sh", "sh_dc", "sh_rest"):        # (depth and alpha do not depend on colour)
            assert scale > 0 and moved > 1e-3 * scale, k


def test_switching_the_term_off_changes_nothing_and_the_offsets_follow_the_rule(dev):
    runs = {}
    cases = {"defaults": (0.0, False), "local mult 0": (0.0, True), "no map": (0.2, False), "on": (0.2, True)}
    for name, (mult, with_map) in cases.items():
        model, view, _ = _model_and_view(dev, 0.0, with_map, mono_depth_local_mult=mult, **(LOCAL_CFG if name != "defaults" else {}))
        if name == "defaults":
            from touch_gs_amd.model import ModelConfig
            assert model.config == ModelConfig(sh_degree=3, sh_degree_interval=0)
        model.train_step(view)
        model.flush()
        keys = set(model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], view))
        runs[name] = (model.params.flat.clone(), keys, model)
    base, keys, _ = runs["defaults"]
    assert keys == {"main_loss", "depth_loss"}
    for name in ("local mult 0", "no map"):
        assert torch.equal(runs[name][0].view(torch.int32), base.view(torch.int32)), name
        assert runs[name][1] == keys, name
        assert "mono_patch_offset" not in runs[name][2].last and "mono_stats" not in runs[name][2].last
    assert runs["on"][1] == keys | {"mono_depth_local_loss"}
    assert not torch.equal(runs["on"][0], base)
    # consecutive steps: off_x = step % k, off_y = (step // k) % k
    model = runs["on"][2]
    assert model.last["mono_patch_offset"] == (0, 0) and model.step == 1
    _, view, _ = _model_and_view(dev, 0.0, True, mono_depth_local_mult=0.2, **LOCAL_CFG)
    seen = [(0, 0)]
    for _ in range(4):
        model.train_step(view)
        seen.append(model.last["mono_patch_offset"])
    assert seen == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 0)]


def test_the_term_optimises_the_local_correlation(dev):
    """5 000 Gaussians at 160x120, k = 2; mono = an affine map of the target's depth times a smooth distortion; start = the
    target with means and scales perturbed; 60 train_steps with mono_depth_local_mult 0 and 0.2 from the same start.  rho_bar
    (forward-only op, offset (0, 0)) must end above its start with the term on, and above the final value without it."""
    from touch_gs_amd import ops
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_camera, synthetic_gaussians
    N, W, H, deg, k = 5000, 160, 120, 1, 2
    P, intr = synthetic_gaussians(N, W, H, deg, 77)
    cam = make_camera(intr, 0, 8)
    T = {kk: v.to(dev).contiguous() for kk, v in P.items()}
    with torch.no_grad():
        rgb, dacc, alpha, _ = ops.render(T["means"], T["log_scales"], T["quats"], T["opac_logit"], T["sh"], cam, deg)
    distortion = 1 + 0.2 * torch.sin(torch.arange(W, device=dev, dtype=torch.float32) / 40.0)[None, :]
    mono = torch.where(alpha > 0.05, (3.0 * dacc / alpha.clamp(min=1e-10) + 0.7) * distortion, torch.zeros_like(dacc)).contiguous()
    view = View(cam=cam, rgb=rgb.clamp(0, 1).contiguous(), mono_depth=mono)
    g = torch.Generator().manual_seed(3)
    start = dict(P)
    start["means"] = P["means"] + 0.3 * torch.randn(N, 3, generator=g)
    start["log_scales"] = P["log_scales"] + 0.3 * torch.randn(N, 3, generator=g)

    def rho_bar(model):
        with torch.no_grad():
            out = model.get_outputs(cam)
        s, _, _ = ops.depth_corr_local_fwd_bwd(out["depth_acc"], 1 - out["alpha"], mono, 0.5, patch_tiles=k, offset=(0, 0),
                                               want_grad=False)
        assert float(s[9]) >= 4
        return float(s[10])

    final = {}
    for mult in (0.0, 0.2):
        params = GaussianParams.from_tensors(*[start[kk].to(dev) for kk in GaussianParams.NAMES])
        model = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=0, lr_means=2e-3, lr_means_final=None,
                                                        mono_depth_local_mult=mult, mono_depth_patch_tiles=k), params)
        first = rho_bar(model)
        for _ in range(60):
            model.train_step(view)
        model.flush()
        final[mult] = rho_bar(model)
        print(f"[depth_corr_local optimises] local mult {mult}: rho_bar {first:.5f} -> {final[mult]:.5f}")
        assert first < 1 - 1e-4        # (there is something to optimise)
    assert final[0.2] > first
    assert final[0.2] > final[0.0]
