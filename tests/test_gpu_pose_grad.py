"""The camera-pose gradient on the GPU (k_pose_grad / k_pose_grad_final, ops.pose_grad, the model's refinement path and the
gsplat-shaped surface) against tests/pose_ref.py and the fp64 oracle.

Units: error per entry of G in 2^-24 x mass, the mass from the reference.  Bar = 4 x the fp32 floor of the same case
(tests/pose_ref.floor, printed by tests/test_cpu_pose_ref.py::test_floors), never below 4 units.  Every figure is printed
before it is asserted (pytest -s); the floor table and the measured figures are in DESIGN.md section 5.1m.
"""
import dataclasses
import types

import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests import project_cases as PC
from tests.test_gpu_project_oracle import _dev, _front, _partials, _runs

pytestmark = pytest.mark.gpu


def _note(name, key, value, bar):
    print(f"FIG {name:22s} {key:14s} measured {value:10.3f}  bar {bar:10.3f}")


def _call(case, dev, D, cam, sp, gb, **kw):
    """ops.pose_grad into NaN-filled outputs with one sentinel row behind the scratch -> out [32] (numpy fp64)."""
    from touch_gs_amd import _lib, ops
    G = _lib.load().tgs_num_groups(case.N)
    res = torch.full((_lib.POSE_OUT,), float("nan"), dtype=torch.float32, device=dev)
    scratch = torch.full((G + 1, _lib.POSE_ROW), float("nan"), dtype=torch.float32, device=dev)
    got = ops.pose_grad(cam, D["means"], D["log_scales"], D["quats"], D["sh"], case.deg, sp, group_base=gb,
                        out=(res, scratch), **kw)
    assert got is res
    assert torch.isnan(scratch[G]).all(), "k_pose_grad wrote behind its last row"
    return res.cpu().double().numpy(), scratch[:G].cpu().numpy()


def _check(name, label, case, out, v, vis):
    ref = PR.pose_grad(case, v, vis)
    assert not np.isnan(out).any()
    assert out[24] == 1.0 and out[25] == float(vis.sum()) and (out[26:] == 0).all()
    mass = ref["mass"].reshape(-1)
    rel = np.abs(out[12:24] - mass) / np.where(mass > 0, mass, 1.0)
    _note(label, "mass rel", float(rel.max()), 1e-5)
    assert (rel <= 1e-5).all() and (out[12:24][mass == 0] == 0).all()
    e, bar = PR.err_units(out[:12], ref["G"], ref["mass"]), PR.bar(name)
    _note(label, "G units", e, bar)
    assert e <= bar, (label, e, bar)


@pytest.mark.parametrize("name", PR.PIN_NAMES)
def test_pin_v_splats_form(dev, name):
    case = PR.pin_case(name)
    D = _dev(case, dev)
    cam, sp, rad, gb, cap = _front(case, dev, D)
    v = PC.upstream(case)
    vs = torch.full((case.N, 12), float("nan"), dtype=torch.float32)     # slots 10, 11 are not the kernel's to read
    vs[:, :10] = torch.from_numpy(v).float()
    out, _ = _call(case, dev, D, cam, sp, None, v_splats=vs.to(dev))
    vis = sp[:, 4].cpu().numpy() > 0
    assert np.array_equal(vis, rad.cpu().numpy() > 0)
    _check(name, name + "/v_splats", case, out, v, vis)


@pytest.mark.parametrize("name,long_run", [(n, 0) for n in PR.PIN_NAMES] + [("clamp", 4), ("fill", 2)])
def test_pin_partials_form(dev, name, long_run):
    """The upstream as hand-built partial records; long_run > 0: runs beyond that many tiles take the shared path of
    group_sum_partials.  The reference takes the fp32 sums as K8a forms them (pinned on their own by
    tests/test_gpu_project_oracle.py), so what is measured here is the pose kernel's arithmetic."""
    from touch_gs_amd import ops
    case = PR.pin_case(name)
    D = _dev(case, dev)
    cam, sp, rad, gb, cap = _front(case, dev, D, **({"long_run": long_run} if long_run else {}))
    base, hits = _runs(sp, gb, cap)
    if long_run:
        assert (hits > long_run).any(), "no Gaussian exceeds cam.long_run tiles"
    buf, S, A = _partials(base, hits, cap, 9, dev)
    v32 = ops.reduce_partials(cam, sp, gb, buf).cpu().double().numpy()[:, :10]
    out, rows = _call(case, dev, D, cam, sp, gb, partials=buf)
    assert not np.isnan(rows).any()
    _check(name, f"{name}/partials/L{long_run}", case, out, v32, sp[:, 4].cpu().numpy() > 0)


def test_sizes(dev):
    """N = 1, 255, 256, 257 (tail and full groups) and 0."""
    # (the sum of one Gaussian has nothing to average its roundings over: each cut is held to its own floor)
    from touch_gs_amd import ops
    full = PR.pin_case("fill")
    for n in (1, 255, 256, 257):
        case = full.take(np.arange(n), name="fill")
        D = _dev(case, dev)
        cam, sp, rad, gb, cap = _front(case, dev, D)
        v = PC.upstream(case)
        vs = torch.zeros(n, 12, dtype=torch.float32)
        vs[:, :10] = torch.from_numpy(v).float()
        out, _ = _call(case, dev, D, cam, sp, None, v_splats=vs.to(dev))
        vis = sp[:, 4].cpu().numpy() > 0
        ref = PR.pose_grad(case, v, vis)
        assert out[25] == vis.sum()
        # the bar of THIS cut of the case: 4 x its own fp32 floor, never below 4 units
        bar = 4.0 * max(PR.err_units(PR.pose_grad(case, v, vis, np.float32)["G"], ref["G"], ref["mass"]), 1.0)
        e = PR.err_units(out[:12], ref["G"], ref["mass"])
        _note(f"fill[:{n}]", "G units", e, bar)
        assert e <= bar, (n, e, bar)
    e = torch.empty(0, 3, device=dev)
    out = ops.pose_grad(full.amd_cam(), e, e, torch.empty(0, 4, device=dev), None, -1, torch.empty(0, 12, device=dev),
                        v_splats=torch.empty(0, 12, device=dev)).cpu().numpy()
    assert out[24] == 1 and (np.delete(out, 24) == 0).all()


def test_voided_frame(dev):
    """status[1] = 1 (set by hand): the group kernel returns before it reads anything, the result is all zeros with
    out[24] = 0, and the refiner leaves the pose untouched."""
    from touch_gs_amd import ops, pose
    case = PR.pin_case("fill")
    D = _dev(case, dev)
    cam, sp, rad, gb, cap = _front(case, dev, D)
    base, hits = _runs(sp, gb, cap)
    buf, S, A = _partials(base, hits, cap, 9, dev)
    guard = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    out, rows = _call(case, dev, D, cam, sp, gb, partials=buf, guard=guard)
    assert (out == 0).all()
    assert np.isnan(rows).all(), "a voided frame writes no scratch row"
    view = types.SimpleNamespace(cam=cam, set_camera=lambda c: (_ for _ in ()).throw(AssertionError("pose changed")))
    ref = pose.PoseRefiner([view], 1e-3, 1e-3)
    assert ref.apply(view, out) is False and view.cam is cam
    live, _ = _call(case, dev, D, cam, sp, gb, partials=buf, guard=torch.zeros(2, dtype=torch.int32, device=dev))
    assert live[24] == 1 and (live[:12] != 0).all()


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def _model(dev, N, W, H, deg, seed, lrs=None, **cfgkw):
    from touch_gs_amd import Camera
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig, View
    from touch_gs_amd.optim import GaussianParams
    P, c, V = PR.tiny_scene(N, W, H, deg, seed)
    params = GaussianParams.from_tensors(*[P[k].float().to(dev) for k in GaussianParams.NAMES])
    cfg = ModelConfig(sh_degree=deg, sh_degree_interval=0, lr_means_final=None, **PR.LOSS_KW, **(lrs or {}), **cfgkw)
    model = DepthGaussianSplattingModel(cfg, params)
    cam = Camera(V, c["fx"], c["fy"], c["cx"], c["cy"], W, H, bg=(0.1, 0.2, 0.3))
    return model, P, c, V, cam, View


def _random_supervision(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(H, W, 3, generator=g, dtype=torch.float64).float().double()
    dgt = (torch.rand(H, W, generator=g, dtype=torch.float64) * 5).float().double()
    dgt[torch.rand(H, W, generator=g) < 0.3] = 0
    unc = (torch.rand(H, W, generator=g, dtype=torch.float64) * 5 + 1e-3).float().double()
    return gt, dgt, unc


def test_end_to_end_against_the_oracle(dev):
    """64 x 48, 300 Gaussians, SH 3, L1 + SSIM + uncertainty-weighted depth: last["pose_grad"] of a train step with
    refinement on against d train_loss / d viewmat of the fp64 oracle.  Floor: the oracle chain in fp32 on the CPU."""
    N, W, H, deg = 300, 64, 48, 3
    model, P, c, V, cam, View = _model(dev, N, W, H, deg, 7, pose_lr_rot=1e-3, pose_lr_trans=1e-3)
    gt, dgt, unc = _random_supervision(H, W)
    view = View(cam=cam, rgb=gt.float().to(dev), depth=dgt.float().to(dev), uncertainty=unc.float().to(dev))
    assert model.enable_pose_refinement([view]) is not None
    model.train_step(view)
    out = model.last["pose_grad"].cpu().double().numpy()
    assert out[24] == 1 and out[25] > 0
    _, G64 = PR.oracle_pose_grad(P, c, V, deg, gt, dgt, unc, torch.float64)
    _, G32 = PR.oracle_pose_grad(P, c, V, deg, gt, dgt, unc, torch.float32)
    mass = out[12:24]
    floor = PR.err_units(G32, G64, mass)
    e, bar = PR.err_units(out[:12], G64, mass), 4.0 * max(floor, 1.0)
    _note("end-to-end", "floor (fp32)", floor, bar)
    _note("end-to-end", "G units", e, bar)
    assert e <= bar, (e, bar)


@pytest.mark.parametrize("form", ["fused", "unfused", "densify"])
def test_refinement_only_reads(dev, form, monkeypatch):
    """One train_step with and one without refinement from the same state and view: parameters, both Adam moments and
    last["rgb"] bit-identical (the pose update waits for the view's next use); off: no "pose_grad", no launch."""
    from touch_gs_amd import ops
    N, W, H, deg = 300, 64, 48, 3
    gt, dgt, unc = _random_supervision(H, W)
    res = {}
    for on in (True, False):
        kw = dict(pose_lr_rot=1e-3, pose_lr_trans=1e-3) if on else {}
        model, P, c, V, cam, View = _model(dev, N, W, H, deg, 7, **kw)
        view = View(cam=cam, rgb=gt.float().to(dev), depth=dgt.float().to(dev), uncertainty=unc.float().to(dev))
        if form == "unfused":
            model.fuse_adam = False
        if form == "densify":
            model.enable_densification()
        if on:
            model.enable_pose_refinement([view])
        else:
            assert model.enable_pose_refinement([view]) is None
            monkeypatch.setattr(ops, "pose_grad", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
        model.train_step(view)
        torch.cuda.synchronize()
        assert ("pose_grad" in model.last) == on
        assert view.cam is cam, "the pose update is applied at the view's next use, not in the step"
        res[on] = [model.params.flat.clone(), model.optimizer.exp_avg.clone(), model.optimizer.exp_avg_sq.clone(),
                   model.last["rgb"].clone()]
        if on:
            out = model.last["pose_grad"].cpu().numpy()
            assert out[24] == 1 and np.abs(out[:12]).max() > 0
            model.flush()
            assert view.cam is not cam and not np.array_equal(view.cam.viewmat, cam.viewmat)
            assert len(model._tuned_cams) <= 1
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_recovery(dev):
    """A frozen model supervised by its own renders from the true pose; one view perturbed (PR.RECOVER), pose-only steps.
    The reference is the same loop driven by the fp64 oracle's gradient (tests/test_cpu_pose_ref.py checks that IT ends
    below one fifth of both initial errors).  The GPU run must do the same and stay near the reference trajectory."""
    k = PR.RECOVER
    zero = dict(lr_means=0.0, lr_scales=0.0, lr_quats=0.0, lr_opac=0.0, lr_sh_dc=0.0, lr_sh_rest=0.0)
    model, P, c, V, cam, View = _model(dev, k["N"], k["W"], k["H"], k["deg"], k["seed"], lrs=zero,
                                       pose_lr_rot=k["lr_rot"], pose_lr_trans=k["lr_trans"])
    gt, dgt, unc = PR.supervision_from(P, c, V, k["deg"])
    V1 = PR.perturbed(V, k["rot_deg"], k["axis"], k["trans"])
    ref = PR.recovery_loop(lambda X: PR.oracle_pose_grad(P, c, X.astype(np.float32).astype(np.float64), k["deg"], gt, dgt, unc)[1],
                           V1, k["lr_rot"], k["lr_trans"], k["steps"])
    view = View(cam=dataclasses.replace(cam, viewmat=V1), rgb=gt.float().to(dev), depth=dgt.float().to(dev),
                uncertainty=unc.float().to(dev))
    model.enable_pose_refinement([view])
    before = model.params.flat.clone()
    traj = [np.array(view.cam.viewmat)]
    for _ in range(k["steps"]):
        model.train_step(view)
        model.flush()
        traj.append(np.array(view.cam.viewmat))
    assert torch.equal(before, model.params.flat), "the model is frozen"
    err = lambda X: PR.pose_error(X[:3, :3], X[:3, 3], V[:3, :3], V[:3, 3])
    (r0, t0), (r1, t1), (rr, tr) = err(traj[0]), err(traj[-1]), err(ref[-1])
    print(f"FIG recovery: start {r0:.4f} deg {t0:.5f}; reference ends {rr:.4f} deg {tr:.5f}; GPU ends {r1:.4f} deg {t1:.5f}")
    assert rr <= r0 / 5 and tr <= t0 / 5
    assert r1 <= r0 / 5 and t1 <= t0 / 5
    gap = max(max(PR.pose_error(a[:3, :3], a[:3, 3], b[:3, :3], b[:3, 3])[0] / r0 for a, b in zip(traj, ref)),
              max(PR.pose_error(a[:3, :3], a[:3, 3], b[:3, :3], b[:3, 3])[1] / t0 for a, b in zip(traj, ref)))
    print(f"FIG recovery: largest gap to the reference trajectory {gap:.3e} of the initial error, bar {PR.RECOVER_GAP_BAR:.3e}")
    assert gap <= PR.RECOVER_GAP_BAR


def _loop(dev, announce, steps=6, nv=3):
    """`steps` train steps over `nv` views under the resolution schedule (downscale 2 for two steps, then full size)."""
    N, W, H, deg = 300, 64, 48, 3
    model, P, c, V, cam, View = _model(dev, N, W, H, deg, 7, pose_lr_rot=1e-3, pose_lr_trans=1e-3, num_downscales=1,
                                       resolution_schedule=2)
    views = []
    for i in range(nv):
        gt, dgt, unc = _random_supervision(H, W, seed=i)
        Vi = PR.perturbed(V, 2.0 * i, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
        views.append(View(cam=dataclasses.replace(cam, viewmat=Vi), rgb=gt.float().to(dev), depth=dgt.float().to(dev),
                          uncertainty=unc.float().to(dev)))
    from touch_gs_amd.model import Tuning
    model.tuning = Tuning(long_run=8)     # not the cameras' own: model.tuned() memoises a copy per camera object
    model.enable_pose_refinement(views)
    for i in range(steps):
        model.train_step(views[i % nv], next_view=views[(i + 1) % nv] if announce else None)
        # the memo holds live cameras only: per view at most its current one at each cached resolution
        live = {id(v.cam) for v in views} | {id(dv.cam) for v in views for dv in v.__dict__.get("_downscaled", {}).values()}
        assert set(model._tuned_cams) <= live, "a replaced camera stayed in model._tuned_cams"
        for v in views:     # never a stale camera under a cached downscaled form
            for d, dv in v.__dict__.get("_downscaled", {}).items():
                assert np.array_equal(dv.cam.viewmat, v.cam.viewmat) and dv.cam.W == v.cam.W // d
    model.flush()
    return model, views


def test_training_loop_schedule_prefetch_and_state(dev):
    """Refinement through the resolution schedule, with and without the announced next view (colour / front prefetch): the
    same poses and parameters bit for bit -- pending updates land before the next camera is armed --, a bounded camera
    memo, and a state_dict that carries the refiner's state only when there is one."""
    m1, v1 = _loop(dev, True)
    m2, v2 = _loop(dev, False)
    assert torch.equal(m1.params.flat, m2.params.flat)
    for a, b in zip(v1, v2):
        assert np.array_equal(a.cam.viewmat, b.cam.viewmat)
    deltas = m1.pose_refiner.deltas()
    assert all(a > 0 and b > 0 for a, b in deltas)
    met = m1.get_metrics_dict(dict(rgb=m1.last["rgb"], depth=m1.last["depth_acc"][..., None]), m1.last["view"])
    assert float(met["pose_delta_deg"]) > 0 and float(met["pose_delta_m"]) > 0
    assert len(m1._tuned_cams) <= len(v1) and len(m2._tuned_cams) <= len(v2)
    sd = m1.state_dict()
    assert set(sd["pose"]) == {"V0", "V", "m", "v", "t"} and sd["pose"]["t"].tolist() == [2, 2, 2]
    want = [np.array(v.cam.viewmat) for v in v1]
    for v in v1:
        m1.pose_refiner.set_pose(v, np.eye(4), m1)
    m1.load_state_dict(sd)
    assert all(np.array_equal(v.cam.viewmat, w) for v, w in zip(v1, want))
    plain, *_ = _model(dev, 64, 32, 32, 3, 7)
    assert "pose" not in plain.state_dict() and "pose_delta_deg" not in plain.get_metrics_dict(
        dict(rgb=torch.zeros(32, 32, 3, device=dev)), types.SimpleNamespace(rgb=torch.zeros(32, 32, 3, device=dev), depth=None))


# ---------------------------------------------------------------------------------------------
# gsplat-shaped surface, refusals
# ---------------------------------------------------------------------------------------------
def test_project_gaussians_viewmat_gradient(dev, monkeypatch):
    from touch_gs_amd import ops
    case = PR.pin_case("nosh")
    D = _dev(case, dev)
    c = case.cam
    v = PC.upstream(case)
    vt = torch.from_numpy(v).float().to(dev)

    def run(req):
        means, scales, quats = (t.clone().requires_grad_(True) for t in (D["means"], torch.exp(D["log_scales"]), D["quats"]))
        V = torch.from_numpy(c.viewmat.numpy()).float().to(dev).requires_grad_(req)
        xys, depths, radii, conics, *_ = ops.project_gaussians(means, scales, 1.0, quats, V, c.fx, c.fy, c.cx, c.cy, c.H, c.W,
                                                               clip_thresh=c.near)
        ((xys * vt[:, 0:2]).sum() + (depths * vt[:, 2]).sum() + (conics * vt[:, 4:7]).sum()).backward()
        return [xys.detach(), depths.detach(), radii, conics.detach(), means.grad, scales.grad, quats.grad], V.grad

    with_grad, gV = run(True)
    assert gV.shape == (4, 4) and (gV[3] == 0).all()
    cam = case.amd_cam()
    ls = torch.log(torch.exp(D["log_scales"]))     # the surface takes post-exp scales: these are the log-scales it forms
    sp, _ = ops.project_fwd(cam, D["means"], ls, D["quats"], torch.zeros(case.N, device=dev), None, -1, want_radii=True)
    vs = torch.zeros(case.N, 12, dtype=torch.float32, device=dev)
    vs[:, 0:3], vs[:, 4:7] = vt[:, 0:3], vt[:, 4:7]
    direct = ops.pose_grad(cam, D["means"], ls, D["quats"], None, -1, sp, v_splats=vs)
    assert torch.equal(gV[:3].reshape(-1), direct[:12])
    v0 = v.copy()
    v0[:, 3], v0[:, 7:] = 0, 0
    case = dataclasses.replace(case, P={**case.P, "log_scales": ls.cpu().double().numpy()})
    ref = PR.pose_grad(case, v0, sp[:, 4].cpu().numpy() > 0)
    assert PR.err_units(gV[:3].cpu().double().numpy(), ref["G"], ref["mass"]) <= PR.bar("nosh")
    monkeypatch.setattr(ops, "pose_grad", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    without, none = run(False)
    assert none is None
    for a, b in zip(with_grad, without):
        assert torch.equal(a, b)


def test_rates_without_registered_views_are_refused(dev):
    model, P, c, V, cam, View = _model(dev, 64, 32, 32, 3, 7, pose_lr_trans=1e-3)
    gt, dgt, unc = _random_supervision(32, 32)
    view = View(cam=cam, rgb=gt.float().to(dev), depth=dgt.float().to(dev), uncertainty=unc.float().to(dev))
    with pytest.raises(ValueError, match="enable_pose_refinement"):
        model.train_step(view)


def test_refusals(dev):
    N, W, H, deg = 64, 32, 32, 3
    model, P, c, V, cam, View = _model(dev, N, W, H, deg, 7, pose_lr_rot=1e-3)
    gt, dgt, unc = _random_supervision(H, W)
    view = View(cam=cam, rgb=gt.float().to(dev), depth=dgt.float().to(dev), uncertainty=unc.float().to(dev))
    model.enable_pose_refinement([view])
    with pytest.raises(ValueError, match="capture_step_graphs"):
        model.capture_step_graphs([view])
    with pytest.raises(ValueError, match="data-parallel"):
        model.train_step(view, dp=types.SimpleNamespace(active=True))
