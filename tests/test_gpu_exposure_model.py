"""Exposure compensation through the model (ModelConfig.exposure_*, enable_exposure, train_step, loss_from, get_outputs,
state_dict): a three-view scene of 300 Gaussians at 64 x 48.  The kernels themselves are held to the reference by
tests/test_gpu_exposure.py."""
import dataclasses
import types

import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests.test_gpu_pose_grad import _model, _random_supervision

pytestmark = pytest.mark.gpu

N, W, H, DEG = 300, 64, 48, 3


def _scene(dev, nv=3, **cfgkw):
    model, P, c, V, cam, View = _model(dev, N, W, H, DEG, 7, **cfgkw)
    views = []
    for i in range(nv):
        gt, dgt, unc = _random_supervision(H, W, seed=i)
        Vi = PR.perturbed(V, 2.0 * i, (0.0, 1.0, 0.0), (0.0, 0.0, 0.0))
        views.append(View(cam=dataclasses.replace(cam, viewmat=Vi), rgb=gt.float().to(dev), depth=dgt.float().to(dev),
                          uncertainty=unc.float().to(dev)))
    return model, views


def _bits(t):
    return t.detach().clone().view(torch.int32)


def test_two_steps_rows_loss_and_state(dev):
    from touch_gs_amd import ops
    model, views = _scene(dev, exposure_lr=1e-2)
    es = model.enable_exposure(views)
    assert es is not None and es.state.shape == (3, 48) and all(es.owns(v) for v in views)
    init = es.state.clone()
    assert np.array_equal(es.matrix(views[1]), np.eye(3, 4, dtype=np.float32))
    for i in (0, 1):
        before = es.row(views[i]).clone()
        model.train_step(views[i])
        out = model.last["exposure"]
        assert float(out[24]) == 1 and float(out[26]) == W * H
        # main_loss against a torch recomputation from last["rgb"], the row BEFORE the step and the view
        lam = model.config.ssim_lambda
        E = before[:12].view(3, 4).double()
        cp = model.last["rgb"].double() @ E[:, :3].T + E[:, 3]
        ssim_sum, _ = ops.ssim_fwd_bwd(cp.float().contiguous(), views[i].rgb, want_grad=False)
        want = (1 - lam) * float((cp - views[i].rgb.double()).abs().mean()) + lam * (1 - float(ssim_sum) / (3 * H * W))
        got = model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], views[i])
        print(f"FIG model step {i}: main_loss fused {float(got['main_loss']):.8f}  torch {want:.8f}")
        assert float(model.last["tile_loss"][:, 0].abs().sum()) == 0, "K7's own L1 column is off under compensation"
        assert abs(float(got["main_loss"]) - want) < 1e-4 * abs(want)
    assert float(es.state[0, 36]) == 1 and float(es.state[1, 36]) == 1
    assert not torch.equal(es.state[0, :12], init[0, :12]) and not torch.equal(es.state[1, :12], init[1, :12])
    assert torch.equal(_bits(es.state[2]), _bits(init[2])), "a view that was not stepped keeps its row bit for bit"
    met = model.get_metrics_dict(dict(rgb=model.last["rgb"], depth=model.last["depth_acc"][..., None]), views[1])
    assert abs(float(met["exposure_gain"]) - 1) < 0.05 and abs(float(met["exposure_offset"])) < 0.05
    # compensated render of an owned view; the default call and a view without a row are unchanged
    raw = model.get_outputs(views[0].cam)["rgb"]
    comp = model.get_outputs(views[0].cam, exposure_of=views[0])
    assert torch.equal(comp["rgb_raw"], raw) and not torch.equal(comp["rgb"], raw)
    assert torch.equal(comp["rgb"], ops.exposure_fwd(raw, es.row(views[0])))
    stranger = types.SimpleNamespace(cam=views[0].cam)
    assert torch.equal(model.get_outputs(views[0].cam, exposure_of=stranger)["rgb"], raw)


def test_state_dict_round_trip_reproduces_the_third_step(dev):
    def run(reload):
        model, views = _scene(dev, exposure_lr=1e-2)
        model.enable_exposure(views)
        model.train_step(views[0])
        model.train_step(views[1])
        if reload:
            sd = model.state_dict()
            assert set(sd["exposure"]) == {"state"} and sd["exposure"]["state"].shape == (3, 48)
            other, views = _scene(dev, exposure_lr=1e-2)
            other.enable_exposure(views)
            other.load_state_dict(sd)
            model = other
        model.train_step(views[0])
        torch.cuda.synchronize()
        return model.params.flat.clone(), model.exposure_set.state.clone()

    (pa, ea), (pb, eb) = run(False), run(True)
    assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ea), _bits(eb))
    assert float(ea[0, 36]) == 2 and float(ea[1, 36]) == 1


def test_downscaled_view_steps_its_parents_row(dev):
    model, views = _scene(dev, exposure_lr=1e-2, num_downscales=1, resolution_schedule=2)
    es = model.enable_exposure(views)
    init = es.state.clone()
    assert model.config.downscale_factor(0) == 2
    model.train_step(views[1])
    assert model.last["view"] is not views[1] and model.last["view"].cam.W == W // 2
    assert float(model.last["exposure"][26]) == (W // 2) * (H // 2)
    assert float(es.state[1, 36]) == 1 and not torch.equal(es.state[1, :12], init[1, :12])
    assert torch.equal(_bits(es.state[0]), _bits(init[0])) and torch.equal(_bits(es.state[2]), _bits(init[2]))


def test_off_is_bit_identical_and_absent(dev, monkeypatch):
    from touch_gs_amd import ops
    res = []
    for kw in (dict(), dict(exposure_lr=0.0, exposure_l2=0.5, exposure_start_step=3)):
        model, views = _scene(dev, **kw)
        if kw:
            assert model.enable_exposure(views) is None
            for name in ("exposure_fwd", "exposure_bwd"):
                monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
        model.train_step(views[0])
        model.train_step(views[1])
        torch.cuda.synchronize()
        assert "exposure" not in model.state_dict() and "exposure" not in model.last
        assert "exposure_gain" not in model.get_metrics_dict(
            dict(rgb=model.last["rgb"], depth=model.last["depth_acc"][..., None]), views[1])
        res.append([model.params.flat.clone(), model.optimizer.exp_avg.clone(), model.optimizer.exp_avg_sq.clone()])
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


def test_start_step_issues_nothing_before(dev, monkeypatch):
    from touch_gs_amd import ops
    model, views = _scene(dev, exposure_lr=1e-2, exposure_start_step=5)
    es = model.enable_exposure(views)
    init = es.state.clone()
    real = (ops.exposure_fwd, ops.exposure_bwd)
    for name in ("exposure_fwd", "exposure_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched before the start step")))
    for i in range(5):
        model.train_step(views[i % 3])
        assert "exposure" not in model.last
    assert torch.equal(_bits(es.state), _bits(init))
    monkeypatch.setattr(ops, "exposure_fwd", real[0])
    monkeypatch.setattr(ops, "exposure_bwd", real[1])
    model.train_step(views[2])
    assert model.step == 6 and float(es.state[2, 36]) == 1 and float(es.state[0, 36]) == 0


def test_refusals(dev):
    model, views = _scene(dev, nv=1, exposure_lr=1e-2)
    with pytest.raises(ValueError, match="exposure_lr.*enable_exposure"):      # a rate set without registered views
        model.train_step(views[0])
    model.enable_exposure(views)
    with pytest.raises(ValueError, match="exposure_lr"):
        model.capture_step_graphs(views)
    with pytest.raises(ValueError, match="exposure_lr"):
        model.train_step(views[0], dp=types.SimpleNamespace(active=True))


def test_autograd_path_takes_the_loss_on_the_compensated_image(dev):
    """get_loss_dict of an owned view goes through ops.apply_exposure: with E off the identity the loss is that of the
    compensated image, and E receives a gradient."""
    model, views = _scene(dev, nv=1, exposure_lr=1e-2)
    es = model.enable_exposure(views)
    es.state[0, 0], es.state[0, 3] = 1.2, 0.05
    out = model.get_outputs(views[0].cam)
    ld = model.get_loss_dict(out, views[0])
    E = es.row(views[0])[:12].view(3, 4).double()
    cp = out["rgb"].detach().double() @ E[:, :3].T + E[:, 3]
    l1 = float((cp - views[0].rgb.double()).abs().mean())
    plain = float((out["rgb"].detach().double() - views[0].rgb.double()).abs().mean())
    assert abs(l1 - plain) > 1e-3
    lam = model.config.ssim_lambda
    from touch_gs_amd import ops
    ssim_sum, _ = ops.ssim_fwd_bwd(cp.float().contiguous(), views[0].rgb, want_grad=False)
    want = (1 - lam) * l1 + lam * (1 - float(ssim_sum) / (3 * H * W))
    assert abs(float(ld["main_loss"]) - want) < 1e-4 * want
    ld["main_loss"].backward()
    assert out["exposure"].grad is not None and out["exposure"].grad.abs().max() > 0


def test_trainer_flags_config_and_exposures_json(dev, tmp_path):
    """touch_gs_amd.train with --exposure-lr: the flags are recorded in config.json (and are 0 / off by default), every
    training view gets a row that steps from the start step on, and the save writes exposures.json."""
    import json
    import os
    from touch_gs_amd import train
    from touch_gs_amd.exposure import EXPOSURES_FILE
    base = ["--synthetic", "2000", "64", "48", "--max-num-iterations", "16", "--steps-per-save", "16", "--steps-per-eval", "16"]
    run = train.main(base + ["--exposure-lr", "0.01", "--exposure-l2", "0.001", "--exposure-start-step", "2",
                             "--output-dir", str(tmp_path / "on")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["exposure_lr"] == 0.01 and cfg["exposure_start_step"] == 2
    assert cfg["model"]["exposure_lr"] == 0.01 and cfg["model"]["exposure_l2"] == 0.001
    rows = json.load(open(os.path.join(run, EXPOSURES_FILE)))
    # 7 training views; steps 2 ... 15 compensate: 14 row steps (a frame of step 0 or 1 that overflowed its intersection buffer
    # and is replayed after the start step would add one each)
    assert len(rows) == 7 and 14 <= sum(r["steps"] for r in rows.values()) <= 16
    assert all(np.asarray(r["E"]).shape == (3, 4) for r in rows.values())
    assert any(not np.array_equal(np.asarray(r["E"]), np.eye(3, 4)) for r in rows.values())
    run = train.main(base + ["--output-dir", str(tmp_path / "off")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["exposure_lr"] == 0.0 and cfg["model"]["exposure_lr"] == 0.0
    assert not os.path.exists(os.path.join(run, EXPOSURES_FILE))
