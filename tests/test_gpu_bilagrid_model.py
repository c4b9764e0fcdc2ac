"""Bilateral grids through the model (ModelConfig.bilagrid_*, enable_bilagrid, train_step, loss_from, get_outputs, state_dict),
the trainer's flags and the colour-corrected evaluation: a three-view scene of 300 Gaussians at 64 x 48.  The kernels
themselves are held to the reference by tests/test_gpu_bilagrid.py."""
import dataclasses
import types

import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests.test_gpu_pose_grad import _model, _random_supervision

pytestmark = pytest.mark.gpu

N, W, H, DEG = 300, 64, 48, 3
SHAPE = (5, 3, 4)
NG = 3 * 5 * 4 * 12


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


def _tv(g):
    return sum(((g.narrow(a, 1, g.shape[a] - 1) - g.narrow(a, 0, g.shape[a] - 1)) ** 2).mean() for a in (0, 1, 2))


def test_start_step_beyond_the_run_is_bit_identical_to_off(dev, monkeypatch):
    from touch_gs_amd import ops
    res = []
    for kw in (dict(), dict(bilagrid_lr=2e-3, bilagrid_shape=SHAPE, bilagrid_start_step=100)):
        model, views = _scene(dev, **kw)
        if kw:
            bs = model.enable_bilagrid(views)
            init = bs.state.clone()
            for name in ("bilagrid_fwd", "bilagrid_bwd"):
                monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched before the start step")))
        else:
            assert model.enable_bilagrid(views) is None and model.bilagrid_set is None
        for i in (0, 1, 2):
            model.train_step(views[i])
        torch.cuda.synchronize()
        assert "bilagrid" not in model.last
        if kw:
            assert torch.equal(_bits(bs.state), _bits(init))
        else:
            assert "bilagrid" not in model.state_dict()
            assert "bilagrid_tv" not in model.get_metrics_dict(dict(rgb=model.last["rgb"], depth=model.last["depth_acc"][..., None]), views[1])
        res.append([model.params.flat.clone(), model.optimizer.exp_avg.clone(), model.optimizer.exp_avg_sq.clone()])
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))


def test_two_steps_rows_loss_and_state(dev):
    from touch_gs_amd import ops
    model, views = _scene(dev, bilagrid_lr=2e-3, bilagrid_shape=SHAPE, bilagrid_tv=10.0)
    bs = model.enable_bilagrid(views)
    assert bs is not None and bs.state.shape == (3, 3 * NG + 16) and all(bs.owns(v) for v in views)
    bs.state[:, :NG] += 0.05 * torch.randn(3, NG, device=dev)      # off the identity: the TV term and the guide term are live
    init = bs.state.clone()
    lam = model.config.ssim_lambda
    for i in (0, 1):
        before = bs.row(views[i]).clone()
        model.train_step(views[i])
        out = model.last["bilagrid"]
        assert float(out[0]) == 1 and float(out[2]) == W * H
        # the losses against a torch recomputation from last["rgb"], the row BEFORE the step and the view
        g = before[:NG].view(3, 5, 4, 12)
        cp = ops.apply_bilagrid(model.last["rgb"], g)
        ssim_sum, _ = ops.ssim_fwd_bwd(cp.contiguous(), views[i].rgb, want_grad=False)
        want = (1 - lam) * float((cp.double() - views[i].rgb.double()).abs().mean()) + lam * (1 - float(ssim_sum) / (3 * H * W))
        want_tv = 10.0 * float(_tv(g.double()))
        got = model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], views[i])
        print(f"FIG model step {i}: main_loss fused {float(got['main_loss']):.8f}  torch {want:.8f}; "
              f"tv loss fused {float(got['bilagrid_tv_loss']):.8f}  torch {want_tv:.8f}")
        assert float(model.last["tile_loss"][:, 0].abs().sum()) == 0, "K7's own L1 column is off under the grid"
        assert abs(float(got["main_loss"]) - want) < 1e-4 * abs(want)
        assert abs(float(got["bilagrid_tv_loss"]) - want_tv) < 1e-4 * want_tv
    assert float(bs.state[0, 3 * NG]) == 1 and float(bs.state[1, 3 * NG]) == 1
    assert not torch.equal(bs.state[0, :NG], init[0, :NG]) and not torch.equal(bs.state[1, :NG], init[1, :NG])
    assert torch.equal(_bits(bs.state[2]), _bits(init[2])), "a view that was not rendered keeps its row bit for bit"
    # the first step's rate is the schedule's: 1 % of the peak, so no entry moved by more than it
    assert float((bs.state[0, :NG] - init[0, :NG]).abs().max()) <= 1.01 * bs.lr_at(0)
    met = model.get_metrics_dict(dict(rgb=model.last["rgb"], depth=model.last["depth_acc"][..., None]), views[1])
    assert float(met["bilagrid_tv"]) > 0 and 0 < float(met["bilagrid_delta"]) < 0.1
    # corrected render of an owned view; the default call and a view without a row are unchanged
    raw = model.get_outputs(views[0].cam)["rgb"]
    comp = model.get_outputs(views[0].cam, bilagrid_of=views[0])
    assert torch.equal(comp["rgb_raw"], raw) and not torch.equal(comp["rgb"], raw)
    assert torch.equal(comp["rgb"], ops.bilagrid_fwd(raw, bs.row(views[0]), SHAPE))
    stranger = types.SimpleNamespace(cam=views[0].cam)
    assert torch.equal(model.get_outputs(views[0].cam, bilagrid_of=stranger)["rgb"], raw)


def test_state_dict_round_trip_reproduces_the_third_step(dev):
    def run(reload):
        model, views = _scene(dev, bilagrid_lr=2e-3, bilagrid_shape=SHAPE)
        model.enable_bilagrid(views)
        model.train_step(views[0])
        model.train_step(views[1])
        if reload:
            sd = model.state_dict()
            assert sd["bilagrid"]["state"].shape == (3, 3 * NG + 16) and tuple(sd["bilagrid"]["shape"]) == SHAPE
            other, views = _scene(dev, bilagrid_lr=2e-3, bilagrid_shape=SHAPE)
            other.enable_bilagrid(views)
            other.load_state_dict(sd)
            plain, _ = _scene(dev)
            plain.load_state_dict(sd)       # a model without a set ignores the key
            assert plain.bilagrid_set is None
            model = other
        model.train_step(views[0])
        torch.cuda.synchronize()
        return model.params.flat.clone(), model.bilagrid_set.state.clone()

    (pa, ga), (pb, gb) = run(False), run(True)
    assert torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(ga), _bits(gb))
    assert float(ga[0, 3 * NG]) == 2 and float(ga[1, 3 * NG]) == 1


def test_downscaled_view_steps_its_parents_row(dev):
    model, views = _scene(dev, bilagrid_lr=2e-3, bilagrid_shape=SHAPE, num_downscales=1, resolution_schedule=2)
    bs = model.enable_bilagrid(views)
    init = bs.state.clone()
    assert model.config.downscale_factor(0) == 2
    model.train_step(views[1])
    assert model.last["view"] is not views[1] and model.last["view"].cam.W == W // 2
    assert float(model.last["bilagrid"][2]) == (W // 2) * (H // 2)
    assert float(bs.state[1, 3 * NG]) == 1 and not torch.equal(bs.state[1, :NG], init[1, :NG])
    assert torch.equal(_bits(bs.state[0]), _bits(init[0])) and torch.equal(_bits(bs.state[2]), _bits(init[2]))


def test_refusals(dev):
    model, views = _scene(dev, nv=1, bilagrid_lr=2e-3, bilagrid_shape=SHAPE)
    with pytest.raises(ValueError, match="bilagrid_lr.*enable_bilagrid"):      # a rate set without registered views
        model.train_step(views[0])
    model.enable_bilagrid(views)
    with pytest.raises(ValueError, match="bilagrid_lr"):
        model.capture_step_graphs(views)
    with pytest.raises(ValueError, match="bilagrid_lr"):
        model.train_step(views[0], dp=types.SimpleNamespace(active=True))
    both, views = _scene(dev, nv=1, bilagrid_lr=2e-3, exposure_lr=1e-2)
    with pytest.raises(ValueError, match="bilagrid_lr.*exposure_lr"):
        both.enable_bilagrid(views)
    with pytest.raises(ValueError, match="exposure_lr.*bilagrid_lr"):
        both.enable_exposure(views)


def test_autograd_path_takes_the_loss_on_the_corrected_image(dev):
    model, views = _scene(dev, nv=1, bilagrid_lr=2e-3, bilagrid_shape=SHAPE)
    bs = model.enable_bilagrid(views)
    bs.state[0, :NG] += 0.1 * torch.randn(NG, device=dev)
    out = model.get_outputs(views[0].cam)
    ld = model.get_loss_dict(out, views[0])
    assert "bilagrid_tv_loss" in ld and float(ld["bilagrid_tv_loss"].detach()) > 0
    (ld["main_loss"] + ld["bilagrid_tv_loss"]).backward()
    assert out["bilagrid"].grad is not None and out["bilagrid"].grad.abs().max() > 0


def test_trainer_flags_files_and_color_corrected_eval(dev, tmp_path):
    """touch_gs_amd.train with --bilagrid-lr: the flags are recorded in config.json (and are 0 / off by default), every
    training view gets a grid that steps, the save writes bilagrids.npz in gsplat's axis order, and run_eval's
    --color-correct adds cc_psnr / cc_ssim and changes no other key."""
    import json
    import os
    from touch_gs_amd import run_eval, train
    from touch_gs_amd.bilagrid import BILAGRIDS_FILE, load_bilagrids
    base = ["--synthetic", "2000", "64", "48", "--max-num-iterations", "16", "--steps-per-save", "16", "--steps-per-eval", "16"]
    run = train.main(base + ["--bilagrid-lr", "0.002", "--bilagrid-shape", "5", "3", "4", "--bilagrid-start-step", "2",
                             "--output-dir", str(tmp_path / "on")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["bilagrid_lr"] == 0.002 and cfg["bilagrid_start_step"] == 2 and cfg["model"]["bilagrid_shape"] == [5, 3, 4]
    assert cfg["model"]["bilagrid_lr"] == 0.002 and cfg["model"]["bilagrid_tv"] == 10.0
    with np.load(os.path.join(run, BILAGRIDS_FILE)) as z:
        assert len(z.files) == 7 and all(z[k].shape == (12, 4, 3, 5) for k in z.files)
    grids = load_bilagrids(os.path.join(run, BILAGRIDS_FILE))
    ident = np.zeros(12, np.float32)
    ident[[0, 5, 10]] = 1
    assert all(g.shape == (3, 5, 4, 12) for g in grids.values()) and any(np.abs(g - ident).max() > 0 for g in grids.values())
    plain = run_eval.eval_run(run, str(tmp_path / "plain.json"))
    cc = run_eval.eval_run(run, str(tmp_path / "cc.json"), color_correct=True)
    assert set(cc) == set(plain) | {"cc_psnr", "cc_ssim"}
    assert all(cc[k] == pytest.approx(plain[k], rel=1e-6, nan_ok=True) for k in plain)
    print(f"FIG eval: psnr {plain['psnr']:.3f}  cc_psnr {cc['cc_psnr']:.3f}  ssim {plain['ssim']:.4f}  cc_ssim {cc['cc_ssim']:.4f}")
    assert cc["cc_psnr"] >= plain["psnr"] - 1e-3, "the least-squares fit contains the identity"
    run = train.main(base + ["--output-dir", str(tmp_path / "off")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["bilagrid_lr"] == 0.0 and cfg["model"]["bilagrid_lr"] == 0.0
    assert not os.path.exists(os.path.join(run, BILAGRIDS_FILE))
