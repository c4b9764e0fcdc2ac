"""The MCMC strategy through the model and the trainer (ModelConfig.opacity_reg / scale_reg / mcmc_noise_lr, enable_mcmc,
train_step, state_dict, touch_gs_amd.train --strategy mcmc): a three-view scene of 300 Gaussians at 64 x 48.  The kernels
themselves are held to their references by tests/test_gpu_mcmc.py."""
import dataclasses
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import pose_ref as PR
from tests.test_gpu_pose_grad import _model, _random_supervision

pytestmark = pytest.mark.gpu

N, W, H, DEG = 300, 64, 48, 3
OFF = dict(opacity_reg=0.0, scale_reg=0.0, noise_lr=0.0)


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


def _state(model):
    torch.cuda.synchronize()
    return [model.params.flat.clone(), model.optimizer.exp_avg.clone(), model.optimizer.exp_avg_sq.clone()]


def _mcmc_scene(dev, far=True, **kw):
    from touch_gs_amd.mcmc import MCMCConfig
    model, views = _scene(dev)
    if far:     # no refinement within the test
        kw = dict(warmup_length=10_000, **kw)
    model.enable_mcmc(MCMCConfig(**kw))
    return model, views


def _seg_masks(model):
    """Boolean masks over the flat buffer: means, log_scales + opac_logit, the rest."""
    from touch_gs_amd.optim import layout
    L = layout(model.params.N, model.params.K)
    tot = L["total"]
    means = torch.zeros(tot, dtype=torch.bool)
    means[L["means"][0]:L["means"][0] + L["means"][1]] = True
    reg = torch.zeros(tot, dtype=torch.bool)
    for k in ("log_scales", "opac_logit"):
        reg[L[k][0]:L[k][0] + L[k][1]] = True
    return means, reg, ~(means | reg)


def test_mcmc_step_with_everything_off_is_the_unfused_step(dev):
    ref, views = _scene(dev)
    ref.fuse_adam = False
    ref.train_step(views[0])
    ref.train_step(views[1])
    model, views = _mcmc_scene(dev, **OFF)
    assert model.mcmc is not None and model.density is not None
    model.train_step(views[0], next_view=views[1])
    assert model._prefetch_ready is None, "MCMC mode arms no prefetch"
    model.train_step(views[1])
    for a, b in zip(_state(model), _state(ref)):
        assert torch.equal(_bits(a), _bits(b))
    assert model.optimizer.t == 2 and model.step == 2


def test_regularisers_and_noise_touch_only_their_elements(dev):
    ref, views = _scene(dev)
    ref.fuse_adam = False
    ref.train_step(views[0])
    base = _state(ref)
    reg_model, views = _mcmc_scene(dev, noise_lr=0.0)          # regularisers at their defaults
    reg_model.train_step(views[0])
    reg = _state(reg_model)
    means, regm, rest = (m.to(dev) for m in _seg_masks(reg_model))
    for a, b in zip(reg, base):     # first step from zero moments: only the opac_logit / log_scales elements can differ
        assert torch.equal(_bits(a)[~regm], _bits(b)[~regm])
    assert not torch.equal(reg[1][regm], base[1][regm]), "the regulariser is in the first moment of logits and log-scales"
    noisy = []
    for _ in range(2):
        m, views = _mcmc_scene(dev, seed=5)                    # ... and the noise
        m.train_step(views[0])
        noisy.append(_state(m))
    assert torch.equal(_bits(noisy[0][1]), _bits(reg[1])) and torch.equal(_bits(noisy[0][2]), _bits(reg[2]))
    assert torch.equal(_bits(noisy[0][0])[~means], _bits(reg[0])[~means]), "the noise moves the means alone"
    assert not torch.equal(noisy[0][0][means], reg[0][means])
    assert torch.isfinite(noisy[0][0]).all()
    for a, b in zip(*noisy):        # the same seed: the same bits
        assert torch.equal(_bits(a), _bits(b))
    other, views = _mcmc_scene(dev, seed=6)
    other.train_step(views[0])
    assert not torch.equal(_state(other)[0][means], noisy[0][0][means])


def test_strategy_off_is_todays_step_and_calls_no_mcmc_entry_point(dev, monkeypatch):
    from touch_gs_amd import ops
    res = []
    calls = dict(n=0)
    real = ops.mcmc_adam_geom
    for count in (False, True):
        model, views = _scene(dev)
        if count:
            def counting(*a, **k):
                calls["n"] += 1
                return real(*a, **k)
            monkeypatch.setattr(ops, "mcmc_adam_geom", counting)
            monkeypatch.setattr(ops, "mcmc_relocate", lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
        model.train_step(views[0], next_view=views[1])
        model.train_step(views[1])
        assert "mcmc" not in model.state_dict() and model.mcmc is None and model.density is None
        res.append(_state(model))
    assert calls["n"] == 0
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    model, views = _mcmc_scene(dev)         # the counter does count when the strategy is on
    model.train_step(views[0])
    assert calls["n"] == 1


def test_growth_to_the_cap(dev):
    model, views = _mcmc_scene(dev, far=False, cap_max=400, refine_every=10, warmup_length=10)
    floor = float(np.float32(0.005)) * (1 - 2.0 ** -21)     # the fp32 logit of a clamped opacity: tests/test_cpu_mcmc.py
    sizes, losses = [], []
    for s in range(70):
        model.train_step(views[s % 3])
        if s < 3 or s >= 67:
            l = model.loss_from(model.last["tile_loss"], model.last["ssim_sum"], model.last["view"])
            losses.append(float(sum(v for v in l.values())))
        if (s + 1) % 10 == 0:
            assert model._refined_at == s + 1 and model.last_refine["after"] == model.params.N
            sizes.append(model.params.N)
            assert torch.isfinite(model.params.flat).all() and torch.isfinite(model.optimizer.exp_avg).all()
            assert float(torch.sigmoid(model.params.opac_logit.double()).min()) >= floor
            assert model.optimizer.exp_avg.numel() == model.params.flat.numel() and model.density.vis_count.numel() == model.params.N
    assert sizes == [315, 330, 346, 363, 381, 400, 400]
    print(f"FIG growth: loss over the first three views {losses[:3]}, the last three {losses[3:]}")
    assert sum(losses[3:]) < sum(losses[:3])
    assert model.density.due(80) and not model.density.due(85)


def test_state_dict_round_trip_reproduces_the_next_step(dev):
    def run(reload):
        model, views = _mcmc_scene(dev, seed=3)
        model.train_step(views[0])
        model.train_step(views[1])
        if reload:
            sd = model.state_dict()
            assert set(sd["mcmc"]) == {"generator"} and sd["config"]["mcmc_noise_lr"] == 5e5
            other, views = _mcmc_scene(dev, seed=99)       # another seed: the checkpoint's stream must win
            other.load_state_dict(sd)
            model = other
        model.train_step(views[2])
        return _state(model)

    for a, b in zip(run(False), run(True)):
        assert torch.equal(_bits(a), _bits(b))


def test_refusals(dev):
    from touch_gs_amd.mcmc import MCMCConfig
    model, views = _scene(dev, nv=1, opacity_reg=0.01)
    with pytest.raises(ValueError, match="opacity_reg.*enable_mcmc"):       # weights set without the strategy
        model.train_step(views[0])
    model, views = _mcmc_scene(dev)
    with pytest.raises(ValueError, match="MCMC"):
        model.train_step(views[0], dp=types.SimpleNamespace(active=True))
    with pytest.raises(ValueError, match="MCMC"):
        model.capture_step_graphs(views)
    with pytest.raises(ValueError, match="MCMC"):
        model.enable_densification()
    model, views = _scene(dev, nv=1)
    model.enable_densification()
    with pytest.raises(ValueError, match="enable_densification"):
        model.enable_mcmc(MCMCConfig())


def test_trainer_flags_reach_the_config_and_the_trainer_state(dev, tmp_path):
    from touch_gs_amd import train
    base = ["--synthetic", "2000", "64", "48", "--max-num-iterations", "16", "--steps-per-save", "16", "--steps-per-eval", "16"]
    run = train.main(base + ["--strategy", "mcmc", "--cap-max", "2100", "--mcmc-noise-lr", "1000", "--opacity-reg", "0.02",
                             "--scale-reg", "0.03", "--mcmc-min-opacity", "0.01", "--refine-every", "8", "--warmup-length", "8",
                             "--output-dir", str(tmp_path / "on")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["strategy"] == "mcmc" and cfg["cap_max"] == 2100 and cfg["mcmc_min_opacity"] == 0.01
    assert cfg["model"]["opacity_reg"] == 0.02 and cfg["model"]["scale_reg"] == 0.03 and cfg["model"]["mcmc_noise_lr"] == 1000
    sd = torch.load(os.path.join(run, "step-000000016.ckpt"), map_location="cpu", weights_only=False)
    assert sd["trainer"]["strategy"] == "mcmc" and "mcmc" in sd and sd["N"] == 2100       # 2000 -> 2100 at steps 8 and 16
    run = train.main(base + ["--output-dir", str(tmp_path / "off")])
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["strategy"] == "default" and cfg["model"]["opacity_reg"] == 0.0 and cfg["model"]["mcmc_noise_lr"] == 0.0
    sd = torch.load(os.path.join(run, "step-000000016.ckpt"), map_location="cpu", weights_only=False)
    assert sd["trainer"]["strategy"] == "default" and "mcmc" not in sd
