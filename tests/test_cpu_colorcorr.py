"""The seam the model talks to (touch_gs_amd.colorcorr.ViewColorSet) on both of its subclasses, built on the CPU: nothing
here loads the library or launches a kernel."""
import types

import pytest
import torch

from touch_gs_amd.bilagrid import BilagridSet
from touch_gs_amd.colorcorr import ViewColorSet
from touch_gs_amd.exposure import ExposureSet

SHAPE = (5, 3, 4)       # (GW, GH, L)
NG = 3 * 5 * 4 * 12
TV_WEIGHT = 7.0
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]

# kind -> (constructor, name, rate field, start field, parameters per row, leaf shape, row length, length of the result vector)
KINDS = {
    "exposure": (lambda v: ExposureSet(v, "cpu", lr=1e-2), "exposure", "exposure_lr", "exposure_start_step", 12, (3, 4), 48, 32),
    "bilagrid": (lambda v: BilagridSet(v, "cpu", lr=2e-3, shape=SHAPE, tv_weight=TV_WEIGHT), "bilagrid", "bilagrid_lr",
                 "bilagrid_start_step", NG, (3, 5, 4, 12), 3 * NG + 16, 8),
}


@pytest.fixture(params=sorted(KINDS))
def case(request):
    make, *facts = KINDS[request.param]
    views = [object(), object(), object()]
    cs = make(views)
    g = torch.Generator().manual_seed(11)
    cs.state[:, :facts[3]] += 0.1 * torch.randn(3, facts[3], generator=g)       # off the identity: every expression is live
    return (cs, views, make, *facts)


def test_base_rows_ownership_and_state_dict(case):
    cs, views, make, name, _, _, n, _, row_len, _ = case
    assert isinstance(cs, ViewColorSet) and cs.state.shape == (3, row_len) and cs.state.dtype == torch.float32
    assert all(cs.owns(v) for v in views) and not cs.owns(object())
    for i, v in enumerate(views):
        assert cs.row(v).data_ptr() == cs.state[i].data_ptr() and cs.row(v).shape == (row_len,)
    fresh = make(views)
    assert torch.equal(fresh.state[:, :n], torch.tensor(IDENTITY, dtype=torch.float32).repeat(3, n // 12))
    assert make([]).state.shape == (0, row_len)
    sd = cs.state_dict()
    assert sd["state"].data_ptr() != cs.state.data_ptr() and (name == "bilagrid") == ("shape" in sd)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.state, cs.state)
    with pytest.raises(ValueError, match="checkpoint holds"):
        make(views[:2]).load_state_dict(sd)


def test_bilagrid_refuses_a_checkpoint_of_another_grid():
    sd = BilagridSet([object()], "cpu", shape=SHAPE).state_dict()
    with pytest.raises(ValueError, match="checkpoint holds bilateral-grid rows"):
        BilagridSet([object()], "cpu", shape=(3, 5, 4)).load_state_dict(sd)    # the same row length, other axes


def test_names_and_config_fields(case):
    from touch_gs_amd.model import ModelConfig
    cs, _, _, name, rate_field, start_field, *_ = case
    assert (cs.name, cs.rate_field, cs.start_field) == (name, rate_field, start_field)
    assert type(cs).name == name and isinstance(type(cs).what, str)
    cfg = ModelConfig()
    assert getattr(cfg, rate_field) == 0.0 and getattr(cfg, start_field) == 0


def test_l1_value_and_loss_terms_need_no_instance(case):
    cs, *_, out_len = case
    result = torch.arange(out_len, dtype=torch.float32)
    cfg = types.SimpleNamespace(bilagrid_tv=TV_WEIGHT)
    if cs.name == "exposure":
        assert float(ExposureSet.l1_value(result)) == 25 and ExposureSet.loss_terms(result, cfg) == {}
    else:
        assert float(BilagridSet.l1_value(result)) == 1
        terms = BilagridSet.loss_terms(result, cfg)
        assert set(terms) == {"bilagrid_tv_loss"} and torch.equal(terms["bilagrid_tv_loss"], TV_WEIGHT * result[3])
    assert float(cs.l1_value(result)) == float(type(cs).l1_value(result))


def test_leaf_is_a_detached_copy(case):
    cs, views, _, _, _, _, n, leaf_shape, _, _ = case
    before = cs.state.clone()
    for rg in (False, True):
        leaf = cs.leaf(views[1], rg)
        assert leaf.shape == leaf_shape and leaf.requires_grad == rg and leaf.is_leaf and leaf.grad_fn is None
        assert torch.equal(leaf.detach().reshape(-1), cs.state[1, :n])
        with torch.no_grad():
            leaf += 1.0
        assert torch.equal(cs.state, before)


def test_metrics_are_the_models_expressions(case):
    cs, _, make, name, *_ = case
    if name == "exposure":
        E = cs.state[:, :12]
        want = dict(exposure_gain=E[:, [0, 5, 10]].mean(), exposure_offset=E[:, [3, 7, 11]].mean())
    else:
        GW, GH, L = SHAPE
        g = cs.state[:, :NG].view(-1, GH, GW, L, 12)
        want = dict(bilagrid_tv=sum(((g.narrow(a, 1, g.shape[a] - 1) - g.narrow(a, 0, g.shape[a] - 1)) ** 2).mean() for a in (1, 2, 3)),
                    bilagrid_delta=(g - g.new_tensor([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])).abs().mean())
    got = cs.metrics()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert make([]).metrics() == {}


def test_leaf_loss_terms(case):
    cs, views, *_ = case
    g = cs.leaf(views[2], True)
    got = cs.leaf_loss_terms(g)
    if cs.name == "exposure":
        assert got == {}
        return
    want = TV_WEIGHT * sum(((g.narrow(a, 1, g.shape[a] - 1) - g.narrow(a, 0, g.shape[a] - 1)) ** 2).mean() for a in (0, 1, 2))
    assert set(got) == {"bilagrid_tv_loss"} and torch.equal(got["bilagrid_tv_loss"], want) and float(want.detach()) > 0
    got["bilagrid_tv_loss"].backward()
    assert g.grad is not None and g.grad.abs().max() > 0
