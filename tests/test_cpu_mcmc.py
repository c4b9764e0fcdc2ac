"""CPU tests of the MCMC strategy: the two entry points exist within TGS_VERSION 320 and refuse bad arguments before any
launch; the references of tests/mcmc_ref.py agree with each other and with torch autograd; ops.mcmc_relocate on CPU tensors
(torch fp64, the single sum) agrees with the 80-digit definition; the controller's two phases on CPU tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import mcmc_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_export_and_binding_within_version_320():
    from touch_gs_amd import _lib, ops
    lib = _lib.load()
    txt = open(os.path.join(ROOT, "include", "tgs.h")).read()
    assert lib.tgs_version() == 320 and "#define TGS_VERSION 320" in txt
    for name in ("tgs_mcmc_adam_geom", "tgs_mcmc_relocate"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    body = re.search(r"typedef struct TgsMcmcSpec \{(.*?)\} TgsMcmcSpec;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"float\s+(\w+);", body) == [f[0] for f in _lib.TgsMcmcSpec._fields_]
    assert C.sizeof(_lib.TgsMcmcSpec) == 20
    s = ops.mcmc_spec()
    assert (s.opacity_reg, s.scale_reg, s.noise_lr, s.gate_k, s.gate_o0) == tuple(
        float(np.float32(x)) for x in (0.01, 0.01, 5e5, 100.0, 0.005))
    assert callable(ops.mcmc_adam_geom) and callable(ops.mcmc_relocate)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from touch_gs_amd import _lib, ops
    lib = _lib.load()
    spec, mc = _lib.TgsAdamSpec(), ops.mcmc_spec()
    spec.bias_corr1 = spec.bias_corr2 = 1.0
    buf = (C.c_float * 64)()        # host memory: a call that got as far as a launch would not return TGS_E_ARG
    p = C.cast(buf, C.c_void_p)
    geom = lambda N, params=p, grads=p, m=p, v=p, sp=C.byref(spec), mcs=C.byref(mc): lib.tgs_mcmc_adam_geom(
        N, 4, params, grads, m, v, sp, C.c_float(1.0), mcs, None, None, None)
    assert geom(-1) == -1 and b"negative" in lib.tgs_last_error()
    assert geom(0) == 0
    for kw in (dict(params=None), dict(grads=None), dict(m=None), dict(v=None)):
        assert geom(5, **kw) == -1 and b"null" in lib.tgs_last_error()
    assert geom(5, sp=None) == -1 and geom(5, mcs=None) == -1
    bad = ops.mcmc_spec(opacity_reg=-1.0)
    assert geom(5, mcs=C.byref(bad)) == -1
    assert geom(5, params=C.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.tgs_last_error()
    reloc = lambda n, ratio=p, ol=p, ls=p, mo=0.005: lib.tgs_mcmc_relocate(n, ratio, ol, ls, C.c_float(mo), None)
    assert reloc(-1) == -1
    assert reloc(0) == 0
    assert reloc(5, ratio=None) == -1 and b"ratio" in lib.tgs_last_error()
    assert reloc(5, ol=None) == -1 and reloc(5, ls=None) == -1
    for mo in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert reloc(5, mo=mo) == -1 and b"min_opacity" in lib.tgs_last_error(), mo
    z = torch.zeros(4)
    with pytest.raises(ValueError):
        ops.mcmc_relocate(torch.ones(4, dtype=torch.int64), z, torch.zeros(4, 3))
    with pytest.raises(ValueError):
        ops.mcmc_relocate(torch.ones(4, dtype=torch.int32), z, torch.zeros(4, 3), min_opacity=0.0)


def test_double_sum_equals_the_hockey_stick_single_sum():
    worst = 0.0
    for o in MR.RELOC_O:
        for r in MR.RELOC_R:
            _, x = MR.reloc_x(MR.logit32(o), r)
            a, b = MR.reloc_sum_definition(x, r), MR.reloc_sum_single(x, r)
            worst = max(worst, float(abs(a - b) / abs(a)))
    assert worst < 1e-60, worst     # 80 digits, cancellation <= 2.9e4, 1326 terms


def test_cancellation_and_scale_multiplier_of_the_grid():
    """The figures the fp64 evaluation rests on: sum|terms| / |S| <= 2.9e4 (3e4 here), at o = 1 - 2^-23, r = 51; the scale
    multiplier o / S lies in [0.504, 1]."""
    worst, lo, hi = 0.0, np.inf, -np.inf
    for o in MR.RELOC_O:
        for r in MR.RELOC_R:
            _, dls, mass = MR.relocation_ref(MR.logit32(o), r, 0.005, definition=False)
            worst, lo, hi = max(worst, mass), min(lo, np.exp(dls)), max(hi, np.exp(dls))
    assert 2.8e4 < worst < 3.0e4 and 0.503 < lo and hi <= 1.0 + 1e-15, (worst, lo, hi)


def test_regulariser_gradient_equals_autograd():
    g = torch.Generator().manual_seed(3)
    N = 37
    ol = (torch.rand(N, generator=g, dtype=torch.float64) * 24 - 12).float().double().requires_grad_(True)
    ls = (torch.rand(N, 3, generator=g, dtype=torch.float64) * 9 - 8).float().double().requires_grad_(True)
    lo, lsr = MR.f32(0.01), MR.f32(0.02)
    (lo * torch.sigmoid(ol).mean() + lsr * torch.exp(ls).mean()).backward()
    go, gs = MR.reg_grad(ol.detach().numpy(), ls.detach().numpy(), 0.01, 0.02)
    assert np.allclose(go, ol.grad.numpy(), rtol=1e-12, atol=0) and np.allclose(gs, ls.grad.numpy(), rtol=1e-12, atol=0)


def _reloc_inputs(extra=()):
    l, r, new_l, dls = MR.relocation_grid(0.005, extra)
    ls0 = np.tile(np.asarray([-3.0, 0.5, -7.25], np.float32), (len(l), 1))
    return l, r, new_l, dls, ls0


def test_cpu_relocation_agrees_with_the_definition():
    from touch_gs_amd import ops
    l, r, new_l, dls, ls0 = _reloc_inputs()
    ol, ls = torch.from_numpy(l.copy()), torch.from_numpy(ls0.copy())
    ops.mcmc_relocate(torch.from_numpy(r.copy()), ol, ls, 0.005)
    one = r == 1
    assert one.sum() == len(MR.RELOC_O)
    assert np.array_equal(ol.numpy()[one].view(np.int32), l[one].view(np.int32)), "ratio 1 leaves the row's bits alone"
    assert np.array_equal(ls.numpy()[one].view(np.int32), ls0[one].view(np.int32))
    m = ~one
    err_l = np.abs(ol.numpy().astype(np.float64) - new_l)[m] / np.abs(new_l[m])
    ref_ls = ls0.astype(np.float64) + dls[:, None]
    err_s = (np.abs(ls.numpy().astype(np.float64) - ref_ls) / np.abs(ref_ls))[m]
    print(f"FIG cpu relocation: worst relative error logit {err_l.max():.3g}, log-scale {err_s.max():.3g} (bound {2.0 ** -23:.3g})")
    assert err_l.max() <= 2.0 ** -23 and err_s.max() <= 2.0 ** -23
    # the clamps: o = 0.005 split 51 ways lands on min_opacity; nothing exceeds 1 - 2^-23
    op = 1.0 / (1.0 + np.exp(-ol.numpy().astype(np.float64)))
    assert op.min() >= MR.f32(0.005) * (1 - 2.0 ** -21) and op.max() <= 1 - 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# controller
# ---------------------------------------------------------------------------------------------------------------------
def _store(N=200, K=4, n_dead=23, seed=0):
    from touch_gs_amd.optim import FusedAdam, GaussianParams
    g = torch.Generator().manual_seed(seed)
    ol = torch.rand(N, generator=g) * 8 - 3                       # opacities 0.047 ... 0.993
    dead = torch.randperm(N, generator=g)[:n_dead]
    ol[dead] = -8.0 - torch.rand(n_dead, generator=g)              # <= 3.4e-4
    means = torch.arange(N, dtype=torch.float32)[:, None].repeat(1, 3) + torch.tensor([0.0, 0.25, 0.5])   # row i: recognisable
    p = GaussianParams.from_tensors(means, torch.rand(N, 3, generator=g) * 4 - 6, torch.randn(N, 4, generator=g), ol,
                                    torch.randn(N, K, 3, generator=g))
    opt = FusedAdam(p, dict(means=1e-4, log_scales=1e-3, quats=1e-3, opac_logit=1e-2, sh_dc=1e-3, sh_rest=1e-4))
    opt.t = 17
    mv, vv = GaussianParams.views_of(opt.exp_avg, N, K), GaussianParams.views_of(opt.exp_avg_sq, N, K)
    for k in GaussianParams.NAMES:      # every moment element non-zero and tied to its row
        shape = mv[k].shape
        rows = torch.arange(1, N + 1, dtype=torch.float32).view(-1, *([1] * (len(shape) - 1)))
        mv[k].copy_(rows.expand(shape))
        vv[k].copy_(rows.expand(shape) + 0.5)
    dead_mask = torch.zeros(N, dtype=torch.bool)
    dead_mask[dead] = True
    return p, opt, dead_mask


def _runs(p):
    """(parent row of every new row, position inside its run) read off the means, which no phase changes."""
    parent = p.means[:, 0].round().long()
    start = torch.ones_like(parent, dtype=torch.bool)
    start[1:] = parent[1:] != parent[:-1]
    first = torch.cummax(torch.where(start, torch.arange(len(parent)), torch.zeros_like(parent)), 0).values
    return parent, torch.arange(len(parent)) - first


def _moments(opt, N, K):
    from touch_gs_amd.optim import GaussianParams
    return GaussianParams.views_of(opt.exp_avg, N, K), GaussianParams.views_of(opt.exp_avg_sq, N, K)


def _controller(**kw):
    from touch_gs_amd.mcmc import MCMCConfig, MCMCController
    cfg = MCMCConfig(**kw)
    return MCMCController(cfg, 0, "cpu")


def _alive_floor(min_opacity=0.005):
    # the clamp is applied to the fp64 opacity; its fp32 logit is off by up to 2^-24 |logit| = 2^-24 x 5.3, which moves
    # the opacity by that much relative: below 2^-21
    return MR.f32(min_opacity) * (1 - 2.0 ** -21)


def test_relocation_keeps_n_and_leaves_no_dead_row():
    from touch_gs_amd.optim import GaussianParams
    N, K = 200, 4
    p, opt, dead = _store(N, K)
    ctl = _controller(cap_max=N)          # at the cap: the relocation alone
    q, qopt, info = ctl.refine(p, opt, 100)
    assert info == dict(before=N, after=N, relocated=23, added=0, dead=23) and q.N == N and qopt.t == 17
    assert float(torch.sigmoid(q.opac_logit.double()).min()) >= _alive_floor()
    parent, within = _runs(q)
    assert not dead[parent].any(), "a dead row survived"
    assert torch.equal(torch.unique_consecutive(parent), torch.nonzero(~dead).squeeze(1)), "children sit behind their parents, in order"
    assert torch.equal(q.means, p.means[parent]) and torch.equal(q.quats, p.quats[parent]) and torch.equal(q.sh, p.sh[parent])
    run_len = torch.bincount(parent, minlength=N)[parent]
    single = run_len == 1
    assert (run_len[~single] > 1).all() and int((run_len - 1)[within == 0].sum()) == 23
    # rows of a run of one are untouched bit for bit, moments included; every row of a longer run starts from zero moments
    assert torch.equal(q.opac_logit[single], p.opac_logit[parent][single]) and torch.equal(q.log_scales[single], p.log_scales[parent][single])
    assert (q.opac_logit[~single] < p.opac_logit[parent][~single]).all() and (q.log_scales[~single] < p.log_scales[parent][~single]).all()
    (m1, v1), (m0, v0) = _moments(qopt, N, K), _moments(opt, N, K)
    for k in GaussianParams.NAMES:
        assert torch.equal(m1[k][single], m0[k][parent][single]) and torch.equal(v1[k][single], v0[k][parent][single]), k
        assert not m1[k][~single].any() and not v1[k][~single].any(), k
    # the relocation values are those of ops.mcmc_relocate with ratio = run length
    ol, ls = p.opac_logit[parent].clone(), p.log_scales[parent].clone()
    from touch_gs_amd import ops
    ops.mcmc_relocate(run_len.to(torch.int32), ol, ls, 0.005)
    assert torch.equal(ol, q.opac_logit) and torch.equal(ls, q.log_scales)
    # the inputs are not modified
    assert p.N == N and torch.equal(_store(N, K)[0].flat, p.flat)


def test_growth_follows_the_cap_and_children_start_at_zero():
    from touch_gs_amd.optim import GaussianParams
    N, K = 200, 4
    p, opt, _ = _store(N, K, n_dead=0)
    ctl = _controller(cap_max=225)
    sizes = []
    q, qopt, info = ctl.refine(p, opt, 100)
    assert info == dict(before=200, after=210, relocated=0, added=10, dead=0)
    parent, within = _runs(q)
    assert torch.equal(torch.unique_consecutive(parent), torch.arange(N)), "every row survives, children directly behind it"
    (m1, v1), (m0, v0) = _moments(qopt, q.N, K), _moments(opt, N, K)
    for k in GaussianParams.NAMES:
        assert torch.equal(m1[k][within == 0], m0[k]) and torch.equal(v1[k][within == 0], v0[k]), "parents keep their moments"
        assert not m1[k][within > 0].any() and not v1[k][within > 0].any(), "children start at zero"
    run_len = torch.bincount(parent, minlength=N)[parent]
    assert torch.equal(q.opac_logit[run_len == 1], p.opac_logit[parent][run_len == 1])
    assert (q.opac_logit[run_len > 1] < p.opac_logit[parent][run_len > 1]).all()
    for step in (200, 300, 400):
        sizes.append(q.N)
        q, qopt, info = ctl.refine(q, qopt, step)
    sizes.append(q.N)
    assert sizes == [210, 220, 225, 225] and info["added"] == 0     # min(cap, int(1.05 N)), then the cap
    assert ctl.grad_norm_sum.numel() == 225         # the per-row fields spatial_sort permutes follow N


def test_same_step_same_draws_and_another_step_others():
    p, opt, _ = _store()
    a = _controller(cap_max=300).refine(p, opt, 100)
    b = _controller(cap_max=300).refine(p, opt, 100)
    c = _controller(cap_max=300).refine(p, opt, 200)
    d = _controller(cap_max=300, seed=1).refine(p, opt, 100)
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(a[0].flat), bits(b[0].flat)) and torch.equal(bits(a[1].exp_avg), bits(b[1].exp_avg))
    assert not torch.equal(a[0].flat, c[0].flat) and not torch.equal(a[0].flat, d[0].flat)


def test_zero_weight_rows_are_never_drawn():
    from touch_gs_amd.mcmc import sample_by_opacity
    w = torch.tensor([0.0, 0.3, 0.0, 0.0, 0.7, 0.0])
    idx = sample_by_opacity(w, 20000, 5)
    cnt = torch.bincount(idx, minlength=6)
    assert cnt[[0, 2, 3, 5]].sum() == 0 and abs(int(cnt[1]) / 20000 - 0.3) < 0.02


def test_all_dead_and_none_dead_are_no_ops():
    N = 50
    for n_dead, cap in ((N, 1000), (0, N)):
        p, opt, _ = _store(N, 1, n_dead=n_dead)
        q, qopt, info = _controller(cap_max=cap).refine(p, opt, 100)
        assert q is p and qopt is opt and info == dict(before=N, after=N, relocated=0, added=0, dead=n_dead)


def test_due_and_refusal_of_data_parallel():
    import types
    ctl = _controller(refine_every=100, warmup_length=500, stop_at=1000)
    assert [s for s in range(0, 1201, 50) if ctl.due(s)] == [500, 600, 700, 800, 900]
    p, opt, _ = _store(20, 1, n_dead=2)
    with pytest.raises(ValueError, match="data-parallel"):
        ctl.refine(p, opt, 500, dp=types.SimpleNamespace(active=True))
    ctl.accumulate(None, None, 0, 0)      # the DensityController surface, a no-op
