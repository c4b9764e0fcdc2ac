"""The two MCMC kernels (csrc/mcmc.hip) against tests/mcmc_ref.py and tests/adam_ref.py.

Shapes (N, K) = (1, 4), (257, 4), (1003, 16): one thread, a ragged second workgroup, and odd N so that every segment trails
a pad.  Inputs: gradients and moments stratified (adam_ref.stratified; the second moments at least the square of the first,
so that an update stays below 4.1 learning rates and the updated log-scales and logits stay where the noise term is finite),
log-scales in [-8, 1], logits in [-12, 12] with a cluster around logit(0.005) where the gate turns and many with t > 80,
|q| in [0.1, 3] (mcmc_ref.noise_inputs).  Every bound is derived in tests/mcmc_ref.py and tests/adam_ref.py."""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from tests import mcmc_ref as MR

pytestmark = pytest.mark.gpu

LRS = A.DEFAULT_LRS
SHAPES = [(1, 4), (257, 4), (1003, 16)]
MCMC = dict(opacity_reg=0.01, scale_reg=0.01, noise_lr=5e5, gate_k=100.0, gate_o0=0.005)


def _bits(t):
    return t.view(torch.int32)


def _state(N, K, mode, seed):
    """(p, g, m, v) float32 [total] and the noise draws float32 [N,3].  mode "zero": zero moments (step 1); "stratified":
    stratified moments with v >= m^2 (step 30 000)."""
    rng = np.random.default_rng(seed)
    p, g, m, v = A.stratified_state(N, K, rng, zero_moments=(mode == "zero"))
    v = np.maximum(v, m * m)
    segs, _ = A.segments(N, K)
    off = {name: start for name, start, _, _ in segs}
    ol, ls, q, n = MR.noise_inputs(N, rng)
    p[off["log_scales"]:off["log_scales"] + 3 * N] = ls.reshape(-1)
    p[off["quats"]:off["quats"] + 4 * N] = q.reshape(-1)
    p[off["opac_logit"]:off["opac_logit"] + N] = ol
    return (p, g, m, v), n, off


def _make(dev, N, K, state, t):
    from touch_gs_amd.optim import FusedAdam, GaussianParams
    p, g, m, v = state
    gp = GaussianParams.allocate(N, K, dev)
    gp.flat.copy_(torch.from_numpy(p))
    gp.grad.copy_(torch.from_numpy(g))
    opt = FusedAdam(gp, LRS, eps=1e-15)
    opt.exp_avg.copy_(torch.from_numpy(m))
    opt.exp_avg_sq.copy_(torch.from_numpy(v))
    opt.t = t
    return gp, opt


def _snap(opt):
    torch.cuda.synchronize()
    return tuple(x.detach().cpu().numpy().copy() for x in (opt.p.flat, opt.exp_avg, opt.exp_avg_sq))


def _run(dev, N, K, state, t, noise=None, guard=None, grad_scale=1.0, **mc):
    from touch_gs_amd import ops
    gp, opt = _make(dev, N, K, state, t)
    opt.begin_step()
    nz = None if noise is None else torch.from_numpy(noise).to(dev)
    ops.mcmc_adam_geom(opt, ops.mcmc_spec(**{**MCMC, **mc}), nz, grad_scale=grad_scale, guard=guard)
    return _snap(opt), opt


@pytest.mark.parametrize("mode,t0", [("zero", 0), ("stratified", 29_999)])
@pytest.mark.parametrize("N,K", SHAPES)
def test_adam_regulariser_and_noise(dev, N, K, mode, t0):
    state, n, off = _state(N, K, mode, 7000 * N + K + t0)
    p0, g, m0, v0 = state
    segs, total = A.segments(N, K)
    ge = off["sh"]                                   # the geometry range [0, ge)
    spec = A.consts(t0 + 1, (0.9, 0.999), 1e-15)
    lr = A.lr_map(N, K, LRS)
    for grad_scale in (1.0, 1.0 / 3):
        plain, _ = _run(dev, N, K, state, t0, noise=None, grad_scale=grad_scale)
        # -- Adam with the regulariser inside the gradient: all 11 values and both moments, dg = C_REG E |reg|
        reg = np.zeros(total)
        ro, rs = MR.reg_grad(p0[off["opac_logit"]:off["opac_logit"] + N], p0[off["log_scales"]:off["log_scales"] + 3 * N].reshape(N, 3),
                             MCMC["opacity_reg"], MCMC["scale_reg"])
        reg[off["opac_logit"]:off["opac_logit"] + N] = ro
        reg[off["log_scales"]:off["log_scales"] + 3 * N] = rs.reshape(-1)
        assert (ro > 0).all() and (rs > 0).all()
        r = A.check_step(tuple(x[:ge] for x in state[:1] + state[2:]), tuple(x[:ge] for x in plain), (g.astype(np.float64) + reg)[:ge],
                         (MR.C_REG * MR.E * np.abs(reg))[:ge], lr[:ge], spec, grad_scale, layout=(N, K))
        print(f"FIG N {N} K {K} {mode} scale {grad_scale:.3f}: Adam worst ratios in E " + ", ".join(f"{k} {x:.2f}" for k, x in sorted(r.items())))
        # the regulariser is really in there: without it the first moment of the logits differs
        none, _ = _run(dev, N, K, state, t0, noise=None, grad_scale=grad_scale, opacity_reg=0.0, scale_reg=0.0)
        sl = slice(off["opac_logit"], off["opac_logit"] + N)
        assert N == 1 or not np.array_equal(none[1][sl], plain[1][sl])
        # -- untouched memory: SH segment, SH moments and every pad
        pads = A.pad_mask(N, K)
        for a, b, name in zip(plain, (p0, m0, v0), ("p", "m", "v")):
            assert np.array_equal(a[ge:].view(np.int32), b[ge:].view(np.int32)), f"the SH segment of {name} was written"
            assert np.array_equal(a[pads].view(np.int32), b[pads].view(np.int32)), f"a pad of {name} was written"
        # -- noise: everything but the means keeps the bits of the run without noise
        noisy, _ = _run(dev, N, K, state, t0, noise=n, grad_scale=grad_scale)
        assert np.array_equal(noisy[1].view(np.int32), plain[1].view(np.int32)) and np.array_equal(noisy[2].view(np.int32), plain[2].view(np.int32))
        assert np.array_equal(noisy[0][3 * N:].view(np.int32), plain[0][3 * N:].view(np.int32))
        # means1 against (Adam part from the kernel's own moments) + delta_ref from the kernel's own updated ls', q', ol'
        p1, m1, v1 = (x.astype(np.float64) for x in noisy)
        ms = slice(0, 3 * N)
        u = A._update64(m1[ms], v1[ms], lr[ms], spec)
        ls1 = noisy[0][off["log_scales"]:off["log_scales"] + 3 * N].reshape(N, 3)
        q1 = noisy[0][off["quats"]:off["quats"] + 4 * N].reshape(N, 4)
        ol1 = noisy[0][off["opac_logit"]:off["opac_logit"] + N]
        assert np.isfinite(p1).all()
        kw = dict(noise_lr=MCMC["noise_lr"], lr_means=LRS["means"], gate_k=MCMC["gate_k"], gate_o0=MCMC["gate_o0"])
        delta, Aj, o1, gate, tt, Tj = MR.noise_ref(ol1, ls1, q1, n, **kw)
        want = p0[ms].astype(np.float64) - u + delta.reshape(-1)
        err = np.abs(p1[ms] - want)
        adam_part = A._ulp32(np.maximum(np.abs(p0[ms].astype(np.float64)), np.abs(p1[ms]))) + A.C_U * A.E * np.abs(u)
        edge = MR.gate_edge_slack(Aj, gate, tt, kw["noise_lr"], kw["lr_means"]).reshape(-1)
        sens = (1.0 + MR.f32(MCMC["gate_k"]) * o1)[:, None]
        for mass, C, name in ((Aj, MR.C_NOISE, "A"), (Tj, MR.C_NOISE_T, "T")):
            unit = (MR.E * sens * mass).reshape(-1)
            bound = adam_part + edge + C * unit
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(unit > 0, np.maximum(err - adam_part - edge, 0) / unit, 0.0)
            print(f"FIG N {N} K {K} {mode} scale {grad_scale:.3f}: noise worst ratio {ratio.max():.2f} E of mass {name} (C = {C:.1f})")
            bad = err > bound
            assert not bad.any(), (name, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()))
        # a closed gate (t > 80) moves nothing: the means keep the bits of the run without noise; an open one moves them
        closed = tt > MR.T_CUT + 1e-3
        open_ = (tt < MR.T_CUT - 1e-3) & (np.abs(n).sum(1) > 0)
        pm, nm = plain[0][ms].reshape(N, 3), noisy[0][ms].reshape(N, 3)
        assert np.array_equal(pm[closed].view(np.int32), nm[closed].view(np.int32))
        if N > 1:
            assert closed.any() and open_.any() and (gate[closed] == 0).all()
            assert (np.abs(nm[open_].astype(np.float64) - pm[open_]).sum(1) > 0).any()
        # the same inputs give the same bits
        again, _ = _run(dev, N, K, state, t0, noise=n, grad_scale=grad_scale)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(noisy, again))


@pytest.mark.parametrize("N,K", SHAPES)
def test_identity_with_the_existing_adam_and_guard(dev, N, K):
    from touch_gs_amd import ops
    for mode, t0 in (("zero", 0), ("stratified", 29_999)):
        state, n, off = _state(N, K, mode, 11 * N + K + t0)
        for grad_scale in (1.0, 1.0 / 3):
            gp, opt = _make(dev, N, K, state, t0)
            opt.begin_step()
            opt.step_range(0, off["sh"], grad_scale)
            want = _snap(opt)
            for kw in (dict(noise=None), dict(noise=n, noise_lr=0.0)):
                got, _ = _run(dev, N, K, state, t0, grad_scale=grad_scale, opacity_reg=0.0, scale_reg=0.0, **kw)
                for a, b, name in zip(got, want, ("p", "m", "v")):
                    assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, mode, grad_scale, sorted(kw))
        # the guard: a status word whose overflow flag is set (as data) makes the launch a no-op; a clear flag does not
        before = tuple(x.copy() for x in (state[0], state[2], state[3]))
        guard = torch.tensor([5, 1], dtype=torch.int32, device=dev)
        got, _ = _run(dev, N, K, state, t0, noise=n, guard=guard)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got, before))
        clear, _ = _run(dev, N, K, state, t0, noise=n, guard=torch.tensor([5, 0], dtype=torch.int32, device=dev))
        free, _ = _run(dev, N, K, state, t0, noise=n)
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(clear, free))
        assert not np.array_equal(free[0], before[0])
    with pytest.raises(ValueError):
        _run(dev, N, K, state, t0, noise=np.zeros((N + 1, 3), np.float32))


def test_relocation_against_the_definition(dev):
    """The CPU grid of o and r, plus r = 52 and 1000 (clamped to 51); o = 0.005 and o = 1 - 2^-23 sit at the clamps.
    |out - ref| <= 2^-23 |ref| + 2^-40 for the logit and each log-scale; ratio 1 rows keep their bits."""
    from touch_gs_amd import ops
    l, r, new_l, dls = MR.relocation_grid(0.005, (52, 1000))
    ls0 = np.tile(np.asarray([-3.0, 0.5, -7.25], np.float32), (len(l), 1))
    ol, ls = torch.from_numpy(l.copy()).to(dev), torch.from_numpy(ls0.copy()).to(dev)
    ops.mcmc_relocate(torch.from_numpy(r.copy()).to(dev), ol, ls, 0.005)
    torch.cuda.synchronize()
    ol, ls = ol.cpu().numpy(), ls.cpu().numpy()
    one = r == 1
    assert np.array_equal(ol[one].view(np.int32), l[one].view(np.int32)) and np.array_equal(ls[one].view(np.int32), ls0[one].view(np.int32))
    ref_ls = ls0.astype(np.float64) + dls[:, None]
    err_l, err_s = np.abs(ol.astype(np.float64) - new_l), np.abs(ls.astype(np.float64) - ref_ls)
    b_l, b_s = 2.0 ** -23 * np.abs(new_l) + 2.0 ** -40, 2.0 ** -23 * np.abs(ref_ls) + 2.0 ** -40
    m = ~one
    new_l, ref_ls = np.where(one, 1.0, new_l), np.where(one[:, None], 1.0, ref_ls)      # (ratio 1: not compared, no 0 / 0 below)
    print(f"FIG relocation: worst error / bound, logit {(err_l / b_l)[m].max():.3f}, log-scale {(err_s / b_s)[m].max():.3f}; "
          f"worst relative error {max((err_l / np.abs(new_l))[m].max(), (err_s / np.abs(ref_ls))[m].max()):.3g}")
    assert (err_l <= b_l)[m].all() and (err_s <= b_s)[m].all()
    assert m.sum() == len(MR.RELOC_O) * 7
    # the clamped ratios give the bits of 51; the CPU path (torch fp64, an independent implementation) agrees to one rounding
    r51 = r == 51
    for big in (52, 1000):
        assert np.array_equal(ol[r == big].view(np.int32), ol[r51].view(np.int32)) and np.array_equal(ls[r == big].view(np.int32), ls[r51].view(np.int32))
    c_ol, c_ls = torch.from_numpy(l.copy()), torch.from_numpy(ls0.copy())
    ops.mcmc_relocate(torch.from_numpy(r.copy()), c_ol, c_ls, 0.005)
    assert (np.abs(c_ol.numpy().astype(np.float64) - ol) <= np.spacing(np.abs(ol))).all()
    assert (np.abs(c_ls.numpy().astype(np.float64) - ls) <= np.spacing(np.abs(ls))).all()
    # more than one workgroup, ragged
    n = 300
    rr = torch.full((n,), 3, dtype=torch.int32, device=dev)
    o2, s2 = torch.zeros(n, device=dev), torch.zeros(n, 3, device=dev)
    ops.mcmc_relocate(rr, o2, s2, 0.005)
    assert bool((o2 == o2[0]).all()) and bool((s2 == s2[0, 0]).all()) and float(o2[0]) < 0
