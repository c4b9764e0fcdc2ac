"""The Adam oracle of tests/adam_ref.py, without a GPU: it is torch.optim.Adam in fp64, its learning-rate map is the
layout of touch_gs_amd.optim, an fp32 emulation of the kernel's arithmetic stays inside the bounds of ``check_step``,
and every deliberately faulty emulation is rejected -- the evidence that tests/test_gpu_adam_oracle.py would notice a
subtly wrong kernel."""
import numpy as np
import pytest
import torch

from tests import adam_ref as A
from touch_gs_amd.optim import layout


@pytest.mark.parametrize("N,K", [(5, 1), (6, 4), (7, 9), (9, 16)])
def test_oracle_is_torch_adam_in_fp64(N, K):
    """adam_step_ref chained over 5 steps == torch.optim.Adam (fp64, one parameter group per segment with SH split into
    DC and rest, eps 1e-15): the semantics FusedAdam documents."""
    rng = np.random.default_rng(N * 100 + K)
    L = layout(N, K)
    total = L["total"]
    lr = A.lr_map(N, K, A.DEFAULT_LRS)
    pads = A.pad_mask(N, K)
    p = rng.standard_normal(total).astype(np.float32)
    p[pads] = 0
    views = lambda flat: {k: flat[L[k][0]:L[k][0] + L[k][1]].reshape(L[k][2]) for k in A.SEGMENTS}

    def groups(flat):
        v = views(flat)
        return [v["means"], v["log_scales"], v["quats"], v["opac_logit"], v["sh"][:, :1], v["sh"][:, 1:]]

    tp = [torch.from_numpy(x.astype(np.float64)).clone().requires_grad_(True) for x in groups(p)]
    # the oracle rounds its constants to fp32 as the kernel's struct does: give torch the same numbers
    opt = torch.optim.Adam([dict(params=[q], lr=A.f32(A.DEFAULT_LRS[k])) for q, k in zip(tp, A.LR_KEYS)],
                           betas=(A.f32(0.9), A.f32(0.999)), eps=A.f32(1e-15))
    b1, b2 = A.f32(0.9), A.f32(0.999)
    p64, m, v = p.astype(np.float64), np.zeros(total), np.zeros(total)
    for t in range(1, 6):
        g = rng.standard_normal(total).astype(np.float32)
        g[pads] = 0
        for q, gg in zip(tp, groups(g)):
            q.grad = torch.from_numpy(gg.astype(np.float64)).clone()
        opt.step()
        spec = A.AdamConsts(b1, b2, A.f32(1e-15), 1.0 - b1 ** t, 1.0 - b2 ** t)   # unrounded corrections, as torch's
        p64, m, v, u, am = A.adam_step_ref(p64, g, m, v, lr, spec, 1.0)            # float64 state: chained unrounded
    for got, want in zip(groups(p64), tp):
        w = want.detach().numpy()
        assert (np.abs(got - w) <= 1e-12 * np.abs(w)).all()
    for q, k in zip(tp, A.LR_KEYS):       # the moments too
        st = opt.state[q]
        i = A.LR_KEYS.index(k)
        assert (np.abs(groups(m)[i] - st["exp_avg"].numpy()) <= 1e-12 * np.abs(st["exp_avg"].numpy())).all()
        assert (np.abs(groups(v)[i] - st["exp_avg_sq"].numpy()) <= 1e-12 * np.abs(st["exp_avg_sq"].numpy())).all()
    assert not p64[pads].any() and not m[pads].any() and not v[pads].any()
    # a non-unit grad_scale is the same step on the scaled gradient (1/8: exact in fp32 and fp64)
    x = A.adam_step_ref(p64, g, m, v, lr, spec, 0.125)
    y = A.adam_step_ref(p64, (g * np.float32(0.125)), m, v, lr, spec, 1.0)
    assert all(np.array_equal(i, j) for i, j in zip(x, y))


@pytest.mark.parametrize("N", [8, 5, 6, 7, 1001, 1002])
@pytest.mark.parametrize("K", [0, 1, 4, 9, 16])
def test_lr_map_agrees_with_the_layout(N, K):
    """N = 0, 1, 2, 3 (mod 4): segment starts, pads and the DC / rest split are where touch_gs_amd.optim.layout puts them."""
    L = layout(N, K)
    segs, total = A.segments(N, K)
    assert total == L["total"]
    for name, start, n, end in segs:
        assert (start, n) == L[name][:2] and start % 4 == 0
    lrs = dict(means=1.0, log_scales=2.0, quats=3.0, opac_logit=4.0, sh_dc=5.0, sh_rest=6.0)
    lr = A.lr_map(N, K, lrs)
    pads = A.pad_mask(N, K)
    want = torch.zeros(total, dtype=torch.float64)
    named = torch.zeros(total, dtype=torch.bool)
    for k in ("means", "log_scales", "quats", "opac_logit"):
        want[L[k][0]:L[k][0] + L[k][1]] = lrs[k]
        named[L[k][0]:L[k][0] + L[k][1]] = True
    sh = want[L["sh"][0]:L["sh"][0] + L["sh"][1]].view(L["sh"][2])
    sh[:, :1] = 5.0
    sh[:, 1:] = 6.0
    named[L["sh"][0]:L["sh"][0] + L["sh"][1]] = True
    assert np.array_equal(pads, ~named.numpy())
    assert pads.sum() == total - 11 * N - 3 * K * N
    assert np.array_equal(lr[~pads], want.numpy()[~pads])
    # a pad takes the rate of the segment it trails
    for i in np.nonzero(pads)[0]:
        j = i
        while pads[j]:
            j -= 1
        seg = [s for s in segs if s[1] <= j < s[1] + s[2]][0][0]
        assert lr[i] == (lrs[seg] if seg != "sh" else 5.0)
    # the emulated kernel's incremental row tracking reproduces the map, with and without grid striding
    for cap in (4096, 1, 3):
        assert np.array_equal(A.kernel_lr_emulated(N, K, lrs, max_blocks=cap).astype(np.float64), lr)


STEPS = (1, 2, 3, 10, 100, 30000)
SCALES = (1.0, 1.0 / 8, 1.0 / 3)


def test_emulation_stays_inside_the_bounds():
    """The fp32 emulation of adam1 passes check_step on stratified inputs (|g|, |m|, sqrt v log-uniform in 1e-30 .. 1e3
    with exact zeros, a quarter of the parameters 0) at steps 1, 2, 3, 10, 100, 30 000 and three grad scales; the worst
    ratios are printed in units of E (the table of tests/adam_ref.py)."""
    N, K = 1003, 16
    lr = A.lr_map(N, K, A.DEFAULT_LRS)
    worst = dict(m=0.0, v=0.0, p=0.0, p_half_ulp=0.0)
    for t in STEPS:
        for s in SCALES:
            rng = np.random.default_rng(t * 7 + int(1 / s))
            p0, g, m0, v0 = A.stratified_state(N, K, rng)
            spec = A.consts(t)
            p1, m1, v1 = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, spec, s, max_blocks=8)
            r = A.check_step((p0, m0, v0), (p1, m1, v1), g, 0.0, lr, spec, s, layout=(N, K))
            worst = {k: max(worst[k], r[k]) for k in worst}
            pads = A.pad_mask(N, K)
            assert not p1[pads].any() and not m1[pads].any() and not v1[pads].any()
    print(f"worst ratios in E: m {worst['m']:.2f} (bound {A.C_M}), v {worst['v']:.2f} (bound {A.C_V}), "
          f"update beyond 1 ulp(p) {worst['p']:.2f}, beyond E max|p| {worst['p_half_ulp']:.2f} (bound {A.C_U})")
    assert 0 < worst["m"] <= A.C_M and 0 < worst["v"] <= A.C_V and worst["p_half_ulp"] <= A.C_U


def _sh_range(N, K):
    segs, total = A.segments(N, K)
    return segs[4][1], total


@pytest.mark.parametrize("N,K", A.GRID_STRIDE_SH)
def test_row_step_is_live_in_the_grid_stride_launches(N, K):
    """The launches of tests/test_gpu_adam_oracle.py::test_adam_step_grid_stride_inside_sh, at the kernel's block cap:
    the SH segment as one range is more than one grid-stride iteration, the emulated row tracking reproduces the
    learning-rate map there, and with row_step off by one it does not -- on thousands of elements, all of them in
    iteration 1.  So a kernel that reads row_step wrongly cannot pass that test."""
    b, e = _sh_range(N, K)
    one_iteration = 4 * 256 * A.MAX_BLOCKS
    assert A.launch_stride(b, e) * 4 == one_iteration and one_iteration + 40_000 < e - b < one_iteration + 55_000
    assert (4 * A.launch_stride(b, e)) % (3 * K) == {16: 16, 9: 16, 4: 4}[K]
    lrs = A.DEFAULT_LRS
    lr = A.lr_map(N, K, lrs).astype(np.float32)
    good = A.kernel_lr_emulated(N, K, lrs, elem_range=(b, e))
    assert np.array_equal(good, lr)
    bad = A.kernel_lr_emulated(N, K, lrs, mutate="row_step_off_by_one", elem_range=(b, e))
    differ = np.nonzero(bad != lr)[0]
    assert differ.size >= 2 * ((e - b - one_iteration) // (3 * K)) - 2     # two columns of every row of iteration 1
    assert differ.min() >= b + one_iteration and differ.max() < e


@pytest.mark.parametrize("N,K", [(71_111, 16), (110_401, 9), (220_003, 4), (300_001, 1)])
def test_whole_model_launches_just_beyond_one_iteration_do_not_read_row_step(N, K):
    """Why the launches above exist: in a whole-model step of the smallest models beyond 4 194 304 elements the second
    iteration is run by lanes that spent the first one in front of the SH segment, so no thread advances its column by
    row_step and the off-by-one mutant is invisible (test_adam_step_grid_stride checks those shapes for everything
    else the second iteration can get wrong)."""
    lrs = A.DEFAULT_LRS
    assert A.segments(N, K)[1] > 4 * 256 * A.MAX_BLOCKS
    assert np.array_equal(A.kernel_lr_emulated(N, K, lrs, mutate="row_step_off_by_one"), A.kernel_lr_emulated(N, K, lrs))


def _mutant_case(mutant):
    """(N, K, t, grad_scale, max_blocks, elem_range) at which the fault can show at all."""
    if mutant == "no_bias_corr2":
        return 1003, 16, 2, 1.0, 8, None          # fp32(1 - 0.999^30000) == 1: only early steps can tell
    if mutant == "grad_scale_m_only":
        return 1003, 16, 10, 1.0 / 3, 8, None
    if mutant == "row_step_off_by_one":           # the second of the GPU test's launches, at the kernel's block cap
        N, K = A.GRID_STRIDE_SH[1]
        return N, K, 3, 0.125, A.MAX_BLOCKS, _sh_range(N, K)
    if mutant == "pad_takes_neighbour":
        return 1003, 4, 3, 1.0, 8, None           # 1003 opacities: one pad behind them
    return 1003, 16, 3, 1.0, 8, None


@pytest.mark.parametrize("mutant", A.MUTANTS)
@pytest.mark.parametrize("zero_moments", [False, True])
def test_every_mutant_fails_check_step(mutant, zero_moments):
    N, K, t, s, cap, rge = _mutant_case(mutant)
    rng = np.random.default_rng(11)
    p0, g, m0, v0 = A.stratified_state(N, K, rng, zero_moments=zero_moments, only=rge)
    b, e = rge or (0, p0.size)
    cut = lambda bufs: tuple(x[b:e] for x in bufs)
    kw = dict(layout=(N, K), base=b, launch=(b, e, cap))
    if mutant == "pad_takes_neighbour":
        g[A.segments(N, K)[0][3][1] + N - 1] = 0.25      # the last opacity's gradient: the non-zero neighbour
    spec = A.consts(t)
    lr = A.lr_map(N, K, A.DEFAULT_LRS)
    good = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, spec, s, max_blocks=cap, elem_range=rge)
    A.check_step(cut((p0, m0, v0)), cut(good), g[b:e], 0.0, lr[b:e], spec, s, **kw)
    bad = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, spec, s, mutate=mutant, max_blocks=cap, elem_range=rge)
    for x, y in zip(bad, (p0, m0, v0)):
        assert np.array_equal(x[:b], y[:b]) and np.array_equal(x[e:], y[e:])
    with pytest.raises(AssertionError) as ei:
        A.check_step(cut((p0, m0, v0)), cut(bad), g[b:e], 0.0, lr[b:e], spec, s, **kw)
    msg = str(ei.value)
    print(mutant, "->", msg[:200])
    expect = {"swap_dc_rest_column": "(c) parameter", "no_bias_corr2": "(c) parameter", "row_step_off_by_one": "(c) parameter",
              "grad_scale_m_only": "(b) exp_avg_sq", "pad_takes_neighbour": "(a) exp_avg"}[mutant]
    assert expect in msg, msg
    if mutant in ("swap_dc_rest_column", "row_step_off_by_one"):
        assert ": sh[" in msg
    if mutant == "row_step_off_by_one":
        assert "grid-stride iteration 1:" in msg, msg
    if mutant == "pad_takes_neighbour":
        assert "(pad)" in msg


@pytest.mark.parametrize("mutant", ["swap_dc_rest_column", "no_bias_corr2", "row_step_off_by_one"])
def test_self_consistency_check_rejects_update_faults(mutant):
    """check_self_consistent (the fused kernel's check: no gradient buffer) accepts the emulation and rejects the
    faults that live in the update; from a zero state it is v1 = (1 - b2) (m1 / (1 - b1))^2 to 16E."""
    N, K, t, s, cap, _ = _mutant_case(mutant)
    if mutant == "row_step_off_by_one":
        N, K, cap = 1003, 9, 2      # 2 blocks of 256 float4: row_step (2048 mod 27) is live from flat 2048 on
    rng = np.random.default_rng(5)
    lr = A.lr_map(N, K, A.DEFAULT_LRS)
    for zero in (True, False):
        p0, g, m0, v0 = A.stratified_state(N, K, rng, zero_moments=zero)
        spec = A.consts(t)
        good = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, spec, 1.0, max_blocks=cap)
        A.check_self_consistent((p0, m0, v0), good, lr, spec, layout=(N, K))
        if zero:
            m1, v1 = good[1].astype(np.float64), good[2].astype(np.float64)
            want = (1 - spec.beta2) * (m1 / (1 - spec.beta1)) ** 2
            assert (np.abs(v1 - want) <= 16 * A.E * want + A.DENORM).all()
        bad = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, spec, 1.0, mutate=mutant, max_blocks=cap)
        with pytest.raises(AssertionError):
            A.check_self_consistent((p0, m0, v0), bad, lr, spec, layout=(N, K))
    # a second moment that does not belong to the first one is rejected too
    p0, g, m0, v0 = A.stratified_state(N, K, rng, zero_moments=True)
    p1, m1, v1 = A.adam1_emulated(N, K, p0, g, m0, v0, A.DEFAULT_LRS, A.consts(1), 1.0)
    with pytest.raises(AssertionError):
        A.check_self_consistent((p0, m0, v0), (p1, m1, (v1 * np.float32(1 + 2e-6)).astype(np.float32)), lr, A.consts(1))
