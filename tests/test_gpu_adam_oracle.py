"""Every kernel that carries the Adam update, per element and per moment, against the fp64 oracle of tests/adam_ref.py
-- in units of the element's own update, moment or ulp (``check_step`` / ``check_self_consistent``; their constants and
the evidence that they reject subtly wrong kernels are in tests/adam_ref.py and tests/test_cpu_adam_ref.py).

    k_adam (tgs_adam_step)                          check_step, dg = 0: small shapes with every pad pattern and SH row
                                                    length, the grid-stride path, element ranges, the overflow guard,
                                                    the device-side bias corrections
    k_adam_sh_gathered (tgs_adam_step_sh_gathered_rows)
                                                    check_step on the SH segment against the fp64 gradient
                                                    sum_r Y(dir_r) (x) v_color_r, known to dg = C_SH E sum_r |Y|_r |v_r|
    fused K8+Adam (tgs_project_bwd_adam[_next_front])
                                                    check_self_consistent: its gradient never reaches memory

The two remaining kernels, k_adam_geom_project_next and k_adam_sh_geom_next (the tail of a data-parallel step), need a
real exchange to be reached; they stay tied bit for bit to k_adam / k_adam_sh_gathered by
tests/test_gpu_api_surfaces.py::test_data_parallel_train_step_two_ranks_one_gpu (the announced against the unannounced
sequence: k_adam_geom_project_next against k_adam) and
::test_fused_data_parallel_tail_is_bit_identical_to_the_chunked_one (k_adam_sh_geom_next against k_adam_sh_gathered +
k_adam_geom_project_next), and so to the oracle through the kernels checked here.
"""
import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import adam_ref as A

pytestmark = pytest.mark.gpu

LRS = A.DEFAULT_LRS
GRID_STRIDE_BEYOND = 4 * 256 * A.MAX_BLOCKS      # flat elements one launch of k_adam covers without grid-striding

# tgs_adam_step_sh_gathered_rows rebuilds the SH gradient in fp32 (direction, normalisation, basis polynomial, one fma
# per rank).  test_gathered_sh_adam measures its distance from the fp64 gradient from a zero state (m1 / ((1 - b1) s)
# is the kernel's gradient to 2E) and prints it for every case, in two units:
#
#   E sum_r |Y(d_r)| |v_r|      the basis value itself.  Measured on an MI355X, worst over the worlds 1..3:
#                               3.34, 5.25, 4.05e5, 5.91e3 at active degrees 0, 1, 2, 3.  At degrees 0 and 1 |Y| has no
#                               cancellation and this is the unit to read.  At degree >= 2 it cannot serve: bases such as
#                               x^2 - y^2 or 2 z^2 - x^2 - y^2 cancel, and next to their zeros ANY fp32 evaluation is
#                               off by thousands of E |Y| (a numpy fp32 restatement of the same sum on 700 rows: 3.3,
#                               5.3, 3.1e3, 8.3e3) -- the figures above say how close a row came to a zero, not how
#                               well the kernel computes.
#   E sum_r |Y|_r |v_r|         with every monomial of Y in absolute value (_sh_basis_magnitude; = |Y(d)| at degrees 0
#                               and 1): the size of the terms an evaluation adds up.  Measured on an MI355X: 3.34,
#                               5.25, 7.35, 8.95 at degrees 0..3 (the fp32 restatement: 3.3, 5.3, 9.1, 8.5).
#
# dg of check_step is in the second unit.  Worst measured ratio 8.95 (K 16, degree 3, world 3); C_SH = 4 x that, for
# other directions and colour gradients than the ones drawn here.  A measured ratio above SH_RATIO_CEILING is a finding
# about the kernel, not a tolerance to adopt: the test asserts it for every case.
C_SH = 36.0
SH_RATIO_CEILING = 16.0


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _make(dev, N, K, state, t=0):
    """GaussianParams + FusedAdam filled directly from (p, g, m, v) float32 [total]; optimizer at step count t."""
    from touch_gs_amd.optim import FusedAdam, GaussianParams
    p, g, m, v = state
    gp = GaussianParams.allocate(N, K, dev)
    assert gp.flat.numel() == p.size
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


def _assert_pads_zero(N, K, after):
    pads = A.pad_mask(N, K)
    for x, name in zip(after, ("p", "m", "v")):
        assert not x[pads].any(), f"a pad of {name} became non-zero"


def _checked_step(opt, N, K, g, grad_scale, lr):
    """opt.step() between two snapshots, against the oracle (dg = 0) and with the pads still exactly 0."""
    before = _snap(opt)
    opt.step(grad_scale)
    after = _snap(opt)
    r = A.check_step(before, after, g, 0.0, lr, A.consts(opt.t, opt.betas, opt.eps), grad_scale, layout=(N, K),
                     launch=(0, before[0].size, A.MAX_BLOCKS))
    _assert_pads_zero(N, K, after)
    return r


SMALL = [(N, K) for N in (1, 5, 1001, 1002, 1003, 4100) for K in (1, 4, 9, 16)] + [(1003, 0)]


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 3])
@pytest.mark.parametrize("N,K", SMALL)
def test_adam_step_small_shapes(dev, N, K, grad_scale):
    """tgs_adam_step through FusedAdam.step: every pad pattern (N = 0..3 mod 4), SH rows of 3, 12, 27 and 48 floats (and
    none), one and several blocks; steps 1, 2, 3 from a zero state with a fresh stratified gradient each, then step
    30 000 on stratified moments."""
    rng = np.random.default_rng(1000 * N + K)
    lr = A.lr_map(N, K, LRS)
    gp, opt = _make(dev, N, K, A.stratified_state(N, K, rng, zero_moments=True))
    worst = {}
    for t in (1, 2, 3):
        if t > 1:
            gp.grad.copy_(torch.from_numpy(A.stratified_state(N, K, rng)[1]))
        r = _checked_step(opt, N, K, gp.grad.cpu().numpy(), grad_scale, lr)
        assert opt.t == t
        worst = {k: max(worst.get(k, 0.0), x) for k, x in r.items()}
    p, g, m, v = A.stratified_state(N, K, rng)
    gp.grad.copy_(torch.from_numpy(g))
    opt.exp_avg.copy_(torch.from_numpy(m))
    opt.exp_avg_sq.copy_(torch.from_numpy(v))
    opt.t = 29_999
    r = _checked_step(opt, N, K, g, grad_scale, lr)
    assert opt.t == 30_000
    worst = {k: max(worst.get(k, 0.0), x) for k, x in r.items()}
    print(f"N {N} K {K} scale {grad_scale:.3f}: worst ratios in E " + ", ".join(f"{k} {x:.2f}" for k, x in sorted(worst.items())))


@pytest.mark.parametrize("N,K", [(71_111, 16), (110_401, 9), (220_003, 4), (300_001, 1)])
def test_adam_step_grid_stride(dev, N, K):
    """The smallest models beyond 4096 blocks of 256 float4: the launch grid-strides, and the lowest lanes run a
    second iteration at the end of the SH segment.  One step from a non-zero state.  These lanes spent the first
    iteration in the means, so they take their column in the SH row from the modulo: the advance by row_step is not
    reached here (tests/test_cpu_adam_ref.py::test_whole_model_launches_just_beyond_one_iteration_do_not_read_row_step)
    but in test_adam_step_grid_stride_inside_sh."""
    total = A.segments(N, K)[1]
    assert total > GRID_STRIDE_BEYOND
    rng = np.random.default_rng(N)
    state = A.stratified_state(N, K, rng)
    gp, opt = _make(dev, N, K, state, t=2)
    r = _checked_step(opt, N, K, state[1], 0.125, A.lr_map(N, K, LRS))
    print(f"N {N} K {K}: worst ratios in E " + ", ".join(f"{k} {x:.2f}" for k, x in sorted(r.items())))


@pytest.mark.parametrize("N,K", A.GRID_STRIDE_SH)
def test_adam_step_grid_stride_inside_sh(dev, N, K):
    """step_range over the SH segment alone, where that is more than one grid-stride iteration (4096 blocks of 256
    float4): more than 10 000 threads are inside the segment in two successive iterations and advance their column in
    the row by row_step (16, 16, 4 for rows of 48, 27, 12 floats) instead of recomputing it.  With row_step off by one
    this launch gives two columns of every row of the second iteration the wrong rate
    (tests/test_cpu_adam_ref.py::test_row_step_is_live_in_the_grid_stride_launches).  One step from a non-zero state
    inside the range; everything in front of it keeps its bits."""
    segs, total = A.segments(N, K)
    b, e = segs[4][1], total
    assert e - b > GRID_STRIDE_BEYOND + 40_000 and GRID_STRIDE_BEYOND % (3 * K) == {16: 16, 9: 16, 4: 4}[K]
    state = A.stratified_state(N, K, np.random.default_rng(N), only=(b, e))
    _, opt = _make(dev, N, K, state, t=2)
    before = _snap(opt)
    opt.begin_step()
    opt.step_range(b, e, 0.125)
    after = _snap(opt)
    for x, y in zip(before, after):
        assert np.array_equal(x[:b].view(np.int32), y[:b].view(np.int32))
    cut = lambda bufs: tuple(x[b:e] for x in bufs)
    r = A.check_step(cut(before), cut(after), state[1][b:e], 0.0, A.lr_map(N, K, LRS)[b:e], A.consts(3), 0.125,
                     layout=(N, K), base=b, launch=(b, e, A.MAX_BLOCKS))
    _assert_pads_zero(N, K, after)
    print(f"N {N} K {K}: worst ratios in E " + ", ".join(f"{k} {x:.2f}" for k, x in sorted(r.items())))


@pytest.mark.parametrize("N,K", [(1003, 9), (110_401, 9)])
def test_adam_step_ranges(dev, N, K):
    """step_range over a partition of [0, total) at multiples of 4 that are no multiples of the SH row -- one inside the
    scales, two inside the SH block -- is bit for bit the one-call step, and every call leaves the elements outside
    its range bitwise alone."""
    segs, total = A.segments(N, K)
    o_scales, o_sh = segs[1][1], segs[4][1]
    mid = o_sh + 4 * ((3 * K * N // 2) // 4)
    while (mid - o_sh) % (3 * K) == 0:
        mid += 4
    cuts = [0, o_scales + 20, o_sh + 28, mid, total]
    assert all(c % 4 == 0 for c in cuts) and cuts == sorted(cuts)
    assert all(c % (3 * K) != 0 and (c - o_sh) % (3 * K) != 0 for c in cuts[1:-1])
    state = A.stratified_state(N, K, np.random.default_rng(N + 1))
    lr = A.lr_map(N, K, LRS)
    _, one = _make(dev, N, K, state, t=4)
    before = _snap(one)
    one.step(1.0 / 3)
    A.check_step(before, _snap(one), state[1], 0.0, lr, A.consts(5), 1.0 / 3, layout=(N, K))
    _, rng_opt = _make(dev, N, K, state, t=4)
    rng_opt.begin_step()
    bufs = lambda o: (o.p.flat, o.exp_avg, o.exp_avg_sq)
    for b, e in reversed(list(zip(cuts[:-1], cuts[1:]))):      # back to front: the order must not matter either
        prev = [x.clone() for x in bufs(rng_opt)]
        rng_opt.step_range(b, e, 1.0 / 3)
        for x, y, z in zip(bufs(rng_opt), prev, bufs(one)):
            assert _same_bits(x[:b], y[:b]) and _same_bits(x[e:], y[e:]), (b, e)
            assert _same_bits(x[b:e], z[b:e]), (b, e)
    for x, z in zip(bufs(rng_opt), bufs(one)):
        assert _same_bits(x, z)


def test_adam_step_guard(dev):
    """skip_if_overflow: with the overflow flag of the status word set nothing is written; with it clear the launch
    is the unguarded one."""
    N, K = 1003, 9
    state = A.stratified_state(N, K, np.random.default_rng(3))
    _, plain = _make(dev, N, K, state, t=1)
    plain.step(1.0 / 3)
    _, guarded = _make(dev, N, K, state, t=1)
    prev = [x.clone() for x in (guarded.p.flat, guarded.exp_avg, guarded.exp_avg_sq)]
    guarded.step(1.0 / 3, guard=torch.tensor([7, 1], dtype=torch.int32, device=dev))
    for x, y in zip((guarded.p.flat, guarded.exp_avg, guarded.exp_avg_sq), prev):
        assert _same_bits(x, y)
    guarded.t -= 1
    guarded.step(1.0 / 3, guard=torch.tensor([7, 0], dtype=torch.int32, device=dev))
    for x, y in zip((guarded.p.flat, guarded.exp_avg, guarded.exp_avg_sq), (plain.p.flat, plain.exp_avg, plain.exp_avg_sq)):
        assert _same_bits(x, y)
    A.check_step(tuple(state[i] for i in (0, 2, 3)), _snap(guarded), state[1], 0.0, A.lr_map(N, K, LRS), A.consts(2),
                 1.0 / 3, layout=(N, K))


@pytest.mark.parametrize("t", [1, 30_000])
def test_adam_step_device_bias_corrections(dev, t):
    """TgsAdamSpec.device_bias_corr ({bias_corr1, bias_corr2, lr_means} read by the kernel) gives the bits of the host
    fields: the same IEEE division and square root on both sides."""
    N, K = 1003, 16
    state = A.stratified_state(N, K, np.random.default_rng(t))
    _, host = _make(dev, N, K, state, t=t - 1)
    host.step(0.125)
    _, devc = _make(dev, N, K, state, t=t - 1)
    devc.begin_step()
    devc.upload_bias_corr()
    devc.use_device_bias_corr = True
    assert devc._spec().device_bias_corr is not None
    devc.step_range(0, -1, 0.125)
    for x, y in zip((devc.p.flat, devc.exp_avg, devc.exp_avg_sq), (host.p.flat, host.exp_avg, host.exp_avg_sq)):
        assert _same_bits(x, y)
    A.check_step(tuple(state[i] for i in (0, 2, 3)), _snap(devc), state[1], 0.0, A.lr_map(N, K, LRS), A.consts(t),
                 0.125, layout=(N, K))
    _assert_pads_zero(N, K, _snap(devc))


# ---------------------------------------------------------------------------------------------------------------------
# Adam on the SH rows from all-gathered colour gradients
# ---------------------------------------------------------------------------------------------------------------------
def _sh_basis_magnitude(deg, d):
    """oracle.sh_basis with every monomial in absolute value: the size of the terms an evaluation of Y adds up."""
    x, y, z = d[:, 0].abs(), d[:, 1].abs(), d[:, 2].abs()
    out = [torch.full_like(x, O.SH_C0)]
    if deg >= 1:
        out += [O.SH_C1 * y, O.SH_C1 * z, O.SH_C1 * x]
    if deg >= 2:
        xx, yy, zz = x * x, y * y, z * z
        c = [abs(t) for t in O.SH_C2]
        out += [c[0] * x * y, c[1] * y * z, c[2] * (2 * zz + xx + yy), c[3] * x * z, c[4] * (xx + yy)]
    if deg >= 3:
        c = [abs(t) for t in O.SH_C3]
        out += [c[0] * y * (3 * xx + yy), c[1] * x * y * z, c[2] * y * (4 * zz + xx + yy), c[3] * z * (2 * zz + 3 * xx + 3 * yy),
                c[4] * x * (4 * zz + xx + yy), c[5] * z * (xx + yy), c[6] * x * (xx + 3 * yy)]
    return torch.stack(out, dim=1)


def _sh_gradient_ref(means, blocks, rows, K, deg):
    """fp64 sum_r Y(normalize(mean - campos_r)) (x) v_color_r over the ranks' blocks [world, 3 n + 4] for the model rows
    [rows[0], rows[1]) -> (gradient, sum_r |Y|_r |v_r| with the monomials of Y in absolute value, sum_r |Y(d_r)| |v_r|),
    all [n, K, 3] with zeros above the active degree."""
    b, e = rows
    n = e - b
    mu = torch.from_numpy(means[b:e].astype(np.float64))
    G = torch.zeros(n, K, 3, dtype=torch.float64)
    Gabs, GabsY = torch.zeros_like(G), torch.zeros_like(G)
    Ka = (deg + 1) ** 2
    for blk in blocks:
        v = torch.from_numpy(blk[:3 * n].astype(np.float64)).view(n, 3)
        campos = torch.from_numpy(blk[3 * n:3 * n + 3].astype(np.float64))
        d = mu - campos
        d = d / d.norm(dim=1, keepdim=True)
        Y, Ymag = O.sh_basis(deg, d), _sh_basis_magnitude(deg, d)
        assert (Y.abs() <= Ymag * (1 + 1e-12)).all() and (deg > 1 or torch.equal(Y.abs(), Ymag))
        G[:, :Ka] += Y[:, :, None] * v[:, None, :]
        Gabs[:, :Ka] += Ymag[:, :, None] * v.abs()[:, None, :]
        GabsY[:, :Ka] += Y.abs()[:, :, None] * v.abs()[:, None, :]
    return G.numpy(), Gabs.numpy(), GabsY.numpy()


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("K,deg", [(4, 0), (4, 1), (16, 0), (16, 2), (16, 3)])
def test_gathered_sh_adam(dev, K, deg, world):
    """tgs_adam_step_sh_gathered_rows, called directly on hand-built blocks (stratified colour gradients, a distinct
    camera position per rank behind them, grad_scale 1 / world): the whole model (blocks of 256, 256 and 188 rows) at
    step 1 from a zero state, then rows (256, 700) at step 3 on a fresh non-zero state.  The SH segment satisfies
    check_step against the fp64 gradient; the geometry segments and the SH rows outside ``rows`` keep their bits.
    Degrees 0 and 2 finish a partial float4 of the row."""
    N = 700
    rng = np.random.default_rng(100 * K + 10 * deg + world)
    segs, total = A.segments(N, K)
    o_sh = segs[4][1]
    lr = A.lr_map(N, K, LRS)[o_sh:o_sh + 3 * K * N]
    s = 1.0 / world
    worst = worst_y = 0.0
    for rows, t, zero in (((0, N), 1, True), ((256, N), 3, False)):
        state = list(A.stratified_state(N, K, rng, zero_moments=zero))
        state[0][:3 * N] = rng.standard_normal(3 * N).astype(np.float32)          # means: a unit cloud at the origin
        gp, opt = _make(dev, N, K, state, t=t - 1)
        n = rows[1] - rows[0]
        blocks = np.zeros((world, 3 * n + 4), dtype=np.float32)
        for r in range(world):
            blocks[r, :3 * n] = A.stratified(3 * n, rng).astype(np.float32)
            blocks[r, 3 * n:3 * n + 3] = (6.0 + 1.5 * r, -4.0 + 2.5 * r, 5.0 - 3.0 * r)
        G, Gabs, GabsY = _sh_gradient_ref(state[0][:3 * N].reshape(N, 3), blocks, rows, K, deg)
        before = _snap(opt)
        opt.begin_step()
        opt.step_sh_gathered(world, deg, torch.from_numpy(blocks).to(dev), s, rows=None if rows == (0, N) else rows)
        after = _snap(opt)
        lo, hi = o_sh + 3 * K * rows[0], o_sh + 3 * K * rows[1]
        for x, y in zip(before, after):
            assert np.array_equal(x[:lo].view(np.int32), y[:lo].view(np.int32))       # geometry, rows in front
            assert np.array_equal(x[hi:].view(np.int32), y[hi:].view(np.int32))
        cut = lambda bufs: tuple(x[lo:hi] for x in bufs)
        if zero:    # the kernel's own gradient, read off its first moment
            gk = after[1][lo:hi].astype(np.float64) / ((1.0 - A.f32(0.9)) * A.f32(s))
            ref, scale = G.reshape(-1), Gabs.reshape(-1)
            ratio = np.abs(gk - ref)[scale > 0] / (A.E * scale[scale > 0])
            worst = max(worst, float(ratio.max()))
            scale_y = GabsY.reshape(-1)
            worst_y = max(worst_y, float((np.abs(gk - ref)[scale_y > 0] / (A.E * scale_y[scale_y > 0])).max()))
            assert not gk[scale == 0].any()
        A.check_step(cut(before), cut(after), G.reshape(-1), C_SH * A.E * Gabs.reshape(-1), lr[lo - o_sh:hi - o_sh],
                     A.consts(t), s, layout=(N, K), base=lo)
    print(f"K {K} deg {deg} world {world}: SH gradient within {worst:.2f} E sum |Y| |v| of fp64 (C_SH {C_SH}); "
          f"{worst_y:.3g} in units of E sum |Y(d)| |v|")
    assert worst <= SH_RATIO_CEILING


# ---------------------------------------------------------------------------------------------------------------------
# fused K8+Adam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "front_prefetch"])
@pytest.mark.parametrize("deg,interval", [(3, 0), (1, 0), (3, 1000)])
def test_fused_backward_adam_is_self_consistent(dev, deg, interval, form):
    """The fused K8+Adam kernel on the scene of test_fused_backward_adam_equals_separate_kernels, two steps: every
    element of (params, exp_avg, exp_avg_sq) satisfies check_self_consistent (step 1 from a zero state: v1 =
    (1 - b2) (m1 / (1 - b1))^2 to 16E and the update that belongs to them); SH rows above the active degree keep
    m = v = 0 and their parameter bits; pads stay 0.  ``front_prefetch`` arms the next view, so the launch is
    tgs_project_bwd_adam_next_front; the colour-prefetch form between the two is tied to both bit for bit by
    tests/test_gpu_api_surfaces.py::test_color_prefetch_is_bit_identical and ::test_front_prefetch_is_bit_identical."""
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_view, synthetic_gaussians
    N, W, H = 4100, 160, 96
    K = (deg + 1) ** 2
    views = [make_view(N, W, H, deg, 7, dev, view=v, n_views=4) for v in range(2)]
    P, _ = synthetic_gaussians(N, W, H, deg, 99)
    params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
    m = DepthGaussianSplattingModel(ModelConfig(sh_degree=deg, sh_degree_interval=interval), params)
    m.fuse_adam = True
    opt = m.optimizer
    segs, total = A.segments(N, K)
    o_sh = segs[4][1]
    for step in range(2):
        adeg = m.active_sh_degree()
        assert opt.can_fuse_with_backward(adeg) and adeg == (0 if interval else deg)
        before = _snap(opt)
        if form == "front_prefetch":
            assert m.front_prefetch
            m.train_step(views[step], next_view=views[1 - step])
            assert m._prefetch_ready is not None and m._prefetch_ready.front_issued
        else:
            m.train_step(views[step])
        after = _snap(opt)
        assert opt.t == step + 1 and not np.array_equal(before[0], after[0])
        if step == 0:
            assert not before[1].any() and not before[2].any()
        lr = A.lr_map(N, K, opt.lrs)
        r = A.check_self_consistent(before, after, lr, A.consts(opt.t, opt.betas, opt.eps), layout=(N, K))
        _assert_pads_zero(N, K, after)
        sh = lambda x: x[o_sh:o_sh + 3 * K * N].reshape(N, 3 * K)[:, 3 * (adeg + 1) ** 2:]
        assert not sh(after[1]).any() and not sh(after[2]).any()
        assert np.array_equal(sh(before[0]).view(np.int32), sh(after[0]).view(np.int32))
        assert np.count_nonzero(after[1]) > N          # the step did reach most Gaussians
        print(f"deg {deg} interval {interval} {form} step {step + 1}: worst ratios in E "
              + ", ".join(f"{k} {x:.2f}" for k, x in sorted(r.items())))
