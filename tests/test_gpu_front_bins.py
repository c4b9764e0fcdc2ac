"""Direct bins (tgs.h: tgs_bins_len and the _bins entry points; csrc/tgs_binning.h group_count_tiles<true>, csrc/binning.hip
PairSrc<true>): K1 stores every (Gaussian, tile) pair in a fixed-capacity bin of its (XCC, tile) and the sorts gather each
list from the tile's 8 sub-bins -- no fill pass.  Every output must be what the fill path gives, bit for bit: the sort keys
(depth bits, gid) are unique, so a sorted list does not depend on where its unsorted pairs came from.

1. Built records (tests/binning_cases.py) through ``tgs_bin_sort_bins`` -- the counting code of the fused K1 and the gathering
   sorts, driven from records -- against the same frame through ``tgs_bin_sort``, and against the exact reference.
2. The capacity edge: ``cap`` = the longest list is valid, one less voids the frame; nothing outside the bins is written.
3. Train steps with ``next_view`` (the production path: K1 inside the fused optimizer kernel, ``tgs_project_bin_sort_front_bins``)
   are byte-identical with the bins on and off, also across a forced overflow; without a list bound or with the bins over the
   ceiling the fill path runs.
4. Two models at different resolutions in one process keep their own bins.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import binning_cases as B
from tests import test_gpu_binning_oracle as O

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# 1. built records: the bins against the fill path
# ---------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 64, 65, 128, 129, 512, 513, 1024, 1025, 4096)     # every class of the wave and the wg4 launch


def lists_frame(W, H, seed):
    """One list of every length in LENGTHS on tiles spread over the image (the last tile among them); 1 x 1 rects, rows
    shuffled over the groups, every third depth tied."""
    TW, TH = (W + 15) // 16, (H + 15) // 16
    T = TW * TH
    tiles = [int(round(i * (T - 1) / (len(LENGTHS) - 1))) for i in range(len(LENGTHS))]
    assert len(set(tiles)) == len(LENGTHS) and tiles[-1] == T - 1
    return B.lists_case(W, H, dict(zip(tiles, LENGTHS)), seed)


def rows_frame(N, seed, pattern):
    """N rows of small rects on the 4 x 3 tiles of a 64 x 48 image: a partial last group, and (N = 700) a middle group
    whose records have no tiles at all."""
    rng = np.random.default_rng(seed)
    TW, TH = 4, 3
    w, h = rng.integers(1, TW + 1, N), rng.integers(1, TH + 1, N)
    x, y = rng.integers(0, TW - w + 1), rng.integers(0, TH - h + 1)
    rects = np.stack([x, y, w, h], 1)
    if N > 512:
        rects[256:512, 2:] = 0
    bits = B.tied(N, seed) if pattern == "tied" else B.depths(pattern, N, seed)
    return B.Case(64, 48, rects, bits, B.LONG_RUN, {})


def built(name):
    kind, _, arg = name.partition(":")
    if kind == "case":
        return B.get(arg)[0]
    if kind == "lists":
        W, H = (int(v) for v in arg.split("x"))
        return lists_frame(W, H, 71)
    N, pattern = arg.split("-")
    return rows_frame(int(N), 80 + int(N), pattern)


FRAMES = ["lists:64x48", "lists:272x272",
          "rows:1-tied", "rows:255-tied", "rows:256-ulp_neighbours", "rows:257-all_equal", "rows:700-tied", "rows:700-ulp_neighbours",
          # depth ties and 1-ulp neighbours inside one long list; members on both sides of long_run (aggregated and direct
          # counting in one group); groups whose every pair is counted directly; one counter that takes every atomic
          "case:one_tile-1025-ulp_neighbours", "case:one_tile-4096-two_values", "case:runs-32", "case:runs-1", "case:all_long",
          "case:long_and_invisible", "case:total-2049", "case:box-25x41", "case:hot_tile", "case:empty_group_between"]


def fill_path(c, dev, hint=-1, sticky=True):
    ref = B.reference(c.rects, c.depth_bits, *B.tiles_of(c))
    b = O.buffers(c, ref.need + 1000, dev, sticky)
    return ref, b, O.call(c, b, hint)


def bins_path(c, capacity, cap, dev, hint=-1, sticky=True):
    """The frame through tgs_bin_sort_bins, the bins exactly tgs_bins_len entries long with a sentinel tail."""
    L = O.lib()
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    n = L.tgs_bins_len(T, cap)
    assert n == 8 * T * cap
    b = O.buffers(c, capacity, dev, sticky)
    b.bins = O.Buf(2 * n, dev)
    cs = O.camera(c).c_struct()
    rc = L.tgs_bin_sort_bins(C.byref(cs), b.N, b.splats.ptr(), b.group_base.ptr(), b.tile_start.ptr(), b.tile_start.n,
                             b.tile_cursor.ptr(), b.sorted_gid.ptr(), b.tile_order.ptr(), b.capacity, b.scratch.ptr(),
                             b.status.ptr(), b.sticky.ptr() if b.sticky else None, hint, b.bins.ptr(), n, cap,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, L.tgs_last_error().decode(errors="replace")
    for name in ("splats", "group_base", "tile_start", "tile_cursor", "sorted_gid", "tile_order", "scratch", "status", "sticky", "bins"):
        buf = getattr(b, name)
        assert buf is None or buf.tail_ok(), f"{name}: the sentinel behind the buffer was overwritten"
    return b, b.status.body().tolist()


def assert_same_frame(c, ref, a, b):
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    assert torch.equal(a.status.w, b.status.w), (a.status.body(), b.status.body())
    assert torch.equal(a.tile_start.w[:T + 1], b.tile_start.w[:T + 1])
    assert torch.equal(a.sorted_gid.w[:ref.n], b.sorted_gid.w[:ref.n])
    assert torch.equal(a.tile_order.w, b.tile_order.w)
    assert torch.equal(a.splats.w, b.splats.w)


@pytest.mark.parametrize("name", FRAMES)
def test_lists_and_status_equal_the_fill_path(dev, name):
    c = built(name)
    ref, a, status = fill_path(c, dev)
    assert status == [ref.n, 0, ref.need, ref.longest]
    cap = max(ref.longest, 1)
    # the list bound as the caller's hint too: the sort classes it selects are the ones the fill path gets with that hint
    _, a_hint, status_hint = fill_path(c, dev, hint=cap)
    assert status_hint == status
    b, got = bins_path(c, ref.need + 1000, cap, dev, hint=cap)
    assert got == status and b.sticky.body().tolist() == [0]
    assert_same_frame(c, ref, a, b)
    assert_same_frame(c, ref, a_hint, b)
    O.assert_frame(c, ref, b, got)                     # ... and the exact reference itself
    # no hint: the bins' capacity bounds the classes
    b2, got2 = bins_path(c, ref.need + 1000, cap, dev, hint=-1)
    assert got2 == status
    assert_same_frame(c, ref, a, b2)


def test_second_frame_in_the_same_bins(dev):
    """The bins are never cleared: a frame with short lists after one with long lists in the same buffers."""
    L = O.lib()
    big, small = built("lists:64x48"), built("rows:700-tied")
    ref_b = B.reference(big.rects, big.depth_bits, *B.tiles_of(big))
    ref_s, a, status = fill_path(small, dev)
    cap = ref_b.longest
    bb, got_b = bins_path(big, ref_b.need + 1000, cap, dev)
    assert got_b == [ref_b.n, 0, ref_b.need, ref_b.longest]
    bs = O.buffers(small, ref_s.need + 1000, dev, True)
    cs = O.camera(small).c_struct()
    rc = L.tgs_bin_sort_bins(C.byref(cs), bs.N, bs.splats.ptr(), bs.group_base.ptr(), bs.tile_start.ptr(), bs.tile_start.n,
                             bs.tile_cursor.ptr(), bs.sorted_gid.ptr(), bs.tile_order.ptr(), bs.capacity, bs.scratch.ptr(),
                             bs.status.ptr(), bs.sticky.ptr(), -1, bb.bins.ptr(), bb.bins.n // 2, cap,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and bb.bins.tail_ok()
    assert bs.status.body().tolist() == status
    assert_same_frame(small, ref_s, a, bs)


# ---------------------------------------------------------------------------------------------
# 2. the capacity edge
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["case:one_tile-65-distinct", "case:hot_tile", "lists:64x48"])
def test_cap_of_the_longest_list_is_valid_and_one_less_voids_the_frame(dev, name):
    c = built(name)
    ref, a, status = fill_path(c, dev)
    b, got = bins_path(c, ref.need + 1000, ref.longest, dev)
    assert got == status and b.sticky.body().tolist() == [0]
    assert_same_frame(c, ref, a, b)
    # one entry short: a sub-list that outgrew its bin dropped pairs (K1 voids the frame: empty lists), or every sub-list
    # fitted and the sort refused the list (unsorted ids) -- which, depends on where the groups ran; void either way, and
    # bins_path has checked the sentinel behind the bins
    v, got = bins_path(c, ref.need + 1000, ref.longest - 1, dev)
    assert got[1] == 1 and v.sticky.body().tolist() == [1]
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    ts = v.tile_start.body()[:T + 1]
    if ts.any():                                         # the sort's verdict: every list is a permutation of its ids
        assert got[3] == ref.longest                     # (K1's verdict empties the lists before the scan measures them)
        assert np.array_equal(ts.astype(np.int64), ref.tile_start)
        sg = v.sorted_gid.body()
        for t in range(T):
            assert np.array_equal(np.sort(sg[ts[t]:ts[t + 1]]), np.sort(ref.sorted_gid[ts[t]:ts[t + 1]])), t
    else:
        assert (v.sorted_gid.body() == O.PRE).all()


# ---------------------------------------------------------------------------------------------
# 3. / 4. the train step
# ---------------------------------------------------------------------------------------------
N_G, W_, H_, DEG = 3000, 160, 96, 3


@pytest.fixture(scope="module")
def scene(dev):
    from touch_gs_amd import ops
    from touch_gs_amd.optim import GaussianParams
    from touch_gs_amd.scene import make_view, synthetic_gaussians
    out = {}
    for W, H in ((W_, H_), (96, 64)):
        views = [make_view(N_G, W, H, DEG, 7, dev, view=v, n_views=3) for v in range(3)]
        P, _ = synthetic_gaussians(N_G, W, H, DEG, 99)
        params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
        longest = 0
        for v in views:
            sp = ops.project_fwd(v.cam, params.means, params.log_scales, params.quats, params.opac_logit, params.sh, DEG)
            b = ops.IntersectBudget()
            ops.bin_sort(v.cam, sp, b)
            longest = max(longest, b.last_longest)
        out[(W, H)] = (views, P, int(1.25 * longest) + 32)
    return out


@pytest.fixture
def bins_switch():
    from touch_gs_amd import ops
    was = ops.set_front_bins()
    yield ops.set_front_bins
    ops.set_front_bins(*was)


class Spy:
    """Counts the frames that got bins, and keeps every frame's lists as project_bin_sort returned them."""

    def __init__(self, monkeypatch):
        from touch_gs_amd import ops
        self.attached, self.frames = [], []
        attach, pbs = ops.FrontBuffers.attach_bins, ops.project_bin_sort

        def attach_bins(fb, hint):
            self.attached.append((attach(fb, hint), fb.cam.W, fb.bins.data_ptr() if fb.bins is not None else 0))
            return self.attached[-1][0]

        def project_bin_sort(cam, *a, **k):
            r = pbs(cam, *a, **k)
            splats, radii, group_base, tile_start, sorted_gid, status = r
            n = int(tile_start[cam.num_tiles])
            self.frames.append((tile_start.clone(), sorted_gid[:n].clone(), tile_start.tile_order.clone(), status.clone()))
            return r

        monkeypatch.setattr(ops.FrontBuffers, "attach_bins", attach_bins)
        monkeypatch.setattr(ops, "project_bin_sort", project_bin_sort)


def fresh_model(dev, P, hint):
    from touch_gs_amd.model import DepthGaussianSplattingModel, ModelConfig
    from touch_gs_amd.optim import GaussianParams
    params = GaussianParams.from_tensors(*[P[k].to(dev) for k in GaussianParams.NAMES])
    m = DepthGaussianSplattingModel(ModelConfig(sh_degree=DEG, sh_degree_interval=0), params)
    m.list_hint = False                       # the bound below stays as set (the trainer would learn its own after some frames)
    m.enable_speculative_budget(capacity=0, max_in_flight=3)
    m.budget.max_list_hint = hint
    return m


def train(dev, scene, steps=6, hint=None, overflow_at=None, size=(W_, H_)):
    views, P, learned = scene[size]
    m = fresh_model(dev, P, learned if hint is None else hint)
    for i in range(steps):
        if i == overflow_at:
            m.budget.capacity = 1000          # this frame overflows: the optimizer kernel is voided, the next frame's tag is stale
        m.train_step(views[i % 3], next_view=views[(i + 1) % 3])
    m.flush()
    torch.cuda.synchronize()
    return m


def assert_same_model(a, b):
    assert a.step == b.step and a.optimizer.t == b.optimizer.t
    for x, y in ((a.params.flat, b.params.flat), (a.optimizer.exp_avg, b.optimizer.exp_avg),
                 (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq), (a.last["rgb"], b.last["rgb"]),
                 (a.last["depth_acc"], b.last["depth_acc"]), (a.last["status"], b.last["status"])):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


@pytest.mark.parametrize("overflow_at", [None, 3])
def test_train_steps_are_byte_identical_with_and_without_bins(dev, scene, bins_switch, monkeypatch, overflow_at):
    spy = Spy(monkeypatch)
    bins_switch(False)
    off = train(dev, scene, overflow_at=overflow_at)
    frames_off, attached_off = spy.frames[:], spy.attached[:]
    del spy.frames[:], spy.attached[:]
    bins_switch(True)
    on = train(dev, scene, overflow_at=overflow_at)
    assert attached_off and not any(a[0] for a in attached_off)
    # every announced frame up to the overflow got bins (the replay runs without a list bound, hence without bins)
    assert sum(a[0] for a in spy.attached) >= (6 if overflow_at is None else 3), spy.attached
    assert (getattr(on, "speculative_replays", 0) > 0) == (overflow_at is not None)
    assert getattr(on, "speculative_replays", 0) == getattr(off, "speculative_replays", 0)
    assert_same_model(on, off)
    assert len(spy.frames) == len(frames_off) >= 6
    for f, g in zip(spy.frames, frames_off):             # every frame's lists, voided and replayed ones included
        for x, y in zip(f, g):
            assert torch.equal(x, y)


def test_without_a_list_bound_or_over_the_ceiling_the_fill_path_runs(dev, scene, bins_switch, monkeypatch):
    spy = Spy(monkeypatch)
    bins_switch(False)
    off = train(dev, scene, steps=4)
    del spy.attached[:]
    bins_switch(True)
    no_hint = train(dev, scene, steps=4, hint=-1)
    assert spy.attached and not any(a[0] for a in spy.attached)
    del spy.attached[:]
    bins_switch(True, 1 << 16)                           # 8 * 60 tiles * hint * 8 bytes is more
    capped = train(dev, scene, steps=4)
    assert spy.attached and not any(a[0] for a in spy.attached)
    assert_same_model(no_hint, off)
    assert_same_model(capped, off)


def test_two_models_keep_their_own_bins(dev, scene, bins_switch, monkeypatch):
    spy = Spy(monkeypatch)
    bins_switch(False)
    ref = [train(dev, scene, steps=4, size=s) for s in ((W_, H_), (96, 64))]
    bins_switch(True)
    del spy.attached[:]
    models = [fresh_model(dev, scene[s][1], scene[s][2]) for s in ((W_, H_), (96, 64))]
    for i in range(4):                                   # interleaved: each model's announced frame waits in its bins
        for m, s in zip(models, ((W_, H_), (96, 64))):
            views = scene[s][0]
            m.train_step(views[i % 3], next_view=views[(i + 1) % 3])
    for m in models:
        m.flush()
    torch.cuda.synchronize()
    assert all(a[0] for a in spy.attached) and {a[1] for a in spy.attached} == {W_, 96}
    live = [(a[1], a[2]) for a in spy.attached[-2:]]      # the two frames announced last are both alive: different buffers
    assert live[0][0] != live[1][0] and live[0][1] != live[1][1]
    for m, r in zip(models, ref):
        assert_same_model(m, r)
