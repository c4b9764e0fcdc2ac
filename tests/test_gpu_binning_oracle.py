"""K2-K5 (csrc/tgs_binning.h, csrc/binning.hip: tile count with the pair allocator, tile scan, bin fill, per-tile sort)
against the exact reference of tests/binning_cases.py, on built splat records: every list length the sort kernels branch
on, the grid-stride loops of the rare sort classes, the three switches of the counting path, the seams of the scan.

``tgs_bin_sort`` is called directly (touch_gs_amd._lib) so that every buffer can be prepared: its length is what the
library's own ``tgs_*_len`` functions ask for, its body is prefilled, and PAD words of a sentinel follow it that must be
bit-unchanged after the call.  ``capacity`` and ``max_list_hint`` are explicit.  The outputs are integers and every
comparison is exact; K1 and the rasterizer never run here.  The fused production path calls the same functions and
tests/test_gpu_parity.py::test_fused_project_bin_sort_equals_separate_calls ties it bit for bit to this entry point.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import binning_cases as B

pytestmark = pytest.mark.gpu

PAD = 64
PRE = 0x5A5A5A5A                 # the prefill of every output buffer
SENT = 0x4B3C614E                # the tail
XCC = 8                          # pair regions (TGS_XCC)
SCRATCH = 512                    # TGS_TILE_START_SCRATCH


# offsets of the rasterizer's words behind the T + 1 tile starts, from the formulas of csrc/tgs_common.h
def walk_at(T, x):
    return T + 1 + 64 * x


def walksum_at(T, x):
    return T + 1 + 64 * x + 1


def slotctr_at(T, x):
    return T + 1 + 64 * x + 32


class Buf:
    """``n`` int32 words of ``fill`` followed by PAD words of the sentinel."""

    def __init__(self, n, dev, fill=PRE):
        self.n = int(n)
        self.w = torch.full((self.n + PAD,), fill, dtype=torch.int32, device=dev)
        self.w[self.n:] = SENT

    def ptr(self):
        return self.w.data_ptr()

    def tail_ok(self):
        return bool((self.w[self.n:] == SENT).all())

    def body(self):
        return self.w[:self.n].cpu().numpy()


def lib():
    from touch_gs_amd import _lib
    return _lib.load()


def camera(c):
    from touch_gs_amd import Camera
    return Camera(np.eye(4), 1.0, 1.0, 0.0, 0.0, c.W, c.H, long_run=c.long_run)


def buffers(c, capacity, dev, sticky=False):
    """Every buffer of one tgs_bin_sort call, sized by the library's own length functions."""
    L = lib()
    N = len(c.rects)
    b = types.SimpleNamespace(N=N, capacity=int(capacity), G=L.tgs_num_groups(N))
    assert b.G == (N + 255) // 256
    b.records = B.records(c.rects, c.depth_bits)
    b.splats = Buf(12 * N, dev)
    b.splats.w[:12 * N] = b.records.view(torch.int32).reshape(-1).to(dev)
    b.group_base = Buf(b.G, dev)
    b.tile_start = Buf(L.tgs_tile_start_len(c.W, c.H), dev)
    b.tile_cursor = Buf(L.tgs_tile_counter_len(c.W, c.H), dev)
    b.sorted_gid = Buf(capacity, dev)
    b.tile_order = Buf(L.tgs_tile_order_len(c.W, c.H), dev)
    nbytes = L.tgs_sort_scratch_bytes(capacity)
    assert nbytes % 4 == 0
    b.scratch = Buf(nbytes // 4, dev)
    b.status = Buf(4, dev)
    b.sticky = Buf(1, dev, fill=0) if sticky else None
    return b


def call(c, b, hint=-1):
    """One tgs_bin_sort on the buffers ``b`` -> status[4]; every sentinel checked."""
    cs = camera(c).c_struct()
    rc = lib().tgs_bin_sort(C.byref(cs), b.N, b.splats.ptr(), b.group_base.ptr(), b.tile_start.ptr(), b.tile_start.n,
                            b.tile_cursor.ptr(), b.sorted_gid.ptr(), b.tile_order.ptr(), b.capacity, b.scratch.ptr(),
                            b.status.ptr(), b.sticky.ptr() if b.sticky else None, hint,
                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib().tgs_last_error().decode(errors="replace")
    for name in ("splats", "group_base", "tile_start", "tile_cursor", "sorted_gid", "tile_order", "scratch", "status", "sticky"):
        buf = getattr(b, name)
        assert buf is None or buf.tail_ok(), f"{name}: the sentinel behind the buffer was overwritten"
    return b.status.body().tolist()


def run(name, dev, capacity=None, hint=-1, sticky=False):
    c, ref = B.get(name)
    b = buffers(c, ref.need if capacity is None else capacity, dev, sticky)
    return c, ref, b, call(c, b, hint)


def assert_records(c, ref, b):
    """Slot 11 of the records with tiles = the in-group offset; every other slot bit-unchanged."""
    got = b.splats.body().reshape(-1, 12)
    want = b.records.view(torch.int32).numpy()
    other = [s for s in range(12) if s != 11]
    assert np.array_equal(got[:, other], want[:, other]), "a record slot other than 11 changed"
    vis = (c.rects[:, 2] * c.rects[:, 3]) > 0
    assert np.array_equal(got[vis, 11].astype(np.int64), ref.offset[vis])


def assert_frame(c, ref, b, status):
    """Everything a valid frame promises, exactly."""
    TW, TH = B.tiles_of(c)
    T = TW * TH
    assert status == [ref.n, 0, ref.need, ref.longest]
    ts = b.tile_start.body()
    assert np.array_equal(ts[:T + 1].astype(np.int64), ref.tile_start)
    sg = b.sorted_gid.body()
    assert np.array_equal(sg[:ref.n].astype(np.int64), ref.sorted_gid)
    assert (sg[ref.n:] == PRE).all(), "sorted_gid was written behind the frame's pairs"
    assert_records(c, ref, b)
    # pair ranges of the groups: disjoint, inside the capacity, each inside one XCD region
    gb = b.group_base.body().astype(np.int64)
    live = np.nonzero(ref.totals > 0)[0]
    lo, hi = gb[live], gb[live] + ref.totals[live]
    assert (lo >= 0).all() and (hi <= b.capacity).all()
    order = np.argsort(lo)
    assert (hi[order][:-1] <= lo[order][1:]).all(), "two groups share pair slots"
    if len(live):
        region = b.capacity // XCC
        assert region > 0 and np.array_equal(lo // region, (hi - 1) // region), "a pair range straddles two regions"
    # schedule: every tile once, the padding says "no tile"
    to = b.tile_order.body()
    assert b.tile_order.n >= T and np.array_equal(np.sort(to), np.concatenate([np.arange(T), np.full(b.tile_order.n - T, T)]))
    # the rasterizer's words behind the tile starts
    assert b.tile_start.n == T + 1 + SCRATCH
    for x in range(XCC):
        assert ts[walk_at(T, x)] == 0 and ts[walksum_at(T, x)] == 0 and ts[slotctr_at(T, x)] == 0, x


def assert_overflow(c, ref, b, status):
    """An overflowed frame: flagged, every list empty, status[0] = status[2] = the sufficient capacity, nothing sorted."""
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    assert status[1] == 1 and status[0] == status[2] == ref.need
    assert not b.tile_start.body()[:T + 1].any()
    assert (b.sorted_gid.body() == PRE).all()


NAMES = list(B.CASES)


# ---------------------------------------------------------------------------------------------
# every case, at the sufficient capacity exactly and at a generous one
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_at_the_sufficient_capacity_and_at_a_generous_one(dev, name):
    c, ref, b, status = run(name, dev)                      # capacity = need: must succeed
    assert_frame(c, ref, b, status)
    c, ref, b2, status2 = run(name, dev, capacity=2 * ref.need + 4099)
    assert_frame(c, ref, b2, status2)
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    assert torch.equal(b.tile_start.w[:T + 1], b2.tile_start.w[:T + 1])
    assert torch.equal(b.sorted_gid.w[:ref.n], b2.sorted_gid.w[:ref.n])


@pytest.mark.parametrize("name", ["one_tile-1025-distinct", "total-2049"])
def test_capacity_of_the_pair_count_alone_overflows_or_gives_the_lists(dev, name):
    """capacity = n < need: the contract of test_pair_allocator_when_xcd_regions_fill_up."""
    c, ref = B.get(name)
    c, ref, b, status = run(name, dev, capacity=ref.n, sticky=True)
    if status[1]:
        assert_overflow(c, ref, b, status)
        assert b.sticky.body().tolist() == [1]
        assert_records(c, ref, b)
    else:
        assert_frame(c, ref, b, status)
        assert b.sticky.body().tolist() == [0]


# ---------------------------------------------------------------------------------------------
# max_list_hint: the same list length through different kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint,n", [(1024, 512), (1024, 513), (1024, 1024),
                                    (4096, 512), (4096, 513), (4096, 1024), (4096, 1025), (4096, 2048), (4096, 2049), (4096, 4096),
                                    (16384, 16384)])
@pytest.mark.parametrize("pattern", ["distinct", "all_equal"])
def test_a_kept_hint_changes_no_bit(dev, hint, n, pattern):
    name = f"one_tile-{n}-{pattern}"
    c, ref, b0, status0 = run(name, dev, sticky=True)
    c, ref, b, status = run(name, dev, hint=hint, sticky=True)
    assert_frame(c, ref, b, status)
    assert status == status0 and b.sticky.body().tolist() == [0]
    assert torch.equal(b.sorted_gid.w, b0.sorted_gid.w) and torch.equal(b.tile_start.w[:2], b0.tile_start.w[:2])


@pytest.mark.parametrize("sticky", [False, True])
@pytest.mark.parametrize("hint,n", [(1024, 1025), (4096, 4097)])
def test_a_broken_hint_voids_the_frame(dev, hint, n, sticky):
    c, ref, b, status = run(f"one_tile-{n}-distinct", dev, hint=hint, sticky=sticky)
    assert status == [n, 1, ref.need, n]
    if sticky:
        assert b.sticky.body().tolist() == [1]
    assert b.tile_start.body()[:2].tolist() == [0, n]
    sg = b.sorted_gid.body()
    assert np.array_equal(np.sort(sg[:n]), np.arange(n)), "the void list is not a permutation of the tile's ids"
    assert (sg[n:] == PRE).all()
    assert_records(c, ref, b)


# ---------------------------------------------------------------------------------------------
# the same buffers twice, the wrapper
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed_classes", "total-2049", "runs-32", "hot_tile", "empty_group_between", "tiles-1025",
                                  "one_tile-1025-two_values"])
def test_second_call_on_the_same_buffers(dev, name):
    """Nothing is cleared by hand between the calls: counters, allocator lines, look-back flags and status are the
    library's to reset, and slot 11 of the second call's input is the first call's output."""
    c, ref, b, status = run(name, dev, capacity=B.get(name)[1].need + 1000)
    assert_frame(c, ref, b, status)
    first = b.sorted_gid.w.clone(), b.tile_start.w.clone()
    status = call(c, b)
    assert_frame(c, ref, b, status)
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    assert torch.equal(b.sorted_gid.w, first[0]) and torch.equal(b.tile_start.w[:T + 1], first[1][:T + 1])


def test_the_wrapper_equals_the_direct_call(dev):
    from touch_gs_amd import ops
    c, ref, b, status = run("mixed_classes", dev)
    sp = B.records(c.rects, c.depth_bits).to(dev)
    budget = ops.IntersectBudget()
    gb, ts, sg, st = ops.bin_sort(camera(c), sp, budget)
    torch.cuda.synchronize()
    T = B.tiles_of(c)[0] * B.tiles_of(c)[1]
    assert budget.last_status4.tolist() == status
    assert torch.equal(ts, b.tile_start.w[:T + 1]) and torch.equal(sg[:ref.n], b.sorted_gid.w[:ref.n])
    assert torch.equal(sp.view(torch.int32).reshape(-1), b.splats.w[:12 * b.N])
    assert torch.equal(torch.sort(ts.tile_order).values, torch.sort(b.tile_order.w[:b.tile_order.n]).values)
