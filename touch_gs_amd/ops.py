"""Operator layer: thin wrappers over the C ABI (include/tgs.h) + the autograd Functions.

Mirrors the operator surface the reference's training loop reaches through
``ns-train depth-gaussian-splatting`` (reference ``scripts/train_bunny_real.sh:52``):

* fused fast path  -- :func:`render` -> (rgb, depth_acc, alpha) in ONE compositing pass;
* gsplat-0.1 shaped -- :func:`project_gaussians`, :func:`rasterize_gaussians`,
  :func:`spherical_harmonics` (these are what nerfstudio's Splatfacto calls);
* INRIA shaped      -- ``touch_gs_amd.rasterizer.GaussianRasterizer`` (App. A.1).

Every op runs the HIP kernels; there is no eager/CPU fallback (tensors must be on the device).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import PARTIAL_FLOATS, SPLAT_FLOATS, check, ptr
from .camera import Camera


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# TGS_SLOT_OK=1: K6 leaves per-quadrant bitmaps of the Gaussians that changed a quadrant's state and K7
# skips the rest (bit-identical results).  OFF by default -- measured at cfg3, same box: K7 -3.3 % (-14 us)
# but K6 +5 % (+9.5 us: four scalar instructions per quadrant evaluation in a kernel that is issue-bound),
# i.e. 0.4 % of the step and a slower render-only path.
import os as _os
SLOT_OK = _os.environ.get("TGS_SLOT_OK", "0") == "1"


def _f32c(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise RuntimeError(f"expected float32, got {t.dtype}")
    return t.contiguous()


# ------------------------------------------------------------------------------------------------
# capacity management for the (tile, Gaussian) intersection buffers
# ------------------------------------------------------------------------------------------------
class IntersectBudget:
    """Remembers how many (tile, Gaussian) intersections recent frames needed.

    ``sync=True`` (default): after binning, the 8-byte status word is read back (one D2H sync per
    frame) and the frame is re-binned with a larger buffer if it overflowed -- always correct.
    ``sync=False``: no read-back; the caller must size ``capacity`` itself and call
    :meth:`check` at a convenient sync point (bench.py does this once after the timed region).
    ``speculative=True`` (implies ``sync=False``): additionally hands the kernels a persistent
    "sticky overflow" word: after an overflowing frame every later frame is empty and the guarded
    optimizer kernels are no-ops, so the caller may read the status words late, grow the buffers,
    clear the word and replay (``DepthGaussianSplattingModel.enable_speculative_budget``).
    """

    def __init__(self, capacity: int = 0, sync: bool = True, growth: float = 1.25, speculative: bool = False,
                 max_list_hint: int = -1):
        self.capacity = int(capacity)
        # the caller's bound on the longest tile list of the frames binned with this budget (tgs.h, max_list_hint):
        # -1 = none, every sort class is launched; a frame that breaks it is void like one that overflowed (sticky
        # word, replay) -- so only budgets that do NOT read the status back per frame may carry one
        self.max_list_hint = int(max_list_hint)
        self.sync = sync and not speculative
        self.speculative = speculative
        self.growth = growth
        self.last_status = None  # device int32[2] of the most recent frame: {#intersections, overflow}
        self.last_status4 = None  # ... and the full word {.., .., required capacity, reserved}
        self.last_n = None       # #intersections of the last frame that was read back
        self.last_need = None    # capacity that frame needs under the per-XCD split (>= last_n; tgs.h)
        self.last_longest = None  # longest tile list of that frame (status[3])
        self.sticky = None       # device int32[1], allocated on first use

    def sticky_word(self, device):
        """Persistent overflow word of every budget that does not read the status back (``sync=False``):
        an overflowing frame sets it, later frames start overflowed (empty lists) and the guarded
        optimizer kernels do nothing -- an undersized buffer can never feed garbage partials to Adam,
        and :meth:`check` sees an overflow of ANY earlier frame, not only of the last one."""
        if self.sync:
            return None
        if self.sticky is None:
            if torch.cuda.is_current_stream_capturing():
                # allocated inside a capture the word would live in the graph's pool and its zero-fill
                # would be a graph node: every replay would forget an earlier overflow
                raise RuntimeError("allocate the sticky overflow word (budget.sticky_word(device)) before graph capture")
            self.sticky = torch.zeros(1, dtype=torch.int32, device=device)
        return self.sticky

    def list_hint(self) -> int:
        return -1 if self.sync else self.max_list_hint

    def initial(self, N: int):
        if self.capacity <= 0:
            self.capacity = max(8 * N, 1 << 16)
        return self.capacity

    def check(self):
        """Read the last frame's status (and the sticky word, which remembers an overflow of any
        earlier frame of a ``sync=False`` budget); raises on overflow.  Returns #intersections."""
        if self.last_status is None:
            return None
        if self.last_status4 is not None:
            n, ovf, need, longest = self.last_status4.tolist()
            self.last_need = max(n, need)
            self.last_longest = longest
            if ovf and 0 <= self.max_list_hint < longest:
                raise RuntimeError(f"a tile list of {longest} entries broke max_list_hint = {self.max_list_hint}: that frame "
                                   "and every frame since were dropped (raise the hint or pass -1)")
        else:
            n, ovf = self.last_status.tolist()
        self.last_n = n
        if self.sticky is not None and int(self.sticky.item()) != 0:
            ovf = 1
        if ovf:
            # the sticky word remembers ANY earlier frame: with a list hint in force the cause may have been a list longer
            # than the hint in a frame whose status words are gone, not the capacity
            why = (f"intersection capacity {self.capacity} too small" if self.max_list_hint < 0 else
                   f"intersection capacity {self.capacity} too small, or a tile list broke max_list_hint = {self.max_list_hint} in an earlier frame")
            raise RuntimeError(f"{why}: a frame needed more (last frame: {n} intersections, longest list "
                               f"{getattr(self, 'last_longest', '?')}); every frame since was dropped")
        return n


_default_budget = IntersectBudget()


def capacity_after_refine(seen: int, old_capacity: int, n_before: int, n_after: int) -> int:
    """Capacity of a speculative budget after a refinement took N from ``n_before`` to ``n_after``: the largest capacity any
    frame since the last refinement needed (``seen``) x the growth of N (at least 1) + 25 % + 4096; nothing seen: the old
    capacity x that growth + 4096 (only then: from the old capacity every time, it would compound)."""
    ratio = max(1.0, n_after / max(n_before, 1))
    return int(seen * ratio * 1.25) + 4096 if seen > 0 else int(old_capacity * ratio) + 4096


# ------------------------------------------------------------------------------------------------
# thin wrappers (one per C entry point)
# ------------------------------------------------------------------------------------------------
def project_fwd(cam: Camera, means, log_scales, quats, opac_logit, sh, sh_deg: int, colors=None,
                want_radii: bool = False):
    """K1 -> splats [N,12] (, radii int32 [N]).  (tgs_project_fwd)"""
    lib = _lib.load()
    N = means.shape[0]
    splats = torch.empty(max(N, 1), SPLAT_FLOATS, dtype=torch.float32, device=means.device)[:N]
    radii = torch.empty(N, dtype=torch.int32, device=means.device) if want_radii else None
    cs = cam.c_struct()
    sh_stride = sh.shape[1] if sh is not None else 0
    check(lib.tgs_project_fwd(C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats), ptr(opac_logit),
                              ptr(sh), sh_stride, sh_deg if sh is not None else -1, ptr(colors),
                              ptr(splats), ptr(radii), _stream()), "tgs_project_fwd")
    return (splats, radii) if want_radii else splats


def bin_sort(cam: Camera, splats, budget: Optional[IntersectBudget] = None):
    """K2-K5 -> (group_base, tile_start, sorted_gid, status).  (tgs_bin_sort)"""
    lib = _lib.load()
    budget = budget or _default_budget
    N = splats.shape[0]
    cs = cam.c_struct()
    fb = FrontBuffers(cam, N, budget.initial(N), False, splats.device, records=False)
    while True:
        check(lib.tgs_bin_sort(C.byref(cs), N, ptr(splats), ptr(fb.group_base), ptr(fb.tile_start), _tile_start_len(fb.tile_start),
                               ptr(fb.tile_cursor), ptr(fb.sorted_gid), ptr(fb.tile_start.tile_order), fb.cap, ptr(fb.scratch),
                               ptr(fb.status), ptr(budget.sticky_word(splats.device)), budget.list_hint(), _stream()), "tgs_bin_sort")
        if not fb.settle(budget):
            return fb.group_base, fb.tile_start, fb.sorted_gid, fb.status


class ColorPrefetch:
    """Colours of the Gaussians for ONE upcoming view, evaluated by the previous step's fused optimizer
    kernel (tgs_project_bwd_adam_next) so that K1 does not re-read the 12K-byte SH rows
    (tgs_project_bin_sort_colors).  ``tag_word`` (device int32) holds ``tag`` once the kernel that was
    asked for this prefetch has run to its end; K1 falls back to the SH rows otherwise."""

    def __init__(self, N: int, device):
        self.colors = torch.empty(max(N, 1), 3, dtype=torch.float32, device=device)
        self.tag_word = torch.zeros(1, dtype=torch.int32, device=device)
        self.tag = 0
        self.cam = None
        self.N, self.sh_deg = N, -1
        self.front = None           # FrontBuffers of that view's frame, if its K1 is prefetched too
        self.front_budget = None    # the IntersectBudget that frame is binned with (capacity, sticky word)
        self.front_issued = False   # the fused optimizer call that fills `front` has been enqueued
        self.colors_valid = True    # False: only `front` is produced (data-parallel form), `colors` stays unwritten

    def arm(self, cam: Camera, sh_deg: int, front: Optional["FrontBuffers"] = None,
            budget: Optional["IntersectBudget"] = None, colors_valid: bool = True) -> "ColorPrefetch":
        self.tag += 1
        self.cam, self.sh_deg = cam, sh_deg
        self.front, self.front_budget, self.front_issued = front, budget, False
        self.colors_valid = colors_valid
        return self

    def matches(self, cam: Camera, N: int, sh_deg: int) -> bool:
        return self.cam is cam and self.N == N and self.sh_deg == sh_deg and self.tag > 0


_SIDE_CLEAR = _os.environ.get("TGS_FRONT_SIDE_CLEAR", "1") != "0"   # A/B switch: next frame's counters cleared by extra workgroups of this frame's scan launch


# Direct bins (tgs.h): the K1 inside the fused optimizer kernel stores every pair in a fixed-capacity bin of its
# (XCC, tile) and the fill pass leaves the step (cfg3: -12 us per step for 534 MB of bins per frame in flight).
# TGS_FRONT_BINS=0 / set_front_bins(False): off (A/B switch);
# TGS_FRONT_BINS_MAX_MB: the most one frame's bins may take (8 * tiles * max_list_hint * 8 bytes), beyond it the frame keeps the fill pass.
_FRONT_BINS = [_os.environ.get("TGS_FRONT_BINS", "1") != "0", int(_os.environ.get("TGS_FRONT_BINS_MAX_MB", "1024")) << 20]
BINS_MAX_CAP = 4096    # the register sorts' classes; longer lists (`huge`) keep the fill pass


def set_front_bins(on: Optional[bool] = None, max_bytes: Optional[int] = None):
    """-> (on, ceiling in bytes) of the direct bins after applying the arguments (None = leave as it is)."""
    if on is not None:
        _FRONT_BINS[0] = bool(on)
    if max_bytes is not None:
        _FRONT_BINS[1] = max(int(max_bytes), 0)
    return _FRONT_BINS[0], _FRONT_BINS[1]


class FrontBuffers:
    """Everything the front half of ONE frame writes (what project_bin_sort allocates per call).  Allocated one
    step ahead when the previous step's fused optimizer kernel also runs this frame's K1 (front prefetch,
    tgs_project_bwd_adam_next_front): records, group bases, per-tile counters and ranks are then filled by that
    kernel, and project_bin_sort only scans, fills and sorts (tgs_project_bin_sort_front) -- or, with ``bins``
    (``attach_bins``), K1 stores the pairs there and project_bin_sort only scans and sorts (the _bins pair of calls)."""
    bins, bin_cap = None, 0
    bins_filled = False      # the optimizer call that ran this frame's K1 took the bins (optim.backward_and_step)

    def __init__(self, cam: Camera, N: int, cap: int, want_radii: bool, dev, records: bool = True):
        lib = _lib.load()
        T = cam.num_tiles
        self.N, self.cam = N, cam
        # non-null even for N = 0; ``records=False``: the caller holds the records already (bin_sort)
        self.splats = torch.empty(max(N, 1), SPLAT_FLOATS, dtype=torch.float32, device=dev)[:N] if records else None
        self.radii = torch.empty(N, dtype=torch.int32, device=dev) if want_radii else None
        self.group_base = torch.empty(max(lib.tgs_num_groups(N), 1), dtype=torch.int32, device=dev)
        self.tile_start = torch.empty(T + 1 + 512, dtype=torch.int32, device=dev)[:T + 1]   # + 512 scratch ints of the rasterizer (tgs.h)
        nc = lib.tgs_tile_counter_len(cam.W, cam.H)
        counters = torch.empty(nc + 4, dtype=torch.int32, device=dev)   # per-XCD tile counters + sub-list starts | status[4]
        self.tile_cursor, self.status, self.status4 = counters[:nc], counters[nc:nc + 2], counters[nc:]
        # block -> tile schedule of K6 / K7 (tiles dealt to the XCDs in granules of 8, longest list first inside each XCD); it rides on the
        # tile_start tensor object so that the (tile_start, sorted_gid) pair keeps its meaning for callers
        self.tile_start.tile_order = torch.empty(lib.tgs_tile_order_len(cam.W, cam.H), dtype=torch.int32, device=dev)
        self.tile_start.slot_ok = None     # quadrant bitmaps K6 leaves for K7 (rasterize_fwd allocates and fills them)
        self.size_lists(cap, dev)
        self.cleared = False     # counters + status word already cleared (by the previous frame's scan launch)

    def size_lists(self, cap: int, dev) -> None:
        """(Re-)allocate what scales with the intersection capacity: the sorted lists and the sort's scratch."""
        self.cap = cap
        self.sorted_gid = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        self.scratch = torch.empty(_lib.load().tgs_sort_scratch_bytes(cap), dtype=torch.uint8, device=dev)

    def attach_bins(self, list_hint: int) -> bool:
        """Direct bins for this frame, ``list_hint`` entries per (XCC, tile), if they are switched on, the hint is a
        bound the register sorts cover and the bins fit the ceiling -> True.  Otherwise the frame keeps the fill pass."""
        on, ceiling = _FRONT_BINS
        T = self.cam.num_tiles
        if not on or self.N <= 0 or not (0 < list_hint <= BINS_MAX_CAP):
            return False
        n = _lib.load().tgs_bins_len(T, int(list_hint))
        if n * 8 > ceiling:
            return False
        self.bins = torch.empty(n, 2, dtype=torch.int32, device=self.group_base.device)   # {gid, depth bits}; never cleared
        self.bin_cap = int(list_hint)
        return True

    def settle(self, budget: IntersectBudget) -> bool:
        """After the front half was launched into these buffers: the frame's status words go to ``budget``; a synchronous
        budget reads them back, and a frame that overflowed grows the capacity and the lists -> True = launch it again."""
        budget.last_status, budget.last_status4 = self.status, self.status4
        if not budget.sync:
            return False
        n, ovf, need, budget.last_longest = self.status4.tolist()
        budget.last_n, budget.last_need = n, max(n, need)
        if ovf:
            budget.capacity = int(n * budget.growth) + 1024
            self.size_lists(budget.capacity, self.sorted_gid.device)
        return bool(ovf)


def project_bin_sort(cam: Camera, means, log_scales, quats, opac_logit, sh, sh_deg: int,
                     budget: Optional[IntersectBudget] = None, want_radii: bool = False,
                     colors: Optional[ColorPrefetch] = None, next_front: Optional["FrontBuffers"] = None):
    """K1 fused with the tile counting, then scan / fill / sort: the front half of a frame in ONE C
    call -> (splats, radii or None, group_base, tile_start, sorted_gid, status).  (tgs_project_bin_sort;
    with ``colors`` -- a ColorPrefetch armed for THIS camera -- tgs_project_bin_sort_colors, or, if the previous
    step's optimizer kernel also ran this frame's K1 into ``colors.front``, tgs_project_bin_sort_front: scan, fill
    and sort only.  ``next_front``: the FrontBuffers of the frame AFTER this one, if this step's optimizer kernel is
    going to fill them -- the front path clears their counters on the side)"""
    lib = _lib.load()
    budget = budget or _default_budget
    N = means.shape[0]
    dev = means.device
    cs = cam.c_struct()
    sh_stride = sh.shape[1] if sh is not None else 0
    cap = budget.initial(N)
    # front prefetch: this frame's K1 already ran inside the previous step's optimizer kernel, into buffers
    # allocated then (same sizes as here) -- usable if nothing changed in between
    fb = colors.front if (colors is not None and sh is not None and N > 0 and colors.front_issued) else None
    if fb is not None:
        colors.front, colors.front_issued = None, False      # single use: the finish below consumes the counters
        if (fb.N != N or fb.cap != cap or fb.cam is not cam or colors.front_budget is not budget
                or (want_radii and fb.radii is None)):
            fb = None
    from_front = fb is not None
    tag_holder = colors
    if colors is not None and not colors.colors_valid:
        colors = None                    # nothing but the front was prefetched: any other path evaluates the SH rows
    if fb is None:
        fb = FrontBuffers(cam, N, cap, want_radii, dev)
    splats, radii, group_base, tile_start = fb.splats, fb.radii, fb.group_base, fb.tile_start
    tile_cursor, status, tile_order = fb.tile_cursor, fb.status, fb.tile_start.tile_order
    while True:
        cap, sorted_gid, scratch = fb.cap, fb.sorted_gid, fb.scratch
        if from_front:
            nf = next_front if (_SIDE_CLEAR and next_front is not None and not next_front.cleared and next_front is not fb and
                                lib.tgs_front_can_clear_next(N, next_front.cam.W, next_front.cam.H)) else None
            ncs = nf.cam.c_struct() if nf is not None else None
            front_args = (C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats), ptr(opac_logit),
                          ptr(sh), sh_stride, sh_deg, ptr(splats), ptr(radii), ptr(group_base),
                          ptr(tile_start), _tile_start_len(tile_start), ptr(tile_cursor), ptr(sorted_gid),
                          ptr(tile_order), cap, ptr(scratch), ptr(status), ptr(budget.sticky_word(dev)),
                          budget.list_hint(), ptr(tag_holder.tag_word), tag_holder.tag,
                          C.byref(ncs) if nf is not None else None,
                          ptr(nf.tile_cursor) if nf is not None else None,
                          ptr(nf.status) if nf is not None else None)
            if fb.bins_filled:           # the K1 that filled these buffers stored its pairs in the bins: no ranks to fill from
                check(lib.tgs_project_bin_sort_front_bins(*front_args, ptr(fb.bins), fb.bins.shape[0], fb.bin_cap, _stream()),
                      "tgs_project_bin_sort_front_bins")
            else:
                check(lib.tgs_project_bin_sort_front(*front_args, _stream()), "tgs_project_bin_sort_front")
            if nf is not None:
                nf.cleared = True
            from_front = False          # a regrown capacity (synchronous budget) goes through the regular K1
        elif colors is None or sh is None:
            check(lib.tgs_project_bin_sort(C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats), ptr(opac_logit),
                                           ptr(sh), sh_stride, sh_deg if sh is not None else -1, ptr(splats),
                                           ptr(radii), ptr(group_base), ptr(tile_start), _tile_start_len(tile_start),
                                           ptr(tile_cursor), ptr(sorted_gid), ptr(tile_order), cap, ptr(scratch), ptr(status),
                                           ptr(budget.sticky_word(dev)), budget.list_hint(), _stream()),
                  "tgs_project_bin_sort")
        else:
            check(lib.tgs_project_bin_sort_colors(C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats),
                                                  ptr(opac_logit), ptr(sh), sh_stride, sh_deg, ptr(splats),
                                                  ptr(radii), ptr(group_base), ptr(tile_start), _tile_start_len(tile_start),
                                                  ptr(tile_cursor), ptr(sorted_gid), ptr(tile_order), cap, ptr(scratch), ptr(status),
                                                  ptr(budget.sticky_word(dev)), budget.list_hint(), ptr(colors.colors),
                                                  ptr(colors.tag_word), colors.tag, _stream()),
                  "tgs_project_bin_sort_colors")
        if not fb.settle(budget):
            return splats, radii, group_base, tile_start, sorted_gid, status


def _tile_start_len(tile_start) -> int:
    """int32 entries of the allocation from the tensor's first element on: the ``tile_start_len`` the C ABI validates
    against ``tgs_tile_start_len`` (TGS_VERSION 300)."""
    return tile_start.untyped_storage().nbytes() // 4 - tile_start.storage_offset()


def raster_opts(k6_blocks=None, k6_split=None, k7_front_to_back=None, k7_quad=None, k7_quad_min_walk=None, k7_blocks=None,
                k6_split_floor=None, k6_split_heads=None):
    """Per-call TgsRasterOpts (tgs.h): the forms of the compositing kernels for ONE rasterize_fwd / rasterize_bwd call,
    independent of the process-wide ``set_raster_variant`` / ``set_k6_split`` / ``set_k6_split_shape`` / ``set_k7_quad``
    defaults.  None = default."""
    f = lambda v: -1 if v is None else int(v)
    return _lib.TgsRasterOpts(f(k6_blocks), f(k6_split), f(k7_front_to_back), f(k7_quad), f(k7_quad_min_walk), f(k7_blocks),
                              f(k6_split_floor), f(k6_split_heads))


def _check_tile_start(tile_start, T: int) -> int:
    """The rasterizer keeps 512 scratch ints behind the T + 1 tile starts (tgs.h, tgs_tile_start_len): a tensor that was
    copied out of the buffer ``bin_sort`` / ``FrontBuffers`` allocated (clone, contiguous, .to) has lost them.  (The C
    ABI checks the same length; this gives the Python caller the reason.)  -> that length, for the C call."""
    have = _tile_start_len(tile_start)
    if have < T + 1 + 512:
        raise ValueError(f"tile_start must be (a view of) a buffer of T + 513 = {T + 513} int32 (got room for {have}): "
                         "pass the tensor ops.bin_sort / ops.project_bin_sort returned, not a copy")
    return have


def rasterize_fwd(cam: Camera, splats, sorted_gid, tile_start, want_idx: bool = False, want_stop: bool = True, opts=None):
    """K6 -> (rgb [H,W,3], depth_acc [H,W], final_T [H,W], final_idx [H,W] or None).  (tgs_rasterize_fwd)

    ``want_stop=False`` (render only: evaluation, ``get_outputs``) skips the per-pixel stop positions the backward needs
    (4 B per pixel not allocated, not written); ``opts`` = ``raster_opts(...)`` for this call only."""
    lib = _lib.load()
    dev = splats.device
    H, W = cam.H, cam.W
    ts_len = _check_tile_start(tile_start, cam.num_tiles)
    rgb = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    fT = torch.empty(H, W, dtype=torch.float32, device=dev)
    fidx = torch.empty(H, W, dtype=torch.int32, device=dev) if want_idx else None
    # per pixel: list position of the Gaussian that stopped it -- where the backward (back to front) starts.
    # It travels with final_T (fT.stop_pos), like tile_order / slot_ok travel with tile_start.
    stop = torch.empty(H, W, dtype=torch.int32, device=dev) if want_stop else None
    fT.stop_pos = stop
    cs = cam.c_struct()
    slot_ok = None
    if SLOT_OK and hasattr(tile_start, "slot_ok"):
        # per batch of 64 list positions: which Gaussians changed the state of each 8x8 quadrant; the
        # backward over the same lists (rasterize_bwd*) skips the rest.  Results are unaffected.
        slot_ok = torch.empty(4 * lib.tgs_slot_ok_len(W, H, sorted_gid.shape[0]), dtype=torch.int64, device=dev)
        tile_start.slot_ok = slot_ok
    check(lib.tgs_rasterize_fwd(C.byref(cs), ptr(splats), ptr(sorted_gid), ptr(tile_start), ts_len,
                                ptr(getattr(tile_start, "tile_order", None)), ptr(rgb),
                                ptr(depth), ptr(fT), ptr(fidx), ptr(stop), ptr(slot_ok),
                                C.byref(opts) if opts is not None else None, _stream()), "tgs_rasterize_fwd")
    return rgb, depth, fT, fidx


def rasterize_depth_stats(cam: Camera, splats, sorted_gid, tile_start, depth_acc, final_T, want_gid: bool = False, opts=None):
    """K6s -> (depth_var [H,W], median_depth [H,W], median_gid int32 [H,W] or None).  (tgs_rasterize_depth_stats)

    A second, forward-only walk over the lists ``rasterize_fwd`` composited; ``depth_acc`` / ``final_T`` are that call's
    outputs.  ``depth_var`` = sum w (d - D)^2 / alpha around the expected depth D = depth_acc / alpha; ``median_depth`` =
    depth of the Gaussian behind which the transmittance first is <= 1/2 (0 where alpha < 1/2, ``median_gid`` -1).  Uses
    ``final_T.stop_pos`` when the forward left it (it only shortens the walk).  No gradients flow through the outputs."""
    lib = _lib.load()
    dev = splats.device
    H, W = cam.H, cam.W
    ts_len = _check_tile_start(tile_start, cam.num_tiles)
    depth_acc, fT = _f32c(depth_acc.detach()), _f32c(final_T.detach())
    if tuple(depth_acc.shape) != (H, W) or tuple(fT.shape) != (H, W):
        raise ValueError(f"depth_acc / final_T must be [{H},{W}]")
    stop = getattr(final_T, "stop_pos", None)
    var = torch.empty(H, W, dtype=torch.float32, device=dev)
    med = torch.empty(H, W, dtype=torch.float32, device=dev)
    gid = torch.empty(H, W, dtype=torch.int32, device=dev) if want_gid else None
    cs = cam.c_struct()
    check(lib.tgs_rasterize_depth_stats(C.byref(cs), ptr(splats), ptr(sorted_gid), ptr(tile_start), ts_len,
                                        ptr(getattr(tile_start, "tile_order", None)), ptr(depth_acc), ptr(fT), ptr(stop),
                                        ptr(var), ptr(med), ptr(gid), C.byref(opts) if opts is not None else None,
                                        _stream()), "tgs_rasterize_depth_stats")
    return var, med, gid


def rasterize_bwd(cam: Camera, splats, group_base, sorted_gid, tile_start, rgb, depth, fT,
                  v_rgb=None, v_depth=None, v_alpha=None, loss: Optional[dict] = None,
                  want_tile_loss: bool = False, stop_pos=None, partials=None, opts=None):
    """K7 -> (partials [cap,12], tile_loss [T,2] or None).  (tgs_rasterize_bwd)

    ``loss`` = dict(gt_rgb, gt_depth, uncertainty, l1_weight, depth_weight, uncertainty_weight, eps).
    ``stop_pos``: the forward's per-pixel stop positions; default = ``fT.stop_pos`` as ``rasterize_fwd`` left it.
    """
    lib = _lib.load()
    dev = splats.device
    ts_len = _check_tile_start(tile_start, cam.num_tiles)
    if partials is None:     # (a caller may hand in the buffer, e.g. pre-filled to detect reads of unwritten records)
        partials = torch.empty(sorted_gid.shape[0], PARTIAL_FLOATS, dtype=torch.float32, device=dev)
    tile_loss = torch.empty(cam.num_tiles, 2, dtype=torch.float32, device=dev) if want_tile_loss else None
    cs = cam.c_struct()
    ls = None
    keep = []
    if loss is not None:
        ls = _loss_spec_struct(loss, keep)
    v_rgb, v_depth, v_alpha = _f32c(v_rgb), _f32c(v_depth), _f32c(v_alpha)
    check(lib.tgs_rasterize_bwd(C.byref(cs), ptr(splats), ptr(group_base), ptr(sorted_gid),
                                ptr(tile_start), ts_len, ptr(getattr(tile_start, "tile_order", None)),
                                ptr(rgb), ptr(depth), ptr(fT), ptr(_stop_pos_of(fT, stop_pos)),
                                ptr(v_rgb), ptr(v_depth), ptr(v_alpha),
                                C.byref(ls) if ls is not None else None, ptr(partials),
                                ptr(tile_loss), ptr(getattr(tile_start, "slot_ok", None)),
                                C.byref(opts) if opts is not None else None, _stream()), "tgs_rasterize_bwd")
    return partials, tile_loss


def set_raster_variant(k6_blocks: Optional[bool] = None, k7_front_to_back: Optional[bool] = None) -> int:
    """Developer switch (tgs_set_raster_variant): K6 in 4x4-block (default) / quadrant form, K7 back to front
    (default) / front to back (the round 1-3 form; the only one that takes the slot_ok bitmaps).  None leaves a
    setting alone.  Returns the settings in force (bit 0 = block-form K6, bit 1 = front-to-back K7)."""
    f = lambda v: -1 if v is None else int(bool(v))
    return _lib.load().tgs_set_raster_variant(f(k6_blocks), f(k7_front_to_back))


def set_k6_split_shape(floor: Optional[int] = None, heads: Optional[int] = None):
    """The shape of K6's split rule (tgs_set_k6_split_shape): the shortest list it splits and how many leading entries of
    the schedule get extra blocks.  None leaves a setting.  Returns (floor, heads)."""
    r = _lib.load().tgs_set_k6_split_shape(-1 if floor is None else int(floor), -1 if heads is None else int(heads))
    return r & 0xffff, r >> 16


def set_long_run(tiles: Optional[int] = None) -> int:
    """Binning: Gaussians covering more than ``tiles`` tiles are long runs (tgs_set_long_run; default 32, None = query):
    counted outside the group's aggregated box, their partial records summed by the whole workgroup in K8.  The
    process-wide default of ``Camera.long_run`` = 0; a camera that carries its own value does not look at it."""
    return _lib.load().tgs_set_long_run(-1 if tiles is None else int(tiles))


def set_k6_split(factor: Optional[int] = None) -> int:
    """The forward splits tiles whose list exceeds max(256, factor x the balanced per-slot load) into four quadrant blocks
    of the same launch (tgs_set_k6_split; default 2, 0 = never, None = query).  Bit-identical outputs."""
    return _lib.load().tgs_set_k6_split(-1 if factor is None else int(factor))


def set_k7_quad(factor: Optional[int] = None, min_walk: Optional[int] = None):
    """K7's four-waves-per-tile form for the tiles of chain-bound frames (deepest walk > factor / 2 x the balanced
    per-slot load; tgs_set_k7_quad; defaults factor 8, min_walk 16; factor 0 = one wave per tile always; None leaves
    a setting).  Returns (factor, min_walk) in effect."""
    r = _lib.load().tgs_set_k7_quad(-1 if factor is None else int(factor), -1 if min_walk is None else int(min_walk))
    return r & 255, r >> 8


def set_k7_scan(min_walk: Optional[int] = None, heads: Optional[int] = None):
    """K7's scan form for the longest tiles of chain-bound frames (tgs_set_k7_scan): tiles walking more than ``min_walk``
    entries among the schedule's first ``heads`` slots; 0 = off; None leaves a setting.  Returns (min_walk, heads)."""
    r = _lib.load().tgs_set_k7_scan(-1 if min_walk is None else int(min_walk), -1 if heads is None else int(heads))
    return r & 0xffff, r >> 16


def _stop_pos_of(fT, stop_pos=None):
    """The stop positions that belong to a forward's final_T (K7 needs them; there is no fallback)."""
    sp = stop_pos if stop_pos is not None else getattr(fT, "stop_pos", None)
    if sp is None:
        raise RuntimeError("rasterize_bwd needs the forward's stop positions: pass the final_T tensor that "
                           "rasterize_fwd returned (it carries .stop_pos) or stop_pos=...")
    return sp


def _loss_spec_struct(loss, keep):
    ls = _lib.TgsLossSpec()
    for k in ("gt_rgb", "gt_depth", "uncertainty"):
        t = _f32c(loss.get(k))
        keep.append(t)
        setattr(ls, k, ptr(t))
    ls.l1_weight = float(loss.get("l1_weight", 0.0))
    ls.depth_weight = float(loss.get("depth_weight", 0.0))
    ls.uncertainty_weight = float(loss.get("uncertainty_weight", 1.0))
    ls.eps = float(loss.get("eps", 1e-6))
    return ls


def band_rows(cam: Camera):
    """Image bands of the K7 band launches -> list of (band, y0, y1, count_y0, count_y1): the pixel rows
    [y0, y1) a band's tiles cover and the rows [count_y0, count_y1) it contributes to image-wide sums (a
    partition of [0, H)).  (tgs_num_bands / tgs_band_tiles)"""
    lib = _lib.load()
    TW = cam.tiles[0]
    out = []
    t0, t1 = C.c_int(), C.c_int()
    for b in range(lib.tgs_num_bands(cam.W, cam.H)):
        check(lib.tgs_band_tiles(cam.W, cam.H, b, C.byref(t0), C.byref(t1)), "tgs_band_tiles")
        if t1.value > t0.value:
            out.append([b, 16 * (t0.value // TW), min(16 * ((t1.value - 1) // TW + 1), cam.H)])
    for i, r in enumerate(out):
        r += [r[1] if i else 0, out[i + 1][1] if i + 1 < len(out) else cam.H]
    return [tuple(r) for r in out]


def rasterize_bwd_ssim_pipelined(cam: Camera, splats, group_base, sorted_gid, tile_start, rgb, depth, fT, gt_rgb,
                                 ssim_weight: float, loss: Optional[dict], side_stream, want_tile_loss: bool = True):
    """SSIM (K10) and K7 pipelined by image bands on two streams: the SSIM gradient of band b is produced
    on ``side_stream`` while K7 composites band b-1 on the current stream (K7 is VALU-bound, the SSIM
    kernels are latency chains: they overlap almost for free), so only the first band's SSIM is exposed.
    Bit-identical to ssim_fwd_bwd followed by rasterize_bwd.  -> (partials, tile_loss, ssim partial sums).
    (tgs_ssim_fwd_bwd_rows, tgs_rasterize_bwd_band)"""
    lib = _lib.load()
    dev = splats.device
    H, W = cam.H, cam.W
    order = getattr(tile_start, "tile_order", None)
    if order is None:
        raise ValueError("the band launches need tile_start.tile_order (ops.bin_sort / project_bin_sort)")
    bands = band_rows(cam)
    rgb, gt_rgb = _f32c(rgb), _f32c(gt_rgb)
    partials = torch.empty(sorted_gid.shape[0], PARTIAL_FLOATS, dtype=torch.float32, device=dev)
    tile_loss = torch.empty(cam.num_tiles, 2, dtype=torch.float32, device=dev) if want_tile_loss else None
    v_img = torch.empty_like(rgb)
    scratch = torch.empty(9 * H * W, dtype=torch.float32, device=dev)
    n_p = ((W + 63) // 64) * ((max(y1 - y0 for _, y0, y1, _, _ in bands) + 10) // 12 + 2)
    bp = torch.empty(len(bands), n_p, dtype=torch.float32, device=dev)
    keep = []
    ls = _loss_spec_struct(loss, keep) if loss is not None else None
    cs = cam.c_struct()
    main = torch.cuda.current_stream(dev)
    ready = torch.cuda.Event()
    ready.record(main)                     # the rendered image is complete on the current stream
    side_stream.wait_event(ready)
    for t in (v_img, scratch, bp, rgb, gt_rgb):
        t.record_stream(side_stream)
    done = []
    with torch.cuda.stream(side_stream):
        for i, (b, y0, y1, c0, c1) in enumerate(bands):
            check(lib.tgs_ssim_fwd_bwd_rows(W, H, ptr(rgb), ptr(gt_rgb), C.c_float(ssim_weight), ptr(bp[i]), n_p,
                                            ptr(v_img), ptr(scratch), y0, y1, c0, c1, _stream()),
                  "tgs_ssim_fwd_bwd_rows")
            ev = torch.cuda.Event()
            ev.record(side_stream)
            done.append(ev)
    for (b, *_), ev in zip(bands, done):
        main.wait_event(ev)
        check(lib.tgs_rasterize_bwd_band(C.byref(cs), ptr(splats), ptr(group_base), ptr(sorted_gid), ptr(tile_start),
                                         _tile_start_len(tile_start), ptr(order), ptr(rgb), ptr(depth), ptr(fT),
                                         ptr(_stop_pos_of(fT)), ptr(v_img), None, None,
                                         C.byref(ls) if ls is not None else None, ptr(partials), ptr(tile_loss),
                                         b, ptr(getattr(tile_start, "slot_ok", None)), None, _stream()), "tgs_rasterize_bwd_band")
    return partials, tile_loss, bp


def reduce_partials(cam: Camera, splats, group_base, partials):
    """K8a -> v_splats [N,12].  (tgs_reduce_partials)"""
    lib = _lib.load()
    N = splats.shape[0]
    v_splats = torch.empty(N, SPLAT_FLOATS, dtype=torch.float32, device=splats.device)
    cs = cam.c_struct()
    check(lib.tgs_reduce_partials(N, ptr(splats), ptr(group_base), C.byref(cs), ptr(partials),
                                  ptr(v_splats), _stream()), "tgs_reduce_partials")
    return v_splats


def project_bwd(cam: Camera, means, log_scales, quats, opac_logit, sh, sh_deg, splats,
                group_base=None, partials=None, v_splats=None, out=None, want_v_xy=False, guard=None):
    """K8 -> (v_means, v_log_scales, v_quats, v_opac_logit, v_sh, v_xy).  (tgs_project_bwd)

    ``out`` may supply pre-allocated gradient tensors (e.g. views into a flat gradient buffer).
    """
    lib = _lib.load()
    N = means.shape[0]
    dev = means.device
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
    if out is None:
        out = (e(N, 3), e(N, 3), e(N, 4), e(N), torch.empty_like(sh) if sh is not None else None)
    v_means, v_ls, v_q, v_ol, v_sh = out
    v_xy = e(N, 2) if want_v_xy else None
    cs = cam.c_struct()
    sh_stride = sh.shape[1] if sh is not None else 0
    check(lib.tgs_project_bwd(C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats), ptr(opac_logit),
                              ptr(sh), sh_stride, sh_deg if sh is not None else -1, ptr(splats),
                              ptr(group_base), ptr(partials), ptr(v_splats), ptr(v_means), ptr(v_ls),
                              ptr(v_q), ptr(v_ol), ptr(v_sh), ptr(v_xy), ptr(guard), _stream()), "tgs_project_bwd")
    return v_means, v_ls, v_q, v_ol, v_sh, v_xy


def pose_grad(cam: Camera, means, log_scales, quats, sh, sh_deg, splats, group_base=None, partials=None,
              v_splats=None, guard=None, out=None):
    """Gradient of the loss w.r.t. rows 0-2 of ``cam.viewmat`` -> device tensor [32] = G[3,4] row-major | the 12
    masses (sum of |products| per entry) | valid flag | number of visible Gaussians | zeros.  (tgs_pose_grad)

    Reads what :func:`project_bwd` reads (``partials`` + ``group_base``, or ``v_splats``) and writes nothing else, so
    it must run BEFORE an optimizer step that changes the parameters of the frame.  ``sh=None``: no colour path (the
    colours did not come from SH rows).  ``guard`` = the frame's status word: an overflowed frame gives all zeros.
    No host synchronisation, no allocation when ``out`` = (result [32], scratch [groups, 25]) is passed: safe under
    stream capture."""
    lib = _lib.load()
    N = means.shape[0]
    dev = means.device
    if out is None:
        out = (torch.empty(_lib.POSE_OUT, dtype=torch.float32, device=dev),
               torch.empty(max(lib.tgs_num_groups(N), 1), _lib.POSE_ROW, dtype=torch.float32, device=dev))
    res, scratch = out
    if res.numel() != _lib.POSE_OUT or scratch.numel() < lib.tgs_num_groups(N) * _lib.POSE_ROW:
        raise ValueError("pose_grad: out = (float32 [32], float32 [tgs_num_groups(N), 25])")
    if partials is None and v_splats is None:
        raise ValueError("pose_grad needs partials (+ group_base) or v_splats")
    cs = cam.c_struct()
    sh_stride = sh.shape[1] if sh is not None else 0
    check(lib.tgs_pose_grad(C.byref(cs), N, ptr(means), ptr(log_scales), ptr(quats), ptr(sh), sh_stride,
                            sh_deg if sh is not None else -1, ptr(splats), ptr(group_base), ptr(partials),
                            ptr(v_splats), ptr(scratch), ptr(res), ptr(guard), _stream()), "tgs_pose_grad")
    return res


def project_bwd_color(cam: Camera, means, log_scales, quats, opac_logit, sh, sh_deg, splats, group_base,
                      partials, out, v_color, want_v_xy=False, guard=None, rows=None, v_xy=None):
    """K8 of the data-parallel step (tgs_project_bwd_color): geometry gradients into ``out`` =
    (v_means, v_log_scales, v_quats, v_opac_logit) and, instead of the SH gradient, the block
    ``v_color`` [3N+4] = clamp-gated colour gradients | camera position | pad.  -> v_xy or None.
    ``rows`` = (begin, end): only these model rows (begin a multiple of 256); ``v_color`` is then the
    chunk's own block [3 (end - begin) + 4] and ``v_xy`` [N,2] (if wanted) must be passed in."""
    lib = _lib.load()
    N = means.shape[0]
    b, e = (0, N) if rows is None else rows
    if v_color.numel() != 3 * (e - b) + 4 or v_color.dtype != torch.float32:
        raise ValueError("v_color must be a float32 tensor of 3*rows+4 elements")
    v_means, v_ls, v_q, v_ol = out
    if v_xy is None and want_v_xy:
        if rows is not None:
            raise ValueError("a row-range call writes into the caller's v_xy [N,2]")
        v_xy = torch.empty(N, 2, dtype=torch.float32, device=means.device)
    cs = cam.c_struct()
    check(lib.tgs_project_bwd_color_rows(C.byref(cs), N, b, e, ptr(means), ptr(log_scales), ptr(quats), ptr(opac_logit),
                                         ptr(sh), sh.shape[1], sh_deg, ptr(splats), ptr(group_base), ptr(partials),
                                         ptr(v_means), ptr(v_ls), ptr(v_q), ptr(v_ol), ptr(v_color), ptr(v_xy),
                                         ptr(guard), _stream()), "tgs_project_bwd_color_rows")
    return v_xy


def dp_agree_overflow(world: int, N: int, v_color_all, status_out, sticky=None):
    """After the all-gather of the colour blocks: status_out = {0, any rank's frame overflowed}
    (identical on every rank); raises ``sticky`` too.  (tgs_dp_agree_overflow)"""
    check(_lib.load().tgs_dp_agree_overflow(world, N, ptr(v_color_all), ptr(status_out), ptr(sticky), _stream()),
          "tgs_dp_agree_overflow")
    return status_out


# ------------------------------------------------------------------------------------------------
# fused differentiable render
# ------------------------------------------------------------------------------------------------
class _Render(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means, log_scales, quats, opac_logit, sh, means2d, cam, sh_deg, budget, need_bwd=True, opts=None,
                depth_stats=False):
        means, log_scales, quats, opac_logit, sh = map(_f32c, (means, log_scales, quats, opac_logit, sh))
        splats, radii, group_base, tile_start, sorted_gid, _ = project_bin_sort(
            cam, means, log_scales, quats, opac_logit, sh, sh_deg, budget, want_radii=True)
        # need_bwd = False: render only (evaluation, get_outputs under no_grad; decided by render(): grad mode is always
        # off in here and needs_input_grad ignores it) -- no backward will ask for the stop positions
        rgb, depth, fT, fidx = rasterize_fwd(cam, splats, sorted_gid, tile_start, want_stop=need_bwd, opts=opts)
        ctx.cam, ctx.sh_deg = cam, sh_deg
        ctx.want_xy = means2d is not None
        if need_bwd:
            ctx.save_for_backward(means, log_scales, quats, opac_logit, sh, splats, group_base,
                                  tile_start, sorted_gid, rgb, depth, fT, fT.stop_pos)
        alpha = 1.0 - fT
        if depth_stats:     # the second walk needs this frame's lists, which do not leave this function
            var, med, gid = rasterize_depth_stats(cam, splats, sorted_gid, tile_start, depth, fT, want_gid=True, opts=opts)
            ctx.mark_non_differentiable(radii, var, med, gid)
            return rgb, depth, alpha, radii, var, med, gid
        ctx.mark_non_differentiable(radii)
        return rgb, depth, alpha, radii

    @staticmethod
    def backward(ctx, v_rgb, v_depth, v_alpha, _v_radii, *_v_stats):
        (means, log_scales, quats, opac_logit, sh, splats, group_base, tile_start, sorted_gid,
         rgb, depth, fT, stop) = ctx.saved_tensors
        cam = ctx.cam
        partials, _ = rasterize_bwd(cam, splats, group_base, sorted_gid, tile_start, rgb, depth, fT,
                                    v_rgb, v_depth, v_alpha, stop_pos=stop)
        v_means, v_ls, v_q, v_ol, v_sh, v_xy = project_bwd(
            cam, means, log_scales, quats, opac_logit, sh, ctx.sh_deg, splats, group_base, partials,
            want_v_xy=ctx.want_xy)
        return v_means, v_ls, v_q, v_ol, v_sh, v_xy, None, None, None, None, None, None


def render(means, log_scales, quats, opac_logit, sh, cam: Camera, sh_deg: int,
           means2d: Optional[torch.Tensor] = None, budget: Optional[IntersectBudget] = None, opts=None,
           depth_stats: bool = False):
    """Fused differentiable render of RGB + depth + alpha in one compositing pass.

    Parameters are the raw (pre-activation) Gaussian parameters of SURVEY App. B.0.
    ``means2d`` ([N,2], requires_grad) optionally receives the screen-space mean gradient
    (INRIA ``means2D.grad`` convention) for densification statistics.
    Returns (rgb [H,W,3] incl. background, depth_acc [H,W] = sum w*z, alpha [H,W], radii [N]).
    Expected depth is ``depth_acc / alpha`` (consumer side, as Splatfacto does).
    ``opts`` = ``raster_opts(...)`` for the forward of this call only.
    ``depth_stats=True`` appends (depth_var [H,W], median_depth [H,W], median_gid int32 [H,W]) of
    :func:`rasterize_depth_stats` to the tuple: a second walk over the same lists.  The three are detached -- there is
    no autograd through the variance or the median; the first four entries are what the default call returns.
    """
    need_bwd = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                               for t in (means, log_scales, quats, opac_logit, sh, means2d))
    if not depth_stats:
        return _Render.apply(means, log_scales, quats, opac_logit, sh, means2d, cam, sh_deg, budget, need_bwd, opts)
    return _Render.apply(means, log_scales, quats, opac_logit, sh, means2d, cam, sh_deg, budget, need_bwd, opts, True)


# ------------------------------------------------------------------------------------------------
# gsplat-0.1 shaped operator surface
# ------------------------------------------------------------------------------------------------
def _sh_basis_torch(deg: int, d: torch.Tensor) -> torch.Tensor:
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [torch.full_like(x, 0.28209479177387814)]
    if deg >= 1:
        c1 = 0.4886025119029199
        out += [-c1 * y, c1 * z, -c1 * x]
    if deg >= 2:
        xx, yy, zz = x * x, y * y, z * z
        out += [1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
                0.31539156525252005 * (2 * zz - xx - yy), -1.0925484305920792 * x * z,
                0.5462742152960396 * (xx - yy)]
    if deg >= 3:
        out += [-0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * x * y * z,
                -0.4570457994644658 * y * (4 * zz - xx - yy),
                0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
                -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy),
                -0.5900435899266435 * x * (xx - 3 * yy)]
    return torch.stack(out, dim=-1)


class _SphericalHarmonics(torch.autograd.Function):
    @staticmethod
    def forward(ctx, degrees_to_use, viewdirs, coeffs):
        lib = _lib.load()
        dirs, coeffs = _f32c(viewdirs.detach()), _f32c(coeffs)
        N = coeffs.shape[0]
        out = torch.empty(N, 3, dtype=torch.float32, device=coeffs.device)
        check(lib.tgs_sh_fwd(N, degrees_to_use, coeffs.shape[1], ptr(dirs), ptr(coeffs), ptr(out), _stream()), "tgs_sh_fwd")
        ctx.deg, ctx.shape = degrees_to_use, coeffs.shape
        ctx.save_for_backward(dirs)
        return out

    @staticmethod
    def backward(ctx, v_colors):
        lib = _lib.load()
        (dirs,) = ctx.saved_tensors
        v = torch.empty(ctx.shape, dtype=torch.float32, device=dirs.device)
        check(lib.tgs_sh_bwd(ctx.shape[0], ctx.deg, ctx.shape[1], ptr(dirs), ptr(_f32c(v_colors)), ptr(v), _stream()),
              "tgs_sh_bwd")
        return None, None, v


def spherical_harmonics(degrees_to_use: int, viewdirs: torch.Tensor, coeffs: torch.Tensor):
    """gsplat-shaped SH evaluation: coeffs [N,K,3], viewdirs [N,3] (normalised in-kernel) -> [N,3]
    (no +0.5 / clamp: the caller applies them, as Splatfacto does).  Gradient flows to ``coeffs``
    only, as in gsplat 0.1.  (tgs_sh_fwd / tgs_sh_bwd; the fused training path evaluates SH inside
    K1/K8 instead.)"""
    return _SphericalHarmonics.apply(degrees_to_use, viewdirs, coeffs)


def record_xy(splats: torch.Tensor) -> torch.Tensor:
    """Absolute screen positions [N,2] from splat records: slots 0, 1 store the position relative to the
    origin (16 x0, 16 y0) of the Gaussian's packed tile rect in slot 10 (include/tgs.h; K1 evaluates
    it in compensated arithmetic, so the relative value is good to ~1e-5 px -- the sum returned here is
    rounded to fp32 like any absolute coordinate)."""
    r = splats[:, 10].contiguous().view(torch.int32)
    org = torch.stack([r & 255, (r >> 8) & 255], 1).to(torch.float32) * 16.0
    return (splats[:, 0:2] + org).contiguous()


class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3d, scales, glob_scale, quats, cam, viewmat=None):
        # viewmat: the caller's world->camera tensor when it asks for its gradient (the values are cam's), else None
        means3d, quats = _f32c(means3d), _f32c(quats)
        log_scales = torch.log(_f32c(scales))
        N = means3d.shape[0]
        zero = torch.zeros(N, dtype=torch.float32, device=means3d.device)
        cam = Camera(cam.viewmat, cam.fx, cam.fy, cam.cx, cam.cy, cam.W, cam.H, cam.near,
                     cam.pix_center, cam.bg, float(glob_scale))
        splats, radii = project_fwd(cam, means3d, log_scales, quats, zero, None, -1, want_radii=True)
        ctx.cam = cam
        ctx.save_for_backward(means3d, log_scales, quats, zero, splats)
        xys = record_xy(splats)
        depths = splats[:, 2].contiguous()
        conics = splats[:, 4:7].contiguous()
        ctx.mark_non_differentiable(radii)
        return xys, depths, radii, conics

    @staticmethod
    def backward(ctx, v_xys, v_depths, _v_radii, v_conics):
        means3d, log_scales, quats, zero, splats = ctx.saved_tensors
        N = means3d.shape[0]
        v_splats = torch.zeros(N, SPLAT_FLOATS, dtype=torch.float32, device=means3d.device)
        if v_xys is not None:
            v_splats[:, 0:2] = v_xys
        if v_depths is not None:
            v_splats[:, 2] = v_depths
        if v_conics is not None:
            v_splats[:, 4:7] = v_conics
        v_means, v_ls, v_q, _, _, _ = project_bwd(ctx.cam, means3d, log_scales, quats, zero, None, -1,
                                                  splats, v_splats=v_splats)
        v_scales = v_ls / torch.exp(log_scales)
        v_view = None
        if ctx.needs_input_grad[5]:   # camera pose: rows 0-2 from tgs_pose_grad (no colour path: viewdirs are torch's own)
            G = pose_grad(ctx.cam, means3d, log_scales, quats, None, -1, splats, v_splats=v_splats)
            v_view = torch.cat([G[:12].view(3, 4), G.new_zeros(1, 4)], 0)
        return v_means, v_scales, None, v_q, None, v_view


def project_gaussians(means3d, scales, glob_scale, quats, viewmat, fx, fy, cx, cy, img_height,
                      img_width, block_width: int = 16, clip_thresh: float = 0.01):
    """gsplat-0.1 ``project_gaussians``: -> (xys, depths, radii, conics, comp, num_tiles_hit, cov3d).

    ``scales`` are post-exp, ``quats`` un-normalised (w,x,y,z), ``viewmat`` world->camera.
    ``comp`` is all ones (no anti-aliasing compensation in App. B); ``cov3d`` is the upper triangle
    of R S S^T R^T computed with device torch ops (not differentiated, as in gsplat 0.1).
    """
    if block_width != 16:
        raise ValueError("only 16x16 tiles are supported (SURVEY App. B.0)")
    cam = Camera(viewmat, fx, fy, cx, cy, img_width, img_height, near=clip_thresh)
    want_pose = torch.is_tensor(viewmat) and viewmat.requires_grad
    xys, depths, radii, conics = _ProjectGaussians.apply(means3d, scales, glob_scale, quats, cam,
                                                         viewmat if want_pose else None)
    with torch.no_grad():
        tw, th = cam.tiles
        r = radii.to(torch.float32)
        x0 = torch.clamp(((xys[:, 0] - r) / 16).to(torch.int32), 0, tw)
        x1 = torch.clamp(((xys[:, 0] + r) / 16).to(torch.int32) + 1, 0, tw)
        y0 = torch.clamp(((xys[:, 1] - r) / 16).to(torch.int32), 0, th)
        y1 = torch.clamp(((xys[:, 1] + r) / 16).to(torch.int32) + 1, 0, th)
        num_tiles_hit = torch.where(radii > 0, (x1 - x0) * (y1 - y0), torch.zeros_like(x0))
        q = quats / quats.norm(dim=-1, keepdim=True)
        w, x, y, z = q.unbind(-1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)
        M = R * (scales * glob_scale)[:, None, :]
        S = M @ M.transpose(1, 2)
        cov3d = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)
        comp = torch.ones_like(depths)
    return xys, depths, radii, conics, comp, num_tiles_hit, cov3d


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xys, depths, radii, conics, colors, opacity, cam, budget):
        N = xys.shape[0]
        dev = xys.device
        op = opacity.reshape(N, 1).to(torch.float32)
        # slot 10 = packed App. B.4 tile rect x0 | y0<<8 | w<<16 | h<<24 (include/tgs.h)
        tw, th = cam.tiles
        r = radii.to(torch.float32)
        xf, yf = xys[:, 0].to(torch.float32), xys[:, 1].to(torch.float32)
        x0 = torch.clamp(((xf - r) * 0.0625).to(torch.int64), 0, tw)
        x1 = torch.clamp(((xf + r) * 0.0625).to(torch.int64) + 1, 0, tw)
        y0 = torch.clamp(((yf - r) * 0.0625).to(torch.int64), 0, th)
        y1 = torch.clamp(((yf + r) * 0.0625).to(torch.int64) + 1, 0, th)
        vis = (radii > 0) & (x1 > x0) & (y1 > y0)
        packed = torch.where(vis, x0 | (y0 << 8) | ((x1 - x0) << 16) | ((y1 - y0) << 24), torch.zeros_like(x0))
        packed = torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)
        # record slots 0, 1 hold the position relative to the origin of the tile rect (include/tgs.h)
        org = torch.stack([x0, y0], 1).to(torch.float32) * 16.0
        org = torch.where(vis[:, None], org, torch.zeros_like(org))
        splats = torch.cat([xys.to(torch.float32) - org, depths.reshape(N, 1).to(torch.float32), op,
                            conics.to(torch.float32), colors.to(torch.float32),
                            packed.reshape(N, 1).view(torch.float32),
                            torch.zeros(N, 1, dtype=torch.float32, device=dev)], dim=1).contiguous()
        group_base, tile_start, sorted_gid, _ = bin_sort(cam, splats, budget)
        rgb, depth, fT, fidx = rasterize_fwd(cam, splats, sorted_gid, tile_start)
        ctx.cam = cam
        ctx.opacity_shape = opacity.shape
        ctx.save_for_backward(splats, group_base, tile_start, sorted_gid, rgb, depth, fT, fT.stop_pos)
        return rgb, 1.0 - fT, depth

    @staticmethod
    def backward(ctx, v_rgb, v_alpha, v_depth):
        splats, group_base, tile_start, sorted_gid, rgb, depth, fT, stop = ctx.saved_tensors
        cam = ctx.cam
        partials, _ = rasterize_bwd(cam, splats, group_base, sorted_gid, tile_start, rgb, depth, fT,
                                    v_rgb, v_depth, v_alpha, stop_pos=stop)
        v = reduce_partials(cam, splats, group_base, partials)
        v_xys, v_depths = v[:, 0:2].contiguous(), v[:, 2].contiguous()
        v_op = v[:, 3].contiguous().reshape(ctx.opacity_shape)
        v_conics, v_colors = v[:, 4:7].contiguous(), v[:, 7:10].contiguous()
        return v_xys, v_depths, None, v_conics, v_colors, v_op, None, None


def rasterize_gaussians(xys, depths, radii, conics, num_tiles_hit, colors, opacity, img_height,
                        img_width, block_width: int = 16, background=None, return_alpha: bool = False,
                        return_depth: bool = False, budget: Optional[IntersectBudget] = None):
    """gsplat-0.1 ``rasterize_gaussians``: -> out_img [H,W,3] (, out_alpha [H,W]) (, depth_acc [H,W]).

    ``num_tiles_hit`` is accepted for signature compatibility and recomputed in-kernel from
    (xys, radii) by the App. B.4 rule.  ``return_depth`` is this build's extension: the depth
    channel composited in the same pass (Splatfacto instead calls the op a second time with
    ``depths.repeat(1,3)`` as colours, which also works here).
    """
    if block_width != 16:
        raise ValueError("only 16x16 tiles are supported (SURVEY App. B.0)")
    if colors.shape[-1] != 3:
        raise ValueError("colors must be [N,3]")
    bg = (0.0, 0.0, 0.0) if background is None else tuple(float(b) for b in background.detach().cpu().tolist())
    eye = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    cam = Camera(eye, 1.0, 1.0, 0.0, 0.0, img_width, img_height, bg=bg)
    rgb, alpha, depth = _RasterizeGaussians.apply(xys, depths, radii, conics, colors, opacity, cam, budget)
    out = (rgb,)
    if return_alpha:
        out += (alpha,)
    if return_depth:
        out += (depth,)
    return out[0] if len(out) == 1 else out


# ------------------------------------------------------------------------------------------------
# image-space loss kernel (K10)
# ------------------------------------------------------------------------------------------------
def ssim_fwd_bwd(img, gt, weight: float = 1.0, want_grad: bool = True, reduce: bool = True):
    """K10 -> (sum of the SSIM map [device scalar], v_img = weight * d(sum)/d(img) or None).
    ``reduce=False`` returns the per-block partial sums instead (the train step only needs the
    total when the loss value is logged, so it skips the extra reduction launch).

    Mean SSIM = sum / (3*H*W).  For the loss term l*(1-mean SSIM) pass weight = -l/(3*H*W).
    (tgs_ssim_fwd_bwd)
    """
    lib = _lib.load()
    img, gt = _f32c(img), _f32c(gt)
    H, W = img.shape[0], img.shape[1]
    dev = img.device
    nb = ((H + 15) // 16) * ((W + 15) // 16)
    bp = torch.empty(nb, dtype=torch.float32, device=dev)
    v_img = torch.empty_like(img) if want_grad else None
    scratch = torch.empty(9 * H * W, dtype=torch.float32, device=dev) if want_grad else None
    check(lib.tgs_ssim_fwd_bwd(W, H, ptr(img), ptr(gt), C.c_float(weight), ptr(bp), ptr(v_img),
                               ptr(scratch), _stream()), "tgs_ssim_fwd_bwd")
    return (bp.sum() if reduce else bp), v_img


# ------------------------------------------------------------------------------------------------
# image-space loss kernels: scale-invariant monocular depth (csrc/depthcorr.hip)
# ------------------------------------------------------------------------------------------------
def depth_corr_fwd_bwd(depth_acc, final_T, mono, alpha_min: float = 0.5, weight: float = 1.0, want_grad: bool = True):
    """-> (stats [8] = {n, mx, my, vx, vy, c, rho, weight * (1 - rho)}, v_depth [H,W] or None, v_alpha [H,W] or None).
    (tgs_depth_corr_fwd_bwd)

    rho = Pearson correlation of the expected depth ``depth_acc / max(1 - final_T, 1e-10)`` and the raw monocular map
    ``mono`` (any positive scale, any shift; 0 = no value) over the pixels with ``mono > 0`` and
    ``1 - final_T >= alpha_min``.  ``v_depth`` / ``v_alpha`` = gradient of ``weight * (1 - rho)`` with respect to
    ``depth_acc`` / ``1 - final_T``: the upstream images :func:`rasterize_bwd` takes.  A degenerate frame (fewer than two
    valid pixels, or no variance) has rho = 0, loss 0 and zero gradients.  ``want_grad=False``: forward only.  No host sync.
    """
    lib = _lib.load()
    depth_acc, final_T, mono = _f32c(depth_acc.detach()), _f32c(final_T.detach()), _f32c(mono)
    if depth_acc.dim() != 2 or depth_acc.shape != final_T.shape or depth_acc.shape != mono.shape:
        raise ValueError(f"depth_acc, final_T and mono must be [H,W] alike, got {tuple(depth_acc.shape)}, "
                         f"{tuple(final_T.shape)}, {tuple(mono.shape)}")
    H, W = depth_acc.shape
    dev = depth_acc.device
    tiles = torch.empty(((H + 15) // 16) * ((W + 15) // 16), 8, dtype=torch.float32, device=dev)
    stats = torch.empty(8, dtype=torch.float32, device=dev)
    v_depth = torch.empty(H, W, dtype=torch.float32, device=dev) if want_grad else None
    v_alpha = torch.empty(H, W, dtype=torch.float32, device=dev) if want_grad else None
    check(lib.tgs_depth_corr_fwd_bwd(W, H, ptr(depth_acc), ptr(final_T), ptr(mono), C.c_float(alpha_min), C.c_float(weight),
                                     ptr(tiles), ptr(stats), ptr(v_depth), ptr(v_alpha), _stream()), "tgs_depth_corr_fwd_bwd")
    return stats, v_depth, v_alpha


class _DepthCorrelation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_acc, alpha, mono, alpha_min):
        # 1 - (1 - T) restores the bits of 1 - T for every T in [0, 1]: the kernel sees the alpha the renderer returned
        stats, v_depth, v_alpha = depth_corr_fwd_bwd(depth_acc, 1.0 - alpha.detach(), mono, alpha_min, weight=-1.0)
        ctx.save_for_backward(v_depth, v_alpha)   # weight -1: the images are d rho / d depth_acc, d rho / d alpha
        return stats[6].clone()

    @staticmethod
    def backward(ctx, g):
        v_depth, v_alpha = ctx.saved_tensors
        return g * v_depth, g * v_alpha, None, None


def depth_correlation(depth_acc, alpha, mono, alpha_min: float = 0.5):
    """Pearson correlation rho (device scalar, differentiable in ``depth_acc`` and ``alpha``) between the expected depth
    ``depth_acc / max(alpha, 1e-10)`` and ``mono`` over the pixels with ``mono > 0`` and ``alpha >= alpha_min``
    (:func:`depth_corr_fwd_bwd`); ``depth_acc`` / ``alpha`` as :func:`render` returns them.  No host sync."""
    return _DepthCorrelation.apply(depth_acc, alpha, mono, alpha_min)


# ------------------------------------------------------------------------------------------------
# the same with a patch-wise (local) correlation term beside the global one
# ------------------------------------------------------------------------------------------------
def depth_corr_patch_min_count(patch_tiles: int, min_fill: float) -> int:
    """The count gate of a patch of ``patch_tiles`` x ``patch_tiles`` tiles: max(2, ceil(min_fill (16 patch_tiles)^2))."""
    return max(2, math.ceil(min_fill * (16 * patch_tiles) ** 2))


def depth_corr_local_fwd_bwd(depth_acc, final_T, mono, alpha_min: float = 0.5, weight_global: float = 1.0,
                             weight_local: float = 1.0, patch_tiles: int = 8, offset=(0, 0), min_fill: float = 0.25,
                             min_var_ratio: float = 1e-3, want_grad: bool = True, return_patches: bool = False):
    """-> (stats [16], v_depth [H,W] or None, v_alpha [H,W] or None[, patch_stats [PH, PW, 8]]).
    (tgs_depth_corr_local_fwd_bwd)

    ``weight_global * (1 - rho) + weight_local * (1 - rho_bar)``: rho as in :func:`depth_corr_fwd_bwd`, rho_bar the mean
    of the per-patch correlations over the ACTIVE patches of ``patch_tiles`` x ``patch_tiles`` tiles (16 ``patch_tiles``
    pixels on a side), the grid shifted by ``offset = (off_x, off_y)`` tiles.  A patch is active with at least
    ``min_fill`` of its full area valid and both its variances at least ``min_var_ratio`` of the image's.
    stats = {[0..7] as the global op with ``weight = weight_global``, [8] patches that pass the count gate, [9] active
    patches A, [10] rho_bar, [11] weight_local (1 - rho_bar), [12] total loss, [13..15] 0}; patch_stats per patch =
    {active, mx, my, beta, 1 / (n sqrt(vx vy)), rho, n, passes the count gate}.  No host sync.
    """
    lib = _lib.load()
    depth_acc, final_T, mono = _f32c(depth_acc.detach()), _f32c(final_T.detach()), _f32c(mono)
    if depth_acc.dim() != 2 or depth_acc.shape != final_T.shape or depth_acc.shape != mono.shape:
        raise ValueError(f"depth_acc, final_T and mono must be [H,W] alike, got {tuple(depth_acc.shape)}, "
                         f"{tuple(final_T.shape)}, {tuple(mono.shape)}")
    k, (off_x, off_y) = int(patch_tiles), (int(o) for o in offset)
    if not 1 <= k <= 16 or not (0 <= off_x < k and 0 <= off_y < k):
        raise ValueError(f"patch_tiles must be 1...16 and the offset in [0, patch_tiles), got {patch_tiles}, {tuple(offset)}")
    H, W = depth_acc.shape
    dev = depth_acc.device
    TW, TH = (W + 15) // 16, (H + 15) // 16
    PW, PH = (TW + off_x + k - 1) // k, (TH + off_y + k - 1) // k
    tiles = torch.empty(TW * TH, 8, dtype=torch.float32, device=dev)
    patches = torch.empty(PH, PW, 8, dtype=torch.float32, device=dev)
    stats = torch.empty(16, dtype=torch.float32, device=dev)
    v_depth = torch.empty(H, W, dtype=torch.float32, device=dev) if want_grad else None
    v_alpha = torch.empty(H, W, dtype=torch.float32, device=dev) if want_grad else None
    check(lib.tgs_depth_corr_local_fwd_bwd(W, H, ptr(depth_acc), ptr(final_T), ptr(mono), C.c_float(alpha_min),
                                           C.c_float(weight_global), C.c_float(weight_local), k, off_x, off_y,
                                           depth_corr_patch_min_count(k, min_fill), C.c_float(min_var_ratio), ptr(tiles),
                                           ptr(patches), ptr(stats), ptr(v_depth), ptr(v_alpha), _stream()),
          "tgs_depth_corr_local_fwd_bwd")
    return (stats, v_depth, v_alpha, patches) if return_patches else (stats, v_depth, v_alpha)


class _DepthCorrelationLocal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_acc, alpha, mono, alpha_min, patch_tiles, offset, min_fill, min_var_ratio):
        # two calls with unit weights (a slow path): the images of the first are d rho / d (depth_acc, alpha), those of the
        # second d rho_bar / d (depth_acc, alpha)
        fT = 1.0 - alpha.detach()
        kw = dict(patch_tiles=patch_tiles, offset=offset, min_fill=min_fill, min_var_ratio=min_var_ratio)
        stats, gd, ga = depth_corr_local_fwd_bwd(depth_acc, fT, mono, alpha_min, -1.0, 0.0, **kw)
        _, ld, la = depth_corr_local_fwd_bwd(depth_acc, fT, mono, alpha_min, 0.0, -1.0, **kw)
        ctx.save_for_backward(gd, ga, ld, la)
        return stats[6].clone(), stats[10].clone()

    @staticmethod
    def backward(ctx, g_rho, g_bar):
        gd, ga, ld, la = ctx.saved_tensors
        return g_rho * gd + g_bar * ld, g_rho * ga + g_bar * la, None, None, None, None, None, None


def depth_correlation_local(depth_acc, alpha, mono, alpha_min: float = 0.5, patch_tiles: int = 8, offset=(0, 0),
                            min_fill: float = 0.25, min_var_ratio: float = 1e-3):
    """(rho, rho_bar): the global Pearson correlation of :func:`depth_correlation` and the mean correlation over the
    active patches (:func:`depth_corr_local_fwd_bwd`), device scalars differentiable in ``depth_acc`` and ``alpha`` with the
    gates held constant.  No host sync."""
    return _DepthCorrelationLocal.apply(depth_acc, alpha, mono, alpha_min, patch_tiles, tuple(offset), min_fill, min_var_ratio)


# ------------------------------------------------------------------------------------------------
# image-space kernels: surface normals of the rendered depth and the normal-prior loss (csrc/depthnormal.hip)
# ------------------------------------------------------------------------------------------------
def depth_normal_fwd_bwd(cam: Camera, depth_acc, final_T, prior, conf=None, alpha_min: float = 0.5, max_jump: float = 0.1,
                         weight: float = 1.0, want_grad: bool = True, want_normals: bool = False, accumulate_into=None):
    """-> (stats [8], normals [H,W,3] or None, v_depth [H,W] or None, v_alpha [H,W] or None).  (tgs_depth_normal_fwd_bwd)

    Normals n of the surface through the back-projected expected depths ``depth_acc / max(1 - final_T, 1e-10)`` (central
    differences over a pixel's four neighbours, OpenCV camera axes, facing the camera; formed where the five pixels have
    ``1 - final_T >= alpha_min`` and the depth steps by at most ``max_jump`` of the centre's depth, ``max_jump <= 0`` = no
    gate), and the loss ``weight * sum c (1 - n . prior / |prior|) / sum c`` over the formed centres with a prior of non-zero
    length and ``conf`` c > 0 (``conf=None``: 1 everywhere; ``prior=None``: no supervision).
    stats = {formed centres, supervised centres, sum c, mean 1 - cos, weight * mean, 0, 0, 0}; ``v_depth`` / ``v_alpha`` =
    gradient of the loss with respect to ``depth_acc`` / ``1 - final_T``: the upstream images :func:`rasterize_bwd` takes.
    ``accumulate_into=(v_depth, v_alpha)``: the gradient is ADDED to these two images (those :func:`depth_corr_fwd_bwd`
    wrote, on the same stream) and they are returned.  No supervised centre: loss 0 and zero gradients.  No host sync.
    """
    lib = _lib.load()
    depth_acc, final_T = _f32c(depth_acc.detach()), _f32c(final_T.detach())
    H, W = cam.H, cam.W
    if depth_acc.shape != (H, W) or final_T.shape != (H, W):
        raise ValueError(f"depth_acc and final_T must be [H,W] = [{H},{W}] of the camera, got {tuple(depth_acc.shape)}, "
                         f"{tuple(final_T.shape)}")
    prior, conf = _f32c(prior), _f32c(conf)
    if prior is not None and prior.shape != (H, W, 3):
        raise ValueError(f"prior must be [H,W,3], got {tuple(prior.shape)}")
    if conf is not None and (prior is None or conf.shape != (H, W)):
        raise ValueError("conf must be [H,W] and needs a prior")
    dev = depth_acc.device
    tiles = torch.empty(((H + 15) // 16) * ((W + 15) // 16), 4, dtype=torch.float32, device=dev)
    stats = torch.empty(8, dtype=torch.float32, device=dev)
    normals = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if want_normals else None
    v_depth = v_alpha = None
    if accumulate_into is not None:
        v_depth, v_alpha = accumulate_into
        for t in (v_depth, v_alpha):
            if t.dtype != torch.float32 or t.shape != (H, W) or not t.is_contiguous() or t.device != dev:
                raise ValueError("accumulate_into must be two contiguous float32 [H,W] images on the images' device")
    elif want_grad:
        v_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        v_alpha = torch.empty(H, W, dtype=torch.float32, device=dev)
    cs = cam.c_struct()
    check(lib.tgs_depth_normal_fwd_bwd(C.byref(cs), ptr(depth_acc), ptr(final_T), ptr(prior), ptr(conf), C.c_float(alpha_min),
                                       C.c_float(max_jump), C.c_float(weight), ptr(tiles), ptr(stats), ptr(normals),
                                       ptr(v_depth), ptr(v_alpha), 1 if accumulate_into is not None else 0, _stream()),
          "tgs_depth_normal_fwd_bwd")
    return stats, normals, v_depth, v_alpha


def depth_normals(cam: Camera, depth_acc, final_T, alpha_min: float = 0.5, max_jump: float = 0.1):
    """The normals image [H,W,3] of :func:`depth_normal_fwd_bwd` alone (forward only, no prior): unit normals in OpenCV camera
    axes on the formed centres, exactly 0 elsewhere."""
    return depth_normal_fwd_bwd(cam, depth_acc, final_T, None, None, alpha_min, max_jump, 0.0, want_grad=False,
                                want_normals=True)[1]


class _DepthNormalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_acc, alpha, prior, conf, cam, alpha_min, max_jump):
        # 1 - (1 - T) restores the bits of 1 - T for every T in [0, 1]: the kernel sees the alpha the renderer returned
        stats, _, v_depth, v_alpha = depth_normal_fwd_bwd(cam, depth_acc, 1.0 - alpha.detach(), prior, conf, alpha_min, max_jump,
                                                          weight=1.0)
        ctx.save_for_backward(v_depth, v_alpha)
        return stats[3].clone()

    @staticmethod
    def backward(ctx, g):
        v_depth, v_alpha = ctx.saved_tensors
        return g * v_depth, g * v_alpha, None, None, None, None, None


def depth_normal_loss(cam: Camera, depth_acc, alpha, prior, conf=None, alpha_min: float = 0.5, max_jump: float = 0.1):
    """The conf-weighted mean of 1 - cos(angle between the depth-derived normal and the prior) over the supervised centres
    (:func:`depth_normal_fwd_bwd`), a device scalar differentiable in ``depth_acc`` and ``alpha`` with validity, the gates and
    the weight sum held constant; ``depth_acc`` / ``alpha`` as :func:`render` returns them.  No host sync."""
    return _DepthNormalLoss.apply(depth_acc, alpha, prior, conf, cam, alpha_min, max_jump)


# ------------------------------------------------------------------------------------------------
# per-view exposure compensation C' = A C + b (csrc/exposure.hip)
# ------------------------------------------------------------------------------------------------
def _expo_row(expo, what: str):
    """The 12 floats E = [A | b] (row-major 3x4) a kernel reads: a [3,4] / [12] tensor, or the head of a [48] state row."""
    if not expo.is_cuda or expo.dtype != torch.float32 or not expo.is_contiguous() or expo.numel() < 12:
        raise ValueError(f"{what}: expo must be a contiguous float32 device tensor of at least 12 elements")
    return expo


def _dev_buf(t, n: int, who: str, what: str, dev, dtype=torch.float32, exact: bool = False):
    """A buffer a kernel of ``who`` writes (or the guard it reads): on the frame's device, contiguous, of the dtype and size
    it assumes."""
    if (not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or not t.is_contiguous()
            or (t.numel() != n if exact else t.numel() < n)):
        raise ValueError(f"{who}: {what} must be a contiguous {dtype} tensor on {dev} of "
                         f"{'' if exact else 'at least '}{n} elements")
    return t


def _rgb_images(who: str, rgb, gt=None, v_img=None, out=None):
    """The images of a colour-correction op of ``who`` -> (rgb [H,W,3] detached, gt, v_img, out): float32 and contiguous,
    ``gt`` / ``v_img`` of rgb's shape or None, ``out`` a caller's image of rgb's shape or None."""
    rgb, gt, v_img = _f32c(rgb.detach()), _f32c(gt), _f32c(v_img)
    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise ValueError(f"{who}: rgb must be [H,W,3], got {tuple(rgb.shape)}")
    for name, t in (("gt", gt), ("v_img", v_img)):
        if t is not None and t.shape != rgb.shape:
            raise ValueError(f"{who}: {name} {tuple(t.shape)} does not match rgb {tuple(rgb.shape)}")
    if out is not None and (out.device != rgb.device or out.dtype != torch.float32 or not out.is_contiguous()
                            or out.shape != rgb.shape):
        raise ValueError(f"{who}: out must be a contiguous float32 tensor of rgb's shape on rgb's device")
    return rgb, gt, v_img, out


def exposure_fwd(rgb, expo, out=None):
    """-> C' [H,W,3] with C'[p][c] = sum_k A[c][k] rgb[p][k] + b[c]; ``expo`` = E = [A | b] on the device ([3,4], [12] or a
    view's [48] state row).  No clamp.  No host sync.  (tgs_exposure_fwd)"""
    lib = _lib.load()
    rgb, _, _, out = _rgb_images("exposure_fwd", rgb, out=out)
    H, W = rgb.shape[0], rgb.shape[1]
    out = torch.empty_like(rgb) if out is None else out
    check(lib.tgs_exposure_fwd(W, H, ptr(rgb), ptr(_expo_row(expo, "exposure_fwd")), ptr(out), _stream()), "tgs_exposure_fwd")
    return out


def exposure_bwd(rgb, expo, gt=None, l1_weight: float = 0.0, v_img=None, guard=None, state=None, adam=None, out=None):
    """The backward of :func:`exposure_fwd` with the L1 term taken on C' -> (out32, v_rgb).  (tgs_exposure_bwd)

    ``v' = v_img + l1_weight * sign(C' - gt)`` (either image may be None), ``v_rgb = A^T v'`` is the upstream image
    :func:`rasterize_bwd` takes (with a loss spec WITHOUT ``gt_rgb``), ``out32`` = G [3,4] row-major | its 12 masses | valid
    flag | ``l1_weight * sum |C' - gt|`` | pixel count | zeros.  ``guard`` = the frame's status word: an overflowed frame
    gives all zeros and leaves ``state`` alone.  ``state`` = a view's [48] row (:class:`touch_gs_amd.exposure.ExposureSet`),
    stepped in the same call with ``adam = dict(lr, betas, eps, l2)``; None = gradient only.  ``expo`` may be ``state``.
    ``out`` = (result [32], scratch [tgs_exposure_num_partials, 32]) to allocate nothing but ``v_rgb``.  No host sync."""
    lib = _lib.load()
    who = "exposure_bwd"
    rgb, gt, v_img, _ = _rgb_images(who, rgb, gt, v_img)
    H, W = rgb.shape[0], rgb.shape[1]
    dev = rgb.device
    P = lib.tgs_exposure_num_partials(W, H)
    if out is None:
        out = (torch.empty(_lib.EXPO_OUT, dtype=torch.float32, device=dev),
               torch.empty(P, _lib.EXPO_OUT, dtype=torch.float32, device=dev))
    res, scratch = out
    _dev_buf(res, _lib.EXPO_OUT, who, "out[0] (the result)", dev, exact=True)
    _dev_buf(scratch, P * _lib.EXPO_OUT, who, "out[1] (the scratch, [tgs_exposure_num_partials(W, H), 32])", dev)
    if guard is not None:
        _dev_buf(guard, 2, who, "guard (the frame's status word)", dev, dtype=torch.int32)
    lr = b1 = b2 = eps = l2 = 0.0
    if state is not None:
        if adam is None:
            raise ValueError("exposure_bwd: a state row needs adam = dict(lr, betas, eps, l2)")
        _dev_buf(state, _lib.EXPO_STATE, who, "state (a view's row)", dev, exact=True)
        lr, (b1, b2), eps, l2 = adam["lr"], adam.get("betas", (0.9, 0.999)), adam.get("eps", 1e-15), adam.get("l2", 0.0)
    v_rgb = torch.empty_like(rgb)
    check(lib.tgs_exposure_bwd(W, H, ptr(rgb), ptr(_expo_row(expo, "exposure_bwd")), ptr(gt), C.c_float(l1_weight), ptr(v_img),
                               ptr(v_rgb), ptr(scratch), ptr(res), ptr(guard), ptr(state), C.c_float(lr), C.c_float(b1),
                               C.c_float(b2), C.c_float(eps), C.c_float(l2), _stream()), "tgs_exposure_bwd")
    return res, v_rgb


class _ApplyExposure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, E):
        Ed = _f32c(E.detach())
        ctx.save_for_backward(rgb.detach(), Ed)
        return exposure_fwd(rgb, Ed)

    @staticmethod
    def backward(ctx, g):
        rgb, Ed = ctx.saved_tensors
        out32, v_rgb = exposure_bwd(rgb, Ed, gt=None, l1_weight=0.0, v_img=g)
        return v_rgb, out32[:12].view(3, 4).clone()


def apply_exposure(rgb, E):
    """C' = A rgb + b for E = [A | b] [3,4] on the device, differentiable in ``rgb`` and ``E`` (the two kernels of
    :func:`exposure_fwd` / :func:`exposure_bwd`): what the gsplat-shaped and INRIA-shaped surfaces compose with their own
    losses.  No host sync."""
    if E.shape != (3, 4):
        raise ValueError(f"apply_exposure: E must be [3,4], got {tuple(E.shape)}")
    return _ApplyExposure.apply(rgb, E)


# ------------------------------------------------------------------------------------------------
# per-view bilateral grid C' = A(p) C + b(p) (csrc/bilagrid.hip)
# ------------------------------------------------------------------------------------------------
def bilagrid_sizes(W: int, H: int, shape):
    """-> (n, scratch floats) of a W x H frame under a grid of ``shape`` = (GW, GH, L): n = GH GW L 12 entries, and the
    scratch :func:`bilagrid_bwd` needs (tgs_bilagrid_scratch_floats).  Functions of the five integers alone."""
    GW, GH, L = (int(x) for x in shape)
    s = _lib.load().tgs_bilagrid_scratch_floats(W, H, GW, GH, L)
    if s == 0:
        raise ValueError(f"bilagrid: bad sizes: image {W} x {H}, grid (GW, GH, L) = {(GW, GH, L)} "
                         "(every grid dimension >= 2, GW and GH <= 4096, L <= 64)")
    return GH * GW * L * 12, int(s)


def _bila_grid(grid, shape, what: str):
    """The n = GH GW L 12 floats a kernel reads: a [GH,GW,L,12] / [n] tensor, or the head of a view's [3n+16] state row."""
    GW, GH, L = (int(x) for x in shape)
    n = GH * GW * L * 12
    if (not torch.is_tensor(grid) or not grid.is_cuda or grid.dtype != torch.float32 or not grid.is_contiguous()
            or grid.numel() < n):
        raise ValueError(f"{what}: grid must be a contiguous float32 device tensor of at least GH GW L 12 = {n} elements")
    return grid


def bilagrid_fwd(rgb, grid, shape, out=None):
    """-> C' [H,W,3]: ``rgb`` through the bilateral grid ``grid`` ([GH,GW,L,12], the last axis a row-major 3x4 [A | b]; or a
    view's state row) of ``shape`` = (GW, GH, L), sliced trilinearly at the pixel's position and the luminance of its
    colour.  No clamp.  No host sync.  (tgs_bilagrid_fwd)"""
    lib = _lib.load()
    rgb, _, _, out = _rgb_images("bilagrid_fwd", rgb, out=out)
    H, W = rgb.shape[0], rgb.shape[1]
    GW, GH, L = (int(x) for x in shape)
    bilagrid_sizes(W, H, shape)
    out = torch.empty_like(rgb) if out is None else out
    check(lib.tgs_bilagrid_fwd(W, H, GW, GH, L, ptr(rgb), ptr(_bila_grid(grid, shape, "bilagrid_fwd")), ptr(out), _stream()),
          "tgs_bilagrid_fwd")
    return out


def bilagrid_bwd(rgb, grid, shape, gt=None, l1_weight: float = 0.0, v_img=None, tv_weight: float = 0.0, guard=None,
                 state=None, adam=None, want_grad: bool = True, out=None):
    """The backward of :func:`bilagrid_fwd` with the L1 term taken on C' -> (out8, v_rgb, grad).  (tgs_bilagrid_bwd)

    ``v' = v_img + l1_weight * sign(C' - gt)`` (either image may be None); ``v_rgb`` (the guide's gradient included) is the
    upstream image :func:`rasterize_bwd` takes (with a loss spec WITHOUT ``gt_rgb``); ``grad`` [2, n] = dL/dgrid of the data
    term, then its masses (None with ``want_grad=False``, which needs ``state``); ``out8`` = valid flag |
    ``l1_weight * sum |C' - gt|`` | pixel count | TV(grid), unweighted | zeros.  ``guard`` = the frame's status word: an
    overflowed frame gives a zero ``out8`` and leaves ``state`` alone.  ``state`` = a view's [3n+16] row
    (:class:`touch_gs_amd.bilagrid.BilagridSet`), stepped in the same call on ``G + tv_weight dTV`` with
    ``adam = dict(lr, betas, eps)``; None = gradient only.  ``grid`` may be ``state``.
    ``out`` = (result [8], scratch [>= bilagrid_sizes(W, H, shape)[1]]) to allocate nothing but ``v_rgb`` and ``grad``;
    (result, scratch, v_rgb [H,W,3]) or (result, scratch, v_rgb, grad [2, n]) to allocate nothing.  No host sync."""
    lib = _lib.load()
    who = "bilagrid_bwd"
    rgb, gt, v_img, _ = _rgb_images(who, rgb, gt, v_img)
    H, W = rgb.shape[0], rgb.shape[1]
    GW, GH, L = (int(x) for x in shape)
    dev = rgb.device
    n, S = bilagrid_sizes(W, H, shape)
    if out is None:
        out = (torch.empty(_lib.BILAGRID_OUT, dtype=torch.float32, device=dev), torch.empty(S, dtype=torch.float32, device=dev))
    res, scratch = out[0], out[1]
    _dev_buf(res, _lib.BILAGRID_OUT, who, "out[0] (the result)", dev, exact=True)
    _dev_buf(scratch, S, who, "out[1] (the scratch, tgs_bilagrid_scratch_floats floats)", dev)
    if guard is not None:
        _dev_buf(guard, 2, who, "guard (the frame's status word)", dev, dtype=torch.int32)
    lr = b1 = b2 = eps = 0.0
    if state is not None:
        if adam is None:
            raise ValueError("bilagrid_bwd: a state row needs adam = dict(lr, betas, eps)")
        _dev_buf(state, 3 * n + _lib.BILAGRID_TAIL, who, "state (a view's row)", dev, exact=True)
        lr, (b1, b2), eps = adam["lr"], adam.get("betas", (0.9, 0.999)), adam.get("eps", 1e-15)
    elif not want_grad:
        raise ValueError("bilagrid_bwd: want_grad=False needs a state row to step")
    grad = None
    if want_grad:
        grad = _dev_buf(out[3], 2 * n, who, "out[3] (grad, [2, n])", dev, exact=True) if len(out) > 3 else \
            torch.empty(2, n, dtype=torch.float32, device=dev)
    v_rgb = _dev_buf(out[2], rgb.numel(), who, "out[2] (v_rgb)", dev, exact=True) if len(out) > 2 else torch.empty_like(rgb)
    check(lib.tgs_bilagrid_bwd(W, H, GW, GH, L, ptr(rgb), ptr(_bila_grid(grid, shape, "bilagrid_bwd")), ptr(gt),
                               C.c_float(l1_weight), ptr(v_img), C.c_float(tv_weight), ptr(v_rgb), ptr(scratch), ptr(grad),
                               ptr(res), ptr(guard), ptr(state), C.c_float(lr), C.c_float(b1), C.c_float(b2), C.c_float(eps),
                               _stream()), "tgs_bilagrid_bwd")
    return res, v_rgb, grad


class _ApplyBilagrid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb, grid):
        gd = _f32c(grid.detach())
        ctx.save_for_backward(rgb.detach(), gd)
        GH, GW, L = gd.shape[:3]
        return bilagrid_fwd(rgb, gd, (GW, GH, L))

    @staticmethod
    def backward(ctx, g):
        rgb, gd = ctx.saved_tensors
        GH, GW, L = gd.shape[:3]
        _, v_rgb, grad = bilagrid_bwd(rgb, gd, (GW, GH, L), gt=None, l1_weight=0.0, v_img=g)
        return v_rgb, grad[0].view(gd.shape)


def apply_bilagrid(rgb, grid):
    """C' = A(p) rgb + b(p) for a bilateral grid ``grid`` [GH,GW,L,12] on the device, differentiable in ``rgb`` (the guide's
    gradient included) and in ``grid`` (the two kernels of :func:`bilagrid_fwd` / :func:`bilagrid_bwd`): what the
    gsplat-shaped and INRIA-shaped surfaces compose with their own losses.  No host sync."""
    if grid.dim() != 4 or grid.shape[3] != 12:
        raise ValueError(f"apply_bilagrid: grid must be [GH,GW,L,12], got {tuple(grid.shape)}")
    return _ApplyBilagrid.apply(rgb, grid)


# ------------------------------------------------------------------------------------------------
# fixed-budget MCMC strategy (csrc/mcmc.hip, touch_gs_amd/mcmc.py)
# ------------------------------------------------------------------------------------------------
def mcmc_spec(opacity_reg: float = 0.01, scale_reg: float = 0.01, noise_lr: float = 5e5, gate_k: float = 100.0,
              gate_o0: float = 0.005) -> "_lib.TgsMcmcSpec":
    """The TgsMcmcSpec of :func:`mcmc_adam_geom` (defaults: gsplat's MCMC trainer)."""
    s = _lib.TgsMcmcSpec()
    s.opacity_reg, s.scale_reg, s.noise_lr, s.gate_k, s.gate_o0 = opacity_reg, scale_reg, noise_lr, gate_k, gate_o0
    return s


def mcmc_adam_geom(optimizer, mcmc, noise=None, grad_scale: float = 1.0, guard=None) -> None:
    """Regularisers + Adam on the geometry segments + noise on the means, one launch (tgs_mcmc_adam_geom): the step of
    ``optimizer`` (a FusedAdam after ``begin_step``) from ``optimizer.p.grad``; the SH segment is the caller's
    (``optimizer.step_range(optimizer.geom_end(), -1)``).  ``mcmc``: a TgsMcmcSpec (:func:`mcmc_spec`); ``noise``: [N,3]
    standard normal draws on the device, or None = no noise; ``guard``: the frame's status word.  No host sync."""
    lib = _lib.load()
    p = optimizer.p
    if noise is not None:
        if noise.dtype != torch.float32 or not noise.is_contiguous() or noise.shape != (p.N, 3) or noise.device != p.flat.device:
            raise ValueError(f"mcmc_adam_geom: noise must be a contiguous float32 [{p.N}, 3] tensor on {p.flat.device}")
    if guard is not None and (guard.dtype != torch.int32 or guard.numel() < 2 or guard.device != p.flat.device):
        raise ValueError("mcmc_adam_geom: guard must be the frame's int32 status word on the parameters' device")
    s = optimizer._spec()
    check(lib.tgs_mcmc_adam_geom(p.N, p.K, ptr(p.flat), ptr(p.grad), ptr(optimizer.exp_avg), ptr(optimizer.exp_avg_sq),
                                 C.byref(s), C.c_float(grad_scale), C.byref(mcmc), ptr(noise), ptr(guard), _stream()),
          "tgs_mcmc_adam_geom")


_RELOC_MAX = 51
_RELOC_TABLE = None


def _reloc_table():
    """[52, 51] float64: row r, column k = C(r, k+1) (-1)^k / sqrt(k+1) for k < r, else 0."""
    global _RELOC_TABLE
    if _RELOC_TABLE is None:
        t = torch.zeros(_RELOC_MAX + 1, _RELOC_MAX, dtype=torch.float64)
        for r in range(1, _RELOC_MAX + 1):
            for k in range(r):
                t[r, k] = float(math.comb(r, k + 1)) * (-1.0) ** k / math.sqrt(k + 1)
        _RELOC_TABLE = t
    return _RELOC_TABLE


def mcmc_relocate(ratio, opac_logit, log_scales, min_opacity: float = 0.005) -> None:
    """gsplat's ``compute_relocation`` in place on rows that are split ``ratio`` ways (int32 [n], >= 1; 1 = untouched):
    new opacity x = 1 - (1 - o)^(1/r), r = min(ratio, 51), clamped to [min_opacity, 1 - 2^-23], and scales times o / S
    with S = sum_{k<r} C(r, k+1) (-1)^k x^(k+1) / sqrt(k+1), in fp64, rounded once (tgs_mcmc_relocate).  ``opac_logit`` [n],
    ``log_scales`` [n,3]: contiguous float32, written in place.  CPU tensors: the same single sum in torch fp64 (host-side
    callers and tests; the training path is on the device)."""
    n = opac_logit.shape[0]
    if not (0.0 < min_opacity < 1.0):
        raise ValueError("mcmc_relocate: min_opacity must lie in (0, 1)")
    if (ratio.dtype != torch.int32 or ratio.shape != (n,) or opac_logit.dtype != torch.float32 or log_scales.dtype != torch.float32
            or log_scales.shape != (n, 3) or not (ratio.is_contiguous() and opac_logit.is_contiguous() and log_scales.is_contiguous())
            or not (ratio.device == opac_logit.device == log_scales.device)):
        raise ValueError("mcmc_relocate: need ratio int32 [n], opac_logit float32 [n], log_scales float32 [n,3], contiguous, on one device")
    if opac_logit.is_cuda:
        check(_lib.load().tgs_mcmc_relocate(n, ptr(ratio), ptr(opac_logit), ptr(log_scales), C.c_float(min_opacity), _stream()),
              "tgs_mcmc_relocate")
        return
    sel = torch.nonzero(ratio > 1).squeeze(1)
    if sel.numel() == 0:
        return
    r = ratio[sel].clamp(max=_RELOC_MAX).long()
    l = opac_logit[sel].double()
    log_1mo = -torch.nn.functional.softplus(l, beta=1.0, threshold=1e9)        # log(1 - sigmoid(l))
    o = torch.sigmoid(l)
    x = -torch.expm1(log_1mo / r.double())
    pw = x[:, None] ** torch.arange(1, _RELOC_MAX + 1, dtype=torch.float64)[None, :]
    S = (_reloc_table()[r] * pw).sum(1)
    lo = float(torch.tensor(min_opacity, dtype=torch.float32))      # the C float argument carries the fp32 rounding
    xc = x.clamp(min=lo, max=1.0 - 2.0 ** -23)
    opac_logit[sel] = (torch.log(xc) - torch.log1p(-xc)).float()
    log_scales[sel] = (log_scales[sel].double() + torch.log(o / S)[:, None]).float()


# ------------------------------------------------------------------------------------------------
# exact k nearest neighbours (csrc/knn.hip)
# ------------------------------------------------------------------------------------------------
def _knn_points(t, what: str):
    if not (isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] == 3 and t.shape[0] >= 1):
        raise ValueError(f"knn: {what} must be a [n, 3] tensor with n >= 1")
    if t.dtype != torch.float32:
        raise ValueError(f"knn: {what} must be float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError("touch_gs_amd ops need device (HIP) tensors; there is no CPU path")
    if t.shape[0] > (1 << 29) - 1:
        raise ValueError(f"knn: {what} holds more points than the 32-bit index (2^29 - 1)")
    return t.detach().contiguous()


def _knn_bounds(t, what: str):
    """(lo, hi) of a [n,3] device tensor as host floats -- ONE host read; NaN and inf both surface in amin / amax."""
    b = torch.stack([t.amin(0), t.amax(0)]).cpu()
    if not bool(torch.isfinite(b).all()):
        raise ValueError(f"knn: {what} holds non-finite coordinates")
    return (C.c_float * 3)(*b[0].tolist()), (C.c_float * 3)(*b[1].tolist())


def _knn_keys(lib, t, lo, hi):
    """The points' 30-bit Morton keys inside [lo, hi] (int32: the sign bit stays clear)."""
    keys = torch.empty(t.shape[0], dtype=torch.int32, device=t.device)
    check(lib.tgs_knn_keys(t.shape[0], ptr(t), lo, hi, ptr(keys), _stream()), "tgs_knn_keys")
    return keys


def knn(points, k: int, queries=None, exclude_self: Optional[bool] = None, sort_queries: bool = True,
        timing: Optional[dict] = None):
    """The ``k`` nearest ``points`` (float32 [n,3] on the device, the references) of every query: ``(dist2 [n_q,k] float32,
    idx [n_q,k] int32)`` on the device, exact -- d2 = (dx*dx + dy*dy) + dz*dz in fp32, each row ascending, equal d2 by the
    lower index, ``+inf`` / ``-1`` where fewer than k references exist (include/tgs.h).  ``queries=None``: the points
    themselves, each without itself (``exclude_self`` defaults to True then, to False with ``queries``; True needs the
    queries to be the points in their order).  1 <= k <= 16.  Non-finite coordinates raise ValueError.  One host read per
    cloud (the bounds); this is an initialisation / evaluation op, not a per-step one.
    ``sort_queries=False`` serves the queries in their own order instead of Morton order (same result, slower: the lanes of
    a wave then want different boxes).  ``timing``: a dict that receives a device event after each stage -- start, bounds,
    keys, sort, build, query (tools/knn_time.py)."""
    lib = _lib.load()
    if not (isinstance(k, int) and 1 <= k <= _lib.KNN_MAX_K):
        raise ValueError(f"knn: k must be an int in [1, {_lib.KNN_MAX_K}], got {k!r}")
    ref = _knn_points(points, "points")
    n = ref.shape[0]
    self_query = queries is None
    qs = ref if self_query else _knn_points(queries, "queries")
    if qs.device != ref.device:
        raise ValueError("knn: points and queries must be on one device")
    if exclude_self is None:
        exclude_self = self_query
    if exclude_self and qs.shape[0] != n:
        raise ValueError("knn: exclude_self needs the queries to be the points themselves (same count and order)")

    def mark(name):
        if timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            timing[name] = ev

    with torch.cuda.device(ref.device):
        mark("start")
        lo, hi = _knn_bounds(ref, "points")
        if not self_query:
            _knn_bounds(qs, "queries")      # (refuses non-finite queries; their keys are clamped into the references' bounds)
        mark("bounds")
        keys = _knn_keys(lib, ref, lo, hi)
        q_keys = _knn_keys(lib, qs, lo, hi) if (sort_queries and not self_query) else None
        mark("keys")
        order = torch.sort(keys).indices.to(torch.int32)
        q_order = None
        if sort_queries:
            q_order = order if self_query else torch.sort(q_keys).indices.to(torch.int32)
        mark("sort")
        sorted_pts = torch.empty(n, 4, dtype=torch.float32, device=ref.device)
        boxes = torch.empty((n + _lib.KNN_BOX - 1) // _lib.KNN_BOX, 8, dtype=torch.float32, device=ref.device)
        check(lib.tgs_knn_build(n, ptr(ref), ptr(order), ptr(sorted_pts), ptr(boxes), _stream()), "tgs_knn_build")
        mark("build")
        n_q = qs.shape[0]
        dist2 = torch.empty(n_q, k, dtype=torch.float32, device=ref.device)
        idx = torch.empty(n_q, k, dtype=torch.int32, device=ref.device)
        check(lib.tgs_knn_query(n_q, ptr(qs), ptr(q_order), n, ptr(sorted_pts), ptr(boxes), k, int(bool(exclude_self)),
                                ptr(dist2), ptr(idx), _stream()), "tgs_knn_query")
        mark("query")
    return dist2, idx
