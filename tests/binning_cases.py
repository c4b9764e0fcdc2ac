"""Built inputs and an exact reference for the front half (K2-K5: csrc/tgs_binning.h, csrc/binning.hip).

The front half reads two slots of every 12-float splat record -- slot 10, the tile rect packed as
``x0 | y0 << 8 | w << 16 | h << 24``, and slot 2, the depth, which it sorts by its fp32 bits -- and writes slot 11, the
record's exclusive pair offset inside its group of 256 rows.  K1 is therefore not needed: :func:`records` builds the
records directly, and every list length, group total and bounding box of a case is controlled to the unit.

:func:`reference` states App. B.4 / B.6 a second time, in vectorised numpy, independently of
``oracle.torch_oracle.bin_and_sort`` (tests/test_cpu_binning_cases.py holds the two against each other).

A case is a function returning ``Case(W, H, rects, depth_bits, long_run, note)``.  ``rects`` is int64 [N, 4] =
(x0, y0, w, h) in tiles, ``depth_bits`` uint32 [N].  ``note`` names the edge the case stands on as exact properties of
the reference (:func:`properties`): tests/test_cpu_binning_cases.py asserts each of them with ``==``, so a case cannot
drift off its edge unnoticed.  Keys of ``note``:

  lists     {tile: length} of every non-empty tile
  longest   the longest list
  n         number of pairs
  totals    pair total of every group of 256 rows
  areas     per group, the tile area of the bounding box of its members with 0 < hits <= long_run (what
            group_count_tiles compares with TGS_AGG_TILES = 1024; 0 = empty box)
  areas_all per group, the same over all members with hits > 0 (shows that a long member WOULD stretch the box)
  long      rows with hits > long_run
  hits      sorted distinct w * h of the rows

The shapes are the smallest that reach each branch; they are not meant to be scaled up.
"""
import collections
import functools

import numpy as np
import torch

GROUP = 256                 # TGS_GROUP: rows per binning group
AGG_TILES = 1024            # TGS_AGG_TILES
LONG_RUN = 32               # TGS_LONG_RUN, passed explicitly by every case that does not choose its own
FILLER = 0.625              # the record slots the front half must neither read nor write

Case = collections.namedtuple("Case", "W H rects depth_bits long_run note")
Reference = collections.namedtuple("Reference", "sorted_gid tile_start offset n longest need totals")

BITS_LO, BITS_HI = 0x00800000, 0x7F7FFFFF     # the positive normal floats


# ---------------------------------------------------------------------------------------------
# records and reference
# ---------------------------------------------------------------------------------------------
def pack_rects(rects):
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    assert r.min(initial=0) >= 0 and r.max(initial=0) <= 255
    return (r[:, 0] | (r[:, 1] << 8) | (r[:, 2] << 16) | (r[:, 3] << 24)).astype(np.uint32)


def records(rects, depth_bits):
    """float32 [N, 12]: slot 10 = packed rect, slot 2 = depth bits, slot 4 = 1.0 (visible), the rest FILLER."""
    packed = pack_rects(rects)
    bits = np.asarray(depth_bits, np.uint32).reshape(-1)
    assert packed.shape == bits.shape
    rec = np.full((len(packed), 12), FILLER, np.float32)
    rec[:, 4] = 1.0
    words = rec.view(np.uint32)
    words[:, 10] = packed
    words[:, 2] = bits
    return torch.from_numpy(rec)


def expand(rects, TW):
    """Every rect -> its (tile, gid) pairs, row by row of the rect (the pair order inside a group)."""
    r = np.asarray(rects, np.int64).reshape(-1, 4)
    hits = r[:, 2] * r[:, 3]
    gid = np.repeat(np.arange(len(r), dtype=np.int64), hits)
    first = np.cumsum(hits) - hits
    k = np.arange(int(hits.sum()), dtype=np.int64) - first[gid]
    w = np.maximum(r[gid, 2], 1)
    tile = (r[gid, 1] + k // w) * TW + r[gid, 0] + k % w
    return tile, gid, hits


def reference(rects, depth_bits, TW, TH):
    """B.4 / B.6 in numpy: pairs ordered by (tile, depth bits as uint32, gid)."""
    T = TW * TH
    bits = np.asarray(depth_bits, np.uint32).reshape(-1)
    tile, gid, hits = expand(rects, TW)
    order = np.lexsort((gid, bits[gid], tile))
    tile, gid = tile[order], gid[order]
    tile_start = np.searchsorted(tile, np.arange(T + 1), side="left").astype(np.int64)
    N = len(hits)
    G = (N + GROUP - 1) // GROUP
    padded = np.zeros(G * GROUP, np.int64)
    padded[:N] = hits
    per_group = padded.reshape(G, GROUP)
    offset = (np.cumsum(per_group, 1) - per_group).reshape(-1)[:N]
    totals = per_group.sum(1)
    n = int(hits.sum())
    lens = np.diff(tile_start)
    return Reference(sorted_gid=gid, tile_start=tile_start, offset=offset, n=n, longest=int(lens.max(initial=0)),
                     need=n + 8 * int(totals.max(initial=0)), totals=totals)


def properties(case):
    """The exact properties ``note`` speaks about, from the rects and :func:`reference` alone."""
    TW, TH = tiles_of(case)
    ref = reference(case.rects, case.depth_bits, TW, TH)
    r = np.asarray(case.rects, np.int64).reshape(-1, 4)
    hits = r[:, 2] * r[:, 3]
    lens = np.diff(ref.tile_start)

    def area(rows):
        if len(rows) == 0:
            return 0
        q = r[rows]
        return int((q[:, 0] + q[:, 2]).max() - q[:, 0].min()) * int((q[:, 1] + q[:, 3]).max() - q[:, 1].min())

    areas, areas_all = [], []
    for g in range(len(ref.totals)):
        rows = np.arange(g * GROUP, min((g + 1) * GROUP, len(r)))
        areas.append(area(rows[(hits[rows] > 0) & (hits[rows] <= case.long_run)]))
        areas_all.append(area(rows[hits[rows] > 0]))
    return dict(lists={int(t): int(lens[t]) for t in np.nonzero(lens)[0]}, longest=ref.longest, n=ref.n,
                totals=[int(t) for t in ref.totals], areas=areas, areas_all=areas_all,
                long=[int(i) for i in np.nonzero(hits > case.long_run)[0]],
                hits=sorted(int(h) for h in set(hits.tolist())))


def tiles_of(case):
    return (case.W + 15) // 16, (case.H + 15) // 16


# ---------------------------------------------------------------------------------------------
# depth patterns (bit patterns of positive finite floats)
# ---------------------------------------------------------------------------------------------
PATTERNS = ("distinct", "all_equal", "two_values", "ulp_neighbours", "ascending", "descending")


def depths(pattern, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(n, dtype=np.int64)
    step = (BITS_HI - BITS_LO) // max(n, 1)          # spread over every exponent: the high key word decides
    if pattern == "distinct":
        bits = BITS_LO + rng.permutation(n).astype(np.int64) * step
    elif pattern == "all_equal":                      # the order is the id order
        bits = np.full(n, 0x40800000, np.int64)
    elif pattern == "two_values":
        bits = np.where(rng.integers(0, 2, n) == 1, 0x40400000, 0x40000000).astype(np.int64)
    elif pattern == "ulp_neighbours":                 # consecutive bit patterns, dealt in descending id order
        bits = 0x3F800000 + (n - 1 - i)
    elif pattern == "ascending":
        bits = BITS_LO + i * step
    elif pattern == "descending":
        bits = BITS_LO + (n - 1 - i) * step
    else:
        raise KeyError(pattern)
    assert bits.min(initial=BITS_LO) >= BITS_LO and bits.max(initial=BITS_LO) <= BITS_HI
    return bits.astype(np.uint32)


def tied(n, seed):
    """Distinct depths with every third row on one common value: both words of the sort key decide somewhere."""
    bits = depths("distinct", n, seed)
    bits[::3] = 0x40800000
    return bits


def ones_at(tiles, TW):
    """1 x 1 rects on the given tiles."""
    t = np.asarray(tiles, np.int64).reshape(-1)
    return np.stack([t % TW, t // TW, np.ones_like(t), np.ones_like(t)], 1)


def lists_case(W, H, lengths, seed):
    """One 1 x 1 Gaussian per pair, ``lengths`` = {tile: list length}, rows interleaved by a seeded shuffle."""
    TW = (W + 15) // 16
    rng = np.random.default_rng(seed)
    t = np.concatenate([np.full(n, tile, np.int64) for tile, n in lengths.items()] + [np.zeros(0, np.int64)])
    t = t[rng.permutation(len(t))]
    note = dict(lists={int(k): int(v) for k, v in lengths.items() if v > 0}, longest=max(lengths.values()))
    return Case(W, H, ones_at(t, TW), tied(len(t), seed), LONG_RUN, note)


# ---------------------------------------------------------------------------------------------
# sort cases
# ---------------------------------------------------------------------------------------------
ONE_TILE_N = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
              4095, 4096, 4097, 16383, 16384, 16385, 32769)
ONE_TILE_ALL_PATTERNS = (512, 513, 1024, 1025, 4096, 4097)


def one_tile(n, pattern="distinct"):
    """``n`` Gaussians on the only tile of a 16 x 16 image: every length the sort kernels branch on."""
    totals = [GROUP] * (n // GROUP) + ([n % GROUP] if n % GROUP else [])
    note = dict(lists={0: n} if n else {}, longest=n, n=n, totals=totals)
    return Case(16, 16, ones_at(np.zeros(n, np.int64), 1), depths(pattern, n, n), LONG_RUN, note)


def mixed_classes():
    """One list of every class in one frame; every group of 256 rows feeds several tiles."""
    lengths = {3: 1, 9: 64, 14: 65, 20: 512, 27: 513, 33: 1024, 42: 1025, 54: 2049, 63: 4097}
    return lists_case(128, 128, lengths, 11)


def wg4_stride():
    """T = 2209 > 2048 blocks of k_sort_tiles_wg4: block b sorts tile b and then tile b + 2048 -- twice the <16, 4> form
    (5, 2053), the <4, 4> then the <16, 4> form (6, 2054), a skipped short list then a long one (7, 2055)."""
    lengths = {5: 1025, 2053: 1025, 6: 600, 2054: 2049, 7: 3, 2055: 1500}
    return lists_case(752, 752, lengths, 12)


def huge_stride():
    """T = 289 > 256 blocks of k_sort_tiles_huge: the LDS sort then the global-memory network in one block (3, 259), and
    the other order (4, 260)."""
    lengths = {3: 4097, 259: 16385, 4: 16385, 260: 4097}
    return lists_case(272, 272, lengths, 13)


# ---------------------------------------------------------------------------------------------
# counting cases
# ---------------------------------------------------------------------------------------------
def spread(rng, n, ox, oy, bw, bh):
    """``n`` tile positions in the box [ox, ox + bw) x [oy, oy + bh), the first ones in its corners."""
    x = ox + rng.integers(0, bw, n)
    y = oy + rng.integers(0, bh, n)
    cx, cy = [ox, ox + bw - 1, ox, ox + bw - 1], [oy, oy, oy + bh - 1, oy + bh - 1]
    x[:4], y[:4] = cx, cy
    return x, y


BOXES = {(1, 1): (48, 48, 1, 1), (32, 32): (640, 640, 5, 7), (25, 41): (480, 800, 3, 6),
         (255, 1): (4080, 16, 0, 0), (1, 255): (16, 4080, 0, 0)}


def box(bw, bh):
    """One group of 256 1 x 1 rects whose bounding box is exactly bw x bh tiles (1024: aggregated, 1025: direct)."""
    W, H, ox, oy = BOXES[(bw, bh)]
    rng = np.random.default_rng(100 * bw + bh)
    x, y = spread(rng, GROUP, ox, oy, bw, bh)
    rects = np.stack([x, y, np.ones_like(x), np.ones_like(x)], 1)
    return Case(W, H, rects, tied(GROUP, bw + bh), LONG_RUN, dict(areas=[bw * bh], totals=[GROUP], n=GROUP))


# k -> (number of 4 x 4, 2 x 2 and 1 x 1 rects).  256 rows of 2 x 2 and 1 x 1 alone reach 1024 and no total that is
# 3 (mod 4) below it, so a few 4 x 4 rects (16 tiles, still short runs) make up the difference.
TOTALS = {1023: (1, 251, 3), 1024: (0, 256, 0), 1025: (1, 252, 1), 2049: (120, 32, 1)}


def total(k):
    """One group of exactly ``k`` pairs inside a 32 x 32 box (aggregated path): the pairs of index >= 1024 = 4 x 256 no
    longer fit the registers of the histogram path and are counted directly."""
    a, b, c = TOTALS[k]
    assert 16 * a + 4 * b + c == k and a + b + c <= GROUP
    rng = np.random.default_rng(k)
    side = np.concatenate([np.full(a, 4), np.full(b, 2), np.full(c, 1)])
    side = side[rng.permutation(len(side))]
    ox, oy, bs = 4, 3, 32
    x = ox + rng.integers(0, bs - side + 1)
    y = oy + rng.integers(0, bs - side + 1)
    x[0], y[0] = ox, oy                                      # two opposite corners pin the box to 32 x 32
    x[1], y[1] = ox + bs - side[1], oy + bs - side[1]
    rects = np.stack([x, y, side, side], 1)
    return Case(640, 640, rects, tied(len(side), k), LONG_RUN, dict(areas=[AGG_TILES], totals=[k], n=k))


# long_run -> rect shapes (w, h) of  long_run - 1, long_run  and the next count above long_run that a rect of 8-bit
# sides can have (257 is prime: 258 = 6 x 43 stands for 256 + 1)
RUNS = {1: ((0, 0), (1, 1), (2, 1)), 32: ((1, 31), (8, 4), (3, 11)), 256: ((15, 17), (16, 16), (6, 43))}


def runs(long_run):
    """Members on both sides of ``hits > long_run``.  The short ones span exactly 32 x 32 tiles; the long ones lie
    anywhere, one of them far away: if it counted towards the box the group would leave the aggregated path."""
    shapes = RUNS[long_run]
    rng = np.random.default_rng(7 + long_run)
    per = 20
    w = np.repeat([s[0] for s in shapes], per)
    h = np.repeat([s[1] for s in shapes], per)
    ox, oy, bs = 2, 2, 32
    x = ox + rng.integers(0, np.maximum(bs - w, 0) + 1)
    y = oy + rng.integers(0, np.maximum(bs - h, 0) + 1)
    k = per                                                   # the members of exactly long_run tiles pin the box
    x[k], y[k] = ox, oy
    x[k + 1], y[k + 1] = ox + bs - w[k + 1], oy + bs - h[k + 1]
    w, h = np.append(w, shapes[2][0]), np.append(h, shapes[2][1])             # the far member, against the image corner
    x, y = np.append(x, 64 - shapes[2][0]), np.append(y, 64 - shapes[2][1])
    order = rng.permutation(len(w))
    rects = np.stack([x, y, w, h], 1)[order]
    hits = rects[:, 2] * rects[:, 3]
    long_rows = [int(i) for i in np.nonzero(hits > long_run)[0]]
    assert len(long_rows) == per + 1
    note = dict(areas=[AGG_TILES], areas_all=[62 * 62], long=long_rows, totals=[int(hits.sum())],
                hits=sorted({s[0] * s[1] for s in shapes}))
    return Case(1024, 1024, rects, tied(len(w), long_run), long_run, note)


def all_long():
    """Every member is a long run: the group's box is empty (area 0) and every pair is counted directly."""
    rng = np.random.default_rng(21)
    n = 64
    x, y = rng.integers(0, 20 - 6 + 1, n), rng.integers(0, 20 - 6 + 1, n)
    rects = np.stack([x, y, np.full(n, 6), np.full(n, 6)], 1)
    return Case(320, 320, rects, tied(n, 21), LONG_RUN, dict(areas=[0], long=list(range(n)), totals=[36 * n]))


def long_and_invisible():
    """Long runs and records without tiles (w = 0, h = 0 or both) and nothing else: still an empty box."""
    rng = np.random.default_rng(22)
    n = 64
    x, y = rng.integers(0, 20 - 7 + 1, n), rng.integers(0, 20 - 5 + 1, n)
    rects = np.stack([x, y, np.full(n, 7), np.full(n, 5)], 1)
    rects[1::4, 2] = 0
    rects[2::4, 3] = 0
    rects[3::8, 2:] = 0
    vis = rects[:, 2] * rects[:, 3] > 0
    note = dict(areas=[0], long=[int(i) for i in np.nonzero(vis)[0]], totals=[35 * int(vis.sum())], hits=[0, 35])
    return Case(320, 320, rects, tied(n, 22), LONG_RUN, note)


GROUPS_N = (1, 255, 256, 257, 513)


def groups(N):
    """N rows around the group size; every rect touches the right and the bottom edge of the image."""
    TW, TH = 5, 4
    rng = np.random.default_rng(30 + N)
    w, h = rng.integers(1, TW + 1, N), rng.integers(1, TH + 1, N)
    w[0], h[0] = TW, TH
    rects = np.stack([TW - w, TH - h, w, h], 1)
    hits = w * h
    totals = [int(hits[g:g + GROUP].sum()) for g in range(0, N, GROUP)]
    return Case(80, 64, rects, tied(N, N), LONG_RUN, dict(totals=totals, n=int(hits.sum()), long=[]))


def empty_group_between():
    """768 rows; the middle group has records without tiles only (total 0: no pair range, no counting)."""
    rng = np.random.default_rng(41)
    N, TW, TH = 768, 6, 6
    w, h = rng.integers(1, 4, N), rng.integers(1, 4, N)
    x, y = rng.integers(0, TW - w + 1), rng.integers(0, TH - h + 1)
    rects = np.stack([x, y, w, h], 1)
    mid = np.arange(GROUP, 2 * GROUP)
    rects[mid[0::3], 2] = 0
    rects[mid[1::3], 3] = 0
    rects[mid[2::3], 2:] = 0
    hits = rects[:, 2] * rects[:, 3]
    totals = [int(hits[:GROUP].sum()), 0, int(hits[2 * GROUP:].sum())]
    return Case(96, 96, rects, tied(N, 41), LONG_RUN, dict(totals=totals, long=[]))


def hot_tile():
    """Four groups of 256 all on tile 0 of a 3 x 3-tile image (one counter takes every atomic) and one 3 x 3 rect."""
    rects = np.concatenate([ones_at(np.zeros(4 * GROUP, np.int64), 3), [[0, 0, 3, 3]]])
    lists = {t: 1 for t in range(9)}
    lists[0] = 4 * GROUP + 1
    return Case(48, 48, rects, tied(len(rects), 51), LONG_RUN, dict(lists=lists, totals=[GROUP] * 4 + [9], areas=[1] * 4 + [9]))


def full_image():
    """255 x 255 tiles (the limit of the packed rect), T = 65025: 64 scan workgroups.  One rect covers the image; a 1 x 1
    rect sits in the first and the last tile of every 1024-tile block of the scan, one more in tile T - 1."""
    TW = TH = 255
    T = TW * TH
    t = []
    for b in range((T + 1023) // 1024):
        t += [1024 * b, min(1024 * b + 1023, T - 1)]
    t.append(T - 1)
    rects = np.concatenate([[[0, 0, TW, TH]], ones_at(t, TW)])
    lists = {k: 1 for k in range(T)}
    for k in t:
        lists[k] += 1
    n = T + len(t)
    return Case(4080, 4080, rects, tied(len(rects), 61), LONG_RUN, dict(n=n, totals=[n], long=[0], longest=3, lists=lists, areas=[TW * TH]))


# ---------------------------------------------------------------------------------------------
# scan cases
# ---------------------------------------------------------------------------------------------
TILES = {1: (16, 16), 1023: (528, 496), 1024: (512, 512), 1025: (400, 656), 2050: (400, 1312)}


def tiles(T):
    """One pair in tile 0 and one in tile T - 1, two in each of tiles 1023 and 1024 (the seam of the scan's workgroups)."""
    W, H = TILES[T]
    TW, TH = (W + 15) // 16, (H + 15) // 16
    assert TW * TH == T
    t = [0, T - 1]
    for seam in (1023, 1024):
        if seam < T:
            t += [seam, seam]
    lists = collections.Counter(t)
    return Case(W, H, ones_at(t, TW), depths("descending", len(t), T), LONG_RUN, dict(lists=dict(lists), n=len(t)))


# ---------------------------------------------------------------------------------------------
# registry
# ---------------------------------------------------------------------------------------------
def _registry():
    reg = collections.OrderedDict()
    for n in ONE_TILE_N:
        pats = PATTERNS if n in ONE_TILE_ALL_PATTERNS else ("distinct", "all_equal")
        for p in pats:
            reg[f"one_tile-{n}-{p}"] = functools.partial(one_tile, n, p)
    for f in (mixed_classes, wg4_stride, huge_stride):
        reg[f.__name__] = f
    for bw, bh in BOXES:
        reg[f"box-{bw}x{bh}"] = functools.partial(box, bw, bh)
    for k in TOTALS:
        reg[f"total-{k}"] = functools.partial(total, k)
    for lr in RUNS:
        reg[f"runs-{lr}"] = functools.partial(runs, lr)
    for f in (all_long, long_and_invisible):
        reg[f.__name__] = f
    for N in GROUPS_N:
        reg[f"groups-{N}"] = functools.partial(groups, N)
    for f in (empty_group_between, hot_tile, full_image):
        reg[f.__name__] = f
    for T in TILES:
        reg[f"tiles-{T}"] = functools.partial(tiles, T)
    return reg


CASES = _registry()


@functools.lru_cache(maxsize=None)
def get(name):
    """The case and its reference, built once and shared (callers must not modify them)."""
    c = CASES[name]()
    c = c._replace(rects=np.ascontiguousarray(c.rects, dtype=np.int64), depth_bits=np.asarray(c.depth_bits, np.uint32))
    TW, TH = tiles_of(c)
    ref = reference(c.rects, c.depth_bits, TW, TH)
    for a in (c.rects, c.depth_bits, *[x for x in ref if isinstance(x, np.ndarray)]):
        a.setflags(write=False)
    return c, ref
