"""The built cases of tests/binning_cases.py stand where they claim to stand, and its reference is right: no GPU here.

Every property a case's ``note`` names is asserted with ``==`` on the reference alone -- a case that drifted off its edge
(a list of 1024 instead of 1025 entries, a box of 1023 tiles) fails here, not silently on the GPU.  The reference is held
against ``oracle.torch_oracle.bin_and_sort``, the other statement of App. B.4 / B.6, on every case and on projected scenes.
"""
import numpy as np
import pytest
import torch

from oracle import torch_oracle as O
from tests import binning_cases as B
from tests.util import scene, splat_fields

NAMES = list(B.CASES)


def oracle_lists(rects, depth_bits, W, H):
    r = torch.from_numpy(np.array(rects, np.int64).reshape(-1, 4))
    rect = torch.stack([r[:, 0], r[:, 1], r[:, 0] + r[:, 2], r[:, 1] + r[:, 3]], 1)
    depth = torch.from_numpy(np.asarray(depth_bits, np.uint32).view(np.float32).copy())
    cam = O.Camera(viewmat=torch.eye(4, dtype=torch.float64), fx=1.0, fy=1.0, cx=0.0, cy=0.0, W=W, H=H)
    return O.bin_and_sort(rect, r[:, 2] * r[:, 3] > 0, depth, cam)


def test_the_issue_list_of_cases_is_complete():
    assert len(NAMES) == len(set(NAMES))
    for n in B.ONE_TILE_N:
        pats = B.PATTERNS if n in (512, 513, 1024, 1025, 4096, 4097) else ("distinct", "all_equal")
        assert [k for k in NAMES if k.startswith(f"one_tile-{n}-")] == [f"one_tile-{n}-{p}" for p in pats]
    assert len(B.ONE_TILE_N) == 28 and len(B.PATTERNS) == 6
    for k in ("mixed_classes", "wg4_stride", "huge_stride", "box-1x1", "box-32x32", "box-25x41", "box-255x1", "box-1x255",
              "total-1023", "total-1024", "total-1025", "total-2049", "runs-1", "runs-32", "runs-256", "all_long",
              "long_and_invisible", "groups-1", "groups-255", "groups-256", "groups-257", "groups-513",
              "empty_group_between", "hot_tile", "full_image", "tiles-1", "tiles-1023", "tiles-1024", "tiles-1025",
              "tiles-2050"):
        assert k in B.CASES, k


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_fits_and_stands_on_its_edge(name):
    c, ref = B.get(name)
    TW, TH = B.tiles_of(c)
    r = c.rects
    assert r.shape == (len(c.depth_bits), 4) and c.depth_bits.dtype == np.uint32
    assert TW <= 255 and TH <= 255 and 1 <= c.long_run <= 256
    assert r.min(initial=0) >= 0 and r.max(initial=0) <= 255                       # the 8-bit fields
    assert ((r[:, 0] + r[:, 2] <= TW) & (r[:, 1] + r[:, 3] <= TH)).all()           # inside the image
    d = c.depth_bits.view(np.float32)
    assert (np.isfinite(d) & (d > 0)).all()
    assert c.note, "a case must say which edge it stands on"
    prop = B.properties(c)
    for key, want in c.note.items():
        assert prop[key] == want, (name, key)
    # the reference is consistent with itself
    assert ref.n == len(ref.sorted_gid) == ref.tile_start[-1] == sum(prop["totals"])
    assert ref.longest == max(prop["lists"].values(), default=0)
    assert ref.need == ref.n + 8 * max(prop["totals"], default=0)


def test_the_named_edges_are_the_ones_the_kernels_branch_on():
    """Literal figures, so that an edit of the builders cannot move them together with the notes."""
    p = {k: B.properties(B.get(k)[0]) for k in ("mixed_classes", "wg4_stride", "huge_stride", "box-32x32", "box-25x41",
                                                 "runs-256", "full_image")}
    assert sorted(p["mixed_classes"]["lists"].values()) == [1, 64, 65, 512, 513, 1024, 1025, 2049, 4097]
    assert len(B.get("mixed_classes")[0].rects) // 256 >= 30
    wl = p["wg4_stride"]["lists"]
    assert (wl[5], wl[2053], wl[6], wl[2054], wl[7]) == (1025, 1025, 600, 2049, 3) and 1024 < wl[2055] <= 4096
    assert B.tiles_of(B.get("wg4_stride")[0]) == (47, 47)
    assert p["huge_stride"]["lists"] == {3: 4097, 259: 16385, 4: 16385, 260: 4097}
    assert B.tiles_of(B.get("huge_stride")[0]) == (17, 17)
    assert p["box-32x32"]["areas"] == [1024] and p["box-25x41"]["areas"] == [1025]
    assert p["runs-256"]["hits"] == [255, 256, 258]
    assert B.tiles_of(B.get("full_image")[0]) == (255, 255) and p["full_image"]["n"] == 65025 + 129


def test_interleaved_rows_feed_several_tiles_from_every_group():
    for name in ("mixed_classes", "wg4_stride", "huge_stride"):
        c, _ = B.get(name)
        tile = c.rects[:, 1] * B.tiles_of(c)[0] + c.rects[:, 0]
        full = len(tile) // 256 * 256
        per_group = [len(set(g.tolist())) for g in tile[:full].reshape(-1, 256)]
        assert min(per_group) >= 2, name


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_the_oracle(name):
    c, ref = B.get(name)
    gid, ts = oracle_lists(c.rects, c.depth_bits, c.W, c.H)
    assert np.array_equal(ts, ref.tile_start)
    assert np.array_equal(gid, ref.sorted_gid)


@pytest.mark.parametrize("N,W,H,seed", [(3000, 160, 96, 5), (800, 50, 35, 6), (2000, 320, 200, 7)])
def test_reference_equals_the_oracle_on_projected_scenes(N, W, H, seed):
    P, cam = scene(N, W, H, 0, seed)
    pr = O.project(P["means"], P["log_scales"], P["quats"], P["opac_logit"], P["sh"], cam, 0)
    rect = pr["rect"].numpy()
    rects = np.stack([rect[:, 0], rect[:, 1], rect[:, 2] - rect[:, 0], rect[:, 3] - rect[:, 1]], 1)
    rects[~pr["valid"].numpy()] = 0
    bits = pr["depth"].detach().to(torch.float32).numpy().view(np.uint32)
    TW, TH = cam.tiles
    ref = B.reference(rects, bits, TW, TH)
    gid, ts = O.bin_and_sort(pr["rect"], pr["valid"], pr["depth"], cam)
    assert ref.n > N                                   # a frame with work in it
    assert np.array_equal(ts, ref.tile_start) and np.array_equal(gid, ref.sorted_gid)


def test_offsets_and_totals_of_the_reference_by_hand():
    rects = np.array([[0, 0, 2, 3], [1, 1, 0, 5], [2, 0, 1, 1]] + [[0, 0, 1, 1]] * 254 + [[1, 2, 2, 1]])
    ref = B.reference(rects, B.depths("all_equal", len(rects)), 3, 3)
    assert ref.offset[:4].tolist() == [0, 6, 6, 7] and ref.offset[255] == 6 + 1 + 252 and ref.offset[256:].tolist() == [0, 1]
    assert ref.totals.tolist() == [260, 3] and ref.n == 263 and ref.need == 263 + 8 * 260
    assert ref.tile_start[:3].tolist() == [0, 255, 256] and ref.sorted_gid[:3].tolist() == [0, 3, 4]
    assert ref.longest == 255


def test_depth_patterns():
    for p in B.PATTERNS:
        for n in (0, 1, 513, 32769):
            b = B.depths(p, n, 3)
            f = b.view(np.float32)
            assert b.dtype == np.uint32 and len(b) == n and (np.isfinite(f) & (f > 0)).all()
    assert len(set(B.depths("distinct", 32769, 1).tolist())) == 32769
    assert len(set(B.depths("all_equal", 100).tolist())) == 1
    assert len(set(B.depths("two_values", 100).tolist())) == 2
    u = B.depths("ulp_neighbours", 100).astype(np.int64)
    assert (np.diff(u) == -1).all()
    assert (np.diff(B.depths("ascending", 100).astype(np.int64)) > 0).all()
    assert (np.diff(B.depths("descending", 100).astype(np.int64)) < 0).all()


@pytest.mark.parametrize("name", ["runs-256", "long_and_invisible", "groups-513", "full_image", "box-1x255"])
def test_packed_rect_round_trips_through_splat_fields(name):
    c, _ = B.get(name)
    rec = B.records(c.rects, c.depth_bits)
    assert rec.dtype == torch.float32 and rec.shape == (len(c.rects), 12)
    f = splat_fields(rec)
    r = torch.from_numpy(c.rects.copy())
    assert torch.equal(f["rect"], torch.stack([r[:, 0], r[:, 1], r[:, 0] + r[:, 2], r[:, 1] + r[:, 3]], 1))
    assert torch.equal(f["hits"], r[:, 2] * r[:, 3]) and bool(f["visible"].all())
    assert np.array_equal(rec[:, 2].numpy().view(np.uint32), c.depth_bits)
    other = [s for s in range(12) if s not in (2, 4, 10)]
    assert bool((rec[:, other] == B.FILLER).all()) and bool(torch.isfinite(rec[:, other]).all())
