"""Preconditions of tests/test_tile_lists_gpu.py, checked without a GPU: the scenes of tests/tile_list_cases.py really hold the lists,
depth classes and rectangles they were designed to hold, the CPU oracle builds exactly the NumPy lists, and its fp32 and fp64 builds
blend the same entries for every pixel -- so an image comparison on these scenes has no contributor flips to allow for."""
import numpy as np
import pytest

import tile_list_cases as tlc


@pytest.fixture(scope="module", autouse=True)
def _release_oracle_runs():
    yield
    tlc.release()


def _lens(ranges):
    return ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)


@pytest.mark.parametrize("cls", sorted(tlc.CLASSES))
def test_depth_classes_have_their_bits_and_ties(cls):
    """nbits as the radix kernel computes it (xor of the list's AND and OR) decides the number of 8-bit passes: 0, 1, 2, 3, 4."""
    fn = tlc.CLASSES[cls]
    for n in (1, 2, 3, 5, 64, 257, 300, 1500, 2048, 4097):
        d = fn(n)
        assert d.dtype == np.uint32 and d.shape == (n,)
        assert np.all(d.view(np.float32) > tlc.NEAR) and np.all(d < 0x7f800000)
        nb, distinct, run = tlc.nbits_of(d), len(np.unique(d)), tlc.longest_tie_run(d)
        print("class %-2s n %5d: nbits %2d (passes %d), %5d distinct depths, longest tie run %d" % (cls, n, nb, (nb + 7) // 8, distinct, run))
        assert nb == (tlc.CLASS_NBITS[cls] if n >= 2 else 0)
        assert distinct <= tlc.CLASS_MAX_DISTINCT[cls](n)
        assert run <= tlc.MAX_TIE_RUN or cls == "E"   # (E is one run by definition: the scenes use it up to 1500 entries, checked per scene)
        if cls == "E":
            assert distinct == 1 and run == n
        elif n >= 2:
            assert distinct >= 2
        if cls in ("B3", "B4"):
            assert distinct >= n - 8          # 2^23 and more values to draw from: ties are accidents
        if cls == "T" and n >= 64:
            assert distinct >= n // 16 and run >= 2   # many short runs
        if cls == "H" and n >= 2:
            assert np.all((d & 0xffff) == 0)      # the two low digits have one occupied bin
        if cls == "B2":
            assert np.all(d & 0xff00)
    assert tlc.longest_tie_run(tlc.depths_T(4097, run=600)) >= 600


def test_pass_counts_cover_zero_to_four():
    assert sorted({(tlc.CLASS_NBITS[c] + 7) // 8 for c in tlc.CLASSES}) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("name", tlc.SCENES)
def test_oracle_builds_the_designed_lists(name):
    s = tlc.scene(name)
    o32 = tlc.oracle(name)
    single = s.tile_of >= 0
    # the depth the rasterizer computes is the designed float, bit for bit
    assert np.array_equal(o32.field("depths").view(np.uint32)[single], s.depth_bits[single])
    assert np.all(o32.radii[single] > 0)
    vis = o32.radii > 0
    assert np.array_equal(o32.field("depths").view(np.uint32)[vis], s.depth_bits[vis])
    pl, ranges, area = tlc.reference_lists(s, o32.field("means2D"), o32.radii)
    # every single-tile surfel touches exactly its own tile under the reference rectangles
    assert np.all(area[single] == 1)
    x0, y0, _, _ = tlc.tile_rects(o32.field("means2D")[:, 0], o32.field("means2D")[:, 1], o32.radii, s.tiles_x, s.tiles_y)
    assert np.array_equal((y0 * s.tiles_x + x0)[single], s.tile_of[single])
    lens = _lens(ranges)
    if single.all():
        assert np.array_equal(lens, s.list_lengths())
        assert o32.num_rendered == s.P == int(s.list_lengths().sum())
        d_pl, d_ranges = s.designed_lists()
        assert np.array_equal(pl, d_pl) and np.array_equal(ranges, d_ranges)
    else:
        assert np.all(lens >= s.list_lengths())
        assert o32.num_rendered == int(s.list_lengths().sum()) + int(area[~single].sum())
    assert o32.num_rendered == len(pl)
    full = lens > 0     # (identifyTileRanges leaves the range of an empty tile untouched: (0, 0) in the oracle, (start, start) here)
    assert np.array_equal(o32.field("ranges")[full], ranges[full]) and np.all(_lens(o32.field("ranges"))[~full] == 0)
    assert np.array_equal(o32.field("point_list"), pl)
    e_pl, e_ranges = tlc.expected(name)
    assert np.array_equal(e_pl, pl) and np.array_equal(e_ranges, ranges)
    r = o32.radii[single]
    print("scene %-11s %dx%d, %d tiles, P %d, R %d, radii of the single-tile surfels %d..%d, lists: %s" % (
        name, s.W, s.H, s.ntiles, s.P, o32.num_rendered, r.min() if len(r) else 0, r.max() if len(r) else 0,
        " ".join("%d:%s/%d" % (t, c, len(d)) for t, c, d in sorted(s.lists, key=lambda l: l[0]))))
    for _, _, d in s.lists:
        assert tlc.longest_tie_run(d) <= tlc.MAX_TIE_RUN


@pytest.mark.parametrize("name", ["edges", "long", "many_tiles", "rectangles"])   # (edges_short and long_fit are these minus one or four lists)
def test_fp32_and_fp64_oracle_blend_the_same_entries(name):
    """Identical n_contrib (last and median contributor of every pixel) in both builds: no entry sits on the 1/255 alpha or the 1e-4
    transmittance threshold, so the image comparison of the GPU test allows no flipped pixel.  Prints the fp32 oracle's own distance
    from the fp64 one, which is what a bound on the HIP deviation is judged against."""
    o32, o64 = tlc.oracle(name), tlc.oracle_f64(name)
    assert o32.num_rendered == o64.num_rendered
    assert np.array_equal(o32.field("point_list"), o64.field("point_list"))
    n32, n64 = o32.field("n_contrib"), o64.field("n_contrib")
    assert np.array_equal(n32, n64), "%d pixels blend different entries" % int((n32 != n64).any(axis=0).sum())
    dc = np.abs(o32.color.astype(np.float64) - o64.color)
    da = np.abs(o32.allmap.astype(np.float64) - o64.allmap) / np.maximum(1.0, np.abs(o64.allmap))
    print("scene %-10s fp32 vs fp64 oracle: colour max |d| %.3e, allmap max |d| / max(1, |x|) %.3e per channel %s, longest walk %d entries" % (
        name, dc.max(), da.max(), " ".join("%.1e" % v for v in da.reshape(8, -1).max(axis=1)), int(n64[0].max())))
    assert (n64[0] > 0).any()


def test_edges_puts_two_long_lists_in_one_workgroup_column():
    """The grid-stride sort kernels run min(ntiles, 256) columns: tiles 4 and 260 share column 4, both lists are longer than one
    segment, and their segment counts differ (rows 0-1 of the column take a second trip, row 2 only the second list)."""
    s = tlc.scene("edges")
    assert s.ntiles == 289 > 256
    lens = s.list_lengths()
    assert lens[4] > 2048 and lens[260] > 2048 and 260 % 256 == 4
    assert -(-int(lens[4]) // 2048) != -(-int(lens[260]) // 2048)
    assert lens.max() == 6000 and tlc.scene("edges_short").list_lengths().max() == 2048
    occupied = np.nonzero(lens)[0]
    assert np.all(occupied % 2 == 0)     # a checkerboard on the 17-wide grid: every list has empty neighbours
    assert lens[0] > 0 and lens[288] > 0
    for n in tlc.EDGE_LENGTHS:
        assert (lens == n).sum() >= 4
    ls = tlc.scene("long").list_lengths()
    assert sorted(ls[ls > 0]) == [4097, 16384, 16385, 57344, 57345]
    assert ls[10] > 16384 and ls[266] > 57344 and ls[30] == 16384 and ls[286] == 57344   # columns 10 and 30 hold two lists each
    assert tlc.scene("long_fit").list_lengths().max() == 57344 == 2048 * 28


def test_many_tiles_is_past_the_lds_histogram():
    s = tlc.scene("many_tiles")
    assert s.ntiles == 193 * 193 > 36864          # 144 KB of counters
    lens = s.list_lengths()
    assert lens[0] == 1 and lens[s.ntiles - 1] == 2049
    assert (lens > 0).sum() == 204
    o = tlc.oracle("many_tiles")
    area = tlc.reference_lists(s, o.field("means2D"), o.radii)[2][s.tile_of < 0]
    print("many_tiles discs cover", sorted(area.tolist()), "tiles")
    assert len(area) == 12 and area.min() == 4 and area.max() == 36
    assert len(set(area.tolist()) & {4, 9, 16, 25, 36}) == 5 and len(set(area.tolist()) - {4, 9, 16, 25, 36}) >= 3   # whole and clipped


def test_rectangles_reach_the_wave_walk_and_its_boundary():
    """count_tiles_lds_kernel / scatter_keys_lds_kernel: a rectangle of more than 64 tiles is walked by the whole wave.  The scene
    holds areas on both sides of the switch, clipped and screen-filling ones, and mixes them inside the lanes one wave holds."""
    s = tlc.scene("rectangles")
    o = tlc.oracle("rectangles")
    m2, rad = o.field("means2D"), o.radii
    assert (rad > 0).sum() >= 0.95 * s.P and (rad == 0).sum() >= 1     # (a few small discs lie wholly outside the image: culled, no entry)
    x0, y0, x1, y1 = tlc.tile_rects(m2[:, 0], m2[:, 1], rad, s.tiles_x, s.tiles_y)
    w, h = x1 - x0, y1 - y0
    area = np.where(rad > 0, w * h, 0)
    hist = np.bincount(area, minlength=290)
    print("rectangles: P %d, R %d, areas present: %s" % (s.P, area.sum(), " ".join("%d:%d" % (a, c) for a, c in enumerate(hist) if c)))
    assert hist[64] >= 5 and hist[1] >= 1
    assert hist[65:82].sum() >= 5 and hist[81] >= 3 and hist[72] >= 1
    assert hist[289] >= 3
    inner = lambda a0, a1, n: (a0 > 0) & (a1 < n)
    for clipped in ((x0 == 0) & (m2[:, 0] - rad < 0), (x1 == s.tiles_x) & (m2[:, 0] + rad > s.W),
                    (y0 == 0) & (m2[:, 1] - rad < 0), (y1 == s.tiles_y) & (m2[:, 1] + rad > s.H)):
        assert (clipped & (area > 64)).sum() >= 3 and (clipped & (area <= 64) & (area > 0)).sum() >= 3
    assert (inner(x0, x1, s.tiles_x) & inner(y0, y1, s.tiles_y)).sum() >= 100
    big = area > 64
    # the issue's figure: 64 consecutive indices; and the kernel's: workgroup g owns surfels [g chunk, (g + 1) chunk), chunk = ceil(P / 256),
    # whose first 64 are one wave
    chunk = -(-s.P // 256)
    mixed64 = [k for k in range(0, s.P - 63) if big[k:k + 64].sum() >= 2 and (~big[k:k + 64] & (area[k:k + 64] > 0)).sum() >= 2]
    mixed_wave = [g for g in range(256) if big[g * chunk:g * chunk + min(chunk, 64)].sum() >= 2
                  and (~big[g * chunk:g * chunk + min(chunk, 64)] & (area[g * chunk:g * chunk + min(chunk, 64)] > 0)).sum() >= 2]
    print("rectangles: %d windows of 64 indices and %d of the 256 workgroups' first waves (chunk %d) mix big and small rectangles" % (
        len(mixed64), len(mixed_wave), chunk))
    assert len(mixed64) >= 1 and len(mixed_wave) >= 100
    assert tlc.nbits_of(s.depth_bits) == 31
