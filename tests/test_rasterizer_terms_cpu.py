"""CPU companion of tests/test_rasterizer_terms_gpu.py: pins, without a GPU, what that file's comparisons rest on, so that a later
change of a scene, of the oracle or of a bound cannot quietly take coverage away from it.  Both builds of the C oracle
(oracle/surfel_oracle.c: fp32 and fp64) on the seven scenes of raster_term_cases, under every one-hot cotangent.

Asserted here (run with -s for the tables; profiles/rasterizer_term_margins.md keeps one printout):
  * every scene really holds the class of surfel it is named after, read from the oracle's fields, and >= 290 visible surfels;
  * the two oracle builds agree on radii, clamped flags and -- on all but <= 2 pixels, measured 0 -- the last and median contributors;
  * e32 = ||oracle_f32 - oracle_f64|| / ||oracle_f64|| per (scene, channel, tensor): the pairs above 1e-3 ("not well conditioned":
    compared absolutely on the GPU) are exactly ILL_CONDITIONED, the terms that do not exist are exactly structural_zeros();
    measured: <= 5e-5 on ten channels, 7e-5 .. 9.6e-4 on the well-conditioned distortion pairs, 1.1e-3 .. 1.3e-3 on the four others;
  * the same holds on the rows of each class of surfel the GPU file compares alone;
  * the two copies of darksh for option 8 cull exactly the 12 surfels moved behind the camera, across every workgroup seam;
  * every GPU bound lies in [1e-4, 1e-2) and a 1 % error in any single well-conditioned term exceeds it.
"""
import numpy as np
import pytest

import raster_term_cases as rtc
from raster_term_cases import CHANNELS, COLOUR_CHANNELS, GPU_BOUND, LOWPASS_RADIUS, WELL_CONDITIONED, term_error

# (scene, channel, tensor) with e32 > 1e-3: the distortion term where almost nothing overlaps (sub-pixel surfels) is a rounding-level
# remainder in fp32.  (`faint` sits just inside: 6.6e-4 .. 9.6e-4.)
ILL_CONDITIONED = {("subpixel", "distortion", k) for k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dscales", "dL_dopacity")}


def structural_zeros(name):
    """The (channel, tensor) pairs of a scene whose fp64 gradient is zero (<= 1e-12 of the all-channel gradient)."""
    colour = "dL_dcolors" if name == "precomp" else "dL_dsh"
    z = {(ch, colour) for ch in CHANNELS if ch not in COLOUR_CHANNELS}          # geometry channels never reach the colours
    z |= {("median_depth", "dL_dopacity"), ("median_depth", "dL_dscales")}      # the picked entry's depth: no alpha, no extent in it
    if name == "subpixel":   # the low-pass disc's depth is the centre's: a function of means3D alone
        z |= {("median_depth", "dL_dmeans2D"), ("median_depth", "dL_drotations")}
    return z


@pytest.mark.parametrize("name", rtc.SCENES)
def test_scene_holds_its_class_and_the_oracle_builds_agree(name):
    t = rtc.oracle_terms(name)
    vis = t.visible()
    final_T, alpha = t.orc64.field("final_T")[0], t.orc64.allmap[1]
    print("\n%s: %d visible, max radius %d, min final_T %.3e, max alpha %.6f, %d clamped entries, %d surfels no pixel blends, %d flipped pixels"
          % (name, vis.sum(), t.orc64.radii[vis].max(), final_T.min(), alpha.max(), t.clamped().sum(), t.never_blended().sum(), t.oracle_flips.sum()))
    assert vis.sum() >= 290
    assert np.array_equal(t.orc32.radii, t.orc64.radii)
    assert np.array_equal(t.orc32.field("clamped"), t.orc64.field("clamped"))
    assert t.oracle_flips.sum() <= 2        # measured 0: if an input breaks this, change the input, not the cap
    assert (t.case["image_height"] % 16, t.case["image_width"] % 16) == (8, 4)   # ragged tiles in y and in x
    if name == "subpixel":
        assert t.orc64.radii[vis].max() <= LOWPASS_RADIUS
    if name == "opaque":
        assert final_T.min() <= 1.1e-4 and alpha.max() > 0.99
        assert t.never_blended().sum() >= 100 and (~t.never_blended()).sum() >= 100
    if name == "faint":
        assert final_T.min() > 0.5
    if name == "darksh":
        assert t.clamped().sum() >= 100
        assert (~t.clamped()).all(axis=1).sum() >= 50 and t.never_blended().sum() >= 10
    if name == "whitebg":
        assert (t.case["bg"] == 1).all()
    if name == "precomp":
        assert t.cp is not None and "dL_dcolors" in t.tensors


@pytest.mark.parametrize("name", rtc.SCENES)
def test_conditioning_and_structural_zeros_of_every_term(name):
    t = rtc.oracle_terms(name)
    ill, zeros = set(), set()
    print("\n%s: e32 per (channel, tensor); Z = structural zero\n%14s %s" % (name, "", " ".join("%13s" % k for k in t.tensors)))
    for ch in CHANNELS:
        row = []
        for k in t.tensors:
            if t.zero(ch, k):
                zeros.add((ch, k))
                row.append("%13s" % "Z")
                continue
            e = t.e32(ch, k)
            row.append("%13.2e" % e)
            if e > WELL_CONDITIONED:
                ill.add((name, ch, k))
            else:
                # the formal form of "no asserted bound may be 1e-2 or more": a 1 % error in this term alone fails the GPU test
                ref = t.g64[ch][k]
                assert term_error(1.01 * ref, ref, t.full64[k]) > GPU_BOUND[ch], (ch, k)
                assert e <= 5e-5 or ch == "distortion", (ch, k, e)     # only the distortion term is near the threshold at all
        print("%14s %s" % (ch, " ".join(row)))
    print("not well conditioned:", sorted(ill), "\nstructural zeros:", sorted(zeros))
    assert ill == {p for p in ILL_CONDITIONED if p[0] == name}
    assert zeros == structural_zeros(name)
    dead = t.never_blended()     # zero under the full cotangent: zero under every channel, in both builds
    for ch, k in t.pairs():
        assert not t.g32[ch][k][dead].any() and not t.g64[ch][k][dead].any(), (ch, k)
    # the one-hot cotangents are the planes of the full one: their gradients add up to the all-channel gradient
    for k in t.tensors:
        total = sum(np.asarray(t.g64[ch][k], np.float64) for ch in CHANNELS)
        assert np.linalg.norm(total - t.full64[k]) <= 1e-12 * np.linalg.norm(t.full64[k]), k


def test_bounds_are_between_the_floor_and_one_percent():
    assert set(GPU_BOUND) == set(CHANNELS)
    for ch, b in GPU_BOUND.items():
        assert 1e-4 <= b < 1e-2, ch
    assert rtc.ABS_BOUND == 1e-4 and rtc.WELL_CONDITIONED == 1e-3 and rtc.ZERO_FACTOR == 8.0


def test_clamped_rows_and_surfels_never_blended_are_exact_zeros():
    """The per-class rows of the GPU file: zero in BOTH oracle builds (so HIP must return exact zeros there), and the classes that
    carry a comparison are as well conditioned on their own rows as the whole tensor."""
    t = rtc.oracle_terms("darksh")
    cl = t.clamped()
    for c, ch in enumerate(COLOUR_CHANNELS):
        for g in (t.g32[ch]["dL_dsh"], t.g64[ch]["dL_dsh"]):
            assert not g[:, :, c][cl[:, c]].any()
            assert all(not g[:, :, o].any() for o in range(3) if o != c)
            assert g[:, :, c][~cl[:, c]].any()
    for name in ("darksh", "opaque"):
        t = rtc.oracle_terms(name)
        dead, cl = t.never_blended(), t.clamped()
        classes = {"reached": ~dead}
        if name == "darksh":
            classes.update(some_clamped=cl.any(axis=1) & ~dead, none_clamped=~cl.any(axis=1) & ~dead)
        for ch, k in t.pairs():
            assert not t.g32[ch][k][dead].any() and not t.g64[ch][k][dead].any(), (name, ch, k)
            if not t.well_conditioned(ch, k):
                continue
            for cname, rows in classes.items():
                e = term_error(t.g32[ch][k][rows], t.g64[ch][k][rows], t.full64[k][rows])
                assert e <= WELL_CONDITIONED, (name, cname, ch, k, e)
        print("\n%s: %s" % (name, ", ".join("%d %s" % (rows.sum(), cname) for cname, rows in classes.items())), "and %d that no pixel blends" % dead.sum())


@pytest.mark.parametrize("name", rtc.OPTION8_SCENES)
def test_option8_scenes_have_culled_clamped_and_unreached_rows(name):
    """The two copies of darksh that the all-rows store of dL_dsh is tested on: exactly the 12 moved surfels are culled (radius 0 in both
    oracle builds), on both sides of every 64-surfel seam and in the ragged last workgroup; clamped entries and surfels no pixel blends
    are there as in darksh; the rows are 48 and 27 floats with coefficients above the degree; every colour term is well conditioned."""
    t = rtc.oracle_terms(name)
    culled = np.zeros(t.orc64.P, bool)
    culled[list(rtc.CULLED_ROWS)] = True
    assert np.array_equal(t.orc64.radii == 0, culled) and np.array_equal(t.orc32.radii, t.orc64.radii)
    assert {i // 64 for i in rtc.CULLED_ROWS} == {0, 1, 2, 3, 4} and {63, 64, 127, 128, 191, 192, 255, 256, 299} <= set(rtc.CULLED_ROWS)
    assert np.array_equal(t.orc32.field("clamped"), t.orc64.field("clamped")) and t.oracle_flips.sum() <= 2
    assert t.clamped().sum() >= 100 and t.never_blended().sum() >= 10
    row = 3 * t.case["shs"].shape[1]
    assert row == (48 if name == "darksh_culled" else 27) and (row % 4 == 0) == (name == "darksh_culled")
    assert t.case["shs"].shape[1] > (t.case["sh_degree"] + 1) ** 2
    print("\n%s: %d culled, %d clamped entries, %d surfels no pixel blends, rows of %d floats" % (name, culled.sum(), t.clamped().sum(), t.never_blended().sum(), row))
    for ch in COLOUR_CHANNELS:
        for k in t.tensors:
            assert t.well_conditioned(ch, k), (ch, k, t.e32(ch, k))
            assert not t.g32[ch][k][culled].any() and not t.g64[ch][k][culled].any()
        assert not t.g32[ch]["dL_dsh"][:, 4:].any() and not t.g64[ch]["dL_dsh"][:, 4:].any()


def test_share_of_each_channel_in_the_aggregate_cotangent():
    """What the per-channel tests are for: under the aggregate test's cotangent (N(0,1) in all channels, test_gpu_parity.CASES[0] and
    [1]) a channel owns this share of a gradient tensor's norm -- an error of that relative size in the channel's whole backward
    moves the aggregate rel-L2 by as much.  The distortion channel cannot be seen by a 1e-4 bound; the others can."""
    from scene_utils import small_case
    from test_gpu_parity import CASES
    shares = [rtc.channel_shares(small_case(**cfg)) for cfg in CASES[:2]]
    print("\nshare of the full gradient's norm, smallest .. largest over the tensors\n%14s %22s %22s" % ("channel", "CASES[0]", "CASES[1] (white bg)"))
    for ch in CHANNELS:
        print("%14s %22s %22s" % ((ch,) + tuple("%.1e .. %.1e" % s[ch] for s in shares)))
    for s in shares:
        assert s["distortion"][1] <= 5e-3      # measured 3.0e-4 / 1.7e-3: a 5 % error in it moves the aggregate rel-L2 by < 1e-4
