"""-m gpu: the rasterizer's backward kernels (csrc/blend_bwd_kernels.h, the per-surfel backward of csrc/surfel_kernels.h), one
output channel and one class of surfel at a time, against the fp64 build of the C oracle.

tests/test_gpu_parity.py sends N(0,1) into all 11 output channels at once and takes one relative L2 per gradient tensor; the
distortion channel owns 1e-4 .. 2e-3 of that norm and the alpha channel 2e-3 on a white background, so their backward could be
10 % off (or absent) unseen.  Here every channel is the only cotangent of its comparison (raster_term_cases.one_hot_cotangents), on
seven 300-surfel 40 x 52 scenes (ragged tiles in x and y) that each put one class of surfel in front: low-pass disc, clamped SH,
0.99 alpha clamp and T < 1e-4 stop, faint, white background, precomputed colours.

Tolerances (tests/test_rasterizer_terms_cpu.py pins their preconditions without a GPU; profiles/rasterizer_term_margins.md has
every observed value of the MI355X session they were measured in):
  * pairs (scene, channel, tensor) on which the oracle's own fp32 and fp64 builds agree to 1e-3 ("well conditioned"):
    ||hip - ref64|| / ||ref64|| <= raster_term_cases.GPU_BOUND[channel] = 3x the largest value seen over scenes and tensors, never
    below SURVEY 8c's 1e-4 and never 1e-2 or above: a 1 % error in any single term fails,
  * the other pairs (the distortion channel where nothing overlaps): ||hip - ref64|| <= 1e-4 ||ref64 under all channels||, the
    aggregate test's bound,
  * terms that do not exist (dL_dsh under a geometry channel, clamped SH rows, surfels behind the stop, ...): exactly 0 where the
    fp32 oracle gives exactly 0, else max|hip| <= 8 max|oracle_f32| (fp32 sums in another order),
  * option 7 = 2 (fixed-point sums): the same bounds plus, per element, n_partial * 2^-44 -- the kernel's documented quantum times
    the number of per-(wave, entry) partial sums of that surfel (at most 4 waves x tiles touched), derived, not measured.
Option 8 (every row of dL_dsh stored) is driven the way the trainer drives it, through a dL/dSH sink registered with all_rows=True and
pre-filled with NaN, on two copies of darksh with 12 culled surfels (rows of 48 and of 27 floats).
Pixels on which HIP takes another last or median contributor than the fp64 oracle (a discrete decision; the median ones are
proven ties, gpu_utils.median_flips; at most 2 per scene) carry no cotangent on any side.
"""
import numpy as np
import pytest

import raster_term_cases as rtc
from raster_term_cases import ABS_BOUND, CHANNELS, COLOUR_CHANNELS, GPU_BOUND, ZERO_FACTOR, abs_error, term_error

pytestmark = pytest.mark.gpu

QUANTUM = 2.0 ** -44    # blend_bwd_kernels.h to_fixed44
_REF, _HIP = {}, {}


def _ref(name):
    """OracleTerms of the scene with HIP's own contributor flips masked as well; computed once per session."""
    if name not in _REF:
        from diff_surfel_rasterization import _C
        from gpu_utils import median_flips, run_hip_raw
        base = rtc.oracle_terms(name)
        _C.set_tight_rects(False)      # the reference's tile rectangles: list positions in the oracle's numbering
        try:
            nc = run_hip_raw(base.case)["n_contrib"]
        finally:
            _C.set_tight_rects(True)
        # (median picks: proven ties; another LAST contributor -- the T < 1e-4 stop one entry earlier or later -- is taken as it is,
        # unproven, under the same cap of 2 pixels; no scene has shown either, so the re-masked reference below has never been built)
        flips = median_flips(nc[1], base.orc64) | (nc[0] != base.orc64.field("n_contrib")[0])
        print("%s: %d pixels with another last / median contributor than the fp64 oracle" % (name, int(flips.sum())))
        assert int((flips | base.oracle_flips).sum()) <= 2, name
        _REF[name] = (rtc.OracleTerms(name, extra_mask=flips) if flips.any() else base), flips
    return _REF[name]


def _hip_terms(name):
    """{channel: run_hip output} of the default backward under each one-hot cotangent; computed once per session."""
    if name not in _HIP:
        from gpu_utils import run_hip
        ref, _ = _ref(name)
        _HIP[name] = {ch: run_hip(ref.case, gc, go, colors_precomp=ref.cp) for ch, gc, go in ref.cotangents()}
    return _HIP[name]


def _rows(a, rows):
    return a if rows is None else a[rows]


def _compare(ref, ch, k, got, g32, g64, bad, label, rows=None, extra=0.0, scale=1.0):
    """One (channel, tensor) comparison by the rule of its kind; records what it saw and appends a line to `bad` if it fails.
    `extra`: an absolute allowance added to the two norm bounds (the fixed-point quantum; never to a term that does not exist: an
    all-zero fixed-point sum is exactly zero); `scale`: the factor on the cotangent (the kind
    of a pair is scale-free, the all-channel gradient it is measured against scales along)."""
    from gpu_utils import _record
    got, g32, g64, full = _rows(got, rows), _rows(g32, rows), _rows(g64, rows), _rows(ref.full64[k], rows) * scale
    name = "%s/%s/%s/%s" % (label, ref.name, ch, k)
    if ref.zero(ch, k) or not np.asarray(g64).any():
        seen, allowed = float(np.abs(got).max(initial=0.0)), ZERO_FACTOR * float(np.abs(g32).max(initial=0.0))
        _record("term_zero", name, {"max_abs_hip": seen, "max_abs_oracle_f32": float(np.abs(g32).max(initial=0.0))}, {"max_abs": allowed})
        if not seen <= allowed:
            bad.append("%s: structural zero, max|hip| %.3e > %.3e" % (name, seen, allowed))
    elif ref.well_conditioned(ch, k):
        e, e32 = term_error(got, g64, full), term_error(g32, g64, full)
        diff, allowed = rtc.norm(np.asarray(got, np.float64) - g64), GPU_BOUND[ch] * rtc.norm(g64) + extra
        _record("term_rel", name, {"term_error": e, "oracle_f32": e32}, {"bound": GPU_BOUND[ch], "extra_abs": extra})
        if not diff <= allowed:
            bad.append("%s: term error %.3e > %.1e (fp32 oracle: %.3e)" % (name, e, GPU_BOUND[ch], e32))
    else:
        e = abs_error(got, g64, full)
        _record("term_abs", name, {"abs_error": e, "oracle_f32": abs_error(g32, g64, full)}, {"bound": ABS_BOUND, "extra_abs": extra})
        if not e * rtc.norm(full) <= ABS_BOUND * rtc.norm(full) + extra:
            bad.append("%s: ||hip - ref64|| / ||full64|| %.3e > %.1e" % (name, e, ABS_BOUND))


@pytest.mark.parametrize("name", rtc.SCENES)
def test_each_cotangent_channel_alone_matches_the_fp64_oracle(name):
    """(a) 11 channels x 6 gradient tensors against the fp64 oracle, each by the rule of its kind (module docstring); the rows of
    surfels that no pixel blends are exactly zero; the images once, as the guard of the scene itself."""
    from gpu_utils import img_close
    ref, flips = _ref(name)
    hip = _hip_terms(name)
    fwd = hip[CHANNELS[0]]
    assert np.array_equal(fwd["radii"], ref.orc32.radii)
    img_close(fwd["color"], ref.orc32.color, "color")
    am, om = fwd["allmap"].copy(), ref.orc32.allmap.copy()
    for c in (5, 7):
        am[c][flips] = om[c][flips]
    img_close(am, om, "allmap")
    bad, dead = [], ref.never_blended()
    for ch, k in ref.pairs():
        assert hip[ch][k].shape == ref.g64[ch][k].shape, (ch, k)
        assert not hip[ch][k][dead].any(), "%s under %s: a surfel that no pixel blends has a gradient" % (k, ch)
        _compare(ref, ch, k, hip[ch][k], ref.g32[ch][k], ref.g64[ch][k], bad, "a")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["darksh", "opaque"])
def test_each_class_of_surfel_alone_matches_the_fp64_oracle(name):
    """(b) The comparison of (a) on the rows of one class, same bounds: the surfels with large gradients own the norm over all rows.
    darksh: surfels with and without a clamped colour, and per colour c the entries dL_dsh[:, :, c] of the rows clamped in c
    (exactly zero) and of the others.  opaque (and darksh): the surfels no pixel reaches before its T < 1e-4 stop are exactly
    zero in every tensor under every channel, the others carry the comparison.  No launch of its own: it re-reads the gradients
    the scene's run of _hip_terms produced (shared with (a): if that run fails, both tests fail)."""
    from gpu_utils import _record
    ref, _ = _ref(name)
    hip = _hip_terms(name)
    dead, clamped = ref.never_blended(), ref.clamped()
    assert dead.sum() >= 10 and (~dead).sum() >= 100
    classes = {"reached": ~dead}
    if name == "darksh":
        assert clamped.sum() >= 100
        classes.update(some_clamped=clamped.any(axis=1) & ~dead, none_clamped=~clamped.any(axis=1) & ~dead)
    bad = []
    for ch, k in ref.pairs():
        assert not hip[ch][k][dead].any(), "%s under %s: a surfel that no pixel blends has a gradient" % (k, ch)
        for cname, rows in classes.items():
            _compare(ref, ch, k, hip[ch][k], ref.g32[ch][k], ref.g64[ch][k], bad, "b:" + cname, rows=rows)
    if name == "darksh":
        for c, ch in enumerate(COLOUR_CHANNELS):
            got, g32, g64 = (g[ch]["dL_dsh"][:, :, c] for g in (hip, ref.g32, ref.g64))
            assert not got[clamped[:, c]].any(), "dL_dsh[:, :, %d] of a clamped row is not zero" % c
            for other in range(3):
                if other != c:
                    assert not hip[ch]["dL_dsh"][:, :, other].any(), "colour %d leaks into dL_dsh[:, :, %d]" % (c, other)
            live = ~clamped[:, c] & ~dead
            assert live.sum() >= 50
            e = term_error(got[live], g64[live], ref.full64["dL_dsh"][:, :, c][live])
            _record("term_rel", "b:unclamped/darksh/%s/dL_dsh[:, :, %d]" % (ch, c),
                    {"term_error": e, "oracle_f32": term_error(g32[live], g64[live], ref.full64["dL_dsh"][:, :, c][live])}, {"bound": GPU_BOUND[ch], "extra_abs": 0.0})
            if not e <= GPU_BOUND[ch]:
                bad.append("dL_dsh[unclamped, :, %d]: %.3e > %.1e" % (c, e, GPU_BOUND[ch]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["plain", "opaque"])
def test_three_ways_of_summing_per_channel_and_at_the_scale_of_a_mean_loss(name):
    """(c) dgs_set_option(7, 0 / 1 / 2) under the colour-0 and the distortion cotangent alone, at N(0,1) and scaled by 1 / (3 H W),
    what a mean-reduced loss sends: the relative bounds of (a) are scale-free and hold for all three; the fixed-point variant
    may add its quantum 2^-44 per partial sum (n_partial <= 4 waves x tiles touched, from the oracle's reference rectangles, of
    which the kernel's lists are sub-lists) -- a small term falling under the quantum shows here and nowhere else.  Variants 1
    and 2 are bit-identical over three runs per channel."""
    from diff_surfel_rasterization import _C
    from gpu_utils import run_hip
    ref, _ = _ref(name)
    H, W = ref.case["image_height"], ref.case["image_width"]
    n_partial = 4.0 * ref.orc64.field("tiles_touched").astype(np.float64)
    cots = {ch: (gc, go) for ch, gc, go in ref.cotangents() if ch in ("color0", "distortion")}
    bad = []
    try:
        for scale in (1.0, 1.0 / (3 * H * W)):
            for ch, (gc, go) in cots.items():
                gc_s, go_s = (gc * np.float32(scale)).astype(np.float32), (go * np.float32(scale)).astype(np.float32)
                g32, g64 = ref.orc32.backward(gc_s, go_s), ref.orc64.backward(gc_s, go_s)
                for variant in (0, 1, 2):
                    _C.set_option(7, variant)
                    runs = [run_hip(ref.case, gc_s, go_s, colors_precomp=ref.cp, debug=False) for _ in range(3 if variant else 1)]
                    for k in ref.tensors:
                        for r in runs[1:]:
                            assert np.array_equal(runs[0][k], r[k]), "variant %d, %s under %s: runs differ" % (variant, k, ch)
                        got = runs[0][k]
                        # the quantum of each element of the surfel's row, as a norm over the tensor
                        extra = QUANTUM * float(np.linalg.norm(np.repeat(n_partial, got[0].size))) if variant == 2 else 0.0
                        _compare(ref, ch, k, got, g32[k], g64[k], bad, "c:v%d:x%.0e" % (variant, scale), extra=extra, scale=scale)
    finally:
        _C.set_option(7, 0)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", rtc.OPTION8_SCENES)
def test_all_rows_of_dL_dsh_stored_under_a_colour_channel(name):
    """(d) Option 8: dL_dsh stored for EVERY row.  The operator sets the option itself around each backward, from the dL/dSH sink of
    the call (set_sh_grad_sink(..., all_rows=True)); a set_option(8, 1) from outside is overwritten, so the test registers a sink,
    filled with NaN: whatever the backward does not store stays NaN.  darksh with 12 culled surfels (raster_term_cases), 16
    coefficients per channel (16-byte stores) and 9 (4-byte stores), under each one-hot colour cotangent: every element finite;
    culled rows, surfels no pixel blends, clamped entries, the other colours and the bands above the degree exactly zero; the rest
    and the five geometry tensors within the bounds of (a).  Control: the same sink WITHOUT all_rows keeps its NaN in the culled
    rows and only there and above the degree -- the zeros are option 8's."""
    import torch
    from diff_surfel_rasterization import _C, set_sh_grad_sink
    from gpu_utils import run_hip
    ref, _ = _ref(name)
    clamped, vis, dead = ref.clamped(), ref.visible(), ref.never_blended()
    culled = np.zeros(ref.orc64.P, bool)
    culled[list(rtc.CULLED_ROWS)] = True
    assert np.array_equal(culled, ~vis) and dead.sum() >= 10 and clamped.sum() >= 100
    bands = (ref.case["sh_degree"] + 1) ** 2
    assert bands < ref.case["shs"].shape[1]
    bad = []
    try:
        for c, (ch, gc, go) in enumerate(list(ref.cotangents())[:3]):
            for all_rows in ((True, False) if c == 0 else (True,)):
                sink = torch.full(tuple(ref.case["shs"].shape), float("nan"), dtype=torch.float32, device="cuda:0")
                set_sh_grad_sink(sink, all_rows=all_rows)
                hip = run_hip(ref.case, gc, go, allow_missing_sh_grad=True)
                assert hip["dL_dsh"] is None, "the backward did not use the sink"
                assert _C.get_option(8) == int(all_rows)
                sh = sink.cpu().numpy()
                if not all_rows:
                    assert np.isnan(sh[culled]).all() and np.isnan(sh[vis][:, bands:]).all() and np.isfinite(sh[vis][:, :bands]).all()
                    continue
                assert np.isfinite(sh).all(), "%d elements of the sink were not stored" % int((~np.isfinite(sh)).sum())
                assert not sh[culled].any() and not sh[dead].any() and not sh[:, bands:].any()
                assert not sh[:, :, c][clamped[:, c]].any()
                assert all(not sh[:, :, o].any() for o in range(3) if o != c)
                assert sh[:, :bands, c][~clamped[:, c] & ~dead].any()
                hip["dL_dsh"] = sh
                for k in ref.tensors:
                    assert not hip[k][culled].any(), k
                    _compare(ref, ch, k, hip[k], ref.g32[ch][k], ref.g64[ch][k], bad, "d")
    finally:
        set_sh_grad_sink(None, device="cuda:0")
        _C.set_option(8, 0)
    assert not bad, "\n".join(bad)
