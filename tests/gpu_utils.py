"""Helpers for the -m gpu parity tests: run the HIP operator through the drop-in Python surface
(which goes through the C ABI) and unpack its private scratch buffers for stage-level comparison."""
import numpy as np
import torch

from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _C


def settings_from_case(case, dev, debug=False):
    return GaussianRasterizationSettings(
        image_height=case["image_height"], image_width=case["image_width"], tanfovx=case["tanfovx"], tanfovy=case["tanfovy"],
        bg=case["bg"].to(dev), scale_modifier=1.0, viewmatrix=case["viewmatrix"].to(dev), projmatrix=case["projmatrix"].to(dev),
        sh_degree=case["sh_degree"], campos=case["campos"].to(dev), prefiltered=False, debug=debug)


def run_hip(case, gc=None, go=None, colors_precomp=None, dev="cuda:0", debug=True, allow_missing_sh_grad=False):
    """Forward (+ backward when cotangents are given). Returns dict of numpy arrays."""
    cfg = settings_from_case(case, dev, debug)
    rast = GaussianRasterizer(cfg)
    leaves = {k: case[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    kw = {}
    if colors_precomp is not None:
        cp = torch.as_tensor(colors_precomp, dtype=torch.float32, device=dev).clone().requires_grad_(True)
        kw["colors_precomp"] = cp
    else:
        kw["shs"] = leaves["shs"]
    color, radii, allmap = rast(means3D=leaves["means3D"], means2D=means2D, opacities=leaves["opacities"],
                                scales=leaves["scales"], rotations=leaves["rotations"], **kw)
    out = dict(color=color.detach().cpu().numpy(), allmap=allmap.detach().cpu().numpy(), radii=radii.cpu().numpy())
    fn = color.grad_fn
    if gc is not None:
        loss = (color * torch.as_tensor(gc, device=dev)).sum() + (allmap * torch.as_tensor(go, device=dev)).sum()
        loss.backward()
        out.update(
            dL_dmeans3D=leaves["means3D"].grad.cpu().numpy(), dL_dmeans2D=means2D.grad.cpu().numpy(),
            dL_dscales=leaves["scales"].grad.cpu().numpy(), dL_drotations=leaves["rotations"].grad.cpu().numpy(),
            dL_dopacity=leaves["opacities"].grad.cpu().numpy())
        if colors_precomp is not None:
            out["dL_dcolors"] = kw["colors_precomp"].grad.cpu().numpy()
        else:
            g_sh = leaves["shs"].grad
            assert g_sh is not None or allow_missing_sh_grad
            out["dL_dsh"] = None if g_sh is None else g_sh.cpu().numpy()
    torch.cuda.synchronize()
    return out


def run_hip_raw(case, dev="cuda:0", planes=True):
    """Calls the extension entry point directly and unpacks the private buffers (layout from
    dgs_debug_layout).  planes=False leaves out final_T and n_contrib (un-tiling them is seconds of NumPy on a 3088 x 3088 image)."""
    P, H, W = case["means3D"].shape[0], case["image_height"], case["image_width"]
    e = torch.empty(0, device=dev)
    t = lambda k: case[k].to(dev).contiguous()
    R, color, allmap, radii, geom, binning, img = _C.rasterize_gaussians(
        t("bg"), t("means3D"), e, t("opacities"), t("scales"), t("rotations"), 1.0, e, t("viewmatrix"), t("projmatrix"),
        case["tanfovx"], case["tanfovy"], H, W, t("shs"), case["sh_degree"], t("campos"), False, True)
    torch.cuda.synchronize()
    g_off = _C.debug_layout(0, P=P)
    i_off = _C.debug_layout(1, width=W, height=H)
    b_off = _C.debug_layout(2, width=W, height=H, R=R)
    gb, bb, ib = geom.cpu().numpy(), binning.cpu().numpy(), img.cpu().numpy()
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    T = tiles_x * tiles_y
    rec = gb[g_off[0]:g_off[0] + P * 96].view(np.float32).reshape(P, 24)
    plane = T * 256

    tid = np.arange(256)
    lane, wave = tid & 63, tid >> 6
    row, j = lane >> 4, lane & 15
    lx, ly = 8 * (wave & 1) + 4 * (row & 1) + (j & 3), 8 * (wave >> 1) + 4 * (row >> 1) + (j >> 2)   # surfel_math.h lane_pixel

    def untile(a):  # [T,256] tile-major (slot = thread id) -> [H,W]
        a = a.reshape(tiles_y, tiles_x, 256)
        img = np.zeros((tiles_y, tiles_x, 16, 16), a.dtype)
        img[:, :, ly, lx] = a
        return img.transpose(0, 2, 1, 3).reshape(tiles_y * 16, tiles_x * 16)[:H, :W]

    # slots of the forward's dispatch order: tile_order_kernels.h order_slots (tile order 4 leaves empty slots), never fewer than T
    order_len = max(T, 8 * 16 * ((((tiles_x + 3) // 4) * ((tiles_y + 3) // 4) + 7) // 8 + 1))
    out = dict(
        R=R, color=color.cpu().numpy(), allmap=allmap.cpu().numpy(), radii=radii.cpu().numpy(), rec=rec,
        order_fwd=ib[i_off[4]:i_off[4] + order_len * 4].view(np.uint32), order_slots=order_len,
        ranges=ib[i_off[2]:i_off[2] + T * 8].view(np.uint32).reshape(T, 2),
        tile_last=ib[i_off[3]:i_off[3] + T * 4].view(np.uint32),
        point_list=bb[b_off[0]:b_off[0] + R * 4].view(np.uint32) if R > 0 else np.zeros(0, np.uint32),
        keys=bb[b_off[1]:b_off[1] + R * 8].view(np.uint64) if R > 0 else np.zeros(0, np.uint64),
    )
    if planes:
        fT = ib[i_off[0]:i_off[0] + 3 * plane * 4].view(np.float32).reshape(3, plane)
        nc = ib[i_off[1]:i_off[1] + 2 * plane * 4].view(np.uint32).reshape(2, plane)
        out.update(final_T=np.stack([untile(fT[i]) for i in range(3)]), n_contrib=np.stack([untile(nc[i]) for i in range(2)]))
    return out


# ---- observed parity margins -----------------------------------------------------------------------------------------------------
# Every comparison below also RECORDS what it measured (per test and call site), next to what it asserted; tests/conftest.py writes
# the records to gpurun_out/parity_r05.json at the end of a GPU session and the summary committed under profiles/ is what the
# asserted tolerances are held against (<= 3x the observed value).
PARITY_LOG = []


def _where():
    import inspect
    import os
    test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
    for fr in inspect.stack(0)[2:]:
        fn = os.path.basename(fr.filename)
        if fn not in ("gpu_utils.py",):
            return test, "%s:%d" % (fn, fr.lineno)
    return test, ""


def _record(kind, name, observed, asserted):
    test, site = _where()
    PARITY_LOG.append({"test": test, "site": site, "kind": kind, "name": name, "observed": observed, "asserted": asserted})


def frac_close(a, b, atol, rtol=0.0, max_bad_frac=0.0, hard_atol=None, name=""):
    """|a-b| <= atol + rtol*|b| everywhere except a fraction max_bad_frac of entries (discrete
    contributor flips at the 1/255 and 1e-4 thresholds), which must still be within hard_atol."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    err = np.abs(a - b)
    bad = err > (atol + rtol * np.abs(b))
    frac = float(bad.mean()) if bad.size else 0.0
    if err.size:
        scaled = err / np.maximum(1.0, np.abs(b))   # abs <= 1e-5 max(1, |x|)
        _record("frac_close", name,
                {"max_err": float(err.max()), "p9999_err": float(np.quantile(err, 0.9999)), "p999_err": float(np.quantile(err, 0.999)),
                 "frac_over_asserted": frac, "frac_over_survey_1e-5": float((scaled > 1e-5).mean()), "n": int(err.size)},
                {"atol": atol, "rtol": rtol, "max_bad_frac": max_bad_frac, "hard_atol": hard_atol})
    assert frac <= max_bad_frac, "%s: %.3e of entries off (max err %.3e)" % (name, frac, float(err.max()))
    if hard_atol is not None and err.size:
        assert float(err.max()) <= hard_atol, "%s: max err %.3e > hard %.3e" % (name, float(err.max()), hard_atol)


def img_close(a, b, name, tol=1e-5, max_bad_frac=0.0, hard=None):
    """SURVEY section 8(c)'s image tolerance: |a - b| <= tol * max(1, |b|), on all but max_bad_frac of the entries (a contributor on the
    1/255 or 1e-4 threshold may flip: only the large scenes allow any), which must still be within `hard`."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    err = np.abs(a - b)
    if not err.size:
        return
    scaled = err / np.maximum(1.0, np.abs(b))
    frac = float((scaled > tol).mean())
    _record("img_close", name, {"max_err": float(err.max()), "max_scaled_err": float(scaled.max()), "p9999_scaled_err": float(np.quantile(scaled, 0.9999)),
                                "frac_over_tol": frac, "n": int(err.size)}, {"tol": tol, "max_bad_frac": max_bad_frac, "hard": hard})
    assert frac <= max_bad_frac, "%s: %.3e of entries beyond %.0e max(1, |x|) (max err %.3e)" % (name, frac, tol, float(err.max()))
    if hard is not None:
        assert float(err.max()) <= hard, "%s: max err %.3e > hard %.3e" % (name, float(err.max()), hard)


def rel_l2(a, b, record=True):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    v = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
    if record:
        _record("rel_l2", "", {"rel_l2": v}, None)   # (the bound is in the assert at the recorded call site)
    return v


def grad_close(a, b, name, tol_trim=2e-4, tol_all=5e-3, trim_frac=1e-3):
    """Per-surfel gradient parity.  fp32 evaluation of near edge-on surfels (p = k x l cancels) and
    contributors sitting on the 1/255 / 1e-4 thresholds make a handful of surfels ill-conditioned: the
    fp32 and fp64 builds of the ORACLE ITSELF differ by rel-L2 ~2.5e-3 on the 200k/800x800 scene with
    >99% of the squared error on <100 surfels.  So: relative L2 <= tol_trim after discarding the
    trim_frac of surfels with the largest error, and <= tol_all over everything."""
    a = np.asarray(a, np.float64).reshape(a.shape[0], -1)
    b = np.asarray(b, np.float64).reshape(b.shape[0], -1)
    e = np.linalg.norm(a - b, axis=1)
    denom = max(np.linalg.norm(b), 1e-30)
    full = float(np.linalg.norm(e) / denom)
    k = int(np.ceil(trim_frac * e.shape[0]))
    trimmed = float(np.linalg.norm(np.sort(e)[:e.shape[0] - k]) / denom) if e.shape[0] > k else 0.0
    _record("grad_close", name, {"rel_l2_trimmed": trimmed, "rel_l2_all": full}, {"tol_trim": tol_trim, "tol_all": tol_all, "trim_frac": trim_frac})
    assert trimmed <= tol_trim, "%s: trimmed rel-L2 %.3e" % (name, trimmed)
    assert full <= tol_all, "%s: rel-L2 %.3e" % (name, full)


def hip_median_contrib(case, dev="cuda:0"):
    """[H,W] 1-based list position of the entry the kernel picked as the median contributor (0: none), in the numbering of the
    REFERENCE's lists: the forward is re-run with the reference's tile rectangles (the default lists omit pairs that cannot reach
    alpha >= 1/255 -- same pixels, same picks, other positions)."""
    _C.set_tight_rects(False)
    try:
        return run_hip_raw(case, dev)["n_contrib"][1]
    finally:
        _C.set_tight_rects(True)


def median_flips(med_contrib, orc, max_frac=2e-4, tie_tol=2.5e-3):
    """The two median channels of the allmap (5: depth, 7: weight alpha*T of the LAST entry blended while T > 0.5,
    forward.cu:421-425) are a discontinuous pick: a pixel whose T sits on 0.5 to rounding takes a neighbouring contributor under
    any other fp32 evaluation order.  `med_contrib` [H,W] is the 1-based list position of the pick (0: none) as the kernel
    stores it for its backward (n_contrib plane 1; run_hip_raw) or as another oracle build computed it.  Returns the boolean mask
    of pixels whose pick differs from the oracle's, after PROVING for each of them, with the oracle's own per-pixel trace, that
    it is exactly a tie:
      * the entry the kernel picked is one the oracle blends for this pixel as well, and
      * every entry between the two picks was blended at a T within tie_tol of 0.5: the picks can only differ across ties.  tie_tol
        is what ONE contributor on the 1/255 alpha threshold upstream moves T by at T = 0.5 (0.5 / 255 = 2e-3; seen at 1 M surfels:
        T = 0.49976) plus rounding; such threshold flips are themselves bounded by the callers' pixel-fraction tolerances.
    Everywhere else the callers hold channels 5 and 7 to the tolerance of the summed channels.  At most max_frac of the pixels
    (never fewer than 2 allowed) may flip.  Gradient comparisons zero the cotangent of channels 5 and 7 on the returned mask: the
    derivative of a different entry's depth is not comparable, everything else is."""
    mc = np.asarray(med_contrib).astype(np.int64)
    diff = mc != orc.field("n_contrib")[1].astype(np.int64)
    ys, xs = np.nonzero(diff)
    assert len(ys) <= max(2, int(max_frac * diff.size)), "%d pixels with a different median contributor" % len(ys)
    for y, x in zip(ys, xs):
        contrib, vals = orc.pixel_trace(int(x), int(y))
        vals = np.asarray(vals, np.float64)
        above = np.nonzero(vals[:, 2] > 0.5)[0]
        i_orc = int(above[-1]) if len(above) else -1                     # the oracle's pick (-1: none)
        if mc[y, x] == 0:
            i_hip = -1
        else:
            at = np.nonzero(contrib == mc[y, x])[0]
            assert len(at) == 1, "pixel (%d,%d): median contributor %d is not an entry the oracle blends" % (x, y, mc[y, x])
            i_hip = int(at[0])
        lo, hi = min(i_hip, i_orc), max(i_hip, i_orc)
        # the picks differ across entries lo+1 .. hi: each of those was blended with T on the threshold
        ties = vals[lo + 1:hi + 1, 2]
        assert len(ties) and np.all(np.abs(ties - 0.5) <= tie_tol), "pixel (%d,%d): median differs without a tie at T = 0.5 (T = %s)" % (x, y, ties)
    return diff
