"""-m gpu: the training-loss kernels of csrc/loss_kernels.h (ssim_fwd_kernel, ssim_bwd_kernel and the combine rider in its last
workgroup, regloss_fwd_kernel / regloss_bwd_kernel, regloss_fused_kernel, loss_fwd_merged_kernel, loss_combine_kernel) against the
float64 reference of tests/loss_ref.py, per output, per REGION of the image and per term of the loss.

Tolerance, per output and per region r (loss_ref.image_regions: border / seam / interior of the 54 x 28 SSIM tiling;
loss_ref.allmap_regions: ordinary / rim pixels, each split into seam / inner of the 30 x 14 and 16 x 16 tilings):
    e_k = max_r |kernel - ref64|,  e_t = max_r |ref32 - ref64|  (ref32: the same formulas evaluated in float32 on the same device)
    e_k <= R * e_t + 4 * 2^-24 * scale_r
scale_r = max_r |ref64|; for dL/dimg it is max_r grad_scale, the adjoint with every term replaced by its absolute value (the
gradient is a sum that cancels: with img == gt it is 0 to 1e-19 in float64), and for the photometric loss value the largest
absolute term of its sum (loss_ref's loss_scale: with img == gt, lam * (1 - ssim) cancels to 1e-17 and the kernel's
A B * (1 / (Cc D)) is one rounding of the 1 away from it, while float32 PyTorch's A B / (Cc D) happens to be exactly 1).  The yardstick is the reference in float32, never the
kernel.  R is measured, not chosen: twice the largest e_k / e_t observed on an MI355X, rounded up to a power of two, one value for
values and maps and one for gradients; comparisons whose e_k lies within the four-ulp floor alone are left out of the maximum.
Every comparison prints one "LOSS ..." line; profiles/loss_fp64_margins.md holds the full listing.

Largest e_k / e_t per output and region over all 3838 comparisons (MI355X, ROCm build of this tree):

    output       region          ratio   case                                            e_k        e_t        floor
    d/ddepth     rim.seam         5.480  reg edges 14x30 ln=0.02 ld=0 g=2.5 atomics     7.314e+00  1.335e+00  2.550e+00
    loss         -                2.806  photo const 3x56x54 lam=1                      1.139e-04  4.059e-05  2.384e-07
    ssim         -                2.805  ssim const 3x56x54                             1.138e-04  4.059e-05  1.269e-07
    d/ddepth     ordinary.inner   1.864  reg plain 17x33 ln=0.02 ld=0 g=1 atomics       3.171e-10  1.702e-10  5.629e-11
    d/ddepth     rim.inner        1.794  reg edges 17x33 ln=0.02 ld=0 g=1 atomics       2.690e-10  1.499e-10  5.607e-11
    dm_dmu1      border           1.720  ssim rand 3x11x1                               3.449e-06  2.005e-06  9.696e-07
    dm_dmu1      seam             1.572  ssim rand 1x28x108                             2.313e-05  1.471e-05  1.592e-06
    dm_ds12      interior         1.422  ssim rand 1x28x108                             5.745e-05  4.041e-05  6.512e-06
    dm_ds12      seam             1.419  ssim rand 1x28x108                             2.587e-05  1.823e-05  4.506e-06
    dL/dimg      seam             1.411  photo smooth 1x28x108 lam=1 g=1                7.211e-08  5.112e-08  6.564e-08
    dm_ds12      border           1.327  ssim rand 1x28x108                             2.974e-05  2.241e-05  6.430e-06
    dm_ds11      border           1.298  ssim rand 1x28x108                             1.672e-05  1.288e-05  1.649e-06
    dL/dimg      border           1.224  photo smooth 3x56x54 lam=0.2 g=1               3.572e-09  2.920e-09  3.057e-09
    d/dnormal.z  all              1.195  reg edges 17x33 ln=0.02 ld=0 g=2.5 atomics     3.782e-11  3.166e-11  1.820e-11
    dL/dimg      interior         1.171  photo smooth 3x29x55 lam=0.2 g=1               1.468e-08  1.253e-08  8.568e-09
    d/dnormal.x  all              1.099  reg edges 43x17 ln=0.02 ld=0 g=1 atomics       2.092e-11  1.904e-11  6.044e-12
    d/ddepth     ordinary.seam    1.084  reg edges 43x17 ln=0.02 ld=0 g=1 fused         2.779e-10  2.563e-10  3.944e-11
    dm_dmu1      interior         1.056  ssim rand 3x29x55                              2.564e-05  2.428e-05  2.349e-06
    dm_ds11      seam             0.995  ssim rand 1x28x108                             1.199e-05  1.204e-05  1.431e-06
    dm_ds11      interior         0.976  ssim rand 3x28x54                              1.727e-05  1.769e-05  1.760e-06
    d/dnormal.y  all              0.793  merged 3x42x45                                 1.373e-11  1.731e-11  2.456e-12
    (within the floor everywhere: dssim/dimg border, dssim/dimg interior, dssim/dimg seam, d/ddist all)

Values and maps: largest 2.806 -> R_VAL = 8.  Gradients: largest 5.480 -> R_GRAD = 16.
No region comes near the 16 that would have wanted an explanation.  The two largest: the rim of the zero-depth block, where the
atomic path adds four terms of up to 1e12 times an ordinary gradient in the order they arrive; and flat images (img = 0.75, gt =
0.25), where s11 - mu1^2 cancels against C2 = 9e-4 and float32 PyTorch itself is 4e-5 off in the SSIM value -- the float32
formulation's own limit, not the kernel's (its gradient stays within the floor).

The depth gradient (plane 5 of d_allmap) is compared on ordinary and rim pixels separately: at the rim of a zero-depth block
F.normalize's eps = 1e-12 branch amplifies it by twelve orders of magnitude, and one maximum over the plane would leave every
ordinary pixel unchecked.

Embedding test (c): the three derivative maps of an image are bit-identical to those of the same image placed anywhere in a larger
zero canvas.  dL/dimg carries the factor 1 / (C H W), which differs between the image and the canvas, so it is bit-identical between
any two OFFSETS in the canvas (same factor) and equal to the small image's to two roundings after rescaling.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch

import loss_ref as lr

pytestmark = pytest.mark.gpu

R_VAL = 8.0
R_GRAD = 16.0
EPS32 = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")


def _ops():
    from dgs_amd import _ops
    return _ops


def _lib():
    return _ops().load()


def _st():
    return _ops()._stream(torch.device("cuda", torch.cuda.current_device()))


def _ok(rc, what):
    _ops()._check(_lib(), rc, what)


def _full(shape, value=NAN):
    return torch.full(shape, value, dtype=F32, device="cuda")


def _scalar(v):
    return torch.tensor([v], dtype=F32, device="cuda")


# ---- thin wrappers of the C entry points: every output buffer is prefilled with NaN --------------------------------------------------
def photo_blocks(C, H, W):
    return int(_lib().dgs_photo_blocks(C, H, W))


def photo_forward(img, gt, gt_slot=None):
    C, H, W = img.shape
    part, maps = _full((2 * photo_blocks(C, H, W),)), _full((3, C, H, W))
    _ok(_lib().dgs_photo_forward(C, H, W, img.data_ptr(), gt.data_ptr(), part.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                 maps[2].data_ptr(), gt_slot, _st()), "dgs_photo_forward")
    return part, maps


def loss_combine(photo, nphoto, reg, nreg, n, lam):
    out = _full((1,))
    _ok(_lib().dgs_loss_combine(photo.data_ptr(), nphoto, reg.data_ptr(), nreg, n, lam, out.data_ptr(), _st()), "dgs_loss_combine")
    return out


def photo_backward(img, gt, maps, lam, g, gt_slot=None, rider=None):
    """rider: None (dgs_photo_backward) or (photo partials, nphoto, reg partials, nreg): dgs_photo_backward_combine -> (dL/dimg, loss)"""
    C, H, W = img.shape
    out = _full((C, H, W))
    gd = _scalar(g)
    if rider is None:
        _ok(_lib().dgs_photo_backward(C, H, W, img.data_ptr(), gt.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                      lam, gd.data_ptr(), out.data_ptr(), gt_slot, _st()), "dgs_photo_backward")
        return out
    loss = _full((1,))
    photo, nphoto, reg, nreg = rider
    _ok(_lib().dgs_photo_backward_combine(C, H, W, img.data_ptr(), gt.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(), maps[2].data_ptr(),
                                          lam, gd.data_ptr(), out.data_ptr(), gt_slot, photo.data_ptr(), nphoto, reg.data_ptr(), nreg,
                                          loss.data_ptr(), _st()), "dgs_photo_backward_combine")
    return out, loss


def reg_forward_partials(allmap, cam, ln, ld, rays_slot=None, zero_plane=None, z=True):
    H, W = allmap.shape[1:]
    rd, ro, wvt = cam
    part = _full((int(_lib().dgs_regloss_blocks(H, W)),))
    if z:
        _ok(_lib().dgs_regloss_forward_partials_z(H, W, allmap.data_ptr(), rd.data_ptr(), ro.data_ptr(), wvt.data_ptr(), ln, ld, part.data_ptr(),
                                                  rays_slot, None if zero_plane is None else zero_plane.data_ptr(), _st()),
            "dgs_regloss_forward_partials_z")
    else:
        _ok(_lib().dgs_regloss_forward_partials(H, W, allmap.data_ptr(), rd.data_ptr(), ro.data_ptr(), wvt.data_ptr(), ln, ld, part.data_ptr(),
                                                rays_slot, _st()), "dgs_regloss_forward_partials")
    return part


def reg_backward_slot(allmap, cam, ln, ld, g, d_allmap, rays_slot=None, write_all=1):
    H, W = allmap.shape[1:]
    rd, ro, wvt = cam
    gd = _scalar(g)
    _ok(_lib().dgs_regloss_backward_slot(H, W, allmap.data_ptr(), rd.data_ptr(), ro.data_ptr(), wvt.data_ptr(), ln, ld, gd.data_ptr(),
                                         d_allmap.data_ptr(), rays_slot, write_all, _st()), "dgs_regloss_backward_slot")
    return d_allmap


def reg_fused(allmap, cam, ln, ld, rays_slot=None):
    H, W = allmap.shape[1:]
    rd, ro, wvt = cam
    part, d_allmap = _full((int(_lib().dgs_regloss_fused_blocks(H, W)),)), _full((8, H, W))
    _ok(_lib().dgs_regloss_fused(H, W, allmap.data_ptr(), rd.data_ptr(), ro.data_ptr(), wvt.data_ptr(), ln, ld, part.data_ptr(),
                                 d_allmap.data_ptr(), rays_slot, _st()), "dgs_regloss_fused")
    return part, d_allmap


def forward_merged(img, gt, allmap, cam, ln, ld, gt_slot=None, rays_slot=None):
    C, H, W = img.shape
    rd, ro, wvt = cam
    pp, maps = _full((2 * photo_blocks(C, H, W),)), _full((3, C, H, W))
    rp, d_allmap = _full((int(_lib().dgs_regloss_fused_blocks(H, W)),)), _full((8, H, W))
    _ok(_lib().dgs_loss_forward_merged(C, H, W, img.data_ptr(), gt.data_ptr(), pp.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                       maps[2].data_ptr(), gt_slot, allmap.data_ptr(), rd.data_ptr(), ro.data_ptr(), wvt.data_ptr(), ln, ld,
                                       rp.data_ptr(), d_allmap.data_ptr(), rays_slot, _st()), "dgs_loss_forward_merged")
    return pp, maps, rp, d_allmap


def reg_value(part):
    """The regulariser partials through dgs_loss_combine: one zero photometric partial, lambda_dssim = 0, n = 1 -> sum(part)."""
    return loss_combine(torch.zeros(2, dtype=F32, device="cuda"), 1, part, part.numel(), 1, 0.0)


# ---- cases: built once, shared, never modified ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _images(kind, shape):
    return tuple(t.cuda() for t in lr.make_images(kind, *shape))


@functools.lru_cache(maxsize=None)
def _photo_refs(kind, shape, lam):
    img, gt = _images(kind, shape)
    return lr.photo_reference(img, gt, lam, F64), lr.photo_reference(img, gt, lam, F32)


@functools.lru_cache(maxsize=None)
def _camera(H, W):
    return lr.make_camera(H, W, "cuda")


@functools.lru_cache(maxsize=None)
def _allmap(kind, H, W):
    return lr.make_allmap(kind, H, W).cuda()


@functools.lru_cache(maxsize=None)
def _reg_refs(kind, H, W, ln, ld, g=1.0):
    am, (rd, ro, wvt) = _allmap(kind, H, W), _camera(H, W)
    return lr.reg_reference(am, rd, ro, wvt, ln, ld, F64, g), lr.reg_reference(am, rd, ro, wvt, ln, ld, F32, g)


@functools.lru_cache(maxsize=None)
def _allmap_regions(kind, H, W):
    r64 = _reg_refs(kind, H, W, 0.02, 1000.0)[0]
    return lr.allmap_regions(_allmap(kind, H, W), r64["vnorm"], r64["interior"])


@functools.lru_cache(maxsize=None)
def _image_regions(H, W):
    return lr.image_regions(H, W, "cuda")


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def _line(case, what, region, e_k, e_t, floor, R, fails):
    ratio = e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf"))
    print("LOSS %-44s %-12s %-15s e_k %.3e e_t %.3e floor %.3e ratio %9.3f %s" % (case, what, region, e_k, e_t, floor, ratio,
                                                                                   "floor" if e_k <= floor else "R"))
    if not e_k <= R * e_t + floor:
        fails.append("%s %s %s: e_k %.3e > %g * e_t %.3e + %.3e" % (case, what, region, e_k, R, e_t, floor))


def _cmp_value(case, what, got, r64, r32, R, fails, scale=None):
    a = float(r64)
    _line(case, what, "-", abs(float(got) - a), abs(float(r32) - a), 4 * EPS32 * (abs(a) if scale is None else float(scale)), R, fails)


def _cmp_field(case, what, got, r64, r32, regions, R, fails, scale=None):
    """got, r64, r32, scale: [..., H, W];  regions: {label: [H,W] bool}"""
    assert got.shape == r64.shape, (case, what, tuple(got.shape), tuple(r64.shape))
    fin = torch.isfinite(got)
    if not bool(fin.all()):
        fails.append("%s %s: %d non-finite elements" % (case, what, int((~fin).sum())))
        return
    ek, et, sc = (got.double() - r64).abs(), (r32.double() - r64).abs(), (r64.abs() if scale is None else scale.double())
    for label, m in regions.items():
        if not bool(m.any()):
            continue
        _line(case, what, label, float(ek[..., m].max()), float(et[..., m].max()), 4 * EPS32 * float(sc[..., m].max()), R, fails)


# ---- a. SSIM alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lr.PHOTO_SHAPES)
def test_ssim_alone(shape):
    """fused_ssim: dgs_ssim_forward with the atomic sum and dgs_ssim_backward, upstream gradient 3; the three derivative maps it
    saves are fetched through the C entry point and compared region by region."""
    C, H, W = shape
    regions = _image_regions(H, W)
    fails = []
    for kind in ("rand", "const"):
        img, gt = _images(kind, shape)
        r64, r32 = _photo_refs(kind, shape, 1.0)
        case = "ssim %s %dx%dx%d" % (kind, C, H, W)
        a = img.clone().requires_grad_(True)
        v = _ops().fused_ssim(a, gt)
        (3.0 * v).backward()
        _cmp_value(case, "ssim", v.detach(), r64["ssim"], r32["ssim"], R_VAL, fails)
        v = v.detach()
        _cmp_field(case, "dssim/dimg", a.grad, 3.0 * r64["ssim_grad"], 3.0 * r32["ssim_grad"], regions, R_GRAD, fails, 3.0 * r64["ssim_grad_scale"])
        total, maps = torch.zeros(1, dtype=F32, device="cuda"), _full((3, C, H, W))
        _ok(_lib().dgs_ssim_forward(C, H, W, img.data_ptr(), gt.data_ptr(), total.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                    maps[2].data_ptr(), _st()), "dgs_ssim_forward")
        assert float(total) / (C * H * W) == pytest.approx(float(v), rel=1e-5)
        for i, k in enumerate(("dm_dmu1", "dm_ds11", "dm_ds12")):
            _cmp_field(case, k, maps[i], r64[k], r32[k], regions, R_VAL, fails)
    assert not fails, "\n".join(fails)


# ---- b. photometric part of the train loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lr.PHOTO_SHAPES)
def test_photometric_part(shape):
    """dgs_photo_forward -> dgs_loss_combine -> dgs_photo_backward with the regularisers' partials of a zero allmap at lambda_normal =
    lambda_dist = 0.  img == gt: dL/dimg within the floor of 0 everywhere, and exactly 0 where only the L1 term is on (sign(0) = 0)."""
    C, H, W = shape
    regions = _image_regions(H, W)
    zero_reg = reg_forward_partials(torch.zeros(8, H, W, device="cuda"), _camera(H, W), 0.0, 0.0)
    assert bool((zero_reg == 0).all())
    fails = []
    for kind in lr.IMAGE_KINDS:
        img, gt = _images(kind, shape)
        part, maps = photo_forward(img, gt)
        assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(maps).all())
        nb = photo_blocks(C, H, W)
        for lam in (0.2, 0.0, 1.0):
            r64, r32 = _photo_refs(kind, shape, lam)
            case = "photo %s %dx%dx%d lam=%g" % (kind, C, H, W, lam)
            loss = loss_combine(part, nb, zero_reg, zero_reg.numel(), C * H * W, lam)
            _cmp_value(case, "loss", loss, r64["loss"], r32["loss"], R_VAL, fails, r64["loss_scale"])
            for g in (1.0, -0.5, 0.0):
                grad = photo_backward(img, gt, maps, lam, g)
                _cmp_field(case + " g=%g" % g, "dL/dimg", grad, g * r64["grad"], g * r32["grad"], regions, R_GRAD, fails, abs(g) * r64["grad_scale"])
                if kind == "equal":
                    floor = 4 * EPS32 * abs(g) * float(r64["grad_scale"].max())
                    assert float(grad.abs().max()) <= floor, (case, g, float(grad.abs().max()), floor)
                    if lam == 0.0:
                        assert float(grad.abs().max()) == 0.0, (case, g)
            if kind == "equal":
                assert float(part[nb:].abs().max()) == 0.0                  # the |img - gt| partials
    assert not fails, "\n".join(fails)


def test_photometric_part_through_fused_train_loss():
    shape = (3, 29, 55)
    C, H, W = shape
    img, gt = _images("rand", shape)
    r64, r32 = _photo_refs("rand", shape, 0.2)
    fails = []
    for g in (1.0, -0.5):
        a = img.clone().requires_grad_(True)
        am = torch.zeros(8, H, W, device="cuda", requires_grad=True)
        loss = _ops().fused_train_loss(a, am, gt, *_camera(H, W), 0.2, 0.0, 0.0)
        loss.backward(torch.tensor(g, device="cuda"))
        case = "train_loss rand %dx%dx%d g=%g" % (C, H, W, g)
        _cmp_value(case, "loss", loss.detach(), r64["loss"], r32["loss"], R_VAL, fails, r64["loss_scale"])
        _cmp_field(case, "dL/dimg", a.grad, g * r64["grad"], g * r32["grad"], _image_regions(H, W), R_GRAD, fails, abs(g) * r64["grad_scale"])
        assert float(am.grad.abs().max()) == 0.0
    assert not fails, "\n".join(fails)


# ---- c. embedding exactness -----------------------------------------------------------------------------------------------------------
def test_embedding_in_a_zero_canvas_is_exact():
    """Zero-padded windows: the blurs of an image are the blurs of the same image placed at (oy, ox) in a larger zero canvas, the
    kernel adds its taps in a fixed order, and adding an exact zero is exact -- wherever the tile seams (x = 54, y = 28) fall."""
    C, h, w, Hc, Wc = 3, 20, 40, 57, 109
    img, gt = _images("rand", (C, h, w))
    _, maps = photo_forward(img, gt)
    one = _scalar(1.0)

    def ssim_backward(a, b, m):
        out = _full(tuple(a.shape))
        _ok(_lib().dgs_ssim_backward(a.shape[0], a.shape[1], a.shape[2], a.data_ptr(), b.data_ptr(), m[0].data_ptr(), m[1].data_ptr(),
                                     m[2].data_ptr(), one.data_ptr(), out.data_ptr(), _st()), "dgs_ssim_backward")
        return out

    small = ssim_backward(img, gt, maps)
    base = None
    for oy, ox in ((0, 0), (20, 30), (27, 53), (9, 14)):
        ci, cg = torch.zeros(C, Hc, Wc, device="cuda"), torch.zeros(C, Hc, Wc, device="cuda")
        ci[:, oy:oy + h, ox:ox + w], cg[:, oy:oy + h, ox:ox + w] = img, gt
        _, cmaps = photo_forward(ci, cg)
        own = cmaps[:, :, oy:oy + h, ox:ox + w]
        for i, k in enumerate(("dm_dmu1", "dm_dsigma1_sq", "dm_dsigma12")):
            diff = own[i] != maps[i]
            assert not bool(diff.any()), "offset (%d, %d) %s: %d elements differ, first at %s" % (oy, ox, k, int(diff.sum()), diff.nonzero()[0].tolist())
        inner = ssim_backward(ci, cg, cmaps)[:, oy + 5:oy + h - 5, ox + 5:ox + w - 5]
        if base is None:
            base = inner
            # against the image on its own: the same sums times 1 / (C h w) instead of 1 / (C Hc Wc) -- the rounding of the factor
            # and of the product on either side: 4 * 2^-24 and second-order terms, element by element
            a, b = small[:, 5:-5, 5:-5].double() * (C * h * w), inner.double() * (C * Hc * Wc)
            assert bool(((a - b).abs() <= 4.5 * EPS32 * a.abs()).all())
        diff = inner != base
        assert not bool(diff.any()), "offset (%d, %d) dL/dimg: %d elements differ, first at %s" % (oy, ox, int(diff.sum()), diff.nonzero()[0].tolist())


# ---- d. regularisers: three implementations --------------------------------------------------------------------------------------------
LAMBDAS = ((0.02, 0.0), (0.0, 1000.0), (0.02, 1000.0))


def _cmp_allmap_grad(case, got, r64, r32, regions, fails):
    assert torch.equal(torch.isfinite(got), torch.isfinite(r64["grad"])), case + ": finite pattern"
    assert float(got[[0, 1, 7]].abs().max()) == 0.0, case + ": planes 0, 1, 7"
    whole = {"all": torch.ones_like(regions["ordinary.inner"])}
    for p, name in ((2, "d/dnormal.x"), (3, "d/dnormal.y"), (4, "d/dnormal.z"), (6, "d/ddist")):
        _cmp_field(case, name, got[p], r64["grad"][p], r32["grad"][p], whole, R_GRAD, fails)
    _cmp_field(case, "d/ddepth", got[5], r64["grad"][5], r32["grad"][5], regions, R_GRAD, fails)


@pytest.mark.parametrize("shape", lr.REG_SHAPES)
def test_regularisers_three_implementations(shape):
    """(i) fused_reg_loss: dgs_regloss_forward / _backward with atomics into a caller-zeroed gradient; (ii) the partials path:
    dgs_regloss_forward_partials_z clearing plane 5 + dgs_loss_combine + dgs_regloss_backward_slot(write_all = 1) into a NaN-prefilled
    buffer; (iii) dgs_regloss_fused into a NaN-prefilled buffer.  Each term's value on its own, plane 5 on ordinary and rim pixels
    separately."""
    H, W = shape
    cam = _camera(H, W)
    fails = []
    for kind in lr.ALLMAP_KINDS:
        am = _allmap(kind, H, W)
        regions = _allmap_regions(kind, H, W)
        for ln, ld in LAMBDAS:
            for g in (1.0, 2.5):
                r64, r32 = _reg_refs(kind, H, W, ln, ld, g)
                case = "reg %s %dx%d ln=%g ld=%g g=%g" % (kind, H, W, ln, ld, g)
                # (i)
                a = am.clone().requires_grad_(True)
                loss = _ops().fused_reg_loss(a, *cam, ln, ld)
                loss.backward(torch.tensor(g, device="cuda"))
                _cmp_value(case + " atomics", "loss", loss.detach(), r64["loss"], r32["loss"], R_VAL, fails)
                _cmp_allmap_grad(case + " atomics", a.grad, r64, r32, regions, fails)
                # (ii)
                d_allmap = _full((8, H, W))
                part = reg_forward_partials(am, cam, ln, ld, zero_plane=d_allmap[5])
                assert bool((d_allmap[5] == 0).all()) and bool(torch.isnan(d_allmap[[0, 1, 2, 3, 4, 6, 7]]).all())
                _cmp_value(case + " partials", "loss", reg_value(part), r64["loss"], r32["loss"], R_VAL, fails)
                d_allmap[5] = NAN
                torch.cuda.synchronize()
                probe = reg_backward_slot(am, cam, ln, ld, g, d_allmap.clone())
                assert bool(torch.isfinite(probe[[0, 1, 2, 3, 4, 6, 7]]).all()), case + ": write_all leaves elements unwritten"
                d_allmap[5] = 0.0
                _cmp_allmap_grad(case + " partials", reg_backward_slot(am, cam, ln, ld, g, d_allmap), r64, r32, regions, fails)
                if g == 1.0:
                    # (iii)
                    part, d_allmap = reg_fused(am, cam, ln, ld)
                    assert bool(torch.isfinite(d_allmap).all()) and bool(torch.isfinite(part).all()), case + ": fused leaves elements unwritten"
                    _cmp_value(case + " fused", "loss", reg_value(part), r64["loss"], r32["loss"], R_VAL, fails)
                    _cmp_allmap_grad(case + " fused", d_allmap, r64, r32, regions, fails)
    assert not fails, "\n".join(fails)


# ---- e. merged forward ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(lr.MERGED_SHAPES))
def test_merged_forward_equals_the_two_calls(shape):
    """include/dgs_train_ops.h: "Same outputs, bit for bit, as the two calls" -- with more, fewer and equally many photometric
    workgroups than regulariser ones, and C = 1."""
    C, H, W = shape
    ns, nr = lr.MERGED_SHAPES[shape]
    assert photo_blocks(C, H, W) == ns and int(_lib().dgs_regloss_fused_blocks(H, W)) == nr
    img, gt = _images("rand", shape)
    am, cam = _allmap("edges", H, W), _camera(H, W)
    ln, ld, lam = 0.02, 1000.0, 0.2
    pp, maps, rp, d_allmap = forward_merged(img, gt, am, cam, ln, ld)
    pp2, maps2 = photo_forward(img, gt)
    rp2, d_allmap2 = reg_fused(am, cam, ln, ld)
    for name, u, v in (("photometric partials", pp, pp2), ("maps", maps, maps2), ("regulariser partials", rp, rp2), ("d_allmap", d_allmap, d_allmap2)):
        assert bool(torch.isfinite(u).all()), name
        assert torch.equal(u, v), "%s: %d elements differ" % (name, int((u != v).sum()))
    grad, loss = photo_backward(img, gt, maps, lam, 1.0, rider=(pp, ns, rp, nr))
    p64, p32 = _photo_refs("rand", shape, lam)
    q64, q32 = _reg_refs("edges", H, W, ln, ld)
    fails = []
    case = "merged %dx%dx%d" % shape
    _cmp_value(case, "loss", loss, p64["loss"] + q64["loss"], p32["loss"] + q32["loss"], R_VAL, fails,
               max(float(p64["loss_scale"]), abs(float(p64["loss"] + q64["loss"]))))
    _cmp_field(case, "dL/dimg", grad, p64["grad"], p32["grad"], _image_regions(H, W), R_GRAD, fails, p64["grad_scale"])
    _cmp_allmap_grad(case, d_allmap, q64, q32, _allmap_regions("edges", H, W), fails)
    assert not fails, "\n".join(fails)


# ---- f. slots -------------------------------------------------------------------------------------------------------------------------
def test_slots_choose_target_and_rays():
    """gt_slot / rays_slot point at the real target and ray table while the plain gt / rays_d arguments hold valid decoys of the right
    size: every output equals the direct call's bit for bit, and follows the slot when it is rewritten."""
    shape = (3, 29, 55)
    C, H, W = shape
    img, gt = _images("rand", shape)
    gt2 = _images("hdr", shape)[1]
    am, (rd, ro, wvt) = _allmap("plain", H, W), _camera(H, W)      # (no rim: the pair path's plane 5 is compared across two launches)
    rd2 = (rd * 1.25 + 0.01).contiguous()
    ln, ld, lam, g = 0.02, 1000.0, 0.2, 1.5
    decoy_gt, decoy_rd = torch.rand_like(gt) + 2.0, torch.rand_like(rd) - 3.0
    slots = torch.zeros(2, dtype=torch.int64, device="cuda")
    gslot, rslot = slots.data_ptr(), slots.data_ptr() + 8

    def run(gt_, rd_, gs, rs):
        cam_ = (rd_, ro, wvt)
        out = {}
        out["photo.part"], out["photo.maps"] = photo_forward(img, gt_, gs)
        out["photo.grad"] = photo_backward(img, gt_, out["photo.maps"], lam, g, gs)
        out["fused.part"], out["fused.d_allmap"] = reg_fused(am, cam_, ln, ld, rs)
        out["pair.part"] = reg_forward_partials(am, cam_, ln, ld, rs, z=False)
        out["pair.d_allmap"] = reg_backward_slot(am, cam_, ln, ld, g, torch.zeros(8, H, W, device="cuda"), rs)
        m = forward_merged(img, gt_, am, cam_, ln, ld, gs, rs)
        out.update({"merged.%d" % i: t for i, t in enumerate(m)})
        torch.cuda.synchronize()
        return out

    prev = None
    for target, rays in ((gt, rd), (gt2, rd2)):
        slots.copy_(torch.tensor([target.data_ptr(), rays.data_ptr()], dtype=torch.int64))
        torch.cuda.synchronize()
        direct = run(target, rays, None, None)
        slotted = run(decoy_gt, decoy_rd, gslot, rslot)
        for k in direct:
            if k == "pair.d_allmap":      # float atomics into plane 5: another launch is another order
                keep = [0, 1, 2, 3, 4, 6, 7]
                assert torch.equal(direct[k][keep], slotted[k][keep]), k
                assert float((direct[k][5] - slotted[k][5]).abs().max()) <= 16 * EPS32 * float(direct[k][5].abs().max()), k
            else:
                assert torch.equal(direct[k], slotted[k]), k
        if prev is not None:
            for k in direct:
                assert not torch.equal(direct[k], prev[k]), k + " does not follow the slot"
        prev = direct


# ---- g. combine -----------------------------------------------------------------------------------------------------------------------
def test_combine_and_its_rider():
    """dgs_loss_combine and the copy in the last workgroup of the SSIM backward on hand-made partials whose counts are no multiples of
    256 or 1024, against the float64 sum.  Bound: every partial passes through at most 2 + 2 + 6 + 3 = 13 float additions (a
    thread's strided sum, its four accumulators, the wave's butterfly, the four waves) and the closing formula has six more
    operations: 2^-24 * 19 <= 32 * 2^-24 times the sum of the terms' absolute values."""
    shape = (3, 29, 55)
    C, H, W = shape
    img, gt = _images("rand", shape)
    _, maps = photo_forward(img, gt)
    plain = photo_backward(img, gt, maps, 0.2, 1.0)
    gen = torch.Generator().manual_seed(7)
    n, lam = 12345, 0.2
    for nphoto in (1, 255, 256, 257, 1023, 1025, 1305):
        for nreg in (1, 257, 1566):
            photo = (torch.randn(2 * nphoto, generator=gen) * torch.pow(10.0, 3 * torch.rand(2 * nphoto, generator=gen))).cuda()
            reg = (torch.randn(nreg, generator=gen) * torch.pow(10.0, -3 * torch.rand(nreg, generator=gen))).cuda()
            a, b, r = photo[:nphoto].double(), photo[nphoto:].double(), reg.double()
            inv_n = 1.0 / n
            want = (1.0 - lam) * float(b.sum()) * inv_n + lam * (1.0 - float(a.sum()) * inv_n) + float(r.sum())
            bound = 32 * EPS32 * ((1.0 - lam) * float(b.abs().sum()) * inv_n + lam * (1.0 + float(a.abs().sum()) * inv_n) + float(r.abs().sum()))
            got = loss_combine(photo, nphoto, reg, nreg, n, lam)
            print("LOSS combine nphoto=%d nreg=%d err %.3e bound %.3e" % (nphoto, nreg, abs(float(got) - want), bound))
            assert abs(float(got) - want) <= bound, (nphoto, nreg, float(got), want, bound)
            # the rider divides by the image's own element count
            alone = loss_combine(photo, nphoto, reg, nreg, C * H * W, lam)
            grad, ridden = photo_backward(img, gt, maps, lam, 1.0, rider=(photo, nphoto, reg, nreg))
            assert torch.equal(ridden, alone), (nphoto, nreg, float(ridden), float(alone))
            assert torch.equal(grad, plain), (nphoto, nreg)


# ---- h. unit-gradient path end to end -------------------------------------------------------------------------------------------------
def test_unit_gradient_end_to_end(tmp_path):
    """fused_train_loss(unit_grad=True) with the merged forward (this process) and with DGS_MERGED_LOSS_FORWARD=0 (a fresh child
    process): both against the references, gradients bit-identical between the two."""
    shape = (3, 57, 109)
    C, H, W = shape
    assert _ops()._MERGED_LOSS_FORWARD, "this test wants the default setting in its own process"
    res = {}
    for merged in (True, False):
        out = str(tmp_path / ("unit_%d.pt" % merged))
        if merged:
            lr.unit_probe(out, C, H, W)
        else:
            env = dict(os.environ, DGS_MERGED_LOSS_FORWARD="0")
            p = subprocess.run([sys.executable, os.path.join(HERE, "loss_ref.py"), out, str(C), str(H), str(W)], env=env, capture_output=True,
                               text=True, timeout=300)
            assert p.returncode == 0, p.stderr[-2000:]
        res[merged] = torch.load(out)
        assert res[merged]["merged"] == merged
    lam, ln, ld = 0.2, 0.02, 1000.0
    p64, p32 = _photo_refs("rand", shape, lam)
    q64, q32 = _reg_refs("edges", H, W, ln, ld)
    fails = []
    for merged in (True, False):
        case = "unit merged=%d" % merged
        r = res[merged]
        _cmp_value(case, "loss", r["loss"], p64["loss"] + q64["loss"], p32["loss"] + q32["loss"], R_VAL, fails,
                   max(float(p64["loss_scale"]), abs(float(p64["loss"] + q64["loss"]))))
        _cmp_field(case, "dL/dimg", r["g_image"].cuda(), p64["grad"], p32["grad"], _image_regions(H, W), R_GRAD, fails, p64["grad_scale"])
        _cmp_allmap_grad(case, r["g_allmap"].cuda(), q64, q32, _allmap_regions("edges", H, W), fails)
    assert torch.equal(res[True]["g_image"], res[False]["g_image"]) and torch.equal(res[True]["g_allmap"], res[False]["g_allmap"])
    assert torch.equal(res[True]["loss"], res[False]["loss"])
    assert not fails, "\n".join(fails)
