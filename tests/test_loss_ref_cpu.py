"""The float64 reference of the loss kernels (tests/loss_ref.py) is itself checked here, without a GPU: against the independent
formulations of dgs_amd (conv2d SSIM, render.depth_to_normal + losses.training_loss), against the golden recorded from the original
project, and for the input conditions the comparisons of tests/test_loss_fp64_gpu.py rest on."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_ref as lr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_loss_golden import View, depth_map, images  # noqa: E402  (input formulas only)

from dgs_amd import losses  # noqa: E402
from dgs_amd import render as render_mod  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "loss_golden.npz"))
F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---- against independent formulations -----------------------------------------------------------------------------------------------
@pytest.fixture
def same_window(monkeypatch):
    """losses._window_1d sums the eleven float weights in torch.sum's order, make_gauss() (and loss_ref) one after the other: the
    normalised weights differ by one float32 ulp.  The conv2d formulation is given the kernel's weights, so that what is compared to
    1e-12 is the formulation, not the window."""
    monkeypatch.setitem(losses._WINDOWS, (11, 1.5, "cpu", F64), lr.gauss_window(F64))


def test_window_is_make_gauss_and_the_conv2d_window():
    w = lr.gauss_window(torch.float32)
    assert float((w - losses._window_1d(11, 1.5, "cpu", torch.float32)).abs().max()) <= 2.0 ** -23 * float(w.max())   # one ulp
    assert torch.equal(w, w.flip(0)) and abs(float(w.double().sum()) - 1.0) < 2e-7
    x = torch.rand(2, 9, 13, dtype=F64)
    got = lr.blur(x, w.double())
    want = losses._blur(x[None], w.double(), 2)[0]
    assert float((got - want).abs().max()) <= 1e-15


@pytest.mark.parametrize("shape", [(3, 6, 11), (1, 28, 108), (3, 57, 109)])
@pytest.mark.parametrize("kind", lr.IMAGE_KINDS)
def test_photo_reference_matches_conv2d_autograd(kind, shape, same_window):
    img, gt = lr.make_images(kind, *shape)
    for lam, g in ((0.2, 1.0), (1.0, -0.5), (0.0, 3.0)):
        r = lr.photo_reference(img, gt, lam, F64, g)
        a = img.double().requires_grad_(True)
        l1, ssim = losses.l1_loss(a, gt.double()), losses.ssim_torch(a, gt.double())
        loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
        grad, = torch.autograd.grad(loss * g, a, retain_graph=True)
        sgrad, = torch.autograd.grad(ssim, a)
        loss, l1, ssim = loss.detach(), l1.detach(), ssim.detach()
        assert abs(float(r["loss"]) - float(loss)) <= 1e-12 * abs(float(loss)) + 1e-300
        assert abs(float(r["l1"]) - float(l1)) <= 1e-12 * abs(float(l1)) and abs(float(r["ssim"]) - float(ssim)) <= 1e-12 * abs(float(ssim))
        # a gradient that cancels (img == gt: 1e-19) is held to 1e-12 of the terms it is the sum of
        assert float((r["grad"] - grad).abs().max()) <= 1e-12 * float(r["grad_scale"].max())
        assert float((r["ssim_grad"] - sgrad).abs().max()) <= 1e-12 * float(r["ssim_grad_scale"].max())
        assert bool((r["grad"].abs() <= r["grad_scale"] * (1 + 1e-12)).all())
    if kind == "equal":
        r = lr.photo_reference(img, gt, 0.2, F64)
        assert float(r["grad"].abs().max()) <= 1e-15 * float(r["grad_scale"].max()) and float(r["l1"]) == 0.0


@pytest.mark.parametrize("shape", [(13, 29), (17, 33), (43, 17)])
@pytest.mark.parametrize("kind", lr.ALLMAP_KINDS)
def test_reg_reference_matches_training_loss(kind, shape):
    H, W = shape
    allmap = lr.make_allmap(kind, H, W)
    rd, ro, wvt = lr.make_camera(H, W)
    cam = SimpleNamespace(rays_d=rd.double(), rays_o=ro.double(), world_view_transform=wvt.double())
    for ln, ld, g in ((0.02, 0.0, 1.0), (0.0, 1000.0, 1.0), (0.02, 1000.0, 2.5)):
        r = lr.reg_reference(allmap, rd, ro, wvt, ln, ld, F64, g)
        am = allmap.double().requires_grad_(True)
        depth = torch.nan_to_num(am[5:6], 0, 0)
        normal, _ = render_mod.depth_to_normal(cam, depth)
        pkg = {"render": torch.zeros(3, H, W, dtype=F64), "rend_dist": am[6:7],
               "rend_normal": (am[2:5].permute(1, 2, 0) @ wvt.double()[:3, :3].T).permute(2, 0, 1),
               "surf_normal": normal.permute(2, 0, 1) * am[1:2].detach()}
        loss = losses.training_loss(pkg, torch.zeros(3, H, W, dtype=F64), 0.2, ln, ld)     # (the image term of two zero images is 0)
        grad, = torch.autograd.grad(loss * g, am)
        assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        assert torch.equal(torch.isfinite(grad), torch.isfinite(r["grad"])) and bool(torch.isfinite(grad).all())
        for p in range(8):
            assert float((r["grad"][p] - grad[p]).abs().max()) <= 1e-12 * float(grad[p].abs().max()), p
        assert float(r["grad"][[0, 1, 7]].abs().max()) == 0.0


# ---- against the recorded golden ------------------------------------------------------------------------------------------------------
def test_reference_matches_recorded_golden():
    a, b = images()
    r = lr.photo_reference(a, b, 0.2, F64)
    assert abs(float(r["l1"]) - float(G["l1"])) <= 1e-7
    assert abs(float(r["ssim"]) - float(G["ssim"])) <= 2e-6
    assert abs(float(lr.photo_reference(a, a, 0.2, F64)["ssim"]) - float(G["ssim_self"])) <= 2e-6
    v = View()
    cam = SimpleNamespace(image_height=v.image_height, image_width=v.image_width, FoVx=v.FoVx, FoVy=v.FoVy, world_view_transform=v.world_view_transform)
    rd, ro = render_mod.camera_rays(cam, "cpu")
    depth = depth_map()
    H, W = depth.shape[1:]
    allmap = torch.zeros(8, H, W)
    allmap[1], allmap[5] = 1.0, depth[0]
    r = lr.reg_reference(allmap, rd, ro, v.world_view_transform, 1.0, 0.0, F64)
    assert np.abs(r["points"].numpy() - G["points"]).max() <= 2e-6 * np.abs(G["points"]).max()
    assert np.abs(r["surf_normal"].numpy() - G["normal"]).max() <= 2e-5


# ---- input conditions -----------------------------------------------------------------------------------------------------------------
def _allmap_cases():
    cases = [(H, W, k) for (H, W) in lr.REG_SHAPES for k in lr.ALLMAP_KINDS]
    cases += [(H, W, "edges") for (_, H, W) in lr.MERGED_SHAPES] + [(57, 109, "edges")]
    return sorted(set(cases))


@pytest.mark.parametrize("H,W,kind", _allmap_cases())
def test_allmap_inputs_take_one_branch_in_both_precisions(H, W, kind):
    """Conditions, not measurements: no comparison of the GPU file rests on a pixel where float32 and float64 disagree about the
    branch of F.normalize's clamp."""
    allmap = lr.make_allmap(kind, H, W)
    rd, ro, wvt = lr.make_camera(H, W)
    r64 = lr.reg_reference(allmap, rd, ro, wvt, 0.02, 1000.0, F64)
    r32 = lr.reg_reference(allmap, rd, ro, wvt, 0.02, 1000.0, torch.float32)
    v64, v32 = r64["vnorm"][r64["interior"]], r32["vnorm"][r32["interior"]]
    assert bool(((v64 == 0) | (v64 >= 1e-9)).all())
    assert torch.equal(v64 == 0, v32 == 0) and bool(((v32 == 0) | (v32 >= 1e-9)).all())
    assert bool(torch.isfinite(r64["grad"]).all()) and bool(torch.isfinite(r32["grad"]).all())
    reg = lr.allmap_regions(allmap, r64["vnorm"], r64["interior"])
    total = sum(m.long() for m in reg.values())
    assert bool((total == 1).all())                                    # a partition
    ordinary = reg["ordinary.inner"] | reg["ordinary.seam"]
    assert torch.equal(ordinary, lr.ordinary_mask(allmap, rd, ro, wvt))
    if kind == "plain":
        assert bool(ordinary.all())
    if H >= 13 and W >= 13:
        assert float(ordinary.float().mean()) >= 0.6
        if kind == "edges":
            assert bool((reg["rim.inner"] | reg["rim.seam"]).any())
            if H >= 17 and W >= 31:                                     # the block crosses a seam of both tilings
                assert bool(reg["ordinary.seam"].any()) and bool(reg["rim.seam"].any())
                assert bool((r64["vnorm"][13:16, 15:30] == 0).all())       # (the block's own corners keep a normal)
            assert bool((v64 == 0).any()) or H < 14                     # the zero-depth block is there
            # this is what the separation is for: the rim's depth gradient dwarfs an ordinary pixel's
            g5 = r64["grad"][5].abs()
            if bool((v64 == 0).any()):
                assert float(g5[~ordinary].max()) > 1e6 * float(g5[ordinary].median())


def _image_cases():
    cases = [(s, k) for s in lr.PHOTO_SHAPES for k in lr.IMAGE_KINDS] + [(s, "rand") for s in lr.MERGED_SHAPES] + [((3, 20, 40), "rand")]
    return sorted(set(cases))


@pytest.mark.parametrize("shape,kind", _image_cases())
def test_image_inputs_have_one_sign_in_both_precisions(shape, kind):
    img, gt = lr.make_images(kind, *shape)
    assert img.dtype == torch.float32 and gt.dtype == torch.float32
    d32, d64 = img - gt, img.double() - gt.double()
    assert torch.equal(torch.sign(d32).double(), torch.sign(d64))
    if kind == "equal":
        assert torch.equal(img, gt)
    if kind == "hdr" and img.numel() > 50:
        assert float(img.min()) < 0 and float(img.max()) > 1
    reg = lr.image_regions(*shape[1:])
    assert bool((sum(m.long() for m in reg.values()) == 1).all())
    if shape[1:] == (57, 109):
        assert all(bool(m.any()) for m in reg.values())


# ---- closed-form maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lr.IMAGE_KINDS)
def test_closed_form_maps_equal_autograd(kind):
    img, gt = lr.make_images(kind, 3, 29, 55)
    r = lr.photo_reference(img, gt, 0.2, F64)
    mu1, s11, s12, mu2, s22 = lr.ssim_terms(img, gt, F64)
    leaves = [t.detach().clone().requires_grad_(True) for t in (mu1, s11, s12)]      # what the adjoint of the three blurs needs
    m = lr.ssim_map_of(leaves[0], mu2, leaves[1] - leaves[0] * leaves[0], s22 - mu2 * mu2, leaves[2] - leaves[0] * mu2)
    assert _rel(m.detach(), r["map"]) <= 1e-12
    grads = torch.autograd.grad(m.sum(), leaves)
    scale = max(float(r[k].abs().max()) for k in ("dm_dmu1", "dm_ds11", "dm_ds12"))
    for k, gk in zip(("dm_dmu1", "dm_ds11", "dm_ds12"), grads):
        assert float((r[k] - gk).abs().max()) <= 1e-12 * scale, k
