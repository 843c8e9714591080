"""Plain-PyTorch reference of the training-loss kernels of csrc/loss_kernels.h (ssim_fwd_kernel / ssim_bwd_kernel, regloss_fwd_kernel /
regloss_bwd_kernel, regloss_fused_kernel, loss_fwd_merged_kernel, loss_combine_kernel), written from the formulas of
include/dgs_train_ops.h and dgs_amd/losses.py, at any floating-point precision: float64 is the reference of
tests/test_loss_fp64_gpu.py, float32 its yardstick (what a straight float32 evaluation of the same formulas loses against float64).
tests/test_loss_ref_cpu.py ties it to losses.ssim_torch / losses.training_loss / render.depth_to_normal and to the recorded golden.
The window is applied as two banded matrix products, so nothing here depends on a float64 convolution of the device's backend.
A helper module: no tests in here.  Run as a program it is the child process of the unit-gradient test (see unit_probe)."""
import math
import os
import sys

import torch

KR = 5                       # window radius
SSIM_TILE = (28, 54)         # (rows, columns) of an SSIM workgroup's output tile
FUSED_TILE = (14, 30)        # own pixels of a regloss_fused workgroup
PAIR_TILE = (16, 16)         # regloss_fwd_kernel / regloss_bwd_kernel
C1, C2 = 0.01 ** 2, 0.03 ** 2
IMAGE_KINDS = ("rand", "equal", "const", "smooth", "hdr")
ALLMAP_KINDS = ("plain", "edges")
# the cases of tests/test_loss_fp64_gpu.py (tests/test_loss_ref_cpu.py asserts the input conditions on every one of them)
PHOTO_SHAPES = ((1, 1, 1), (3, 1, 7), (1, 5, 5), (3, 6, 11), (3, 27, 53), (3, 28, 54), (3, 29, 55), (1, 28, 108), (3, 56, 54), (3, 57, 109),
                (3, 11, 1))
REG_SHAPES = ((1, 1), (2, 40), (3, 3), (13, 29), (14, 30), (15, 31), (16, 16), (17, 33), (28, 60), (29, 61), (43, 17))
# (C, H, W) -> photometric against regulariser workgroups of the merged grid: more, fewer, equally many
MERGED_SHAPES = {(3, 96, 144): (36, 35), (3, 61, 47): (9, 10), (3, 42, 45): (6, 6), (1, 57, 109): (9, 20), (3, 1, 1): (3, 1)}


# ---- window ---------------------------------------------------------------------------------------------------------------------
def gauss_window(dtype, device="cpu"):
    """The 11 weights as make_gauss() builds them: exp in double, cast to float, summed and divided in float; then cast to dtype."""
    g = [torch.tensor(math.exp(-float((i - KR) * (i - KR)) / (2.0 * 1.5 * 1.5)), dtype=torch.float64).to(torch.float32) for i in range(11)]
    s = torch.zeros((), dtype=torch.float32)
    for v in g:
        s = s + v
    return torch.stack([v / s for v in g]).to(device=device, dtype=dtype)


def toeplitz(n, w):
    """[n,n] band matrix of the zero-padded window: T[i, j] = w[j - i + 5] for |j - i| <= 5."""
    i = torch.arange(n, device=w.device)
    d = i[None, :] - i[:, None] + KR
    ok = (d >= 0) & (d <= 2 * KR)
    return torch.where(ok, w[d.clamp(0, 2 * KR)], torch.zeros((), dtype=w.dtype, device=w.device))


def blur(x, w):
    """x[..., H, W] -> Tv @ x @ Th.T"""
    return toeplitz(x.shape[-2], w) @ x @ toeplitz(x.shape[-1], w).T


# ---- photometric part -------------------------------------------------------------------------------------------------------------
def ssim_map_of(mu1, mu2, sigma1_sq, sigma2_sq, sigma12):
    return ((2 * mu1 * mu2 + C1) * (2 * sigma12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (sigma1_sq + sigma2_sq + C2))


def photo_reference(img, gt, lam, dtype, g=1.0):
    """(1 - lam) * mean|img - gt| + lam * (1 - mean SSIM map) at precision `dtype`, on the device of img.  img, gt: float32 [C,H,W].
    -> dict of detached tensors:
       loss, l1, ssim (scalars);  loss_scale: the largest absolute term of the sum the loss is, max(|loss|, |1 - lam| l1, |lam|,
       |lam ssim|) -- with img == gt, lam * (1 - ssim) cancels to 1e-17 in float64 and no float32 evaluation is closer to it than a
       rounding of the 1;  grad = g * dloss/dimg (autograd);  grad_scale: the same adjoint expression with every term replaced
       by its absolute value -- |g| * (|lam| / n * (blur|dm_dmu1| + 2 |img| blur|dm_ds11| + |gt| blur|dm_ds12|) + |1 - lam| / n);
       map, dm_dmu1, dm_ds11, dm_ds12: the SSIM map and its three derivative maps in the closed form ssim_fwd_body stores;
       ssim_grad, ssim_grad_scale: d mean(map) / dimg and its scale (fused_ssim's backward, upstream gradient 1)."""
    a = img.detach().to(dtype).clone().requires_grad_(True)
    b = gt.detach().to(dtype)
    w = gauss_window(dtype, a.device)
    n = a.numel()
    mu1, mu2, s11, s22, s12 = blur(a, w), blur(b, w), blur(a * a, w), blur(b * b, w), blur(a * b, w)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sg1, sg2, sg12 = s11 - mu1_sq, s22 - mu2_sq, s12 - mu12
    A, B, Cc, D = 2 * mu12 + C1, 2 * sg12 + C2, mu1_sq + mu2_sq + C1, sg1 + sg2 + C2
    inv_cd = 1.0 / (Cc * D)
    m = A * B * inv_cd
    ssim = m.mean()
    l1 = (a - b).abs().mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    grad, = torch.autograd.grad(loss * g, a, retain_graph=True)
    ssim_grad, = torch.autograd.grad(ssim, a)
    with torch.no_grad():
        dm_dmu1 = (2 * mu2 * B - 2 * mu2 * A) * inv_cd - m * (2 * mu1 / Cc - 2 * mu1 / D)
        dm_ds11 = -m / D
        dm_ds12 = 2 * A * inv_cd
        adj = (blur(dm_dmu1.abs(), w) + 2 * a.abs() * blur(dm_ds11.abs(), w) + b.abs() * blur(dm_ds12.abs(), w)) / n
        grad_scale = abs(g) * (abs(lam) * adj + abs(1.0 - lam) / n)
    loss_scale = torch.stack([loss.abs(), abs(1.0 - lam) * l1, abs(lam) * torch.ones_like(l1), abs(lam) * ssim.abs()]).max()
    out = dict(loss=loss, l1=l1, ssim=ssim, loss_scale=loss_scale, grad=grad, grad_scale=grad_scale, map=m, dm_dmu1=dm_dmu1, dm_ds11=dm_ds11, dm_ds12=dm_ds12,
               ssim_grad=ssim_grad, ssim_grad_scale=adj)
    return {k: v.detach() for k, v in out.items()}


def ssim_terms(img, gt, dtype):
    """The five blurs (mu1, s11, s12, mu2, s22) = blur(img, img^2, img gt, gt, gt^2): the kernel's dm_dmu1 / dm_dsigma1_sq / dm_dsigma12
    are the map's derivatives with respect to the first three (sigma1_sq = s11 - mu1^2 and sigma12 = s12 - mu1 mu2 depend on mu1:
    dm_dmu1 includes that path, and d/ds11 = d/dsigma1_sq, d/ds12 = d/dsigma12)."""
    a, b = img.to(dtype), gt.to(dtype)
    w = gauss_window(dtype, a.device)
    return blur(a, w), blur(a * a, w), blur(a * b, w), blur(b, w), blur(b * b, w)


# ---- regularisers -----------------------------------------------------------------------------------------------------------------
def reg_reference(allmap, rays_d, rays_o, wvt, ln, ld, dtype, g=1.0):
    """ln * mean(1 - <rend_normal_world, surf_normal>) + ld * mean(plane 6) of an allmap[8,H,W] at precision `dtype`.
    Non-finite depth -> 0 (NaN and +inf; -inf would be the lowest finite number, which overflows the float32 products).
    -> dict: loss, normal (mean(1 - dot)), dist (mean of plane 6), grad [8,H,W] = g * dloss/dallmap (planes 0, 1, 7 exactly zero),
       vnorm [H,W]: |dx x dy| of the interior pixels (0 elsewhere), interior [H,W] bool, points [H,W,3], surf_normal [H,W,3] (before
       the multiplication by alpha)."""
    am = allmap.detach().to(dtype).clone().requires_grad_(True)
    H, W = am.shape[1:]
    rd, ro, wv = rays_d.detach().to(dtype), rays_o.detach().to(dtype), wvt.detach().to(dtype)
    raw = am[5]
    depth = torch.where(torch.isfinite(raw), raw, torch.zeros((), dtype=dtype, device=am.device))
    points = (depth.reshape(-1, 1) * rd + ro).reshape(H, W, 3)
    surf = torch.zeros_like(points)
    vnorm = torch.zeros((H, W), dtype=dtype, device=am.device)
    interior = torch.zeros((H, W), dtype=torch.bool, device=am.device)
    if H >= 3 and W >= 3:
        dx = points[2:, 1:-1] - points[:-2, 1:-1]
        dy = points[1:-1, 2:] - points[1:-1, :-2]
        v = torch.cross(dx, dy, dim=-1)
        L = torch.linalg.vector_norm(v, dim=-1, keepdim=True)      # (its backward is 0 at v = 0, and the clamp cuts it there anyway)
        inner = v / L.clamp_min(1e-12)
        surf = torch.nn.functional.pad(inner, (0, 0, 1, 1, 1, 1))
        vnorm[1:-1, 1:-1] = L[..., 0].detach()
        interior[1:-1, 1:-1] = True
    surf_normal = surf.detach()
    surf = surf.permute(2, 0, 1) * am[1].detach()
    rend = (am[2:5].permute(1, 2, 0) @ wv[:3, :3].T).permute(2, 0, 1)
    normal = (1.0 - (rend * surf).sum(0)).mean()
    dist = am[6].mean()
    loss = ln * normal + ld * dist
    grad, = torch.autograd.grad(loss * g, am)
    return dict(loss=loss.detach(), normal=normal.detach(), dist=dist.detach(), grad=grad.detach(), vnorm=vnorm, interior=interior,
                points=points.detach(), surf_normal=surf_normal)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def make_images(kind, C, H, W, seed=0):
    """(img, gt): float32 CPU tensors [C,H,W]."""
    gen = torch.Generator().manual_seed(2000 + seed)
    if kind == "rand":
        gt = torch.rand(C, H, W, generator=gen)
        img = 0.6 * torch.rand(C, H, W, generator=gen) + 0.4 * gt
    elif kind == "equal":
        gt = torch.rand(C, H, W, generator=gen)
        img = gt.clone()
    elif kind == "const":
        img, gt = torch.full((C, H, W), 0.75), torch.full((C, H, W), 0.25)
    elif kind == "smooth":
        y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
        c = torch.arange(C, dtype=torch.float64)[:, None, None]
        img = 0.5 + 0.3 * torch.sin(0.21 * x + 0.13 * y + c) + 1e-3 * torch.randn(C, H, W, generator=gen).double()
        gt = 0.5 + 0.3 * torch.sin(0.19 * x + 0.16 * y + 0.4 + c) + 1e-3 * torch.randn(C, H, W, generator=gen).double()
    elif kind == "hdr":
        img = 4.0 * torch.rand(C, H, W, generator=gen) - 1.0
        gt = 4.0 * torch.rand(C, H, W, generator=gen) - 1.0
    else:
        raise ValueError(kind)
    return img.float().contiguous(), gt.float().contiguous()


def make_allmap(kind, H, W, seed=0):
    """float32 CPU allmap[8,H,W]: alpha in [0.2, 1], unit view-space normals, depth in [2, 3], distortion <= 1e-3 (the order the
    rasterizer produces: neither regulariser drowns the other at lambda_normal = 0.02, lambda_dist = 1000).
    kind "edges" adds, clipped to the image: a zero-depth block over rows 12..16 and columns 14..30 (it spans the seams at row 14 /
    column 30 of the 30 x 14 tiling and at 16 of the 16 x 16 one), NaN at (5, 7) and (0, 0), +inf at (9, 3) and (H-1, W-1), and a
    patch of alpha = 0."""
    gen = torch.Generator().manual_seed(3000 + seed)
    am = torch.rand(8, H, W, generator=gen)
    am[1] = 0.2 + 0.8 * am[1]
    am[2:5] = torch.nn.functional.normalize(torch.randn(3, H, W, generator=gen), dim=0)
    am[5] += 2.0
    am[6] *= 1e-3
    if kind == "edges":
        am[5, 12:17, 14:31] = 0.0
        for (y, x, v) in ((5, 7, float("nan")), (9, 3, float("inf")), (0, 0, float("nan")), (H - 1, W - 1, float("inf"))):
            if y < H and x < W:
                am[5, y, x] = v
        am[1, H // 2: H // 2 + 4, W // 2: W // 2 + 5] = 0.0
    elif kind != "plain":
        raise ValueError(kind)
    return am.contiguous()


def make_camera(H, W, device="cpu"):
    """(rays_d [H*W,3], rays_o [3], wvt [4,4]) of the first camera of an orbit: wvt[:3,:3] is a real rotation."""
    from dgs_amd.cameras import orbit_cameras
    from dgs_amd.render import camera_rays
    cam = orbit_cameras(1, W, H)[0]
    rays_d, rays_o = camera_rays(cam, "cpu")
    return rays_d.float().contiguous().to(device), rays_o.float().contiguous().to(device), cam.world_view_transform.float().contiguous().to(device)


# ---- regions ----------------------------------------------------------------------------------------------------------------------
def _near_multiples(n, step, r, device):
    """[n] bool: within r pixels of a tile boundary (the boundary lies between step * k - 1 and step * k, k >= 1)."""
    i = torch.arange(n, device=device)
    out = torch.zeros(n, dtype=torch.bool, device=device)
    for b in range(step, n, step):
        out |= (i >= b - r) & (i < b + r)
    return out


def image_regions(H, W, device="cpu"):
    """{"border", "seam", "interior"}: [H,W] bool, a partition.  border: within 5 px of the image edge; seam: within 5 px of a multiple
    of 54 in x or of 28 in y, and not border."""
    y, x = torch.arange(H, device=device)[:, None], torch.arange(W, device=device)[None, :]
    border = (y < KR) | (y >= H - KR) | (x < KR) | (x >= W - KR)
    seam = (_near_multiples(H, SSIM_TILE[0], KR, device)[:, None] | _near_multiples(W, SSIM_TILE[1], KR, device)[None, :]) & ~border
    return {"border": border.expand(H, W).clone(), "seam": seam, "interior": ~border & ~seam}


def allmap_regions(allmap, vnorm, interior):
    """{"ordinary.inner", "ordinary.seam", "rim.inner", "rim.seam"}: [H,W] bool, a partition.  rim: a degenerate (interior, |v| <
    1e-12) or non-finite-depth pixel within 2 px; seam: within 2 px of a multiple of 30 / 14 (fused tiling) or of 16 (pair tiling)."""
    H, W = allmap.shape[1:]
    dev = allmap.device
    bad = (interior & (vnorm < 1e-12)) | ~torch.isfinite(allmap[5])
    rim = torch.nn.functional.max_pool2d(bad[None, None].float(), 5, stride=1, padding=2)[0, 0] > 0
    sy = _near_multiples(H, FUSED_TILE[0], 2, dev) | _near_multiples(H, PAIR_TILE[0], 2, dev)
    sx = _near_multiples(W, FUSED_TILE[1], 2, dev) | _near_multiples(W, PAIR_TILE[1], 2, dev)
    seam = (sy[:, None] | sx[None, :]).expand(H, W)
    return {"ordinary.inner": ~rim & ~seam, "ordinary.seam": ~rim & seam, "rim.inner": rim & ~seam, "rim.seam": rim & seam}


def ordinary_mask(allmap, rays_d, rays_o, wvt):
    """[H,W] bool: no degenerate or non-finite pixel within 2 px (float64 evaluation)."""
    r = reg_reference(allmap, rays_d, rays_o, wvt, 1.0, 0.0, torch.float64)
    reg = allmap_regions(allmap, r["vnorm"], r["interior"])
    return reg["ordinary.inner"] | reg["ordinary.seam"]


# ---- child process of test_unit_gradient_end_to_end ---------------------------------------------------------------------------------
def unit_probe(path, C, H, W):
    """fused_train_loss(unit_grad=True) on the (C, H, W) rand / edges case under this process's DGS_MERGED_LOSS_FORWARD; saves
    (loss, dL/dimage, dL/dallmap) to `path`."""
    from dgs_amd import _ops
    img, gt = (t.cuda() for t in make_images("rand", C, H, W))
    allmap = make_allmap("edges", H, W).cuda()
    rd, ro, wvt = make_camera(H, W, "cuda")
    image, am = img.clone().requires_grad_(True), allmap.clone().requires_grad_(True)
    loss = _ops.fused_train_loss(image, am, gt, rd, ro, wvt, 0.2, 0.02, 1000.0, unit_grad=True)
    loss.backward(torch.ones((), device="cuda"))
    torch.cuda.synchronize()
    torch.save({"merged": bool(_ops._MERGED_LOSS_FORWARD), "loss": loss.detach().cpu(), "g_image": image.grad.cpu(), "g_allmap": am.grad.cpu()}, path)


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (root, os.path.join(root, "dynamic-2dgs_amd"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    unit_probe(sys.argv[1], *[int(v) for v in sys.argv[2:5]])
