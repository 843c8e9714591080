"""Images of the extracted meshes: what the reference's render_mesh.py:221-240 does after it has written frame_<i>.ply -- draw mesh i
with its vertex colours from test camera i on a white background (mesh_image/), draw a shaded "shape" image (mesh_shape/) -- and
what metrics_mesh.py then does with mesh_image/: PSNR, SSIM, MS-SSIM against the ground-truth test images.  The reference draws with
nvdiffrast and PyTorch3D; this module has its own z-buffer rasterizer, stated once in include/dgs_mesh_ops.h (VERTEX, FACE, PIXEL,
ATTRIBUTES, THE TABLE) and twice implemented:

  raster_table      per-face rows of that header from (vertices, faces, camera): elementwise PyTorch, any dtype, any device
  rasterize_torch   the PyTorch statement of the coverage / depth test, faces chunked against all pixels: the CPU path, the
                    comparator of the GPU tests and the baseline of tools/mesh_render_timing.py
  rasterize         HIP tensors: dgs_mesh_raster + dgs_mesh_resolve of libdgs_mesh_ops.so, bit-identical to the statement in fp32;
                    CPU tensors: the statement.  On a HIP device a missing library is an error, never a reason to run the statement.
  interpolate       perspective-correct per-pixel attributes of the winning faces
  vertex_normals    area-weighted vertex normals, summed on the host in float64 (deterministic)
  render_mesh       colour image on a background, alpha, depth, face ids; supersample = k averages k x k samples per pixel
  render_mesh_shape white material under one directional light (Phong)
  render_meshes     frame_<i>.ply of a directory from the test cameras of a D-NeRF dataset -> mesh_image/, mesh_shape/,
                    mesh_render_results.json, mesh_render_per_view.json

Departures from the reference, all stated: no clipping at the near plane (a face with a corner at w <= near is dropped; the
protocol's meshes lie in front of the camera), no nvdiffrast edge antialiasing (supersample is the stand-in), no LPIPS (the
networks' weights are not available), not differentiable, and no image flips: everything is drawn in the surfel rasterizer's pixel
convention, the one the ground-truth images of load_dnerf are in.

Shell form:  python -m dgs_amd.mesh_render MESH_DIR DATA [--out-dir DIR] [--supersample k] [--float] [--black-background] [--device cuda:0]
"""
import json
import math
import os
import re

import numpy as np
import torch

ROW, VALUES = 24, 19          # floats of a table row (= dgs_mesh_raster_layout()[2]); 0..18 are floats, 19 padding, 20..23 the int32 box
_PAIR_BUDGET = 1 << 22        # elements of one [chunk, pixels] intermediate of rasterize_torch
_GROUP = 4096                 # faces that share one window of the image in rasterize_torch


# ---- the table ------------------------------------------------------------------------------------------------------------------
def project_vertices(vertices, camera):
    """(sx, sy, w, iw) [Nv] each, in the dtype of `vertices`: VERTEX of include/dgs_mesh_ops.h."""
    v = vertices.detach().reshape(-1, 3)
    m = camera.full_proj_transform.to(device=v.device, dtype=v.dtype)
    H, W = int(camera.image_height), int(camera.image_width)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    hom = lambda c: x * m[0, c] + ((y * m[1, c] + z * m[2, c]) + m[3, c])
    h0, h1, w = hom(0), hom(1), hom(3)
    sx = ((h0 / w + 1) * W - 1) / 2          # / 2 is exact however it is evaluated
    sy = ((h1 / w + 1) * H - 1) / 2
    return sx, sy, w, torch.ones_like(w) / w


@torch.no_grad()
def raster_table(vertices, faces, camera, near=0.01):
    """(table [Nf, ROW] in the dtype and on the device of `vertices`, box [Nf,4] int32 = x0, x1, y0, y1): the rows of THE TABLE of
    include/dgs_mesh_ops.h, elementwise operations only, every one rounded on its own.  In an fp32 table columns 20..23 hold the
    bits of `box` (what the kernels read); in any other dtype they are zero and `box` alone carries it.  A dropped face (a corner
    with w <= near, a non-finite screen coordinate, A == 0) has sign-of-A 0 and, like a face whose box misses the image, the
    empty box (0, -1, 0, -1)."""
    if not float(near) > 0.0:
        raise ValueError("raster_table: near must be positive")
    H, W = int(camera.image_height), int(camera.image_width)
    sx, sy, w, iw = project_vertices(vertices, camera)
    f = faces.detach().reshape(-1, 3).long().to(sx.device)
    X, Y = [sx[f[:, k]] for k in range(3)], [sy[f[:, k]] for k in range(3)]
    Wc, IW = [w[f[:, k]] for k in range(3)], [iw[f[:, k]] for k in range(3)]
    one = torch.ones_like(X[0])
    cols, sign = [], []
    for k in range(3):
        px, py, qx, qy = X[(k + 1) % 3], Y[(k + 1) % 3], X[(k + 2) % 3], Y[(k + 2) % 3]
        swap = (qx < px) | ((qx == px) & (qy < py))
        xa, ya, xb, yb = torch.where(swap, qx, px), torch.where(swap, qy, py), torch.where(swap, px, qx), torch.where(swap, py, qy)
        cols += [xa, ya, xb - xa, yb - ya]
        sign.append(torch.where(swap, -one, one))
    A = sign[0] * (cols[2] * (Y[0] - cols[1]) - cols[3] * (X[0] - cols[0]))
    finite = torch.isfinite(torch.stack(X + Y)).all(0)
    valid = (Wc[0] > near) & (Wc[1] > near) & (Wc[2] > near) & finite & ((A > 0) | (A < 0))
    sa = torch.where(valid, torch.where(A > 0, one, -one), torch.zeros_like(one))
    lo = lambda c, top: torch.where(valid, torch.ceil(torch.minimum(torch.minimum(c[0], c[1]), c[2])).clamp(0, top), one).to(torch.int32)
    hi = lambda c, top: torch.where(valid, torch.floor(torch.maximum(torch.maximum(c[0], c[1]), c[2])).clamp(-1, top - 1), -one).to(torch.int32)
    x0, x1, y0, y1 = lo(X, W), hi(X, W), lo(Y, H), hi(Y, H)
    empty = ~valid | (x0 > x1) | (y0 > y1)
    box = torch.stack([x0, x1, y0, y1], 1)
    box = torch.where(empty[:, None], torch.tensor([0, -1, 0, -1], dtype=torch.int32, device=box.device), box).contiguous()
    zero = torch.zeros_like(one)
    table = torch.stack(cols + sign + [sa] + IW + [zero] * (ROW - VALUES), 1).contiguous()
    if table.dtype == torch.float32:
        table.view(torch.int32)[:, 20:24] = box
    return table, box


# ---- the PyTorch statement ------------------------------------------------------------------------------------------------------
def _pair(col, px, py):
    """FACE of the header for broadcastable (rows, pixels): col[i] = table column i, px / py = pixel centres.
    -> (inside [all three e_k on A's side, S != 0 and q > 0], (b_0, b_1, b_2), z)."""
    e = [col[12 + k] * (col[4 * k + 2] * (py - col[4 * k + 1]) - col[4 * k + 3] * (px - col[4 * k])) for k in range(3)]
    pos = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
    neg = (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)
    S = (e[0] + e[1]) + e[2]
    b = [e[k] / S for k in range(3)]
    q = (b[0] * col[16] + b[1] * col[17]) + b[2] * col[18]
    inside = (((col[15] > 0) & pos) | ((col[15] < 0) & neg)) & (S != 0) & (q > 0)
    one = torch.ones((1,) * q.dim(), dtype=q.dtype, device=q.device)      # a tensor / tensor division: the IEEE one on every device
    return inside, b, one / q


def _pixels(H, W, device, dtype):
    iy, ix = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
    ix, iy = ix.reshape(-1), iy.reshape(-1)
    return ix, iy, ix.to(dtype), iy.to(dtype)


@torch.no_grad()
def rasterize_torch(table, box, H, W, chunk=None):
    """PIXEL of the header in PyTorch, in the dtype and on the device of `table`: groups of faces against all pixels of the window
    that holds the group's boxes (one host read per group; chunked further so that an intermediate stays within _PAIR_BUDGET
    elements, or to `chunk` faces), the minimum depth over the covering faces and, among equal depths, the lowest face -- written out, not left to what torch.min
    returns.  -> (face_id [H,W] int32, -1 = nothing; depth [H,W], 0 there; bary [H,W,3], 0 there), depth and bary recomputed for
    the winner by the same expressions."""
    nf, P = table.shape[0], H * W
    dev, dt = table.device, table.dtype
    ix, iy, px, py = _pixels(H, W, dev, dt)
    zbest = torch.full((P,), float("inf"), dtype=dt, device=dev)
    fbest = torch.full((P,), -1, dtype=torch.int64, device=dev)
    index = torch.arange(nf, dtype=torch.int64, device=dev)
    keep = torch.nonzero(box[:, 1] >= box[:, 0]).reshape(-1)                # faces with an empty box never enter a list
    for g in range(0, keep.numel(), _GROUP):
        group = keep[g:g + _GROUP]
        gb = box[group].long()
        # no pixel outside the union of the group's boxes can be covered by it: only that window of the image is evaluated
        ux0, ux1, uy0, uy1 = torch.stack([gb[:, 0].min(), gb[:, 1].max(), gb[:, 2].min(), gb[:, 3].max()]).tolist()
        sel = ((iy >= uy0) & (iy <= uy1) & (ix >= ux0) & (ix <= ux1)).nonzero().reshape(-1)
        sx, sy, spx, spy = ix[sel][None], iy[sel][None], px[sel][None], py[sel][None]
        step = max(1, _PAIR_BUDGET // sel.numel()) if chunk is None else chunk
        for s in range(0, group.numel(), step):
            ids, bx = group[s:s + step], gb[s:s + step]
            col = table[ids, :VALUES].t().contiguous().unsqueeze(2)         # [19, F, 1]: col[i] broadcasts against [1, pixels]
            inbox = (sx >= bx[:, 0:1]) & (sx <= bx[:, 1:2]) & (sy >= bx[:, 2:3]) & (sy <= bx[:, 3:4])
            inside, _, z = _pair(col, spx, spy)
            cov = inbox & inside
            zc = torch.where(cov, z, torch.full_like(z, float("inf")))
            m = zc.min(dim=0).values
            who = torch.where(cov & (zc == m[None]), index[ids][:, None], nf).min(dim=0).values
            better = (who < nf) & (m < zbest[sel])                          # strict: an earlier chunk holds the lower faces
            zbest[sel], fbest[sel] = torch.where(better, m, zbest[sel]), torch.where(better, who, fbest[sel])
    hit = fbest >= 0
    depth, bary = torch.zeros(P, dtype=dt, device=dev), torch.zeros((P, 3), dtype=dt, device=dev)
    if nf:
        col = table[fbest.clamp(min=0), :VALUES].t()
        _, b, z = _pair(col, px, py)
        depth = torch.where(hit, z, depth)
        bary = torch.where(hit[:, None], torch.stack(b, 1), bary)
    return fbest.to(torch.int32).reshape(H, W), depth.reshape(H, W), bary.reshape(H, W, 3)


@torch.no_grad()
def interpolate(attr, faces, table, face_id, bary, depth, background=None):
    """ATTRIBUTES of the header: [C,H,W] from attr [Nv,C] for the winners (face_id, bary, depth) of a rasterization of `table`;
    background [C] (default zeros) where face_id < 0."""
    H, W = face_id.shape
    dt, dev = bary.dtype, bary.device
    attr = attr.to(device=dev, dtype=dt)
    C = attr.shape[1]
    bg = torch.zeros(C, dtype=dt, device=dev) if background is None else background.to(device=dev, dtype=dt).reshape(C)
    if faces.shape[0] == 0:
        return bg[:, None, None].expand(C, H, W).contiguous()
    fid = face_id.reshape(-1).long().clamp(min=0)
    corner = faces.detach().reshape(-1, 3).long().to(dev)[fid]
    b, z = bary.reshape(-1, 3), depth.reshape(-1, 1)
    w = [(b[:, k] * table[fid, 16 + k].to(dt))[:, None] for k in range(3)]
    a = ((w[0] * attr[corner[:, 0]] + w[1] * attr[corner[:, 1]]) + w[2] * attr[corner[:, 2]]) * z
    out = torch.where((face_id.reshape(-1) >= 0)[:, None], a, bg[None])
    return out.t().reshape(C, H, W).contiguous()


def _check_mesh(vertices, faces, who):
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_floating_point():
        raise ValueError("%s: vertices must be a floating-point tensor [Nv,3]" % who)
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError("%s: faces must be an integer tensor [Nf,3]" % who)
    if faces.device != vertices.device:
        raise ValueError("%s: vertices and faces live on different devices" % who)
    if not bool(torch.isfinite(vertices).all()):
        raise ValueError("%s: vertices holds non-finite coordinates" % who)
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= vertices.shape[0]):
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (who, vertices.shape[0]))
    if faces.shape[0] >= 2 ** 31:
        raise ValueError("%s: %d faces do not fit the 31-bit face index" % (who, faces.shape[0]))


@torch.no_grad()
def rasterize(vertices, faces, camera, attr=None, background=None, near=0.01, best=None):
    """Draw the mesh from the camera -> {"face" [H,W] int32 (-1 = nothing), "depth" [H,W] (view depth, 0 = nothing), "bary"
    [H,W,3], "image" [C,H,W] (the interpolated attr [Nv,C] on background [C]; None without attr), "table"}.
    HIP tensors (fp32): the kernels; `best` may name an int64 [H*W] buffer to reuse (it is fully re-initialised).  CPU tensors:
    rasterize_torch + interpolate in the dtype of `vertices`.  Zero faces are legal and give an empty image."""
    _check_mesh(vertices, faces, "rasterize")
    H, W = int(camera.image_height), int(camera.image_width)
    if H < 1 or W < 1:
        raise ValueError("rasterize: the image must be at least 1 x 1")
    dev = vertices.device
    if attr is not None:
        if attr.dim() != 2 or attr.shape[0] != vertices.shape[0] or attr.shape[1] < 1:
            raise ValueError("rasterize: attr must be [Nv,C] with C >= 1")
        if background is None:
            background = torch.zeros(attr.shape[1])
    if dev.type == "cpu":
        table, box = raster_table(vertices, faces, camera, near)
        face, depth, bary = rasterize_torch(table, box, H, W)
        image = None if attr is None else interpolate(attr, faces, table, face, bary, depth, background)
        return {"face": face, "depth": depth, "bary": bary, "image": image, "table": table}
    from . import _mesh_ops
    table, box = raster_table(vertices.float(), faces, camera, near)
    if attr is not None:
        if attr.shape[1] > _mesh_ops.raster_layout()[3]:
            raise ValueError("rasterize: at most %d attribute channels per call" % _mesh_ops.raster_layout()[3])
        attr = attr.to(device=dev, dtype=torch.float32).contiguous()
        background = background.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    best = _mesh_ops.raster(table, box, H, W, best)
    face, depth, bary, image = _mesh_ops.resolve(best, table, faces.to(torch.int32).contiguous(), H, W, attr, background)
    return {"face": face, "depth": depth, "bary": bary, "image": image, "table": table}


# ---- shading --------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def vertex_normals(vertices, faces):
    """[Nv,3] float32 on the device of `vertices`: the normalised sum of the face normals cross(B - A, C - A) (twice the area as
    weight) over the faces at each vertex; zero for a vertex no face with area touches.  Deterministic: the sums are taken ON THE
    HOST, in float64, one np.bincount per component (a sequential loop in face order) -- no float atomics anywhere."""
    v = vertices.detach().cpu().double().numpy().reshape(-1, 3)
    f = faces.detach().cpu().long().numpy().reshape(-1, 3)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    idx = f.reshape(-1)
    acc = np.stack([np.bincount(idx, weights=np.repeat(n[:, c], 3), minlength=v.shape[0]) for c in range(3)], 1)
    norm = np.linalg.norm(acc, axis=1, keepdims=True)
    out = np.divide(acc, norm, out=np.zeros_like(acc), where=norm > 0)
    return torch.from_numpy(out.astype(np.float32)).to(vertices.device)


def _scaled(camera, k):
    return camera if k == 1 else camera._replace(image_height=int(camera.image_height) * k, image_width=int(camera.image_width) * k)


def _block_mean(x, k):
    """[C, kH, kW] -> [C, H, W]: the mean of every k x k block."""
    C, Hk, Wk = x.shape
    return x.reshape(C, Hk // k, k, Wk // k, k).mean(dim=(2, 4))


def _supersample(k):
    k = int(k)
    if k < 1:
        raise ValueError("supersample must be >= 1")
    return k


@torch.no_grad()
def render_mesh(camera, vertices, faces, colors, white_background=True, supersample=1, near=0.01):
    """The mesh with its vertex colours [Nv,3] from the camera -> {"render" [3,H,W] on white (or black), "alpha" [1,H,W] (share of
    the pixel's samples that hit the mesh), "depth" [1,H,W] (view depth, mean over the samples that hit; 0 = nothing), "face" [H,W]
    int32 (the face at the first sample of the pixel; -1 = nothing)}.  supersample = k draws k H x k W and averages k x k blocks:
    the stand-in for nvdiffrast's edge antialiasing, which is not restated."""
    k = _supersample(supersample)
    bg = torch.full((3,), 1.0 if white_background else 0.0)
    out = rasterize(vertices, faces, _scaled(camera, k), attr=colors, background=bg, near=near)
    hit = (out["face"] >= 0).to(out["image"].dtype)[None]
    depth, face = out["depth"][None], out["face"]
    if k == 1:
        return {"render": out["image"], "alpha": hit, "depth": depth, "face": face}
    alpha = _block_mean(hit, k)
    depth = torch.where(alpha > 0, _block_mean(depth, k) / alpha.clamp_min(1.0 / (k * k)), torch.zeros_like(alpha))
    return {"render": _block_mean(out["image"], k), "alpha": alpha, "depth": depth, "face": face[::k, ::k].contiguous()}


@torch.no_grad()
def render_mesh_shape(camera, vertices, faces, supersample=1, near=0.01):
    """[3,H,W]: the mesh as a white material under one directional light, on a white background -- the role of the reference's
    mesh_renderer/__init__.py:139-225.  With n the interpolated, renormalised vertex normal, l the unit vector from the mesh's vertex
    mean towards the camera centre, v the unit vector from the surface point towards the camera centre and r = 2 (n.l) n - l:
        colour = 0.5 + 0.3 * max(n.l, 0) + 0.2 * 0.2 * max(r.v, 0)^10
    -- PyTorch3D's default ambient (0.5) and diffuse (0.3) light colours, its default specular light colour 0.2 times the
    reference's specular material 0.2, shininess 10.  PyTorch3D is not installed where this package is built and tested, so the
    line above -- not a run of that library -- is the contract.  No image flips: the rasterizer's own convention."""
    k = _supersample(supersample)
    if vertices.shape[0] == 0 or faces.shape[0] == 0:
        return torch.ones((3, int(camera.image_height), int(camera.image_width)), dtype=torch.float32, device=vertices.device)
    dt, dev = vertices.dtype, vertices.device
    attr = torch.cat([vertex_normals(vertices, faces).to(dt), vertices.detach()], 1)
    out = rasterize(vertices, faces, _scaled(camera, k), attr=attr, background=torch.zeros(6), near=near)
    n, pos = out["image"][:3], out["image"][3:]
    n = n / n.norm(dim=0, keepdim=True).clamp_min(1e-12)
    centre = camera.camera_center.to(device=dev, dtype=n.dtype)
    l = centre - vertices.detach().to(n.dtype).mean(0)
    l = (l / l.norm().clamp_min(1e-12))[:, None, None]
    v = centre[:, None, None] - pos
    v = v / v.norm(dim=0, keepdim=True).clamp_min(1e-12)
    nl = (n * l).sum(0, keepdim=True)
    rv = ((2 * nl * n - l) * v).sum(0, keepdim=True)
    shade = 0.5 + 0.3 * nl.clamp_min(0) + 0.2 * 0.2 * rv.clamp_min(0) ** 10
    img = torch.where((out["face"] >= 0)[None], shade, torch.ones_like(shade)).expand(3, -1, -1)
    return _block_mean(img, k).contiguous() if k > 1 else img.contiguous()


# ---- the product step -----------------------------------------------------------------------------------------------------------
def _default_out_dir(mesh_dir):
    """<model> for <model>/train/ours_<it>, else mesh_dir."""
    d = os.path.abspath(mesh_dir)
    if re.fullmatch(r"ours_\d+", os.path.basename(d)) and os.path.basename(os.path.dirname(d)) == "train":
        return os.path.dirname(os.path.dirname(d))
    return mesh_dir


def render_meshes(mesh_dir, data_path, out_dir=None, white_background=True, device="cuda:0", supersample=1, quantize=True, log=None):
    """render_mesh.py:221-240 + metrics_mesh.py: frame_<i>.ply of mesh_dir (i = 0 .. n-1, as evaluate_meshes pairs them) drawn from
    test camera i of load_dnerf(data_path, white_background=True) ->
      <out>/mesh_image/%05d.png   the mesh with its vertex colours on a white (white_background=False: black) background
      <out>/mesh_shape/%05d.png   render_mesh_shape
      <out>/mesh_render_results.json   {"PSNR", "SSIM", "MS-SSIM"}: means over the frames of mesh_image against the test images
      <out>/mesh_render_per_view.json  {"PSNR": {file name: value}, ...}
    (NaN as null: MS-SSIM below 161 pixels a side).  quantize=True scores the images as the 8-bit files hold them, False the float
    renders.  out_dir defaults to the model directory when mesh_dir is <model>/train/ours_<it>, else to mesh_dir.  A different
    number of frames and test cameras is an error.  Returns {"results": ..., "per_view": ...} as written."""
    from . import io as dio
    from .evaluate import image_metrics, save_png
    device = torch.device(device)
    frames = {}
    for name in os.listdir(mesh_dir):
        m = re.fullmatch(r"frame_(\d+)\.ply", name)
        if m:
            frames[int(m.group(1))] = name
    if not frames:
        raise ValueError("render_meshes: no frame_<i>.ply in %s" % mesh_dir)
    test = dio.load_dnerf(data_path, white_background=True)["test"]
    if len(frames) != len(test) or sorted(frames) != list(range(len(frames))):
        raise ValueError("render_meshes: %d frame_<i>.ply files in %s (i = %s) but %d test cameras in %s"
                         % (len(frames), mesh_dir, sorted(frames)[:3] + (["..."] if len(frames) > 3 else []), len(test), data_path))
    out_dir = out_dir or _default_out_dir(mesh_dir)
    dirs = {k: os.path.join(out_dir, k) for k in ("mesh_image", "mesh_shape")}
    for p in dirs.values():
        os.makedirs(p, exist_ok=True)
    per_view = {"SSIM": {}, "PSNR": {}, "MS-SSIM": {}}
    for i, fr in enumerate(test):
        v, f, c = dio.read_mesh_ply(os.path.join(mesh_dir, frames[i]))
        if c is None:
            raise ValueError("render_meshes: %s has no vertex colours" % frames[i])
        v, f, c = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(c).to(device)
        cam = fr.camera.to(device)
        image = render_mesh(cam, v, f, c, white_background=white_background, supersample=supersample)["render"].clamp(0, 1)
        shape = render_mesh_shape(cam, v, f, supersample=supersample)
        name = "%05d.png" % i
        save_png(image, os.path.join(dirs["mesh_image"], name))
        save_png(shape, os.path.join(dirs["mesh_shape"], name))
        m = image_metrics(image, fr.image.to(device=device, dtype=image.dtype).clamp(0, 1), quantize=quantize)
        per_view["PSNR"][name], per_view["SSIM"][name], per_view["MS-SSIM"][name] = float(m["psnr"]), float(m["ssim"]), float(m["ms_ssim"])
        if log is not None:
            log("%s (%s, %d faces): PSNR %.4f SSIM %.6f MS-SSIM %.6f" % (name, frames[i], f.shape[0], float(m["psnr"]), float(m["ssim"]), float(m["ms_ssim"])))
    results = {k: float(np.mean(list(per_view[k].values()))) for k in ("PSNR", "SSIM", "MS-SSIM")}
    number = lambda x: float(x) if math.isfinite(float(x)) else None       # NaN -> null, as evaluate.write_results writes it
    clean = lambda d: {k: (clean(x) if isinstance(x, dict) else number(x)) for k, x in d.items()}
    for name, d in (("mesh_render_results.json", results), ("mesh_render_per_view.json", per_view)):
        with open(os.path.join(out_dir, name), "w") as fp:
            json.dump(clean(d), fp, indent=True)
    if log is not None:
        log("mesh renders: PSNR %.4f SSIM %.6f MS-SSIM %.6f" % (results["PSNR"], results["SSIM"], results["MS-SSIM"]))
    return {"results": results, "per_view": per_view}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_render",
                                 description="Draw frame_<i>.ply from the test cameras of a D-NeRF dataset (mesh_image/, mesh_shape/) and score "
                                             "mesh_image/ against the test images: PSNR, SSIM, MS-SSIM.")
    ap.add_argument("mesh_dir")
    ap.add_argument("data_path")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--supersample", type=int, default=1)
    ap.add_argument("--float", action="store_true", help="score the float renders instead of their 8-bit files")
    ap.add_argument("--black-background", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    return render_meshes(a.mesh_dir, a.data_path, out_dir=a.out_dir, white_background=not a.black_background, device=a.device,
                         supersample=a.supersample, quantize=not a.float, log=print)


if __name__ == "__main__":
    main()
