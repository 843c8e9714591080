"""A surface mesh of the dynamic scene at any time t: what the reference's render_mesh.py produces (render every training camera
with the time pinned, fuse the depth maps into a truncated signed distance volume, extract the surface, drop small components,
write frame_<i>.ply), without open3d / trimesh / mcubes.

  views_at_time            <- scene/__init__.py:120-131 getTrainCameras_mesh + utils/mesh_utils.py:94-155 reconstruction(state="mesh")
  TSDFVolume.integrate     <- utils/mesh_utils.py:218-266 compute_sdf_perframe + compute_unbounded_tsdf (inv_contraction=None)
  TSDFVolume.extract       <- the surface extraction of :158-199 / :268-271, here marching TETRAHEDRA (below)
  keep_largest_components  <- utils/mesh_utils.py:24-45 post_process_mesh (on the host; mesh_clean.filter_components is the same
                              rule on the mesh's own device, which extract_meshes uses for a mesh that lies on a HIP device)
  extract_meshes           <- render_mesh.py:169-219

On a HIP device the fuser and the extraction are the kernels of libdgs_mesh_ops.so (include/dgs_mesh_ops.h, which states the
arithmetic, the grid layout and the output order); on CPU tensors this module runs the PyTorch / NumPy statement of the same
arithmetic: every fp32 operation in the same order, so the two agree bit for bit wherever no accept / reject decision differs.

Four departures from the reference's fuser (header): weights start at 0 (prior_weight=1 gives the reference's
start tsdf = 1, w = 1); the pixel convention is the rasterizer's own; a voxel-view whose four depth taps are not all valid is
rejected instead of interpolated across the silhouette; the colour is sampled only where |sdf| < trunc.  And one in the view
preparation: depth is masked by the rendered alpha (alpha < alpha_min -> 0), not by the reference's colour threshold
(`depth_filtering`), which deletes dark surfaces on a black background.

Marching tetrahedra: every cell is cut into the six Kuhn tetrahedra around its diagonal corner 0 -> corner 7.  The decomposition is
translation invariant, so the faces of neighbouring cells agree and the surface is watertight by construction, with no ambiguous
cases and no 256-entry table.  Every tetrahedron edge runs from a grid point in one of 7 non-negative directions, which gives every
mesh vertex the key (grid point) * 7 + direction and its id as the rank of that key: an indexed mesh without hashing."""
import math
import os

import numpy as np
import torch

# Kuhn tetrahedra: corner c of a cell = (c & 1, c >> 1 & 1, c >> 2 & 1) in (x, y, z); tetrahedron of the permutation (a, b, c) of
# (0, 1, 2), lexicographic order, = corners {0, 1<<a, 1<<a | 1<<b, 7}
_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
_TETS = tuple((0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in _PERMS)
_TET_ODD = (False, True, True, False, False, True)       # parity of the permutation = orientation of the tetrahedron
# bit S (bit p of S set: chain position p negative) = the triangles of an EVEN tetrahedron, as listed, already face the positive side
_KEEP_EVEN = 0x32DA


# ---- views ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def views_at_time(surfels, deform, cameras, t, bg, alpha_min=0.5, rasterizer_cls=None):
    """Every camera of `cameras` rendered with the scene at time t -> (depth [V,H,W], rgb [V,3,H,W], proj [V,16]) on the model's device.
    Camera poses come from `cameras`, the time is t for all of them (reconstruction(state="mesh"): the time input of the deformation
    is t for every node); the colour is the diffuse one (active_sh_degree 0, render_mesh.py:200-201).  deform=None renders the
    surfels as they are.  depth = render()'s 'depth' (median depth), 0 where alpha < alpha_min.  Nothing goes to the host per view."""
    from .render import render
    dev = surfels.get_xyz.device
    d = {}
    if deform is not None:
        tt = torch.tensor([float(t)], dtype=torch.float32, device=dev)
        d = deform(surfels.get_xyz.detach(), deform.expand_time(tt), surfels.feature, surfels.motion_mask)
        d = {"d_xyz": d["d_xyz"], "d_rotation": d["d_rotation"], "d_scaling": d["d_scaling"]}
    degree = surfels.active_sh_degree
    surfels.active_sh_degree = 0
    try:
        depth, rgb, proj = [], [], []
        for cam in cameras:
            cam = cam.to(dev)
            out = render(cam, surfels, bg, rasterizer_cls=rasterizer_cls, **d)
            depth.append(torch.where(out["alpha"][0] >= alpha_min, out["depth"][0], torch.zeros_like(out["depth"][0])))
            rgb.append(out["render"])
            proj.append(cam.full_proj_transform.reshape(16))
    finally:
        surfels.active_sh_degree = degree
    return torch.stack(depth).float().contiguous(), torch.stack(rgb).float().contiguous(), torch.stack(proj).float().contiguous()


def bounds_from_surfels(xyz, quantile=0.01, margin=0.1):
    """(lo [3], hi [3]) python floats: the [quantile, 1 - quantile] range of the positions per axis, grown by `margin` on every side."""
    x = xyz.detach().float().cpu().numpy()
    lo, hi = np.quantile(x, quantile, axis=0) - margin, np.quantile(x, 1.0 - quantile, axis=0) + margin
    return [float(v) for v in lo], [float(v) for v in hi]


# ---- the volume -----------------------------------------------------------------------------------------------------------------
def integrate_torch(tsdf, weight, color, origin, voxel_size, depth, rgb, proj, trunc, depth_trunc):
    """The five steps of include/dgs_mesh_ops.h for all voxels at once, view by view, in the dtype of the volume.  Returns the new
    (tsdf, weight, color).  Also the comparator of the GPU tests and the baseline of tools/mesh_timing.py."""
    dt, dev = tsdf.dtype, tsdf.device
    Nx, Ny, Nz = tsdf.shape
    sc = lambda x: torch.tensor(x, dtype=dt, device=dev)
    V, H, W = depth.shape
    h = sc(voxel_size)
    px = (sc(origin[0]) + h * torch.arange(Nx, dtype=dt, device=dev)).view(Nx, 1, 1)
    py = (sc(origin[1]) + h * torch.arange(Ny, dtype=dt, device=dev)).view(1, Ny, 1)
    pz = (sc(origin[2]) + h * torch.arange(Nz, dtype=dt, device=dev)).view(1, 1, Nz)
    Wf, Hf, trunc, depth_trunc, one, zero = sc(W), sc(H), sc(trunc), sc(depth_trunc), sc(1.0), sc(0.0)
    for v in range(V):
        m = proj[v].to(dt).view(4, 4)
        hom = lambda c: px * m[0, c] + ((py * m[1, c] + pz * m[2, c]) + m[3, c])
        z = hom(3)
        ok = z > 0
        zs = torch.where(ok, z, one)
        nx, ny = hom(0) / zs, hom(1) / zs
        ok = ok & (nx > -1) & (nx < 1) & (ny > -1) & (ny < 1)
        u, vv = ((nx + 1) * Wf - 1) / 2, ((ny + 1) * Hf - 1) / 2
        u0 = torch.where(ok, torch.floor(u).clamp(0, W - 2), zero)      # (a rejected voxel taps pixel (0, 0): any valid address)
        v0 = torch.where(ok, torch.floor(vv).clamp(0, H - 2), zero)
        fu, fv = (u - u0).clamp(0, 1), (vv - v0).clamp(0, 1)
        a = v0.long() * W + u0.long()
        D = depth[v].reshape(-1).to(dt)
        d00, d01, d10, d11 = D[a], D[a + 1], D[a + W], D[a + W + 1]
        for tap in (d00, d01, d10, d11):
            ok = ok & (tap > 0) & (tap <= depth_trunc)
        gu, gv = 1 - fu, 1 - fv
        d = (d00 * gu + d01 * fu) * gv + (d10 * gu + d11 * fu) * fv
        sdf = d - z
        ok = ok & (sdf > -trunc)
        s = (sdf / trunc).clamp(-1, 1)
        wn = weight + 1
        tsdf = torch.where(ok, (tsdf * weight + s) / wn, tsdf)
        okc = ok & (sdf < trunc)
        chans = []
        for ch in range(3):
            C = rgb[v, ch].reshape(-1).to(dt)
            c = (C[a] * gu + C[a + 1] * fu) * gv + (C[a + W] * gu + C[a + W + 1] * fu) * fv
            chans.append(torch.where(okc, (color[..., ch] * weight + c) / wn, color[..., ch]))
        color = torch.stack(chans, -1)
        weight = torch.where(ok, wn, weight)
    return tsdf, weight, color


def _march_numpy(tsdf, weight, color, origin, voxel_size):
    """Marching tetrahedra in NumPy with the kernels' bookkeeping: per-cell triangle counts, per-grid-point edge masks, ids from
    prefix sums, the winding from the sign pattern.  Arithmetic in the dtype of tsdf."""
    f = np.ascontiguousarray(tsdf)
    dt = f.dtype.type
    Nx, Ny, Nz = f.shape
    neg, obs = f < 0, np.asarray(weight) > 0
    sl = lambda arr, c: arr[(c & 1):Nx - 1 + (c & 1), (c >> 1 & 1):Ny - 1 + (c >> 1 & 1), (c >> 2 & 1):Nz - 1 + (c >> 2 & 1)]
    nc = [sl(neg, c) for c in range(8)]
    seen = np.logical_and.reduce([sl(obs, c) for c in range(8)])
    active = np.zeros((Nx, Ny, Nz), bool)
    active[:Nx - 1, :Ny - 1, :Nz - 1] = seen & np.logical_or.reduce(nc) & ~np.logical_and.reduce(nc)
    # per grid point: the 7 edges that start there; an edge g -> g + d is held by the cells g - o with o & d == 0
    pad = np.zeros((Nx + 1, Ny + 1, Nz + 1), bool)
    pad[1:, 1:, 1:] = active
    act_o = [pad[1 - (o & 1):Nx + 1 - (o & 1), 1 - (o >> 1 & 1):Ny + 1 - (o >> 1 & 1), 1 - (o >> 2 & 1):Nz + 1 - (o >> 2 & 1)] for o in range(8)]
    mask = np.zeros((Nx, Ny, Nz), np.uint8)
    for d in range(1, 8):
        dx, dy, dz = d & 1, d >> 1 & 1, d >> 2 & 1
        held = np.logical_or.reduce([act_o[o] for o in range(8) if o & d == 0])
        differ = np.zeros((Nx, Ny, Nz), bool)
        differ[:Nx - dx, :Ny - dy, :Nz - dz] = neg[:Nx - dx, :Ny - dy, :Nz - dz] != neg[dx:, dy:, dz:]
        mask |= ((held & differ).astype(np.uint8) << (d - 1)).astype(np.uint8)
    popc = np.array([bin(i).count("1") for i in range(128)], np.int64)
    mask_flat = mask.reshape(-1)
    vert_excl = np.cumsum(popc[mask_flat]) - popc[mask_flat]
    n_verts = int(popc[mask_flat].sum())
    # vertices, ascending by key
    sx, sy = Ny * Nz, Nz
    off = lambda c: (c & 1) * sx + (c >> 1 & 1) * sy + (c >> 2 & 1)
    pts = np.flatnonzero(mask_flat)
    bits = (mask_flat[pts, None] >> np.arange(7, dtype=np.uint8)[None, :]) & 1
    pi, di = np.nonzero(bits)                                   # row-major: ascending (point, direction) = ascending key
    la = pts[pi]
    dd = di + 1
    lb = la + (dd & 1) * sx + (dd >> 1 & 1) * sy + (dd >> 2 & 1)
    ff = f.reshape(-1)
    fa, fb = ff[la], ff[lb]
    t = fa / (fa - fb)
    o3, hh = np.asarray(origin, f.dtype), dt(voxel_size)
    ijk_a = np.stack((la // sx, (la // sy) % Ny, la % Nz), -1)
    ijk_b = ijk_a + np.stack((dd & 1, dd >> 1 & 1, dd >> 2 & 1), -1)
    pa, pb = o3 + hh * ijk_a.astype(f.dtype), o3 + hh * ijk_b.astype(f.dtype)
    vertices = pa + t[:, None] * (pb - pa)
    colors = None
    if color is not None:
        cc = np.asarray(color).reshape(-1, 3)
        colors = cc[la] + t[:, None].astype(cc.dtype) * (cc[lb] - cc[la])
    assert vertices.shape[0] == n_verts
    # faces, ascending by (cell, tetrahedron, triangle)
    cells = np.flatnonzero(active.reshape(-1))
    negc = np.stack([neg.reshape(-1)[cells + off(c)] for c in range(8)], -1)

    def eid(cl, a, b):   # id of the vertex on the edge between corners a and b (a a subset of b) of the cells cl
        p = cl + _off_arr(a, sx, sy)
        return vert_excl[p] + popc[mask_flat[p].astype(np.int64) & ((1 << ((a ^ b) - 1)) - 1)]

    rows = []
    for ti, ch in enumerate(_TETS):
        chv = np.array(ch)
        S = sum(negc[:, ch[p]].astype(np.int64) << p for p in range(4))
        cnt = popc[S]
        keep = (((_KEEP_EVEN >> S) & 1) == 1) != _TET_ODD[ti]
        # one or three negative corners: the lone corner joined to the other three in ascending order
        sel = np.flatnonzero((cnt == 1) | (cnt == 3))
        lone = np.where(cnt[sel] == 1, S[sel], ~S[sel] & 15)
        apex = np.log2(lone).astype(np.int64)
        others = np.array([[p for p in range(4) if p != a] for a in range(4)])[apex]          # [m,3]
        lo_, hi_ = np.minimum(others, apex[:, None]), np.maximum(others, apex[:, None])
        q = np.stack([eid(cells[sel], chv[lo_[:, n]], chv[hi_[:, n]]) for n in range(3)], -1)
        k1 = keep[sel]
        tri = np.stack((q[:, 0], np.where(k1, q[:, 1], q[:, 2]), np.where(k1, q[:, 2], q[:, 1])), -1)
        rows.append((cells[sel], np.full(sel.size, ti), np.zeros(sel.size, np.int64), tri))
        # two negative corners a < b, non-negative c < d: the quad (a,c), (a,d), (b,d), (b,c)
        sel = np.flatnonzero(cnt == 2)
        bitsS = (S[sel, None] >> np.arange(4)[None, :]) & 1
        order = np.argsort(-bitsS, axis=1, kind="stable")       # the two negative positions (ascending), then the two others
        a_, b_, c_, d_ = order[:, 0], order[:, 1], order[:, 2], order[:, 3]
        quad = []
        for x, y in ((a_, c_), (a_, d_), (b_, d_), (b_, c_)):
            lo2, hi2 = chv[np.minimum(x, y)], chv[np.maximum(x, y)]
            quad.append(eid(cells[sel], lo2, hi2))
        k2 = keep[sel]
        t0 = np.stack((quad[0], np.where(k2, quad[1], quad[2]), np.where(k2, quad[2], quad[1])), -1)
        t1 = np.stack((quad[0], np.where(k2, quad[2], quad[3]), np.where(k2, quad[3], quad[2])), -1)
        rows.append((cells[sel], np.full(sel.size, ti), np.zeros(sel.size, np.int64), t0))
        rows.append((cells[sel], np.full(sel.size, ti), np.ones(sel.size, np.int64), t1))
    cell_k = np.concatenate([r[0] for r in rows])
    tet_k = np.concatenate([r[1] for r in rows])
    tri_k = np.concatenate([r[2] for r in rows])
    faces = np.concatenate([r[3] for r in rows]).reshape(-1, 3)
    faces = faces[np.lexsort((tri_k, tet_k, cell_k))]
    return vertices, faces.astype(np.int32 if n_verts < 2 ** 31 else np.int64), colors


def _off_arr(c, sx, sy):
    return (c & 1) * sx + (c >> 1 & 1) * sy + (c >> 2 & 1)


class TSDFVolume:
    """A dense truncated signed distance volume: grid point (i, j, k) at origin + voxel_size * (i, j, k), tensors tsdf / weight
    [Nx,Ny,Nz] and color [Nx,Ny,Nz,3] on `device`.  HIP device: libdgs_mesh_ops.so; CPU: the PyTorch / NumPy statement (dtype may
    then be torch.float64: the comparator of the parity margins)."""

    def __init__(self, origin, voxel_size, dims, device="cpu", prior_weight=0.0, dtype=torch.float32):
        self.device = torch.device(device)
        self.dims = tuple(int(n) for n in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError("TSDFVolume: three dimensions of at least 2 grid points each")
        if self.device.type != "cpu" and dtype != torch.float32:
            raise ValueError("TSDFVolume: the HIP path is fp32")
        self.dtype = dtype
        # the kernels receive origin and voxel size as fp32: keep exactly those values on every path of an fp32 volume
        rnd = (lambda x: float(np.float32(x))) if dtype == torch.float32 else float
        self.origin = tuple(rnd(v) for v in origin)
        self.voxel_size = rnd(voxel_size)
        self.prior_weight = float(prior_weight)
        self.tsdf = self.weight = self.color = None
        self.reset()

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size, device="cpu", **kw):
        dims = [max(2, int(math.ceil((h - l) / voxel_size)) + 1) for l, h in zip(lo, hi)]
        return cls(lo, voxel_size, dims, device, **kw)

    def reset(self):
        kw = dict(dtype=self.dtype, device=self.device)
        self.weight = torch.full(self.dims, self.prior_weight, **kw)
        self.tsdf = torch.full(self.dims, 1.0 if self.prior_weight > 0 else 0.0, **kw)
        self.color = torch.zeros(self.dims + (3,), **kw)
        self._fresh = True

    @torch.no_grad()
    def integrate(self, depth, rgb, proj, trunc=None, depth_trunc=6.0):
        """Fuse the views depth [V,H,W], rgb [V,3,H,W], proj [V,16] (views_at_time) into the volume; may be called repeatedly with
        chunks of views (bit-identical to one call).  trunc defaults to 5 voxels (render_mesh.py:210)."""
        trunc = 5.0 * self.voxel_size if trunc is None else float(trunc)
        depth, rgb, proj = (x.to(self.device) for x in (depth, rgb, proj))
        if depth.dim() != 3 or depth.shape[1] < 2 or depth.shape[2] < 2:
            raise ValueError("TSDFVolume.integrate: depth [V,H,W] with H, W >= 2")
        if self.device.type == "cpu":
            self.tsdf, self.weight, self.color = integrate_torch(self.tsdf, self.weight, self.color, self.origin, self.voxel_size, depth, rgb,
                                                                 proj.reshape(-1, 16), trunc, depth_trunc)
        else:
            from . import _mesh_ops   # a missing library is an error, never a reason to run the PyTorch statement instead
            _mesh_ops.tsdf_integrate(self.dims, self.origin, self.voxel_size, depth.float().contiguous(), rgb.float().contiguous(),
                                     proj.reshape(-1, 16).float().contiguous(), trunc, float(depth_trunc), self.prior_weight,
                                     not self._fresh, self.tsdf, self.weight, self.color)
        self._fresh = False
        return self

    @torch.no_grad()
    def extract(self):
        """-> (vertices [Nv,3] f32, faces [Nf,3] int32, colors [Nv,3] f32): vertices ascending by key, faces by (cell, tetrahedron,
        triangle), normals pointing from negative to positive tsdf (outward, toward the cameras)."""
        if self.device.type == "cpu":
            v, f, c = _march_numpy(self.tsdf.numpy(), self.weight.numpy(), self.color.numpy(), self.origin, self.voxel_size)
            return torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(f), torch.from_numpy(np.ascontiguousarray(c))
        from . import _mesh_ops
        return _mesh_ops.marching_tetrahedra(self.dims, self.origin, self.voxel_size, self.tsdf, self.weight, self.color)


# ---- post-processing ------------------------------------------------------------------------------------------------------------
def vertex_components(n_vertices, faces):
    """Label [n_vertices] of the connected component (over shared vertices) of every vertex: the smallest vertex id in it.  Label
    propagation with pointer jumping, NumPy only."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    label = np.arange(n_vertices, dtype=np.int64)
    while True:
        m = label[faces].min(axis=1)
        new = label.copy()
        for c in range(3):
            np.minimum.at(new, faces[:, c], m)
        new = np.minimum(new, new[new])
        while True:                      # pointer jumping: every label points at its root
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, label):
            return label
        label = new


def keep_largest_components(vertices, faces, colors=None, n_keep=1000, min_faces=50):
    """post_process_mesh (utils/mesh_utils.py:24-45) without open3d: keep the components that have at least as many faces as the
    n_keep-th largest one, and at least min_faces; renumber the faces and drop the vertices nothing refers to.  Components are
    connected over shared vertices.  Returns (vertices, faces, colors) as tensors on the CPU (colors None if none were given)."""
    v = vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    c = None if colors is None else (colors.detach().cpu().numpy() if torch.is_tensor(colors) else np.asarray(colors))
    f = f.reshape(-1, 3)
    if f.shape[0]:
        face_label = vertex_components(v.shape[0], f)[f[:, 0]]
        labels, inverse, counts = np.unique(face_label, return_inverse=True, return_counts=True)
        ranked = np.sort(counts)
        threshold = max(int(ranked[-min(int(n_keep), ranked.size)]), int(min_faces))
        f = f[counts[inverse] >= threshold]
    used = np.zeros(v.shape[0], bool)
    used[f.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    f = remap[f].astype(f.dtype)
    out_c = None if c is None else torch.from_numpy(np.ascontiguousarray(c[used]))
    return torch.from_numpy(np.ascontiguousarray(v[used])), torch.from_numpy(np.ascontiguousarray(f)), out_c


# ---- the product ----------------------------------------------------------------------------------------------------------------
def extract_meshes(model_path, data_path, times=None, voxel_size=0.004, depth_trunc=6.0, n_keep=1000, out_dir=None, iteration=-1,
                   device="cuda:0", white_background=False, alpha_min=0.5, bounds=None, quantile=0.01, margin=None, view_chunk=32,
                   min_faces=50, rasterizer_cls=None, log=None, simplify_cell=None, smooth_iterations=None, smooth_method="taubin",
                   decimate_faces=None, decimate_ratio=None, fill_holes=None):
    """render_mesh.py:169-219: restore() the checkpoint, take the training cameras of the dataset, and for every time (default: the
    times of the test split) render them all at that time, fuse, extract, filter and write <out_dir>/frame_<i>.ply
    (out_dir default: <model_path>/train/ours_<iteration>).  bounds: (lo, hi) of the volume; default: bounds_from_surfels of the
    deformed surfel positions at that time, margin 10 voxels + the truncation.  simplify_cell: if given, the filtered mesh goes
    through mesh_simplify.simplify_mesh with that cell size before it is written (None: written as extracted).
    smooth_iterations: if given, the filtered mesh first goes through mesh_smooth.smooth_mesh(method=smooth_method) with that many
    iterations -- before the simplification, whose plane quadrics then see cleaner normals (None: nothing is called).
    fill_holes: if given, mesh_fill.fill_holes(max_hole_edges=fill_holes) closes the holes of the filtered mesh before the smoothing,
    which then blends the fill into the surface (None: nothing is called).  Returns the list of files written."""
    from . import io as dio
    from .fit import restore
    device = torch.device(device)
    it = dio.search_for_max_iteration(os.path.join(model_path, "point_cloud")) if iteration == -1 else iteration
    surfels, deform = restore(model_path, iteration=it, device=device)
    data = dio.load_dnerf(data_path, white_background=white_background)
    cams = [fr.camera for fr in data["train"]]
    if times is None:
        times = [float(fr.camera.fid) for fr in data["test"]]
    out_dir = out_dir or os.path.join(model_path, "train", "ours_{}".format(it))
    os.makedirs(out_dir, exist_ok=True)
    bg = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], device=device)
    trunc = 5.0 * voxel_size
    written = []
    for i, t in enumerate(times):
        if bounds is None:
            with torch.no_grad():
                tt = torch.tensor([float(t)], dtype=torch.float32, device=device)
                dx = deform(surfels.get_xyz.detach(), deform.expand_time(tt), surfels.feature, surfels.motion_mask)["d_xyz"]
                lo, hi = bounds_from_surfels((surfels.get_xyz + dx)[surfels.alive], quantile, trunc + 10 * voxel_size if margin is None else margin)
        else:
            lo, hi = bounds
        vol = TSDFVolume.from_bounds(lo, hi, voxel_size, device)
        for s in range(0, len(cams), view_chunk):        # the rendered stack of a chunk lives on the device only
            depth, rgb, proj = views_at_time(surfels, deform, cams[s:s + view_chunk], t, bg, alpha_min=alpha_min, rasterizer_cls=rasterizer_cls)
            vol.integrate(depth, rgb, proj, trunc=trunc, depth_trunc=depth_trunc)
        v, f, c = vol.extract()
        if v.is_cuda:                                    # the same mesh, filtered where it lies: it leaves the device once, for the writer
            from .mesh_clean import filter_components
            v, f, c = filter_components(v, f, c, n_keep=n_keep, min_faces=min_faces)
        else:
            v, f, c = keep_largest_components(v, f, c, n_keep=n_keep, min_faces=min_faces)
        if fill_holes is not None:                       # still where it lies: the cells no view saw, closed before the smoothing blends them
            from .mesh_fill import fill_holes as fill
            v, f, c = fill(v, f, c, max_hole_edges=fill_holes)
        if smooth_iterations is not None:                # still where it lies: the voxel staircase goes before the quadrics see it
            from .mesh_smooth import smooth_mesh
            v, f, c = smooth_mesh(v, f, c, method=smooth_method, iterations=smooth_iterations)
        if simplify_cell is not None:                    # still where it lies: vertex clustering with quadric placement
            from .mesh_simplify import simplify_mesh
            v, f, c = simplify_mesh(v, f, c, cell_size=simplify_cell)
        if decimate_faces is not None or decimate_ratio is not None:   # last: edge collapse to a face budget, still a manifold
            from .mesh_decimate import decimate_mesh
            v, f, c = decimate_mesh(v, f, c, target_faces=decimate_faces, ratio=decimate_ratio)
        path =os.path.join(out_dir, "frame_{}.ply".format(i))
        dio.write_mesh_ply(path, v, f, c)
        written.append(path)
        if log is not None:
            log("t = %.4f: grid %s, %d vertices, %d faces -> %s" % (t, "x".join(str(n) for n in vol.dims), v.shape[0], f.shape[0], path))
    return written


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh", description="One mesh per timestamp from a trained model (render_mesh.py).")
    ap.add_argument("model")
    ap.add_argument("data")
    ap.add_argument("--times", type=float, nargs="*", default=None, help="default: the times of the dataset's test split")
    ap.add_argument("--voxel-size", type=float, default=0.004)
    ap.add_argument("--depth-trunc", type=float, default=6.0)
    ap.add_argument("--num-cluster", type=int, default=1000)
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--white-background", action="store_true")
    ap.add_argument("--simplify-cell", type=float, default=None, help="simplify every mesh by vertex clustering with this cell size (default: no)")
    ap.add_argument("--smooth-iterations", type=int, default=None, help="smooth every mesh with this many iterations before it is simplified or written (default: no)")
    ap.add_argument("--smooth-method", choices=("simple", "laplacian", "taubin"), default="taubin")
    ap.add_argument("--decimate-faces", type=int, default=None, help="decimate every mesh by edge collapse to this many faces, last (default: no)")
    ap.add_argument("--decimate-ratio", type=float, default=None, help="decimate every mesh by edge collapse to this share of its faces, last (default: no)")
    ap.add_argument("--fill-holes", type=int, default=None, metavar="N",
                    help="close every hole of up to N edges after the component filter, before the smoothing (default: no)")
    a = ap.parse_args(argv)
    extract_meshes(a.model, a.data, times=a.times, voxel_size=a.voxel_size, depth_trunc=a.depth_trunc, n_keep=a.num_cluster, out_dir=a.out_dir,
                   iteration=a.iteration, device=a.device, white_background=a.white_background, log=print, simplify_cell=a.simplify_cell,
                   smooth_iterations=a.smooth_iterations, smooth_method=a.smooth_method, decimate_faces=a.decimate_faces,
                   decimate_ratio=a.decimate_ratio, fill_holes=a.fill_holes)


if __name__ == "__main__":
    main()
