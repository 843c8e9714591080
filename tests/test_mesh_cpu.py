"""Mesh extraction on the CPU: marching tetrahedra on an exact field, the vectorised fuser against a plain loop, a sphere fused from
analytic depth maps, the component filter and the mesh PLY.  The helpers here (cameras, analytic depth maps, the independent
statement of marching tetrahedra, the mesh checks) are also what tests/test_mesh_gpu.py compares the HIP path with."""
import math
import os

import numpy as np
import pytest
import torch

from dgs_amd.cameras import make_camera, pose_spherical

R_S = 0.55
C_S = np.array([-0.1, 0.05, 0.2])
BOX, BOX_OFFSET = 1.6, np.array([0.013, -0.007, 0.003])
FOV = 0.6911
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def spread_cameras(n, W, H, t=0.0, fov=FOV, radius=4.0):
    """theta_k = -180 + 360 frac(0.6180339887 k), phi_k = -70 + 140 frac(0.7548776662 k): views from above AND below."""
    out = []
    for k in range(n):
        theta = -180.0 + 360.0 * ((k * 0.6180339887) % 1.0)
        phi = -70.0 + 140.0 * ((k * 0.7548776662) % 1.0)
        out.append(make_camera(pose_spherical(theta, phi, radius), fov, fov, W, H, t))
    return out


def _pixel_rays(cam):
    W, H = cam.image_width, cam.image_height
    x = ((2 * np.arange(W) + 1) / W - 1) * math.tan(cam.FoVx / 2)
    y = ((2 * np.arange(H) + 1) / H - 1) * math.tan(cam.FoVy / 2)
    return np.stack(np.broadcast_arrays(x[None, :], y[:, None], np.ones((H, W))), -1)   # view-space directions with d_z = 1


def sphere_depth(cam, centre=C_S, radius=R_S):
    """Analytic view-space z of the sphere hit through the pixel centres (float64), 0 where the ray misses."""
    w2c = cam.world_view_transform.double().numpy().T
    c = w2c[:3, :3] @ centre + w2c[:3, 3]
    d = _pixel_rays(cam)
    a, b, cc = (d * d).sum(-1), d @ c, c @ c - radius ** 2
    disc = b * b - a * cc
    return np.where(disc > 0, (b - np.sqrt(np.maximum(disc, 0))) / a, 0.0)


PLATE_C, PLATE_HALF = np.array([0.68, 0.0, 0.15]), 0.15
_a = 0.5
PLATE_E1, PLATE_E2 = np.array([-math.sin(_a), 0.0, math.cos(_a)]), np.array([0.0, 1.0, 0.0])   # 0.11 (6.5 voxels at N = 96) clear of the sphere


def plate_depth(cam):
    """A tilted square plate behind the sphere (half in, half out of the box): view-space z of the hit, 0 where missed."""
    w2c = cam.world_view_transform.double().numpy().T
    R = w2c[:3, :3]
    c, e1, e2 = R @ PLATE_C + w2c[:3, 3], R @ PLATE_E1, R @ PLATE_E2
    n = np.cross(e1, e2)
    d = _pixel_rays(cam)
    den = d @ n
    t = np.where(np.abs(den) > 1e-9, (c @ n) / np.where(np.abs(den) > 1e-9, den, 1.0), 0.0)
    p = t[..., None] * d - c
    hit = (t > 0) & (np.abs(p @ e1) <= PLATE_HALF) & (np.abs(p @ e2) <= PLATE_HALF)
    return np.where(hit, t, 0.0)


def nearest_depth(a, b):
    return np.where((a > 0) & (b > 0), np.minimum(a, b), np.maximum(a, b))


def view_colors(V, H, W):
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    return np.stack([np.stack([0.5 + 0.4 * np.sin(5.0 * x + 0.7 * v + c) * np.cos(3.0 * y + c) for c in range(3)]) for v in range(V)])


def sphere_box(N):
    h = BOX / (N - 1)
    return C_S - BOX / 2 + BOX_OFFSET, h


def fusion_inputs(n_views=24, size=200, plate=False, dtype=torch.float32):
    cams = spread_cameras(n_views, size, size)
    deps = [nearest_depth(sphere_depth(c), plate_depth(c)) if plate else sphere_depth(c) for c in cams]
    depth = torch.tensor(np.stack(deps), dtype=dtype)
    rgb = torch.tensor(view_colors(n_views, size, size), dtype=dtype)
    proj = torch.stack([c.full_proj_transform.reshape(16) for c in cams]).to(dtype)
    return depth, rgb, proj


# ---- an independent statement of marching tetrahedra ----------------------------------------------------------------------------
def marching_tets_reference(tsdf, weight, origin, h):
    """Vertex keys from np.unique, the winding from the geometry (normal . (centroid of the non-negative corners - centroid of the
    negative ones) in float64): neither the prefix sums nor the sign-pattern table of the implementation.
    -> (vertices [Nv,3] float32, faces [Nf,3] int64, keys [Nv] int64)."""
    f = np.asarray(tsdf, np.float32)
    Nx, Ny, Nz = f.shape
    sx, sy = Ny * Nz, Nz
    neg, obs = f < 0, np.asarray(weight) > 0
    cn = lambda arr, c: arr[(c & 1):Nx - 1 + (c & 1), (c >> 1 & 1):Ny - 1 + (c >> 1 & 1), (c >> 2 & 1):Nz - 1 + (c >> 2 & 1)]
    ncorn = np.stack([cn(neg, c) for c in range(8)], -1)
    act = np.stack([cn(obs, c) for c in range(8)], -1).all(-1) & ncorn.any(-1) & ~ncorn.all(-1)
    ci, cj, ck = np.nonzero(act)
    cell_lin = (ci * Ny + cj) * Nz + ck
    corner_xyz = np.array([[c & 1, c >> 1 & 1, c >> 2 & 1] for c in range(8)])
    negc = ncorn[ci, cj, ck]                                       # [M,8]
    recs = []                                                     # (cell, tet, tri, lo[3] lin, hi[3] lin, flip)
    for ti, p in enumerate(PERMS):
        chain = [0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7]
        S = sum(negc[:, chain[q]].astype(int) << q for q in range(4))
        for s in range(1, 15):
            sel = np.flatnonzero(S == s)
            if not sel.size:
                continue
            ins = [q for q in range(4) if s >> q & 1]
            outs = [q for q in range(4) if not s >> q & 1]
            if len(ins) == 2:
                (a, b), (c, d) = ins, outs
                quad = [(a, c), (a, d), (b, d), (b, c)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            else:
                apex = ins[0] if len(ins) == 1 else outs[0]
                tris = [[(apex, q) for q in range(4) if q != apex]]
            cell_ijk = np.stack((ci[sel], cj[sel], ck[sel]), -1)
            pos = [cell_ijk + corner_xyz[chain[q]] for q in range(4)]            # grid coordinates of the 4 chain corners
            lin = [(x[:, 0] * Ny + x[:, 1]) * Nz + x[:, 2] for x in pos]
            val = [f.reshape(-1)[l].astype(np.float64) for l in lin]
            toward = np.mean([pos[q] for q in outs], 0) - np.mean([pos[q] for q in ins], 0)
            for k, tri in enumerate(tris):
                pts = []
                for (x, y) in tri:
                    lo, hi = min(x, y), max(x, y)
                    t = val[lo] / (val[lo] - val[hi])
                    pts.append(pos[lo] + t[:, None] * (pos[hi] - pos[lo]))
                flip = np.einsum("ij,ij->i", np.cross(pts[1] - pts[0], pts[2] - pts[0]), toward) < 0
                lo = np.stack([lin[min(x, y)] for x, y in tri], -1)
                hi = np.stack([lin[max(x, y)] for x, y in tri], -1)
                recs.append((cell_lin[sel], np.full(sel.size, ti), np.full(sel.size, k), lo, hi, flip))
    if not recs:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros(0, np.int64)
    cell, tet, tri, lo, hi, flip = (np.concatenate([r[i] for r in recs]) for i in range(6))
    order = np.lexsort((tri, tet, cell))
    lo, hi, flip = lo[order], hi[order], flip[order]
    delta = hi - lo                                               # offset of the upper end: dx * sx + dy * sy + dz
    dcode = np.zeros_like(delta)
    for d in range(1, 8):
        dcode[delta == (d & 1) * sx + (d >> 1 & 1) * sy + (d >> 2 & 1)] = d
    assert (dcode > 0).all()
    keys = lo * 7 + (dcode - 1)
    ukeys, faces = np.unique(keys.reshape(-1), return_inverse=True)
    faces = faces.reshape(-1, 3)
    faces[flip] = faces[flip][:, [0, 2, 1]]
    la, d = ukeys // 7, ukeys % 7 + 1
    lb = la + (d & 1) * sx + (d >> 1 & 1) * sy + (d >> 2 & 1)
    ijk = lambda l: np.stack((l // sx, (l // sy) % Ny, l % Nz), -1).astype(np.float32)
    o, hh = np.asarray(origin, np.float32), np.float32(h)
    fa, fb = f.reshape(-1)[la], f.reshape(-1)[lb]
    t = fa / (fa - fb)
    pa, pb = o + hh * ijk(la), o + hh * ijk(lb)
    return pa + t[:, None] * (pb - pa), faces, ukeys


# ---- mesh checks ----------------------------------------------------------------------------------------------------------------
def mesh_report(V, F):
    """closed: every undirected edge in exactly two triangles; oriented: every directed edge in exactly one; chi = V - E + F over the
    vertices the faces use; signed volume; number of zero-area triangles."""
    V, F = np.asarray(V, np.float64), np.asarray(F, np.int64)
    n = int(F.max()) + 1
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    directed = e[:, 0] * n + e[:, 1]
    undirected = e.min(1) * n + e.max(1)
    _, cu = np.unique(undirected, return_counts=True)
    _, cd = np.unique(directed, return_counts=True)
    p = V[F]
    area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    return {"closed": bool((cu == 2).all()), "oriented": bool((cd == 1).all()), "chi": int(np.unique(F).size - cu.size + F.shape[0]),
            "volume": float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0), "degenerate": int((area2 == 0).sum())}


def assert_closed_sphere(V, F, what=""):
    r = mesh_report(V, F)
    assert r["closed"] and r["oriented"] and r["chi"] == 2 and r["volume"] > 0, (what, r)
    return r


# ---- 1: extraction on an exact field --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [48, 96])
def test_marching_tetrahedra_on_sphere_distance_field(N):
    from dgs_amd.mesh import TSDFVolume
    origin, h = sphere_box(N)
    vol = TSDFVolume(origin, h, (N, N, N), "cpu")
    ax = [np.float64(vol.origin[i]) + np.float64(vol.voxel_size) * np.arange(N) for i in range(3)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    vol.tsdf = torch.tensor(np.linalg.norm(G - C_S, axis=-1) - R_S, dtype=torch.float32)
    vol.weight = torch.ones_like(vol.tsdf)
    v, f, c = vol.extract()
    V, F = v.numpy(), f.numpy()
    assert V.dtype == np.float32 and F.dtype == np.int32 and c.shape == V.shape
    r = assert_closed_sphere(V, F)
    assert r["degenerate"] == 0, r
    h = vol.voxel_size
    eps = 3 * h * h / (8 * R_S)
    dist = np.abs(np.linalg.norm(V.astype(np.float64) - C_S, axis=1) - R_S)
    print("N=%d: %d vertices, %d faces, max |dist| %.4e (bound %.4e), volume %.5f" % (N, len(V), len(F), dist.max(), eps, r["volume"]))
    assert dist.max() <= eps
    assert 4 / 3 * math.pi * (R_S - 2 * eps) ** 3 <= r["volume"] <= 4 / 3 * math.pi * (R_S + eps) ** 3
    Vr, Fr, keys = marching_tets_reference(vol.tsdf.numpy(), vol.weight.numpy(), vol.origin, vol.voxel_size)
    assert (np.diff(keys) > 0).all()
    assert np.array_equal(F, Fr) and np.array_equal(V, Vr)


def test_marching_tetrahedra_skips_unobserved_cells_and_is_empty_without_a_crossing():
    from dgs_amd.mesh import TSDFVolume
    vol = TSDFVolume((0.0, 0.0, 0.0), 0.1, (6, 5, 4), "cpu")
    vol.tsdf = torch.full(vol.dims, 0.5)
    vol.weight = torch.ones(vol.dims)
    v, f, c = vol.extract()
    assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    vol.tsdf[2, 2, 1] = -0.5                  # one negative grid point: a closed surface around it ...
    v, f, _ = vol.extract()
    assert_closed_sphere(v.numpy(), f.numpy())
    Vr, Fr, _ = marching_tets_reference(vol.tsdf.numpy(), vol.weight.numpy(), vol.origin, vol.voxel_size)
    assert np.array_equal(f.numpy(), Fr) and np.array_equal(v.numpy(), Vr)
    vol.weight[3, 3, 2] = 0.0                 # ... which opens where a corner of its cells was never observed
    v2, f2, _ = vol.extract()
    assert 0 < f2.shape[0] < f.shape[0] and not mesh_report(v2.numpy(), f2.numpy())["closed"]
    Vr, Fr, _ = marching_tets_reference(vol.tsdf.numpy(), vol.weight.numpy(), vol.origin, vol.voxel_size)
    assert np.array_equal(f2.numpy(), Fr) and np.array_equal(v2.numpy(), Vr)


# ---- 2: fusion against a plain loop ---------------------------------------------------------------------------------------------
def fuse_loop(origin, h, dims, depth, rgb, proj, trunc, depth_trunc, prior_weight=0.0):
    """Voxel by voxel, view by view, in Python floats (float64): the five steps of include/dgs_mesh_ops.h."""
    Nx, Ny, Nz = dims
    V, H, W = depth.shape
    tsdf = np.full(dims, 1.0 if prior_weight > 0 else 0.0)
    wgt = np.full(dims, float(prior_weight))
    col = np.zeros(dims + (3,))
    for i in range(Nx):
        for j in range(Ny):
            for k in range(Nz):
                p = (origin[0] + h * i, origin[1] + h * j, origin[2] + h * k)
                for v in range(V):
                    m = proj[v].reshape(4, 4)
                    hx, hy, z = (p[0] * m[0, c] + ((p[1] * m[1, c] + p[2] * m[2, c]) + m[3, c]) for c in (0, 1, 3))
                    if not z > 0:
                        continue
                    nx, ny = hx / z, hy / z
                    if not (-1 < nx < 1 and -1 < ny < 1):
                        continue
                    u, vv = ((nx + 1) * W - 1) / 2, ((ny + 1) * H - 1) / 2
                    u0, v0 = min(max(math.floor(u), 0), W - 2), min(max(math.floor(vv), 0), H - 2)
                    fu, fv = min(max(u - u0, 0.0), 1.0), min(max(vv - v0, 0.0), 1.0)
                    taps = [depth[v, v0, u0], depth[v, v0, u0 + 1], depth[v, v0 + 1, u0], depth[v, v0 + 1, u0 + 1]]
                    if not all(0 < t <= depth_trunc for t in taps):
                        continue
                    bil = lambda q: (q[0] * (1 - fu) + q[1] * fu) * (1 - fv) + (q[2] * (1 - fu) + q[3] * fu) * fv
                    sdf = bil(taps) - z
                    if not sdf > -trunc:
                        continue
                    s = min(max(sdf / trunc, -1.0), 1.0)
                    w = wgt[i, j, k]
                    tsdf[i, j, k] = (tsdf[i, j, k] * w + s) / (w + 1)
                    if sdf < trunc:
                        for ch in range(3):
                            img = rgb[v, ch]
                            col[i, j, k, ch] = (col[i, j, k, ch] * w + bil([img[v0, u0], img[v0, u0 + 1], img[v0 + 1, u0], img[v0 + 1, u0 + 1]])) / (w + 1)
                    wgt[i, j, k] = w + 1
    return tsdf, wgt, col


@pytest.mark.parametrize("prior_weight", [0.0, 1.0])
def test_vectorised_fuser_equals_plain_loop(prior_weight):
    from dgs_amd.mesh import TSDFVolume
    W, H, N = 20, 16, 12
    origin, h = (-0.6, -0.55, -0.5), 0.1
    cams = [make_camera(pose_spherical(30.0, -40.0, 3.0), FOV, FOV, W, H, 0.0),
            make_camera(pose_spherical(-100.0, 20.0, 0.2), 1.2, 1.2, W, H, 0.0),        # inside the box
            make_camera(pose_spherical(160.0, -10.0, 3.0), FOV, FOV, W, H, 0.0)]         # sees nothing (all depths 0)
    g = np.random.default_rng(5)
    depth = g.uniform(2.4, 3.4, (3, H, W))
    depth[0][g.uniform(size=(H, W)) < 0.15] = 0.0
    depth[0, 3, 4] = 7.0                                                                 # beyond depth_trunc
    depth[1] = g.uniform(0.05, 0.6, (H, W))
    depth[2] = 0.0
    rgb = g.uniform(size=(3, 3, H, W))
    proj = np.stack([c.full_proj_transform.double().numpy().reshape(16) for c in cams])
    trunc = 2.5 * h
    vol = TSDFVolume(origin, h, (N, N, N), "cpu", prior_weight=prior_weight, dtype=torch.float64)
    vol.integrate(torch.tensor(depth), torch.tensor(rgb), torch.tensor(proj), trunc=trunc, depth_trunc=6.0)
    t, w, c = fuse_loop(origin, h, (N, N, N), depth, rgb, proj, trunc, 6.0, prior_weight)
    counts = w - prior_weight
    print("accepted voxel-views per view count:", np.unique(counts, return_counts=True))
    assert counts.max() == 2 and (counts == 0).any() and (counts == 1).any()            # the third camera adds nothing
    assert np.array_equal(vol.weight.numpy(), w)
    assert np.abs(vol.tsdf.numpy() - t).max() <= 1e-12
    assert np.abs(vol.color.numpy() - c).max() <= 1e-12
    # fed view by view, the volume ends bit-identical
    vol2 = TSDFVolume(origin, h, (N, N, N), "cpu", prior_weight=prior_weight, dtype=torch.float64)
    for v in range(3):
        vol2.integrate(torch.tensor(depth[v:v + 1]), torch.tensor(rgb[v:v + 1]), torch.tensor(proj[v:v + 1]), trunc=trunc, depth_trunc=6.0)
    assert torch.equal(vol2.tsdf, vol.tsdf) and torch.equal(vol2.weight, vol.weight) and torch.equal(vol2.color, vol.color)


# ---- 3: fused sphere ------------------------------------------------------------------------------------------------------------
def test_sphere_fused_from_analytic_depth_maps():
    from dgs_amd.mesh import TSDFVolume
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = fusion_inputs(24, 200)
    vol = TSDFVolume(origin, h, (N, N, N), "cpu").integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    h = vol.voxel_size
    v, f, c = vol.extract()
    V, F = v.numpy(), f.numpy()
    assert_closed_sphere(V, F)
    dist = np.abs(np.linalg.norm(V.astype(np.float64) - C_S, axis=1) - R_S) / h
    print("fused sphere: %d vertices, %d faces, distance max %.3f h, p95 %.3f h" % (len(V), len(F), dist.max(), np.quantile(dist, 0.95)))
    assert dist.max() <= 1.0
    assert c.min() >= 0.0 and c.max() <= 1.0 and float(c.std()) > 0.01
    # a voxel no view accepted has weight 0: deeper inside the sphere than the truncation, every view measures sdf < -trunc
    ax = [vol.origin[i] + h * np.arange(N) for i in range(3)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    deep = np.linalg.norm(G - C_S, axis=-1) < R_S - 6 * h - h
    w = vol.weight.numpy()
    assert deep.sum() > 1000 and (w[deep] == 0).all() and (w == np.round(w)).all() and w.max() <= 24
    # ... and no triangle touches one: both ends of every vertex's edge were observed
    Vr, Fr, keys = marching_tets_reference(vol.tsdf.numpy(), w, vol.origin, vol.voxel_size)
    assert np.array_equal(F, Fr) and np.array_equal(V, Vr)
    la, d = keys // 7, keys % 7 + 1
    lb = la + (d & 1) * N * N + (d >> 1 & 1) * N + (d >> 2 & 1)
    assert (w.reshape(-1)[la] > 0).all() and (w.reshape(-1)[lb] > 0).all()


# ---- 4: component filter, mesh PLY ----------------------------------------------------------------------------------------------
def two_spheres():
    from dgs_amd.mesh import TSDFVolume
    N = 40
    vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (N - 1), (N, N, N), "cpu")
    ax = [vol.origin[i] + vol.voxel_size * np.arange(N) for i in range(3)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    big = np.linalg.norm(G - np.array([0.3, 0.2, 0.1]), axis=-1) - 0.5
    small = np.linalg.norm(G - np.array([-0.62, -0.6, -0.55]), axis=-1) - 0.22
    vol.tsdf = torch.tensor(np.minimum(big, small), dtype=torch.float32)
    vol.weight = torch.ones_like(vol.tsdf)
    vol.color = torch.tensor(np.clip(G * 0.5 + 0.5, 0, 1), dtype=torch.float32)
    return vol.extract()


def test_component_filter_keeps_the_larger_sphere():
    from dgs_amd.mesh import keep_largest_components, vertex_components
    v, f, c = two_spheres()
    labels = vertex_components(v.shape[0], f.numpy())
    assert np.unique(labels).size == 2
    v1, f1, c1 = keep_largest_components(v, f, c, n_keep=1)
    assert 0 < v1.shape[0] < v.shape[0] and c1.shape == v1.shape
    assert int(f1.min()) == 0 and int(f1.max()) == v1.shape[0] - 1 and np.unique(f1.numpy()).size == v1.shape[0]
    assert_closed_sphere(v1.numpy(), f1.numpy())
    centre = v1.numpy().mean(0)
    assert np.abs(centre - np.array([0.3, 0.2, 0.1])).max() < 0.02
    # geometry and colours travel with the renumbering
    big = np.flatnonzero(np.linalg.norm(v.numpy() - np.array([0.3, 0.2, 0.1]), axis=1) < 0.6)
    assert np.array_equal(v.numpy()[big], v1.numpy()) and np.array_equal(c.numpy()[big], c1.numpy())
    # n_keep = 2 keeps both; min_faces above the small sphere's size drops it again
    v2, f2, _ = keep_largest_components(v, f, c, n_keep=2)
    assert v2.shape == v.shape and f2.shape == f.shape
    small_faces = f.shape[0] - f1.shape[0]
    v3, f3, _ = keep_largest_components(v, f, c, n_keep=1000, min_faces=small_faces + 1)
    assert f3.shape == f1.shape
    v4, f4, _ = keep_largest_components(v, f, c, n_keep=1000, min_faces=50)
    assert f4.shape == f.shape


def test_mesh_ply_round_trip(tmp_path):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    v, f, c = two_spheres()
    path = str(tmp_path / "sub" / "mesh.ply")
    write_mesh_ply(path, v, f, c)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n") + len(b"end_header\n")].decode("ascii").split("\n")
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0], "property float x", "property float y",
                    "property float z", "property uchar red", "property uchar green", "property uchar blue", "element face %d" % f.shape[0],
                    "property list uchar int vertex_indices", "end_header", ""]
    assert len(raw) == len("\n".join(head)) + v.shape[0] * 15 + f.shape[0] * 13
    v2, f2, c2 = read_mesh_ply(path)
    assert v2.dtype == np.float32 and f2.dtype == np.int32
    assert np.array_equal(v2, v.numpy()) and np.array_equal(f2, f.numpy())
    assert np.abs(c2 - c.numpy()).max() <= 0.5 / 255 + 1e-7
    write_mesh_ply(path, v, f)                       # without colours
    v3, f3, c3 = read_mesh_ply(path)
    assert c3 is None and np.array_equal(v3, v.numpy()) and np.array_equal(f3, f.numpy())
    with pytest.raises(ValueError):
        write_mesh_ply(path, v[:10], f)


def test_bounds_from_surfels():
    from dgs_amd.mesh import TSDFVolume, bounds_from_surfels
    g = torch.Generator().manual_seed(0)
    xyz = torch.rand(5000, 3, generator=g) * torch.tensor([2.0, 1.0, 0.5]) - torch.tensor([1.0, 0.5, 0.25])
    xyz[0] = torch.tensor([50.0, 50.0, 50.0])       # an outlier does not blow the box up
    lo, hi = bounds_from_surfels(xyz, 0.01, 0.1)
    assert all(-1.12 < l < -0.1 for l in lo[:1]) and hi[0] < 1.12 and hi[2] < 0.36
    vol = TSDFVolume.from_bounds(lo, hi, 0.05)
    assert all(vol.origin[i] + vol.voxel_size * (vol.dims[i] - 1) >= hi[i] - 1e-6 for i in range(3))
