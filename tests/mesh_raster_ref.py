"""Inputs, float64 brute force and a-priori exclusion set shared by tests/test_mesh_render_cpu.py and tests/test_mesh_render_gpu.py:
what the rasterizer of dgs_amd.mesh_render is measured against.

The brute force is NOT the statement under test in another precision: it projects with a matrix product, uses the textbook edge
functions E_k(P) = cross(v_{k+2} - v_{k+1}, P - v_{k+1}) in the face's own vertex order (no canonical edge order, no pixel box),
normalises by the signed area and takes all faces against all pixels in float64 NumPy.

THE EXCLUSION SET is decided from float64 alone, before any fp32 number exists.  A pixel is excluded when
  (a) some face has a barycentric within EDGE_BAND = 1e-4 of zero there while its other two are >= -EDGE_BAND: fp32 may put the
      pixel centre on either side of that edge; or
  (b) its two nearest depths differ by less than DEPTH_BAND = 1e-5 relative: fp32 may order them either way.
Every case handed out is checked to exclude at most 1 % of its covered pixels: a condition on the inputs, not on the code."""
import functools

import numpy as np
import torch

from test_mesh_metrics_cpu import uv_sphere

U32 = 2.0 ** -24
EDGE_BAND, DEPTH_BAND, MAX_EXCLUDED = 1e-4, 1e-5, 0.01
NEAR = 0.01


# ---- cameras and meshes ---------------------------------------------------------------------------------------------------------
def orbit_camera(H, W, theta=30.0, phi=-30.0, radius=4.0, fov=0.6911):
    from dgs_amd.cameras import make_camera, pose_spherical
    focal = W / (2 * np.tan(fov / 2))
    return make_camera(pose_spherical(theta, phi, radius), fov, 2 * np.arctan(H / (2 * focal)), W, H, 0.0)


def pixel_camera(H, W):
    """A camera whose screen point of (x, y, z) is (x, y) and whose view depth is z: meshes can be written in pixels."""
    from dgs_amd.cameras import Camera
    m = torch.zeros(4, 4)
    m[0, 0], m[2, 0] = 2.0 / W, 1.0 / W - 1.0          # hom_0 = x 2/W + z (1/W - 1), w = z: at z = 1 sx = x up to rounding
    m[1, 1], m[2, 1] = 2.0 / H, 1.0 / H - 1.0
    m[2, 3] = 1.0
    return Camera(H, W, 1.0, 1.0, torch.eye(4), m, torch.zeros(3), torch.zeros(1))


def sphere(nu=32, nv=16, radius=0.8, centre=(0.05, -0.1, 0.02)):
    """UV sphere (2 nu (nv - 1) faces), colours a smooth function of the normal."""
    v, f = uv_sphere(radius, centre, nu, nv)
    v, f = torch.from_numpy(v), torch.from_numpy(f).long()
    n = (v - torch.tensor(centre)) / radius
    return v, f, (0.5 + 0.45 * torch.sin(3.0 * n + torch.tensor([0.0, 2.0, 4.0]))).float()


def quad(H, W, z=2.0):
    """Two triangles larger than the image, in the pixel camera's coordinates at depth z (x, y scaled by z: hom / w gives pixels)."""
    x0, x1, y0, y1 = -0.75 * W, 1.8 * W + 0.5, -1.25 * H - 0.5, 2.1 * H
    v = torch.tensor([[x0, y0, 1.0], [x1, y0, 1.0], [x1, y1, 1.0], [x0, y1, 1.0]]) * z
    c = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    return v, torch.tensor([[0, 1, 2], [0, 2, 3]]), c


def needle_fan(H, W, n=40, z=1.5):
    """A fan of n needle triangles around a hub left of the image centre: apex angle 1.2 / n radians each, legs about 0.45 of the
    smaller image side, depth rising along the fan (pixel camera coordinates)."""
    hub = np.array([0.31 * W + 0.137, 0.47 * H + 0.291])
    leg = 0.45 * min(H, W)
    ang = -0.6 + 1.2 * np.arange(n + 1) / n + 0.0123
    rim = hub[None] + leg * np.stack([np.cos(ang), np.sin(ang)], 1) * (1.0 + 0.07 * np.sin(5.0 * np.arange(n + 1)))[:, None]
    depth = np.concatenate([[z], z * (1.0 + 0.3 * np.arange(n + 1) / n)])
    xy = np.concatenate([hub[None], rim])
    v = torch.from_numpy(np.concatenate([xy * depth[:, None], depth[:, None]], 1)).float()
    f = torch.tensor([[0, 1 + i, 2 + i] for i in range(n)])
    g = torch.Generator().manual_seed(7)
    return v, f, torch.rand(v.shape[0], 3, generator=g)


def overflowing_face():
    """A legal face (finite corners, in front of the camera, A = +inf) in the pixel camera's coordinates whose edge 0 has one product
    beyond fp32 at every pixel of a small image: e_0 = +inf, S = +inf, b_0 = inf / inf = NaN, so q and z are NaN while the three
    sign tests pass.  Such a pixel is not covered (q > 0 fails)."""
    return torch.tensor([[-10.0, 50.0, 1.0], [0.0, -1e14, 1.0], [1e25, 0.0, 1.0]]), torch.tensor([[0, 1, 2]])


def unweld(v, f, c=None):
    """Every face gets its own three vertices."""
    idx = f.reshape(-1)
    return v[idx].contiguous(), torch.arange(idx.numel()).reshape(-1, 3), None if c is None else c[idx].contiguous()


# ---- float64 brute force --------------------------------------------------------------------------------------------------------
def brute_force64(vertices, faces, camera, colors=None, near=NEAR, chunk=128):
    """-> dict of float64 / int arrays over the H x W pixels: face (-1 = nothing), depth, bary [H,W,3], color [H,W,C], excluded
    (bool), h_min (the winner's smallest height in pixels), second (the second nearest depth, inf if none)."""
    H, W = int(camera.image_height), int(camera.image_width)
    v = vertices.detach().cpu().double().numpy()
    f = faces.detach().cpu().long().numpy()
    m = camera.full_proj_transform.detach().cpu().double().numpy()
    hom = np.concatenate([v, np.ones((v.shape[0], 1))], 1) @ m
    w = hom[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.stack([((hom[:, 0] / w + 1) * W - 1) / 2, ((hom[:, 1] / w + 1) * H - 1) / 2], 1)
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    P = np.stack([px.reshape(-1), py.reshape(-1)], 1)                       # [N, 2]
    N = P.shape[0]
    best, second = np.full(N, np.inf), np.full(N, np.inf)
    face = np.full(N, -1, dtype=np.int64)
    bary = np.zeros((N, 3))
    band = np.zeros(N, dtype=bool)
    cross = lambda a, b: a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    for s0 in range(0, f.shape[0], chunk):
        fc = f[s0:s0 + chunk]
        T = s[fc]                                                           # [F, 3, 2]
        wc = w[fc]
        area = cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
        ok = (wc > near).all(1) & np.isfinite(T).all((1, 2)) & (area != 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = np.stack([cross((T[:, (k + 2) % 3] - T[:, (k + 1) % 3])[:, None], P[None] - T[:, (k + 1) % 3][:, None]) for k in range(3)], -1) / area[:, None, None]
            z = 1.0 / (b / wc[:, None, :]).sum(-1)                          # [F, N]
        cov = ok[:, None] & (b >= 0).all(-1)
        band |= (ok[:, None] & (b >= -EDGE_BAND).all(-1) & (np.abs(b) <= EDGE_BAND).any(-1)).any(0)
        zc = np.where(cov, z, np.inf)
        first = np.argmin(zc, axis=0)                                       # the first occurrence: the lowest face among equal depths
        z1 = zc[first, np.arange(N)]
        zc[first, np.arange(N)] = np.inf
        z2 = zc.min(axis=0)
        better = z1 < best
        second = np.where(better, np.minimum(best, z2), np.minimum(second, z1))
        bary = np.where(better[:, None], b[first, np.arange(N)], bary)
        face = np.where(better, s0 + first, face)
        best = np.where(better, z1, best)
    hit = face >= 0
    with np.errstate(invalid="ignore"):
        close = hit & np.isfinite(second) & (second - best < DEPTH_BAND * best)
    out = {"face": face.reshape(H, W), "depth": np.where(hit, best, 0.0).reshape(H, W), "bary": np.where(hit[:, None], bary, 0.0).reshape(H, W, 3),
           "excluded": (band | close).reshape(H, W), "second": second.reshape(H, W)}
    T = s[f[np.maximum(face, 0)]]                                           # the winners' corners [N, 3, 2]
    edge = np.stack([np.linalg.norm(T[:, (k + 2) % 3] - T[:, (k + 1) % 3], axis=-1) for k in range(3)], -1)
    area = np.abs(cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        out["h_min"] = np.where(hit, area / edge.max(-1), np.inf).reshape(H, W)
    out["coord"] = float(np.abs(T[hit]).max()) if hit.any() else 0.0       # largest screen coordinate among the winners' corners
    if colors is not None:
        c = colors.detach().cpu().double().numpy()[f[np.maximum(face, 0)]]  # [N, 3, C]
        wgt = bary / w[f[np.maximum(face, 0)]]
        with np.errstate(divide="ignore", invalid="ignore"):
            col = (wgt[:, :, None] * c).sum(1) / wgt.sum(1, keepdims=True)
        out["color"] = np.where(hit[:, None], col, 0.0).reshape(H, W, -1)
    return out


def check_case(name, ref):
    """The condition on the inputs: at most 1 % of the covered pixels are excluded."""
    covered = ref["face"] >= 0
    n_cov, n_exc = int(covered.sum()), int((ref["excluded"] & covered).sum())
    assert n_cov > 0, "%s: nothing covered" % name
    assert n_exc <= MAX_EXCLUDED * n_cov, "%s: %d of %d covered pixels are excluded: change the inputs, not the cap" % (name, n_exc, n_cov)
    return n_cov, n_exc


SIZES = ((96, 96), (37, 53))


@functools.lru_cache(maxsize=None)
def case(name, H, W):
    """(camera, vertices, faces, colors, float64 reference) of a named case at H x W, on the CPU, computed once and shared."""
    if name in ("sphere", "sphere unwelded", "sphere coarse"):
        cam = orbit_camera(H, W)
        v, f, c = sphere(16, 8) if name == "sphere coarse" else sphere()
        if name == "sphere unwelded":
            v, f, c = unweld(v, f, c)
    elif name == "quad":
        cam = pixel_camera(H, W)
        v, f, c = quad(H, W)
    elif name == "needles":
        cam = pixel_camera(H, W)
        v, f, c = needle_fan(H, W)
    else:
        raise KeyError(name)
    ref = brute_force64(v, f, cam, c)
    check_case("%s %dx%d" % (name, H, W), ref)
    return cam, v, f, c, ref


CASES = ("sphere", "sphere unwelded", "sphere coarse", "quad", "needles")


def compare_with_float64(name, out, image, ref, W, H):
    """The rules of the fp32-vs-float64 comparison, outside the exclusion set: identical coverage and face ids; depth within
    32 * 2^-24 relative; barycentrics and colours within the conditioning bound below.  `out` is the rasterizer's dict of tensors
    ("face", "depth", "bary"), image [C,H,W] the interpolated colours (0 background).

    Barycentric bound: a screen coordinate of magnitude <= M carries the roundings of its projection (two products, three sums, a
    division, the map to pixels), delta <= 2 * 2^-24 * M after cancellations; an edge function then moves by about delta * (edge
    length) and a barycentric e_k / (2 area) by delta / h_k, h_k the face's height over that edge in pixels:
    |db| <= 4 * delta / h_min (factor 4: both endpoints and the pixel difference of an edge function, and S in the quotient).
    Colours (|a| <= 1, the perspective weights of one face within a factor ~ 1 of each other) move by at most 3 |db| + 16 * 2^-24."""
    keep = ~ref["excluded"]
    face = out["face"].cpu().numpy().astype(np.int64)
    assert np.array_equal(face[keep] >= 0, ref["face"][keep] >= 0), "%s: coverage differs outside the exclusion set" % name
    assert np.array_equal(face[keep], ref["face"][keep]), "%s: face ids differ outside the exclusion set" % name
    hit = keep & (ref["face"] >= 0)
    depth = out["depth"].cpu().double().numpy()
    rel = np.abs(depth[hit] - ref["depth"][hit]) / ref["depth"][hit]
    M = max(W, H, ref["coord"])
    tol_b = 4 * (2 * U32 * M) / ref["h_min"][hit]
    db = np.abs(out["bary"].cpu().double().numpy()[hit] - ref["bary"][hit]).max(-1)
    dc = np.abs(image.cpu().double().numpy().transpose(1, 2, 0)[hit] - ref["color"][hit]).max(-1)
    print("%s: %d pixels compared (%d excluded); depth max rel %.3e (cap %.3e); bary max %.3e, max ratio to its bound %.3f; colour max %.3e, "
          "max ratio to its bound %.3f" % (name, int(hit.sum()), int((ref["excluded"] & (ref["face"] >= 0)).sum()), rel.max(), 32 * U32, db.max(),
                                           (db / tol_b).max(), dc.max(), (dc / (3 * tol_b + 16 * U32)).max()))
    assert bool((depth[keep & (ref["face"] < 0)] == 0).all())
    assert rel.max() <= 32 * U32, "%s: depth" % name
    assert bool((db <= tol_b).all()), "%s: barycentrics" % name
    assert bool((dc <= 3 * tol_b + 16 * U32).all()), "%s: colours" % name
