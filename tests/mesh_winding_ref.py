"""Inputs, float64 brute force and tolerance shared by tests/test_mesh_winding_cpu.py, tests/test_mesh_winding_gpu.py and
tools/mesh_winding_margins.py: what the winding number of dgs_amd.mesh_metrics is measured against.

The brute force is NOT the statement under test in another precision: it is van Oosterom and Strackee's formula in its textbook
form -- the triple product a . (b x c) over |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b| -- in float64 with torch.atan2, on the same
fp32 inputs, summed in float64.

The tolerance is absolute, on W, and there are two, each 4 x the largest |W32 - W64| over ALL queries of its input sets, the
fp32 side being the PyTorch statement on the CPU (never the kernel):
  W_TOL       = 4 * W_MEASURED        the shape sets and the cap (cpu_sets minus the soups): queries at a distance from the surface
  W_TOL_SOUP  = 4 * W_MEASURED_SOUP   the soups of cpu_sets and every gpu_cases shape: a third of their queries lie within 0.02 of a
                                      face, where num = a . n is a small difference of large terms, and slivers abound
tools/mesh_winding_margins.py measures both and writes profiles/mesh_winding_margins.md.  The fp32 side is bit-defined (integer
sums, the same on every device), so the factor 4 only covers another libm's or a device's rounding of the float64 side.
POLY_MEASURED is the largest error of the atan polynomial, evaluated in fp32, against float64 atan on a dense sweep of r in [0, 1]
(the same tool).

Every query of the shape sets is BUILT at a distance from the surface (offsets of OFFSET along +- a face's normal from its centroid;
box points pushed out of a shell of half-width SHELL around the analytic surface), so none needs excluding.  The soups' queries
are mesh_surface_ref.queries: a third of them within 0.02 of a face, none exactly in one."""
import functools
import math

import torch

import mesh_surface_ref as surface

W_MEASURED, W_MEASURED_SOUP = 1.1e-07, 2.1e-05     # profiles/mesh_winding_margins.md
W_TOL, W_TOL_SOUP = 4.0 * W_MEASURED, 4.0 * W_MEASURED_SOUP
POLY_MEASURED = 1.3e-07                            # rad; profiles/mesh_winding_margins.md
OFFSET, SHELL, BOX = 0.05, 0.1, 1.6
TORUS_R, TORUS_r = 0.7, 0.3


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def icosphere(level, radius=1.0):
    """(vertices [Nv,3] float32, faces [20 * 4^level, 3] int64) of the subdivided icosahedron on the sphere, wound outward."""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [tuple(x / math.sqrt(1 + p * p) for x in q) for q in v]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = [(a + b) / 2 for a, b in zip(v[i], v[j])]
                n = math.sqrt(sum(x * x for x in m))
                v.append(tuple(x / n for x in m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (torch.tensor(v, dtype=torch.float64) * radius).float().contiguous(), torch.tensor(f, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def torus(nu=64, nv=32, R=TORUS_R, r=TORUS_r):
    """(vertices [nu nv, 3] float32, faces [2 nu nv, 3] int64) of a torus around the z axis, wound outward."""
    u = 2 * math.pi * torch.arange(nu, dtype=torch.float64) / nu
    w = 2 * math.pi * torch.arange(nv, dtype=torch.float64) / nv
    rho = R + r * torch.cos(w)[None, :]
    v = torch.stack([rho * torch.cos(u)[:, None], rho * torch.sin(u)[:, None], (r * torch.sin(w))[None, :].expand(nu, nv)], -1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(nu), torch.arange(nv), indexing="ij")
    vid = lambda i, j: ((i % nu) * nv + (j % nv)).reshape(-1)
    f = torch.cat([torch.stack([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], 1), torch.stack([vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)], 1)])
    return v.float().contiguous(), f


def flipped(mesh):
    v, f = mesh
    return v, f[:, [0, 2, 1]].contiguous()


def nested():
    """Two equally wound icospheres (level 3), radii 1 and 0.5, as one mesh."""
    (v1, f1), (v2, f2) = icosphere(3), icosphere(3, 0.5)
    return torch.cat([v1, v2]), torch.cat([f1, f2 + v1.shape[0]])


def cap(mesh, direction=(0.2, 0.45, 0.87)):
    """The faces of a centrally symmetric mesh whose centroid lies on the positive side of a plane through the centre: of every
    antipodal pair of faces exactly one, so the cap subtends exactly half of everything seen from the centre.  The plane must keep
    clear of every centroid, by far more than any rounding of the dot product (checked: at least 1e-4; 1.7e-3 for the level-3
    icosphere and this direction), so every machine selects the same faces; (0.3, -0.5, 0.8) passes through one."""
    v, f = mesh
    m = v.double()[f].mean(1)
    c = m[:, 0] * direction[0] + m[:, 1] * direction[1] + m[:, 2] * direction[2]
    assert float(c.abs().min()) > 1e-4 and int((c > 0).sum()) * 2 == f.shape[0]
    return v, f[c > 0].contiguous()


# ---- queries --------------------------------------------------------------------------------------------------------------------
def offsets(mesh, stride=1, offset=OFFSET):
    """Centroids of every stride-th face moved by +offset and by -offset along the face's unit normal (float64, then fp32)
    -> (points [2 n, 3], outside [2 n] bool: the +offset half)."""
    v, f = mesh
    t = v.double()[f[::stride]]
    n = torch.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], dim=1)
    n = n / n.norm(dim=1, keepdim=True)
    c = t.mean(1)
    k = c.shape[0]
    return torch.cat([c + offset * n, c - offset * n]).float().contiguous(), torch.arange(2 * k) < k


def _box(n, seed, half):
    return (torch.rand(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * torch.tensor(half, dtype=torch.float64)


def sphere_box(n, seed, radius=1.0):
    """n points uniform in the box BOX x the sphere, those within SHELL of it moved radially to SHELL from it
    -> (points fp32, inside bool).  The polyhedral sphere lies within its sagitta (0.4 % at level 3) of the analytic one."""
    p = _box(n, seed, (BOX * radius,) * 3)
    d = p.norm(dim=1, keepdim=True)
    sd = d - radius
    near = sd.abs() < SHELL
    p = torch.where(near, p / d * (radius + torch.where(sd >= 0, SHELL, -SHELL)), p)
    return p.float().contiguous(), (p.norm(dim=1) < radius)


def torus_box(n, seed, R=TORUS_R, r=TORUS_r):
    """The same for the torus: the signed distance is |(rho - R, z)| - r in the plane through the axis."""
    p = _box(n, seed, (BOX * (R + r), BOX * (R + r), BOX * r))
    rho = (p[:, 0] ** 2 + p[:, 1] ** 2).sqrt()
    e = torch.stack([rho - R, p[:, 2]], 1)
    t = e.norm(dim=1)
    sd = t - r
    near = sd.abs() < SHELL
    e2 = e / t[:, None] * (r + torch.where(sd >= 0, SHELL, -SHELL))[:, None]
    rho2 = R + e2[:, 0]
    moved = torch.stack([p[:, 0] / rho * rho2, p[:, 1] / rho * rho2, e2[:, 1]], 1)
    p = torch.where(near[:, None], moved, p)
    rho = (p[:, 0] ** 2 + p[:, 1] ** 2).sqrt()
    return p.float().contiguous(), ((rho - R) ** 2 + p[:, 2] ** 2).sqrt() < r


def shells(n, seed, radii):
    """n random directions at each of the radii -> points [len(radii) n, 3] fp32, radius by radius."""
    d = torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([d * r for r in radii]).float().contiguous()


# ---- float64 brute force --------------------------------------------------------------------------------------------------------
def brute_force64(points, vertices, faces, chunk=256):
    """W [Nq] float64 of the mesh at the points, all pairs, torch.atan2."""
    p, v = points.detach().cpu().double(), vertices.detach().cpu().double()
    t = v[faces.detach().cpu().long()]
    out = torch.empty(p.shape[0], dtype=torch.float64)
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        a, b, c = t[None, :, 0] - q, t[None, :, 1] - q, t[None, :, 2] - q
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = (a * torch.cross(b, c, dim=-1)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out[s:s + chunk] = torch.atan2(num, den).sum(1) / (2 * math.pi)
    return out


def statement32(points, vertices, faces):
    """W [Nq] float64 from the PyTorch statement in fp32 on the CPU."""
    from dgs_amd.mesh_metrics import winding_number
    return winding_number(points.float().cpu(), vertices.float().cpu(), faces.cpu())


def measure(points, vertices, faces):
    """Largest |W32 - W64| over the queries."""
    return float((statement32(points, vertices, faces) - brute_force64(points, vertices, faces)).abs().max())


def polynomial_error(n=2_000_001):
    """Largest |p(r) - atan(r)| for r = k / (n - 1), p the statement's polynomial evaluated in fp32, atan in float64."""
    from dgs_amd.mesh_metrics import _wind_atan2
    r = torch.linspace(0, 1, n, dtype=torch.float64).float()
    return float((_wind_atan2(r, torch.ones_like(r)).double() - torch.atan(r.double())).abs().max())


# ---- the input sets ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_set(name):
    """(points, vertices, faces, expected W as integers [Nq]) of one named shape set, on the CPU."""
    if name in ("icosphere 3", "icosphere 3 flipped", "icosphere 5", "icosphere 5 flipped"):
        level = int(name.split()[1])
        mesh = icosphere(level)
        p, out = offsets(mesh, 1 if level == 3 else 128)
        b, inside = sphere_box(500 if level == 3 else 100, 70 + level)
        want = torch.cat([(~out).long(), inside.long()])
        p = torch.cat([p, b])
    elif name in ("torus 64x32", "torus 64x32 flipped"):
        mesh = torus()
        p, out = offsets(mesh, 8)
        b, inside = torus_box(300, 81)
        want = torch.cat([(~out).long(), inside.long()])
        p = torch.cat([p, b])
    elif name == "nested spheres":
        mesh = nested()
        p = shells(60, 91, (0.2, 0.4, 0.75, 1.3))
        want = torch.tensor([2, 2, 1, 0]).repeat_interleave(60)
    else:
        raise KeyError(name)
    if name.endswith("flipped"):
        mesh, want = flipped(mesh), -want
    return p.contiguous(), mesh[0], mesh[1], want


SHAPE_SETS = ("icosphere 3", "icosphere 3 flipped", "icosphere 5", "icosphere 5 flipped", "torus 64x32", "torus 64x32 flipped", "nested spheres")
SOUP_SETS = (("soup around 0", 0.0, 41), ("soup around 1", 1.0, 42))


def cap_set():
    """The open hemisphere cap of the level-3 icosphere and queries off its surface: the centre first (W = 1/2 there)."""
    v, f = cap(icosphere(3))
    return torch.cat([torch.zeros(1, 3), shells(40, 95, (0.5, 1.4))]).contiguous(), v, f


def soup_set(centre, seed):
    v, f = surface.soup(1200, seed, centre)
    return surface.queries(900, seed + 10, v, f, centre), v, f


def cpu_sets():
    """[(name, points, vertices, faces, soup)]: every named set of the CPU test; soup: bounded by W_TOL_SOUP, not W_TOL."""
    out = [(name,) + shape_set(name)[:3] + (False,) for name in SHAPE_SETS]
    out.append(("hemisphere cap",) + cap_set() + (False,))
    out += [(name,) + soup_set(centre, seed) + (True,) for name, centre, seed in SOUP_SETS]
    return out


# ---- the cases of the GPU test, also measured by tools/mesh_winding_margins.py --------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(nq, nf):
    """(points, vertices, faces) of one (Nq, Nf) case, on the CPU: a triangle soup and queries around it."""
    v, f = surface.soup(nf, 3000 + nf)
    return surface.queries(nq, 4000 + nq, v, f), v, f


def gpu_cases(layout):
    """Every (Nq, Nf) the GPU test runs, from dgs_winding_layout's Q, T, C: the cross of the edge sizes, ragged slices, Nf > C."""
    q, t, c = layout[:3]
    cross = [(nq, nf) for nq in (1, q - 1, q, q + 1, 3 * q + 5) for nf in (1, 2, t - 1, t, t + 1, 2 * t + 3)]
    return cross + [(q + 1, 5 * t + 7), (q + 1, c + t + 5), (7, 2 * c + 1)]
