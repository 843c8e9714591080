"""Inputs, float64 brute force and tolerance shared by tests/test_mesh_surface_cpu.py, tests/test_mesh_surface_gpu.py and
tools/mesh_surface_margins.py: what the closest-face search of dgs_amd.mesh_metrics is measured against.

The brute force is NOT the statement under test in another precision: it is the closest point of Ericson's "Real-Time Collision
Detection" (5.1.5) -- the Voronoi region of the triangle that holds the query, decided from the six dot products d1..d6 and the
three barycentric numerators va, vb, vc -- evaluated in float64 for every pair, and the distance to that point.

The tolerance of one pair is  C * 2^-24 * L * kappa  on the distance (not squared), with L the largest float64 distance from the
query to a corner and kappa = |AB| |AC| / |n| = 1 / sin(angle at A) of the face (1 for a face whose float64 normal is exactly zero:
it acts as its segments).  C_MEASURED is the largest  |d32 - d64| / (2^-24 L kappa)  over ALL pairs of every input set below, the
fp32 side being the PyTorch statement on the CPU (never the kernel); tools/mesh_surface_margins.py measures it and writes
profiles/mesh_surface_margins.md.  C = 4 * C_MEASURED: a device's elementwise code may round the last bit of an operation
differently from the CPU's, and a factor 4 covers that over the ~100 operations of a pair with room to spare."""
import functools

import numpy as np
import torch

U32 = 2.0 ** -24
C_MEASURED = 3.08          # profiles/mesh_surface_margins.md
C = 4.0 * C_MEASURED


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def soup(nf, seed, centre=0.0):
    """nf random triangles as (vertices [3 nf, 3] float32, faces [nf, 3] int64): first corners uniform in centre + [-1, 1]^3, the two
    edge vectors uniform in [-s, s]^3 with s = 1 for even faces and 0.05 for odd ones."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(nf, 3, generator=g) * 2 - 1 + centre
    s = torch.where(torch.arange(nf) % 2 == 0, 1.0, 0.05).unsqueeze(1)
    b = a + (torch.rand(nf, 3, generator=g) * 2 - 1) * s
    c = a + (torch.rand(nf, 3, generator=g) * 2 - 1) * s
    v = torch.stack([a, b, c], 1).reshape(-1, 3).float().contiguous()
    return v, torch.arange(3 * nf).reshape(nf, 3)


def queries(nq, seed, vertices, faces, centre=0.0):
    """nq points float32: two thirds uniform in centre + [-1.5, 1.5]^3, the rest within 0.02 of a random point of a random face
    (the plane branch of the statement only decides near the faces)."""
    g = torch.Generator().manual_seed(seed)
    p = (torch.rand(nq, 3, generator=g) * 3 - 1.5 + centre).float()
    k = nq // 3
    if k:
        f = faces[torch.randint(0, faces.shape[0], (k,), generator=g)]
        u = torch.rand(k, 3, generator=g)
        u = u / u.sum(1, keepdim=True)
        on = u[:, 0:1] * vertices[f[:, 0]] + u[:, 1:2] * vertices[f[:, 1]] + u[:, 2:3] * vertices[f[:, 2]]
        p[:k] = on + (torch.rand(k, 3, generator=g) * 2 - 1) * 0.02
    return p[torch.randperm(nq, generator=g)].contiguous()


def needles(per_angle=6, seed=5):
    """Needle triangles, corner angle 1e-1 ... 1e-4 at A, legs 0.1, each rotated and moved at random, with queries straight above
    them at height 0.3 (8 per needle, above random points of the needle) -> (vertices, faces, points)."""
    g = torch.Generator().manual_seed(seed)
    vs, ps = [], []
    for angle in (1e-1, 1e-2, 1e-3, 1e-4):
        for _ in range(per_angle):
            rot, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
            shift = torch.rand(3, generator=g, dtype=torch.float64) * 2 - 1
            tri = torch.tensor([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.1 * np.cos(angle), 0.1 * np.sin(angle), 0.0]], dtype=torch.float64)
            u = torch.rand(8, 3, generator=g, dtype=torch.float64)
            u = u / u.sum(1, keepdim=True)
            above = u @ tri + torch.tensor([0.0, 0.0, 0.3], dtype=torch.float64)
            vs.append(tri @ rot.T + shift)
            ps.append(above @ rot.T + shift)
    v = torch.cat(vs).float().contiguous()
    return v, torch.arange(v.shape[0]).reshape(-1, 3), torch.cat(ps).float().contiguous()


def degenerates():
    """Faces without area, every corner a small integer (their fp32 normals are exactly zero): collinear corners, three coincident
    corners, A = B, B = C, and one proper triangle far away -> (vertices, faces, points, distances) with the closed-form distance
    of every point to the NEAREST of the faces."""
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0],            # collinear
                      [3, 3, 3], [3, 3, 3], [3, 3, 3],            # a point
                      [-4, 0, 0], [-4, 0, 0], [-4, 2, 0],         # A = B: the segment (-4, 0..2, 0)
                      [0, -5, 0], [0, -5, 1], [0, -5, 1],         # B = C: the segment (0, -5, 0..1)
                      [20, 20, 20], [21, 20, 20], [20, 21, 20]], dtype=torch.float32)
    p = torch.tensor([[1, 1, 0], [3, 3, 4], [-5, 1, 0], [-4, 3, 0], [0, -5, 3], [1, -5, 0.5], [2.5, 0, 0]], dtype=torch.float32)
    return v, torch.arange(15).reshape(5, 3), p, torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0, 1.0, 0.5], dtype=torch.float64)


# ---- float64 brute force --------------------------------------------------------------------------------------------------------
def _ericson(p, a, b, c):
    """Distance of p [Q,1,3] to the triangles (a, b, c) [1,F,3], float64, by Voronoi region."""
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
        inner = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]      # NaN only for faces that brute_force64 replaces
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    shape = d1.shape + (3,)
    pts = [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + t_ab[..., None] * ab, np.broadcast_to(c, shape),
           a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b)]
    closest = inner
    for cond, pt in reversed(list(zip(conds, pts))):            # the first region that holds wins, as in the sequential code
        closest = np.where(cond[..., None], pt, closest)
    return np.sqrt(dot(p - closest, p - closest))


def _segment(p, a, b):
    e, w = b - a, p - a
    ee = (e * e).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ee > 0, np.clip((w * e).sum(-1) / ee, 0.0, 1.0), 0.0)
    c = w - t[..., None] * e
    return np.sqrt((c * c).sum(-1))


def brute_force64(points, vertices, faces, chunk=256):
    """-> (d [Nq, Nf] float64 distance of every pair, tolerance-per-C [Nq, Nf] = 2^-24 L kappa)."""
    p = points.detach().cpu().double().numpy()
    v = vertices.detach().cpu().double().numpy()
    f = faces.detach().cpu().long().numpy()
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = np.cross(b - a, c - a)
    nn = np.linalg.norm(n, axis=-1)
    flat = nn[0] == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(nn > 0, np.linalg.norm(b - a, axis=-1) * np.linalg.norm(c - a, axis=-1) / nn, 1.0)
    d = np.empty((p.shape[0], f.shape[0]))
    unit = np.empty_like(d)
    for s in range(0, p.shape[0], chunk):
        q = p[s:s + chunk, None, :]
        d[s:s + chunk] = _ericson(q, a, b, c)
        if flat.any():
            fa, fb, fc = a[:, flat], b[:, flat], c[:, flat]
            d[s:s + chunk, flat] = np.minimum(np.minimum(_segment(q, fa, fb), _segment(q, fb, fc)), _segment(q, fc, fa))
        far = np.maximum(np.maximum(np.linalg.norm(q - a, axis=-1), np.linalg.norm(q - b, axis=-1)), np.linalg.norm(q - c, axis=-1))
        unit[s:s + chunk] = U32 * far * kappa
    return torch.from_numpy(d), torch.from_numpy(unit)


def measure_c(points, vertices, faces):
    """Largest |d32 - d64| / (2^-24 L kappa) over ALL pairs, d32 from the PyTorch statement in fp32 on the CPU."""
    from dgs_amd.mesh_metrics import TRI_VALUES, _pair_d2, triangle_table
    table = triangle_table(vertices.float().cpu(), faces.cpu())
    d32 = _pair_d2(points.float().cpu(), table[:, :TRI_VALUES].t().contiguous().unsqueeze(1)).double().sqrt()
    d64, unit = brute_force64(points, vertices, faces)
    assert not bool(torch.isnan(d32).any()) and not bool(torch.isnan(d64).any())
    return float(((d32 - d64).abs() / unit).max())


def check_against_float64(d2, face, d64, unit, what=""):
    """The two bounds of a search result (d2 [Nq] of any float dtype, face [Nq]) against brute_force64's matrices:
    |d - d64(face)| <= C unit(face)  and  d64(face) <= min64 + C (unit(face) + unit(argmin64))."""
    d = d2.detach().cpu().double().sqrt()
    face = face.detach().cpu()
    at, unit_at = d64.gather(1, face[:, None])[:, 0], unit.gather(1, face[:, None])[:, 0]
    m64, arg64 = d64.min(dim=1)
    unit_min = unit.gather(1, arg64[:, None])[:, 0]
    e_d, e_arg = ((d - at).abs() / unit_at).max(), ((at - m64) / (unit_at + unit_min)).max()
    print("%s: max |d - d64(face)| / (2^-24 L kappa) = %.3f, max (d64(face) - min64) / (sum of the two) = %.3f  (cap %.2f)"
          % (what, float(e_d), float(e_arg), C))
    assert bool(((d - at).abs() <= C * unit_at).all()), "distance bound"
    assert bool((at <= m64 + C * (unit_at + unit_min)).all()), "argmin bound"


# ---- the cases of the GPU test, also measured by tools/mesh_surface_margins.py --------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(nq, nf):
    """(points, vertices, faces) of one (Nq, Nf) case, on the CPU."""
    v, f = soup(nf, 1000 + nf)
    return queries(nq, 2000 + nq, v, f), v, f


def gpu_cases(layout):
    """Every (Nq, Nf) the GPU test searches, from dgs_tri_layout's Q, T, C: the cross of the edge sizes, misaligned slices, Nf > C."""
    q, t, c = layout[:3]
    cross = [(nq, nf) for nq in (1, q - 1, q, q + 1, 3 * q + 5) for nf in (1, 2, t - 1, t, t + 1, 2 * t + 3)]
    return cross + [(q + 1, 5 * t + 7), (q + 1, c + t + 5), (7, 2 * c + 1)]


def cpu_sets():
    """The named input sets of the CPU test: random soups around 0 and around 1 (edge scales 1 and 0.05 mixed), the needles, the
    degenerate faces -> [(name, points, vertices, faces)]."""
    out = []
    for name, centre, seed in (("soup around 0", 0.0, 41), ("soup around 1", 1.0, 42)):
        v, f = soup(1200, seed, centre)
        out.append((name, queries(900, seed + 10, v, f, centre), v, f))
    v, f, p = needles()
    out.append(("needles", p, v, f))
    v, f, p, _ = degenerates()
    out.append(("degenerate faces", p, v, f))
    return out
