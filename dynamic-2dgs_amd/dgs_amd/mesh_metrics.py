"""Geometry metrics between two triangle meshes: how far the surface written by dgs_amd.mesh is from a ground-truth surface.  The
reference's meshes are judged on the DG-Mesh benchmark by the Chamfer distance to a ground-truth mesh per frame (its tree carries
the reader of those, read_gt_mesh.py: load_obj); this module samples both surfaces, finds every sample's nearest neighbour in the
other set and reports the directed means, Chamfer distance, precision / recall / F-score and normal consistency.  With
mode="surface" a sample's distance is the exact one to the other SURFACE (the minimum over its triangles), which has no sampling floor.

  nearest          all-pairs nearest neighbour; HIP device: dgs_nn_search of libdgs_mesh_ops.so (include/dgs_mesh_ops.h states the
                   arithmetic and the tie rule); CPU tensors: nearest_torch, the PyTorch statement of the same arithmetic
  closest_face     exact point-to-triangle distance to the closest face of a mesh; HIP device: dgs_tri_search over the rows of
                   triangle_table; CPU tensors: closest_face_torch, the PyTorch statement of the same arithmetic
  winding_number   generalised winding number of a mesh at query points (1 inside, 0 outside, smooth near an open rim); HIP device:
                   dgs_winding_sum over the rows of winding_table; CPU tensors: winding_sums_torch, the same arithmetic -- the sums
                   are integers and bit-identical between the two; contains, signed_distance, mesh_volume, is_outward and
                   volume_iou are built on it
  emd              earth mover's distance of two equal-sized point sets: a one-to-one matching by an integer auction; HIP device:
                   dgs_emd_auction; CPU tensors: emd_torch, the PyTorch statement of the same schedule (bit-identical)
  sample_surface   area-weighted uniform samples of a mesh, the same points on every device
  mesh_distance    the metrics of one pair of meshes (iou_samples > 0: with volume_iou)
  read_mesh        .ply (io.read_mesh_ply) or .obj (io.read_mesh_obj)
  evaluate_meshes  frame_<i>.ply of a directory against the i-th ground-truth mesh of another -> mesh_metrics.json

On a HIP device a missing library is an error, never a reason to run the PyTorch statement instead."""
import json
import math
import os
import re

import numpy as np
import torch

_PAIR_BUDGET = 1 << 24   # elements of one [chunk, Nr] intermediate of nearest_torch
_TRI_LIVE = 16           # closest_face_torch keeps about twenty [chunk, Nf] intermediates alive: its chunk is that much smaller
TRI_VALUES, TRI_ROW = 34, 36   # values of a triangle_table row, floats of a row (padded to 16 bytes; = dgs_tri_layout()[3])


# ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
def nearest_torch(query, ref, chunk=None):
    """The arithmetic of dgs_nn_search in PyTorch, in the dtype and on the device of the tensors, chunked over the queries:
    d2 = (dx * dx + dy * dy) + dz * dz as elementwise operations (one rounding each), the minimum over the reference set, and
    among equal distances the lowest index -- written out, not left to what torch.min returns.
    -> (d2 [Nq], idx [Nq] int64).  Also the comparator of the GPU tests and the baseline of tools/mesh_metrics_timing.py."""
    nq, nr = query.shape[0], ref.shape[0]
    if nr < 1:
        raise ValueError("nearest: the reference set is empty")
    if chunk is None:
        chunk = max(1, _PAIR_BUDGET // nr)
    rx, ry, rz = ref[:, 0].unsqueeze(0), ref[:, 1].unsqueeze(0), ref[:, 2].unsqueeze(0)
    index = torch.arange(nr, dtype=torch.int64, device=ref.device).unsqueeze(0)
    d2 = torch.empty(nq, dtype=query.dtype, device=query.device)
    idx = torch.empty(nq, dtype=torch.int64, device=query.device)
    for s in range(0, nq, chunk):
        q = query[s:s + chunk]
        dx, dy, dz = q[:, 0:1] - rx, q[:, 1:2] - ry, q[:, 2:3] - rz
        d = dx * dx + dy * dy + dz * dz
        m = d.min(dim=1, keepdim=True).values
        d2[s:s + chunk] = m[:, 0]
        idx[s:s + chunk] = torch.where(d == m, index, nr).min(dim=1).values
    return d2, idx


def _points(x, what, who="nearest"):
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
        raise ValueError("%s: %s must be a floating-point tensor [N,3]" % (who, what))
    if not bool(torch.isfinite(x).all()):
        raise ValueError("%s: %s holds non-finite coordinates" % (who, what))
    return x


@torch.no_grad()
def nearest(query, ref, ref_chunk=None):
    """(d2 [Nq], idx [Nq] int64): squared distance to, and index of, the nearest point of ref [Nr,3] for every point of query
    [Nq,3]; equal distances go to the lowest index.  HIP tensors (fp32): the kernel, ref_chunk = its slice of the reference set per
    workgroup (the result does not depend on it); CPU tensors: nearest_torch in their dtype.  Nr = 0 and non-finite coordinates
    raise ValueError before anything is launched."""
    _points(query, "query"), _points(ref, "ref")
    if ref.shape[0] < 1:
        raise ValueError("nearest: the reference set is empty")
    if query.device != ref.device:
        raise ValueError("nearest: query and ref live on different devices")
    if query.device.type == "cpu":
        return nearest_torch(query, ref)
    from . import _mesh_ops
    return _mesh_ops.nearest(query.float().contiguous(), ref.float().contiguous(), ref_chunk)


# ---- closest face ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]          # (x x' + y y') + z z', one rounding per operation


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _safe_reciprocal(x):
    """1 / x where x > 0 and the quotient is finite, else 0."""
    r = 1.0 / x
    return torch.where((x > 0) & torch.isfinite(r), r, torch.zeros_like(r))


@torch.no_grad()
def triangle_table(vertices, faces):
    """[Nf, TRI_ROW] in the dtype and on the device of `vertices`: per face with corners A, B, C the row A, B, C, e0 = B - A,
    e1 = C - B, e2 = A - C, n = cross(e0, C - A), m_k = cross(n, e_k), r_k = 1 / dot(e_k, e_k), rn = 1 / dot(n, n) (0 where the
    dot product is not positive or the quotient not finite) and two zeros of padding -- the table of dgs_tri_search
    (include/dgs_mesh_ops.h), elementwise operations only, every one rounded on its own."""
    v = vertices.detach().reshape(-1, 3)
    f = faces.detach().reshape(-1, 3).long().to(v.device)
    xyz = lambda p: (p[:, 0], p[:, 1], p[:, 2])
    a, b, c = xyz(v[f[:, 0]]), xyz(v[f[:, 1]]), xyz(v[f[:, 2]])
    sub = lambda p, q: (p[0] - q[0], p[1] - q[1], p[2] - q[2])
    e0, e1, e2 = sub(b, a), sub(c, b), sub(a, c)
    n = _cross(e0, sub(c, a))
    m0, m1, m2 = _cross(n, e0), _cross(n, e1), _cross(n, e2)
    tail = (_safe_reciprocal(_dot(e0, e0)), _safe_reciprocal(_dot(e1, e1)), _safe_reciprocal(_dot(e2, e2)), _safe_reciprocal(_dot(n, n)))
    zero = torch.zeros_like(tail[0])
    return torch.stack(a + b + c + e0 + e1 + e2 + n + m0 + m1 + m2 + tail + (zero,) * (TRI_ROW - TRI_VALUES), dim=1).contiguous()


def _pair_d2(points, col):
    """[Nq, Nf] squared distances of every (point, row) pair; col = the table's 34 value columns as [34, 1, Nf]."""
    tri = lambda i: (col[i], col[i + 1], col[i + 2])
    p = (points[:, 0:1], points[:, 1:2], points[:, 2:3])
    best, inside, w0 = None, col[33] > 0, None
    for k in range(3):
        o, e = tri(3 * k), tri(9 + 3 * k)
        w = (p[0] - o[0], p[1] - o[1], p[2] - o[2])
        t = (_dot(w, e) * col[30 + k]).clamp(0, 1)
        c = (w[0] - t * e[0], w[1] - t * e[1], w[2] - t * e[2])
        sk = _dot(c, c)
        best = sk if best is None else torch.minimum(best, sk)
        inside = inside & (_dot(w, tri(21 + 3 * k)) >= 0)
        w0 = w if k == 0 else w0
    h = _dot(w0, tri(18))
    return torch.where(inside, torch.minimum(h * h * col[33], best), best)


def closest_face_torch(points, table, chunk=None):
    """The arithmetic of dgs_tri_search in PyTorch, in the dtype and on the device of the tensors, chunked over the queries.  Per
    pair (P, row):  w_k = P - O_k;  t = clamp(dot(w_k, e_k) * r_k, 0, 1);  c = w_k - t e_k;  s_k = dot(c, c);  best = min(s_0, s_1,
    s_2);  inside = (dot(w_k, m_k) >= 0 for all k) & (rn > 0);  h = dot(w_0, n);  pl = (h h) rn;  d2 = inside ? min(pl, best) : best
    -- elementwise operations, one rounding each (_pair_d2); then the minimum over the faces and, among equal distances, the
    lowest face, written out.  -> (d2 [Nq], face [Nq] int64).  The CPU path, the comparator of the GPU tests and the baseline of
    tools/mesh_surface_timing.py."""
    nq, nf = points.shape[0], table.shape[0]
    if nf < 1:
        raise ValueError("closest_face: the mesh has no faces")
    if chunk is None:
        chunk = max(1, _PAIR_BUDGET // _TRI_LIVE // nf)
    col = table[:, :TRI_VALUES].t().contiguous().unsqueeze(1)               # [34, 1, Nf]: col[i] broadcasts against [chunk, 1]
    index = torch.arange(nf, dtype=torch.int64, device=table.device).unsqueeze(0)
    d2 = torch.empty(nq, dtype=points.dtype, device=points.device)
    face = torch.empty(nq, dtype=torch.int64, device=points.device)
    for s in range(0, nq, chunk):
        d = _pair_d2(points[s:s + chunk], col)
        m = d.min(dim=1, keepdim=True).values
        d2[s:s + chunk] = m[:, 0]
        face[s:s + chunk] = torch.where(d == m, index, nf).min(dim=1).values
    return d2, face


@torch.no_grad()
def closest_face(points, vertices, faces, face_chunk=None):
    """(d2 [Nq], face [Nq] int64): squared distance from every point of points [Nq,3] to the surface of the mesh (vertices [Nv,3],
    faces [Nf,3]) -- the exact point-to-triangle distance, minimised over the faces -- and the face that attains it; equal
    distances go to the lowest face.  Degenerate faces are legal: they act as their segments or their point.  HIP tensors (fp32):
    the kernel, face_chunk = its slice of the faces per workgroup (the result does not depend on it); CPU tensors:
    closest_face_torch in the dtype of `points`.  Nf = 0, non-finite coordinates and mixed devices raise ValueError before
    anything is launched."""
    _points(points, "points", "closest_face"), _points(vertices, "vertices", "closest_face")
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError("closest_face: faces must be an integer tensor [Nf,3]")
    if faces.shape[0] < 1:
        raise ValueError("closest_face: the mesh has no faces")
    if points.device != vertices.device or points.device != faces.device:
        raise ValueError("closest_face: points, vertices and faces live on different devices")
    if int(faces.min()) < 0 or int(faces.max()) >= vertices.shape[0]:
        raise ValueError("closest_face: a face names a vertex outside [0, %d)" % vertices.shape[0])
    if points.device.type == "cpu":
        return closest_face_torch(points, triangle_table(vertices.to(points.dtype), faces))
    from . import _mesh_ops
    return _mesh_ops.closest_face(points.float().contiguous(), triangle_table(vertices.float(), faces), face_chunk)


# ---- winding number -------------------------------------------------------------------------------------------------------------
WIND_ROW = 12                      # floats of a winding_table row (= dgs_winding_layout()[3])
WIND_SCALE = float(1 << 28)        # a pair's half solid angle enters the sum as rint(theta * 2^28)
# W = sum * WIND_UNIT in float64: one correctly rounded multiplication on any device (a division by a Python scalar is not one
# everywhere: a device may multiply by the reciprocal), so equal sums give equal W
WIND_UNIT = 1.0 / (2.0 * math.pi * WIND_SCALE)
_WIND_LIVE = 32                    # winding_sums_torch keeps about thirty [chunk, Nf] intermediates alive, float64 ones among them
_WIND_PI, _WIND_HALF_PI = 3.1415927410125732, 1.5707963705062866     # the fp32 values nearest to pi and pi / 2
# atan(r) = r (c0 + c1 s + ... + c7 s^7), s = r r, on [0, 1]: fp32 values, c0 pinned to 1 (include/dgs_mesh_ops.h says why)
_WIND_ATAN = (1.0, -0.3333165943622589, 0.19962704181671143, -0.13976581394672394, 0.09794232249259949, -0.05777356028556824,
              0.02304011397063732, -0.004355399403721094)


def _faces(faces, who):
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point():
        raise ValueError("%s: faces must be an integer tensor [Nf,3]" % who)
    return faces


@torch.no_grad()
def winding_table(vertices, faces):
    """[Nf', WIND_ROW] fp32 on the device of `vertices`: per face with corners A, B, C the row A, B, C, n = cross(B - A, C - A) --
    the table of dgs_winding_sum (include/dgs_mesh_ops.h), elementwise fp32 operations, every one rounded on its own.  Faces that
    name a vertex twice are dropped first (they subtend nothing), so Nf' <= Nf."""
    v = vertices.detach().reshape(-1, 3).float()
    f = faces.detach().reshape(-1, 3).long().to(v.device)
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
    xyz = lambda p: (p[:, 0], p[:, 1], p[:, 2])
    a, b, c = xyz(v[f[:, 0]]), xyz(v[f[:, 1]]), xyz(v[f[:, 2]])
    sub = lambda p, q: (p[0] - q[0], p[1] - q[1], p[2] - q[2])
    return torch.stack(a + b + c + _cross(sub(b, a), sub(c, a)), dim=1).contiguous()


def _sqrt32(x):
    """The correctly rounded fp32 square root on any device (the float64 one rounded to fp32: see _emd_costs)."""
    return torch.sqrt(x.double()).float()


def _wind_atan2(y, x):
    """ATAN2 of include/dgs_mesh_ops.h on fp32 tensors, one rounding per operation; the division is the float64 one rounded to fp32,
    which is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits) whatever the device's own fp32 division does."""
    ay, ax = y.abs(), x.abs()
    mx, mn = torch.maximum(ay, ax), torch.minimum(ay, ax)
    r = torch.where(mx > 0, (mn.double() / mx.double()).float(), torch.zeros_like(mx))
    s = r * r
    p = torch.full_like(s, _WIND_ATAN[7])
    for c in _WIND_ATAN[6::-1]:
        p = p * s + c
    p = p * r
    p = torch.where(ay > ax, _WIND_HALF_PI - p, p)
    p = torch.where(x < 0, _WIND_PI - p, p)
    p = torch.where(y < 0, -p, p)
    return torch.where(torch.isfinite(y) & torch.isfinite(x) & (mx > 0), p, torch.zeros_like(p))


def _pair_terms(points, col):
    """[Nq, Nf] int64: rint(theta * 2^28) of every (point, row) pair; col = the table's columns as [12, 1, Nf]."""
    q = (points[:, 0:1], points[:, 1:2], points[:, 2:3])
    a, b, c = ((col[3 * k] - q[0], col[3 * k + 1] - q[1], col[3 * k + 2] - q[2]) for k in range(3))
    la, lb, lc = _sqrt32(_dot(a, a)), _sqrt32(_dot(b, b)), _sqrt32(_dot(c, c))
    num = _dot(a, (col[9], col[10], col[11]))
    den = ((la * lb) * lc + _dot(a, b) * lc) + (_dot(b, c) * la + _dot(c, a) * lb)
    return torch.round(_wind_atan2(num, den) * WIND_SCALE).to(torch.int64)


@torch.no_grad()
def winding_sums_torch(points, table, chunk=None):
    """The arithmetic of dgs_winding_sum in PyTorch, in fp32 on the device of the tensors: per pair a = A - q, b, c likewise, their
    norms by the correctly rounded sqrt, num = dot(a, n), den = ((la lb) lc + dot(a, b) lc) + (dot(b, c) la + dot(c, a) lb),
    theta = ATAN2(num, den) (_wind_atan2), term = rint(theta 2^28) as int64; then the integer sum over the faces.  chunk: faces per
    partial sum (None: all at once) -- integer addition has no order, so the result does not depend on it, nor on the order of the
    rows.  -> sums [Nq] int64.  The CPU path, the comparator of the GPU tests and the baseline of tools/mesh_winding_timing.py."""
    nq, nf = points.shape[0], table.shape[0]
    if nf < 1:
        raise ValueError("winding_number: the mesh has no faces")
    points, table = points.float(), table.float()
    chunk = nf if chunk is None else max(1, int(chunk))
    step = max(1, _PAIR_BUDGET // _WIND_LIVE // min(chunk, nf))
    sums = torch.zeros(nq, dtype=torch.int64, device=points.device)
    for fs in range(0, nf, chunk):
        col = table[fs:fs + chunk].t().contiguous().unsqueeze(1)            # [12, 1, n]: col[i] broadcasts against [step, 1]
        for s in range(0, nq, step):
            sums[s:s + step] += _pair_terms(points[s:s + step], col).sum(dim=1)
    return sums


def _winding_args(points, vertices, faces, who):
    """Shapes, devices and face indices; the coordinates may be anything -- a non-finite pair adds 0 to the sum."""
    for x, what in ((points, "points"), (vertices, "vertices")):
        if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
            raise ValueError("%s: %s must be a floating-point tensor [N,3]" % (who, what))
    _faces(faces, who)
    if faces.shape[0] < 1:
        raise ValueError("%s: the mesh has no faces" % who)
    if points.device != vertices.device or points.device != faces.device:
        raise ValueError("%s: points, vertices and faces live on different devices" % who)
    if int(faces.min()) < 0 or int(faces.max()) >= vertices.shape[0]:
        raise ValueError("%s: a face names a vertex outside [0, %d)" % (who, vertices.shape[0]))


@torch.no_grad()
def winding_sums(points, vertices, faces, face_chunk=None):
    """sums [Nq] int64 of dgs_winding_sum for the mesh at the points, in fp32: HIP tensors use the kernel (a missing library is an
    error), CPU tensors winding_sums_torch; the two give the same integers."""
    _winding_args(points, vertices, faces, "winding_number")
    table = winding_table(vertices, faces)
    if table.shape[0] < 1:
        raise ValueError("winding_number: every face of the mesh names a vertex twice")
    if points.device.type == "cpu":
        return winding_sums_torch(points, table, face_chunk)
    from . import _mesh_ops
    return _mesh_ops.winding_sums(points.float().contiguous(), table, face_chunk)


def winding_number(points, vertices, faces, face_chunk=None):
    """W [Nq] float64: the generalised winding number of the mesh (vertices [Nv,3], faces [Nf,3]) at every point of points [Nq,3]:
    the signed solid angle the faces subtend, over 4 pi.  1 inside a closed mesh wound outward, 0 outside, -1 inside one wound
    inward, k inside k nested shells; near an open rim a smooth value in between, which is why it -- not a ray's parity -- is the
    inside test for extracted frames and unwelded ground truth.  A point ON the surface has no answer (about 1/2 on a smooth
    patch).  Brute force over all (point, face) pairs, fp32 per pair, summed as integers: W = winding_sums * WIND_UNIT (1 / (2 pi 2^28)), identical on
    every device and for every face order.  face_chunk: the kernel's slice of the faces per workgroup, the statement's faces per
    partial sum; the result does not depend on it.  Non-finite points or vertices are legal: their pairs add 0.  Nf = 0, bad
    shapes, face indices out of range and mixed devices raise ValueError before anything is launched."""
    return winding_sums(points, vertices, faces, face_chunk).double() * WIND_UNIT


def contains(points, vertices, faces, threshold=0.5):
    """bool [Nq]: winding_number > threshold.  For a closed mesh wound outward this is "inside"; a mesh wound inward contains
    nothing (its W is -1 inside: is_outward tells)."""
    return winding_number(points, vertices, faces) > threshold


def signed_distance(points, vertices, faces):
    """[Nq]: the distance of closest_face with a sign, -sqrt(d2) where `contains` says inside and +sqrt(d2) outside; the dtype is
    closest_face's (fp32 on a HIP device).  Finite coordinates only, as for closest_face."""
    d2, _ = closest_face(points, vertices, faces)
    d = d2.sqrt()
    return torch.where(contains(points, vertices, faces), -d, d)


@torch.no_grad()
def mesh_volume(vertices, faces):
    """The signed volume the mesh encloses, a Python float: the divergence sum over the faces of A . (B x C) / 6 in float64.
    Positive for a closed mesh wound outward; for an open mesh it depends on the origin and means little."""
    v = vertices.detach().reshape(-1, 3).double()
    f = _faces(faces, "mesh_volume").long().to(v.device)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * torch.cross(b, c, dim=1)).sum() / 6.0)


def is_outward(vertices, faces):
    """mesh_volume(vertices, faces) > 0: the faces of a closed mesh are wound counter-clockwise seen from outside, which is what
    makes winding_number +1 inside.  No more than that sign: an open or self-intersecting mesh gets an answer too."""
    return mesh_volume(vertices, faces) > 0.0


def _volume_iou(pv, pf, gv, gf, n_samples, seed):
    """volume_iou on mesh tensors that share a device."""
    n = int(n_samples)
    if n < 1:
        raise ValueError("volume_iou: n_samples must be >= 1")
    lo = torch.minimum(pv.min(0).values, gv.min(0).values).double().cpu()     # the six extrema are exact on any device; the
    hi = torch.maximum(pv.max(0).values, gv.max(0).values).double().cpu()     # arithmetic on them runs on the CPU
    u = torch.rand((n, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed)))
    pts = (lo + u * (hi - lo)).float().to(pv.device)
    in_p, in_g = contains(pts, pv, pf), contains(pts, gv, gf)
    n_p, n_g, n_i, n_u = int(in_p.sum()), int(in_g.sum()), int((in_p & in_g).sum()), int((in_p | in_g).sum())
    box = float((hi - lo).prod())
    return {"iou": n_i / n_u if n_u else 0.0, "volume_pred": box * n_p / n, "volume_gt": box * n_g / n, "volume_intersection": box * n_i / n,
            "iou_samples": n}


@torch.no_grad()
def volume_iou(pred, gt, n_samples=100_000, seed=0, device="cuda:0", gt_transform=None):
    """Volumetric intersection over union of two meshes, each a (vertices, faces) pair of arrays or tensors, by Monte Carlo:
    n_samples points uniform in the joint bounding box of the two meshes -- [n,3] float64 uniforms from a CPU
    torch.Generator().manual_seed(seed), scaled into the box in float64 on the CPU, then cast to fp32, so every device tests the same
    points -- and `contains` against both meshes on `device`.  gt_transform: as in mesh_distance.
      iou                  samples inside both / samples inside either; 0 when no sample is inside either
      volume_pred, volume_gt, volume_intersection    box volume x the share of the samples inside
      iou_samples          n_samples
    The samples and the winding sums are the same on every device, so are the returned floats.  The standard deviation of a share p
    is sqrt(p (1 - p) / n); meshes must be wound outward (is_outward) to contain anything."""
    dev = torch.device(device)
    pv, pf = _mesh_tensors(pred, dev)
    gv, gf = _mesh_tensors(gt, dev)
    if gt_transform is not None:
        gv = _transformed(gv, gt_transform)
    return _volume_iou(pv, pf, gv, gf, n_samples, seed)


# ---- earth mover's distance -------------------------------------------------------------------------------------------------------
EMD_COST_CAP = 1 << 20     # costs are integers in [0, 2^20]: the bounding-box diagonal of both sets is 2^20 quanta
EMD_BIDDER_BITS, EMD_BID_BITS = 24, 39   # the packed word of an object: bid << 24 | bidder, below 2^63 (signed = unsigned order)


def _emd_quantum(a, b):
    """(q, inv_q) as Python floats that hold fp32 values: q = diag / 2^20 with diag the fp32 bounding-box diagonal of both sets
    together, sqrt((ex * ex + ey * ey) + ez * ez) of the fp32 extents; inv_q = 1 / q in fp32, 0 where q is not positive (all
    points coincide: every cost is 0).  The six extrema are exact on any device; the arithmetic on them runs on the CPU, so the
    HIP path and the statement are handed the same number."""
    lo = torch.minimum(a.min(0).values, b.min(0).values).float().cpu()
    hi = torch.maximum(a.max(0).values, b.max(0).values).float().cpu()
    e = hi - lo
    diag = torch.sqrt(((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]).double()).float()    # correctly rounded (see _emd_costs)
    q = diag / float(EMD_COST_CAP)
    inv_q = 1.0 / q
    if not float(q) > 0.0 or not math.isfinite(float(inv_q)):
        return float(q) if float(q) > 0.0 else 0.0, 0.0
    return float(q), float(inv_q)


def _emd_costs(a, b, inv_q):
    """[n, n] int64: c_ij = min(rint(sqrt((dx * dx + dy * dy) + dz * dz) * inv_q), 2^20) in fp32, one rounding per operation -- the
    expression of include/dgs_mesh_ops.h (the kernels recompute it per pair; the statement and the tests may hold the matrix)."""
    dx, dy, dz = a[:, 0:1] - b[:, 0].unsqueeze(0), a[:, 1:2] - b[:, 1].unsqueeze(0), a[:, 2:3] - b[:, 2].unsqueeze(0)
    # torch.sqrt of an fp32 CPU tensor is not correctly rounded; the float64 one rounded to fp32 is (53 >= 2 * 24 + 2 bits: the double
    # rounding is innocuous for a square root), and that is the number the kernel's IEEE sqrt gives
    d = torch.sqrt((dx * dx + dy * dy + dz * dz).double()).float()
    return torch.round(d * torch.tensor(inv_q, dtype=torch.float32, device=a.device)).clamp(max=float(EMD_COST_CAP)).to(torch.int64)


def emd_torch(a, b, max_rounds=2_000_000, inv_q=None):
    """The statement of dgs_emd_auction in PyTorch (CPU or any device; fp32 costs, int64 everything else): a synchronous forward
    auction with eps-scaling on the integer costs of _emd_costs.
      phases   eps_0 = max(1, max_cost // 2), then eps <- max(1, eps // 4) until a phase with eps = 1 has run; every phase starts with
               nobody assigned and keeps the prices, which start at 0
      round    every unassigned i bids at once against the prices at the start of the round: j1 = the lowest index minimising
               w = c_ij + p_j (value w1), w2 = the minimum over j != j1, bid = p_j1 + (w2 - w1) + eps; every object that received
               bids takes the largest packed word bid << 24 | bidder, its price becomes that bid, its former owner is unassigned
    (the words are kept across rounds: a new bid on an object exceeds its price, which is the last word's bid, so an old word never
    wins and never equals a new one -- what the kernels do too).  n = 1 is the trivial matching without a round.
    -> (assignment [n] int64: the object of person i, prices [n] int64, primal, dual, rounds) with
       primal = sum_i c_{i,assignment(i)} <= OPT + n and dual = sum_i min_j (c_ij + p_j) - sum_j p_j <= OPT.
    RuntimeError when a round beyond max_rounds would be needed, or a bid does not fit 39 bits."""
    n = a.shape[0]
    dev = a.device
    if inv_q is None:
        inv_q = _emd_quantum(a, b)[1]
    cost = _emd_costs(a.float(), b.float(), inv_q)
    price = torch.zeros(n, dtype=torch.int64, device=dev)
    if n == 1:
        c = int(cost[0, 0])
        return torch.zeros(1, dtype=torch.int64, device=dev), price, c, c, 0
    index = torch.arange(n, dtype=torch.int64, device=dev)
    word = torch.zeros(n, dtype=torch.int64, device=dev)
    big = torch.iinfo(torch.int64).max
    eps, rounds, phase = max(1, int(cost.max()) // 2), 0, 0
    while True:
        owner = torch.full((n,), -1, dtype=torch.int64, device=dev)
        free = torch.ones(n, dtype=torch.bool, device=dev)
        bidders = index
        while bidders.numel():
            if rounds >= max_rounds:
                raise RuntimeError("emd: max_rounds = %d reached in phase %d (eps %d) with %d of %d still unassigned"
                                   % (max_rounds, phase, eps, bidders.numel(), n))
            w = cost.index_select(0, bidders) + price
            w1 = w.min(dim=1, keepdim=True).values
            j1 = torch.where(w == w1, index, n).min(dim=1, keepdim=True).values     # the lowest index among equal w, written out
            w2 = w.scatter_(1, j1, big).min(dim=1).values
            j1, w1 = j1.squeeze(1), w1.squeeze(1)
            bid = price.index_select(0, j1) + (w2 - w1) + eps
            if int(bid.max()) >= 1 << EMD_BID_BITS:
                raise RuntimeError("emd: a bid of phase %d does not fit %d bits" % (phase, EMD_BID_BITS))
            packed = (bid << EMD_BIDDER_BITS) | bidders
            word.scatter_reduce_(0, j1, packed, "amax", include_self=True)
            won = torch.nonzero(word.index_select(0, j1) == packed).squeeze(1)      # (index_* calls: the round is op-count bound)
            wj, wi = j1.index_select(0, won), bidders.index_select(0, won)
            evicted = owner.index_select(0, wj)
            price.index_copy_(0, wj, bid.index_select(0, won))
            owner.index_copy_(0, wj, wi)
            free.index_fill_(0, wi, False)
            free.index_fill_(0, torch.masked_select(evicted, evicted >= 0), True)
            bidders = torch.nonzero(free).squeeze(1)
            rounds += 1
        if eps == 1:
            break
        eps, phase = max(1, eps // 4), phase + 1
    assignment = torch.empty(n, dtype=torch.int64, device=dev)
    assignment[owner] = index
    primal = int(cost[index, assignment].sum())
    dual = int((cost + price).min(dim=1).values.sum()) - int(price.sum())
    return assignment, price, primal, dual, rounds


@torch.no_grad()
def emd(a, b, max_rounds=2_000_000):
    """Earth mover's distance between two point sets a, b [n,3] of the same size: the mean length of the pairs of a one-to-one
    matching that is optimal, to a certified gap, for the distances quantised to q = diag / 2^20 (diag: the fp32 bounding-box
    diagonal of both sets together).  HIP tensors: dgs_emd_auction of libdgs_mesh_ops.so (include/dgs_mesh_ops.h states the cost,
    the schedule and the field widths); CPU tensors: emd_torch, the same schedule in PyTorch -- the two agree bit for bit.
      emd          float64 mean of the true Euclidean distances |a_i - b_assignment(i)|: an upper bound on the exact EMD of the
                   samples, because any matching is
      emd_gap      (primal - dual) * q / n: the matching is within emd_gap of the optimum of the quantised problem; emd_gap <= q
      emd_samples  n;   emd_rounds: the auction's rounds;   assignment [n] int64: the object of person i
    Conventions as in mesh_distance: Euclidean, not squared, mean per point, nothing halved.  Published protocols differ in the
    number of samples and in normalisation (unit box, unit sphere, squared or halved distances): compare like with like.
    ValueError: a wrong shape, unequal sizes, no points, non-finite coordinates, mixed devices, n >= 2^24.  RuntimeError: max_rounds
    reached (the message names the phase, eps and the persons left) -- a partial matching is never returned."""
    _points(a, "a", "emd"), _points(b, "b", "emd")
    if a.shape[0] != b.shape[0]:
        raise ValueError("emd: the two sets must have the same size, not %d and %d" % (a.shape[0], b.shape[0]))
    n = a.shape[0]
    if n < 1 or n >= 1 << EMD_BIDDER_BITS:
        raise ValueError("emd: n must be in [1, 2^24)")
    if a.device != b.device:
        raise ValueError("emd: a and b live on different devices")
    if int(max_rounds) < 1:
        raise ValueError("emd: max_rounds must be >= 1")
    a32, b32 = a.float().contiguous(), b.float().contiguous()
    q, inv_q = _emd_quantum(a32, b32)
    if a.device.type == "cpu":
        assignment, _, primal, dual, rounds = emd_torch(a32, b32, int(max_rounds), inv_q)
    else:
        from . import _mesh_ops
        assignment, _, primal, dual, rounds, _ = _mesh_ops.emd_auction(a32, b32, inv_q, int(max_rounds))
        assignment = assignment.long()
    d = a32.double() - b32.double()[assignment]
    length = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt()
    return {"emd": float(length.mean()), "emd_gap": (primal - dual) * q / n, "emd_samples": int(n), "emd_rounds": int(rounds),
            "assignment": assignment}


# ---- sampling -------------------------------------------------------------------------------------------------------------------
def _mesh_tensors(mesh, device):
    v, f = mesh[0], mesh[1]
    v = (v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(device)
    f = (f.detach() if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))).to(device)
    return v.reshape(-1, 3), f.reshape(-1, 3).long()


def _transformed(vertices, transform):
    """x' = M[:3,:3] x + M[:3,3] of the [4,4] transform (column-vector convention), in float64, back in the dtype of the vertices."""
    m = torch.as_tensor(np.asarray(transform, dtype=np.float64), device=vertices.device)
    return (vertices.double() @ m[:3, :3].T + m[:3, 3]).to(vertices.dtype)


@torch.no_grad()
def sample_surface(vertices, faces, n, seed):
    """n points uniform over the surface of the mesh -> (points [n,3] f32, face_ids [n] int64, normals [n,3] f32 -- the unit normal
    of each point's face) on the device of `vertices`.  The uniforms are [n,3] float64 from a CPU torch.Generator().manual_seed(seed),
    so every device samples the same points; face areas and their cumulative sum are float64.  Face: searchsorted(cum, u0 * total,
    right=True) clamped to Nf - 1 (a zero-area face spans an empty interval and is never drawn); point: (1 - sqrt(u1)) A +
    sqrt(u1) (1 - u2) B + sqrt(u1) u2 C.  ValueError for a mesh without faces or with total area 0."""
    dev = vertices.device
    v = vertices.detach().reshape(-1, 3).double()
    f = faces.detach().reshape(-1, 3).long().to(dev)
    if f.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cross = torch.cross(b - a, c - a, dim=1)
    twice = (cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1] + cross[:, 2] * cross[:, 2]).sqrt()
    cum = torch.cumsum(0.5 * twice, 0)
    total = cum[-1]
    if not float(total) > 0.0 or not math.isfinite(float(total)):
        raise ValueError("sample_surface: the total area of the mesh is %r" % float(total))
    u = torch.rand((int(n), 3), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed))).to(dev)
    fid = torch.searchsorted(cum, (u[:, 0] * total).contiguous(), right=True).clamp(max=f.shape[0] - 1)
    fid = _skip_empty(fid, twice)
    s = u[:, 1].sqrt().unsqueeze(1)
    t = u[:, 2].unsqueeze(1)
    pts = (1 - s) * a[fid] + s * (1 - t) * b[fid] + s * t * c[fid]
    nrm = cross[fid] / twice[fid].unsqueeze(1)
    return pts.float(), fid, nrm.float()


def _skip_empty(fid, twice):
    """The clamp of searchsorted can only land on the last face; should that one have no area (u0 * total rounding up to the total),
    the draw goes to the last face that has some."""
    if bool((twice[fid] > 0).all()):
        return fid
    good = torch.nonzero(twice > 0).reshape(-1)
    pos = torch.searchsorted(good, fid, right=True).clamp(min=1) - 1
    return torch.where(twice[fid] > 0, fid, good[pos])


# ---- metrics of one pair --------------------------------------------------------------------------------------------------------
def _tkey(tau):
    return "%g" % tau


def _surface_hits(points, vertices, faces):
    """closest_face of the points on the mesh without its zero-area faces (float64 area, the faces sample_surface never draws
    either) -> (d2 [Nq], unit normal of the hit face [Nq,3] float64)."""
    v = vertices.double()
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    cross = torch.cross(b - a, c - a, dim=1)
    twice = (cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1] + cross[:, 2] * cross[:, 2]).sqrt()
    keep = twice > 0
    d2, hit = closest_face(points, vertices.float(), faces[keep])
    return d2, cross[keep][hit] / twice[keep][hit].unsqueeze(1)


@torch.no_grad()
def mesh_distance(pred, gt, n_samples=100_000, seed=0, thresholds=(0.005, 0.01, 0.02), device="cuda:0", gt_transform=None, mode="samples",
                  emd_samples=0, iou_samples=0):
    """Metrics between the surfaces of pred and gt, each a (vertices [Nv,3], faces [Nf,3]) pair of arrays or tensors.  n_samples
    points are drawn on pred with `seed` and on gt with `seed + 1` (sample_surface), then `nearest` runs both ways on `device`.
    gt_transform: optional [4,4] (column-vector convention, x' = M[:3,:3] x + M[:3,3]) applied to the ground-truth vertices first.
    mode: "samples" (default) measures every sample against the nearest SAMPLE of the other mesh; "surface" measures it against
    the other SURFACE -- `closest_face`, the exact point-to-triangle distance minimised over the other mesh's faces (zero-area faces
    dropped first) -- and takes the normal of the face that was hit.  The same samples, the same keys; no sampling floor.

    Conventions: distances are Euclidean, in the units of the meshes, NOT squared unless the name says so; nothing is halved.
      accuracy            mean over the pred samples of the distance to the nearest gt sample (mode "surface": to the gt surface)
      completeness        mean over the gt samples of the distance to the nearest pred sample (mode "surface": to the pred surface)
      chamfer             accuracy + completeness
      chamfer_sq          the same sum with squared distances
      precision[tau]      share of the pred samples within tau of gt (<=);  recall[tau]: share of the gt samples within tau of pred
      fscore[tau]         2 P R / (P + R), 0 where P + R = 0
      normal_consistency  mean |n . n'| of a sample's face normal and its nearest neighbour's (mode "surface": the hit face's,
                          float64), averaged over the two directions
      n_samples, pred_faces, gt_faces, pred_vertices, gt_vertices
      emd, emd_gap, emd_samples, emd_rounds   only with emd_samples > 0: `emd` of the first emd_samples pred samples against the
                          first emd_samples gt samples (the samples are independent draws, so a prefix is a uniform sample too); at
                          most n_samples.  A one-to-one matching: a dense blob near the surface, cheap for the Chamfer distance, is not.
      iou, volume_pred, volume_gt, volume_intersection, iou_samples   only with iou_samples > 0: `volume_iou` of the two meshes with
                          iou_samples points and `seed` -- the one score here that asks whether the meshes enclose the same volume.
    The per-threshold entries are dicts keyed by '%g' % tau.  Sample-to-sample distances carry the sampling floor: a surface against
    itself measures about 0.5 sqrt(area / n_samples) per direction, not 0; sample-to-surface distances (mode "surface") measure 0."""
    if mode not in ("samples", "surface"):
        raise ValueError("mesh_distance: mode must be 'samples' or 'surface', not %r" % (mode,))
    emd_samples = int(emd_samples)
    if emd_samples < 0 or emd_samples > int(n_samples):
        raise ValueError("mesh_distance: emd_samples must be in [0, n_samples = %d], not %d" % (int(n_samples), emd_samples))
    iou_samples = int(iou_samples)
    if iou_samples < 0:
        raise ValueError("mesh_distance: iou_samples must be >= 0, not %d" % iou_samples)
    dev = torch.device(device)
    pv, pf = _mesh_tensors(pred, dev)
    gv, gf = _mesh_tensors(gt, dev)
    if gt_transform is not None:
        gv = _transformed(gv, gt_transform)
    pp, _, pn = sample_surface(pv, pf, n_samples, seed)
    gp, _, gn = sample_surface(gv, gf, n_samples, seed + 1)
    if mode == "samples":
        d2_pg, i_pg = nearest(pp, gp)
        d2_gp, i_gp = nearest(gp, pp)
        hit_p, hit_g = gn[i_pg].double(), pn[i_gp].double()
    else:
        d2_pg, hit_p = _surface_hits(pp, gv, gf)
        d2_gp, hit_g = _surface_hits(gp, pv, pf)
    d_pg, d_gp = d2_pg.double().sqrt(), d2_gp.double().sqrt()
    out = {"accuracy": float(d_pg.mean()), "completeness": float(d_gp.mean())}
    out["chamfer"] = out["accuracy"] + out["completeness"]
    out["chamfer_sq"] = float(d2_pg.double().mean()) + float(d2_gp.double().mean())
    out["precision"], out["recall"], out["fscore"] = {}, {}, {}
    for tau in thresholds:
        p, r = float((d_pg <= tau).double().mean()), float((d_gp <= tau).double().mean())
        out["precision"][_tkey(tau)], out["recall"][_tkey(tau)] = p, r
        out["fscore"][_tkey(tau)] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    nc_p = (pn.double() * hit_p).sum(1).abs().mean()
    nc_g = (gn.double() * hit_g).sum(1).abs().mean()
    out["normal_consistency"] = 0.5 * (float(nc_p) + float(nc_g))
    out.update(n_samples=int(n_samples), pred_faces=int(pf.shape[0]), gt_faces=int(gf.shape[0]), pred_vertices=int(pv.shape[0]),
               gt_vertices=int(gv.shape[0]))
    if emd_samples > 0:
        m = emd(pp[:emd_samples], gp[:emd_samples])
        out.update({k: m[k] for k in ("emd", "emd_gap", "emd_samples", "emd_rounds")})
    if iou_samples > 0:
        out.update(_volume_iou(pv, pf, gv, gf, iou_samples, seed))
    return out


# ---- files ----------------------------------------------------------------------------------------------------------------------
def read_mesh(path):
    """(vertices [Nv,3] float32, faces [Nf,3] int32) of a .ply (io.read_mesh_ply) or .obj (io.read_mesh_obj) file."""
    from . import io as dio
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        v, f, _ = dio.read_mesh_ply(path)
        return v, f
    if ext == ".obj":
        return dio.read_mesh_obj(path)
    raise ValueError("read_mesh: %s is neither .ply nor .obj" % path)


def _natural(name):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r"(\d+)", name)]


def _flat(m):
    """The scalar entries of a mesh_distance result: 'fscore' {'0.01': x} -> 'fscore@0.01': x."""
    out = {}
    for k, v in m.items():
        if isinstance(v, dict):
            out.update({"%s@%s" % (k, t): x for t, x in v.items()})
        else:
            out[k] = v
    return out


def evaluate_meshes(pred_dir, gt_dir, n_samples=100_000, seed=0, thresholds=(0.005, 0.01, 0.02), device="cuda:0", gt_transform=None, log=None,
                    mode="samples", clean_gt=False, emd_samples=0, iou_samples=0):
    """frame_<i>.ply of pred_dir against the i-th ground-truth mesh of gt_dir (its .obj / .ply files in natural sort order), for
    every i.  A different number of frames and ground-truth meshes is an error.  Writes <pred_dir>/mesh_metrics.json:
    {"frames": [{"frame": i, "pred": ..., "gt": ..., <metrics>}], "mean": {<metric>: mean over the frames}, "settings": ...} with
    the per-threshold metrics flattened to 'fscore@0.01', and returns that dict.  mode: as in mesh_distance, recorded under "settings".
    clean_gt: weld and clean every ground-truth mesh on load (mesh_clean.clean_mesh on `device`: an OBJ whose faces each carry their
    own three vertices becomes an indexed mesh again, duplicated and degenerate triangles go); recorded under "settings" when set.
    emd_samples: as in mesh_distance (0: no earth mover's distance, the result is what it was without the argument); the four emd
    keys then appear per frame and in "mean", and the value is recorded under "settings" when set.
    iou_samples: as in mesh_distance, under the same rule: 0 changes nothing, otherwise the five volume keys appear per frame and in
    "mean" and the value is recorded under "settings"."""
    def load_gt(path):
        v, f = read_mesh(path)
        if not clean_gt:
            return v, f
        from .mesh_clean import clean_mesh
        v, f, _ = clean_mesh(torch.from_numpy(np.ascontiguousarray(v)).to(device), torch.from_numpy(np.ascontiguousarray(f)).to(device))
        return v, f

    frames = {}
    for name in os.listdir(pred_dir):
        m = re.fullmatch(r"frame_(\d+)\.ply", name)
        if m:
            frames[int(m.group(1))] = name
    gts = sorted((n for n in os.listdir(gt_dir) if os.path.splitext(n)[1].lower() in (".obj", ".ply")), key=_natural)
    if len(frames) != len(gts) or sorted(frames) != list(range(len(frames))):
        raise ValueError("evaluate_meshes: %d frame_<i>.ply files in %s (i = %s) but %d ground-truth meshes in %s"
                         % (len(frames), pred_dir, sorted(frames)[:3] + (["..."] if len(frames) > 3 else []), len(gts), gt_dir))
    if not frames:
        raise ValueError("evaluate_meshes: no frame_<i>.ply in %s" % pred_dir)
    rows = []
    for i in range(len(gts)):
        m = _flat(mesh_distance(read_mesh(os.path.join(pred_dir, frames[i])), load_gt(os.path.join(gt_dir, gts[i])), n_samples=n_samples,
                                seed=seed, thresholds=thresholds, device=device, gt_transform=gt_transform, mode=mode, emd_samples=emd_samples,
                                iou_samples=iou_samples))
        rows.append(dict({"frame": i, "pred": frames[i], "gt": gts[i]}, **m))
        if log is not None:
            log("frame %d (%s vs %s): chamfer %.6f, accuracy %.6f, completeness %.6f, normal consistency %.4f"
                % (i, frames[i], gts[i], m["chamfer"], m["accuracy"], m["completeness"], m["normal_consistency"]))
    keys = [k for k in rows[0] if k not in ("frame", "pred", "gt")]
    result = {"frames": rows, "mean": {k: sum(r[k] for r in rows) / len(rows) for k in keys},
              "settings": {"n_samples": int(n_samples), "seed": int(seed), "thresholds": [float(t) for t in thresholds], "device": str(device),
                           "mode": mode, "gt_transform": None if gt_transform is None else np.asarray(gt_transform, dtype=np.float64).tolist()}}
    if clean_gt:
        result["settings"]["clean_gt"] = True
    if emd_samples:
        result["settings"]["emd_samples"] = int(emd_samples)
    if iou_samples:
        result["settings"]["iou_samples"] = int(iou_samples)
    with open(os.path.join(pred_dir, "mesh_metrics.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    return result


def _parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_metrics",
                                 description="Chamfer distance, F-score and normal consistency of frame_<i>.ply against ground-truth meshes.")
    ap.add_argument("pred_dir")
    ap.add_argument("gt_dir")
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.005, 0.01, 0.02])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--mode", choices=("samples", "surface"), default="samples",
                    help="samples: sample to nearest sample (carries the sampling floor); surface: sample to the other surface, exact")
    ap.add_argument("--clean-gt", action="store_true", help="weld and clean the ground-truth meshes on load (dgs_amd.mesh_clean.clean_mesh)")
    ap.add_argument("--emd", type=int, default=0, metavar="N",
                    help="also the earth mover's distance of the first N samples of each mesh (one-to-one matching, dgs_amd.mesh_metrics.emd)")
    ap.add_argument("--iou", type=int, default=0, metavar="N",
                    help="also the volumetric IoU from N points in the joint bounding box (winding numbers, dgs_amd.mesh_metrics.volume_iou)")
    return ap


def main(argv=None):
    a = _parser().parse_args(argv)
    return evaluate_meshes(a.pred_dir, a.gt_dir, n_samples=a.samples, seed=a.seed, thresholds=tuple(a.thresholds), device=a.device, log=print,
                           mode=a.mode, clean_gt=a.clean_gt, emd_samples=a.emd, iou_samples=a.iou)


if __name__ == "__main__":
    main()
