"""What the mesh edit modules (mesh_clean, mesh_simplify, mesh_smooth, mesh_decimate, mesh_fill) share: input checks and compaction,
the undirected edges of a face list, small geometry, the statement of the regularised quadric solve and the switch between the HIP
kernels and the PyTorch statements.  A helper lives here when two of those modules use it, under a name that belongs to neither;
csrc/mesh_common.h is the same shelf for the kernels.  Everything is PyTorch on the tensors' own device."""
import math

import torch

LAMBDA_EXP = -10                       # the quadric solve is regularised by lambda = 2^LAMBDA_EXP times the trace


# ---- input checks and compaction ------------------------------------------------------------------------------------------------
def _check_mesh(what, vertices, faces, colors=None):
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3 or not vertices.is_floating_point():
        raise ValueError("%s: vertices must be a floating-point tensor [V,3]" % what)
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: faces must be an int32 or int64 tensor [F,3]" % what)
    if faces.device != vertices.device or (colors is not None and (colors.device != vertices.device or colors.shape[0] != vertices.shape[0])):
        raise ValueError("%s: vertices, faces and colors must live on one device, one colour per vertex" % what)
    if vertices.shape[0] >= 2 ** 31 or faces.shape[0] >= 2 ** 31:
        raise ValueError("%s: at most 2^31 - 1 vertices and faces" % what)


def _faces_checked(what, n_vertices, faces):
    """faces [F,3] as int64 after the range check (one aminmax, read on the host)."""
    if not torch.is_tensor(faces) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("%s: faces must be an int32 or int64 tensor [F,3]" % what)
    n_vertices = int(n_vertices)
    if n_vertices < 0 or n_vertices >= 2 ** 31:
        raise ValueError("%s: n_vertices must be in [0, 2^31)" % what)
    f = faces.long()
    if f.shape[0]:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(f)).tolist())
        if lo < 0 or hi >= n_vertices:
            raise ValueError("%s: face index out of range (ids in [%d, %d], %d vertices)" % (what, lo, hi, n_vertices))
    return f


def _three_distinct(f):
    """[F] bool for faces f [F,3]: true for a face that names three different vertices."""
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


def _compact(vertices, faces, colors, keep_face):
    """Keep the faces of the mask, drop the vertices nothing refers to, renumber: the tail of mesh.keep_largest_components."""
    f = faces[keep_face]
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[f.reshape(-1).long()] = True
    remap = torch.cumsum(used, 0) - 1
    f = remap[f.long()].to(faces.dtype)
    return vertices[used], f, None if colors is None else colors[used]


def _first_proper_faces(f):
    """[F] bool for faces f [F,3] int64: steps (b) and (c) of clean_mesh (simplify_mesh applies them to the cluster ids) -- true for
    a face that names three different vertices and repeats no earlier face up to a rotation of its corners."""
    F, dev = f.shape[0], f.device
    keep = torch.ones(F, dtype=torch.bool, device=dev)
    if F:
        # (b): rotate the smallest corner to the front; rows that are equal then are rotations of each other
        shift = f.argmin(1, keepdim=True)
        canon = torch.gather(f, 1, (shift + torch.arange(3, device=dev)) % 3)
        _, inverse = torch.unique(canon, dim=0, return_inverse=True)
        ids = torch.arange(F, dtype=torch.int64, device=dev)
        first = torch.full((F,), F, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, ids, "amin")
        keep = first[inverse] == ids
        keep &= _three_distinct(f)                                                                  # (c)
    return keep


# ---- the undirected edges of a face list ----------------------------------------------------------------------------------------
def half_edges(f):
    """(a [3F], b [3F]) for faces f [F,3]: half-edge 3 g + c runs from corner c (a) to corner c + 1 (b) of face g."""
    return f.reshape(-1), f.roll(-1, 1).reshape(-1)


def sorted_edge_keys(a, b):
    """(key [3F], order [3F]) int64 for the half-edges a -> b of half_edges(f) (int64 ids in [0, 2^31)): the keys min << 32 | max in
    ascending order, by ONE stable sort, so equal keys stay in half-edge (face) order, and the half-edge behind every sorted key.
    A face that names a vertex twice contributes the key v << 32 | v: a caller that takes such faces tells it by its equal halves."""
    return torch.sort((torch.minimum(a, b) << 32) | torch.maximum(a, b), stable=True)


def undirected_edges(f):
    """(key [3F], order [3F], start [E], count [E]) int64 for faces f [F,3] int64: sorted_edge_keys of its half-edges and, on top of
    them, the runs of equal keys -- start: the first position of every run, count: its length, so key[start] are the E distinct
    edges, ascending, and count the half-edges of each.  A caller that needs less takes sorted_edge_keys and adds its own lines."""
    key, order = sorted_edge_keys(*half_edges(f))
    count = torch.unique_consecutive(key, return_counts=True)[1]
    return key, order, torch.cumsum(count, 0) - count, count


# ---- small geometry -------------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return torch.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), -1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def face_normals(p):
    """(n [F,3], l [F]) fp32 for the fp32 corners p [F,3 corners,3] of F faces: the normal (b - a) x (c - a) and its length through
    the fp64 square root (the device's fp32 square root is not correctly rounded) -- face_normal of csrc/mesh_common.h."""
    n = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    return n, torch.sqrt(_dot(n, n).double()).float()


def normal_lengths(pos, f):
    """face_normals of the faces f [F,3] int64 of the vertices pos [V,3] fp32."""
    return face_normals(pos[f])


def _frame(vertices):
    """(centre [3] fp32 tensor, scale: a power of two) -- |(v - centre) * scale| <= 1 (+ one rounding) per axis."""
    lo, hi = vertices.amin(0), vertices.amax(0)
    centre = (lo + hi) * 0.5
    half = float(((hi - lo) * 0.5).max())
    exp = 0 if not (half > 0.0 and math.isfinite(half)) else min(max(math.frexp(half)[1], -100), 100)
    return centre, 2.0 ** -exp


def quadric_solve(A, b, anchor):
    """(y [N,3] fp64, good [N] bool): the regularised system (A + g I) y = g anchor - b with g = trace(A) * 2^LAMBDA_EXP, by
    cofactors, operation by operation -- quadric_solve of csrc/mesh_common.h.  A: the six fp64 columns xx xy xz yy yz zz, b: the
    three of the linear term, anchor [N,3] fp64.  good: the trace and the determinant are positive and the determinant is finite;
    the caller adds its own test of how far y may lie."""
    a00, a01, a02, a11, a12, a22 = A
    b0, b1, b2 = b
    t = (a00 + a11) + a22
    g = t * 2.0 ** LAMBDA_EXP
    m00, m11, m22 = a00 + g, a11 + g, a22 + g
    r0, r1, r2 = g * anchor[:, 0] - b0, g * anchor[:, 1] - b1, g * anchor[:, 2] - b2
    c00, c01, c02 = m11 * m22 - a12 * a12, a02 * a12 - a01 * m22, a01 * a12 - a02 * m11
    c11, c12, c22 = m00 * m22 - a02 * a02, a01 * a02 - m00 * a12, m00 * m11 - a01 * a01
    det = (m00 * c00 + a01 * c01) + a02 * c02
    y = torch.stack((((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det,
                     ((c02 * r0 + c12 * r1) + c22 * r2) / det), -1)
    return y, (t > 0) & (det > 0) & torch.isfinite(det)


# ---- the HIP switch -------------------------------------------------------------------------------------------------------------
_STATEMENT_EVERYWHERE = False          # tools/mesh_decimate_timing.py and tools/mesh_fill_timing.py set it to time the PyTorch statements on a HIP device; nothing else does


def _kernels(dev):
    """The binding of the HIP kernels for tensors on dev, or None where the PyTorch statement runs (CPU tensors)."""
    if dev.type == "cpu" or _STATEMENT_EVERYWHERE:
        return None
    from . import _mesh_ops   # a missing library is an error, never a reason to run the PyTorch statement instead
    return _mesh_ops
