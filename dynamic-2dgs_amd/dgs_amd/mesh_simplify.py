"""Mesh simplification on the tensors' own device: vertex clustering with quadric placement, without open3d.

  simplify_mesh  <- open3d's TriangleMesh.simplify_vertex_clustering(voxel_size, contraction=Quadric / Average)

All vertices of one cell of a regular grid become one vertex; a face whose corners fall into fewer than three cells disappears.
Under "quadric" the new vertex minimises the summed squared distances to the planes of the faces that touch the cell (area-weighted,
regularised towards the cell's mean), so corners and creases stay where they are; under "average" it is the mean of the cell's
vertices.  It cannot fail on bad topology, and it promises none: clustering can pinch thin parts into non-manifold edges.

include/dgs_mesh_ops.h states the arithmetic.  The sums are int64 fixed-point sums, exact in any order, and the solve is spelled out
operation by operation, so the HIP kernels (dgs_simplify_accumulate, dgs_simplify_solve) and the PyTorch statement below give the
same bits.  HIP tensors run the kernels, CPU tensors the statement; the cells before them (a sort and its run lengths) and the
faces after them are PyTorch on the tensors' device either way."""
import math

import numpy as np
import torch

from .mesh_topology import LAMBDA_EXP, _check_mesh, _compact, _first_proper_faces, face_normals, quadric_solve

Q, W_MAX = 24, 16                         # fixed-point bits of the quadric sums, largest face weight (lambda = 2^LAMBDA_EXP)
POS_BITS, COL_BITS = 30, 24               # fixed-point bits of the position and colour sums
GRID_BITS = 21                            # cells per axis: ijk in [0, 2^21)
_PLACEMENT = ("average", "quadric")


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _cells(vertices, cell, origin):
    """(cluster [V] int64, centre [C,3] fp32, problems [4] bool -- read once by the caller) for fp32 vertices [V >= 1,3]; cell and
    origin are fp32 tensors [1] and [3] on the device (tensors, not Python numbers: a division by a number may be computed as a
    multiplication by its reciprocal)."""
    q = torch.floor((vertices - origin) / cell)
    problems = torch.stack((~torch.isfinite(vertices).all(), ~torch.isfinite(origin).all(), (q < 0).any() | ~torch.isfinite(q).all(),
                            (q >= 2 ** GRID_BITS).any()))
    ijk = q.clamp(0, 2 ** GRID_BITS - 1).long()             # (the clamp only matters for input that is refused anyway)
    key = (ijk[:, 0] << (2 * GRID_BITS)) | (ijk[:, 1] << GRID_BITS) | ijk[:, 2]
    occupied, cluster = torch.unique(key, return_inverse=True)                  # ascending: the rank of (i, j, k)
    mask = 2 ** GRID_BITS - 1
    ijk_c = torch.stack((occupied >> (2 * GRID_BITS), (occupied >> GRID_BITS) & mask, occupied & mask), -1)
    centre = origin + (ijk_c.float() + 0.5) * cell
    return cluster, centre, problems


def _fixed(x, bits):
    return torch.round(x * float(2 ** bits)).long()


def _accumulate_torch(vertices, colors, faces, cluster, centre, cell):
    """rows [C,16] int64: the sums of include/dgs_mesh_ops.h, step 2, with index_add_ (integers: exact on every device)."""
    C, dev = centre.shape[0], vertices.device
    add = lambda idx, val: torch.zeros((C,) + val.shape[1:], dtype=torch.int64, device=dev).index_add_(0, idx, val)
    count = add(cluster, torch.ones_like(cluster))
    pos = add(cluster, _fixed((vertices - centre[cluster]) / cell, POS_BITS))
    col = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    if colors is not None:
        col = add(cluster, _fixed(torch.nan_to_num(colors, nan=0.0).clamp(0.0, 1.0), COL_BITS))
    quad = torch.zeros((C, 9), dtype=torch.int64, device=dev)
    if faces.shape[0]:
        p = vertices[faces]                                                     # [F,3 corners,3]
        k = cluster[faces]                                                      # [F,3]
        n, l = face_normals(p)
        ok = (l > 0) & torch.isfinite(l)
        p, k, n, l = p[ok], k[ok], n[ok], l[ok]
        nh = n / l[:, None]
        w = torch.minimum((0.5 * l) / (cell * cell), torch.full_like(l, float(W_MAX)))
        for c in range(3):                                                      # corner c speaks for its cluster if no earlier corner is in it
            first = torch.ones(l.shape[0], dtype=torch.bool, device=dev)
            for e in range(c):
                first &= k[:, c] != k[:, e]
            kc, pc, nc, wc = k[first, c], p[first, c], nh[first], w[first]
            m = (k[first] == kc[:, None]).sum(1)
            u = (pc - centre[kc]) / cell
            d = -((nc[:, 0] * u[:, 0] + nc[:, 1] * u[:, 1]) + nc[:, 2] * u[:, 2])
            terms = [(wc * nc[:, i]) * nc[:, j] for i in range(3) for j in range(i, 3)] + [(wc * d) * nc[:, i] for i in range(3)]
            quad += add(kc, _fixed(torch.stack(terms, -1), Q) * m[:, None])
    return torch.cat((count[:, None], pos, col, quad), 1)


def _solve_torch(rows, centre, cell, quadric, with_colors):
    """(vertices [C,3] fp32, colors [C,3] fp32 or None): include/dgs_mesh_ops.h, step 3, operation by operation in float64."""
    r = rows.double()
    count = r[:, 0]
    xb = torch.nan_to_num(r[:, 1:4] / (count * float(2 ** POS_BITS))[:, None], nan=0.0).clamp(-1.0, 1.0)
    x = xb
    if quadric:
        y, good = quadric_solve([r[:, 7 + i] for i in range(6)], [r[:, 13 + i] for i in range(3)], xb)
        good = good & (y.abs() <= 1.0).all(1)
        x = torch.where(good[:, None], y, xb)
    vertices = centre + x.float() * cell
    colors = None
    if with_colors:
        colors = torch.where((count > 0)[:, None], (r[:, 4:7] / (count * float(2 ** COL_BITS))[:, None]).float(), torch.zeros((), device=rows.device))
    return vertices, colors


# ---- the function ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def simplify_mesh(vertices, faces, colors=None, cell_size=None, placement="quadric", origin=None, return_cluster=False):
    """open3d's simplify_vertex_clustering -> (vertices [C',3] fp32, faces [F',3] in the dtype of `faces`, colors [C',3] or None)
    on the tensors' device, and with return_cluster=True also [V] int64: the output vertex of every input vertex, -1 where it was
    dropped.
      cell_size   the edge of the grid's cells (open3d's voxel_size), in the units of the mesh
      placement   "quadric" (default) or "average"
      origin      three numbers, the grid's corner; default: the per-axis minimum of the vertices - cell_size / 2 (open3d's)
    Output vertices are ordered by their cell (i, j, k) ascending; surviving faces keep their order and winding; every output
    vertex lies within one cell of its cell's centre per axis.  A face with corners in fewer than three cells, a later repeat of a
    face up to rotation and the vertices nothing refers to any more are dropped.
    ValueError: cell_size not positive and finite, non-finite coordinates, a face index out of range, a grid of more than 2^21
    cells along an axis (or vertices below a given origin).  HIP tensors run the kernels of libdgs_mesh_ops.so -- a missing library
    is an error --, CPU tensors the PyTorch statement above: the results are bit-identical."""
    _check_mesh("simplify_mesh", vertices, faces, colors)
    if vertices.dtype != torch.float32 or (colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape)):
        raise ValueError("simplify_mesh: vertices and colors must be fp32 [V,3]")
    if placement not in _PLACEMENT:
        raise ValueError("simplify_mesh: placement must be 'quadric' or 'average', not %r" % (placement,))
    if cell_size is None or isinstance(cell_size, bool) or not isinstance(cell_size, (int, float, np.floating, np.integer)):
        raise ValueError("simplify_mesh: cell_size must be a number")
    cell_f = float(np.float32(cell_size))
    if not (cell_f > 0.0 and math.isfinite(cell_f)):
        raise ValueError("simplify_mesh: cell_size must be positive and finite (as fp32)")
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    f = faces.long()
    empty_map = torch.full((V,), -1, dtype=torch.int64, device=dev)
    if V == 0:
        if F:
            raise ValueError("simplify_mesh: face index out of range")
        out = (vertices.clone(), faces.clone(), None if colors is None else colors.clone())
        return out + (empty_map,) if return_cluster else out
    cell = torch.full((1,), cell_f, dtype=torch.float32, device=dev)
    if origin is None:
        org = vertices.amin(0) - cell * 0.5
    else:
        org = torch.as_tensor(origin, dtype=torch.float32).reshape(3).to(dev)
    vertices = vertices.contiguous()
    cluster, centre, problems = _cells(vertices, cell, org)
    if F:
        problems = torch.cat((problems, ((f < 0) | (f >= V)).any().reshape(1)))
    problems = problems.tolist()                                                # the one read of the checks
    if problems[0]:
        raise ValueError("simplify_mesh: non-finite vertex coordinates")
    if problems[1]:
        raise ValueError("simplify_mesh: non-finite origin")
    if problems[2]:
        raise ValueError("simplify_mesh: vertices below the grid's origin, or a grid too large for fp32")
    if problems[3]:
        raise ValueError("simplify_mesh: more than 2^%d cells along an axis: raise cell_size" % GRID_BITS)
    if F and problems[4]:
        raise ValueError("simplify_mesh: face index out of range")
    quadric = placement == "quadric"
    if dev.type == "cpu":
        rows = _accumulate_torch(vertices, colors, f, cluster, centre, cell)
        new_v, new_c = _solve_torch(rows, centre, cell, quadric, colors is not None)
    else:
        from . import _mesh_ops   # a missing library is an error, never a reason to run the PyTorch statement instead
        rows = _mesh_ops.simplify_accumulate(vertices, None if colors is None else colors.contiguous(), f.to(torch.int32).contiguous(),
                                             cluster.to(torch.int32), centre.contiguous(), cell_f)
        new_v, new_c = _mesh_ops.simplify_solve(rows, centre.contiguous(), cell_f, quadric, colors is not None)
    g = cluster[f]                                                              # step 4
    g = g[_first_proper_faces(g)]
    C = centre.shape[0]
    used = torch.zeros(C, dtype=torch.bool, device=dev)
    used[g.reshape(-1)] = True
    out = _compact(new_v, g.to(faces.dtype), new_c, torch.ones(g.shape[0], dtype=torch.bool, device=dev))
    if not return_cluster:
        return out
    remap = torch.where(used, torch.cumsum(used, 0) - 1, torch.full((), -1, dtype=torch.int64, device=dev))
    return out + (remap[cluster],)


# ---- shell ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    import os
    from . import io as dio
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_simplify",
                                 description="Simplify a triangle mesh by vertex clustering (open3d's simplify_vertex_clustering).")
    ap.add_argument("input", help=".ply or .obj")
    ap.add_argument("output", help=".ply")
    ap.add_argument("--cell", type=float, required=True, help="edge of the grid's cells, in the units of the mesh")
    ap.add_argument("--placement", choices=_PLACEMENT, default="quadric")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    ext = os.path.splitext(a.input)[1].lower()
    if ext == ".ply":
        v, f, c = dio.read_mesh_ply(a.input)
    elif ext == ".obj":
        (v, f), c = dio.read_mesh_obj(a.input), None
    else:
        raise ValueError("%s is neither .ply nor .obj" % a.input)
    dev = torch.device(a.device)
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    v, f, c = to(v), to(f), to(c)
    n_v, n_f = v.shape[0], f.shape[0]
    v, f, c = simplify_mesh(v, f, c, cell_size=a.cell, placement=a.placement)
    dio.write_mesh_ply(a.output, v, f, c)
    print("%s: %d vertices, %d faces -> %s: %d vertices, %d faces" % (a.input, n_v, n_f, a.output, v.shape[0], f.shape[0]))


if __name__ == "__main__":
    main()
