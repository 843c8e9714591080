"""Mesh clean-up on the tensors' own device: connected components, component statistics and the reference's clean_mesh, without
open3d / trimesh.

  component_labels             the primitive: connected components of a graph given as groups of nodes
  cluster_connected_triangles  <- open3d's TriangleMesh.cluster_connected_triangles (utils/mesh_utils.py:24-45 and
                                  render_mesh_trajectory.py:41-88 are built on it): a cluster per triangle, triangles and area per cluster
  filter_components            <- utils/mesh_utils.py:24-45 post_process_mesh: mesh.keep_largest_components with every step on the device
  clean_mesh                   <- render_mesh_trajectory.py:41-88 clean_mesh; its fill_holes is dgs_amd.mesh_fill's, off by default
(Simplification -- open3d's simplify_vertex_clustering -- is dgs_amd.mesh_simplify; it shares the face steps of clean_mesh.)

On a HIP device the components are the union-find kernels of libdgs_mesh_ops.so (dgs_cc_labels, include/dgs_mesh_ops.h); on CPU
tensors component_labels runs a PyTorch label propagation.  The label of a node is the smallest node id of its component, which is
unique, so both paths and every run give the same integers.  Everything around the labels is PyTorch on the tensors' device
(sorts, run lengths, cumsum, gathers): integer work whose result does not depend on the device either.

ADJACENCY.  "vertex": two triangles that share a vertex are connected (what mesh.keep_largest_components does).  "edge": two
triangles are connected when they share an edge, open3d's meaning: two pieces that touch in one vertex are two clusters.  An edge
that more than two triangles share (non-manifold) connects all of them; an "edge" from a vertex to itself (a degenerate triangle)
connects nothing."""
import numpy as np
import torch

from .mesh_topology import _check_mesh, _compact, _first_proper_faces, half_edges, sorted_edge_keys

_ADJACENCY = ("vertex", "edge")


# ---- the primitive --------------------------------------------------------------------------------------------------------------
def _labels_torch(groups, n_nodes):
    """Label propagation with pointer jumping, any k: every round each group pulls the labels of its nodes, and of their current
    labels' nodes, down to the group's minimum; then every label is replaced by its root.  label[x] <= x and label[x] is in x's
    component throughout, so the fixed point -- every group of one label, every label its own label -- is the component's minimum."""
    label = torch.arange(n_nodes, dtype=torch.int64, device=groups.device)
    if groups.shape[0] == 0:
        return label
    k = groups.shape[1]
    flat = groups.reshape(-1)
    while True:
        cur = label[groups]                                   # [G,k]
        m = cur.amin(1, keepdim=True).expand(-1, k).reshape(-1)
        new = label.clone()
        new.scatter_reduce_(0, flat, m, "amin")               # the nodes of the group ...
        new.scatter_reduce_(0, cur.reshape(-1), m, "amin")    # ... and the roots they hung below
        while True:                                           # pointer jumping: every label points at its root
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        if torch.equal(new, label):
            return label
        label = new


def component_labels(groups, n_nodes):
    """label [n_nodes] int64 on the device of groups [G,k] (an integer tensor, k >= 1): the smallest node id of the component of
    every node, where all nodes named by one group are in the same component.  A node that no group names keeps its own id; repeated
    groups and groups that name a node twice are legal; an id outside [0, n_nodes) is a ValueError.  A mesh's faces [F,3] are a
    valid input as they stand (components over shared vertices).
    HIP tensors: dgs_cc_labels (k in {2, 3}; other k are rewritten as the k - 1 pairs (first node, other node)).  CPU tensors: the
    PyTorch statement above.  The result is the same integers on both."""
    if not torch.is_tensor(groups) or groups.dim() != 2 or groups.is_floating_point() or groups.dtype == torch.bool:
        raise ValueError("component_labels: groups must be an integer tensor [G,k]")
    n_nodes = int(n_nodes)
    if n_nodes < 0 or n_nodes >= 2 ** 31:
        raise ValueError("component_labels: n_nodes must be in [0, 2^31)")
    G, k = groups.shape
    on_host = groups.device.type == "cpu"
    if G and k and (on_host or k == 1 or groups.dtype != torch.int32):      # (int32 groups of a HIP tensor: _mesh_ops.cc_labels checks)
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(groups)).tolist())
        if lo < 0 or hi >= n_nodes:                           # before any narrowing: an id that does not fit int32 must not wrap into the range
            raise ValueError("component_labels: node ids in [%d, %d] but n_nodes is %d" % (lo, hi, n_nodes))
    if G == 0 or k < 2:
        return torch.arange(n_nodes, dtype=torch.int64, device=groups.device)
    if on_host:
        return _labels_torch(groups.long(), n_nodes)
    from . import _mesh_ops   # a missing library is an error, never a reason to run the PyTorch statement instead
    groups = groups.to(torch.int32)
    if k > 3:
        groups = torch.stack((groups[:, :1].expand(-1, k - 1), groups[:, 1:]), -1).reshape(-1, 2)
    return _mesh_ops.cc_labels(groups.contiguous(), n_nodes).long()


# ---- triangles ------------------------------------------------------------------------------------------------------------------
def _face_labels(n_vertices, faces, adjacency):
    """[F] int64: a label per face that is equal for two faces iff they are in one cluster (a vertex id under "vertex", a face id
    under "edge").  Raises ValueError for a vertex id outside [0, n_vertices)."""
    if adjacency not in _ADJACENCY:
        raise ValueError("adjacency must be 'vertex' or 'edge', not %r" % (adjacency,))
    F = faces.shape[0]
    if adjacency == "vertex" or F == 0:
        return component_labels(faces, n_vertices)[faces[:, 0].long()]
    f = faces.long()
    lo, hi = (int(x) for x in torch.stack(torch.aminmax(f)).tolist())
    if lo < 0 or hi >= n_vertices:
        raise ValueError("component_labels: node ids in [%d, %d] but n_nodes is %d" % (lo, hi, n_vertices))
    key, order = sorted_edge_keys(*half_edges(f))            # edge e of face i: corners e and e + 1; half-edge 3 i + e
    face = order // 3
    # neighbours in a run of equal keys: a run of m faces gives a chain of m - 1 pairs; a key of two equal halves is no edge
    pair = (key[1:] == key[:-1]) & ((key[1:] >> 32) != (key[1:] & 0xFFFFFFFF))
    groups = torch.stack((face[:-1][pair], face[1:][pair]), -1)
    return component_labels(groups, F)


def _number_clusters(face_label, n_label_nodes):
    """(cluster [F] int64, n): clusters numbered 0 .. n - 1 in ascending order of their smallest face."""
    F = face_label.shape[0]
    dev = face_label.device
    if F == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev), 0
    ids = torch.arange(F, dtype=torch.int64, device=dev)
    first = torch.full((n_label_nodes,), F, dtype=torch.int64, device=dev).scatter_reduce_(0, face_label, ids, "amin")
    rep = first[face_label]                                   # the smallest face of every face's cluster
    is_rep = torch.zeros(F, dtype=torch.bool, device=dev)
    is_rep[rep] = True
    rank = torch.cumsum(is_rep, 0) - 1
    cluster = rank[rep]
    return cluster, int(rank[-1]) + 1


def _label_counts(label, n_nodes):
    """(counts [n_nodes] int64: how often every value occurs in label, 0 for values that do not occur; sizes [n]: the non-zero
    counts in ascending order of their value).  A sort and its run lengths, not bincount: a mesh is mostly one component, and a
    histogram by atomics sends every face to the same address (19 ms for 1.6 M faces of one component on an MI355X; the sort takes
    0.2 ms and does not care)."""
    values, sizes = torch.unique_consecutive(torch.sort(label).values, return_counts=True)
    counts = torch.zeros(n_nodes, dtype=torch.int64, device=label.device)
    counts[values] = sizes
    return counts, sizes


def face_areas(vertices, faces):
    """[F] float64: half the norm of the cross product of two edge vectors, computed in float64."""
    v = vertices.double()
    f = faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)


@torch.no_grad()
def cluster_connected_triangles(vertices, faces, adjacency="vertex"):
    """open3d's cluster_connected_triangles -> (face_cluster [F] int64, n_triangles [n] int64, area [n] float64) on the tensors'
    device.  Clusters are numbered 0 .. n - 1 in ascending order of their smallest face index.  face_cluster and n_triangles are exact
    and the same on every device and run.  The areas are float64 sums formed by index_add_, which on a device adds in the order
    its atomics land: the one output that is not bit-reproducible there (it differs from the CPU sum by the rounding of a
    reordered float64 sum, ~1e-16 relative per term)."""
    _check_mesh("cluster_connected_triangles", vertices, faces)
    n_nodes = vertices.shape[0] if adjacency == "vertex" else faces.shape[0]
    cluster, n = _number_clusters(_face_labels(vertices.shape[0], faces, adjacency), n_nodes)
    counts = _label_counts(cluster, n)[0]
    area = torch.zeros(n, dtype=torch.float64, device=faces.device).index_add_(0, cluster, face_areas(vertices, faces))
    return cluster, counts, area


@torch.no_grad()
def filter_components(vertices, faces, colors=None, n_keep=1000, min_faces=50, adjacency="vertex"):
    """The rule of mesh.keep_largest_components -- keep the components that have at least as many faces as the n_keep-th largest
    one, and at least min_faces; renumber the faces and drop the vertices nothing refers to -- with every step on the tensors'
    device (a sort and its run lengths for the sizes, threshold, mask, cumsum remap, gathers); the result stays there.  With
    adjacency="vertex" it returns exactly what keep_largest_components returns: the same vertices, faces and colours in the same
    order, bit for bit.  adjacency="edge" counts components open3d's way."""
    _check_mesh("filter_components", vertices, faces, colors)
    F, dev = faces.shape[0], faces.device
    keep = torch.ones(F, dtype=torch.bool, device=dev)
    if F:
        label = _face_labels(vertices.shape[0], faces, adjacency)
        n_nodes = vertices.shape[0] if adjacency == "vertex" else F
        counts, sizes = _label_counts(label, n_nodes)         # faces per component at its label, 0 elsewhere; the n components' sizes
        ranked = torch.sort(sizes, descending=True).values
        k = min(int(n_keep), ranked.shape[0])                 # ranked ascending [-k] = descending [k - 1]; k < 1 means index 0 ascending
        kth = ranked[k - 1 if k >= 1 else ranked.shape[0] - 1]
        keep = counts[label] >= torch.clamp(kth, min=int(min_faces))
    return _compact(vertices, faces, colors, keep)


@torch.no_grad()
def clean_mesh(vertices, faces, colors=None, min_triangles_connected=-1, adjacency="edge", fill_holes=None):
    """The reference's clean_mesh (render_mesh_trajectory.py:41-88), on the tensors' device -> (vertices, faces, colors), colors None
    if none were given.  Without fill_holes (None, the default) it is the reference's without its last step:
      (a) weld vertices with exactly equal coordinates (-0.0 equals 0.0; no tolerance): the first occurrence survives and keeps its
          colour, survivors stay in their original order;
      (b) drop a triangle that repeats an earlier one up to a rotation of its corners (opposite winding is a different triangle):
          the first occurrence survives;
      (c) drop triangles that name a vertex twice;
      (d) if min_triangles_connected > 0, drop the components (by `adjacency`) with fewer faces than that;
      (e) drop the vertices nothing refers to and renumber;
      (f) if fill_holes is an integer, close every hole of up to that many edges: mesh_fill.fill_holes(max_hole_edges=fill_holes)
          (fp32 vertices only).  The reference's filler, trimesh's, closes loops of 3 and 4 edges.
    Surviving faces keep their order and winding.  Idempotent."""
    _check_mesh("clean_mesh", vertices, faces, colors)
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    f = faces.long()
    if F and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError("clean_mesh: face index out of range")
    if V:                                                     # (a): rows of equal bit patterns after -0.0 -> 0.0
        bits = (vertices + 0.0).contiguous().view(torch.int32 if vertices.dtype == torch.float32 else
                                                  torch.int64 if vertices.dtype == torch.float64 else torch.int16)
        _, inverse = torch.unique(bits, dim=0, return_inverse=True)
        ids = torch.arange(V, dtype=torch.int64, device=dev)
        first = torch.full((V,), V, dtype=torch.int64, device=dev).scatter_reduce_(0, inverse, ids, "amin")
        f = first[inverse][f]                                 # every corner named by the first vertex at its position
    f = f[_first_proper_faces(f)]                             # (b), (c)
    if min_triangles_connected > 0 and f.shape[0]:            # (d)
        label = _face_labels(V, f, adjacency)
        counts = _label_counts(label, V if adjacency == "vertex" else f.shape[0])[0]
        f = f[counts[label] >= int(min_triangles_connected)]
    out = _compact(vertices, f.to(faces.dtype), colors, torch.ones(f.shape[0], dtype=torch.bool, device=dev))   # (e)
    if fill_holes is None:
        return out
    from .mesh_fill import fill_holes as fill                 # (f); (mesh_fill imports this module)
    return fill(*out, max_hole_edges=fill_holes)


# ---- shell ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    import os
    from . import io as dio
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_clean",
                                 description="Weld and clean a triangle mesh (the reference's clean_mesh; holes: python -m dgs_amd.mesh_fill); optionally keep its largest components.")
    ap.add_argument("input", help=".ply or .obj")
    ap.add_argument("output", help=".ply")
    ap.add_argument("--min-triangles", type=int, default=-1, help="drop components with fewer faces (default: keep all)")
    ap.add_argument("--keep", type=int, default=None, help="then keep the N largest components (post_process_mesh)")
    ap.add_argument("--adjacency", choices=_ADJACENCY, default="edge")
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
    v, f, c = clean_mesh(v, f, c, min_triangles_connected=a.min_triangles, adjacency=a.adjacency)
    if a.keep is not None:
        v, f, c = filter_components(v, f, c, n_keep=a.keep, min_faces=0, adjacency=a.adjacency)
    dio.write_mesh_ply(a.output, v, f, c)
    print("%s: %d vertices, %d faces -> %s: %d vertices, %d faces" % (a.input, n_v, n_f, a.output, v.shape[0], f.shape[0]))


if __name__ == "__main__":
    main()
