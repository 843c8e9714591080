"""Mesh hole filling on the tensors' own device: boundary loops by list ranking, and a ring fill of every loop, without trimesh.

  boundary_loops  the rims of the holes of a mesh, each in hole order
  is_watertight   every undirected edge has exactly two half-edges, of opposite direction
  fill_holes      <- trimesh's fill_holes at the end of the reference's clean_mesh (render_mesh_trajectory.py:41-88), which closes
                     3- and 4-edge loops only; this one closes every simple loop of up to max_hole_edges edges

A TSDF fused from a finite set of views has cells that no view saw; marching tetrahedra skip them, so an extracted frame carries
open rims.  A HOLE is a closed cycle of boundary half-edges over simple vertices (one boundary half-edge in, one out).  Its rim is
found by numbering the boundary half-edges by tail vertex, labelling their cycles with the connected components of
dgs_amd.mesh_clean and ranking every cycle by pointer jumping (dgs_fill_rank).  A loop of n edges is closed by R = n / 2 pi
concentric rings of new vertices that shrink a smoothed copy of the rim onto its centre, joined by triangle strips; a loop of 3
gets one triangle.

include/dgs_mesh_ops.h states every step.  The sums of a loop are int64 fixed-point sums, exact in any order; everything else is
fp64, spelled out operation by operation, and rounded to fp32 once.  So the HIP kernels (dgs_fill_*) and the PyTorch statement below
give the same bits: HIP tensors run the kernels, CPU tensors the statement; the tables (one sort of packed keys, run lengths,
prefix sums) are PyTorch on the tensors' device either way.

WHAT IT IS NOT.  No fairing of the new vertices (uniform-weight Jacobi fairing made the fold-over count worse on staircase rims:
the rim is not convex, so Tutte's guarantee does not hold), no triangulation without new vertices, no rims through a bow-tie
vertex (they are left open), and no guarantee against fold-over on a rim that is not star-shaped about its centre or is strongly
non-planar."""
import numpy as np
import torch

from .mesh_clean import component_labels
from .mesh_topology import _check_mesh, _cross, _dot, _faces_checked, _frame, _kernels, _three_distinct, half_edges, sorted_edge_keys

POS_BITS, NRM_BITS, COL_BITS = 30, 28, 24              # fixed-point bits of the position, Newell and colour sums of a loop
TAPS = (1.0 / 256, 8.0 / 256, 28.0 / 256, 56.0 / 256, 70.0 / 256, 56.0 / 256, 28.0 / 256, 8.0 / 256, 1.0 / 256)   # [1/4 1/2 1/4] four times
RING_COLS = 10                                         # loop, k, R, n, count, first vertex, count before, first vertex before, first face, faces
DEFAULT_MAX_HOLE_EDGES = 128                           # a policy, not a measurement: a hole about 20 voxels across
_ID_LIMIT = 2 ** 31                                    # vertex and face totals stay below it (ids are int32 in the kernels)


def ring_count(n):
    """R of a loop of n edges: max(1, (113 n + 355) // 710), n / 2 pi in integers."""
    return max(1, (113 * int(n) + 355) // 710)


def fill_counts(n):
    """(new vertices, new faces) of a loop of n >= 3 edges."""
    n = int(n)
    if n == 3:
        return 0, 1
    R = ring_count(n)
    if R == 1:
        return 1, n
    m = [n, n] + [(n * (R - k) + R // 2) // R for k in range(2, R)]          # m[0]: the rim, m[k]: ring k < R
    return sum(m[1:]) + 1, 2 * n + sum(m[k - 1] + m[k] for k in range(2, R)) + m[R - 1]


# ---- half-edges and loops (PyTorch on the tensors' device, integers only) -------------------------------------------------------
def _proper(f):
    return f[_three_distinct(f)]


def boundary_half_edges(n_vertices, f):
    """The nodes of step 1 for faces f [F,3] int64 (three different vertices each) -> (tail [NB], head [NB], face [NB]) int64, in
    ascending order of (tail, head): the half-edges (a -> b) whose undirected edge occurs once among all half-edges, and the face
    each comes from.  One sort of the 3 F packed keys min << 32 | max, and one of the NB boundary half-edges."""
    a, b = half_edges(f)
    if a.shape[0] == 0:
        z = torch.zeros(0, dtype=torch.int64, device=f.device)
        return z, z, z
    key, order = sorted_edge_keys(a, b)
    differs = key[1:] != key[:-1]
    edge = torch.ones(1, dtype=torch.bool, device=f.device)
    once = order[torch.cat((edge, differs)) & torch.cat((differs, edge))]                     # a run of one: both neighbours differ
    tail, head = a[once], b[once]
    by_tail = torch.sort((tail << 32) | head).indices
    return tail[by_tail], head[by_tail], (once // 3)[by_tail]


def successors(n_vertices, tail, head):
    """succ [NB] int64: the node whose tail is the head of node h if that head is a simple vertex, else -1."""
    V = int(n_vertices)
    out_deg, in_deg = torch.bincount(tail, minlength=V), torch.bincount(head, minlength=V)
    simple = (out_deg == 1) & (in_deg == 1)
    first = torch.cumsum(out_deg, 0) - out_deg                # nodes are numbered by tail: the first node that leaves every vertex
    return torch.where(simple[head], first[head], torch.full_like(head, -1))


def rank_torch(succ, leader, n_rounds):
    """Step 2, the statement: rank [n] int32 from succ, leader [n] (any integer dtype) by n_rounds rounds of pointer jumping."""
    n, dev = succ.shape[0], succ.device
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    s, l = succ.long(), leader.long()
    end = (l < 0) | (s < 0) | (s >= n) | (s == l)
    nxt, dist = torch.where(end, ids, s), torch.where(end, 0, 1)
    for _ in range(int(n_rounds)):
        nxt, dist = nxt[nxt], (dist + dist[nxt]) & 0xFFFFFFFF
    rank = torch.where(l < 0, torch.full_like(l, -1), torch.where(l == ids, torch.zeros_like(l), (dist + 1) & 0x7FFFFFFF))
    return rank.to(torch.int32)


def rank_inputs(n_vertices, f, max_edges=None):
    """Step 1 for proper faces f [F,3] int64 -> None if no loop is to be ranked, else a dict of the nodes' tail and face [NB] int64,
    succ [NB] int64, leader [NB] int32 (-1: not ranked), label and size [NB] int64 (size at the leaders), ranked [NB] bool and
    n_rounds = ceil(log2(longest ranked loop)), fixed by one host read of the loop sizes."""
    dev = f.device
    tail, head, face = boundary_half_edges(n_vertices, f)
    NB = tail.shape[0]
    if NB == 0:
        return None
    if NB >= _ID_LIMIT:
        raise ValueError("boundary_loops: %d boundary half-edges do not fit int32 node ids" % NB)
    succ = successors(n_vertices, tail, head)
    has = succ >= 0
    ids = torch.arange(NB, dtype=torch.int64, device=dev)
    label = component_labels(torch.stack((ids[has], succ[has]), -1).to(torch.int32), NB)      # the smallest node of every list: its leader
    values, sizes = torch.unique_consecutive(torch.sort(label).values, return_counts=True)
    size = torch.zeros(NB, dtype=torch.int64, device=dev)
    size[values] = sizes
    open_list = torch.zeros(NB, dtype=torch.bool, device=dev)
    open_list[label[~has]] = True                                                             # a list is a cycle iff every node has a successor
    ranked = ~open_list[label] & (size[label] >= 3)
    if max_edges is not None:
        ranked &= size[label] <= int(max_edges)
    longest = int(torch.where(ranked, size[label], torch.zeros_like(size)).max())             # the host read that fixes the round count
    if longest == 0:
        return None
    return {"tail": tail, "face": face, "succ": succ, "leader": torch.where(ranked, label, torch.full_like(label, -1)).to(torch.int32),
            "label": label, "size": size, "ranked": ranked, "n_rounds": (longest - 1).bit_length()}


def _loops(n_vertices, f, max_edges=None):
    """Steps 1 and 2 for proper faces f [F,3] int64 -> (loop_vertices [B] int32, loop_offsets [L+1] int64, loop_faces [B] int64: the
    face behind every rim edge)."""
    dev = f.device
    t = rank_inputs(n_vertices, f, max_edges)
    if t is None:
        return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
    label, size, ranked = t["label"], t["size"], t["ranked"]
    ops = _kernels(dev)
    rank = (ops.fill_rank(t["succ"].to(torch.int32), t["leader"], t["n_rounds"]) if ops else rank_torch(t["succ"], t["leader"], t["n_rounds"])).long()
    is_leader = ranked & (label == torch.arange(label.shape[0], dtype=torch.int64, device=dev))
    loop_of = (torch.cumsum(is_leader, 0) - 1)[label]                                         # leaders ascend with their smallest vertex
    n_of = size[is_leader]
    offsets = torch.zeros(n_of.shape[0] + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(n_of, 0)
    at = (offsets[loop_of] + rank)[ranked]
    B = int(offsets[-1])
    loop_vertices = torch.zeros(B, dtype=torch.int32, device=dev)
    loop_vertices[at] = t["tail"][ranked].to(torch.int32)
    loop_faces = torch.zeros(B, dtype=torch.int64, device=dev)
    loop_faces[at] = t["face"][ranked]
    return loop_vertices, offsets, loop_faces


@torch.no_grad()
def boundary_loops(n_vertices, faces, max_edges=None):
    """(loop_vertices [B] int32, loop_offsets [L+1] int64) on the device of faces [F,3]: the rims of the holes, concatenated.  A hole
    is a closed cycle of boundary half-edges -- half-edges whose undirected edge occurs exactly once among all half-edges, the rule
    of mesh_smooth.boundary_vertices -- that visits simple vertices only (exactly one boundary half-edge leaves the vertex and one
    enters it): a cycle through a bow-tie vertex and an open chain are no holes.  Faces that name a vertex twice take no part.
    Every rim is in HOLE ORDER, the reverse of the boundary direction, so that a triangle (r_i, r_i+1, x) has the winding of the
    mesh; it starts at its smallest vertex id, and the rims are ordered by that id.  max_edges: only the loops of at most that many
    edges (default: all).  HIP tensors rank the cycles with dgs_fill_rank, CPU tensors with rank_torch: the same integers.
    ValueError: a face index outside [0, n_vertices), max_edges negative."""
    f = _faces_checked("boundary_loops", n_vertices, faces)
    if max_edges is not None and (isinstance(max_edges, bool) or not isinstance(max_edges, (int, np.integer)) or max_edges < 0):
        raise ValueError("boundary_loops: max_edges must be a non-negative integer")
    return _loops(int(n_vertices), _proper(f), max_edges)[:2]


@torch.no_grad()
def is_watertight(n_vertices, faces):
    """True when every undirected edge of the faces (those that name a vertex twice take no part) has exactly two half-edges, of
    opposite direction; a mesh without edges is not watertight.  ValueError: a face index outside [0, n_vertices)."""
    f = _proper(_faces_checked("is_watertight", n_vertices, faces))
    if f.shape[0] == 0:
        return False
    a, b = half_edges(f)
    directed = torch.sort((a << 32) | b).values
    count = torch.unique_consecutive(sorted_edge_keys(a, b)[0], return_counts=True)[1]
    return bool((count == 2).all() & (directed[1:] != directed[:-1]).all())


# ---- the layout of the new vertices and faces -----------------------------------------------------------------------------------
def ring_layout(n_old, loop_offsets):
    """Step 3 for the loops to fill -> dict of rings [NR,10] int32, vert_ring [n_new] int32, face_ring [n_new_faces] int32 and the two
    totals n_new, n_new_faces (the one host read that sizes the outputs)."""
    dev = loop_offsets.device
    n = loop_offsets[1:] - loop_offsets[:-1]
    L = n.shape[0]
    R = torch.clamp((113 * n + 355) // 710, min=1)
    start = torch.cumsum(R, 0) - R
    loop = torch.repeat_interleave(torch.arange(L, dtype=torch.int64, device=dev), R)
    k = torch.arange(loop.shape[0], dtype=torch.int64, device=dev) - start[loop] + 1
    nr, Rr = n[loop], R[loop]
    cnt = torch.where(k == Rr, (nr != 3).long(), torch.where(k == 1, nr, (nr * (Rr - k) + Rr // 2) // Rr))
    pcnt = torch.where(k == 1, nr, cnt.roll(1))
    nf = torch.where(nr == 3, torch.ones_like(nr), torch.where(k == Rr, pcnt, torch.where(k == 1, 2 * nr, pcnt + cnt)))
    vbase = int(n_old) + torch.cumsum(cnt, 0) - cnt
    pbase = torch.where(k == 1, torch.full_like(k, -1), vbase.roll(1))
    fbase = torch.cumsum(nf, 0) - nf
    n_new, n_new_faces = (int(x) for x in torch.stack((cnt.sum(), nf.sum())).tolist())
    if int(n_old) + n_new >= _ID_LIMIT or n_new_faces >= _ID_LIMIT:
        raise ValueError("fill_holes: %d vertices / %d new faces do not fit int32 ids" % (int(n_old) + n_new, n_new_faces))
    rows = torch.arange(loop.shape[0], dtype=torch.int32, device=dev)
    return {"rings": torch.stack((loop, k, Rr, nr, cnt, vbase, pcnt, pbase, fbase, nf), -1).to(torch.int32).contiguous(),
            "vert_ring": torch.repeat_interleave(rows, cnt, output_size=n_new), "face_ring": torch.repeat_interleave(rows, nf, output_size=n_new_faces),
            "n_new": n_new, "n_new_faces": n_new_faces}


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _frame_point(vertices, centre, scale):
    return (vertices.double() - torch.tensor(centre, dtype=torch.float64, device=vertices.device)) * scale


def rim_torch(vertices, colors, loop_vertices, rim_loop, loop_offsets, centre, scale):
    """Step 5 -> (S [B,3] fp64, SC [B,3] fp64 or None, rows [L,16] int64)."""
    dev = vertices.device
    lv, rl = loop_vertices.long(), rim_loop.long()
    B, L = lv.shape[0], loop_offsets.shape[0] - 1
    off, n = loop_offsets[:-1][rl], (loop_offsets[1:] - loop_offsets[:-1])[rl]
    i = torch.arange(B, dtype=torch.int64, device=dev) - off
    P = _frame_point(vertices[lv], centre, scale)
    C = None
    if colors is not None:
        c = colors[lv]
        C = torch.where(c > 0, torch.where(c < 1, c, torch.ones_like(c)), torch.zeros_like(c)).double()
    S = SC = None
    for t, w in enumerate(TAPS):
        at = off + (i + (t - 4)) % n                          # (Python's remainder: never negative)
        S = w * P[at] if t == 0 else S + w * P[at]
        if C is not None:
            SC = w * C[at] if t == 0 else SC + w * C[at]
    nxt = P[off + (i + 1) % n]
    rows = torch.zeros((L, 16), dtype=torch.int64, device=dev)
    newell = torch.stack([(P[:, (a + 1) % 3] - nxt[:, (a + 1) % 3]) * (P[:, (a + 2) % 3] + nxt[:, (a + 2) % 3]) for a in range(3)], -1)
    val = [torch.round(P * float(2 ** POS_BITS)).long(), torch.round(newell * float(2 ** NRM_BITS)).long(),
           torch.round(C * float(2 ** COL_BITS)).long() if C is not None else torch.zeros((B, 3), dtype=torch.int64, device=dev)]
    rows[:, :9] = torch.zeros((L, 9), dtype=torch.int64, device=dev).index_add_(0, rl, torch.cat(val, -1))
    return S, SC, rows


def _ring_columns(lay, which):
    r = lay["rings"].long()[lay[which].long()]
    return [r[:, c] for c in range(RING_COLS)]


def vertices_torch(n_old, lay, loop_offsets, rows, S, SC, centre, scale):
    """Step 6 -> (new vertices [n_new,3] fp32, new colours [n_new,3] fp32 or None)."""
    dev = S.device
    loop, k, R, n, m, vbase = _ring_columns(lay, "vert_ring")[:6]
    off = loop_offsets[loop]
    j = int(n_old) + torch.arange(lay["n_new"], dtype=torch.int64, device=dev) - vbase
    num = j * n
    i0 = (num // m) % n
    i1 = (i0 + 1) % n
    t = ((num % m).double() / m.double())[:, None]
    u = (1.0 - k.double() / R.double())[:, None]
    inner = (k < R)[:, None]

    def ring(row_cols, bits, table):
        ce = row_cols.double() / (n.double() * float(2 ** bits))[:, None]
        s0, s1 = table[off + i0], table[off + i1]
        s = s0 + t * (s1 - s0)
        return torch.where(inner, ce + u * (s - ce), ce)

    y = ring(rows[loop, 0:3], POS_BITS, S)
    out = (torch.tensor(centre, dtype=torch.float64, device=dev) + y * (1.0 / scale)).float()
    return out, None if SC is None else ring(rows[loop, 6:9], COL_BITS, SC).float()


def _area(a, b, c, N):
    return _dot(_cross(b - a, c - a), N)


def faces_torch(lay, loop_offsets, loop_vertices, rows, vertices_out):
    """Step 7 -> new faces [n_new_faces,3] int64 (vertices_out: the input's vertices followed by the new ones)."""
    dev = loop_vertices.device
    lv = loop_vertices.long()
    loop, k, R, n, mi, vbase, m, pbase, fbase, nf = _ring_columns(lay, "face_ring")
    off = loop_offsets[loop]
    e = torch.arange(lay["n_new_faces"], dtype=torch.int64, device=dev) - fbase
    out = torch.zeros((lay["n_new_faces"], 3), dtype=torch.int64, device=dev)
    tri = n == 3
    fan = ~tri & (k == R)
    quad = ~tri & ~fan & (k == 1)
    merge = ~tri & ~fan & ~quad
    g = torch.nonzero(tri).reshape(-1)
    out[g] = torch.stack((lv[off[g]], lv[off[g] + 1], lv[off[g] + 2]), -1)
    for rim in (True, False):                                   # the fan over the rim (R = 1) and over ring R - 1
        g = torch.nonzero(fan & ((pbase < 0) == rim)).reshape(-1)
        a0, a1 = e[g], (e[g] + 1) % m[g]
        prev = (lambda i: lv[off[g] + i]) if rim else (lambda i: pbase[g] + i)
        out[g] = torch.stack((prev(a0), prev(a1), vbase[g]), -1)
    g = torch.nonzero(quad).reshape(-1)
    if g.shape[0]:
        i = e[g] >> 1
        i1 = (i + 1) % n[g]
        ids = [lv[off[g] + i], lv[off[g] + i1], vbase[g] + i1, vbase[g] + i]                  # r0 r1 q1 q0
        p = [vertices_out[x].double() for x in ids]
        N = rows[loop[g], 3:6].double()
        first = torch.minimum(_area(p[0], p[1], p[2], N), _area(p[0], p[2], p[3], N))         # diagonal r0 - q1
        second = torch.minimum(_area(p[0], p[1], p[3], N), _area(p[1], p[2], p[3], N))        # diagonal r1 - q0
        # (minimum propagates a NaN; the kernel's a < b ? a : b does not, but a NaN position is refused before it gets here)
        swap, odd = second > first, (e[g] & 1) == 1
        pick = lambda x, y, z: torch.stack((ids[x], ids[y], ids[z]), -1)
        out[g] = torch.where(swap[:, None], torch.where(odd[:, None], pick(1, 2, 3), pick(0, 1, 3)),
                             torch.where(odd[:, None], pick(0, 2, 3), pick(0, 1, 2)))
    g = torch.nonzero(merge & (e < m)).reshape(-1)
    out[g] = torch.stack((pbase[g] + e[g], pbase[g] + (e[g] + 1) % m[g], vbase[g] + (((e[g] + 1) * mi[g] - 1) // m[g]) % mi[g]), -1)
    g = torch.nonzero(merge & (e >= m)).reshape(-1)
    j = e[g] - m[g]
    out[g] = torch.stack((pbase[g] + (((j + 1) * m[g]) // mi[g]) % m[g], vbase[g] + (j + 1) % mi[g], vbase[g] + j), -1)
    return out


# ---- the function ---------------------------------------------------------------------------------------------------------------
def fill_loops(vertices, colors, loop_vertices, loop_offsets, clock=None):
    """Steps 3 to 7 for the rims loop_vertices [B] int32 / loop_offsets [L+1] int64 (L >= 1) of vertices [V,3] fp32 -> (vertices
    [V + n_new,3], colors likewise or None, new faces [n_new_faces,3] int32) on either device.  clock: called with the name of every
    phase as it ends (the timing tool's stopwatch)."""
    clock = clock or (lambda name: None)
    dev, V = vertices.device, vertices.shape[0]
    ops = _kernels(dev)
    centre, scale = _frame(vertices)
    centre = [float(x) for x in centre.tolist()]
    lay = ring_layout(V, loop_offsets)
    L = loop_offsets.shape[0] - 1
    rim_loop = torch.repeat_interleave(torch.arange(L, dtype=torch.int32, device=dev), loop_offsets[1:] - loop_offsets[:-1],
                                       output_size=loop_vertices.shape[0])
    vout = torch.empty((V + lay["n_new"], 3), dtype=torch.float32, device=dev)
    vout[:V] = vertices
    cout = None
    if colors is not None:
        cout = torch.empty((V + lay["n_new"], 3), dtype=torch.float32, device=dev)
        cout[:V] = colors
    clock("layout")
    if ops:
        S, SC, rows = ops.fill_rim(vertices, colors, loop_vertices, rim_loop, loop_offsets, centre, scale)
        clock("rim")
        fout = torch.empty((lay["n_new_faces"], 3), dtype=torch.int32, device=dev)
        ops.fill_emit(V, lay, loop_vertices, loop_offsets, rows, S, SC, centre, scale, vout, cout, fout)
        clock("emit")
    else:
        S, SC, rows = rim_torch(vertices, colors, loop_vertices, rim_loop, loop_offsets, centre, scale)
        clock("rim")
        vout[V:], new_c = vertices_torch(V, lay, loop_offsets, rows, S, SC, centre, scale)
        if cout is not None:
            cout[V:] = new_c
        fout = faces_torch(lay, loop_offsets, loop_vertices, rows, vout).to(torch.int32)
        clock("emit")
    return vout, cout, fout


@torch.no_grad()
def fill_holes(vertices, faces, colors=None, max_hole_edges=DEFAULT_MAX_HOLE_EDGES, clock=None):
    """Close the holes of a mesh -> (vertices [V',3] fp32, faces [F',3] in the dtype of `faces`, colors [V',3] or None) on the tensors'
    device.  The input's vertices, faces and colours come back as the leading rows with their bits unchanged; new vertices and
    faces follow, loop by loop in the order of boundary_loops.  A mesh without a loop to close is returned as it is.
      max_hole_edges  every simple boundary loop of 3 to max_hole_edges edges is closed.  THE OUTER RIM OF AN OPEN SHEET IS A HOLE
                      LIKE ANY OTHER: nothing but this cap separates it from a real hole, so choose it below the rim lengths
                      that are to stay open.  The default of 128 edges is a policy, not a measurement: a hole about 20 voxels
                      across in an extracted mesh.
    A loop of 3 gets one triangle -- unless its three vertices already form a face, in either winding (a lone triangle would
    become a two-face pillow).  A loop of n > 3 gets R = max(1, (113 n + 355) // 710) rings of new vertices between a smoothed copy
    of the rim and the mean of the rim, and the triangle strips between them (include/dgs_mesh_ops.h states every step;
    fill_counts(n) gives the counts).  New colours are built like the positions from the rim's colours clamped to [0, 1].  Loops
    through a bow-tie vertex, open chains and longer loops are left as they are.  Nothing keeps a fill from folding over where a
    rim is not star-shaped about its centre or is far from planar.
    ValueError: vertices or colors not fp32 [V,3], non-finite coordinates, a face index out of range, max_hole_edges not a
    non-negative integer, vertex or face totals that leave int32.  HIP tensors run the kernels of libdgs_mesh_ops.so -- a missing
    library is an error --, CPU tensors the PyTorch statement above: the results are bit-identical."""
    clock = clock or (lambda name: None)
    _check_mesh("fill_holes", vertices, faces, colors)
    if vertices.dtype != torch.float32 or (colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape)):
        raise ValueError("fill_holes: vertices and colors must be fp32 [V,3]")
    if isinstance(max_hole_edges, bool) or not isinstance(max_hole_edges, (int, np.integer)) or max_hole_edges < 0:
        raise ValueError("fill_holes: max_hole_edges must be a non-negative integer")
    V, F = vertices.shape[0], faces.shape[0]
    f = _faces_checked("fill_holes", V, faces)
    if V and not bool(torch.isfinite(vertices).all()):
        raise ValueError("fill_holes: non-finite vertex coordinates")
    if V == 0 or F == 0 or max_hole_edges < 3:
        return vertices, faces, colors
    lv, offsets, lf = _loops(V, _proper(f), int(max_hole_edges))
    clock("loops")
    L = offsets.shape[0] - 1
    if L:                                                     # the lone triangle: a loop of 3 whose rim edges all come from one face
        n = offsets[1:] - offsets[:-1]
        at = offsets[:-1]
        lone = (n == 3) & (lf[at] == lf[(at + 1).clamp(max=lf.shape[0] - 1)]) & (lf[at] == lf[(at + 2).clamp(max=lf.shape[0] - 1)])
        if bool(lone.any()):
            keep = ~torch.repeat_interleave(lone, n)
            lv, n = lv[keep], n[~lone]
            offsets = torch.zeros(n.shape[0] + 1, dtype=torch.int64, device=n.device)
            offsets[1:] = torch.cumsum(n, 0)
            L = n.shape[0]
    if L == 0:
        return vertices, faces, colors
    if F >= _ID_LIMIT - 1:
        raise ValueError("fill_holes: the faces do not fit int32 ids")
    vout, cout, fnew = fill_loops(vertices.contiguous(), None if colors is None else colors.contiguous(), lv.contiguous(), offsets, clock)
    if F + fnew.shape[0] >= _ID_LIMIT:
        raise ValueError("fill_holes: %d faces do not fit int32 ids" % (F + fnew.shape[0]))
    return vout, torch.cat((faces, fnew.to(faces.dtype))), cout


# ---- shell ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    import os
    from . import io as dio
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_fill",
                                 description="Close the holes of a triangle mesh: every simple boundary loop of up to --max-edges edges.")
    ap.add_argument("input", help=".ply or .obj")
    ap.add_argument("output", help=".ply")
    ap.add_argument("--max-edges", type=int, default=DEFAULT_MAX_HOLE_EDGES, help="longest loop to close; longer rims (an open sheet's) stay open")
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
    n_loops = boundary_loops(n_v, f)[1].shape[0] - 1
    v, f, c = fill_holes(v, f, c, max_hole_edges=a.max_edges)
    left = boundary_loops(v.shape[0], f)[1].shape[0] - 1
    dio.write_mesh_ply(a.output, v, f, c)
    print("%s: %d vertices, %d faces, %d loops -> %s: %d vertices, %d faces, %d loops%s" %
          (a.input, n_v, n_f, n_loops, a.output, v.shape[0], f.shape[0], left, ", watertight" if is_watertight(v.shape[0], f) else ""))


if __name__ == "__main__":
    main()
