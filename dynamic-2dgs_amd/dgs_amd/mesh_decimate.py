"""Mesh decimation on the tensors' own device: quadric edge collapse in parallel rounds, without open3d.

  decimate_mesh  <- open3d's TriangleMesh.simplify_quadric_decimation(target_number_of_triangles)

"This surface at N faces, still a manifold."  Every vertex carries the area-weighted plane quadric of its faces; collapsing an edge
merges its two vertices into one placed at the minimiser of the summed quadric, and costs the value of the quadric there.  Where a
serial decimator pops the cheapest edge off a heap, this one runs SYNCHRONOUS ROUNDS: every round rebuilds the edges of the current
faces, prices and validates all of them at once, selects an independent set of the cheapest ones (no two selected edges share an
endpoint or have adjacent endpoints) and collapses the whole set.  A collapse is only valid if it keeps the surface a manifold (link
condition), leaves no interior vertex with fewer than four neighbours and flips no face.

include/dgs_mesh_ops.h states every step.  The quadrics are int64 fixed-point sums, exact in any order; cost, placement and the flip
test are fp64, spelled out operation by operation; ties are broken by packed 64-bit keys.  So the HIP kernels (dgs_decimate_*) and
the PyTorch statement below give the same bits: HIP tensors run the kernels, CPU tensors the statement; the tables of a round (sorts,
run lengths, prefix sums) are PyTorch on the tensors' device either way.

WHAT IT IS NOT.  No attribute or texture seams (colours are interpolated along the collapsed edge and nothing else is carried), no
boundary-error quadrics (an open rim is either locked, the default, or free to shrink), and vertex and edge ids break cost ties, so
the result depends on the vertex numbering."""
import math

import numpy as np
import torch

from .mesh_topology import (LAMBDA_EXP, _check_mesh, _compact, _cross, _dot, _frame, _kernels, _three_distinct, half_edges, normal_lengths, quadric_solve,
                            sorted_edge_keys)

W_MAX = 16                             # largest face weight (in mean face areas); lambda = 2^LAMBDA_EXP
Q_MAX, Q_BUDGET = 40, 59               # fixed-point bits of the quadric sums: Q = min(Q_MAX, Q_BUDGET - ceil(log2(F)))
LEN_BITS = 28                          # fixed-point bits of the face-normal lengths behind the mean face area
MIN_VALENCE = 5                        # an interior vertex opposite a collapsed edge must have at least this many neighbours
FLAG_LOCKED, FLAG_BOUNDARY = 1, 2      # bits of the per-vertex flags of a round
NO_KEY = 2 ** 63 - 1                   # "no competing edge here": above every packed key (cost bits << 32 | edge id)
# Edges that compete in a round: the OVERSUBSCRIBE * (collapses still wanted) cheapest valid ones.  1 follows the serial order most
# closely and needs the most rounds; large values collapse locally cheapest edges that a serial decimator would not have reached
# yet.  Chosen from the quality-against-rounds table of tools/mesh_decimate_timing.py: the largest value
# whose rms distance to the analytic surface stays within 5 % of the best one on both meshes of the tool.
OVERSUBSCRIBE = 8.0


def quadric_bits(n_faces):
    """Q: the fixed-point bits of the quadric rows of a mesh of n_faces faces (include/dgs_mesh_ops.h derives the bound)."""
    return min(Q_MAX, Q_BUDGET - max(int(n_faces) - 1, 0).bit_length())


def default_max_rounds(n_faces, target):
    """The rounds after which decimate_mesh gives up.  A round takes at least the cheapest competing edge, so it always makes
    progress, and on a mesh without locks it takes a constant share of the collapses still wanted (a selected edge keeps at most the
    edges within two rings of it from being selected).  tools/mesh_decimate_timing.py counts fewer than 20 rounds per halving of
    the face count on its two meshes of 10^6 faces; 64 per halving is three times that, and 64 more cover the tail, where few
    edges are still valid."""
    n_faces, target = max(int(n_faces), 1), max(int(target), 1)
    return 64 + 64 * max(0, math.ceil(math.log2(max(n_faces / target, 1.0))))


# ---- the tables of a round (PyTorch on the tensors' device, integers only) ------------------------------------------------------
def round_tables(n_vertices, f, preserve_boundary=True):
    """Step (a) for faces f [F >= 1,3] int64 (three different vertices each) -> dict of
      edges [5,E] int32   rows u, v (u < v; ascending by (u, v)), the number of faces at the edge, the vertex opposite the edge in
                          the first and in the second of its faces, faces in ascending order (-1 where there is no second face)
      flags [V] uint8     FLAG_LOCKED | FLAG_BOUNDARY
      adj_offsets [V+1] int64, adj [2E] int32          the CSR vertex adjacency, rows ascending
      vf_offsets [V+1] int64, vf [3F] int32            the faces of every vertex, rows ascending
    and "dkey" [2E] int64, the sorted directed pairs i << 32 | j behind adj (the statement's membership test)."""
    V, F, dev = int(n_vertices), f.shape[0], f.device
    (i, j), opp = half_edges(f), f.roll(-2, 1).reshape(-1)  # half-edge 3 g + c: corners c, c + 1; opposite c + 2
    key, order = sorted_edge_keys(i, j)                      # equal keys stay in face order
    ekey, count = torch.unique_consecutive(key, return_counts=True)
    start = torch.cumsum(count, 0) - count
    opp_s = opp[order]
    opp0 = opp_s[start]
    opp1 = torch.where(count >= 2, opp_s[torch.clamp(start + 1, max=3 * F - 1)], torch.full_like(opp0, -1))
    u, v = ekey >> 32, ekey & 0xFFFFFFFF
    rim = torch.zeros(V, dtype=torch.bool, device=dev)
    once = count == 1
    rim[u[once]] = True
    rim[v[once]] = True
    lock = torch.zeros(V, dtype=torch.bool, device=dev)
    many = count > 2
    lock[u[many]] = True
    lock[v[many]] = True
    if preserve_boundary:
        lock |= rim
    flags = lock.to(torch.uint8) * FLAG_LOCKED + rim.to(torch.uint8) * FLAG_BOUNDARY
    dkey = torch.sort(torch.cat((ekey, (v << 32) | u))).values
    adj_offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    adj_offsets[1:] = torch.cumsum(torch.bincount(dkey >> 32, minlength=V), 0)
    vf_order = torch.sort(i, stable=True).indices           # face-major input: every row ascending by face
    vf_offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    vf_offsets[1:] = torch.cumsum(torch.bincount(i, minlength=V), 0)
    return {"edges": torch.stack((u, v, count, opp0, opp1)).to(torch.int32).contiguous(), "flags": flags, "adj_offsets": adj_offsets,
            "adj": (dkey & 0xFFFFFFFF).to(torch.int32), "dkey": dkey, "vf_offsets": vf_offsets, "vf": (vf_order // 3).to(torch.int32)}


# ---- the statement --------------------------------------------------------------------------------------------------------------
def mean_length(l):
    """The mean of the countable lengths as an fp32 Python number, from an integer sum (exact on every device): every term is
    rounded UP to a multiple of 2^-LEN_BITS, so the mean is not below the true one and the weights sum to at most F."""
    ok = (l > 0) & torch.isfinite(l)
    n = int(ok.sum())
    if n == 0:
        return 1.0
    total = int(torch.ceil(l[ok].double() * float(2 ** LEN_BITS)).long().sum())
    return float(np.float32(np.float64(total) / np.float64(n) * 2.0 ** -LEN_BITS)) if total > 0 else 1.0


def quadrics_torch(pos, f, mean_len, q_bits):
    """rows [V,10] int64 of step 1 (A: xx xy xz yy yz zz, b: x y z, c) from index_add_ (integers: exact in any order)."""
    V, dev = pos.shape[0], pos.device
    rows = torch.zeros((V, 10), dtype=torch.int64, device=dev)
    if f.shape[0] == 0:
        return rows
    n, l = normal_lengths(pos, f)
    ok = (l > 0) & torch.isfinite(l)
    f, n, l = f[ok], n[ok], l[ok]
    nh = n / l[:, None]
    w = torch.minimum(l / torch.full((1,), mean_len, dtype=torch.float32, device=dev), torch.full_like(l, float(W_MAX))).double()
    nd, p0 = nh.double(), pos[f[:, 0]].double()
    d = -_dot(nd, p0)
    wd = w * d
    terms = [(w * nd[:, a]) * nd[:, b] for a in range(3) for b in range(a, 3)] + [wd * nd[:, a] for a in range(3)] + [wd * d]
    val = torch.round(torch.stack(terms, -1) * float(2 ** q_bits)).long()
    for c in range(3):
        rows.index_add_(0, f[:, c], val)
    return rows


def _expand(offsets, ids, rows_of):
    """All (item, entry) pairs of the CSR rows rows_of [N]: (item index [M], entry [M])."""
    b, n = offsets[rows_of], offsets[rows_of + 1] - offsets[rows_of]
    item = torch.repeat_interleave(torch.arange(rows_of.shape[0], device=rows_of.device), n)
    at = torch.arange(item.shape[0], device=rows_of.device) - (torch.cumsum(n, 0) - n)[item] + b[item]
    return item, ids[at].long()


def edge_costs_torch(pos, rows, f, tab, q_bits, max_cost):
    """Steps 2b and 2c -> (cost [E] fp32, place [E,3] fp32, valid [E] bool).  cost and place are defined for every edge whose
    endpoints are not both locked (0 there); valid also asks for cost <= max_cost and the three conditions."""
    dev = pos.device
    e = tab["edges"].long()
    u, v, cnt, o0, o1 = e[0], e[1], e[2], e[3], e[4]
    E = u.shape[0]
    flags = tab["flags"]
    lu, lv = (flags[u] & FLAG_LOCKED) != 0, (flags[v] & FLAG_LOCKED) != 0
    pu, pv = pos[u].double(), pos[v].double()
    mid = (pu + pv) * 0.5
    r = (rows[u] + rows[v]).double()
    y, good = quadric_solve([r[:, k] for k in range(6)], [r[:, 6 + k] for k in range(3)], mid)
    dlt = pv - pu
    rad = (dlt[:, 0].abs() + dlt[:, 1].abs()) + dlt[:, 2].abs()
    good = good & ((y - mid).abs() <= rad[:, None]).all(1)
    x = torch.where(good[:, None], y, mid)
    x = torch.where(lu[:, None], pu, torch.where(lv[:, None], pv, x))
    place = x.float()
    x = place.double()
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = (r[:, k] for k in range(10))
    x0, x1, x2 = x[:, 0], x[:, 1], x[:, 2]
    q0, q1, q2 = (a00 * x0 + a01 * x1) + a02 * x2, (a01 * x0 + a11 * x1) + a12 * x2, (a02 * x0 + a12 * x1) + a22 * x2
    raw = (((x0 * q0 + x1 * q1) + x2 * q2) + 2.0 * ((b0 * x0 + b1 * x1) + b2 * x2)) + c
    cost = (torch.where(raw > 0, raw, torch.zeros_like(raw)) * 2.0 ** -q_bits).float()      # a NaN counts as 0 here and fails below
    both = lu & lv
    cand = ~both & ~torch.isnan(raw) & (cost <= max_cost)
    cost = torch.where(both, torch.zeros_like(cost), cost)
    place = torch.where(both[:, None], torch.zeros_like(place), place)
    # (c) on the candidates only
    ids = torch.nonzero(cand).reshape(-1)
    cu, cv, ccnt, co0, co1 = u[ids], v[ids], cnt[ids], o0[ids], o1[ids]
    deg = tab["adj_offsets"][1:] - tab["adj_offsets"][:-1]
    rimf = (flags & FLAG_BOUNDARY) != 0
    ok = (ccnt <= 2) & (co0 != co1) & ~((ccnt == 2) & rimf[cu] & rimf[cv])
    for o in (co0, co1):                                    # valence
        oc = o.clamp(min=0)
        ok &= (o < 0) | (deg[oc] >= torch.where(rimf[oc], 3, MIN_VALENCE))
    item, nb = _expand(tab["adj_offsets"], tab["adj"], cu)  # link: the common neighbours are the opposite vertices
    q = (cv[item] << 32) | nb
    dkey = tab["dkey"]
    at = torch.searchsorted(dkey, q).clamp(max=max(dkey.shape[0] - 1, 0))
    common = dkey[at] == q
    n_common = torch.zeros(ids.shape[0], dtype=torch.int64, device=dev).index_add_(0, item, common.long())
    stranger = common & (nb != co0[item]) & (nb != co1[item])
    n_bad = torch.zeros(ids.shape[0], dtype=torch.int64, device=dev).index_add_(0, item, stranger.long())
    ok &= (n_common == ccnt) & (n_bad == 0)
    xc = x[ids]
    for w in (cu, cv):                                      # flip: every surviving face at u, then at v
        item, g = _expand(tab["vf_offsets"], tab["vf"], w)
        fg = f[g]
        is_u, is_v = fg == cu[item, None], fg == cv[item, None]
        moved = is_u | is_v
        lives = ~(is_u.any(1) & is_v.any(1))
        p = pos[fg].double()                                # [M,3 corners,3]
        pn = torch.where(moved[:, :, None], xc[item, None, :], p)
        n0 = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        n1 = _cross(pn[:, 1] - pn[:, 0], pn[:, 2] - pn[:, 0])
        flip = lives & ~(_dot(n0, n1) > 0)
        ok &= torch.zeros(ids.shape[0], dtype=torch.int64, device=dev).index_add_(0, item, flip.long()) == 0
    valid = torch.zeros(E, dtype=torch.bool, device=dev)
    valid[ids] = ok
    return cost, place, valid


def edge_keys(cost):
    """key [E] int64 = cost bits << 32 | scramble(edge id): the packed word whose minimum decides a round.  scramble is a bijection
    of the 32-bit integers (two odd multiplications and two xor-shifts), so keys stay distinct and ties between equal costs are
    broken by a pseudo-random order instead of the edge order -- on a flat region, where every cost is 0, the edge order has one
    local minimum and a round would select one edge."""
    h = torch.arange(cost.shape[0], dtype=torch.int64, device=cost.device)
    h = (h * 0x9E3779B1) & 0xFFFFFFFF
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    return (cost.view(torch.int32).long() << 32) | h


def select_torch(n_vertices, edges, cost, compete):
    """Step 2e -> (m1 [V], m2 [V], selected [E] bool)."""
    dev = cost.device
    u, v = edges[0].long(), edges[1].long()
    key = edge_keys(cost)
    m1 = torch.full((n_vertices,), NO_KEY, dtype=torch.int64, device=dev)
    m1.scatter_reduce_(0, u[compete], key[compete], "amin")
    m1.scatter_reduce_(0, v[compete], key[compete], "amin")
    m2 = m1.clone()
    m2.scatter_reduce_(0, u, m1[v], "amin")
    m2.scatter_reduce_(0, v, m1[u], "amin")
    return m1, m2, compete & (m2[u] == key) & (m2[v] == key)


def apply_torch(pos, rows, colors, moved, f, tab, place, sel):
    """Step 2f, in place on pos, rows, colors, moved -> (vmap [V] int64, faces [F,3] int64 re-indexed, keep [F] bool)."""
    V, dev = pos.shape[0], pos.device
    e = tab["edges"].long()
    u, v = e[0][sel], e[1][sel]
    lu, lv = (tab["flags"][u] & FLAG_LOCKED) != 0, (tab["flags"][v] & FLAG_LOCKED) != 0
    s = torch.where(lv & ~lu, v, u)                         # the survivor: the smaller id, unless only the larger one is locked
    d = u + v - s
    x = place[sel]
    if colors is not None:
        pu, dl = pos[u].double(), pos[v].double() - pos[u].double()
        t = _dot(x.double() - pu, dl) / _dot(dl, dl)
        t = torch.where(t > 0, torch.where(t < 1, t, torch.ones_like(t)), torch.zeros_like(t)).float()
        cu, cv = colors[u], colors[v]
        colors[s] = cu + t[:, None] * (cv - cu)
    pos[s] = x
    moved[s] |= ~(lu | lv)
    rows[s] = rows[u] + rows[v]
    vmap = torch.arange(V, dtype=torch.int64, device=dev)
    vmap[d] = s
    g = vmap[f]
    keep = (g[:, 0] != g[:, 1]) & (g[:, 1] != g[:, 2]) & (g[:, 2] != g[:, 0])
    return vmap, g, keep


# ---- one round, on either device ------------------------------------------------------------------------------------------------
class _State:
    """What a run carries from round to round: pos [V,3] fp32 (the frame), rows [V,10] int64, colors [V,3] or None, moved [V] bool,
    faces [F,3] int64 (ids of the input), rep [V] int64 (the vertex every input vertex has been merged into)."""


def decimate_round(st, target, q_bits, max_cost, preserve_boundary, oversubscribe=None, clock=None):
    """One round on the state -> (collapses applied, dict of the round's tensors for the tests and the timing tool).  clock: called
    with the name of every phase as it ends (the timing tool's stopwatch)."""
    clock = clock or (lambda name: None)
    dev = st.pos.device
    ops = _kernels(dev)
    V, F = st.pos.shape[0], st.faces.shape[0]
    tab = round_tables(V, st.faces, preserve_boundary)
    edges = tab["edges"]
    E = edges.shape[1]
    f32 = st.faces.to(torch.int32) if ops else None
    clock("tables")
    if ops:
        cost, place, valid = ops.decimate_edges(st.pos, st.rows, f32, tab, q_bits, max_cost)
    else:
        cost, place, valid = edge_costs_torch(st.pos, st.rows, st.faces, tab, q_bits, max_cost)
    clock("edges")
    # (d) the throttle: the k-th smallest of the costs, +inf where an edge is not valid
    want = max(F - target, 0)
    k = min(E, max(1, math.ceil((want + 1) // 2 * (OVERSUBSCRIBE if oversubscribe is None else oversubscribe))))
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    kth = torch.sort(torch.where(valid, cost, inf)).values[k - 1]     # the value of torch.kthvalue(.., k); on a HIP device a radix sort is the faster way to it
    compete = valid & (cost <= kth)
    clock("throttle")
    if ops:
        m1, m2, selected = ops.decimate_select(V, edges, cost, compete)
    else:
        m1, m2, selected = select_torch(V, edges, cost, compete)
    clock("select")
    # the cheapest prefix by key whose collapses the budget still asks for (keys ascend with the cost)
    sel = torch.nonzero(selected).reshape(-1)
    order = torch.sort(edge_keys(cost)[sel]).indices
    sel = sel[order]
    gone = torch.cumsum(edges[2].long()[sel], 0)
    sel = sel[(gone - edges[2].long()[sel]) < want]
    n_sel = sel.shape[0]                                     # (nonzero and the mask have read the counts already)
    out = {"tab": tab, "cost": cost, "place": place, "valid": valid, "compete": compete, "m1": m1, "m2": m2, "selected": selected, "sel": sel}
    clock("prefix")
    if n_sel == 0:
        return 0, out
    if ops:
        vmap, g, keep = ops.decimate_apply(st.pos, st.rows, st.colors, st.moved, f32, tab, place, sel.to(torch.int32))
        vmap, g = vmap.long(), g.long()
    else:
        vmap, g, keep = apply_torch(st.pos, st.rows, st.colors, st.moved, st.faces, tab, place, sel)
    clock("apply")
    st.faces = g[keep]
    st.rep = vmap[st.rep]
    clock("compact")
    out.update(vmap=vmap, keep=keep)
    return n_sel, out


def prepare(vertices, faces, colors, preserve_boundary=True):
    """Step 0 and step 1 -> (state, q_bits, scale, centre); the faces that name a vertex twice are dropped here."""
    dev = vertices.device
    V = vertices.shape[0]
    f = faces.long()
    f = f[_three_distinct(f)]
    centre, scale = _frame(vertices)
    st = _State()
    st.pos = ((vertices - centre) * scale).contiguous()
    st.colors = None if colors is None else colors.contiguous().clone()
    st.moved = torch.zeros(V, dtype=torch.bool, device=dev)
    st.faces = f
    st.rep = torch.arange(V, dtype=torch.int64, device=dev)
    q_bits = quadric_bits(f.shape[0])
    mean_len = mean_length(normal_lengths(st.pos, f)[1]) if f.shape[0] else 1.0
    ops = _kernels(dev)
    if ops:
        st.rows = ops.decimate_quadrics(st.pos, f.to(torch.int32).contiguous(), mean_len, q_bits)
    else:
        st.rows = quadrics_torch(st.pos, f, mean_len, q_bits)
    return st, q_bits, scale, centre


# ---- the function ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def decimate_mesh(vertices, faces, colors=None, target_faces=None, ratio=None, max_error=None, preserve_boundary=True, max_rounds=None,
                  return_map=False):
    """open3d's simplify_quadric_decimation -> (vertices [V',3] fp32, faces [F',3] in the dtype of `faces`, colors [V',3] or None) on
    the tensors' device, and with return_map=True also [V] int64: the output vertex every input vertex was merged into, -1 for a
    vertex that no face with three different corners referred to.
      target_faces / ratio  exactly one: the face budget, or the share of the input's faces (0 < ratio <= 1; the budget is
                            floor(ratio * F))
      max_error             a distance in the units of the mesh: no edge whose quadric cost exceeds its square is collapsed
      preserve_boundary     lock the vertices of open edges (default); unset, the rim may shrink, but never flips or pinches
      max_rounds            default: default_max_rounds(F, budget)
    Surviving vertices appear in ascending input id, surviving faces keep their order and winding; a vertex that was never part of
    a collapse keeps its bits.  When the budget is reachable the output has `budget` or `budget - 1` faces; otherwise the function
    returns what it reached -- locks, the three validity conditions and max_error can all stop it early -- and raises nothing.
    A closed manifold stays a closed manifold of the same genus.  Faces that name a vertex twice are dropped; repeated faces lock
    their vertices (their edges have more than two faces).
    ValueError: both or neither of target_faces / ratio, a ratio outside (0, 1], a negative budget, max_error negative or NaN,
    vertices or colors not fp32, non-finite coordinates, a face index out of range.  HIP tensors run the kernels of
    libdgs_mesh_ops.so -- a missing library is an error --, CPU tensors the PyTorch statement above: the results are bit-identical.
    They depend on the vertex numbering (ids break cost ties)."""
    _check_mesh("decimate_mesh", vertices, faces, colors)
    if vertices.dtype != torch.float32 or (colors is not None and (colors.dtype != torch.float32 or colors.shape != vertices.shape)):
        raise ValueError("decimate_mesh: vertices and colors must be fp32 [V,3]")
    if (target_faces is None) == (ratio is None):
        raise ValueError("decimate_mesh: give exactly one of target_faces and ratio")
    V, F, dev = vertices.shape[0], faces.shape[0], vertices.device
    number = lambda x: not isinstance(x, bool) and isinstance(x, (int, float, np.floating, np.integer))
    if ratio is not None:
        if not number(ratio) or not (0.0 < float(ratio) <= 1.0):
            raise ValueError("decimate_mesh: ratio must be a number in (0, 1]")
        target = int(math.floor(float(ratio) * F))
    else:
        if isinstance(target_faces, bool) or not isinstance(target_faces, (int, np.integer)) or target_faces < 0:
            raise ValueError("decimate_mesh: target_faces must be a non-negative integer")
        target = int(target_faces)
    max_cost = float("inf")
    if max_error is not None:
        if not number(max_error) or not (float(max_error) >= 0.0):
            raise ValueError("decimate_mesh: max_error must be a non-negative number")
    if max_rounds is not None and (isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 0):
        raise ValueError("decimate_mesh: max_rounds must be a non-negative integer")
    f = faces.long()
    if F:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(f)).tolist())
        if lo < 0 or hi >= V:
            raise ValueError("decimate_mesh: face index out of range (ids in [%d, %d], %d vertices)" % (lo, hi, V))
    if V and not bool(torch.isfinite(vertices).all()):
        raise ValueError("decimate_mesh: non-finite vertex coordinates")
    if V == 0 or F == 0:
        out = _compact(vertices, faces, colors, torch.ones(F, dtype=torch.bool, device=dev))
        return out + (torch.full((V,), -1, dtype=torch.int64, device=dev),) if return_map else out
    st, q_bits, scale, centre = prepare(vertices.contiguous(), f, colors, preserve_boundary)
    if max_error is not None:
        with np.errstate(over="ignore"):
            e = np.float32(max_error) * np.float32(scale)
            max_cost = float(e * e)
    rounds = default_max_rounds(F, target) if max_rounds is None else int(max_rounds)
    for _ in range(rounds):
        if st.faces.shape[0] <= target or st.faces.shape[0] == 0:
            break
        if decimate_round(st, target, q_bits, max_cost, preserve_boundary)[0] == 0:
            break
    new_v = torch.where(st.moved[:, None], centre + st.pos * (1.0 / scale), vertices)
    used = torch.zeros(V, dtype=torch.bool, device=dev)
    used[st.faces.reshape(-1)] = True
    out = _compact(new_v, st.faces.to(faces.dtype), st.colors, torch.ones(st.faces.shape[0], dtype=torch.bool, device=dev))
    if not return_map:
        return out
    index = torch.cumsum(used, 0) - 1
    return out + (torch.where(used[st.rep], index[st.rep], torch.full((), -1, dtype=torch.int64, device=dev)),)


# ---- shell ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    import os
    from . import io as dio
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_decimate",
                                 description="Decimate a triangle mesh by quadric edge collapse (open3d's simplify_quadric_decimation).")
    ap.add_argument("input", help=".ply or .obj")
    ap.add_argument("output", help=".ply")
    budget = ap.add_mutually_exclusive_group(required=True)
    budget.add_argument("--ratio", type=float, default=None, help="share of the faces to keep, in (0, 1]")
    budget.add_argument("--faces", type=int, default=None, help="number of faces to keep")
    ap.add_argument("--max-error", type=float, default=None, help="collapse no edge that costs more than this distance, in the units of the mesh")
    ap.add_argument("--free-boundary", action="store_true", help="let open edges shrink (default: their vertices are locked)")
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
    v, f, c = decimate_mesh(v, f, c, target_faces=a.faces, ratio=a.ratio, max_error=a.max_error, preserve_boundary=not a.free_boundary)
    dio.write_mesh_ply(a.output, v, f, c)
    print("%s: %d vertices, %d faces -> %s: %d vertices, %d faces" % (a.input, n_v, n_f, a.output, v.shape[0], f.shape[0]))


if __name__ == "__main__":
    main()
