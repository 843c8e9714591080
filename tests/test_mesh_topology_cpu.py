"""dgs_amd.mesh_topology on the CPU: undirected_edges against a brute-force dictionary on the smallest meshes that can go wrong, the
shared checks, and the four callers of undirected_edges against the integers they returned before they shared it."""
import pytest
import torch


def sheet(n, permute=True):
    """(vertex count, faces [2 (n - 1)^2, 3] int64) of an n x n grid cut into triangles; permute: vertex i is renamed 7 i + 3 mod n^2
    (n^2 prime to 7), so neighbouring faces no longer name neighbouring ids."""
    ids = torch.arange(n * n).reshape(n, n)
    a, b, c, d = ids[:-1, :-1], ids[:-1, 1:], ids[1:, :-1], ids[1:, 1:]
    f = torch.cat((torch.stack((a, b, c), -1).reshape(-1, 3), torch.stack((b, d, c), -1).reshape(-1, 3)))
    if permute:
        f = ((torch.arange(n * n) * 7 + 3) % (n * n))[f]
    return n * n, f


MESHES = {
    "empty": (0, torch.zeros((0, 3), dtype=torch.int64)),
    "triangle": (3, torch.tensor([[0, 1, 2]])),
    "tetrahedron": (4, torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])),
    # two triangles on one edge, a repeat of the first, and a face that names a vertex twice
    "pair_repeat_degenerate": (5, torch.tensor([[0, 1, 2], [2, 1, 3], [0, 1, 2], [3, 3, 4]])),
    "fan_of_three": (5, torch.tensor([[0, 1, 2], [0, 1, 3], [0, 1, 4]])),
    "sheet": sheet(6),
}
# (distinct edges, {count: edges with it}) of every mesh, by hand
SHAPE = {"empty": (0, {}), "triangle": (3, {1: 3}), "tetrahedron": (6, {2: 6}), "pair_repeat_degenerate": (7, {1: 3, 2: 3, 3: 1}),
         "fan_of_three": (7, {1: 6, 3: 1}), "sheet": (85, {1: 20, 2: 65})}


def check_edges(f, key, order, start, count):
    """The contract of undirected_edges for faces f (a CPU tensor) and its four outputs (CPU tensors)."""
    F = f.shape[0]
    want = {}                                                  # key -> its half-edges, ascending
    for g in range(F):
        for c in range(3):
            a, b = int(f[g, c]), int(f[g, (c + 1) % 3])
            want.setdefault((min(a, b) << 32) | max(a, b), []).append(3 * g + c)
    assert key.shape == order.shape == (3 * F,) and key.dtype == order.dtype == start.dtype == count.dtype == torch.int64
    assert key.tolist() == sorted(key.tolist())                                             # keys ascending
    assert sorted(order.tolist()) == list(range(3 * F))                                     # a permutation of the half-edges
    assert key[start].tolist() == sorted(want) and count.tolist() == [len(want[k]) for k in sorted(want)]
    assert int(count.sum()) == 3 * F
    for s, n, k in zip(start.tolist(), count.tolist(), sorted(want)):
        assert order[s:s + n].tolist() == want[k]                                           # every run in half-edge (face) order
    return want


@pytest.mark.parametrize("name", list(MESHES))
def test_undirected_edges(name):
    from dgs_amd.mesh_topology import half_edges, sorted_edge_keys, undirected_edges
    V, f = MESHES[name]
    key, order, start, count = undirected_edges(f)
    want = check_edges(f, key, order, start, count)
    n_edges, by_count = SHAPE[name]
    assert len(want) == n_edges and {n: count.tolist().count(n) for n in set(count.tolist())} == by_count
    a, b = half_edges(f)                                       # corner c -> corner c + 1, face-major
    assert a.tolist() == f.reshape(-1).tolist() and b.tolist() == f[:, [1, 2, 0]].reshape(-1).tolist()
    k2, o2 = sorted_edge_keys(a, b)                            # the sort alone: the same keys and order
    assert torch.equal(k2, key) and torch.equal(o2, order)
    if name == "pair_repeat_degenerate":                       # the face (3, 3, 4): the key of a vertex with itself, and 3 - 4 twice
        assert want[(3 << 32) | 3] == [9] and want[(3 << 32) | 4] == [10, 11]


def test_moved_checks():
    from dgs_amd import mesh_clean, mesh_decimate, mesh_fill, mesh_simplify, mesh_smooth, mesh_topology as mt
    v, f = torch.zeros((4, 3)), MESHES["tetrahedron"][1]
    mt._check_mesh("t", v, f), mt._check_mesh("t", v, f.int(), torch.zeros((4, 3)))
    for bad in ((v[:, :2], f), (v.long(), f), (v, f[:, :2]), (v, f.float()), (v, f.short())):
        with pytest.raises(ValueError, match="t: "):
            mt._check_mesh("t", *bad)
    with pytest.raises(ValueError, match="one colour per vertex"):
        mt._check_mesh("t", v, f, torch.zeros((3, 3)))
    assert mt._faces_checked("t", 4, f.int()).dtype == torch.int64 and mt._faces_checked("t", 0, f[:0]).shape == (0, 3)
    for n, bad in ((3, f), (4, f - 1), (-1, f[:0]), (2 ** 31, f), (4, f.float())):
        with pytest.raises(ValueError, match="t: "):
            mt._faces_checked("t", n, bad)
    g = MESHES["pair_repeat_degenerate"][1]
    assert mt._three_distinct(g).tolist() == [True, True, True, False] and mt._three_distinct(g[:0]).shape == (0,)
    assert mt._first_proper_faces(g).tolist() == [True, True, False, False]
    assert mt._first_proper_faces(torch.tensor([[0, 1, 2], [1, 2, 0], [2, 1, 0]])).tolist() == [True, False, True]   # a rotation; the other winding
    cv, cf, cc = mt._compact(torch.arange(15.0).reshape(5, 3), g, torch.arange(15.0).reshape(5, 3) / 15, torch.tensor([False, True, False, False]))
    assert cv[:, 0].tolist() == [3.0, 6.0, 9.0] and cf.tolist() == [[1, 0, 2]] and torch.equal(cc, cv / 15)
    # the names other modules, tests and tools import from where they were
    assert mesh_clean._compact is mt._compact and mesh_clean._check_mesh is mt._check_mesh and mesh_clean._first_proper_faces is mt._first_proper_faces
    assert mesh_smooth._faces_checked is mt._faces_checked and mesh_decimate._frame is mt._frame and mesh_decimate.normal_lengths is mt.normal_lengths
    assert mesh_decimate._kernels is mt._kernels and mesh_fill._kernels is mt._kernels and mesh_fill._frame is mt._frame
    assert mesh_simplify.LAMBDA_EXP == mesh_decimate.LAMBDA_EXP == mt.LAMBDA_EXP == -10
    assert mt._kernels(torch.device("cpu")) is None


def test_small_geometry():
    from dgs_amd import mesh_topology as mt
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((50, 3), generator=g, dtype=torch.float64), torch.randn((50, 3), generator=g, dtype=torch.float64)
    assert torch.allclose(mt._cross(a, b), torch.linalg.cross(a, b), rtol=1e-14, atol=1e-15)
    assert torch.allclose(mt._dot(a, b), (a * b).sum(1), rtol=1e-14, atol=1e-15)
    pos = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.0]])
    n, l = mt.normal_lengths(pos, torch.tensor([[0, 1, 2], [0, 3, 1]]))
    assert n.tolist() == [[0.0, 0.0, 12.0], [0.0, 0.0, 0.0]] and l.tolist() == [12.0, 0.0] and l.dtype == torch.float32
    assert all(torch.equal(x, y) for x, y in zip(mt.face_normals(pos[torch.tensor([[0, 1, 2], [0, 3, 1]])]), (n, l)))
    centre, scale = mt._frame(torch.tensor([[-1.0, 0.0, 2.0], [5.0, 1.0, 2.0]]))
    assert centre.tolist() == [2.0, 0.5, 2.0] and scale == 0.25                             # half extent 3 < 4 = 2^2
    assert mt._frame(torch.zeros((2, 3)))[1] == 1.0
    # the solve: A = w n n^T of the plane z = 0.25 plus the pull towards the anchor -> the anchor's foot on the plane, nearly
    A = [torch.tensor([x], dtype=torch.float64) for x in (0.0, 0.0, 0.0, 0.0, 0.0, 8.0)]
    rhs = [torch.tensor([x], dtype=torch.float64) for x in (0.0, 0.0, -2.0)]
    y, good = mt.quadric_solve(A, rhs, torch.tensor([[0.5, -0.5, 0.0]], dtype=torch.float64))
    assert bool(good) and abs(float(y[0, 0]) - 0.5) < 1e-12 and abs(float(y[0, 1]) + 0.5) < 1e-12 and abs(float(y[0, 2]) - 0.25) < 0.25 * 2.0 ** -9
    zero = [torch.zeros(1, dtype=torch.float64)] * 6
    assert not bool(mt.quadric_solve(zero, rhs, torch.zeros((1, 3), dtype=torch.float64))[1])   # no plane: trace 0


# What boundary_vertices (as indices), round_tables(...)["edges"] / ["flags"], boundary_half_edges and the edge-adjacency
# cluster_connected_triangles (clusters, triangles per cluster) returned on MESHES before they were built on undirected_edges;
# round_tables and boundary_half_edges are given the faces with three different vertices, as their callers give them.
BEFORE = {
    "empty": {"boundary_vertices": [], "clusters": [[], []], "half_edges": [[], [], []]},
    "triangle": {"boundary_vertices": [0, 1, 2], "clusters": [[0], [1]],
                 "edges": [[0, 0, 1], [1, 2, 2], [1, 1, 1], [2, 1, 0], [-1, -1, -1]], "flags": [3, 3, 3],
                 "half_edges": [[0, 1, 2], [1, 2, 0], [0, 0, 0]]},
    "tetrahedron": {"boundary_vertices": [], "clusters": [[0, 0, 0, 0], [4]],
                    "edges": [[0, 0, 0, 1, 1, 2], [1, 2, 3, 2, 3, 3], [2, 2, 2, 2, 2, 2], [2, 1, 1, 0, 0, 1], [3, 3, 2, 3, 2, 0]],
                    "flags": [0, 0, 0, 0], "half_edges": [[], [], []]},
    "pair_repeat_degenerate": {"boundary_vertices": [1, 2, 3], "clusters": [[0, 0, 0, 1], [3, 1]],
                               "edges": [[0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [2, 2, 3, 1, 1], [2, 1, 0, 2, 1], [2, 1, 3, -1, -1]],
                               "flags": [0, 3, 3, 3, 0], "half_edges": [[1, 3], [3, 2], [1, 1]]},
    "fan_of_three": {"boundary_vertices": [0, 1, 2, 3, 4], "clusters": [[0, 0, 0], [3]],
                     "edges": [[0, 0, 0, 0, 1, 1, 1], [1, 2, 3, 4, 2, 3, 4], [3, 1, 1, 1, 1, 1, 1], [2, 1, 1, 1, 0, 0, 0], [3, -1, -1, -1, -1, -1, -1]],
                     "flags": [3, 3, 3, 3, 3], "half_edges": [[1, 1, 1, 2, 3, 4], [2, 3, 4, 0, 0, 0], [0, 1, 2, 0, 1, 2]]},
    "sheet": {"boundary_vertices": [2, 3, 4, 8, 9, 10, 11, 14, 15, 17, 18, 20, 21, 24, 25, 26, 27, 31, 32, 33],
              "clusters": [[0] * 50, [50]],
              "edges": [[0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 8, 9, 9, 9, 10, 10, 11,
                         11, 12, 12, 12, 13, 13, 13, 14, 15, 15, 15, 16, 16, 16, 17, 17, 18, 18, 19, 19, 19, 20, 21, 21, 21, 22, 22, 22, 23,
                         23, 23, 24, 24, 25, 25, 26, 27, 27, 27, 28, 28, 28, 29, 29, 30, 33, 34],
                        [1, 6, 7, 29, 30, 35, 2, 7, 8, 30, 31, 8, 31, 9, 10, 5, 11, 33, 34, 6, 11, 12, 34, 35, 7, 12, 13, 35, 8, 13, 14, 14,
                         10, 15, 16, 16, 17, 12, 18, 13, 18, 19, 14, 19, 20, 20, 16, 21, 22, 17, 22, 23, 23, 24, 19, 25, 20, 25, 26, 26, 22,
                         27, 28, 23, 28, 29, 24, 29, 30, 30, 31, 26, 32, 32, 28, 33, 34, 29, 34, 35, 30, 35, 31, 34, 35],
                        [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 2, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 2, 1, 2, 2, 1, 2, 1,
                         2, 2, 2, 2, 2, 2, 1, 2, 1, 2, 2, 2, 2, 2, 1, 2, 1, 2, 2, 2, 1, 2, 1, 2, 2, 2, 2, 2, 2, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2,
                         2, 2, 2, 2, 2, 2, 2],
                        [30, 7, 6, 35, 1, 29, 31, 8, 7, 0, 2, 1, 1, 10, 9, 34, 5, 34, 5, 35, 12, 11, 4, 6, 0, 13, 12, 5, 1, 14, 13, 7, 3, 16,
                         15, 17, 16, 5, 12, 6, 19, 18, 7, 20, 19, 13, 9, 22, 21, 10, 23, 22, 24, 23, 12, 19, 13, 26, 25, 19, 15, 28, 27, 16,
                         29, 28, 17, 30, 29, 31, 30, 19, 26, 25, 21, 34, 33, 22, 35, 34, 23, 0, 24, 27, 28],
                        [7, 35, 1, 30, 29, 6, 8, 0, 2, 31, 30, -1, -1, -1, -1, 11, -1, -1, 33, 12, 4, 6, 35, 34, 13, 5, 7, 0, 14, 6, 8, -1, 16,
                         -1, 10, 9, -1, 18, -1, 19, 11, 13, 20, 12, 14, -1, 22, -1, 16, 23, 15, 17, 16, -1, 25, -1, 26, 18, 20, -1, 28, -1, 22,
                         29, 21, 23, 30, 22, 24, 23, -1, 32, -1, -1, 34, -1, 28, 35, 27, 29, 0, 28, 1, 4, 5]],
              "flags": [0, 0, 3, 3, 3, 0, 0, 0, 3, 3, 3, 3, 0, 0, 3, 3, 0, 3, 3, 0, 3, 3, 0, 0, 3, 3, 3, 3, 0, 0, 0, 3, 3, 3, 0, 0],
              "half_edges": [[2, 3, 4, 8, 9, 10, 11, 14, 15, 17, 18, 20, 21, 24, 25, 26, 27, 31, 32, 33],
                             [8, 10, 33, 14, 3, 17, 4, 20, 9, 24, 11, 26, 15, 31, 18, 32, 21, 2, 25, 27],
                             [29, 0, 45, 34, 0, 1, 46, 39, 5, 2, 47, 44, 10, 3, 48, 49, 15, 4, 49, 20]]},
}


@pytest.mark.parametrize("name", list(MESHES))
def test_callers_return_what_they_returned(name):
    from dgs_amd.mesh_clean import cluster_connected_triangles
    from dgs_amd.mesh_decimate import round_tables
    from dgs_amd.mesh_fill import boundary_half_edges
    from dgs_amd.mesh_smooth import boundary_vertices
    from dgs_amd.mesh_topology import _three_distinct
    V, f = MESHES[name]
    want = BEFORE[name]
    proper = f[_three_distinct(f)]
    assert torch.nonzero(boundary_vertices(V, f)).reshape(-1).tolist() == want["boundary_vertices"]
    if proper.shape[0]:                                        # (round_tables takes at least one face)
        tab = round_tables(V, proper)
        assert tab["edges"].dtype == torch.int32 and tab["edges"].tolist() == want["edges"]
        assert tab["flags"].dtype == torch.uint8 and tab["flags"].tolist() == want["flags"]
    assert [x.tolist() for x in boundary_half_edges(V, proper)] == want["half_edges"]
    cluster, triangles, _ = cluster_connected_triangles(torch.zeros((V, 3)), f, "edge")
    assert [cluster.tolist(), triangles.tolist()] == want["clusters"]
