"""dgs_amd.mesh_clean on CPU tensors: the component labels against mesh.vertex_components and a plain union-find, the component
filter against mesh.keep_largest_components, the two adjacencies, clean_mesh step by step, and the refusals of dgs_cc_labels (no
device needed).  The mesh builders are shared with tests/test_mesh_clean_gpu.py."""
import functools

import numpy as np
import pytest
import torch


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def two_spheres_with_floater(N=48):
    """Two spheres through the CPU marching tetrahedra at N^3, plus a 24-face floater (a small closed surface: three octahedra that
    share no vertex with the spheres but touch each other in a vertex chain) appended.  -> (v f32, f int32, c f32) tensors."""
    from dgs_amd.mesh import TSDFVolume
    vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (N - 1), (N, N, N), "cpu")
    ax = [vol.origin[i] + vol.voxel_size * np.arange(N) for i in range(3)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    big = np.linalg.norm(G - np.array([0.3, 0.2, 0.1]), axis=-1) - 0.5
    small = np.linalg.norm(G - np.array([-0.62, -0.6, -0.55]), axis=-1) - 0.22
    vol.tsdf = torch.tensor(np.minimum(big, small), dtype=torch.float32)
    vol.weight = torch.ones_like(vol.tsdf)
    vol.color = torch.tensor(np.clip(G * 0.5 + 0.5, 0, 1), dtype=torch.float32)
    v, f, c = vol.extract()
    # an octahedron: 6 vertices, 8 faces; three of them chained through a shared apex = 16 vertices, 24 faces, one vertex component
    octa_v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32) * 0.02
    octa_f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    float_v, ff, prev0 = [], [], None
    for i in range(3):                      # vertex 1 of an octahedron (x = -0.02) IS vertex 0 of the one before it (x = +0.02)
        ids = np.empty(6, np.int64)
        for l in range(6):
            if l == 1 and prev0 is not None:
                ids[l] = prev0
            else:
                ids[l] = len(float_v)
                float_v.append(octa_v[l] + np.array([-0.9 + 0.04 * i, 0.9, 0.9], np.float32))
        prev0 = ids[0]
        ff.append(ids[octa_f])
    float_v = np.stack(float_v).astype(np.float32)
    assert float_v.shape == (16, 3)
    base = v.shape[0]
    v = torch.cat((v, torch.from_numpy(float_v)))
    c = torch.cat((c, torch.full((16, 3), 0.5)))
    f = torch.cat((f, torch.from_numpy(np.concatenate(ff) + base).to(f.dtype)))
    return v, f, c


def sheet(n, permute=False, seed=0):
    """An n x n grid of vertices, two triangles per cell: (vertices f32 [n*n,3], faces int32 [2 (n-1)^2,3]) as NumPy arrays; with
    `permute` the vertex ids are a fixed random permutation of the raster numbering (the hard case for label propagation)."""
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack((ii, jj, np.zeros_like(ii)), -1).reshape(-1, 3).astype(np.float32)
    a = (ii[:-1, :-1] * n + jj[:-1, :-1]).reshape(-1)
    f = np.concatenate((np.stack((a, a + 1, a + n), -1), np.stack((a + 1, a + n + 1, a + n), -1))).astype(np.int32)
    if permute:
        perm = np.random.default_rng(seed).permutation(n * n)
        vp = np.empty_like(v)
        vp[perm] = v
        v, f = vp, perm[f].astype(np.int32)
    return v, f


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def union_find(groups, n):
    """The plain statement: a Python union-find that hangs the larger root below the smaller one."""
    parent = list(range(n))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for g in groups:
        for b in g[1:]:
            ra, rb = root(int(g[0])), root(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([root(x) for x in range(n)], np.int64)


# ---- component_labels -----------------------------------------------------------------------------------------------------------
def test_component_labels_match_vertex_components():
    from dgs_amd.mesh import vertex_components
    from dgs_amd.mesh_clean import component_labels
    v, f, _ = two_spheres_with_floater()
    meshes = [(v.shape[0], f.numpy()), (60 * 60, sheet(60)[1]), (60 * 60, sheet(60, permute=True)[1]), (6, octahedron()[1])]
    for n, faces in meshes:
        got = component_labels(torch.from_numpy(faces), n)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), vertex_components(n, faces))
    assert np.unique(component_labels(f, v.shape[0]).numpy()[f.numpy().reshape(-1)]).size == 3


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_component_labels_general_k_against_union_find(k):
    from dgs_amd.mesh_clean import component_labels
    rng = np.random.default_rng(k)
    n = 700
    groups = rng.integers(0, n, size=(260, k))
    groups[::7] = groups[::7][:, :1]                   # groups that name one node k times
    groups = np.concatenate((groups, groups[:40]))     # repeated groups
    got = component_labels(torch.from_numpy(groups), n).numpy()
    assert np.array_equal(got, union_find(groups, n))
    assert (got <= np.arange(n)).all()


def test_component_labels_edge_cases():
    from dgs_amd.mesh_clean import component_labels
    assert component_labels(torch.zeros((0, 3), dtype=torch.int32), 5).tolist() == [0, 1, 2, 3, 4]
    assert component_labels(torch.zeros((0, 2), dtype=torch.int64), 0).shape == (0,)
    assert component_labels(torch.tensor([[3, 1], [4, 3]]), 6).tolist() == [0, 1, 2, 1, 1, 5]
    for bad in ([[0, 6]], [[-1, 2]]):
        with pytest.raises(ValueError):
            component_labels(torch.tensor(bad), 6)
    with pytest.raises(ValueError):
        component_labels(torch.tensor([[0.0, 1.0]]), 6)


# ---- filter_components ----------------------------------------------------------------------------------------------------------
def same_mesh(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            x, y = x.cpu(), y.cpu()
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)


FILTER_CASES = [(1, 50), (2, 50), (1000, 50), (1000, 24), (1000, 25), (1000, 0), (3, 0)]


@pytest.mark.parametrize("n_keep,min_faces", FILTER_CASES)
def test_filter_components_equals_keep_largest_components(n_keep, min_faces):
    """The floater has 24 faces: min_faces 24 keeps it, 25 drops it."""
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import cluster_connected_triangles, filter_components
    v, f, c = two_spheres_with_floater()
    want = keep_largest_components(v, f, c, n_keep=n_keep, min_faces=min_faces)
    same_mesh(filter_components(v, f, c, n_keep=n_keep, min_faces=min_faces), want)
    same_mesh(filter_components(v, f, None, n_keep=n_keep, min_faces=min_faces), keep_largest_components(v, f, None, n_keep=n_keep, min_faces=min_faces))
    n_faces = {(1, 50): 1, (2, 50): 2, (1000, 50): 2, (1000, 24): 3, (1000, 25): 2, (1000, 0): 3, (3, 0): 3}[(n_keep, min_faces)]
    sizes = sorted(cluster_connected_triangles(v, f)[1].tolist())
    assert sizes[0] == 24 and want[1].shape[0] == sum(sizes[-n_faces:] if n_faces < 3 else sizes)


def test_filter_components_on_an_empty_mesh():
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import filter_components
    v, f = torch.rand(5, 3), torch.zeros((0, 3), dtype=torch.int32)
    same_mesh(filter_components(v, f, None), keep_largest_components(v, f, None))


# ---- adjacency, statistics ------------------------------------------------------------------------------------------------------
def two_tetrahedra_touching_in_a_vertex():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], np.float32)
    t1 = [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]
    t2 = [[0, 4, 5], [0, 6, 4], [0, 5, 6], [4, 6, 5]]
    return torch.from_numpy(v), torch.tensor(t1 + t2, dtype=torch.int32)


def test_two_tetrahedra_touching_in_one_vertex():
    from dgs_amd.mesh_clean import cluster_connected_triangles, filter_components
    v, f = two_tetrahedra_touching_in_a_vertex()
    cl, n, area = cluster_connected_triangles(v, f, "vertex")
    assert cl.tolist() == [0] * 8 and n.tolist() == [8] and area.dtype == torch.float64
    cl, n, area = cluster_connected_triangles(v, f, "edge")
    assert cl.tolist() == [0] * 4 + [1] * 4 and n.tolist() == [4, 4]
    one = 3 * 0.5 + 0.5 * np.sqrt(3.0)
    assert np.allclose(area.numpy(), [one, one], rtol=1e-15)
    # the order of the clusters follows their smallest face, not a vertex id
    cl, n, _ = cluster_connected_triangles(v, f.flip(0), "edge")
    assert cl.tolist() == [0] * 4 + [1] * 4
    assert filter_components(v, f, None, n_keep=1, min_faces=0, adjacency="edge")[1].shape[0] == 8      # equal sizes: both stay
    assert filter_components(v, f[:7], None, n_keep=1, min_faces=0, adjacency="edge")[1].shape[0] == 4
    assert filter_components(v, f[:7], None, n_keep=1, min_faces=0, adjacency="vertex")[1].shape[0] == 7
    with pytest.raises(ValueError):
        cluster_connected_triangles(v, f, "corner")


def test_three_faces_on_one_edge_are_one_cluster():
    from dgs_amd.mesh_clean import cluster_connected_triangles
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [5, 6, 7], [1, 0, 3], [0, 1, 4]], dtype=torch.int64)
    cl, n, area = cluster_connected_triangles(v, f, "edge")
    assert cl.tolist() == [0, 1, 0, 0] and n.tolist() == [3, 1] and np.allclose(area.numpy(), [1.5, 0.5], rtol=1e-15)


def test_cluster_statistics_on_the_two_spheres():
    from dgs_amd.mesh_clean import cluster_connected_triangles, face_areas
    v, f, _ = two_spheres_with_floater()
    for adjacency, n_clusters in (("vertex", 3), ("edge", 5)):      # the floater's octahedra share vertices, not edges
        cl, n, area = cluster_connected_triangles(v, f, adjacency)
        assert n.shape == (n_clusters,) and int(n.sum()) == f.shape[0] and np.array_equal(np.bincount(cl.numpy()), n.numpy())
        first = [int(np.flatnonzero(cl.numpy() == i)[0]) for i in range(n_clusters)]
        assert first == sorted(first)
        fa = face_areas(v, f).numpy()
        assert np.allclose(area.numpy(), [fa[cl.numpy() == i].sum() for i in range(n_clusters)], rtol=1e-12)
    big = area.numpy()[np.argmax(n.numpy())]
    assert abs(big - 4 * np.pi * 0.25) < 0.02 * np.pi


# ---- clean_mesh -----------------------------------------------------------------------------------------------------------------
def unwelded(v, f):
    """Every face with its own three vertices, in face order."""
    return v[f.reshape(-1).long()].clone(), torch.arange(3 * f.shape[0], dtype=f.dtype).reshape(-1, 3)


def test_clean_mesh_welds_an_unwelded_closed_mesh():
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import clean_mesh, cluster_connected_triangles
    v, f, c = two_spheres_with_floater()
    v, f, c = keep_largest_components(v, f, c, n_keep=1)
    uv, uf = unwelded(v, f)
    assert cluster_connected_triangles(uv, uf, "vertex")[1].shape[0] == f.shape[0]      # falls apart into one component per face
    wv, wf, wc = clean_mesh(uv, uf, c[f.reshape(-1).long()])
    assert wv.shape == v.shape and wf.shape == f.shape and wf.dtype == f.dtype
    assert torch.equal(wv[wf.long()], v[f.long()])                                        # the same triangles, in the same order
    assert torch.equal(wc[wf.long()], c[f.long()])
    assert cluster_connected_triangles(wv, wf, "edge")[1].tolist() == [f.shape[0]]
    # survivors stay in their original order: the order of first appearance in the face list
    first = np.unique(f.numpy().reshape(-1), return_index=True)[1]
    assert torch.equal(wv, v[f.reshape(-1).long()[np.sort(first)]])
    # an indexed mesh that is already clean comes back as it is, and the function is idempotent
    same_mesh(clean_mesh(v, f, c), (v, f, c))
    same_mesh(clean_mesh(wv, wf, wc), (wv, wf, wc))


def test_clean_mesh_steps():
    from dgs_amd.mesh_clean import clean_mesh
    ov, of = octahedron()
    v = torch.from_numpy(np.concatenate((ov, [[9, 9, 9]], ov[:1], [[-0.0, 1, 0]]))).float()      # 6: unreferenced, 7: copy of 0, 8: copy of 2 with -0.0
    c = torch.arange(9, dtype=torch.float32)[:, None].expand(-1, 3).contiguous() / 10
    f = torch.cat((torch.from_numpy(of), torch.tensor([[2, 4, 0],        # face 0 rotated: dropped
                                                       [4, 2, 0],        # face 0 reversed: kept
                                                       [1, 1, 3],        # degenerate: dropped
                                                       [7, 5, 0],        # degenerate after welding 7 -> 0: dropped
                                                       [8, 7, 5]],       # = (2, 0, 5) after welding = face 4: dropped
                                                      dtype=torch.int32)))
    wv, wf, wc = clean_mesh(v, f, c)
    assert torch.equal(wv, torch.from_numpy(ov)) and torch.equal(wc, c[:6])                 # colours follow the first occurrence
    assert torch.equal(wf, torch.cat((torch.from_numpy(of), torch.tensor([[4, 2, 0]], dtype=torch.int32))))
    same_mesh(clean_mesh(wv, wf, wc), (wv, wf, wc))
    assert clean_mesh(v, f)[2] is None
    # (d): a lone triangle next to the octahedron
    v2 = torch.cat((wv, torch.tensor([[5.0, 5, 5], [6, 5, 5], [5, 6, 5]])))
    f2 = torch.cat((torch.tensor([[6, 7, 8]], dtype=torch.int32), wf[:8]))
    assert clean_mesh(v2, f2, min_triangles_connected=-1)[1].shape[0] == 9
    kv, kf, _ = clean_mesh(v2, f2, min_triangles_connected=2)
    assert torch.equal(kv, wv) and torch.equal(kf, wf[:8])
    assert clean_mesh(v2, f2, min_triangles_connected=9)[1].shape[0] == 0 and clean_mesh(v2, f2, min_triangles_connected=9)[0].shape[0] == 0
    with pytest.raises(ValueError):
        clean_mesh(v2, torch.tensor([[0, 1, 99]], dtype=torch.int32))


def test_clean_mesh_shell(tmp_path):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    from dgs_amd.mesh_clean import main
    ov, of = octahedron()
    uv, uf = unwelded(torch.from_numpy(ov), torch.from_numpy(of))
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    write_mesh_ply(src, torch.cat((uv, torch.tensor([[5.0, 5, 5], [6, 5, 5], [5, 6, 5]]))), torch.cat((uf, torch.tensor([[24, 25, 26]], dtype=torch.int32))))
    main([src, dst, "--device", "cpu"])
    v, f, _ = read_mesh_ply(dst)
    assert v.shape == (9, 3) and f.shape == (9, 3)
    main([src, dst, "--device", "cpu", "--min-triangles", "2"])
    v, f, _ = read_mesh_ply(dst)
    assert np.array_equal(np.unique(v, axis=0), np.unique(ov, axis=0)) and f.shape == (8, 3) and np.array_equal(v[f], ov[of])
    main([src, dst, "--device", "cpu", "--keep", "1", "--adjacency", "vertex"])
    assert read_mesh_ply(dst)[1].shape == (8, 3)
    with open(str(tmp_path / "in.obj"), "w") as fh:
        fh.write("".join("v %g %g %g\n" % tuple(p) for p in uv.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in uf.tolist()))
    main([str(tmp_path / "in.obj"), dst, "--device", "cpu"])
    assert read_mesh_ply(dst)[0].shape == (6, 3)


def test_evaluate_meshes_cleans_the_ground_truth_on_request(tmp_path):
    """An unwelded ground-truth OBJ with a duplicated and a degenerate face: clean_gt=True welds it on load; the default does not
    touch it and writes the settings it always wrote."""
    import json
    from dgs_amd import mesh_clean, mesh_metrics
    from dgs_amd.io import write_mesh_ply
    ov, of = octahedron()
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    pred.mkdir(), gt.mkdir()
    write_mesh_ply(str(pred / "frame_0.ply"), ov, of)
    uv, uf = unwelded(torch.from_numpy(ov), torch.from_numpy(of))
    uf = torch.cat((uf, uf[:1].roll(1, 1), uf[:1, [0, 0, 1]]))
    with open(str(gt / "m0.obj"), "w") as fh:
        fh.write("".join("v %g %g %g\n" % tuple(p) for p in uv.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in uf.tolist()))
    seen = []
    real = mesh_clean.clean_mesh
    mesh_clean.clean_mesh = lambda *a, **k: seen.append(real(*a, **k)) or seen[-1]
    try:
        plain = mesh_metrics.evaluate_meshes(str(pred), str(gt), n_samples=2000, seed=1, device="cpu")
        assert not seen and "clean_gt" not in plain["settings"]
        clean = mesh_metrics.evaluate_meshes(str(pred), str(gt), n_samples=2000, seed=1, device="cpu", clean_gt=True)
        assert len(seen) == 1 and seen[0][0].shape == (6, 3) and seen[0][1].shape == (8, 3)
        assert clean["settings"]["clean_gt"] is True and json.load(open(str(pred / "mesh_metrics.json")))["settings"]["clean_gt"] is True
        assert np.isfinite(clean["mean"]["chamfer"]) and clean["mean"]["chamfer"] < 0.1
        mesh_metrics.main([str(pred), str(gt), "--samples", "500", "--device", "cpu", "--clean-gt"])
        assert len(seen) == 2
    finally:
        mesh_clean.clean_mesh = real


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_cc_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    import ctypes
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    buf = (ctypes.c_int * 16)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    assert lib.dgs_cc_labels(4, ptr, 2, 4, ptr, None) < 0 and b"k must be 2 or 3" in err()
    assert lib.dgs_cc_labels(4, ptr, 2, 1, ptr, None) < 0 and b"k must be 2 or 3" in err()
    assert lib.dgs_cc_labels(-1, ptr, 2, 3, ptr, None) < 0 and b"negative" in err()
    assert lib.dgs_cc_labels(4, ptr, -2, 3, ptr, None) < 0 and b"negative" in err()
    assert lib.dgs_cc_labels(2 ** 31, ptr, 2, 3, ptr, None) < 0 and b"2^31" in err()
    assert lib.dgs_cc_labels(4, None, 2, 3, ptr, None) < 0 and b"null" in err()
    assert lib.dgs_cc_labels(4, ptr, 2, 3, None, None) < 0 and b"null" in err()
    assert lib.dgs_cc_labels(0, None, 0, 3, None, None) == 0                    # nothing to do: nothing is launched
    assert lib.dgs_cc_labels(0, ptr, 2, 2, None, None) == 0
    assert lib.dgs_cc_layout(None) < 0 and b"null" in err()
    threads, per_thread = _mesh_ops.cc_layout()
    assert threads % 64 == 0 and per_thread >= 1
    assert {"dgs_cc_labels", "dgs_cc_layout"} <= set(_mesh_ops.exported_symbols())
