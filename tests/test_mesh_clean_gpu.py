"""-m gpu: dgs_cc_labels against the CPU statements -- every comparison exact integer equality -- and the functions of
dgs_amd.mesh_clean on a HIP device against their CPU runs and against mesh.keep_largest_components."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_mesh_clean_cpu import FILTER_CASES, octahedron, same_mesh, sheet, two_spheres_with_floater, union_find, unwelded
from test_mesh_cpu import fusion_inputs, sphere_box

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hip_labels(groups, n):
    from dgs_amd import _mesh_ops
    g = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(DEV)
    label = _mesh_ops.cc_labels(g, n)
    assert label.dtype == torch.int32 and label.shape == (n,) and label.device == g.device
    return label.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def device_mesh():
    """A mesh extracted on the device: the sphere and the plate of tests/test_mesh_cpu.py fused at 96^3 from 24 views of 200^2 (the
    sizes of tests/test_mesh_gpu.py, at which the plate is a component of its own)."""
    from dgs_amd.mesh import TSDFVolume
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = (x.to(DEV) for x in fusion_inputs(24, 200, plate=True))
    v, f, c = TSDFVolume(origin, h, (N,) * 3, DEV).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0).extract()
    assert v.is_cuda and f.shape[0] > 10000
    return v, f, c


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numbering", ["ascending", "descending", "permuted"])
def test_chains(numbering):
    """A path graph of 4097 nodes: deep trees, 17 workgroups of groups, a ragged tail of one node."""
    n = 4097
    ids = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "permuted": np.random.default_rng(7).permutation(n)}[numbering]
    groups = np.stack((ids[:-1], ids[1:]), -1)
    assert np.array_equal(hip_labels(groups, n), np.zeros(n, np.int64))
    # the same path cut in the middle: two components, each labelled by its smallest id
    cut = np.delete(groups, n // 2, axis=0)
    assert np.array_equal(hip_labels(cut, n), union_find(cut, n))


def test_small_and_degenerate_inputs():
    from dgs_amd import _mesh_ops
    assert np.array_equal(hip_labels(np.zeros((0, 3)), 10000), np.arange(10000))          # n_groups == 0: only the init runs
    assert np.array_equal(hip_labels(np.zeros((0, 2)), 10000), np.arange(10000))
    assert hip_labels(np.zeros((0, 3)), 0).shape == (0,)                                   # n_nodes == 0: nothing is launched
    rep = np.array([[5, 2, 5], [2, 5, 5], [5, 2, 5], [7, 7, 7], [9, 9, 8], [5, 2, 5]])     # repeats, a node named twice / three times
    assert np.array_equal(hip_labels(rep, 12), union_find(rep, 12))
    assert hip_labels(rep, 12).tolist() == [0, 1, 2, 3, 4, 2, 6, 7, 8, 8, 10, 11]
    pairs = np.random.default_rng(3).permutation(10000).reshape(5000, 2)                   # 5000 two-node components
    want = union_find(pairs, 10000)
    assert np.array_equal(hip_labels(pairs, 10000), want) and np.unique(want).size == 5000
    # the wrapper refuses what the contract excludes
    g = torch.tensor([[0, 1, 12]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        _mesh_ops.cc_labels(g, 12)
    with pytest.raises(ValueError):
        _mesh_ops.cc_labels(torch.tensor([[0, -1]], dtype=torch.int32, device=DEV), 12)
    with pytest.raises(RuntimeError):
        _mesh_ops.cc_labels(g.long(), 13)
    with pytest.raises(RuntimeError):
        _mesh_ops.cc_labels(torch.zeros((2, 4), dtype=torch.int32, device=DEV), 13)


def test_ids_outside_the_range_are_skipped_by_the_kernel():
    """The C call itself (the wrapper refuses such input): an id outside [0, n_nodes) is skipped, the rest of its group counts."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    n = 10
    groups = torch.tensor([[n, 3, 4], [6, -1, 7], [8, 2 ** 31 - 1, -2 ** 31], [n + 1, n, -5], [1, 9, n]], dtype=torch.int32, device=DEV)
    guard = torch.full((n + 64,), -7, dtype=torch.int32, device=DEV)
    label = guard[32:32 + n]
    rc = lib.dgs_cc_labels(n, groups.data_ptr(), groups.shape[0], 3, label.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert label.tolist() == [0, 1, 2, 3, 3, 5, 6, 6, 8, 1]
    assert bool((guard[:32] == -7).all()) and bool((guard[32 + n:] == -7).all())


def test_random_graph_is_reproducible_and_order_independent():
    rng = np.random.default_rng(11)
    n = 20000
    groups = rng.integers(0, n, size=(30000, 3))
    first = hip_labels(groups, n)
    assert np.array_equal(first, hip_labels(groups, n))
    assert np.array_equal(first, hip_labels(groups[::-1], n))
    assert np.array_equal(first, hip_labels(groups[:, ::-1], n))
    assert np.array_equal(first, union_find(groups, n))
    assert 1 < np.unique(first).size < n


@pytest.mark.parametrize("k", [2, 3])
def test_layout_boundaries(k):
    """Group counts of one less than, exactly and one more than what one workgroup handles."""
    from dgs_amd import _mesh_ops
    threads, per_thread = _mesh_ops.cc_layout()
    per_group = threads * per_thread
    rng = np.random.default_rng(k)
    for G in (per_group - 1, per_group, per_group + 1, 2 * per_group, 2 * per_group + 1):
        n = 2 * G + 3
        groups = rng.integers(0, n - k, size=(G, k))
        groups[-1] = n - 1 - np.arange(k)                       # the last group of the last workgroup must count
        want = union_find(groups, n)
        assert want[n - 1] == n - k
        assert np.array_equal(hip_labels(groups, n), want), G


def test_sheet_with_permuted_vertex_ids():
    """300 x 300 vertices, 178 802 faces, vertex ids permuted: the hard case for propagation (NumPy: about 2 s)."""
    from dgs_amd.mesh import vertex_components
    from dgs_amd.mesh_clean import component_labels
    _, f = sheet(300, permute=True)
    assert f.shape == (178802, 3)
    # a second, small sheet that does not touch the first, so that the answer is not a constant
    faces = np.concatenate((f, sheet(10)[1] + 90000)).astype(np.int32)
    got = hip_labels(faces, 90100)
    assert np.array_equal(got, vertex_components(90100, faces))
    assert np.array_equal(np.unique(got), [0, 90000])
    assert np.array_equal(component_labels(torch.from_numpy(faces).to(DEV), 90100).cpu().numpy(), got)


# ---- mesh_clean on the device ---------------------------------------------------------------------------------------------------
def test_component_labels_other_k_and_dtypes():
    from dgs_amd.mesh_clean import component_labels
    rng = np.random.default_rng(5)
    for k in (1, 2, 3, 4, 5):
        groups = rng.integers(0, 900, size=(300, k))
        got = component_labels(torch.from_numpy(groups).to(DEV), 900)
        assert got.dtype == torch.int64 and got.is_cuda and np.array_equal(got.cpu().numpy(), union_find(groups, 900))
    with pytest.raises(ValueError):
        component_labels(torch.tensor([[0, 2 ** 32 + 1]], device=DEV), 900)               # must not wrap into the range


@pytest.mark.parametrize("n_keep,min_faces", FILTER_CASES)
def test_filter_components_on_the_two_spheres(n_keep, min_faces):
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import filter_components
    v, f, c = two_spheres_with_floater()
    got = filter_components(v.to(DEV), f.to(DEV), c.to(DEV), n_keep=n_keep, min_faces=min_faces)
    assert all(x.is_cuda for x in got)
    same_mesh(got, keep_largest_components(v, f, c, n_keep=n_keep, min_faces=min_faces))


def test_filter_components_on_a_mesh_extracted_on_the_device(device_mesh):
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import filter_components
    v, f, c = device_mesh
    kept = []
    for n_keep, min_faces in ((1, 50), (2, 0), (1000, 50), (1000, 0)):
        got = filter_components(v, f, c, n_keep=n_keep, min_faces=min_faces)
        assert all(x.is_cuda for x in got)
        same_mesh(got, keep_largest_components(v, f, c, n_keep=n_keep, min_faces=min_faces))
        kept.append(got[1].shape[0])
    print("faces kept of %d: %s" % (f.shape[0], kept))
    assert kept[0] < kept[-1] == f.shape[0]                  # the sphere and the plate are separate components
    same_mesh(filter_components(v, f, None, n_keep=1), keep_largest_components(v, f, None, n_keep=1))
    empty = f[:0]
    same_mesh(filter_components(v, empty, c), keep_largest_components(v, empty, c))


@pytest.mark.parametrize("adjacency", ["vertex", "edge"])
def test_cluster_connected_triangles_on_the_device(device_mesh, adjacency):
    """Counts and labels exact; the areas are float64 sums whose order differs: 1e-12 relative (at most 10^6 terms of similar size
    at 1.1e-16 each would allow 1e-10 in the worst case and ~1e-13 in the random-walk case)."""
    from dgs_amd.mesh_clean import cluster_connected_triangles
    worst = 0.0
    for v, f in (two_spheres_with_floater()[:2], tuple(x.cpu() for x in device_mesh[:2])):
        cl0, n0, a0 = cluster_connected_triangles(v, f, adjacency)
        cl1, n1, a1 = cluster_connected_triangles(v.to(DEV), f.to(DEV), adjacency)
        assert cl1.is_cuda and cl1.dtype == torch.int64 and a1.dtype == torch.float64
        assert torch.equal(cl1.cpu(), cl0) and torch.equal(n1.cpu(), n0)
        rel = float(((a1.cpu() - a0).abs() / a0).max())
        worst = max(worst, rel)
        print("%s adjacency: %d clusters, largest relative area deviation %.3e" % (adjacency, n0.shape[0], rel))
    assert worst <= 1e-12


def test_clean_mesh_on_the_device(device_mesh):
    from dgs_amd.mesh_clean import clean_mesh, cluster_connected_triangles
    v, f, c = (x.cpu() for x in device_mesh)
    uv, uf = unwelded(v, f)
    uc = c[f.reshape(-1).long()]
    uf = torch.cat((uf, uf[:100].roll(1, 1), uf[:50].flip(1), uf[:10, [0, 0, 1]]))          # rotated copies go, reversed ones stay, degenerate go
    for mt in (-1, 30):
        want = clean_mesh(uv, uf, uc, min_triangles_connected=mt)
        got = clean_mesh(uv.to(DEV), uf.to(DEV), uc.to(DEV), min_triangles_connected=mt)
        assert all(x.is_cuda for x in got)
        same_mesh(got, want)
    wv, wf, _ = clean_mesh(uv.to(DEV), uf[:f.shape[0]].to(DEV))
    same_mesh((wv, wf), clean_mesh(uv, uf[:f.shape[0]])[:2])
    assert wv.shape[0] <= torch.unique(f.reshape(-1)).numel() < uv.shape[0] and wf.shape[0] <= f.shape[0]
    assert cluster_connected_triangles(wv, wf, "edge")[1].cpu().tolist() == cluster_connected_triangles(wv.cpu(), wf.cpu(), "edge")[1].tolist()
    ov, of = octahedron()
    same_mesh(clean_mesh(torch.from_numpy(ov).to(DEV), torch.from_numpy(of).to(DEV)), (torch.from_numpy(ov), torch.from_numpy(of), None))


# ---- the product ----------------------------------------------------------------------------------------------------------------
def test_extract_meshes_filters_on_the_device_and_writes_the_same_files(tmp_path, monkeypatch):
    """The scene and sizes of tests/test_mesh_gpu.py::test_extract_meshes_on_a_short_fit.  extract_meshes filters the device mesh
    with filter_components; a second run whose filter is forced to keep_largest_components -- called on the very same extracted
    tensors, and compared with filter_components there -- writes byte-identical files."""
    from dgs_amd import mesh_clean
    from dgs_amd.fit import fit
    from dgs_amd.mesh import extract_meshes, keep_largest_components
    from dgs_amd.synthetic import write_dynamic_dnerf
    data, model = str(tmp_path / "scene"), str(tmp_path / "model")
    write_dynamic_dnerf(data, n_train=24, n_test=3, H=128, W=128, device=DEV)
    fit(data, model, iterations=300, device=DEV, num_pts=5000, node_num=128, seed=0, warm_up=100, regularize_from=180, densify_from=100,
        densify_interval=50, opacity_reset_interval=10_000)
    real, calls = mesh_clean.filter_components, []

    def counting(v, f, c=None, **kw):
        calls.append(("device", v.is_cuda, f.shape[0]))
        return real(v, f, c, **kw)

    def forced(v, f, c=None, **kw):
        host = keep_largest_components(v, f, c, **kw)
        same_mesh(real(v, f, c, **kw), host)
        calls.append(("host", v.is_cuda, f.shape[0], host[1].shape[0]))
        return host

    monkeypatch.setattr(mesh_clean, "filter_components", counting)
    a = extract_meshes(model, data, times=[0.2, 0.7], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "a"))
    monkeypatch.setattr(mesh_clean, "filter_components", forced)
    b = extract_meshes(model, data, times=[0.2, 0.7], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "b"))
    print(calls)
    assert [c[0] for c in calls] == ["device", "device", "host", "host"] and all(c[1] for c in calls)
    assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b] == ["frame_0.ply", "frame_1.ply"]
    for pa, pb in zip(a, b):
        ba, bb = open(pa, "rb").read(), open(pb, "rb").read()
        assert len(ba) > 1000 and ba == bb
