"""-m gpu: dgs_tri_search against the PyTorch statement of its arithmetic (bit for bit) and the float64 brute force of
tests/mesh_surface_ref.py, at the sizes where the kernel changes path (from dgs_tri_layout: Q queries per workgroup, T triangles per
LDS round, C the default slice), the tie rule across slices, the initialisation of the output, faces without area and needles on the
device, and mesh_distance(mode="surface") on the device against the CPU path."""
import ctypes
import functools

import pytest
import torch

import mesh_surface_ref as ref
from test_mesh_metrics_cpu import concentric_spheres

pytestmark = pytest.mark.gpu


def _layout():
    from dgs_amd import _mesh_ops
    return _mesh_ops.tri_layout()


Q, T, C, ROW = _layout()
NQ = [1, Q - 1, Q, Q + 1, 3 * Q + 5]
NF = [1, 2, T - 1, T, T + 1, 2 * T + 3]


@functools.lru_cache(maxsize=None)
def reference(nq, nf):
    """One (Nq, Nf) case on the device and what it must give: the table, the PyTorch statement in fp32 on the device, and the
    float64 brute force on the CPU (distance and tolerance unit of every pair).  Computed once per shape, never modified."""
    from dgs_amd.mesh_metrics import closest_face_torch, triangle_table
    p, v, f = ref.case(nq, nf)
    pd, table = p.cuda(), triangle_table(v.cuda(), f.cuda())
    d2_t, face_t = closest_face_torch(pd, table)
    d64, unit = ref.brute_force64(p, v, f)
    return pd, table, d2_t, face_t, d64, unit


def check_case(nq, nf, tri_chunk):
    from dgs_amd import _mesh_ops
    pd, table, d2_t, face_t, d64, unit = reference(nq, nf)
    assert table.shape == (nf, ROW)
    d2, face = _mesh_ops.closest_face(pd, table, tri_chunk)
    torch.cuda.synchronize()
    assert d2.dtype == torch.float32 and face.dtype == torch.int64 and d2.shape == face.shape == (nq,)
    assert int(face.min()) >= 0 and int(face.max()) < nf
    assert torch.equal(face, face_t) and torch.equal(d2, d2_t)
    ref.check_against_float64(d2, face, d64, unit, "Nq %d Nf %d chunk %s" % (nq, nf, tri_chunk))
    ref.check_against_float64(d2_t, face_t, d64, unit, "  the statement on the device")


@pytest.mark.parametrize("chunk", ["default", "T"])
@pytest.mark.parametrize("nf", NF)
@pytest.mark.parametrize("nq", NQ)
def test_tri_search_edge_sizes(nq, nf, chunk):
    """chunk = T: several slices of a single round each, meeting through the atomic minimum."""
    check_case(nq, nf, None if chunk == "default" else T)


def test_tri_search_slices_that_do_not_align_with_the_rounds():
    """tri_chunk = T + 1: every slice is one full round and a round of one triangle, the last slice is ragged."""
    check_case(Q + 1, 5 * T + 7, T + 1)


def test_tri_search_default_chunk_with_more_than_one_slice():
    check_case(Q + 1, C + T + 5, None)
    check_case(7, 2 * C + 1, None)


def test_the_cases_are_the_measured_ones():
    """tools/mesh_surface_margins.py measured the tolerance's constant on exactly the shapes above."""
    mine = [(nq, nf) for nq in NQ for nf in NF] + [(Q + 1, 5 * T + 7), (Q + 1, C + T + 5), (7, 2 * C + 1)]
    assert sorted(mine) == sorted(ref.gpu_cases((Q, T, C, ROW)))


def test_ties_across_slices_go_to_the_lowest_face():
    """The same triangle at faces 3, T + 3 and 2T + 3 with tri_chunk = T: three slices report the same distance for the queries
    around it, and the packed minimum keeps face 3 whichever slice's atomic lands first."""
    from dgs_amd.mesh_metrics import closest_face, closest_face_torch, triangle_table
    v, f = ref.soup(2 * T + 10, 11)
    v[9:12] = torch.tensor([[5.0, 5.0, 5.0], [5.5, 5.0, 5.0], [5.0, 5.5, 5.25]])
    f[T + 3] = f[3]
    f[2 * T + 3] = f[3]
    g = torch.Generator().manual_seed(12)
    q = torch.cat([v[9:10], v[9:10] + torch.rand(Q + 40, 3, generator=g) * 0.5, ref.queries(50, 13, v[:9], f[:3])])
    qd, vd, fd = q.cuda(), v.cuda(), f.cuda()
    d2, face = closest_face(qd, vd, fd, face_chunk=T)
    d2_t, face_t = closest_face_torch(qd, triangle_table(vd, fd))
    assert torch.equal(face[:Q + 41], torch.full((Q + 41,), 3, dtype=torch.int64, device="cuda"))
    assert float(d2[0]) == 0.0 and torch.equal(face, face_t) and torch.equal(d2, d2_t)
    assert bool((face[Q + 41:] != 3).all())


def test_output_buffer_is_initialised_by_every_call():
    """Two calls on ONE output buffer through the C ABI, the first with a mesh that is near the queries, the second with one that is
    far: the second result holds no minimum of the first."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import closest_face_torch, triangle_table
    lib = _mesh_ops.load()
    v, f = ref.soup(T + 9, 22)
    q = ref.queries(Q + 3, 21, v, f).cuda()
    near, far = triangle_table(v.cuda(), f.cuda()), triangle_table((v + 7.0).cuda(), f.cuda())
    best = torch.empty(q.shape[0], dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    unpack = lambda b: ((b >> 32).to(torch.int32).view(torch.float32), b & 0xFFFFFFFF)
    for table in (near, far):
        assert lib.dgs_tri_search(q.shape[0], q.data_ptr(), table.shape[0], table.data_ptr(), C, best.data_ptr(), stream) == 0
        d2, face = unpack(best.clone())
        d2_t, face_t = closest_face_torch(q, table)
        assert torch.equal(d2, d2_t) and torch.equal(face, face_t)
    assert float(d2.min()) > 9.0


def test_faces_without_area_and_needles_on_the_device():
    from dgs_amd.mesh_metrics import closest_face, closest_face_torch, triangle_table
    v, f, p, want = ref.degenerates()
    d2, face = closest_face(p.cuda(), v.cuda(), f.cuda())
    assert not bool(torch.isnan(d2).any())
    assert torch.equal(d2.cpu().double().sqrt(), want) and torch.equal(face.cpu(), torch.tensor([0, 1, 2, 2, 3, 3, 0]))
    v, f, p = ref.needles()
    d2, face = closest_face(p.cuda(), v.cuda(), f.cuda())
    d2_t, face_t = closest_face_torch(p.cuda(), triangle_table(v.cuda(), f.cuda()))
    assert torch.equal(d2, d2_t) and torch.equal(face, face_t)
    d64, unit = ref.brute_force64(p, v, f)
    ref.check_against_float64(d2, face, d64, unit, "needles")


def test_closest_face_refuses_bad_input_before_any_launch():
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import closest_face, triangle_table
    v, f = ref.soup(12, 32)
    q = ref.queries(9, 31, v, f)
    qd, vd, fd = q.cuda(), v.cuda(), f.cuda()
    bad = qd.clone()
    bad[4, 2] = float("inf")
    with pytest.raises(ValueError):
        closest_face(bad, vd, fd)
    bad = vd.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(ValueError):
        closest_face(qd, bad, fd)
    with pytest.raises(ValueError):
        closest_face(qd, vd, fd[:0])
    with pytest.raises(ValueError):
        closest_face(qd, v, f)
    d2, face = closest_face(qd[:0], vd, fd)
    assert d2.shape == (0,) and face.shape == (0,) and d2.is_cuda and face.dtype == torch.int64
    with pytest.raises(RuntimeError, match="tri_chunk"):
        closest_face(qd, vd, fd, face_chunk=0)
    with pytest.raises(RuntimeError, match="table"):
        _mesh_ops.closest_face(qd, triangle_table(vd, fd)[:, :34].contiguous())


def test_mesh_distance_surface_on_the_device_equals_the_cpu_path():
    """The samples are the same points (CPU generator, float64 sampling) and the arithmetic of the search is the same: identical
    faces, metrics equal to 1e-6 relative.  S_DEV samples span five query blocks; the spheres have 3968 faces, 16 rounds."""
    from dgs_amd.mesh_metrics import closest_face, mesh_distance, sample_surface
    S_DEV = 4 * Q + 77
    inner, outer = concentric_spheres()
    kw = dict(n_samples=S_DEV, seed=0, thresholds=(0.05, 0.15), mode="surface")
    cpu = mesh_distance(inner, outer, device="cpu", **kw)
    dev = mesh_distance(inner, outer, device="cuda:0", **kw)
    print(dev)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "normal_consistency"):
        assert dev[k] == pytest.approx(cpu[k], rel=1e-6), k
    for k in ("precision", "recall", "fscore"):
        assert dev[k] == cpu[k]
    assert dev["fscore"] == {"0.05": 0.0, "0.15": 1.0} and set(dev) == set(cpu)
    t = lambda m, d: (torch.from_numpy(m[0]).to(d), torch.from_numpy(m[1]).long().to(d))
    pc, _, _ = sample_surface(*t(inner, "cpu"), S_DEV, 0)
    gc, _, _ = sample_surface(*t(outer, "cpu"), S_DEV, 1)
    for pts, mesh in ((pc, outer), (gc, inner)):
        d2, face = closest_face(pts.cuda(), *t(mesh, "cuda"))
        d2_c, face_c = closest_face(pts, *t(mesh, "cpu"))
        print("d2 bit-identical to the CPU path:", torch.equal(d2.cpu(), d2_c))
        assert torch.equal(face.cpu(), face_c)
        torch.testing.assert_close(d2.cpu(), d2_c, rtol=1e-5, atol=0.0)     # the two tables' reciprocals come from two divisions
