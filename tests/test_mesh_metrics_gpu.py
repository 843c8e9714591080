"""-m gpu: dgs_nn_search against the PyTorch statement of its arithmetic (bit for bit) and a float64 brute force, at the sizes where
the kernel changes path (taken from dgs_nn_layout: Q queries per workgroup, T reference points per LDS round, C the default slice),
the tie rule across slices, the initialisation of the output, and the public metrics on the device against the CPU path."""
import ctypes
import functools
import math

import pytest
import torch

from test_mesh_metrics_cpu import (S_SAMPLES, U32, analytic_sphere, brute_force64, cloud, concentric_cpu, concentric_spheres,
                                   fused_sphere_bound)
from test_mesh_cpu import fusion_inputs, sphere_box

pytestmark = pytest.mark.gpu


def _layout():
    from dgs_amd import _mesh_ops
    return _mesh_ops.nn_layout()


Q, T, C = _layout()
NQ = [1, Q - 1, Q, Q + 1, 3 * Q + 5]
NR = [1, 2, T - 1, T, T + 1, 2 * T + 3]


@functools.lru_cache(maxsize=None)
def reference(nq, nr):
    """Inputs of one (Nq, Nr) case on the device and what they must give: the PyTorch statement in fp32 on the device, and the
    float64 brute force (minimum per query, and d2 of a query to any index).  Computed once per shape, never modified."""
    from dgs_amd.mesh_metrics import nearest_torch
    q, r = cloud(nq, 100 + nq), cloud(nr, 200 + nr)
    qd, rd = q.cuda(), r.cuda()
    d2_t, idx_t = nearest_torch(qd, rd)
    m64, _, at = brute_force64(q, r)
    return qd, rd, d2_t, idx_t, m64, at


def check_case(nq, nr, ref_chunk):
    from dgs_amd.mesh_metrics import nearest
    qd, rd, d2_t, idx_t, m64, at = reference(nq, nr)
    d2, idx = nearest(qd, rd, ref_chunk=ref_chunk)
    torch.cuda.synchronize()
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64 and d2.shape == idx.shape == (nq,)
    assert int(idx.min()) >= 0 and int(idx.max()) < nr
    assert torch.equal(idx, idx_t) and torch.equal(d2, d2_t)
    d_at = at(idx)
    err = (d2.cpu().double() - d_at).abs()
    print("Nq %d Nr %d chunk %s: max |d2 - d2_64| / d2_64 = %.3e (cap %.3e), max d2_64(idx) / min_64 - 1 = %.3e (cap %.3e)"
          % (nq, nr, ref_chunk, float((err / d_at.clamp(min=1e-300)).max()), 6 * U32, float((d_at / m64.clamp(min=1e-300)).max() - 1), 12 * U32))
    assert bool((err <= 6 * U32 * d_at).all())
    assert bool((d_at <= m64 * (1 + 12 * U32)).all())


@pytest.mark.parametrize("chunk", ["default", "T"])
@pytest.mark.parametrize("nr", NR)
@pytest.mark.parametrize("nq", NQ)
def test_nn_search_edge_sizes(nq, nr, chunk):
    """chunk = T: several slices of a single round each, meeting through the atomic minimum."""
    check_case(nq, nr, None if chunk == "default" else T)


def test_nn_search_slices_that_do_not_align_with_the_rounds():
    """ref_chunk = T + 1: every slice is one full round and a round of one point, the last slice is ragged."""
    check_case(Q + 1, 5 * T + 7, T + 1)


def test_nn_search_default_chunk_with_more_than_one_slice():
    check_case(Q + 1, C + T + 5, None)
    check_case(7, 2 * C + 1, None)


def test_ties_across_slices_go_to_the_lowest_index():
    """The same point at indices 3, T + 3 and 2T + 3 with ref_chunk = T: three slices report the same distance for the queries
    around it, and the packed minimum keeps index 3 whichever slice's atomic lands first."""
    from dgs_amd.mesh_metrics import nearest, nearest_torch
    r = cloud(2 * T + 10, 11)
    r[3] = torch.tensor([5.0, 5.0, 5.0])
    r[T + 3] = r[3]
    r[2 * T + 3] = r[3]
    g = torch.Generator().manual_seed(12)
    q = torch.cat([r[3:4], r[3:4] + (torch.rand(Q + 40, 3, generator=g) - 0.5), cloud(50, 13)])
    qd, rd = q.cuda(), r.cuda()
    d2, idx = nearest(qd, rd, ref_chunk=T)
    d2_t, idx_t = nearest_torch(qd, rd)
    assert torch.equal(idx[:Q + 41], torch.full((Q + 41,), 3, dtype=torch.int64, device="cuda"))
    assert float(d2[0]) == 0.0 and torch.equal(idx, idx_t) and torch.equal(d2, d2_t)
    assert bool((idx[Q + 41:] != 3).all())


def test_output_buffer_is_initialised_by_every_call():
    """Two calls on ONE output buffer through the C ABI, the first with a reference set that is near the queries, the second with one
    that is far: the second result holds no minimum of the first.  Then the same through the binding, whose buffers the caching
    allocator reuses."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import nearest, nearest_torch
    lib = _mesh_ops.load()
    q = cloud(Q + 3, 21).cuda()
    near, far = cloud(T + 9, 22).cuda(), (cloud(T + 9, 23) + 7.0).cuda()
    best = torch.empty(q.shape[0], dtype=torch.int64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    unpack = lambda b: ((b >> 32).to(torch.int32).view(torch.float32), b & 0xFFFFFFFF)
    for ref in (near, far):
        assert lib.dgs_nn_search(q.shape[0], q.data_ptr(), ref.shape[0], ref.data_ptr(), C, best.data_ptr(), stream) == 0
        d2, idx = unpack(best.clone())
        d2_t, idx_t = nearest_torch(q, ref)
        assert torch.equal(d2, d2_t) and torch.equal(idx, idx_t)
    assert float(d2.min()) > 30.0
    a = nearest(q, near)
    del a
    d2, idx = nearest(q, far)
    assert torch.equal(d2, d2_t) and torch.equal(idx, idx_t)


def test_nearest_refuses_bad_input_before_any_launch():
    from dgs_amd.mesh_metrics import nearest
    q, r = cloud(9, 31).cuda(), cloud(12, 32).cuda()
    bad = q.clone()
    bad[4, 2] = float("inf")
    with pytest.raises(ValueError):
        nearest(bad, r)
    bad = r.clone()
    bad[0, 0] = float("nan")
    with pytest.raises(ValueError):
        nearest(q, bad)
    with pytest.raises(ValueError):
        nearest(q, r[:0])
    with pytest.raises(ValueError):
        nearest(q, r.cpu())
    d2, idx = nearest(q[:0], r)
    assert d2.shape == (0,) and idx.shape == (0,) and d2.is_cuda and idx.dtype == torch.int64
    with pytest.raises(RuntimeError, match="ref_chunk"):
        nearest(q, r, ref_chunk=0)


def test_mesh_distance_on_the_device_equals_the_cpu_path():
    """The samples are the same points (CPU generator, float64 sampling), the arithmetic of the search is the same: identical
    indices, metrics equal to 1e-6 relative.  S_DEV samples keep the CPU side of the comparison under a second; they span five
    query blocks and more than one slice of the reference set."""
    from dgs_amd.mesh_metrics import mesh_distance, nearest, sample_surface
    S_DEV = 4 * Q + C // 2 + 77
    inner, outer = concentric_spheres()
    cpu = concentric_cpu(S_DEV)
    dev = mesh_distance(inner, outer, n_samples=S_DEV, seed=0, thresholds=(0.05, 0.15), device="cuda:0")
    print(dev)
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "normal_consistency"):
        assert dev[k] == pytest.approx(cpu[k], rel=1e-6), k
    for k in ("precision", "recall", "fscore"):
        assert dev[k] == cpu[k]
    assert dev["fscore"] == {"0.05": 0.0, "0.15": 1.0}
    assert all(dev[k] == cpu[k] for k in ("n_samples", "pred_faces", "gt_faces", "pred_vertices", "gt_vertices"))
    t = lambda m, d: (torch.from_numpy(m[0]).to(d), torch.from_numpy(m[1]).to(d))
    pc, fc, nc = sample_surface(*t(inner, "cpu"), S_DEV, 0)
    pd, fd, nd = sample_surface(*t(inner, "cuda"), S_DEV, 0)
    gc, _, _ = sample_surface(*t(outer, "cpu"), S_DEV, 1)
    gd, _, _ = sample_surface(*t(outer, "cuda"), S_DEV, 1)
    assert torch.equal(pd.cpu(), pc) and torch.equal(fd.cpu(), fc) and torch.equal(gd.cpu(), gc)
    assert float((nd.cpu() - nc).abs().max()) <= 1e-6
    for a_dev, b_dev, a_cpu, b_cpu in ((pd, gd, pc, gc), (gd, pd, gc, pc)):
        d2, idx = nearest(a_dev, b_dev)
        d2_c, idx_c = nearest(a_cpu, b_cpu)
        assert torch.equal(idx.cpu(), idx_c) and torch.equal(d2.cpu(), d2_c)


def test_fused_sphere_on_the_device_against_the_analytic_sphere():
    """The HIP fuser and extraction (N = 96, 24 views) against a UV sphere of the true radius and centre, with the bound of the CPU
    test: both directed means <= h + sqrt(A / S)."""
    from dgs_amd.mesh import TSDFVolume
    from dgs_amd.mesh_metrics import mesh_distance
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = (x.cuda() for x in fusion_inputs(24, 200))
    vol = TSDFVolume(origin, h, (N, N, N), "cuda:0").integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    v, f, _ = vol.extract()
    m = mesh_distance((v, f), analytic_sphere(), n_samples=S_SAMPLES, seed=0, device="cuda:0")
    bound = fused_sphere_bound(vol.voxel_size)
    print("fused sphere (HIP) vs analytic: accuracy %.6f, completeness %.6f (bound %.6f, h %.6f), fscore %s, normal consistency %.4f"
          % (m["accuracy"], m["completeness"], bound, vol.voxel_size, m["fscore"], m["normal_consistency"]))
    assert m["accuracy"] <= bound and m["completeness"] <= bound
    assert math.isfinite(m["chamfer"]) and m["pred_faces"] == f.shape[0]
