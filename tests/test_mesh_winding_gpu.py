"""-m gpu: dgs_winding_sum against the PyTorch statement of its arithmetic (bit for bit, on the device and on the CPU) and the
float64 brute force of tests/mesh_winding_ref.py, at the sizes where the kernel changes path (from dgs_winding_layout: Q queries per
workgroup, T triangles per LDS round, C the default slice), determinism, the initialisation and the margins of the output, edge
inputs on the device, and contains / volume_iou / mesh_distance on the device against the CPU path."""
import ctypes
import functools

import pytest
import torch

import mesh_winding_ref as ref
from test_mesh_winding_cpu import IOU_KEYS, cube, edge_queries

pytestmark = pytest.mark.gpu


def _layout():
    from dgs_amd import _mesh_ops
    return _mesh_ops.winding_layout()


Q, T, C, ROW = _layout()
NQ = [1, Q - 1, Q, Q + 1, 3 * Q + 5]
NF = [1, 2, T - 1, T, T + 1, 2 * T + 3]


@functools.lru_cache(maxsize=None)
def reference(nq, nf):
    """One (Nq, Nf) case on the device and what it must give: the table, the int64 sums of the PyTorch statement on the device and
    on the CPU, and W of the float64 brute force on the CPU.  Computed once per shape, never modified."""
    from dgs_amd.mesh_metrics import winding_sums_torch, winding_table
    p, v, f = ref.case(nq, nf)
    pd, table = p.cuda(), winding_table(v.cuda(), f.cuda())
    return pd, table, winding_sums_torch(pd, table), winding_sums_torch(p, winding_table(v, f)), ref.brute_force64(p, v, f)


def check_case(nq, nf, tri_chunk):
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import WIND_UNIT
    pd, table, sums_dev, sums_cpu, w64 = reference(nq, nf)
    assert table.shape == (nf, ROW)
    sums = _mesh_ops.winding_sums(pd, table, tri_chunk)
    torch.cuda.synchronize()
    assert sums.dtype == torch.int64 and sums.shape == (nq,) and sums.is_cuda
    assert torch.equal(sums, sums_dev), "the kernel against the statement on the device"
    assert torch.equal(sums.cpu(), sums_cpu), "the kernel against the statement on the CPU"
    w = sums.cpu().double() * WIND_UNIT
    err = float((w - w64).abs().max())
    print("Nq %d Nf %d chunk %s: max |W - W64| = %.3e (cap %.1e)" % (nq, nf, tri_chunk, err, ref.W_TOL_SOUP))
    assert err <= ref.W_TOL_SOUP


@pytest.mark.parametrize("chunk", ["default", "T"])
@pytest.mark.parametrize("nf", NF)
@pytest.mark.parametrize("nq", NQ)
def test_winding_sum_edge_sizes(nq, nf, chunk):
    """chunk = T: several slices of a single round each, meeting through the atomic add."""
    check_case(nq, nf, None if chunk == "default" else T)


def test_winding_sum_slices_that_do_not_align_with_the_rounds():
    """tri_chunk = T + 1: every slice is one full round and a round of one triangle, the last slice is ragged."""
    check_case(Q + 1, 5 * T + 7, T + 1)


def test_winding_sum_default_chunk_with_more_than_one_slice():
    check_case(Q + 1, C + T + 5, None)
    check_case(7, 2 * C + 1, None)


def test_the_cases_are_the_measured_ones():
    """tools/mesh_winding_margins.py measured the tolerance on exactly the shapes above."""
    mine = [(nq, nf) for nq in NQ for nf in NF] + [(Q + 1, 5 * T + 7), (Q + 1, C + T + 5), (7, 2 * C + 1)]
    assert sorted(mine) == sorted(ref.gpu_cases((Q, T, C, ROW))) and ROW == 12


def test_two_calls_are_equal_and_a_stale_buffer_is_overwritten_inside_its_margins():
    """The C ABI on ONE output buffer with guard words on both sides: filled with a stale pattern, called twice; the sums are
    the statement's both times (cleared by the call, not accumulated) and the guards are untouched."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    nq, nf = Q + 1, 2 * T + 3
    pd, table, sums_dev, _, _ = reference(nq, nf)
    G, stale = 64, -0x0123456789ABCDEF
    buf = torch.full((G + nq + G,), stale, dtype=torch.int64, device="cuda")
    out = buf[G:G + nq]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = []
    for _ in range(2):
        assert lib.dgs_winding_sum(nq, pd.data_ptr(), nf, table.data_ptr(), T, out.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        got.append(out.clone())
    assert torch.equal(got[0], sums_dev) and torch.equal(got[1], sums_dev)
    assert bool((buf[:G] == stale).all()) and bool((buf[G + nq:] == stale).all())
    a, b = _mesh_ops.winding_sums(pd, table), _mesh_ops.winding_sums(pd, table, 3 * T)
    assert torch.equal(a, b) and torch.equal(a, sums_dev) and a.dtype == torch.int64 and a.shape == (nq,)


def test_edge_inputs_on_the_device():
    from dgs_amd.mesh_metrics import winding_sums
    v, f = cube()
    p = edge_queries()
    want = winding_sums(p, v, f)
    got = winding_sums(p.cuda(), v.cuda(), f.cuda())
    assert got.is_cuda and torch.equal(got.cpu(), want) and want[5:8].tolist() == [0, 0, 0]
    for bad in (float("nan"), float("inf")):
        vb = v.clone()
        vb[7, 1] = bad
        assert torch.equal(winding_sums(p.cuda(), vb.cuda(), f.cuda()).cpu(), winding_sums(p, vb, f))
    flat = torch.cat([v, torch.tensor([[3.0, 3, 3], [4, 4, 4], [6, 6, 6]])]), torch.cat([f, torch.tensor([[8, 9, 10], [0, 0, 5]])])
    assert torch.equal(winding_sums(p.cuda(), flat[0].cuda(), flat[1].cuda()).cpu(), winding_sums(p, *flat))
    assert winding_sums(p[:0].cuda(), v.cuda(), f.cuda()).shape == (0,)
    with pytest.raises(ValueError, match="no faces"):
        winding_sums(p.cuda(), v.cuda(), f[:0].cuda())
    with pytest.raises(ValueError):
        winding_sums(p.cuda(), v, f)
    with pytest.raises(RuntimeError, match="tri_chunk"):
        winding_sums(p.cuda(), v.cuda(), f.cuda(), face_chunk=0)


@pytest.mark.parametrize("name", ["icosphere 3", "icosphere 5", "torus 64x32", "torus 64x32 flipped", "nested spheres"])
def test_contains_on_the_device_equals_the_cpu_mask(name):
    from dgs_amd.mesh_metrics import contains, winding_number, winding_sums
    p, v, f, want = ref.shape_set(name)
    assert torch.equal(winding_sums(p.cuda(), v.cuda(), f.cuda()).cpu(), winding_sums(p, v, f))
    w_cpu = winding_number(p, v, f)
    w_dev = winding_number(p.cuda(), v.cuda(), f.cuda())
    assert w_dev.dtype == torch.float64 and torch.equal(w_dev.cpu(), w_cpu)
    assert bool(((w_dev.cpu() - want).abs() <= ref.W_TOL).all())
    mask = contains(p.cuda(), v.cuda(), f.cuda())
    assert mask.dtype == torch.bool and torch.equal(mask.cpu(), contains(p, v, f)) and torch.equal(mask.cpu(), want > 0)


def test_volume_iou_on_the_device_returns_the_floats_of_the_cpu():
    from dgs_amd.mesh_metrics import volume_iou
    v, f = ref.icosphere(3)
    a, b = (v.numpy(), f.numpy()), ((v + torch.tensor([0.5, 0.0, 0.0])).numpy(), f.numpy())
    n = 2 * Q + 77
    cpu, dev = volume_iou(a, b, n_samples=n, seed=0, device="cpu"), volume_iou(a, b, n_samples=n, seed=0, device="cuda:0")
    print(dev)
    assert dev == cpu and set(dev) == IOU_KEYS and 0.3 < dev["iou"] < 0.6


def test_mesh_distance_with_iou_on_the_device_equals_the_cpu_path():
    from dgs_amd.mesh_metrics import mesh_distance
    v, f = ref.icosphere(3)
    a, b = (v.numpy(), f.numpy()), ((v * 1.1).numpy(), f.numpy())
    kw = dict(n_samples=2000, seed=0, thresholds=(0.05, 0.15), iou_samples=2000)
    cpu, dev = mesh_distance(a, b, device="cpu", **kw), mesh_distance(a, b, device="cuda:0", **kw)
    assert set(dev) == set(cpu) and IOU_KEYS <= set(dev)
    assert {k: dev[k] for k in IOU_KEYS} == {k: cpu[k] for k in IOU_KEYS} and 0.6 < dev["iou"] < 0.9
    assert dev["chamfer"] == pytest.approx(cpu["chamfer"], rel=1e-5)
