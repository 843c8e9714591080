"""-m gpu: dgs_simplify_accumulate / dgs_simplify_solve and dgs_amd.mesh_simplify on a HIP device against the CPU statement.  Every
comparison is exact: the int64 rows, the fp32 bit patterns of vertices and colours, the faces and the cluster map."""
import ctypes

import numpy as np
import pytest
import torch

from test_mesh_cpu import fusion_inputs, sphere_box
from test_mesh_simplify_cpu import analytic_mesh, same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cells_cpu(v, cell, origin=None):
    from dgs_amd.mesh_simplify import _cells
    cell_t = torch.full((1,), float(np.float32(cell)), dtype=torch.float32)
    org = v.amin(0) - cell_t * 0.5 if origin is None else torch.tensor(origin, dtype=torch.float32)
    cluster, centre, problems = _cells(v, cell_t, org)
    assert not any(problems.tolist())
    return cluster, centre, cell_t


def check_rows(v, f, c, cell, origin=None):
    """The rows of the kernel from the CPU's cells against the rows of the CPU statement; -> the number of clusters."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_simplify import _accumulate_torch
    cluster, centre, cell_t = cells_cpu(v, cell, origin)
    want = _accumulate_torch(v, c, f.long(), cluster, centre, cell_t)
    got = _mesh_ops.simplify_accumulate(v.to(DEV), None if c is None else c.to(DEV), f.to(torch.int32).to(DEV), cluster.to(torch.int32).to(DEV),
                                        centre.to(DEV), float(cell_t))
    assert got.dtype == torch.int64 and got.is_cuda and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    return centre.shape[0]


def check_mesh(v, f, c, cell, origin=None, placements=("quadric", "average")):
    """simplify_mesh on the device (cells, kernels and faces there) against the CPU run; -> the CPU result."""
    from dgs_amd.mesh_simplify import simplify_mesh
    for placement in placements:
        want = simplify_mesh(v, f, c, cell_size=cell, placement=placement, origin=origin, return_cluster=True)
        got = simplify_mesh(v.to(DEV), f.to(DEV), None if c is None else c.to(DEV), cell_size=cell, placement=placement, origin=origin, return_cluster=True)
        assert all(x.is_cuda for x in got if x is not None)
        same_bits(got, want)
    return want


@pytest.fixture(scope="module")
def device_mesh():
    """The recipe of tests/test_mesh_clean_gpu.py: the sphere and the plate of tests/test_mesh_cpu.py fused at 96^3 from 24 views
    of 200^2 and extracted on the device; here as CPU tensors."""
    from dgs_amd.mesh import TSDFVolume
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = (x.to(DEV) for x in fusion_inputs(24, 200, plate=True))
    v, f, c = TSDFVolume(origin, h, (N,) * 3, DEV).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0).extract()
    assert v.is_cuda and f.shape[0] > 10000
    return v.cpu(), f.cpu(), c.cpu(), h


def random_soup(n_tris, seed, size=0.01):
    """n_tris small triangles in the unit cube, three vertices each -> (v [3n,3], f [n,3] int32, c [3n,3])."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n_tris, 1, 3), generator=g) * (1 - 2 * size) + size
    v = (base + (torch.rand((n_tris, 3, 3), generator=g) - 0.5) * size).reshape(-1, 3).contiguous()
    f = torch.arange(3 * n_tris, dtype=torch.int32).reshape(n_tris, 3)
    return v, f, torch.rand((3 * n_tris, 3), generator=g)


# ---- the analytic shapes and an extracted mesh -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sphere", "cube"])
def test_analytic_shapes(shape):
    v, f, c, h = analytic_mesh(shape)
    n = check_rows(v, f, c, 2 * h)
    assert n > 500
    sv, sf, sc, cmap = check_mesh(v, f, c, 2 * h)
    assert sf.shape[0] * 8 < f.shape[0]
    check_mesh(v, f.long(), None, 3 * h, placements=("quadric",))


def test_a_mesh_extracted_on_the_device(device_mesh):
    v, f, c, h = device_mesh
    check_rows(v, f, c, 2 * h)
    sv, sf, sc, cmap = check_mesh(v, f, c, 2 * h)
    print("extracted mesh: %d -> %d faces" % (f.shape[0], sf.shape[0]))
    assert sf.shape[0] * 6 < f.shape[0]
    check_mesh(v, f, c, 5 * h, placements=("quadric",))


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def test_layout_boundaries():
    """F and V at 1, at one workgroup - 1, + 0, + 1 and at a ragged second workgroup; the last item must count."""
    from dgs_amd import _mesh_ops
    threads, per_thread = _mesh_ops.simplify_layout()[:2]
    per_group = threads * per_thread
    g = torch.Generator().manual_seed(3)
    for n in (1, per_group - 1, per_group, per_group + 1, 2 * per_group - 37):
        v, c = torch.rand((n, 3), generator=g), torch.rand((n, 3), generator=g)                     # V = n, F = 300 (F = 1 for one vertex)
        f = torch.randint(0, n, (300 if n > 1 else 1, 3), generator=g, dtype=torch.int32)
        check_rows(v, f, c, 0.25, origin=(0, 0, 0))
        check_mesh(v, f, c, 0.25)
        v, c = torch.rand((40, 3), generator=g), torch.rand((40, 3), generator=g)                   # F = n, V = 40
        f = torch.randint(0, 40, (n, 3), generator=g, dtype=torch.int32)
        f[-1] = torch.tensor([37, 38, 39])
        check_rows(v, f, None, 0.25, origin=(0, 0, 0))
        check_mesh(v, f, c, 0.25)


# ---- combining and contention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["by cluster", "shuffled"])
def test_eight_clusters_take_every_add(order):
    """10^5 small triangles in the unit cube at cell 0.5: eight rows take 3 * 10^5 vertex adds and at least 10^5 face adds.  Sorted by
    cluster, whole workgroups combine into one run; shuffled, neighbouring lanes rarely share a cluster and the atomics carry it."""
    v, f, c = random_soup(100_000, seed=9)
    key = ((v[f[:, 0].long()] >= 0.5).long() * torch.tensor([4, 2, 1])).sum(1)
    perm = torch.argsort(key, stable=True) if order == "by cluster" else torch.randperm(f.shape[0], generator=torch.Generator().manual_seed(2))
    v = v.reshape(-1, 3, 3)[perm].reshape(-1, 3).contiguous()
    c = c.reshape(-1, 3, 3)[perm].reshape(-1, 3).contiguous()
    assert check_rows(v, f, c, 0.5, origin=(0, 0, 0)) == 8
    check_mesh(v, f, c, 0.5, origin=(0, 0, 0))


def test_two_runs_are_bit_identical(device_mesh):
    from dgs_amd.mesh_simplify import simplify_mesh
    v, f, c, h = (x.to(DEV) if torch.is_tensor(x) else x for x in device_mesh)
    first = simplify_mesh(v, f, c, cell_size=3 * h, return_cluster=True)
    same_bits(simplify_mesh(v, f, c, cell_size=3 * h, return_cluster=True), first)
    sv, sf, sc = random_soup(20_000, seed=4)
    a = simplify_mesh(sv.to(DEV), sf.to(DEV), sc.to(DEV), cell_size=0.5, origin=(0, 0, 0))
    same_bits(simplify_mesh(sv.to(DEV), sf.to(DEV), sc.to(DEV), cell_size=0.5, origin=(0, 0, 0)), a)


# ---- the guards --------------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_range_are_skipped_by_the_kernel():
    """The C call itself (the wrapper produces no such ids): a vertex id outside [0, V) drops its face, a cluster id outside [0, C)
    drops that vertex and that corner's contribution; the other corners of the face still count, and a sentinel-filled margin
    around the rows is untouched."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_simplify import _accumulate_torch
    lib = _mesh_ops.load()
    g = torch.Generator().manual_seed(6)
    V = 300
    v, c = torch.rand((V, 3), generator=g), torch.rand((V, 3), generator=g)
    cluster, centre, cell_t = cells_cpu(v, 0.25, (0, 0, 0))
    C = centre.shape[0]
    f = torch.randint(0, V, (500, 3), generator=g, dtype=torch.int32)
    bad_cluster = cluster.clone()
    bad_ids = torch.tensor([-1, C, C + 1, 2 ** 31 - 1, -2 ** 31, -5])
    bad_at = torch.arange(0, V, 7)
    bad_cluster[bad_at] = bad_ids[torch.arange(bad_at.numel()) % bad_ids.numel()]
    bad_f = f.clone()
    bad_f[::9, 1] = torch.tensor([V, -1, V + 3, 2 ** 31 - 1, -2 ** 31])[torch.arange(bad_f[::9].shape[0]) % 5].to(torch.int32)
    # the statement on what is left: the bad vertices moved into an extra cluster whose row is thrown away, the bad faces removed
    moved = cluster.clone()
    moved[bad_at] = C
    ok_f = torch.ones(500, dtype=torch.bool)
    ok_f[::9] = False
    want = _accumulate_torch(v, c, f[ok_f].long(), moved, torch.cat((centre, torch.zeros((1, 3)))), cell_t)[:C]
    guard = torch.full((C * 16 + 64,), -7, dtype=torch.int64, device=DEV)
    rows = guard[32:32 + C * 16]
    dv, dc, df, dk, dctr = v.to(DEV), c.to(DEV), bad_f.to(DEV), bad_cluster.to(torch.int32).to(DEV), centre.to(DEV)
    assert dk.dtype == torch.int32 and int((dk.cpu() == bad_cluster.to(torch.int32)).all())
    rc = lib.dgs_simplify_accumulate(V, dv.data_ptr(), dc.data_ptr(), 500, df.data_ptr(), dk.data_ptr(), C, dctr.data_ptr(), float(cell_t),
                                     rows.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu().reshape(C, 16), want)
    assert bool((guard[:32] == -7).all()) and bool((guard[32 + C * 16:] == -7).all())


# ---- the product -------------------------------------------------------------------------------------------------------------------
def test_extract_meshes_simplifies_on_the_device(tmp_path, monkeypatch):
    """The scene and sizes of tests/test_mesh_gpu.py::test_extract_meshes_on_a_short_fit.  With simplify_cell the filtered frame --
    the very mesh the run without it writes -- goes through simplify_mesh on the device, and what is written is bit for bit the CPU
    simplify_mesh of that frame."""
    from dgs_amd import mesh_simplify
    from dgs_amd.fit import fit
    from dgs_amd.io import write_mesh_ply
    from dgs_amd.mesh import extract_meshes
    from dgs_amd.synthetic import write_dynamic_dnerf
    data, model = str(tmp_path / "scene"), str(tmp_path / "model")
    write_dynamic_dnerf(data, n_train=24, n_test=3, H=128, W=128, device=DEV)
    fit(data, model, iterations=300, device=DEV, num_pts=5000, node_num=128, seed=0, warm_up=100, regularize_from=180, densify_from=100,
        densify_interval=50, opacity_reset_interval=10_000)
    real, seen = mesh_simplify.simplify_mesh, []

    def recording(v, f, c=None, **kw):
        out = real(v, f, c, **kw)
        seen.append(((v, f, c), kw, out))
        return out

    monkeypatch.setattr(mesh_simplify, "simplify_mesh", recording)
    full = extract_meshes(model, data, times=[0.2], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "a"))
    assert not seen
    light = extract_meshes(model, data, times=[0.2], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "b"), simplify_cell=0.06)
    assert len(seen) == 1
    frame, kw, out = seen[0]
    assert all(x.is_cuda for x in frame + out) and kw == {"cell_size": 0.06}
    same_bits(out, real(*(x.cpu() for x in frame), cell_size=0.06))
    print("frame: %d -> %d faces" % (frame[1].shape[0], out[1].shape[0]))
    assert 0 < out[1].shape[0] * 4 < frame[1].shape[0]
    for mesh, path in ((frame, full[0]), (out, light[0])):
        want = str(tmp_path / "want.ply")
        write_mesh_ply(want, *mesh)
        assert open(path, "rb").read() == open(want, "rb").read()
