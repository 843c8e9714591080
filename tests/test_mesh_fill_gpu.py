"""-m gpu: dgs_fill_rank, dgs_fill_rim, dgs_fill_emit and dgs_amd.mesh_fill on a HIP device against the CPU statement.  Every comparison
is exact: the integer loops, ranks and faces, and the bit patterns of the fp64 rim tables and of the fp32 vertices and colours."""
import numpy as np
import pytest
import torch

from test_mesh_cpu import fusion_inputs, sphere_box
from test_mesh_fill_cpu import annulus, compact, grid_faces, loops_of, punched_torus
from test_mesh_simplify_cpu import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def punched_grid(nu, nw, blocks, triangles=()):
    """A planar nu x nw vertex grid with the quad blocks (column, row, columns, rows, one more face) and single faces taken out, as
    tests/test_mesh_fill_cpu.py: punched_torus does it -> (v, f int64)."""
    quads, rows = grid_faces(nu, nw, False)
    keep = np.ones((quads.shape[0], 2), dtype=bool)
    for u0, w0, a, b, extra in blocks:
        for i in range(u0, u0 + a):
            keep[i * rows + w0:i * rows + w0 + b] = False
        if extra:
            keep[(u0 + a) * rows + w0 + b - 1, 1] = False
    for u0, w0 in triangles:
        keep[u0 * rows + w0, 0] = False
    x, y = np.meshgrid(np.arange(nu), np.arange(nw), indexing="ij")
    v = np.stack((x, y, 0.05 * np.sin(0.3 * x) * np.cos(0.2 * y)), -1).reshape(-1, 3).astype(np.float32)
    return compact(torch.from_numpy(v), torch.from_numpy(quads[keep]))[:2]


def strip(n_boundary):
    """A triangle strip with n_boundary boundary half-edges (n_boundary - 2 faces): one loop."""
    k = n_boundary - 2
    return torch.tensor([(i, i + 1, i + 2) if i % 2 == 0 else (i + 1, i, i + 2) for i in range(k)], dtype=torch.int64), k + 2


def check_loops(V, f, **kw):
    """boundary_loops on the device against the CPU's; -> the CPU's rims."""
    from dgs_amd.mesh_fill import boundary_loops
    want = boundary_loops(V, f, **kw)
    got = boundary_loops(V, f.to(DEV), **kw)
    assert all(x.is_cuda for x in got) and got[0].dtype == torch.int32 and got[1].dtype == torch.int64
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
    return loops_of(V, f, **kw)


def check_fill(v, f, c=None, **kw):
    """fill_holes on the device against the CPU run; -> the CPU result."""
    from dgs_amd.mesh_fill import fill_holes
    want = fill_holes(v, f, c, **kw)
    got = fill_holes(v.to(DEV), f.to(DEV), None if c is None else c.to(DEV), **kw)
    assert all(x.is_cuda for x in got if x is not None) and got[1].dtype == f.dtype
    same_bits(got, want)
    return want


# ---- ranks --------------------------------------------------------------------------------------------------------------------------
RANK_SIZES = [3, 4, 5, 7, 8, 9, 31, 32, 33, 127, 128, 129]


@pytest.fixture(scope="module")
def many_loops():
    blocks = ((2, 2, 31, 32, 1), (40, 2, 32, 32, 0), (78, 2, 32, 32, 1), (2, 40, 7, 8, 1), (14, 40, 8, 8, 0), (26, 40, 8, 8, 1),
              (40, 40, 2, 2, 1), (46, 40, 2, 2, 0), (52, 40, 1, 2, 1), (58, 40, 1, 1, 1), (64, 40, 1, 1, 0))
    return punched_grid(116, 54, blocks, triangles=((70, 40),))


def test_ranks_across_the_round_counts(many_loops):
    """One mesh with loops of 3 .. 129 edges: the round count changes from 2 to 8 across them, and odd and even counts leave the
    result in different buffers.  Every cap ranks another set of loops with another number of rounds."""
    v, f = many_loops
    V = v.shape[0]
    rims = check_loops(V, f)
    assert sorted(len(r) for r in rims) == sorted(RANK_SIZES + [2 * (115 + 53)])
    for cap in RANK_SIZES:
        got = check_loops(V, f, max_edges=cap)
        assert sorted(len(r) for r in got) == [n for n in RANK_SIZES if n <= cap]
    assert check_loops(V, f, max_edges=2) == []                                              # nothing is eligible: no launch
    assert check_loops(V, f.to(torch.int32), max_edges=64) == [r for r in rims if len(r) <= 64]


def test_five_thousand_triangular_holes():
    quads, rows = grid_faces(145, 145, False)
    keep = np.ones((quads.shape[0], 2), dtype=bool)
    i, j = np.meshgrid(np.arange(71), np.arange(71), indexing="ij")
    keep[((2 * i + 1) * rows + 2 * j + 1).reshape(-1)[:5000], 0] = False
    f = torch.from_numpy(quads[keep])
    rims = check_loops(145 * 145, f, max_edges=3)
    assert len(rims) == 5000 and all(len(r) == 3 for r in rims)
    v = torch.rand((145 * 145, 3), generator=torch.Generator().manual_seed(3))
    out = check_fill(v, f, max_hole_edges=3)
    assert out[0].shape[0] == v.shape[0] and out[1].shape[0] == f.shape[0] + 5000


def test_workgroup_edges_and_permuted_ids():
    """Boundary half-edge counts of T - 1, T, T + 1 and 2 T + 1 with T the nodes of a workgroup (a ragged last workgroup, a full one,
    one node in a second and in a third), and the torus with its vertex ids reversed and permuted."""
    from dgs_amd import _mesh_ops
    T = _mesh_ops.fill_layout()[0] * _mesh_ops.fill_layout()[1]
    for nb in (T - 1, T, T + 1, 2 * T + 1):
        f, V = strip(nb)
        rims = check_loops(V, f)
        assert len(rims) == 1 and len(rims[0]) == nb
        assert check_loops(V, f, max_edges=nb - 1) == []
    v, f, c = punched_torus()
    V = v.shape[0]
    want = check_loops(V, f)
    for perm in (torch.arange(V - 1, -1, -1), torch.randperm(V, generator=torch.Generator().manual_seed(5))):
        got = check_loops(V, perm[f])
        assert sorted(len(r) for r in got) == sorted(len(r) for r in want)


def test_rank_binding_twice_on_the_same_buffers():
    """The raw binding against the statement: rings of 5, 8 and 9 nodes, an open chain and unranked nodes in one table; round counts
    of both parities; a second call on the buffers the first one left; a table where nothing is ranked; a malformed table (a
    ring that is never cut) ends after the same launches."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_fill import rank_torch
    g = torch.Generator().manual_seed(11)
    sizes = (5, 8, 9, 300)
    n = sum(sizes) + 7
    perm = torch.randperm(n, generator=g)
    succ = torch.full((n,), -1, dtype=torch.int64)
    leader = torch.full((n,), -1, dtype=torch.int64)
    at = 0
    for k in sizes:
        ring = perm[at:at + k]
        succ[ring] = ring.roll(-1)
        leader[ring] = ring.min()
        at += k
    chain = perm[at:]
    succ[chain[:-1]] = chain[1:]                                                             # an open chain, not ranked
    succ32, leader32 = succ.to(torch.int32).to(DEV), leader.to(torch.int32).to(DEV)
    a, b = (torch.full((n,), -7, dtype=torch.int64, device=DEV) for _ in range(2))
    r = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    for rounds in (9, 10, 0, 3):
        want = rank_torch(succ, leader, rounds)
        for _ in range(2):
            got = _mesh_ops.fill_rank(succ32, leader32, rounds, a, b, r)
            assert got is r and torch.equal(got.cpu(), want)
    want = rank_torch(succ, leader, 9)
    for k in sizes:                                                                          # the statement itself: every ring ranked 0 .. k - 1
        ring = (leader == leader[perm[sum(sizes[:sizes.index(k)])]]).nonzero().reshape(-1)
        assert sorted(want[ring].tolist()) == list(range(k))
    assert bool((want[chain] == -1).all())
    nothing = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    assert bool((_mesh_ops.fill_rank(succ32, nothing, 9) == -1).all())
    uncut = torch.full((n,), n + 5, dtype=torch.int64)                                       # no node is anybody's leader: the rings are never cut
    got = _mesh_ops.fill_rank(succ32, uncut.to(torch.int32).to(DEV), 9)
    assert torch.equal(got.cpu(), rank_torch(succ, uncut, 9))


# ---- emission -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 9, 10, 16, 100, 128])
def test_emission(n):
    """An n-gon hole in a tilted, slightly buckled fan, with and without colours, int32 and int64 faces: the rim tables, and the
    emitted vertices, colours and faces inside guard margins that stay untouched."""
    from dgs_amd import _mesh_ops, mesh_fill as mf
    from dgs_amd.mesh_decimate import _frame
    v, f = annulus(n)
    g = torch.Generator().manual_seed(n)
    v = v + 0.02 * torch.randn(v.shape, generator=g)
    v = (v @ torch.linalg.qr(torch.randn((3, 3), generator=g))[0] + torch.tensor([0.3, -1.2, 0.7])).contiguous()
    c = torch.rand(v.shape, generator=g) * 1.2 - 0.1                                         # some outside [0, 1]: clamped
    c[1, 0] = float("nan")
    for colors in (c, None):
        for faces in (f, f.to(torch.int32)):
            out = check_fill(v, faces, colors, max_hole_edges=n)
            assert (out[0].shape[0] - v.shape[0], out[1].shape[0] - f.shape[0]) == mf.fill_counts(n)
    V = v.shape[0]
    lv, off = mf.boundary_loops(V, f, max_edges=n)
    assert off.tolist() == [0, n]
    centre, scale = _frame(v)
    centre = [float(x) for x in centre.tolist()]
    lay = mf.ring_layout(V, off)
    rim_loop = torch.zeros(n, dtype=torch.int32)
    S, SC, rows = mf.rim_torch(v, c, lv, rim_loop, off, centre, scale)
    new_v, new_c = mf.vertices_torch(V, lay, off, rows, S, SC, centre, scale)
    vout = torch.cat((v, new_v))
    new_f = mf.faces_torch(lay, off, lv, rows, vout).to(torch.int32)
    dS, dSC, drows = _mesh_ops.fill_rim(v.to(DEV), c.to(DEV), lv.to(DEV), rim_loop.to(DEV), off.to(DEV), centre, scale)
    assert dS.dtype == torch.float64 and torch.equal(dS.cpu().view(torch.int64), S.view(torch.int64))
    assert torch.equal(dSC.cpu().view(torch.int64), SC.view(torch.int64)) and torch.equal(drows.cpu(), rows)

    def margin(shape, dtype, fill):
        k = int(np.prod(shape))
        whole = torch.full((k + 128,), fill, dtype=dtype, device=DEV)
        return whole, whole[64:64 + k].view(shape)

    def untouched(whole, k, fill):
        return bool((whole[:64] == fill).all()) and bool((whole[64 + k:] == fill).all())

    NV, NF = lay["n_new"], lay["n_new_faces"]
    wv, dv = margin((V + NV, 3), torch.float32, -7.0)
    wc, dc = margin((V + NV, 3), torch.float32, -7.0)
    wf, df = margin((NF, 3), torch.int32, -7)
    dv[:V], dc[:V] = v.to(DEV), c.to(DEV)
    dlay = {k: (x.to(DEV) if torch.is_tensor(x) else x) for k, x in lay.items()}
    for _ in range(2):
        _mesh_ops.fill_emit(V, dlay, lv.to(DEV), off.to(DEV), drows, dS, dSC, centre, scale, dv, dc, df)
        torch.cuda.synchronize()
        same_bits((dv.cpu(), dc[V:].cpu(), df.cpu()), (vout, new_c, new_f))
        assert untouched(wv, 3 * (V + NV), -7.0) and untouched(wc, 3 * (V + NV), -7.0) and untouched(wf, 3 * NF, -7)
    assert torch.equal(dc[:V].cpu().view(torch.int32), c.view(torch.int32))                  # the input's rows are read, never written


# ---- the whole function -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4, 16, 64, 1000])
def test_the_torus(cap):
    from dgs_amd.mesh_fill import is_watertight
    v, f, c = punched_torus()
    gv, gf, gc = check_fill(v, f, c, max_hole_edges=cap)
    assert is_watertight(gv.shape[0], gf.to(DEV)) == is_watertight(gv.shape[0], gf) == (cap >= 64)
    check_fill(v, f.to(torch.int32), None, max_hole_edges=cap)


@pytest.fixture(scope="module")
def device_mesh():
    """The recipe of tests/test_mesh_smooth_gpu.py: the sphere and the plate of tests/test_mesh_cpu.py fused at 96^3 from 24 views of
    200^2 and extracted on the device; here as CPU tensors."""
    from dgs_amd.mesh import TSDFVolume
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = (x.to(DEV) for x in fusion_inputs(24, 200, plate=True))
    v, f, c = TSDFVolume(origin, h, (N,) * 3, DEV).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0).extract()
    assert v.is_cuda and f.shape[0] > 10000
    return v.cpu(), f.cpu(), c.cpu(), h


def test_a_mesh_extracted_on_the_device(device_mesh):
    """The extracted mesh (24 views leave it a handful of holes of 4 to 102 edges) with four discs of faces taken out: fill_holes
    closes everything, bit-identical to the CPU; the result is watertight and stays so through decimate_mesh(ratio=0.5)."""
    from dgs_amd.mesh_decimate import decimate_mesh
    from dgs_amd.mesh_fill import fill_holes, is_watertight
    v, f, c, h = device_mesh
    V, fl = v.shape[0], f.long()
    gone = torch.zeros(f.shape[0], dtype=torch.bool)
    for seed, rings in ((1000, 1), (20000, 3), (40000, 6), (60000, 10)):                     # a disc: the faces inside `rings` rings of a vertex
        mark = torch.zeros(V, dtype=torch.bool)
        mark[seed] = True
        for _ in range(rings):
            mark[fl[mark[fl].any(1)].reshape(-1)] = True
        gone |= mark[fl].all(1)
    v, f, c = compact(v, f[~gone], c)
    rims = check_loops(v.shape[0], f)
    assert len(rims) >= 4 and max(len(r) for r in rims) <= 128 and not is_watertight(v.shape[0], f)
    gv, gf, gc = check_fill(v, f, c)
    assert gf.shape[0] > f.shape[0] and is_watertight(gv.shape[0], gf) and is_watertight(gv.shape[0], gf.to(DEV))
    dv, df, dc = decimate_mesh(gv.to(DEV), gf.to(DEV), gc.to(DEV), ratio=0.5)
    assert df.shape[0] <= gf.shape[0] // 2 and is_watertight(dv.shape[0], df)


def test_extract_meshes_fills_on_the_device(tmp_path, monkeypatch):
    """extract_meshes on the device over the analytic sphere views of tests/test_mesh_cpu.py (six views leave the sphere holes of 4
    to 144 edges): with fill_holes the file is, byte for byte, what the CPU path writes for the same filtered mesh; without, what
    it wrote before."""
    from types import SimpleNamespace
    from dgs_amd import fit, io as dio, mesh
    from dgs_amd.mesh_clean import filter_components
    from dgs_amd.mesh_fill import fill_holes, is_watertight
    N = 28
    origin, h = sphere_box(N)
    views = tuple(x.to(DEV) for x in fusion_inputs(6, 64))
    lo = np.asarray(origin, dtype=np.float64)
    monkeypatch.setattr(fit, "restore", lambda *a, **k: (None, None))
    monkeypatch.setattr(dio, "load_dnerf", lambda *a, **k: {"train": [SimpleNamespace(camera=None)] * 6, "test": []})
    monkeypatch.setattr(mesh, "views_at_time", lambda surfels, deform, cams, t, bg, **k: views)
    kw = dict(times=[0.5], voxel_size=h, bounds=(lo, lo + h * (N - 1)), iteration=7, device=DEV, min_faces=0)
    vol = mesh.TSDFVolume.from_bounds(*kw["bounds"], h, DEV).integrate(*views, trunc=5 * h, depth_trunc=6.0)
    v, f, c = (x.cpu() for x in filter_components(*vol.extract(), n_keep=1000, min_faces=0))
    want = str(tmp_path / "want.ply")
    dio.write_mesh_ply(want, v, f, c)
    plain = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "a"), **kw)
    assert open(plain[0], "rb").read() == open(want, "rb").read()
    for cap, closed in ((32, False), (200, True)):
        got = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / str(cap)), fill_holes=cap, **kw)
        gv, gf, gc = fill_holes(v, f, c, max_hole_edges=cap)
        assert gf.shape[0] > f.shape[0] and is_watertight(gv.shape[0], gf) == closed
        dio.write_mesh_ply(want, gv, gf, gc)
        assert open(got[0], "rb").read() == open(want, "rb").read()
