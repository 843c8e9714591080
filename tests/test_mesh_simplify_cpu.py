"""dgs_amd.mesh_simplify on CPU tensors: the statement of include/dgs_mesh_ops.h against independent facts -- a closed sphere stays
closed, quadrics keep a cube's corners, integer rows written out by hand, order independence, degenerate input and refusals, and
the plumbing through extract_meshes and the shell (no device needed).  The mesh builders are shared with
tests/test_mesh_simplify_gpu.py."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

BOX = 2.6          # the analytic volumes live in [-1.3, 1.3]^3
SPHERE_R, CUBE_S = 0.9, 0.703


# ---- meshes ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def analytic_mesh(shape, N=40):
    """(v f32 [V,3], f int32 [F,3], c f32 [V,3], h) -- the sphere |p| = 0.9 or the cube max |p_i| = 0.703 through the CPU marching
    tetrahedra at N^3 over [-1.3, 1.3]^3.  Cached: do not modify."""
    from dgs_amd.mesh import TSDFVolume
    h = BOX / (N - 1)
    vol = TSDFVolume((-BOX / 2,) * 3, h, (N, N, N), "cpu")
    ax = [vol.origin[i] + vol.voxel_size * np.arange(N) for i in range(3)]
    G = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    sdf = np.linalg.norm(G, axis=-1) - SPHERE_R if shape == "sphere" else np.abs(G).max(-1) - CUBE_S
    vol.tsdf = torch.tensor(sdf, dtype=torch.float32)
    vol.weight = torch.ones_like(vol.tsdf)
    vol.color = torch.tensor(np.clip(G / BOX + 0.5, 0, 1), dtype=torch.float32)
    v, f, c = vol.extract()
    return v, f, c, float(vol.voxel_size)


def edge_counts(f):
    """How many faces every undirected edge lies in."""
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    e.sort(1)
    return np.unique(e, axis=0, return_counts=True)[1]


def no_face_repeats(f):
    f = np.asarray(f, dtype=np.int64)
    canon = np.stack([np.roll(r, -int(np.argmin(r))) for r in f])
    return np.unique(canon, axis=0).shape[0] == f.shape[0]


def cube_surface_distance(p, s=CUBE_S):
    a = np.abs(np.asarray(p, dtype=np.float64))
    outside = np.linalg.norm(np.maximum(a - s, 0.0), axis=1)
    return np.where((a <= s).all(1), s - a.max(1), outside)


def same_bits(a, b):
    """Two meshes (v, f, c[, map]) with equal bit patterns, dtypes and shapes."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is None:
            continue
        x, y = x.cpu(), y.cpu()
        assert x.dtype == y.dtype and x.shape == y.shape
        if x.is_floating_point():
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y)


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def test_a_closed_sphere_stays_closed():
    from dgs_amd.mesh_simplify import _cells, simplify_mesh
    v, f, c, h = analytic_mesh("sphere")
    assert (edge_counts(f) == 2).all()
    cell = 2 * h
    sv, sf, sc, cmap = simplify_mesh(v, f, c, cell_size=cell, return_cluster=True)
    print("sphere: %d -> %d faces, %d -> %d vertices" % (f.shape[0], sf.shape[0], v.shape[0], sv.shape[0]))
    assert sv.dtype == torch.float32 and sf.dtype == f.dtype and sc.shape == sv.shape and cmap.dtype == torch.int64
    assert (edge_counts(sf) == 2).all() and no_face_repeats(sf)
    assert sf.shape[0] * 8 < f.shape[0]
    assert int(sf.min()) == 0 and int(sf.max()) == sv.shape[0] - 1 and torch.unique(sf).numel() == sv.shape[0]
    # every output vertex within one cell of its cell's centre per axis.  |fp32(x)| <= 1, so the product with cell is at most cell
    # in magnitude and only the final fp32 addition can add half a unit in the last place of the result.
    cell_t = torch.full((1,), cell, dtype=torch.float32)
    cluster, centre, _ = _cells(v, cell_t, v.amin(0) - cell_t * 0.5)
    kept = cmap >= 0
    assert kept.any() and int(cmap.max()) == sv.shape[0] - 1
    off = (sv[cmap[kept]].double() - centre[cluster[kept]].double()).abs()
    slack = np.spacing(np.abs(sv.numpy()).max().astype(np.float32)) / 2
    assert float(off.max()) <= float(cell_t.double()) + slack
    # and on the sphere: the largest radial error is far below a voxel (1.3e-3 at 64^3 in float64; a 40^3 grid is coarser)
    err = float((sv.double().norm(dim=1) - SPHERE_R).abs().max())
    print("sphere: max | |v| - r | = %.3e (h = %.3e)" % (err, h))
    assert err < 0.1 * h
    assert float(sc.min()) >= 0.0 and float(sc.max()) <= 1.0
    # the colour of a cluster is the mean of its vertices' colours up to the fixed point (2^-25 per term) and the fp32 rounding
    k = int(cmap[kept][0])
    assert torch.allclose(sc[k], c[cmap == k].double().mean(0).float(), atol=1e-6)


def test_quadrics_keep_the_corners_of_a_cube():
    from dgs_amd.mesh_simplify import simplify_mesh
    v, f, c, h = analytic_mesh("cube")
    worst = {}
    for placement in ("quadric", "average"):
        sv, sf, _ = simplify_mesh(v, f, None, cell_size=2 * h, placement=placement)
        assert (edge_counts(sf) == 2).all() and no_face_repeats(sf)
        worst[placement] = float(cube_surface_distance(sv.numpy()).max())
    print("cube: max distance to the surface %s (h = %.3e)" % (worst, h))
    assert worst["quadric"] < worst["average"] / 20


# ---- the integers ---------------------------------------------------------------------------------------------------------------
def hand_case():
    """cell 1, origin 0.  A flat square z = 0.25 of two triangles in cell (0,0,0) (centre (.5,.5,.5)) and a roof triangle (1, 4, 2)
    that climbs into cell (1,0,0): its normal is (-0.1875, 0, 0.25), length 0.3125, direction (-0.6, 0, 0.8), weight 0.15625.
    Flat faces: nh = (0, 0, 1), w = 0.125, d = 0.25, three corners in the cell: zz = 3 * 0.125 * 2^24 each, b_z = 3 * 2^19 each.
    Roof: corners 1 and 2 in cluster 0 (m = 2, p = vertex 1), corner 4 in cluster 1 (m = 1): with x = fp32(-0.6), z = fp32(0.8)
    cluster 0 gets 2 * rn(w x x 2^24) = 2 * 943718, 2 * rn(w x z 2^24) = 2 * -1258291, 2 * rn(w z z 2^24) = 2 * 1677722, and
    d = -(x * 0.25 + z * -0.25) = 0.35: 2 * rn(w d x 2^24) = 2 * -550502, 2 * rn(w d z 2^24) = 2 * 734003."""
    v = torch.tensor([[.25, .25, .25], [.75, .25, .25], [.75, .75, .25], [.25, .75, .25], [1.25, .25, .625]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [1, 4, 2]], dtype=torch.int32)
    rows = [[4, 0, 0, -2 ** 30, 0, 0, 0, 2 * 943718, 0, 2 * -1258291, 0, 0, 6 * 2 ** 21 + 2 * 1677722, 2 * -550502, 0, 6 * 2 ** 19 + 2 * 734003],
            [1, -2 ** 28, -2 ** 28, 2 ** 27, 0, 0, 0, 943718, 0, -1258291, 0, 0, 1677722, 393216, 0, -524288]]
    return v, f, rows


def test_rows_of_a_hand_computed_case():
    from dgs_amd.mesh_simplify import _accumulate_torch, _cells, simplify_mesh
    v, f, want = hand_case()
    cell = torch.ones(1)
    cluster, centre, problems = _cells(v, cell, torch.zeros(3))
    assert cluster.tolist() == [0, 0, 0, 0, 1] and centre.tolist() == [[.5, .5, .5], [1.5, .5, .5]] and not any(problems.tolist())
    rows = _accumulate_torch(v, None, f.long(), cluster, centre, cell)
    assert rows.dtype == torch.int64 and rows.tolist() == want
    col = torch.tensor([[0.5, 2.0, -1.0], [0.25, float("nan"), 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.125, 0.5, 1.0]])
    rows = _accumulate_torch(v, col, f.long(), cluster, centre, cell)
    assert rows[:, 4:7].tolist() == [[int(1.75 * 2 ** 24), 2 * 2 ** 24, 2 ** 24], [2 ** 21, 2 ** 23, 2 ** 24]]      # clamped; NaN is 0
    assert rows[:, :4].tolist() == [r[:4] for r in want] and rows[:, 7:].tolist() == [r[7:] for r in want]
    # two clusters cannot carry a face
    sv, sf, sc, cmap = simplify_mesh(v, f, col, cell_size=1.0, origin=(0, 0, 0), return_cluster=True)
    assert sv.shape == (0, 3) and sf.shape == (0, 3) and sf.dtype == torch.int32 and sc.shape == (0, 3) and cmap.tolist() == [-1] * 5


def test_the_solve_on_planes_it_can_check():
    """Three faces in one cell on the planes x = .25, y = .5, z = .75 (in cell units from the corner): the quadric vertex is their
    intersection up to the pull of the regulariser towards the mean, lambda t (xb - x) with lambda = 2^-10.  A flat cluster goes
    to its mean projected onto the plane; a cluster without faces goes to its mean."""
    from dgs_amd.mesh_simplify import _accumulate_torch, _solve_torch
    cell, centre = torch.full((1,), 2.0), torch.tensor([[1.0, 1.0, 1.0]])
    P = lambda *p: [2.0 * x for x in p]
    v = torch.tensor([P(.25, .2, .2), P(.25, .6, .2), P(.25, .2, .6), P(.2, .5, .2), P(.2, .5, .6), P(.6, .5, .2), P(.2, .2, .75), P(.6, .2, .75), P(.2, .6, .75)])
    f = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    cluster = torch.zeros(9, dtype=torch.int64)
    rows = _accumulate_torch(v, None, f, cluster, centre, cell)
    x, _ = _solve_torch(rows, centre, cell, True, False)
    assert torch.allclose(x, torch.tensor([P(.25, .5, .75)]), atol=2e-3) and not torch.equal(x, torch.tensor([P(.25, .5, .75)]))
    mean, _ = _solve_torch(rows, centre, cell, False, False)
    assert torch.allclose(mean, v.mean(0, keepdim=True), atol=1e-6)
    flat, _ = _solve_torch(_accumulate_torch(v[:3], None, f[:1], cluster[:3], centre, cell), centre, cell, True, False)
    want = v[:3].mean(0)
    assert abs(float(flat[0, 0]) - 0.5) < 1e-6 and torch.allclose(flat[0, 1:], want[1:], atol=1e-6)
    lone, _ = _solve_torch(_accumulate_torch(v[:3], None, f[:0], cluster[:3], centre, cell), centre, cell, True, False)
    assert torch.allclose(lone, want[None], atol=1e-6)


# ---- order ----------------------------------------------------------------------------------------------------------------------
def test_the_order_of_faces_and_vertices_does_not_matter():
    from dgs_amd.mesh_simplify import simplify_mesh
    v, f, c, h = analytic_mesh("sphere")
    base = simplify_mesh(v, f, c, cell_size=3 * h)
    g = torch.Generator().manual_seed(5)
    fp = torch.randperm(f.shape[0], generator=g)
    got = simplify_mesh(v, f[fp], c, cell_size=3 * h)
    same_bits((got[0], got[2]), (base[0], base[2]))
    canon = lambda t: sorted(tuple(np.roll(r, -int(np.argmin(r)))) for r in t.tolist())
    assert canon(got[1]) == canon(base[1])
    vp = torch.randperm(v.shape[0], generator=g)                  # new id -> old id
    inv = torch.empty_like(vp)
    inv[vp] = torch.arange(v.shape[0])
    same_bits(simplify_mesh(v[vp], inv[f.long()].to(f.dtype), c[vp], cell_size=3 * h), base)
    same_bits(simplify_mesh(v, f.long(), c, cell_size=3 * h), (base[0], base[1].long(), base[2]))


# ---- degenerate input -----------------------------------------------------------------------------------------------------------
def test_degenerate_input():
    from dgs_amd.mesh_simplify import simplify_mesh
    e3, ef = torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)
    out = simplify_mesh(e3, ef, e3, cell_size=0.1, return_cluster=True)
    assert [tuple(x.shape) for x in out] == [(0, 3), (0, 3), (0, 3), (0,)]
    pts = torch.rand((50, 3), generator=torch.Generator().manual_seed(1))
    out = simplify_mesh(pts, ef, None, cell_size=0.25, return_cluster=True)               # F = 0: every vertex is unreferenced
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[2] is None and (out[3] == -1).all()
    tri = torch.tensor([[0, 1, 2], [3, 4, 5], [0, 2, 4]], dtype=torch.int64)
    out = simplify_mesh(pts, tri, cell_size=10.0)                                          # everything in one cell
    assert out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[1].dtype == torch.int64
    # faces without area and a repeated index add nothing to the sums and vanish; -0.0 is 0.0
    v = torch.tensor([[-0.0, 0.0, -0.0], [1.0, -0.0, 0.0], [0.0, 1.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    good = torch.tensor([[0, 1, 2], [0, 2, 4], [0, 4, 1], [1, 4, 2]], dtype=torch.int32)
    bad = torch.tensor([[0, 1, 3], [1, 1, 2], [2, 2, 2], [0, 3, 1]], dtype=torch.int32)     # collinear, repeated indices
    a = simplify_mesh(v, good, cell_size=0.5, origin=(-0.25,) * 3, return_cluster=True)
    b = simplify_mesh(v, torch.cat((good, bad)), cell_size=0.5, origin=(-0.25,) * 3, return_cluster=True)
    # the two collinear faces with three cells survive as index triples (and keep vertex 3 alive), the repeated indices go ...
    assert a[1].shape[0] == 4 and a[3].tolist()[3] == -1 and b[1].shape[0] == 6 and b[0].shape[0] == 5
    keep = [0, 1, 2, 4]
    same_bits((b[0][b[3][keep]],), (a[0][a[3][keep]],))                                    # ... and none of them moved a vertex
    assert torch.isfinite(b[0]).all()
    same_bits(simplify_mesh(v.abs(), good, cell_size=0.5, origin=(-0.25,) * 3, return_cluster=True), a)
    # a triangle 10^4 cells wide next to small ones: the weight clamp holds, everything stays finite and inside its cell
    big = torch.tensor([[0.0, 0.0, 0.0], [1e4, 0.0, 0.0], [0.0, 1e4, 0.5], [0.3, 0.2, 0.0], [0.2, 0.4, 0.1], [1.2, 0.1, 0.3]])
    bf = torch.tensor([[0, 1, 2], [0, 3, 4], [3, 5, 4], [1, 2, 5]], dtype=torch.int32)
    sv, sf, _ = simplify_mesh(big, bf, cell_size=1.0)
    assert torch.isfinite(sv).all() and sf.shape[0] >= 1 and float(sv.max()) < 1.0002e4


def test_refusals():
    from dgs_amd.mesh_simplify import simplify_mesh
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for cell in (0.0, -1.0, float("inf"), float("nan"), 1e-60, None):
        with pytest.raises(ValueError, match="cell_size"):
            simplify_mesh(v, f, cell_size=cell)
    for bad in (float("nan"), float("inf")):
        w = v.clone()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            simplify_mesh(w, f, cell_size=0.5)
    for idx in (3, -1):
        with pytest.raises(ValueError, match="out of range"):
            simplify_mesh(v, torch.tensor([[0, 1, idx]], dtype=torch.int32), cell_size=0.5)
    with pytest.raises(ValueError, match="out of range"):
        simplify_mesh(v[:0], f, cell_size=0.5)
    with pytest.raises(ValueError, match="2\\^21"):
        simplify_mesh(v * 3.0, f, cell_size=1e-6)
    assert simplify_mesh(v, f, cell_size=1.0 / 2 ** 20)[1].shape[0] == 1          # 2^20 + 1 cells along two axes: accepted
    with pytest.raises(ValueError, match="origin"):
        simplify_mesh(v, f, cell_size=0.5, origin=(0.5, 0.0, 0.0))
    with pytest.raises(ValueError, match="placement"):
        simplify_mesh(v, f, cell_size=0.5, placement="median")
    with pytest.raises(ValueError):
        simplify_mesh(v.double(), f, cell_size=0.5)
    with pytest.raises(ValueError):
        simplify_mesh(v, f.float(), cell_size=0.5)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def test_extract_meshes_simplifies_on_request_only(tmp_path, monkeypatch):
    """extract_meshes on CPU tensors with the model and the views replaced by the analytic sphere views of tests/test_mesh_cpu.py:
    simplify_cell=None writes the bytes of extract + filter + write_mesh_ply, as before; a cell writes simplify_mesh of that."""
    from types import SimpleNamespace
    from test_mesh_cpu import fusion_inputs, sphere_box
    from dgs_amd import fit, io as dio, mesh
    from dgs_amd.mesh_simplify import simplify_mesh
    N = 28
    origin, h = sphere_box(N)
    views = fusion_inputs(6, 64)
    lo = np.asarray(origin, dtype=np.float64)
    monkeypatch.setattr(fit, "restore", lambda *a, **k: (None, None))
    monkeypatch.setattr(dio, "load_dnerf", lambda *a, **k: {"train": [SimpleNamespace(camera=None)] * 6, "test": []})
    monkeypatch.setattr(mesh, "views_at_time", lambda surfels, deform, cams, t, bg, **k: views)
    kw = dict(times=[0.5], voxel_size=h, bounds=(lo, lo + h * (N - 1)), iteration=7, device="cpu", min_faces=0)
    plain = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "a"), **kw)
    light = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "b"), simplify_cell=2 * h, **kw)
    vol = mesh.TSDFVolume.from_bounds(*kw["bounds"], h, "cpu").integrate(*views, trunc=5 * h, depth_trunc=6.0)
    v, f, c = mesh.keep_largest_components(*vol.extract(), n_keep=1000, min_faces=0)
    assert f.shape[0] > 1000
    want = str(tmp_path / "want.ply")
    dio.write_mesh_ply(want, v, f, c)
    assert open(plain[0], "rb").read() == open(want, "rb").read()
    sv, sf, sc = simplify_mesh(v, f, c, cell_size=2 * h)
    assert 0 < sf.shape[0] * 4 < f.shape[0]
    dio.write_mesh_ply(want, sv, sf, sc)
    assert open(light[0], "rb").read() == open(want, "rb").read()


def test_simplify_shell(tmp_path):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    from dgs_amd.mesh_simplify import main, simplify_mesh
    v, f, c, h = analytic_mesh("cube")
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    write_mesh_ply(src, v, f, c)
    rv, rf, rc = (torch.from_numpy(np.ascontiguousarray(x)) for x in read_mesh_ply(src))
    for extra, placement in (([], "quadric"), (["--placement", "average"], "average")):
        main([src, dst, "--cell", str(2.5 * h), "--device", "cpu"] + extra)
        sv, sf, sc = simplify_mesh(rv, rf, rc, cell_size=2.5 * h, placement=placement)
        gv, gf, gc = read_mesh_ply(dst)
        assert np.array_equal(gv, sv.numpy()) and np.array_equal(gf, sf.numpy()) and 0 < gf.shape[0] < f.shape[0] // 8
    with open(str(tmp_path / "in.obj"), "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in f.tolist()))
    main([str(tmp_path / "in.obj"), dst, "--cell", str(2.5 * h), "--device", "cpu"])
    assert read_mesh_ply(dst)[1].shape == gf.shape
    with pytest.raises(SystemExit):
        main([src, dst, "--device", "cpu"])                       # --cell is required


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_simplify_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops, mesh_simplify
    lib = _mesh_ops.load()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    acc, solve = lib.dgs_simplify_accumulate, lib.dgs_simplify_solve
    assert acc(-1, p, p, 1, p, p, 1, p, 0.5, p, None) < 0 and b"negative" in err()
    assert acc(1, p, p, -1, p, p, 1, p, 0.5, p, None) < 0 and b"negative" in err()
    assert acc(1, p, p, 1, p, p, -1, p, 0.5, p, None) < 0 and b"negative" in err()
    assert acc(2 ** 31, p, p, 1, p, p, 1, p, 0.5, p, None) < 0 and b"2^31" in err()
    assert acc(1, p, p, 2 ** 31, p, p, 1, p, 0.5, p, None) < 0 and b"2^31" in err()
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert acc(1, p, p, 1, p, p, 1, p, cell, p, None) < 0 and b"cell" in err()
        assert solve(1, p, p, cell, 1, p, p, None) < 0 and b"cell" in err()
    assert acc(1, None, p, 1, p, p, 1, p, 0.5, p, None) < 0 and b"null" in err()
    assert acc(1, p, p, 1, None, p, 1, p, 0.5, p, None) < 0 and b"null" in err()
    assert acc(1, p, p, 1, p, None, 1, p, 0.5, p, None) < 0 and b"null" in err()
    assert acc(1, p, p, 1, p, p, 1, None, 0.5, p, None) < 0 and b"null" in err()
    assert acc(1, p, p, 1, p, p, 1, p, 0.5, None, None) < 0 and b"null" in err()
    assert acc(0, None, None, 0, None, None, 0, None, 0.5, None, None) == 0                # nothing to do: nothing is launched
    assert acc(5, p, None, 3, p, p, 0, None, 0.5, None, None) == 0
    assert solve(-1, p, p, 0.5, 1, p, p, None) < 0 and b"negative" in err()
    assert solve(2 ** 31, p, p, 0.5, 1, p, p, None) < 0 and b"2^31" in err()
    assert solve(1, p, p, 0.5, 2, p, p, None) < 0 and b"placement" in err()
    assert solve(1, None, p, 0.5, 1, p, p, None) < 0 and b"null" in err()
    assert solve(1, p, p, 0.5, 1, None, p, None) < 0 and b"null" in err()
    assert solve(0, None, None, 0.5, 0, None, None, None) == 0
    assert lib.dgs_simplify_layout(None) < 0 and b"null" in err()
    threads, per_thread, q, w_max, lam = _mesh_ops.simplify_layout()
    assert threads % 64 == 0 and per_thread >= 1
    assert (q, w_max, lam) == (mesh_simplify.Q, mesh_simplify.W_MAX, mesh_simplify.LAMBDA_EXP)
    assert w_max * 2 ** q <= 2 ** 28                              # the overflow derivation of include/dgs_mesh_ops.h
    assert {"dgs_simplify_accumulate", "dgs_simplify_solve", "dgs_simplify_layout"} <= set(_mesh_ops.exported_symbols())
