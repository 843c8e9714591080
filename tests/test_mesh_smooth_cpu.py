"""dgs_amd.mesh_smooth on CPU tensors: the statement of include/dgs_mesh_ops.h against independent facts -- the adjacency against a
brute-force set construction, steps written out by hand, noise taken off a sphere without shrinking it (taubin) and with (laplacian,
simple), a cube's edges, pinning, a float64 run of the same steps, refusals, and the plumbing through extract_meshes and the shell
(no device needed).  The mesh builders are shared with tests/test_mesh_smooth_gpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_mesh_simplify_cpu import analytic_mesh, cube_surface_distance, same_bits


# ---- meshes and references --------------------------------------------------------------------------------------------------------
def sheet(m):
    """An m x m sheet of integer points (x, y, 0), two triangles per square -> (v f32 [m*m,3], f int32 [2(m-1)^2,3])."""
    ij = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    v = np.concatenate((ij, np.zeros((m * m, 1))), 1).astype(np.float32)
    q = (np.arange(m - 1)[:, None] * m + np.arange(m - 1)[None, :]).reshape(-1)
    f = np.concatenate((np.stack((q, q + m, q + m + 1), 1), np.stack((q, q + m + 1, q + 1), 1))).astype(np.int32)
    return torch.from_numpy(v), torch.from_numpy(f)


def brute_adjacency(V, faces):
    """Rows as sorted Python lists, by sets."""
    rows = [set() for _ in range(V)]
    for tri in np.asarray(faces).tolist():
        for a in tri:
            for b in tri:
                if a != b:
                    rows[a].add(b)
    return [sorted(r) for r in rows]


def rows_of(offsets, neighbours):
    o, n = offsets.tolist(), neighbours.tolist()
    return [n[o[i]:o[i + 1]] for i in range(len(o) - 1)]


HAND_V = 7
HAND_F = [[0, 1, 2], [0, 1, 2], [2, 1, 0], [2, 3, 3], [4, 4, 4], [5, 2, 1]]      # repeats, a vertex named twice and thrice; 6 is isolated


@functools.lru_cache(maxsize=None)
def noisy_sphere():
    """(v, f, c, h, noisy v): the analytic sphere with its vertices displaced along their normals by uniform noise of amplitude
    0.25 h.  Cached: do not modify."""
    v, f, c, h = analytic_mesh("sphere")
    g = torch.Generator().manual_seed(11)
    n = v / v.norm(dim=1, keepdim=True)
    return v, f, c, h, v + n * ((torch.rand(v.shape[0], generator=g) * 2 - 1) * (0.25 * h))[:, None]


def radii(p):
    r = p.double().norm(dim=1)
    return float(r.mean()), float(r.std())


# ---- adjacency and boundary ---------------------------------------------------------------------------------------------------------
def test_adjacency_against_sets():
    from dgs_amd.mesh_smooth import vertex_adjacency
    for dtype in (torch.int32, torch.int64):
        off, nb = vertex_adjacency(HAND_V, torch.tensor(HAND_F, dtype=dtype))
        assert off.dtype == torch.int64 and nb.dtype == torch.int32 and off.shape == (HAND_V + 1,)
        assert rows_of(off, nb) == [[1, 2], [0, 2, 5], [0, 1, 3, 5], [2], [], [1, 2], []] == brute_adjacency(HAND_V, HAND_F)
    v, f, _, _ = analytic_mesh("sphere")
    off, nb = vertex_adjacency(v.shape[0], f)
    assert rows_of(off, nb) == brute_adjacency(v.shape[0], f)
    d = off[1:] - off[:-1]
    print("sphere: %d vertices, %d faces, degrees %d..%d" % (v.shape[0], f.shape[0], int(d.min()), int(d.max())))
    assert (int(d.min()), int(d.max())) == (4, 10) and int(off[-1]) == nb.numel() == 2 * (f.shape[0] * 3 // 2)
    off, nb = vertex_adjacency(3, torch.zeros((0, 3), dtype=torch.int32))
    assert off.tolist() == [0, 0, 0, 0] and nb.shape == (0,)
    off, nb = vertex_adjacency(0, torch.zeros((0, 3), dtype=torch.int64))
    assert off.tolist() == [0] and nb.shape == (0,)


def test_boundary():
    from dgs_amd.mesh_smooth import boundary_vertices
    v, f, _, _ = analytic_mesh("sphere")
    b = boundary_vertices(v.shape[0], f)
    assert b.dtype == torch.bool and b.shape == (v.shape[0],) and not b.any()
    m = 12
    sv, sf = sheet(m)
    b = boundary_vertices(m * m, sf)
    assert int(b.sum()) == 4 * m - 4 == 44
    rim = ((sv[:, :2] == 0) | (sv[:, :2] == m - 1)).any(1)
    assert torch.equal(b, rim)
    # the edges of the thrice repeated face lie in three faces, the edge 2 - 3 of the face (2, 3, 3) in that face twice; only 5 - 2 and
    # 1 - 5 of the last face lie in one
    assert boundary_vertices(HAND_V, torch.tensor(HAND_F)).tolist() == [False, True, True, False, False, True, False]


# ---- steps by hand ------------------------------------------------------------------------------------------------------------------
def test_one_step_by_hand():
    """A tetrahedron with small-integer coordinates, every vertex next to the other three.
    laplacian, s = 0.5: out = x + 0.5 * (sum of the others / 3 - x); the sums are multiples of 3, so every number is exact.
    simple: out = (x + sum of the others) / 4 = the centroid, for every vertex."""
    from dgs_amd.mesh_smooth import smooth_mesh
    v = torch.tensor([[0.0, 0.0, 0.0], [12.0, 0.0, 0.0], [0.0, 24.0, 0.0], [0.0, 0.0, 36.0]])
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)
    got = smooth_mesh(v, f, method="laplacian", iterations=1, lam=0.5)
    assert got[0].tolist() == [[2.0, 4.0, 6.0], [6.0, 4.0, 6.0], [2.0, 12.0, 6.0], [2.0, 4.0, 18.0]]
    assert got[1] is not f and torch.equal(got[1], f) and got[2] is None
    got = smooth_mesh(v, f, method="simple", iterations=1)
    assert got[0].tolist() == [[3.0, 6.0, 9.0]] * 4
    # taubin x 1 with mu = -1: the step above, then out = x + (-1) * (mean of the others - x).  The sums are integers (exact in any
    # order); the division by 3 and the three operations after it are single fp32 roundings, spelled out here
    x = torch.tensor([[2.0, 4.0, 6.0], [6.0, 4.0, 6.0], [2.0, 12.0, 6.0], [2.0, 4.0, 18.0]])
    mean = (x.sum(0) - x) / torch.tensor([3.0])
    got = smooth_mesh(v, f, method="taubin", iterations=1, lam=0.5, mu=-1.0)
    same_bits((got[0],), (x + torch.tensor([-1.0]) * (mean - x),))
    assert got[0][0].tolist() == [float(np.float32(2) - (np.float32(10) / np.float32(3) - np.float32(2))), float(np.float32(4) - (np.float32(20) / np.float32(3) - np.float32(4))), 2.0]
    # a path 0 - 1 - 2 from two faces that name a vertex twice: (0, 1, 1) is the edge 0 - 1, (1, 2, 2) the edge 1 - 2
    pv = torch.tensor([[0.0, 0.0, 0.0], [8.0, 0.0, 0.0], [8.0, 16.0, 0.0]])
    pf = torch.tensor([[0, 1, 1], [1, 2, 2]])
    got = smooth_mesh(pv, pf, method="laplacian", iterations=1, lam=0.25)[0]
    assert got.tolist() == [[2.0, 0.0, 0.0], [7.0, 2.0, 0.0], [8.0, 12.0, 0.0]]
    got = smooth_mesh(pv, pf, method="simple", iterations=1)[0]
    third = float(np.float32(16.0) / np.float32(3.0))                                               # one IEEE fp32 division
    assert got.tolist() == [[4.0, 0.0, 0.0], [third, third, 0.0], [8.0, 8.0, 0.0]]


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_noise_on_a_sphere():
    """Conditions on the statement: taubin halves the noise and keeps the radius, laplacian and simple shrink.  Measured: see the
    prints (std of |p| 9.6e-3 noisy)."""
    from dgs_amd.mesh_smooth import smooth_mesh
    v, f, c, h, noisy = noisy_sphere()
    mean0, std0 = radii(noisy)
    print("noisy: mean radius %.6f, std %.3e (h = %.4f)" % (mean0, std0, h))
    assert 9.0e-3 < std0 < 10.2e-3
    out = {}
    for method in ("taubin", "laplacian", "simple"):
        p = smooth_mesh(noisy, f, method=method, iterations=10)[0]
        out[method] = radii(p)
        print("%s x 10: mean radius %.6f (%+.2e), std %.3e" % (method, out[method][0], out[method][0] - mean0, out[method][1]))
    assert out["taubin"][1] <= 0.5 * std0
    assert abs(out["taubin"][0] - mean0) < 1e-3
    assert mean0 - out["laplacian"][0] > 3e-3
    assert mean0 - out["simple"][0] > 5e-3


def test_a_cubes_edges():
    from dgs_amd.mesh_smooth import smooth_mesh
    v, f, c, h = analytic_mesh("cube")
    worst = {m: float(cube_surface_distance(smooth_mesh(v, f, method=m, iterations=10)[0].numpy()).max()) for m in ("taubin", "laplacian")}
    print("cube: max distance to the surface %s" % worst)
    assert worst["taubin"] < 0.01
    assert worst["laplacian"] > 0.02


def test_pinning():
    from dgs_amd.mesh_smooth import boundary_vertices, smooth_mesh
    m = 12
    v, f = sheet(m)
    extent = lambda p: float((p[:, :2].amax(0) - p[:, :2].amin(0)).max())
    held = smooth_mesh(v, f, method="laplacian", iterations=10, pin_boundary=True)[0]
    same_bits((held,), (v,))                                   # the rim is held and every inner vertex is the mean of its neighbours
    assert extent(held) == 11.0
    free = smooth_mesh(v, f, method="laplacian", iterations=10)[0]
    print("sheet: extent %.3f unpinned" % extent(free))
    assert extent(free) < 9.5
    mask = torch.zeros(m * m, dtype=torch.bool)
    mask[::5] = True
    got = smooth_mesh(v, f, method="laplacian", iterations=3, pinned=mask)[0]
    moved = (got != v).any(1)
    rim = boundary_vertices(m * m, f)
    assert not moved[mask].any() and moved[rim & ~mask].all() and moved.any()
    both = smooth_mesh(v, f, method="taubin", iterations=3, pinned=mask, pin_boundary=True)[0]
    assert not (both != v).any(1)[mask | rim].any()


def test_against_float64():
    """The same steps in float64 with the factor taken as its fp32 value.  Per step and vertex the fp32 run rounds at most
    max degree additions, a division, a subtraction, a product and an addition, each by at most 2^-24 of a number no larger than
    max |x| (a convex combination, or 1.53 times one at most under taubin); the step's own map has norm <= 1 + 2 |s| <= 2.06 at
    most and 1 for a smoothing step -- the bound of the issue: n_steps * (max degree + 4) * 2^-24 * max |x|."""
    from dgs_amd.mesh_smooth import MODE_LAPLACIAN, smooth_mesh, smooth_steps_torch, vertex_adjacency
    v, f, c, h, noisy = noisy_sphere()
    off, nb = vertex_adjacency(v.shape[0], f)
    factors = [0.5, -0.53] * 10
    ref = smooth_steps_torch(off, nb, noisy.double(), MODE_LAPLACIAN, factors)
    assert ref.dtype == torch.float64
    got = smooth_mesh(noisy, f, method="taubin", iterations=10)[0]
    err = float((got.double() - ref).abs().max())
    bound = len(factors) * (int((off[1:] - off[:-1]).max()) + 4) * 2.0 ** -24 * float(noisy.abs().max())
    print("fp32 against fp64 after %d steps: %.3e (bound %.3e)" % (len(factors), err, bound))
    assert err <= bound


# ---- plumbing -----------------------------------------------------------------------------------------------------------------------
def test_zero_iterations_and_colours():
    from dgs_amd.mesh_smooth import smooth_mesh
    v, f, c, h = analytic_mesh("cube")
    for method in ("simple", "laplacian", "taubin"):
        got = smooth_mesh(v, f, c, method=method, iterations=0, smooth_colors=True)
        same_bits(got, (v, f, c))
        assert got[0] is not v
    got = smooth_mesh(v, f.long(), c, iterations=2)
    same_bits(got[1:], (f.long(), c))                          # faces and colours as given
    assert not torch.equal(got[0], v)
    rough = (c + torch.rand(c.shape, generator=torch.Generator().manual_seed(2)) - 0.5)
    sm = smooth_mesh(v, f, rough, iterations=2, smooth_colors=True)
    same_bits((sm[0],), (got[0],))                             # the position channels do not see the colour channels
    assert float(sm[2].min()) >= 0.0 and float(sm[2].max()) <= 1.0
    assert float((sm[2] - c).abs().mean()) < float((rough.clamp(0, 1) - c).abs().mean())
    e3, ef = torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)
    assert [tuple(x.shape) for x in smooth_mesh(e3, ef, e3)] == [(0, 3)] * 3
    lone = smooth_mesh(v[:5], ef, iterations=3)                # no faces: nobody has a neighbour
    same_bits((lone[0],), (v[:5],))


def test_refusals():
    from dgs_amd.mesh_smooth import boundary_vertices, smooth_mesh, vertex_adjacency
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="method"):
        smooth_mesh(v, f, method="cotangent")
    for it in (-1, 2.0, 1.5, None, True, "3"):
        with pytest.raises(ValueError, match="iterations"):
            smooth_mesh(v, f, iterations=it)
    for bad in (float("nan"), float("inf"), -float("inf"), 1e60, None, "x"):
        with pytest.raises(ValueError, match="lam"):
            smooth_mesh(v, f, lam=bad)
        with pytest.raises(ValueError, match="mu"):
            smooth_mesh(v, f, mu=bad)
    with pytest.raises(ValueError, match="fp32"):
        smooth_mesh(v.double(), f)
    for bad in (float("nan"), float("inf")):
        w = v.clone()
        w[1, 2] = bad
        with pytest.raises(ValueError, match="non-finite"):
            smooth_mesh(w, f)
    for mask in (torch.zeros(4, dtype=torch.bool), torch.zeros(3, dtype=torch.uint8), torch.zeros((3, 1), dtype=torch.bool), [False] * 3):
        with pytest.raises(ValueError, match="pinned"):
            smooth_mesh(v, f, pinned=mask)
    for idx in (3, -1):
        bad_f = torch.tensor([[0, 1, idx]], dtype=torch.int32)
        for call in (lambda: smooth_mesh(v, bad_f), lambda: smooth_mesh(v, bad_f, iterations=0), lambda: vertex_adjacency(3, bad_f),
                     lambda: boundary_vertices(3, bad_f)):
            with pytest.raises(ValueError, match="out of range"):
                call()
    with pytest.raises(ValueError, match="out of range"):
        smooth_mesh(v[:0], f)
    with pytest.raises(ValueError):
        smooth_mesh(v, f.float())
    with pytest.raises(ValueError, match="smooth_colors"):
        smooth_mesh(v, f, smooth_colors=True)


def test_smooth_arguments_are_validated_before_any_launch():
    """Bad arguments are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fac = lambda *s: ctypes.cast((ctypes.c_float * len(s))(*s), ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    steps = lib.dgs_smooth_steps
    threads, per_group, max_c, max_steps = _mesh_ops.smooth_layout()
    assert threads % 64 == 0 and per_group >= 1 and max_c == 8 and max_steps >= 64 and max_steps % 2 == 0
    ok = fac(0.5, -0.53)
    assert steps(-1, p, p, 1, 3, 0, ok, 2, None, p, p, None) < 0 and b"negative" in err()
    assert steps(1, p, p, -1, 3, 0, ok, 2, None, p, p, None) < 0 and b"negative" in err()
    assert steps(1, p, p, 1, 3, 0, ok, -1, None, p, p, None) < 0 and b"negative" in err()
    assert steps(2 ** 31, p, p, 1, 3, 0, ok, 2, None, p, p, None) < 0 and b"2^31" in err()
    assert steps(1, p, p, 2 ** 31, 3, 0, ok, 2, None, p, p, None) < 0 and b"2^31" in err()
    for C in (0, -1, max_c + 1):
        assert steps(1, p, p, 1, C, 0, ok, 2, None, p, p, None) < 0 and b"C must" in err()
    for mode in (-1, 2):
        assert steps(1, p, p, 1, 3, mode, ok, 2, None, p, p, None) < 0 and b"mode" in err()
    many = fac(*([0.5] * (max_steps + 1)))
    assert steps(1, p, p, 1, 3, 0, many, max_steps + 1, None, p, p, None) < 0 and b"n_steps" in err()
    assert steps(1, None, p, 1, 3, 0, ok, 2, None, p, p, None) < 0 and b"null" in err()
    assert steps(1, p, None, 1, 3, 0, ok, 2, None, p, p, None) < 0 and b"null" in err()
    assert steps(1, p, p, 1, 3, 0, None, 2, None, p, p, None) < 0 and b"null" in err()
    assert steps(1, p, p, 1, 3, 0, ok, 2, None, None, p, None) < 0 and b"null" in err()
    assert steps(1, p, p, 1, 3, 0, ok, 2, None, p, None, None) < 0 and b"null" in err()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert steps(1, p, p, 1, 3, 0, fac(0.5, bad), 2, None, p, p, None) < 0 and b"finite" in err()
        assert steps(1, p, p, 1, 3, 1, fac(bad), 1, None, p, p, None) < 0 and b"finite" in err()
    assert steps(0, None, None, 0, 3, 0, ok, 2, None, None, None, None) == 0            # nothing to do: nothing is launched
    assert steps(5, p, p, 7, 3, 0, None, 0, None, p, p, None) == 0
    assert lib.dgs_smooth_layout(None) < 0 and b"null" in err()
    assert {"dgs_smooth_steps", "dgs_smooth_layout"} <= set(_mesh_ops.exported_symbols())


def test_extract_meshes_smooths_on_request_only(tmp_path, monkeypatch):
    """The recipe of tests/test_mesh_simplify_cpu.py: extract_meshes on CPU tensors with the model and the views replaced by the
    analytic sphere views.  smooth_iterations=None calls nothing and writes the bytes of extract + filter; a number smooths the
    filtered mesh, and before the simplification when both are asked for."""
    from types import SimpleNamespace
    from test_mesh_cpu import fusion_inputs, sphere_box
    from dgs_amd import fit, io as dio, mesh, mesh_simplify, mesh_smooth
    N = 28
    origin, h = sphere_box(N)
    views = fusion_inputs(6, 64)
    lo = np.asarray(origin, dtype=np.float64)
    monkeypatch.setattr(fit, "restore", lambda *a, **k: (None, None))
    monkeypatch.setattr(dio, "load_dnerf", lambda *a, **k: {"train": [SimpleNamespace(camera=None)] * 6, "test": []})
    monkeypatch.setattr(mesh, "views_at_time", lambda surfels, deform, cams, t, bg, **k: views)
    calls = []
    real_smooth, real_simplify = mesh_smooth.smooth_mesh, mesh_simplify.simplify_mesh

    def smooth(v, f, c=None, **kw):
        calls.append(("smooth", kw))
        return real_smooth(v, f, c, **kw)

    def simplify(v, f, c=None, **kw):
        calls.append(("simplify", kw))
        return real_simplify(v, f, c, **kw)

    monkeypatch.setattr(mesh_smooth, "smooth_mesh", smooth)
    monkeypatch.setattr(mesh_simplify, "simplify_mesh", simplify)
    kw = dict(times=[0.5], voxel_size=h, bounds=(lo, lo + h * (N - 1)), iteration=7, device="cpu", min_faces=0)
    plain = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "a"), **kw)
    assert calls == []
    vol = mesh.TSDFVolume.from_bounds(*kw["bounds"], h, "cpu").integrate(*views, trunc=5 * h, depth_trunc=6.0)
    v, f, c = mesh.keep_largest_components(*vol.extract(), n_keep=1000, min_faces=0)
    want = str(tmp_path / "want.ply")
    dio.write_mesh_ply(want, v, f, c)
    assert open(plain[0], "rb").read() == open(want, "rb").read()
    smooth_only = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "b"), smooth_iterations=3, **kw)
    assert calls == [("smooth", {"method": "taubin", "iterations": 3})]
    sv, sf, sc = real_smooth(v, f, c, iterations=3)
    assert not torch.equal(sv, v)
    dio.write_mesh_ply(want, sv, sf, sc)
    assert open(smooth_only[0], "rb").read() == open(want, "rb").read()
    del calls[:]
    both = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "c"), smooth_iterations=2, smooth_method="laplacian",
                               simplify_cell=2 * h, **kw)
    assert calls == [("smooth", {"method": "laplacian", "iterations": 2}), ("simplify", {"cell_size": 2 * h})]
    dio.write_mesh_ply(want, *real_simplify(*real_smooth(v, f, c, method="laplacian", iterations=2), cell_size=2 * h))
    assert open(both[0], "rb").read() == open(want, "rb").read()


def test_smooth_shell(tmp_path):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    from dgs_amd.mesh_smooth import main, smooth_mesh
    v, f = sheet(6)
    v = v + torch.rand(v.shape, generator=torch.Generator().manual_seed(4)) * 0.25
    c = torch.rand(v.shape, generator=torch.Generator().manual_seed(5))
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    write_mesh_ply(src, v, f, c)
    rv, rf, rc = (torch.from_numpy(np.ascontiguousarray(x)) for x in read_mesh_ply(src))
    for extra, kw in (([], {}), (["--method", "laplacian", "--iterations", "3", "--lam", "0.25", "--pin-boundary"],
                                 dict(method="laplacian", iterations=3, lam=0.25, pin_boundary=True)),
                      (["--method", "simple", "--iterations", "2"], dict(method="simple", iterations=2)),
                      (["--mu", "-0.6", "--iterations", "1"], dict(mu=-0.6, iterations=1))):
        main([src, dst, "--device", "cpu"] + extra)
        sv, sf, sc = smooth_mesh(rv, rf, rc, **kw)
        gv, gf, gc = read_mesh_ply(dst)
        assert np.array_equal(gv, sv.numpy()) and np.array_equal(gf, sf.numpy()) and not np.array_equal(gv, rv.numpy())
    with open(str(tmp_path / "in.obj"), "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in f.tolist()))
    main([str(tmp_path / "in.obj"), dst, "--device", "cpu"])
    assert read_mesh_ply(dst)[1].shape == gf.shape
    with pytest.raises(SystemExit):
        main([src, dst, "--method", "cotangent"])
