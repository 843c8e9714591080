"""dgs_amd.mesh_decimate on CPU tensors: the statement of include/dgs_mesh_ops.h against independent facts -- closed manifolds stay
closed manifolds of their genus, planes stay planes, creases and corners stay, the selected set of a round is independent, locks
hold, and at an equal face budget the result is not further from the analytic surface than vertex clustering's.  The mesh builders
are shared with tests/test_mesh_decimate_gpu.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch


# ---- meshes (cached: do not modify) ---------------------------------------------------------------------------------------------
def weld(v, f):
    """Merge vertices with equal coordinates after rounding to 1e-6; faces follow."""
    key = np.round(np.asarray(v, dtype=np.float64) * 1e6).astype(np.int64)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return np.asarray(v)[first], inverse.reshape(-1)[np.asarray(f)]


def as_mesh(v, f, seed=0):
    v = torch.tensor(np.asarray(v), dtype=torch.float32)
    c = torch.rand((v.shape[0], 3), generator=torch.Generator().manual_seed(seed))
    return v, torch.tensor(np.asarray(f), dtype=torch.int32), c


@functools.lru_cache(maxsize=None)
def icosphere(levels=3):
    """The unit sphere: an icosahedron subdivided `levels` times (3: 642 vertices, 1 280 faces), outward winding."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return as_mesh(np.stack(v), f, 1)


TORUS_R, TORUS_r = 1.0, 0.4


@functools.lru_cache(maxsize=None)
def torus(n=32, m=16):
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * i / n, 2 * np.pi * j / m
    v = np.stack(((TORUS_R + TORUS_r * np.cos(b)) * np.cos(a), (TORUS_R + TORUS_r * np.cos(b)) * np.sin(a), TORUS_r * np.sin(b)), -1).reshape(-1, 3)
    idx = lambda p, q: (p % n) * m + q % m
    f = [t for p in range(n) for q in range(m) for t in ((idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)), (idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)))]
    return as_mesh(v, f, 2)


def grid_np(n, jitter=0.0, seed=0):
    """An n x n vertex grid over [0, 1]^2 at z = 0, normals +z; interior vertices jittered in the plane."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack((i, j, np.zeros_like(i)), -1).reshape(-1, 3) / (n - 1.0)
    if jitter:
        inner = ((i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)).reshape(-1)
        v[inner, :2] += (np.random.default_rng(seed).random((int(inner.sum()), 2)) - 0.5) * jitter / (n - 1.0)
    idx = lambda p, q: p * n + q
    f = [t for p in range(n - 1) for q in range(n - 1) for t in ((idx(p, q), idx(p + 1, q), idx(p + 1, q + 1)), (idx(p, q), idx(p + 1, q + 1), idx(p, q + 1)))]
    return v, np.array(f)


@functools.lru_cache(maxsize=None)
def flat_grid(n=17):
    return as_mesh(*grid_np(n), 3)


@functools.lru_cache(maxsize=None)
def cube(n=9):
    """[-1/2, 1/2]^3 as six welded grids of (n - 1)^2 cells, outward winding."""
    g, f = grid_np(n)
    g = g - np.array([0.5, 0.5, 0.0])
    vs, fs = [], []
    for axis in range(3):
        for side in (-1, 1):
            p = np.zeros_like(g)
            p[:, axis] = 0.5 * side
            p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = g[:, 0], g[:, 1]
            fs.append((f if side > 0 else f[:, ::-1]) + sum(x.shape[0] for x in vs))
            vs.append(p)
    return as_mesh(*weld(np.concatenate(vs), np.concatenate(fs)), 4)


@functools.lru_cache(maxsize=None)
def random_sheet(n=24, seed=5):
    """A jittered grid, slightly curved, with shuffled vertex ids."""
    v, f = grid_np(n, jitter=0.6, seed=seed)
    v[:, 2] = 0.1 * np.sin(3 * v[:, 0]) * np.cos(2 * v[:, 1])
    perm = np.random.default_rng(seed).permutation(v.shape[0])
    out = np.empty_like(v)
    out[perm] = v
    return as_mesh(out, perm[f], 5)


@functools.lru_cache(maxsize=None)
def glued_sheets(n=9):
    """Three sheets that meet in the line x = 0, z = 0: every edge of that line lies in three faces."""
    g, f = grid_np(n)
    vs, fs = [], []
    for k, ang in enumerate((0.0, 2.0, 4.0)):
        p = np.stack((g[:, 0] * np.cos(ang), g[:, 1], g[:, 0] * np.sin(ang) + 0.02 * np.sin(5 * g[:, 0]) * g[:, 0]), -1)
        fs.append(f + k * g.shape[0])
        vs.append(p)
    return as_mesh(*weld(np.concatenate(vs), np.concatenate(fs)), 6)


@functools.lru_cache(maxsize=None)
def hub(valence=500):
    """A cone: a hub vertex of the given valence over two rings, so that one thread walks a row of `valence` entries."""
    a = 2 * np.pi * np.arange(valence) / valence
    ring = lambda r, z: np.stack((r * np.cos(a), r * np.sin(a), np.full_like(a, z)), -1)
    v = np.concatenate((np.array([[0.0, 0.0, 0.3]]), ring(0.5, 0.15), ring(1.0, 0.0)))
    r1, r2 = 1 + np.arange(valence), 1 + valence + np.arange(valence)
    n1, n2 = np.roll(r1, -1), np.roll(r2, -1)
    f = np.concatenate((np.stack((np.zeros_like(r1), r1, n1), -1), np.stack((r1, r2, n2), -1), np.stack((r1, n2, n1), -1)))
    return as_mesh(v, f, 7)


def shuffled(mesh, seed=11):
    v, f, c = mesh
    perm = torch.randperm(v.shape[0], generator=torch.Generator().manual_seed(seed))
    nv, nc = torch.empty_like(v), torch.empty_like(c)
    nv[perm], nc[perm] = v, c
    return nv, perm[f.long()].to(f.dtype), nc


# ---- facts ----------------------------------------------------------------------------------------------------------------------
def undirected_counts(f):
    f = np.asarray(f, dtype=np.int64)
    e = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    e.sort(1)
    return np.unique(e, axis=0, return_counts=True)


def signed_volume(v, f):
    p = np.asarray(v, dtype=np.float64)[np.asarray(f, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6)


def assert_closed_manifold(v, f, euler):
    from dgs_amd.mesh_clean import component_labels
    fn = f.numpy().astype(np.int64)
    edges, counts = undirected_counts(fn)
    assert (counts == 2).all()                                                              # every undirected edge: two faces
    d = np.concatenate((fn[:, [0, 1]], fn[:, [1, 2]], fn[:, [2, 0]]))
    assert np.unique(d, axis=0).shape[0] == d.shape[0]                                      # every directed edge once
    assert (fn[:, 0] != fn[:, 1]).all() and (fn[:, 1] != fn[:, 2]).all() and (fn[:, 2] != fn[:, 0]).all()
    assert torch.unique(component_labels(f, v.shape[0])).numel() == 1
    assert torch.unique(f).numel() == v.shape[0]
    assert v.shape[0] - edges.shape[0] + fn.shape[0] == euler


def sphere_distance(p):
    return np.abs(np.linalg.norm(p, axis=1) - 1.0)


def torus_distance(p):
    return np.abs(np.hypot(np.hypot(p[:, 0], p[:, 1]) - TORUS_R, p[:, 2]) - TORUS_r)


def surface_rms(v, f, distance):
    p = v.double().numpy()
    cen = p[f.numpy().astype(np.int64)].mean(1)
    return float(np.sqrt(np.mean(distance(np.concatenate((p, cen))) ** 2)))


def diag(v):
    return float((v.amax(0) - v.amin(0)).double().norm())


def bits(x):
    return x.contiguous().view(torch.int32)


# ---- closed manifolds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_closed_manifolds_stay_closed_manifolds(name):
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = icosphere() if name == "sphere" else torus()
    euler = 2 if name == "sphere" else 0
    assert f.shape[0] == (1280 if name == "sphere" else 1024)
    assert_closed_manifold(v, f, euler)
    target = f.shape[0] // 4
    dv, df, dc, vmap = decimate_mesh(v, f, c, ratio=0.25, return_map=True)
    print("%s: %d -> %d faces, %d -> %d vertices" % (name, f.shape[0], df.shape[0], v.shape[0], dv.shape[0]))
    assert dv.dtype == torch.float32 and df.dtype == f.dtype and dc.shape == dv.shape and vmap.dtype == torch.int64
    assert_closed_manifold(dv, df, euler)
    assert signed_volume(v, f) > 0 and signed_volume(dv, df) > 0
    assert df.shape[0] in (target, target - 1)
    assert decimate_mesh(v, f, target_faces=target)[1].shape == df.shape


def test_a_tetrahedron_and_an_octahedron_come_back_unchanged():
    from dgs_amd.mesh_decimate import decimate_mesh
    tet = as_mesh([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])
    oct_ = as_mesh([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
                   [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)])
    for v, f, c in (tet, oct_):
        for target in (0, 1, 2, 3, f.shape[0] - 1, f.shape[0], f.shape[0] + 5):
            dv, df, dc, vmap = decimate_mesh(v, f, c, target_faces=target, return_map=True)
            assert torch.equal(bits(dv), bits(v)) and torch.equal(df, f) and torch.equal(bits(dc), bits(c))
            assert torch.equal(vmap, torch.arange(v.shape[0]))


# ---- planes and creases ---------------------------------------------------------------------------------------------------------
def test_planes_stay_planes():
    from dgs_amd.mesh_decimate import decimate_mesh
    from dgs_amd.mesh_smooth import boundary_vertices
    v, f, c = flat_grid()
    rim = boundary_vertices(v.shape[0], f)
    dv, df, dc, vmap = decimate_mesh(v, f, c, ratio=0.1, return_map=True)
    print("grid, locked rim: %d -> %d faces" % (f.shape[0], df.shape[0]))
    assert df.shape[0] < f.shape[0] // 2
    assert float(dv[:, 2].abs().max()) <= 1e-5 * diag(v)
    assert (vmap[rim] >= 0).all() and torch.equal(bits(dv[vmap[rim]]), bits(v[rim]))       # the rim: every vertex, bit for bit
    assert torch.equal(vmap[rim], torch.sort(vmap[rim]).values)
    normal = lambda v, f: torch.linalg.cross(v[f[:, 1].long()] - v[f[:, 0].long()], v[f[:, 2].long()] - v[f[:, 0].long()])
    assert (normal(dv, df)[:, 2] > 0).all()
    fv, ff, fc = decimate_mesh(v, f, c, ratio=0.1, preserve_boundary=False)
    print("grid, free rim: %d -> %d faces" % (f.shape[0], ff.shape[0]))
    assert ff.shape[0] in (f.shape[0] // 10, f.shape[0] // 10 - 1)
    assert float(fv[:, 2].abs().max()) <= 1e-5 * diag(v)
    assert (normal(fv, ff)[:, 2] > 0).all()
    assert (undirected_counts(ff)[1] <= 2).all()


def test_creases_stay():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = cube()
    assert f.shape[0] == 768 and (undirected_counts(f)[1] == 2).all()
    dv, df, dc = decimate_mesh(v, f, c, ratio=0.1)
    print("cube: %d -> %d faces" % (f.shape[0], df.shape[0]))
    assert df.shape[0] in (76, 75)
    assert_closed_manifold(dv, df, 2)
    a = dv.double().abs().numpy()
    tol = 1e-5 * diag(v)
    outside = np.linalg.norm(np.maximum(a - 0.5, 0.0), axis=1)
    dist = np.where((a <= 0.5).all(1), 0.5 - a.max(1), outside)
    assert dist.max() <= tol
    for corner in np.array([(x, y, z) for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)]):
        assert np.linalg.norm(dv.double().numpy() - corner, axis=1).min() <= tol


# ---- one round ------------------------------------------------------------------------------------------------------------------
def one_round(mesh, ratio=0.5, preserve_boundary=True, oversubscribe=None):
    from dgs_amd import mesh_decimate as md
    v, f, c = mesh
    st, q_bits, scale, centre = md.prepare(v, f, c, preserve_boundary)
    before = st.faces.clone()
    n, out = md.decimate_round(st, int(f.shape[0] * ratio), q_bits, float("inf"), preserve_boundary, oversubscribe)
    return st, before, n, out


def test_the_selected_set_is_independent():
    v, f, c = random_sheet()
    st, before, n, out = one_round((v, f, c), preserve_boundary=False, oversubscribe=1000.0)
    e = out["tab"]["edges"].long()
    sel = out["selected"].nonzero().reshape(-1)
    print("sheet: %d edges, %d valid, %d competing, %d selected" % (e.shape[1], int(out["valid"].sum()), int(out["compete"].sum()), sel.numel()))
    assert sel.numel() > 10 and n == sel.numel()
    assert out["valid"][sel].all() and out["compete"][sel].all()                            # every selected edge passed (c)
    ends = torch.cat((e[0][sel], e[1][sel]))
    assert torch.unique(ends).numel() == ends.numel()                                       # no shared endpoint
    mark = torch.zeros(v.shape[0], dtype=torch.bool)
    mark[ends] = True
    owner = torch.full((v.shape[0],), -1, dtype=torch.int64)
    owner[e[0][sel]] = sel
    owner[e[1][sel]] = sel
    both = mark[e[0]] & mark[e[1]]                                                          # edges between two endpoints: only the selected ones
    assert torch.equal(both.nonzero().reshape(-1), sel)
    # and (c) again, independently: the common neighbours of a selected edge are its opposite vertices
    nb = [set() for _ in range(v.shape[0])]
    for a, b in zip(e[0].tolist(), e[1].tolist()):
        nb[a].add(b), nb[b].add(a)
    for k in sel.tolist():
        a, b, cnt, o0, o1 = e[:, k].tolist()
        assert nb[a] & nb[b] == {o for o in (o0, o1) if o >= 0} and len(nb[a] & nb[b]) == cnt


def test_locks():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = glued_sheets()
    edges, counts = undirected_counts(f)
    seam = torch.tensor(np.unique(edges[counts == 3]))
    assert seam.numel() == 9
    dv, df, dc, vmap = decimate_mesh(v, f, c, ratio=0.2, return_map=True)
    print("glued sheets: %d -> %d faces" % (f.shape[0], df.shape[0]))
    assert df.shape[0] < f.shape[0] // 2
    assert (vmap[seam] >= 0).all() and torch.equal(vmap[seam], torch.sort(vmap[seam]).values) and torch.unique(vmap[seam]).numel() == 9
    assert torch.equal(bits(dv[vmap[seam]]), bits(v[seam])) and torch.equal(bits(dc[vmap[seam]]), bits(c[seam]))
    e2, c2 = undirected_counts(df)
    assert set(map(tuple, vmap[torch.tensor(edges[counts == 3])].tolist())) == set(map(tuple, e2[c2 == 3].tolist()))


def test_awkward_input():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = icosphere(2)
    extra = torch.tensor([[0, 0, 5], [3, 4, 4], [7, 7, 7]], dtype=f.dtype)                  # faces that name a vertex twice
    line = torch.tensor([[0.0, 0, 2], [0, 0, 3], [0, 0, 4], [9, 9, 9]])                     # three collinear vertices and a loose one
    V = v.shape[0]
    av = torch.cat((v, line))
    af = torch.cat((f, f[:5], extra, torch.tensor([[V, V + 1, V + 2]], dtype=f.dtype)))     # + repeats + a face without area
    ac = torch.cat((c, torch.rand((4, 3), generator=torch.Generator().manual_seed(1))))
    dv, df, dc, vmap = decimate_mesh(av, af, ac, ratio=0.5, return_map=True)
    print("awkward: %d -> %d faces" % (af.shape[0], df.shape[0]))
    assert 0 < df.shape[0] < af.shape[0] - 3 and int(df.max()) == dv.shape[0] - 1 and torch.unique(df).numel() == dv.shape[0]
    assert vmap[V + 3] == -1 and (vmap[:V + 3] >= 0).all()
    fn = df.long()
    assert ((fn[:, 0] != fn[:, 1]) & (fn[:, 1] != fn[:, 2]) & (fn[:, 2] != fn[:, 0])).all()


def test_return_map_colours_and_max_error():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = icosphere()
    dv, df, dc, vmap = decimate_mesh(v, f, c, ratio=0.25, return_map=True)
    assert vmap.shape == (v.shape[0],) and (vmap >= 0).all() and torch.unique(vmap).numel() == dv.shape[0]
    # survivors appear in ascending input id; an input vertex lies near the vertex it was merged into (a few input edge lengths)
    first = torch.full((dv.shape[0],), v.shape[0], dtype=torch.int64).scatter_reduce_(0, vmap, torch.arange(v.shape[0]), "amin")
    assert torch.equal(first, torch.sort(first).values)
    assert float((dv[vmap] - v).norm(dim=1).max()) < 0.6
    assert float(dc.min()) >= 0.0 and float(dc.max()) <= 1.0
    # a vertex that nothing was merged into keeps its bits
    mv, mf, mc, mmap = decimate_mesh(v, f, c, ratio=0.9, return_map=True)
    own = (torch.bincount(mmap, minlength=mv.shape[0]) == 1)[mmap]
    assert own.sum() > v.shape[0] // 2 and torch.equal(bits(mv[mmap[own]]), bits(v[own])) and torch.equal(bits(mc[mmap[own]]), bits(c[own]))
    # -1 only for vertices nothing referred to
    lv = torch.cat((v, torch.tensor([[5.0, 5, 5]])))
    assert decimate_mesh(lv, f, None, ratio=0.5, return_map=True)[3].tolist().count(-1) == 1
    # max_error = 0: only edges that cost nothing
    sv, sf, sc = decimate_mesh(v, f, c, ratio=0.25, max_error=0.0)
    assert torch.equal(sf, f) and torch.equal(bits(sv), bits(v))
    gv, gf, gc = flat_grid()
    fv, ff, fc = decimate_mesh(gv, gf, gc, ratio=0.25, max_error=0.0)
    assert ff.shape[0] < gf.shape[0] // 2 and float(fv[:, 2].abs().max()) == 0.0
    some = decimate_mesh(v, f, c, ratio=0.25, max_error=0.02)[1].shape[0]
    assert df.shape[0] < some < f.shape[0]                                                   # a bound between the two stops in between


# ---- against vertex clustering --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_better_than_vertex_clustering_at_equal_budget(name):
    """simplify_mesh at a cell that leaves about a quarter of the faces, decimate_mesh at that face count: the RMS distance of the
    vertices and face centroids to the analytic surface must not be larger.  No margin."""
    from dgs_amd.mesh_decimate import decimate_mesh
    from dgs_amd.mesh_simplify import simplify_mesh
    v, f, c = icosphere() if name == "sphere" else torus()
    distance = sphere_distance if name == "sphere" else torus_distance
    best = None
    for cell in np.linspace(0.15, 0.6, 46):                                                 # the cell whose face count is nearest a quarter
        cf = simplify_mesh(v, f, c, cell_size=float(cell))[1].shape[0]
        if best is None or abs(cf - f.shape[0] / 4) < abs(best[1] - f.shape[0] / 4):
            best = (float(cell), cf)
    cv, cf, cc = simplify_mesh(v, f, c, cell_size=best[0])
    dv, df, dc = decimate_mesh(v, f, c, target_faces=cf.shape[0])
    rms_c, rms_d = surface_rms(cv, cf, distance), surface_rms(dv, df, distance)
    print("%s: clustering at cell %.3f: %d faces, rms %.5f;  decimation: %d faces, rms %.5f" % (name, best[0], cf.shape[0], rms_c, df.shape[0], rms_d))
    assert abs(cf.shape[0] - f.shape[0] / 4) < f.shape[0] / 16
    assert df.shape[0] in (cf.shape[0], cf.shape[0] - 1)
    assert rms_d <= rms_c


# ---- refusals, plumbing, the C ABI ----------------------------------------------------------------------------------------------
def test_errors():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = icosphere(1)
    for kw in ({}, {"target_faces": 10, "ratio": 0.5}, {"ratio": 0.0}, {"ratio": 1.5}, {"ratio": -0.1}, {"ratio": float("nan")},
               {"target_faces": -1}, {"target_faces": 2.5}, {"ratio": 0.5, "max_error": -1.0}, {"ratio": 0.5, "max_rounds": -1}):
        with pytest.raises(ValueError):
            decimate_mesh(v, f, c, **kw)
    bad = v.clone()
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        decimate_mesh(bad, f, ratio=0.5)
    for wrong in (f.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(v.shape[0], dtype=f.dtype)),
                  f.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(-1, dtype=f.dtype))):
        with pytest.raises(ValueError, match="out of range"):
            decimate_mesh(v, wrong, ratio=0.5)
    with pytest.raises(ValueError):
        decimate_mesh(v.double(), f, ratio=0.5)
    with pytest.raises(ValueError):
        decimate_mesh(v, f.float(), ratio=0.5)
    with pytest.raises(ValueError):
        decimate_mesh(v, f, c.double(), ratio=0.5)
    assert decimate_mesh(v, f, c, ratio=1.0)[1].shape == f.shape                            # nothing to do
    assert decimate_mesh(v, f, c, ratio=0.5, max_rounds=0)[1].shape == f.shape
    ev, ef, ec, em = decimate_mesh(v[:0], f[:0], None, ratio=0.5, return_map=True)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec is None and em.shape == (0,)


def test_faces_keep_their_dtype_and_order():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = icosphere(2)
    a, b = decimate_mesh(v, f, c, ratio=0.5, return_map=True), decimate_mesh(v, f.long(), c, ratio=0.5, return_map=True)
    assert a[1].dtype == torch.int32 and b[1].dtype == torch.int64 and torch.equal(a[1].long(), b[1]) and torch.equal(bits(a[0]), bits(b[0]))
    # surviving faces keep their order and winding: every output face is the image of an input face, in input order
    img = a[3][f.long()]
    alive = (img[:, 0] != img[:, 1]) & (img[:, 1] != img[:, 2]) & (img[:, 2] != img[:, 0])
    assert torch.equal(img[alive], a[1].long())


def test_extract_meshes_decimates_on_request_only(tmp_path, monkeypatch):
    """The harness of tests/test_mesh_simplify_cpu.py: extract_meshes on CPU tensors over analytic sphere views.  The defaults write
    what they wrote; decimate_ratio / decimate_faces write decimate_mesh of that, applied after the clustering."""
    from types import SimpleNamespace
    from test_mesh_cpu import fusion_inputs, sphere_box
    from dgs_amd import fit, io as dio, mesh
    from dgs_amd.mesh_decimate import decimate_mesh
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
    vol = mesh.TSDFVolume.from_bounds(*kw["bounds"], h, "cpu").integrate(*views, trunc=5 * h, depth_trunc=6.0)
    v, f, c = mesh.keep_largest_components(*vol.extract(), n_keep=1000, min_faces=0)
    want = str(tmp_path / "want.ply")
    dio.write_mesh_ply(want, v, f, c)
    assert open(plain[0], "rb").read() == open(want, "rb").read()
    light = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "b"), decimate_ratio=0.25, **kw)
    dv, df, dc = decimate_mesh(v, f, c, ratio=0.25)
    assert 0 < df.shape[0] <= f.shape[0] // 4
    dio.write_mesh_ply(want, dv, df, dc)
    assert open(light[0], "rb").read() == open(want, "rb").read()
    both = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "c"), simplify_cell=2 * h, decimate_faces=200, **kw)
    dio.write_mesh_ply(want, *decimate_mesh(*simplify_mesh(v, f, c, cell_size=2 * h), target_faces=200))
    assert open(both[0], "rb").read() == open(want, "rb").read()


def test_decimate_shell(tmp_path):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    from dgs_amd.mesh_decimate import decimate_mesh, main
    v, f, c = flat_grid()
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    write_mesh_ply(src, v, f, c)
    rv, rf, rc = (torch.from_numpy(np.ascontiguousarray(x)) for x in read_mesh_ply(src))
    for extra, kw in ((["--ratio", "0.3"], {"ratio": 0.3}), (["--faces", "100", "--free-boundary"], {"target_faces": 100, "preserve_boundary": False}),
                      (["--ratio", "0.3", "--max-error", "0.0"], {"ratio": 0.3, "max_error": 0.0})):
        main([src, dst, "--device", "cpu"] + extra)
        sv, sf, sc = decimate_mesh(rv, rf, rc, **kw)
        gv, gf, gc = read_mesh_ply(dst)
        assert np.array_equal(gv, sv.numpy()) and np.array_equal(gf, sf.numpy()) and 0 < gf.shape[0] < f.shape[0]
    with open(str(tmp_path / "in.obj"), "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in f.tolist()))
    main([str(tmp_path / "in.obj"), dst, "--ratio", "0.3", "--device", "cpu"])
    assert read_mesh_ply(dst)[1].shape[0] < f.shape[0]
    for bad in ([], ["--ratio", "0.5", "--faces", "10"]):
        with pytest.raises(SystemExit):
            main([src, dst, "--device", "cpu"] + bad)


def test_decimate_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops, mesh_decimate
    lib = _mesh_ops.load()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    big = 2 ** 31
    quad, edges, select, apply_ = lib.dgs_decimate_quadrics, lib.dgs_decimate_edges, lib.dgs_decimate_select, lib.dgs_decimate_apply
    # quadrics(V, pos, F, faces, mean_len, q_bits, rows, stream)
    assert quad(-1, p, 1, p, 1.0, 30, p, None) < 0 and b"negative" in err()
    assert quad(1, p, -1, p, 1.0, 30, p, None) < 0 and b"negative" in err()
    assert quad(big, p, 1, p, 1.0, 30, p, None) < 0 and b"2^31" in err()
    assert quad(1, p, big, p, 1.0, 30, p, None) < 0 and b"2^31" in err()
    assert quad(1, None, 1, p, 1.0, 30, p, None) < 0 and b"null" in err()
    assert quad(1, p, 1, None, 1.0, 30, p, None) < 0 and b"null" in err()
    assert quad(1, p, 1, p, 1.0, 30, None, None) < 0 and b"null" in err()
    assert quad(1, p, 1, p, 0.0, 30, p, None) < 0 and b"mean_len" in err()
    assert quad(1, p, 1, p, 1.0, 41, p, None) < 0 and b"q_bits" in err()
    assert quad(1, p, 2 ** 30, p, 1.0, 30, p, None) < 0 and b"q_bits" in err()             # 2^30 faces at Q = 30: the sums could overflow
    assert quad(0, None, 0, None, 1.0, 30, None, None) == 0
    # edges(V, pos, rows, flags, F, faces, E, edges, adj_offsets, adj, n_adj, vf_offsets, vf, n_vf, q_bits, max_cost, cost, place, valid, stream)
    ok = [4, p, p, p, 2, p, 5, p, p, p, 10, p, p, 6, 30, 1.0, p, p, p, None]
    for at, what in ((0, b"negative"), (4, b"negative"), (6, b"negative"), (10, b"negative"), (13, b"negative")):
        a = list(ok)
        a[at] = -1
        assert edges(*a) < 0 and what in err()
    for at in (0, 4, 6, 10, 13):
        a = list(ok)
        a[at] = big
        assert edges(*a) < 0 and b"2^31" in err()
    for at in (1, 2, 3, 5, 7, 8, 9, 11, 12, 16, 17, 18):
        a = list(ok)
        a[at] = None
        assert edges(*a) < 0 and b"null" in err()
    a = list(ok)
    a[14] = 99
    assert edges(*a) < 0 and b"q_bits" in err()
    a = list(ok)
    a[15] = float("nan")
    assert edges(*a) < 0 and b"max_cost" in err()
    a = list(ok)
    a[6] = 0
    assert edges(*a) == 0                                                                    # no edges: nothing is launched
    # select(V, E, edges, cost, compete, m1, m2, selected, stream)
    ok = [4, 5, p, p, p, p, p, p, None]
    for at in (0, 1):
        a = list(ok)
        a[at] = -1
        assert select(*a) < 0 and b"negative" in err()
        a[at] = big
        assert select(*a) < 0 and b"2^31" in err()
    for at in range(2, 8):
        a = list(ok)
        a[at] = None
        assert select(*a) < 0 and b"null" in err()
    assert select(0, 0, None, None, None, None, None, None, None) == 0
    # apply(V, pos, rows, colors, flags, moved, vmap, E, edges, place, n_sel, sel, F, faces, keep, stream)
    ok = [4, p, p, p, p, p, p, 5, p, p, 1, p, 2, p, p, None]
    for at in (0, 7, 10, 12):
        a = list(ok)
        a[at] = -1
        assert apply_(*a) < 0 and b"negative" in err()
        a[at] = big
        assert apply_(*a) < 0 and b"2^31" in err()
    for at in (1, 2, 4, 5, 6, 8, 9, 11, 13, 14):
        a = list(ok)
        a[at] = None
        assert apply_(*a) < 0 and b"null" in err()
    assert apply_(0, None, None, None, None, None, None, 0, None, None, 0, None, 0, None, None, None) == 0
    assert lib.dgs_decimate_layout(None) < 0 and b"null" in err()
    lay = _mesh_ops.decimate_layout()
    assert lay[0] % 64 == 0 and lay[1] >= 1
    assert lay[2:] == (mesh_decimate.Q_MAX, mesh_decimate.Q_BUDGET, mesh_decimate.W_MAX, mesh_decimate.LAMBDA_EXP, mesh_decimate.MIN_VALENCE,
                       mesh_decimate.LEN_BITS)
    assert mesh_decimate.quadric_bits(1) == 40 and mesh_decimate.quadric_bits(2 ** 19) == 40 and mesh_decimate.quadric_bits(2 ** 19 + 1) == 39
    assert mesh_decimate.quadric_bits(2 ** 31 - 1) == 28
    # the overflow derivation of include/dgs_mesh_ops.h: 3 corners * F faces * (3.02 * 2^Q + 1/2) stays below 2^63
    for n in (1, 1000, 2 ** 19, 2 ** 19 + 1, 10 ** 6, 2 ** 31 - 1):
        assert 3 * n * (3.02 * 2 ** mesh_decimate.quadric_bits(n) + 0.5) * 1.001 < 2 ** 63
    assert {"dgs_decimate_quadrics", "dgs_decimate_edges", "dgs_decimate_select", "dgs_decimate_apply", "dgs_decimate_layout"} <= set(_mesh_ops.exported_symbols())
