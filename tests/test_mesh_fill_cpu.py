"""dgs_amd.mesh_fill on CPU tensors (the PyTorch statement): boundary loops against a plain Python walk, the fill of a punched torus,
regular polygons, a sweep of staircase-rimmed holes in a planar grid, and the plumbing through clean_mesh, extract_meshes, the
shell and the C ABI's refusals (no device needed).  The mesh builders are shared with tests/test_mesh_fill_gpu.py."""
import ctypes
from collections import Counter, defaultdict

import numpy as np
import pytest
import torch

NU, NW = 96, 48                                                  # the torus grid
# (first quad column, first quad row, columns, rows, one more triangle beside the block) -> a hole of 2 (columns + rows) + extra edges
TORUS_BLOCKS = ((2, 2, 20, 8, 1), (32, 2, 4, 4, 0), (40, 2, 2, 3, 0), (46, 2, 2, 2, 1), (52, 2, 1, 2, 1), (57, 2, 1, 1, 0))
TORUS_TRIANGLE = (62, 2)                                         # a single face: the hole of 3
TORUS_HOLES = [57, 16, 10, 9, 7, 4, 3]


def bits(x):
    return x.contiguous().view(torch.int32)


def compact(v, f, c=None):
    from dgs_amd.mesh_clean import _compact
    return _compact(v, f, c, torch.ones(f.shape[0], dtype=torch.bool))


def grid_faces(nu, nw, wrap):
    """Two faces per quad of an nu x nw vertex grid (wrap: a torus): [quads, 2, 3]; quad (i, j) at index i * rows + j."""
    cu, cw = (nu, nw) if wrap else (nu - 1, nw - 1)
    i, j = np.meshgrid(np.arange(cu), np.arange(cw), indexing="ij")
    idx = lambda a, b: (a % nu) * nw + (b % nw)
    v00, v10, v11, v01 = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
    return np.stack((np.stack((v00, v10, v11), -1), np.stack((v00, v11, v01), -1)), 2).reshape(cu * cw, 2, 3), cw


def punched_torus(colors=True):
    """A 96 x 48 torus with the holes of TORUS_HOLES (edges), unreferenced vertices dropped -> (v, f int64, c)."""
    u, w = np.meshgrid(np.arange(NU) * 2 * np.pi / NU, np.arange(NW) * 2 * np.pi / NW, indexing="ij")
    v = np.stack(((2 + 0.7 * np.cos(w)) * np.cos(u), (2 + 0.7 * np.cos(w)) * np.sin(u), 0.7 * np.sin(w)), -1).reshape(-1, 3).astype(np.float32)
    quads, rows = grid_faces(NU, NW, True)
    keep = np.ones((quads.shape[0], 2), dtype=bool)
    for u0, w0, a, b, extra in TORUS_BLOCKS:
        for i in range(u0, u0 + a):
            keep[i * rows + w0:i * rows + w0 + b] = False
        if extra:
            keep[(u0 + a) * rows + w0 + b - 1, 1] = False        # the face (v00, v11, v01) right of the block's last row shares its left edge with it
    keep[TORUS_TRIANGLE[0] * rows + TORUS_TRIANGLE[1], 0] = False
    vt = torch.from_numpy(v)
    c = (0.5 + 0.5 * torch.sin(vt * 3.0)).contiguous() if colors else None
    return compact(vt, torch.from_numpy(quads[keep]), c)


def annulus(n, inner=1.0, outer=2.0):
    """A regular n-gon hole in a planar fan: n inner and 2 n outer vertices, 3 n faces, normal +z -> (v, f int64)."""
    ai, ao = np.arange(n) * 2 * np.pi / n, np.arange(2 * n) * np.pi / n
    v = np.concatenate((inner * np.stack((np.cos(ai), np.sin(ai), 0 * ai), -1), outer * np.stack((np.cos(ao), np.sin(ao), 0 * ao), -1))).astype(np.float32)
    f = []
    for i in range(n):
        o0, o1, o2, i1 = n + 2 * i, n + (2 * i + 1) % (2 * n), n + (2 * i + 2) % (2 * n), (i + 1) % n
        f += [(i, o0, o1), (i, o1, i1), (i1, o1, o2)]
    return torch.from_numpy(v), torch.tensor(f, dtype=torch.int64)


def jagged_hole(k, n=48):
    """Hole k of 40 in an n x n planar grid (z = 0, normal +z): the quads whose centre lies within r of a jittered centre are
    removed -- the staircase rim a voxel mesh has; r sweeps 1 .. 14.3, rims of 8 to 116 edges.  -> (v, f int64)."""
    g = np.random.default_rng(1000 + k)
    r = 1.0 + 13.3 * k / 39.0
    cx, cy = (n - 1) / 2 + g.uniform(-3, 3, 2)
    quads, rows = grid_faces(n, n, False)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    gone = ((i + 0.5 - cx) ** 2 + (j + 0.5 - cy) ** 2 <= r * r).reshape(-1)
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack((x, y, 0 * x), -1).reshape(-1, 3).astype(np.float32)
    return compact(torch.from_numpy(v), torch.from_numpy(quads[~gone].reshape(-1, 3)))[:2]


def walk_loops(faces):
    """The definition, walked: -> list of rims (lists of vertex ids) in hole order, each from its smallest id, ordered by it."""
    half = [(t[c], t[(c + 1) % 3]) for t in faces if len(set(t)) == 3 for c in range(3)]
    count = Counter((min(a, b), max(a, b)) for a, b in half)
    out, inn = defaultdict(list), Counter()
    for a, b in half:
        if count[(min(a, b), max(a, b))] == 1:
            out[a].append(b)
            inn[b] += 1
    simple = lambda x: len(out[x]) == 1 and inn[x] == 1
    seen, loops = set(), []
    for start in sorted(x for x in list(out) if simple(x)):
        if start in seen:
            continue
        path, cur, closed = [], start, False
        while simple(cur) and cur not in seen:
            path.append(cur)
            seen.add(cur)
            cur = out[cur][0]
            if cur == start:
                closed = True
                break
        if closed and len(path) >= 3:
            loops.append([path[0]] + path[:0:-1])                # the reverse of the boundary direction
    return loops


def loops_of(V, f, **kw):
    from dgs_amd.mesh_fill import boundary_loops
    lv, off = boundary_loops(V, f, **kw)
    assert lv.dtype == torch.int32 and off.dtype == torch.int64 and off[0] == 0 and off[-1] == lv.shape[0]
    return [lv[a:b].tolist() for a, b in zip(off[:-1].tolist(), off[1:].tolist())]


def euler(f):
    f = f.long()
    e = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])).sort(1).values
    return int(torch.unique(f).numel()) - int(torch.unique(e, dim=0).shape[0]) + f.shape[0]


def fill_normals(v, f, n_old_faces):
    p = v[f[n_old_faces:].long()].double()
    return torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


@pytest.fixture(scope="module")
def torus():
    return punched_torus()


# ---- loops --------------------------------------------------------------------------------------------------------------------------
def test_loops_of_the_torus_match_the_walk(torus):
    v, f, c = torus
    V = v.shape[0]
    want = walk_loops(f.tolist())
    assert sorted(len(r) for r in want) == sorted(TORUS_HOLES)
    assert loops_of(V, f) == want == loops_of(V, f.to(torch.int32))
    assert loops_of(V, f, max_edges=16) == [r for r in want if len(r) <= 16]
    assert loops_of(V, f, max_edges=2) == []
    g = torch.Generator().manual_seed(5)
    for perm in (torch.arange(V - 1, -1, -1), torch.randperm(V, generator=g)):          # reversed and permuted ids
        pf = perm[f]
        assert loops_of(V, pf) == walk_loops(pf.tolist())
    # faces that name a vertex twice take no part, wherever they sit
    junk = torch.tensor([[5, 5, 9], [7, 3, 7], [11, 12, 12]])
    assert loops_of(V, torch.cat((junk, f, junk))) == want


def test_loops_of_small_cases():
    from dgs_amd.mesh_fill import boundary_loops, is_watertight
    quads, _ = grid_faces(6, 5, False)
    sheet = torch.from_numpy(quads.reshape(-1, 3))
    got = loops_of(30, sheet)
    assert got == walk_loops(sheet.tolist()) and len(got) == 1 and len(got[0]) == 2 * (5 + 4) and got[0][0] == 0      # the outer rim
    tet = lambda a, b, c, d: [(a, b, c), (a, c, d), (a, d, b), (b, d, c)]
    two = tet(0, 1, 2, 3) + tet(0, 4, 5, 6)                      # two tetrahedra sharing vertex 0
    assert loops_of(7, torch.tensor(two)) == []
    bow = torch.tensor([t for t in two if t not in ((0, 1, 2), (0, 4, 5))])              # a face at the shared vertex off each: a bow-tie
    assert walk_loops(bow.tolist()) == [] == loops_of(7, bow)
    apart = torch.tensor([t for t in two if t not in ((1, 3, 2), (4, 6, 5))])            # the faces away from it: two holes of 3
    assert loops_of(7, apart) == walk_loops(apart.tolist()) == [[1, 3, 2], [4, 6, 5]]
    fin = torch.tensor([(0, 1, 2), (0, 1, 3), (0, 1, 4)])        # three faces on one edge: open chains only
    assert loops_of(5, fin) == walk_loops(fin.tolist()) == []
    flipped = torch.tensor(tet(0, 1, 2, 3)[:3] + [(1, 2, 3)])    # a closed tetrahedron with one face flipped: every edge is used twice
    assert loops_of(4, flipped) == walk_loops(flipped.tolist()) == [] and not is_watertight(4, flipped)
    sheet_flipped = sheet.clone()
    sheet_flipped[18] = sheet_flipped[18, [0, 2, 1]]               # an interior face flipped: the rim is what it was
    assert loops_of(30, sheet_flipped) == walk_loops(sheet_flipped.tolist()) == got
    sheet_flipped[0] = sheet_flipped[0, [0, 2, 1]]               # a rim face flipped: the rim's directions clash, vertices lose simplicity
    assert loops_of(30, sheet_flipped) == walk_loops(sheet_flipped.tolist())
    assert is_watertight(4, torch.tensor(tet(0, 1, 2, 3))) and is_watertight(7, torch.tensor(two)) and not is_watertight(30, sheet)
    assert not is_watertight(5, fin) and not is_watertight(3, torch.zeros((0, 3), dtype=torch.int64))
    lv, off = boundary_loops(4, torch.zeros((0, 3), dtype=torch.int32))
    assert lv.shape == (0,) and off.tolist() == [0]
    for bad in (torch.tensor([[0, 1, 4]]), torch.tensor([[0, -1, 2]])):
        with pytest.raises(ValueError, match="out of range"):
            boundary_loops(4, bad)
        with pytest.raises(ValueError, match="out of range"):
            is_watertight(4, bad)
    with pytest.raises(ValueError):
        boundary_loops(4, torch.tensor([[0, 1, 2]]), max_edges=-1)


def test_rank_statement_counts_rounds():
    """rank_torch on rings of every size around the powers of two: ceil(log2 n) rounds rank a ring of n, and so do more; rounds
    with 2^rounds < n - 2 do not."""
    from dgs_amd.mesh_fill import rank_torch
    for n in (3, 4, 5, 8, 9, 31, 32, 33, 128, 129):
        succ = (torch.arange(n) + 1) % n
        leader = torch.zeros(n, dtype=torch.int64)
        want = torch.cat((torch.zeros(1), torch.arange(n - 1, 0, -1))).to(torch.int32)
        rounds = (n - 1).bit_length()
        assert torch.equal(rank_torch(succ, leader, rounds), want) and torch.equal(rank_torch(succ, leader, rounds + 3), want)
        # 2^rounds < n - 2: the node behind the leader has not reached the end (the leader's own rank is 0 whatever its distance)
        assert n == 3 or not torch.equal(rank_torch(succ, leader, (n - 3).bit_length() - 1), want)
    # a malformed table (a ring that is never cut) gives some answer after the same number of rounds
    assert rank_torch((torch.arange(8) + 1) % 8, torch.full((8,), 99), 3).shape == (8,)


# ---- the fill -----------------------------------------------------------------------------------------------------------------------
def test_counts_follow_the_formulas():
    from dgs_amd.mesh_fill import fill_counts, fill_holes, ring_count
    assert [ring_count(n) for n in (3, 4, 9, 10, 16, 100)] == [1, 1, 1, 2, 3, 16]
    assert fill_counts(3) == (0, 1) and fill_counts(4) == (1, 4) and fill_counts(9) == (1, 9) and fill_counts(10) == (11, 30)
    assert fill_counts(16) == (16 + 5 + 1, 32 + 21 + 5)
    for n in (4, 9, 10, 16, 100):
        v, f = annulus(n)
        gv, gf, gc = fill_holes(v, f, max_hole_edges=n)
        assert (gv.shape[0] - v.shape[0], gf.shape[0] - f.shape[0]) == fill_counts(n) and gc is None


@pytest.mark.parametrize("cap", [4, 16, 64, 1000])
def test_fill_on_the_torus(torus, cap):
    from dgs_amd.mesh_fill import fill_counts, fill_holes, is_watertight
    v, f, c = torus
    V, F = v.shape[0], f.shape[0]
    before = loops_of(V, f)
    gv, gf, gc = fill_holes(v, f, c, max_hole_edges=cap)
    closed = [r for r in before if len(r) <= cap]
    assert loops_of(gv.shape[0], gf) == [r for r in before if len(r) > cap]                 # exactly the loops within the cap
    assert euler(gf) == euler(f) + len(closed)
    assert is_watertight(gv.shape[0], gf) == (cap >= 64) and (cap < 64 or euler(gf) == 0)
    assert torch.equal(bits(gv[:V]), bits(v)) and torch.equal(gf[:F], f) and torch.equal(bits(gc[:V]), bits(c)) and gf.dtype == f.dtype
    counts = [fill_counts(len(r)) for r in closed]
    assert gv.shape[0] - V == sum(a for a, b in counts) and gf.shape[0] - F == sum(b for a, b in counts) and gc.shape == gv.shape
    # new vertices and faces follow loop by loop in the order of boundary_loops: every loop's faces name its rim and its own vertices
    at_v, at_f = V, F
    for r, (nv, nf) in zip(closed, counts):
        mine = gf[at_f:at_f + nf]
        assert set(mine.reshape(-1).tolist()) == set(r) | set(range(at_v, at_v + nv))
        at_v, at_f = at_v + nv, at_f + nf
    assert float(gc[V:].min()) >= 0.0 and float(gc[V:].max()) <= 1.0 and bool(torch.isfinite(gv).all())
    # the fills of the small holes face the way the surface does: along the torus' outward normal at the face centre.  (The rim of
    # 57 bends through 75 degrees of the torus; its fill is closed and consistently wound -- is_watertight above -- but a membrane
    # that far from a plane may fold: DESIGN.md section 21, "what it is not".)
    small = sum(b for r, (a, b) in zip(closed, counts) if len(r) > 16)
    ctr = gv[gf[F + small:].long()].double().mean(1)
    ring = torch.stack((ctr[:, 0], ctr[:, 1], torch.zeros_like(ctr[:, 0])), -1)
    outward = ctr - 2.0 * ring / ring.norm(dim=1, keepdim=True)
    assert bool(((fill_normals(gv, gf, F + small) * outward).sum(1) > 0).all())
    again = fill_holes(gv, gf, gc, max_hole_edges=cap)                                      # a second call returns its input
    assert again[0] is gv and again[1] is gf and again[2] is gc
    iv, i_f, ic = fill_holes(v, f.to(torch.int32), None, max_hole_edges=cap)
    assert i_f.dtype == torch.int32 and torch.equal(i_f.long(), gf) and torch.equal(bits(iv), bits(gv)) and ic is None


def test_the_lone_triangle_is_skipped():
    from dgs_amd.mesh_fill import fill_holes
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5], [5, 5, 6]])
    for tri in ([0, 1, 2], [0, 2, 1]):                           # either winding
        f = torch.tensor([tri])
        assert loops_of(7, f) == [[0] + ([2, 1] if tri[1] == 1 else [1, 2])]
        gv, gf, gc = fill_holes(v, f)
        assert gv is v and gf is f and gc is None
    open_tet = torch.tensor([tri, (3, 4, 5), (3, 5, 6), (3, 6, 4)])                         # ... while the tetrahedron's hole beside it is closed
    gv, gf, _ = fill_holes(v, open_tet)
    assert gv.shape[0] == 7 and gf.tolist() == open_tet.tolist() + [[4, 6, 5]]


@pytest.mark.parametrize("n", [4, 9, 10, 16, 64])
def test_regular_polygons(n):
    """A regular n-gon hole in a planar fan (tilted, so that no axis is special): every new normal points the sheet's way and the
    new vertices lie in its plane to 1e-6 of its size; the centre vertex is the polygon's centre."""
    from dgs_amd.mesh_fill import fill_holes
    v, f = annulus(n)
    rot = torch.linalg.qr(torch.tensor([[1.0, 2, 3], [-2, 1, 0.5], [0.3, -1, 2]], dtype=torch.float64))[0]
    if torch.linalg.det(rot) < 0:
        rot[:, 2] = -rot[:, 2]
    shift = torch.tensor([0.3, -1.2, 0.7], dtype=torch.float64)
    w = (v.double() @ rot.T + shift).float()
    c = torch.rand(w.shape, generator=torch.Generator().manual_seed(n))
    gv, gf, gc = fill_holes(w, f, c, max_hole_edges=n)
    normal = rot[:, 2]
    assert bool((fill_normals(gv, gf, f.shape[0]) @ normal > 0).all())
    new = gv[w.shape[0]:].double()
    assert float(((new - shift) @ normal).abs().max()) <= 1e-6 * 4.0                        # the sheet is 4 across
    assert float((new[-1] - shift).norm()) <= 1e-6 * 4.0                                    # ring R: the centre
    assert float(((new - shift) @ rot)[:, :2].norm(dim=1).max()) < 1.0                      # inside the hole
    assert torch.allclose(gc[-1].double(), c[:n].double().mean(0), atol=1e-6)
    # flat colours give flat colours back, exactly representable ones exactly
    flat = fill_holes(w, f, torch.full_like(w, 0.25), max_hole_edges=n)[2]
    assert bool((flat == 0.25).all())


def test_jagged_planar_sweep():
    """40 round holes with staircase rims of 8 to 114 edges in a 48 x 48 planar grid.  Every fill is a valid strip complex (the
    sheet's Euler characteristic rises by one, the outer rim is all that stays open, every new edge has two faces), and AT MOST
    0.1 % OF THE FILL TRIANGLES FACE AWAY from the sheet: a condition that keeps a broken strip from hiding, not a measurement.
    Measured for this recipe: 0 of 30 532, 0.000 % (the figure is printed)."""
    from dgs_amd.mesh_fill import fill_counts, fill_holes
    total = away = 0
    sizes = []
    for k in range(40):
        v, f = jagged_hole(k)
        before = loops_of(v.shape[0], f)
        assert len(before) == 2 and len(before[0]) == 4 * 47                                # the outer rim starts at vertex 0
        n = len(before[1])
        sizes.append(n)
        gv, gf, _ = fill_holes(v, f, max_hole_edges=150)
        assert loops_of(gv.shape[0], gf) == before[:1] and euler(gf) == euler(f) + 1
        assert (gv.shape[0] - v.shape[0], gf.shape[0] - f.shape[0]) == fill_counts(n)
        assert float(gv[v.shape[0]:, 2].abs().max()) == 0.0
        nz = fill_normals(gv, gf, f.shape[0])[:, 2]
        total, away = total + nz.shape[0], away + int((nz <= 0).sum())
    print("jagged sweep: rims of %d to %d edges, %d of %d fill triangles face away (%.4f %%)" % (min(sizes), max(sizes), away, total, 100.0 * away / total))
    assert min(sizes) == 8 and 100 <= max(sizes) <= 120
    assert away <= 0.001 * total


# ---- wrappers -----------------------------------------------------------------------------------------------------------------------
def test_clean_mesh_fills_on_request_only(torus):
    from dgs_amd.mesh_clean import clean_mesh
    from dgs_amd.mesh_fill import fill_holes
    v, f, c = torus
    v, f, c = torch.cat((v, v[:5])), torch.cat((f, f[:3])), torch.cat((c, c[:5]))           # something to weld and to drop
    plain = clean_mesh(v, f, c)
    assert all(torch.equal(a, b) for a, b in zip(plain, clean_mesh(v, f, c, fill_holes=None)))
    filled = clean_mesh(v, f, c, fill_holes=16)
    want = fill_holes(*plain, max_hole_edges=16)
    assert all(torch.equal(a, b) for a, b in zip(filled, want)) and filled[1].shape[0] > plain[1].shape[0]
    assert [len(r) for r in loops_of(filled[0].shape[0], filled[1])] == [57]
    with pytest.raises(ValueError):
        clean_mesh(v, f, c, fill_holes=-1)
    with pytest.raises(ValueError):
        clean_mesh(v.double(), f, c, fill_holes=16)


def test_extract_meshes_fills_on_request_only(tmp_path, monkeypatch):
    """The harness of tests/test_mesh_simplify_cpu.py: extract_meshes on CPU tensors over analytic sphere views, with the faces at two
    vertices taken out behind the component filter.  The defaults write what they wrote; fill_holes writes fill_holes of that,
    watertight where the loops fit the cap, and the smoothing comes after it."""
    from types import SimpleNamespace
    from test_mesh_cpu import fusion_inputs, sphere_box
    from dgs_amd import fit, io as dio, mesh
    from dgs_amd.mesh_fill import fill_holes, is_watertight
    from dgs_amd.mesh_smooth import smooth_mesh
    N = 28
    origin, h = sphere_box(N)
    views = fusion_inputs(6, 64)
    lo = np.asarray(origin, dtype=np.float64)
    keep_largest = mesh.keep_largest_components

    def punched(v, f, c, **kw):
        v, f, c = keep_largest(v, f, c, **kw)
        return compact(v, f[~((f == 100) | (f == 400)).any(1)], c)

    monkeypatch.setattr(fit, "restore", lambda *a, **k: (None, None))
    monkeypatch.setattr(dio, "load_dnerf", lambda *a, **k: {"train": [SimpleNamespace(camera=None)] * 6, "test": []})
    monkeypatch.setattr(mesh, "views_at_time", lambda surfels, deform, cams, t, bg, **k: views)
    monkeypatch.setattr(mesh, "keep_largest_components", punched)
    kw = dict(times=[0.5], voxel_size=h, bounds=(lo, lo + h * (N - 1)), iteration=7, device="cpu", min_faces=0)
    plain = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "a"), **kw)
    vol = mesh.TSDFVolume.from_bounds(*kw["bounds"], h, "cpu").integrate(*views, trunc=5 * h, depth_trunc=6.0)
    v, f, c = punched(*vol.extract(), n_keep=1000, min_faces=0)
    want = str(tmp_path / "want.ply")
    dio.write_mesh_ply(want, v, f, c)
    assert open(plain[0], "rb").read() == open(want, "rb").read() and not is_watertight(v.shape[0], f)
    assert open(mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "b"), fill_holes=None, **kw)[0], "rb").read() == open(want, "rb").read()
    part = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "p"), fill_holes=32, **kw)
    gv, gf, gc = fill_holes(v, f, c, max_hole_edges=32)
    assert gf.shape[0] > f.shape[0] and min(len(r) for r in loops_of(gv.shape[0], gf)) > 32    # six views leave holes of up to 144 edges
    dio.write_mesh_ply(want, gv, gf, gc)
    assert open(part[0], "rb").read() == open(want, "rb").read()
    filled = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "c"), fill_holes=200, **kw)
    gv, gf, gc = fill_holes(v, f, c, max_hole_edges=200)
    assert gf.shape[0] > f.shape[0] and is_watertight(gv.shape[0], gf)
    dio.write_mesh_ply(want, gv, gf, gc)
    assert open(filled[0], "rb").read() == open(want, "rb").read()
    both = mesh.extract_meshes(str(tmp_path), "data", out_dir=str(tmp_path / "d"), fill_holes=200, smooth_iterations=2, **kw)
    dio.write_mesh_ply(want, *smooth_mesh(gv, gf, gc, iterations=2))
    assert open(both[0], "rb").read() == open(want, "rb").read()


def test_fill_shell(tmp_path, capsys, torus):
    from dgs_amd.io import read_mesh_ply, write_mesh_ply
    from dgs_amd.mesh_fill import fill_holes, main
    v, f, c = torus
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    write_mesh_ply(src, v, f, c)
    rv, rf, rc = (torch.from_numpy(np.ascontiguousarray(x)) for x in read_mesh_ply(src))
    for extra, kw, tail in (([], {}, "0 loops, watertight"), (["--max-edges", "10"], {"max_hole_edges": 10}, "2 loops")):
        main([src, dst, "--device", "cpu"] + extra)
        sv, sf, sc = fill_holes(rv, rf, rc, **kw)
        gv, gf, gc = read_mesh_ply(dst)
        assert np.array_equal(gv, sv.numpy()) and np.array_equal(gf, sf.numpy()) and gc.shape == gv.shape and gf.shape[0] > f.shape[0]
        before, after = capsys.readouterr().out.strip().split("->")
        assert before.strip().endswith("7 loops") and after.endswith(tail)
    with open(str(tmp_path / "in.obj"), "w") as fh:
        fh.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()) + "".join("f %d %d %d\n" % tuple(i + 1 for i in t) for t in f.tolist()))
    main([str(tmp_path / "in.obj"), dst, "--device", "cpu"])
    assert read_mesh_ply(dst)[1].shape[0] > f.shape[0]
    with pytest.raises(ValueError):
        main([str(tmp_path / "in.stl"), dst, "--device", "cpu"])
    with pytest.raises(SystemExit):
        main([src])


def test_refusals(monkeypatch):
    from dgs_amd import mesh_fill
    from dgs_amd.mesh_fill import fill_holes
    v, f = annulus(8)
    c = torch.rand(v.shape)
    for kw in ({"max_hole_edges": -1}, {"max_hole_edges": 2.5}, {"max_hole_edges": True}, {"max_hole_edges": None}):
        with pytest.raises(ValueError, match="max_hole_edges"):
            fill_holes(v, f, c, **kw)
    bad = v.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        fill_holes(bad, f)
    for wrong in (f.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(v.shape[0])),
                  f.clone().index_put_((torch.tensor(2), torch.tensor(1)), torch.tensor(-1))):
        with pytest.raises(ValueError, match="out of range"):
            fill_holes(v, wrong)
    for args in ((v.double(), f), (v, f.float()), (v, f, c.double()), (v, f, c[:5]), (v[:, :2], f), (v, f[:, :2])):
        with pytest.raises(ValueError):
            fill_holes(*args)
    assert fill_holes(v, f, c, max_hole_edges=0)[1] is f and fill_holes(v, f, c, max_hole_edges=7)[1] is f       # nothing to do
    ev, ef, ec = fill_holes(v[:0], f[:0], None)
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ec is None
    # totals that leave int32, with the limit brought down to this mesh's size
    monkeypatch.setattr(mesh_fill, "_ID_LIMIT", v.shape[0] + 1)
    with pytest.raises(ValueError, match="int32"):
        fill_holes(v, f, max_hole_edges=8)
    monkeypatch.setattr(mesh_fill, "_ID_LIMIT", f.shape[0] + 8)
    with pytest.raises(ValueError, match="int32"):
        fill_holes(v, f, max_hole_edges=8)


def test_fill_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops, mesh_fill
    lib = _mesh_ops.load()
    buf, other = (ctypes.c_longlong * 64)(), (ctypes.c_longlong * 64)()
    p, q = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(other, ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    big = 2 ** 31
    rank, rim, emit = lib.dgs_fill_rank, lib.dgs_fill_rim, lib.dgs_fill_emit
    # rank(n, succ, leader, n_rounds, buf_a, buf_b, rank, stream)
    assert rank(-1, p, p, 3, p, q, p, None) < 0 and b"negative" in err()
    assert rank(big, p, p, 3, p, q, p, None) < 0 and b"2^31" in err()
    assert rank(4, p, p, -1, p, q, p, None) < 0 and b"n_rounds" in err()
    assert rank(4, p, p, 32, p, q, p, None) < 0 and b"n_rounds" in err()
    assert rank(4, p, p, 3, p, p, p, None) < 0 and b"two buffers" in err()
    for k in (1, 2, 4, 5, 6):
        args = [4, p, p, 3, p, q, p, None]
        args[k] = None
        assert rank(*args) < 0 and b"null" in err()
    assert rank(0, None, None, 3, None, None, None, None) == 0
    # rim(V, vertices, colors, B, loop_vertices, rim_loop, L, offsets, cx, cy, cz, scale, S, SC, rows, stream)
    good = [8, p, p, 8, p, p, 1, p, 0.0, 0.0, 0.0, 1.0, p, p, p, None]
    change = lambda base, **kw: [kw.get(str(i), x) for i, x in enumerate(base)]
    for k in (0, 3, 6):
        assert rim(*change(good, **{str(k): -1})) < 0 and b"negative" in err()
        assert rim(*change(good, **{str(k): big})) < 0 and b"2^31" in err()
    for k in (1, 4, 5, 7, 12, 14):
        assert rim(*change(good, **{str(k): None})) < 0 and b"null" in err()
    assert rim(*change(good, **{"2": None})) < 0 and b"together" in err()                  # colors without SC's partner
    assert rim(*change(good, **{"13": None})) < 0 and b"together" in err()
    for k, x in ((8, float("nan")), (9, float("inf")), (11, 0.0), (11, -1.0), (11, float("inf")), (11, float("nan"))):
        assert rim(*change(good, **{str(k): x})) < 0 and b"frame" in err()
    assert rim(*change(good, **{"3": 0, "6": 0})) == 0
    # emit(n_old, n_new, vert_ring, n_new_faces, face_ring, n_rings, rings, L, offsets, B, loop_vertices, rows, S, SC, cx, cy, cz, scale,
    #      vertices_out, colors_out, faces_out, stream)
    good = [8, 4, p, 4, p, 1, p, 1, p, 8, p, p, p, p, 0.0, 0.0, 0.0, 1.0, p, p, p, None]
    for k in (0, 1, 3, 5, 7, 9):
        assert emit(*change(good, **{str(k): -1})) < 0 and b"negative" in err()
        assert emit(*change(good, **{str(k): big})) < 0 and b"2^31" in err()
    assert emit(*change(good, **{"0": big - 2})) < 0 and b"2^31" in err()                  # n_old + n_new
    for k in (2, 4, 6, 8, 10, 11, 12, 18, 20):
        assert emit(*change(good, **{str(k): None})) < 0 and b"null" in err()
    assert emit(*change(good, **{"13": None})) < 0 and b"together" in err()
    assert emit(*change(good, **{"19": None})) < 0 and b"together" in err()
    assert emit(*change(good, **{"17": 0.0})) < 0 and b"frame" in err()
    for k in (5, 7, 9):
        assert emit(*change(good, **{str(k): 0})) < 0 and b"without" in err()
    assert emit(*change(good, **{"1": 0, "3": 0})) == 0
    assert lib.dgs_fill_layout(None) < 0 and b"null" in err()
    lay = _mesh_ops.fill_layout()
    assert lay == (256, 1, mesh_fill.POS_BITS, mesh_fill.NRM_BITS, mesh_fill.COL_BITS, mesh_fill.RING_COLS, len(mesh_fill.TAPS), 31)
