"""-m gpu: the dgs_decimate_* kernels and dgs_amd.mesh_decimate on a HIP device against the CPU statement.  Every comparison is
exact: int64 rows, fp32 bit patterns of costs, placements, vertices and colours, the packed minima, faces and maps."""
import ctypes

import numpy as np
import pytest
import torch

from test_mesh_decimate_cpu import as_mesh, cube, flat_grid, glued_sheets, hub, icosphere, shuffled, undirected_counts
from test_mesh_simplify_cpu import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")


def to_dev(x):
    if isinstance(x, dict):
        return {k: to_dev(v) for k, v in x.items()}
    return None if x is None else x.to(DEV)


def padded(mesh, n_vertices):
    """The mesh with loose vertices appended up to n_vertices (nothing refers to them)."""
    v, f, c = mesh
    extra = n_vertices - v.shape[0]
    if extra <= 0:
        return mesh
    g = torch.Generator().manual_seed(extra)
    return torch.cat((v, torch.rand((extra, 3), generator=g))), f, torch.cat((c, torch.rand((extra, 3), generator=g)))


def first_round(mesh, n_items, preserve_boundary=True):
    """The CPU state of a mesh after step 1 and the tables of its first round, cut to the first n_items edges: what every kernel of
    a round is handed.  (An edge's cost, placement and validity do not depend on the other edges, so a cut table is a valid input.)"""
    from dgs_amd import mesh_decimate as md
    st, q_bits, scale, centre = md.prepare(*mesh, preserve_boundary)
    tab = md.round_tables(st.pos.shape[0], st.faces, preserve_boundary)
    tab["edges"] = tab["edges"][:, :n_items].contiguous()
    return st, q_bits, tab


def sizes():
    from dgs_amd import _mesh_ops
    threads, items = _mesh_ops.decimate_layout()[:2]
    return threads * items * 2 + 3          # two whole workgroups and a ragged third: a seam and a tail


# ---- each kernel alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "glued sheets"])
def test_each_kernel_alone(name):
    from dgs_amd import _mesh_ops, mesh_decimate as md
    n = sizes()
    mesh = icosphere() if name == "sphere" else padded(glued_sheets(13), n)          # 642 vertices / n vertices: both ragged
    st, q_bits, tab = first_round(mesh, n)
    V, F, E = st.pos.shape[0], st.faces.shape[0], tab["edges"].shape[1]
    assert E == n and F > n and V > 2 * 256
    # initial quadrics, over the first n faces and over all of them
    mean_len = md.mean_length(md.normal_lengths(st.pos, st.faces)[1])
    for cut in (n, F):
        want = md.quadrics_torch(st.pos, st.faces[:cut], mean_len, q_bits)
        got = _mesh_ops.decimate_quadrics(st.pos.to(DEV), st.faces[:cut].to(torch.int32).to(DEV), mean_len, q_bits)
        assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    assert torch.equal(want, st.rows) and int(want.abs().max()) > 2 ** 30
    # cost, placement, validity
    f32 = st.faces.to(torch.int32)
    dtab = to_dev(tab)
    for max_cost in (INF, 1e-6):
        cost, place, valid = md.edge_costs_torch(st.pos, st.rows, st.faces, tab, q_bits, max_cost)
        got = _mesh_ops.decimate_edges(st.pos.to(DEV), st.rows.to(DEV), f32.to(DEV), dtab, q_bits, max_cost)
        same_bits(got, (cost, place, valid))
    cost, place, valid = md.edge_costs_torch(st.pos, st.rows, st.faces, tab, q_bits, INF)
    locked = (tab["flags"] & md.FLAG_LOCKED) != 0
    print("%s: %d of %d edges valid, %d locked vertices" % (name, int(valid.sum()), E, int(locked.sum())))
    assert 0 < int(valid.sum()) < E or name == "sphere"
    assert (name == "sphere") == (not locked.any())
    # the two selection passes, for a narrow and a wide throttle
    for k in (20, E):
        kth = torch.kthvalue(torch.where(valid, cost, torch.full((), INF)), k).values
        compete = valid & (cost <= kth)
        m1, m2, selected = md.select_torch(V, tab["edges"], cost, compete)
        got = _mesh_ops.decimate_select(V, dtab["edges"], cost.to(DEV), compete.to(DEV))
        same_bits(got, (m1, m2, selected))
        assert selected.any() and (m1 <= m2.new_tensor(md.NO_KEY)).all() and (m2 <= m1).all()
    # apply
    sel = selected.nonzero().reshape(-1)
    assert sel.numel() > 3
    state = lambda dev: [st.pos.clone().to(dev), st.rows.clone().to(dev), st.colors.clone().to(dev), st.moved.clone().to(dev)]
    cpu, dev = state("cpu"), state(DEV)
    vmap, g, keep = md.apply_torch(*cpu, st.faces, tab, place, sel)
    dvmap, dg, dkeep = _mesh_ops.decimate_apply(*dev, f32.to(DEV), dtab, place.to(DEV), sel.to(torch.int32).to(DEV))
    same_bits(dev, cpu)
    same_bits((dvmap.long(), dg.long(), dkeep), (vmap, g, keep))
    assert int((vmap != torch.arange(V)).sum()) == sel.numel() and int((~keep).sum()) >= sel.numel()


# ---- the whole function ---------------------------------------------------------------------------------------------------------
def check_mesh(mesh, **kw):
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = mesh
    want = decimate_mesh(v, f, c, return_map=True, **kw)
    got = decimate_mesh(v.to(DEV), f.to(DEV), None if c is None else c.to(DEV), return_map=True, **kw)
    assert all(x.is_cuda for x in got if x is not None)
    same_bits(got, want)
    return want


def test_the_icosphere():
    v, f, c = icosphere()
    dv, df, dc, vmap = check_mesh((v, f, c), ratio=0.25)
    assert df.shape[0] in (320, 319) and (undirected_counts(df)[1] == 2).all()
    check_mesh((v, f, None), target_faces=500, max_error=0.05)


@pytest.mark.parametrize("preserve_boundary", [True, False])
def test_the_open_grid(preserve_boundary):
    dv, df, dc, vmap = check_mesh(flat_grid(), ratio=0.1, preserve_boundary=preserve_boundary)
    assert df.shape[0] < 100 and float(dv[:, 2].abs().max()) == 0.0


def test_the_cube():
    dv, df, dc, vmap = check_mesh(cube(), ratio=0.1)
    assert df.shape[0] in (76, 75)


def test_a_hub_of_valence_500():
    """One thread walks the hub's rows: 500 neighbours, 500 faces."""
    v, f, c = hub(500)
    assert int(torch.bincount(f.reshape(-1).long()).max()) == 500
    dv, df, dc, vmap = check_mesh((v, f, c), ratio=0.5, preserve_boundary=False)
    assert df.shape[0] < f.shape[0]
    check_mesh((v, f, c), ratio=0.5)


def test_shuffled_ids_and_both_face_dtypes():
    v, f, c = shuffled(icosphere())
    a = check_mesh((v, f, c), ratio=0.25)
    b = check_mesh((v, f.long(), c), ratio=0.25)
    assert a[1].dtype == torch.int32 and b[1].dtype == torch.int64 and torch.equal(a[1].long(), b[1])
    assert (undirected_counts(a[1])[1] == 2).all()


def test_an_empty_mesh_and_a_single_face():
    v, f, c = as_mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)])
    for mesh in ((v[:0], f[:0], c[:0]), (v, f[:0], c), (v, f, c), (v, f, None)):
        for kw in ({"ratio": 0.5}, {"target_faces": 0}, {"ratio": 0.5, "preserve_boundary": False}):
            out = check_mesh(mesh, **kw)
            assert out[1].shape[0] == mesh[1].shape[0]


def test_two_runs_are_bit_identical():
    from dgs_amd.mesh_decimate import decimate_mesh
    v, f, c = (x.to(DEV) for x in glued_sheets(13))
    first = decimate_mesh(v, f, c, ratio=0.3, return_map=True)
    same_bits(decimate_mesh(v, f, c, ratio=0.3, return_map=True), first)


# ---- the guards -----------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_range_add_nothing():
    """The C calls themselves (the wrapper produces no such ids), the guard cases of tests/test_mesh_simplify_gpu.py: a face with a
    vertex id outside [0, V) adds nothing to the rows; an edge with such an endpoint gets the neutral outputs and takes no part in
    the selection; an opposite vertex, a face id or a selected entry outside its range is skipped; the others are computed as if
    the bad ones were not there, and a sentinel-filled margin around every output is untouched."""
    from dgs_amd import _mesh_ops, mesh_decimate as md
    lib = _mesh_ops.load()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    st, q_bits, tab = first_round(glued_sheets(13), 10 ** 9)
    V, F, E = st.pos.shape[0], st.faces.shape[0], tab["edges"].shape[1]
    bad_ids = torch.tensor([-1, V, V + 7, 2 ** 31 - 1, -2 ** 31, -9], dtype=torch.int32)
    pick = lambda n, step: (torch.arange(0, n, step), bad_ids[torch.arange(len(range(0, n, step))) % bad_ids.numel()])

    def margin(shape, dtype, fill):
        n = int(np.prod(shape))
        whole = torch.full((n + 128,), fill, dtype=dtype, device=DEV)
        return whole, whole[64:64 + n].view(shape)

    def untouched(whole, n, fill):
        return bool((whole[:64] == fill).all()) and bool((whole[64 + n:] == fill).all())

    # quadrics
    f32 = st.faces.to(torch.int32)
    bad_f = f32.clone()
    at, ids = pick(F, 9)
    bad_f[at, 1] = ids
    ok_f = torch.ones(F, dtype=torch.bool)
    ok_f[at] = False
    mean_len = md.mean_length(md.normal_lengths(st.pos, st.faces)[1])
    whole, rows = margin((V, 10), torch.int64, -7)
    dpos, dbad_f = st.pos.to(DEV), bad_f.to(DEV)
    assert lib.dgs_decimate_quadrics(V, dpos.data_ptr(), F, dbad_f.data_ptr(), mean_len, q_bits, rows.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(rows.cpu(), md.quadrics_torch(st.pos, st.faces[ok_f], mean_len, q_bits)) and untouched(whole, V * 10, -7)
    # edges: bad endpoints on some, bad opposite vertices on others, a bad face id in the rows of the faces, a face with a bad vertex
    cost, place, valid = md.edge_costs_torch(st.pos, st.rows, st.faces, tab, q_bits, INF)
    edges = tab["edges"].clone()
    at_u, ids_u = pick(E, 11)
    at_v, ids_v = pick(E - 3, 13)
    at_v = at_v + 3
    edges[0, at_u], edges[1, at_v] = ids_u, ids_v
    at_o = torch.arange(5, E, 17)
    edges[3, at_o] = bad_ids[torch.arange(at_o.numel()) % bad_ids.numel()].clamp(min=V)          # (-1 means "no second face": not a bad id)
    vf = tab["vf"].clone()
    vf_at = torch.arange(2, vf.numel(), 97)
    vf[vf_at] = torch.tensor([F, -1, F + 5, 2 ** 31 - 1], dtype=torch.int32)[torch.arange(vf_at.numel()) % 4]
    dead = torch.zeros(E, dtype=torch.bool)
    dead[at_u] = True
    dead[at_v] = True
    out_c, dcost = margin((E,), torch.float32, -7.0)
    out_p, dplace = margin((E, 3), torch.float32, -7.0)
    out_v, dvalid = margin((E,), torch.uint8, 9)
    dev = to_dev({"rows": st.rows, "flags": tab["flags"], "faces": bad_f, "edges": edges, "ao": tab["adj_offsets"], "adj": tab["adj"], "vo": tab["vf_offsets"], "vf": vf})
    rc = lib.dgs_decimate_edges(V, dpos.data_ptr(), dev["rows"].data_ptr(), dev["flags"].data_ptr(), F, dev["faces"].data_ptr(), E, dev["edges"].data_ptr(),
                                dev["ao"].data_ptr(), dev["adj"].data_ptr(), dev["adj"].numel(), dev["vo"].data_ptr(), dev["vf"].data_ptr(), dev["vf"].numel(),
                                q_bits, INF, dcost.data_ptr(), dplace.data_ptr(), dvalid.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    gc, gp, gv = dcost.cpu(), dplace.cpu(), dvalid.cpu().bool()
    assert untouched(out_c, E, -7.0) and untouched(out_p, 3 * E, -7.0) and untouched(out_v, E, 9)
    assert (gc[dead] == 0).all() and (gp[dead] == 0).all() and not gv[dead].any()
    same_bits((gc[~dead], gp[~dead]), (cost[~dead], place[~dead]))                             # cost and placement do not read what was spoilt
    assert not gv[at_o].any() and not (gv & ~valid).any()                                      # spoilt neighbourhoods only ever take validity away
    clean = torch.ones(E, dtype=torch.bool)                                                    # edges none of whose inputs were touched
    clean[dead] = False
    clean[at_o] = False
    e = tab["edges"].long()
    face_hit = torch.zeros(V, dtype=torch.bool)
    face_hit[st.faces[~ok_f].reshape(-1)] = True
    row_hit = torch.zeros(V, dtype=torch.bool)
    row_hit[torch.searchsorted(tab["vf_offsets"], vf_at, right=True) - 1] = True
    clean &= ~(face_hit | row_hit)[e[0]] & ~(face_hit | row_hit)[e[1]]
    assert clean.sum() > 100 and torch.equal(gv[clean], valid[clean])
    # select: the bad edges take no part -- the statement with them moved to a loop at an extra vertex
    compete = valid.clone()
    compete[dead] = True
    moved_e = edges.clone()
    moved_e[0, dead], moved_e[1, dead] = V, V
    m1, m2, selected = md.select_torch(V + 1, moved_e, cost, compete & ~dead)
    w1, dm1 = margin((V,), torch.int64, -7)
    w2, dm2 = margin((V,), torch.int64, -7)
    ws, dsel = margin((E,), torch.uint8, 9)
    dc, dk = cost.to(DEV), compete.to(DEV)
    assert lib.dgs_decimate_select(V, E, dev["edges"].data_ptr(), dc.data_ptr(), dk.data_ptr(), dm1.data_ptr(), dm2.data_ptr(), dsel.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(dm1.cpu(), m1[:V]) and torch.equal(dm2.cpu(), m2[:V]) and torch.equal(dsel.cpu().bool(), selected)
    assert untouched(w1, V, -7) and untouched(w2, V, -7) and untouched(ws, E, 9) and selected.any() and not selected[dead].any()
    # apply: a list with entries outside [0, E) and with bad edges; faces with bad ids keep them
    sel = selected.nonzero().reshape(-1)
    lst = torch.cat((torch.tensor([-1, E, 2 ** 31 - 1], dtype=torch.int32), sel.to(torch.int32), at_u[:4].to(torch.int32), torch.tensor([-2 ** 31, E + 3], dtype=torch.int32)))
    cpu = [st.pos.clone(), st.rows.clone(), st.colors.clone(), st.moved.clone()]
    vmap, g, keep = md.apply_torch(*cpu, st.faces[ok_f], tab, place, sel)
    wp, apos = margin((V, 3), torch.float32, -7.0)
    wr, arows = margin((V, 10), torch.int64, -7)
    wm, avmap = margin((V,), torch.int32, -7)
    apos.copy_(st.pos), arows.copy_(st.rows)
    acol, amoved, dlst, dkeep = st.colors.to(DEV), st.moved.to(torch.uint8).to(DEV), lst.to(DEV), torch.empty(F, dtype=torch.uint8, device=DEV)
    dfaces, dplace2 = bad_f.to(DEV), place.to(DEV)
    rc = lib.dgs_decimate_apply(V, apos.data_ptr(), arows.data_ptr(), acol.data_ptr(), dev["flags"].data_ptr(), amoved.data_ptr(), avmap.data_ptr(), E,
                                dev["edges"].data_ptr(), dplace2.data_ptr(), lst.numel(), dlst.data_ptr(), F, dfaces.data_ptr(), dkeep.data_ptr(), stream())
    assert rc == 0
    torch.cuda.synchronize()
    same_bits((apos.cpu(), arows.cpu(), acol.cpu(), amoved.cpu().bool(), avmap.cpu().long()), tuple(cpu) + (vmap,))
    assert untouched(wp, 3 * V, -7.0) and untouched(wr, 10 * V, -7) and untouched(wm, V, -7)
    got_f = dfaces.cpu()
    assert torch.equal(got_f[ok_f].long(), g) and torch.equal(dkeep.cpu().bool()[ok_f], keep)
    assert torch.equal(got_f[~ok_f][:, 1], bad_f[~ok_f][:, 1])                                  # a bad id stays as it is


# ---- the product ----------------------------------------------------------------------------------------------------------------
def test_extract_meshes_decimates_on_the_device(tmp_path):
    """The scene and sizes of tests/test_mesh_gpu.py::test_extract_meshes_on_a_short_fit: every frame written with
    decimate_ratio=0.25 has at most a quarter of the undecimated frame's faces, plus one, and no more boundary edges."""
    from dgs_amd.fit import fit
    from dgs_amd.io import read_mesh_ply
    from dgs_amd.mesh import extract_meshes
    from dgs_amd.synthetic import write_dynamic_dnerf
    data, model = str(tmp_path / "scene"), str(tmp_path / "model")
    write_dynamic_dnerf(data, n_train=24, n_test=3, H=128, W=128, device=DEV)
    fit(data, model, iterations=300, device=DEV, num_pts=5000, node_num=128, seed=0, warm_up=100, regularize_from=180, densify_from=100,
        densify_interval=50, opacity_reset_interval=10_000)
    full = extract_meshes(model, data, times=[0.2, 0.7], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "a"))
    light = extract_meshes(model, data, times=[0.2, 0.7], voxel_size=0.03, device=DEV, out_dir=str(tmp_path / "b"), decimate_ratio=0.25)
    assert len(full) == len(light) == 2
    for a, b in zip(full, light):
        (va, fa, ca), (vb, fb, cb) = read_mesh_ply(a), read_mesh_ply(b)
        rim = lambda f: int((undirected_counts(f)[1] == 1).sum())
        print("frame: %d -> %d faces, %d -> %d boundary edges" % (fa.shape[0], fb.shape[0], rim(fa), rim(fb)))
        assert 0 < fb.shape[0] <= fa.shape[0] // 4 + 1
        assert rim(fb) <= rim(fa)
        assert cb.shape == vb.shape and np.isfinite(vb).all() and fb.max() == vb.shape[0] - 1
