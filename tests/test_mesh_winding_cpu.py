"""Winding numbers on the CPU: the PyTorch statement of dgs_winding_sum on closed-form cases, against the float64 brute force of
tests/mesh_winding_ref.py, its freedom from the order of the faces, edge inputs, the functions built on it (contains,
signed_distance, mesh_volume, is_outward, volume_iou), the wiring into mesh_distance / evaluate_meshes / the shell, and the
host-side refusals of the C ABI (no device is touched)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_winding_ref as ref
from test_mesh_decimate_cpu import sphere_distance

IOU_KEYS = {"iou", "volume_pred", "volume_gt", "volume_intersection", "iou_samples"}


def cube():
    """The unit cube [0, 1]^3, wound outward; every coordinate an integer, so in-plane dot products are exactly 0."""
    v = torch.tensor([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=torch.float32)
    f = torch.tensor([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    return v, f


# ---- 1. known answers -----------------------------------------------------------------------------------------------------------
def test_an_octant_triangle_seen_from_the_origin_is_an_eighth():
    from dgs_amd.mesh_metrics import winding_number
    v, f = torch.tensor([[1.0, 0, 0], [0, 1, 0], [0, 0, 1]]), torch.tensor([[0, 1, 2]])
    w = winding_number(torch.zeros(1, 3), v, f)
    assert w.dtype == torch.float64 and w.shape == (1,) and abs(float(w) - 0.125) <= ref.W_TOL
    assert abs(float(winding_number(torch.zeros(1, 3), *ref.flipped((v, f)))) + 0.125) <= ref.W_TOL


def test_an_open_hemisphere_cap_seen_from_the_centre_is_a_half():
    from dgs_amd.mesh_metrics import winding_number
    p, v, f = ref.cap_set()
    assert 0 < f.shape[0] == ref.icosphere(3)[1].shape[0] // 2 and not bool(p[0].any())
    w = winding_number(p, v, f)
    print("W at the centre of the cap: %.9f" % float(w[0]))
    assert abs(float(w[0]) - 0.5) <= ref.W_TOL
    assert bool(((w[1:] > 0.01) & (w[1:] < 0.99)).any())                     # off the centre an open mesh gives neither 0 nor 1


@pytest.mark.parametrize("name", ref.SHAPE_SETS)
def test_closed_shapes_give_integers(name):
    """1 inside and 0 outside the icospheres and the torus, -1 inside the flipped ones, 2 inside the inner of two nested spheres."""
    from dgs_amd.mesh_metrics import is_outward, winding_number
    p, v, f, want = ref.shape_set(name)
    assert is_outward(v, f) == (not name.endswith("flipped")) and len(set(want.tolist())) >= 2
    w = winding_number(p, v, f)
    print("%s: %d queries, max |W - integer| = %.3e (cap %.1e)" % (name, p.shape[0], float((w - want).abs().max()), ref.W_TOL))
    assert bool(((w - want).abs() <= ref.W_TOL).all())


def test_the_shapes_have_the_sizes_the_issue_names():
    assert ref.icosphere(3)[1].shape[0] == 1280 and ref.icosphere(5)[1].shape[0] == 20480 and ref.torus()[1].shape[0] == 2 * 64 * 32
    assert ref.OFFSET >= 0.05 and ref.BOX == 1.6 and ref.W_TOL == 4 * ref.W_MEASURED and ref.W_TOL_SOUP == 4 * ref.W_MEASURED_SOUP


# ---- 2. the statement against the float64 brute force ---------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(ref.SHAPE_SETS) + 1 + len(ref.SOUP_SETS)))
def test_statement_against_float64(index):
    name, p, v, f, soup = ref.cpu_sets()[index]
    tol = ref.W_TOL_SOUP if soup else ref.W_TOL
    err = ref.measure(p, v, f)
    print("%s: max |W32 - W64| = %.3e (cap %.1e)" % (name, err, tol))
    assert err <= tol


def test_the_polynomial_against_float64_atan():
    """The sweep of tools/mesh_winding_margins.py; its first coefficient is exactly 1, so tiny angles carry no relative bias."""
    from dgs_amd.mesh_metrics import _WIND_ATAN, _wind_atan2
    assert _WIND_ATAN[0] == 1.0 and len(_WIND_ATAN) == 8 and all(float(np.float32(c)) == c for c in _WIND_ATAN)
    err = ref.polynomial_error()
    print("polynomial: max error %.3e rad (recorded %.1e)" % (err, ref.POLY_MEASURED))
    assert err <= 4 * ref.POLY_MEASURED
    r = torch.tensor([1e-3, 1e-5, 1e-8, 1e-20], dtype=torch.float32)
    assert torch.equal(_wind_atan2(r[1:], torch.ones(3)), r[1:])              # below 1e-4 the fp32 atan IS its argument
    # the reflections: all eight octants and the axes against torch.atan2
    y = torch.tensor([0.3, 2.0, 2.0, 0.3, -0.3, -2.0, -2.0, -0.3, 0.0, 1.0, 0.0, -1.0])
    x = torch.tensor([2.0, 0.3, -0.3, -2.0, -2.0, -0.3, 0.3, 2.0, 1.0, 0.0, -1.0, 0.0])
    assert bool(((_wind_atan2(y, x).double() - torch.atan2(y.double(), x.double())).abs() <= 4 * ref.POLY_MEASURED).all())


# ---- 3. order freedom -----------------------------------------------------------------------------------------------------------
def test_sums_do_not_depend_on_the_order_or_the_chunking_of_the_faces():
    from dgs_amd.mesh_metrics import winding_sums_torch, winding_table
    for (p, v, f), chunks in ((ref.cap_set(), (1, 7, None)), (ref.soup_set(0.0, 41), (7, 500, None))):
        table = winding_table(v, f)
        want = winding_sums_torch(p, table)
        assert want.dtype == torch.int64 and want.shape == (p.shape[0],) and bool((want != 0).any())
        for chunk in chunks:
            assert torch.equal(winding_sums_torch(p, table, chunk=chunk), want), chunk
        perm = torch.randperm(table.shape[0], generator=torch.Generator().manual_seed(5))
        assert torch.equal(winding_sums_torch(p, table[perm].contiguous()), want)
        assert torch.equal(winding_sums_torch(p, table[perm].contiguous(), chunk=7), want)
        assert torch.equal(winding_sums_torch(p, table), want)                # and from run to run


# ---- 4. edge inputs -------------------------------------------------------------------------------------------------------------
def edge_queries():
    """On a vertex, on an edge, in a face (on the surface), in a face's plane outside the cube, far away, NaN, +inf, -inf."""
    nan, inf = float("nan"), float("inf")
    return torch.tensor([[0, 0, 0], [0.5, 0, 0], [0.5, 0.25, 0], [2, 0.5, 0], [1e6, 1e6, 1e6], [nan, 0.5, 0.5], [inf, 0.5, 0.5],
                         [0.5, -inf, 0.5], [0.5, 0.5, 0.5]], dtype=torch.float32)


def test_edge_queries_give_finite_sums():
    """The cube's in-plane pairs have num = 0 exactly (integer coordinates): a vertex sees the three far faces (W = 1/8), an edge
    midpoint the four faces off its edge (1/4); the 12 pairs of a query each err by at most 2e-7 rad, so 1e-6 bounds W."""
    from dgs_amd.mesh_metrics import contains, winding_number, winding_sums
    v, f = cube()
    p = edge_queries()
    s = winding_sums(p, v, f)
    w = winding_number(p, v, f)
    print(s.tolist(), w.tolist())
    assert s.dtype == torch.int64 and bool(torch.isfinite(w).all()) and bool((s.abs() <= 12 << 30).all())
    assert abs(float(w[0]) - 0.125) <= 1e-6 and abs(float(w[1]) - 0.25) <= 1e-6 and abs(float(w[3])) <= 1e-6 and abs(float(w[8]) - 1) <= 1e-6
    assert -1e-6 <= float(w[2]) <= 1 + 1e-6                                   # on the surface: ambiguous by definition
    assert abs(float(w[4])) <= 1e-6 and s[5:8].tolist() == [0, 0, 0]          # every pair of a NaN or infinite query adds 0
    assert contains(p, v, f).tolist() == [False, False, bool(w[2] > 0.5), False, False, False, False, False, True]


def test_non_finite_vertices_give_finite_sums():
    from dgs_amd.mesh_metrics import winding_number, winding_sums, winding_table
    v, f = cube()
    p = edge_queries()[[3, 4, 8]]
    for bad in (float("nan"), float("inf"), float("-inf")):
        vb = v.clone()
        vb[7, 1] = bad
        touched = (f == 7).any(1)
        w = winding_number(p, vb, f)
        assert bool(torch.isfinite(w).all())
        assert torch.equal(winding_sums(p, vb, f), winding_sums(p, v, f[~touched]))   # the faces at the bad vertex add 0
        assert winding_table(vb, f).shape == (12, 12)


def test_faces_without_area_and_faces_that_name_a_vertex_twice():
    from dgs_amd.mesh_metrics import winding_sums, winding_table
    v, f = cube()
    v2 = torch.cat([v, torch.tensor([[3.0, 3, 3], [4, 4, 4], [6, 6, 6]])])
    flat = torch.tensor([[8, 9, 10]])                                         # collinear corners: n = 0 exactly
    twice = torch.tensor([[0, 0, 5], [3, 7, 7], [2, 6, 2]])
    p = edge_queries()[[0, 1, 3, 8]]                                          # none on the line x = y = z beyond the cube
    want = winding_sums(p, v, f)
    assert torch.equal(winding_sums(p, v2, torch.cat([f, flat])), want)
    assert winding_table(v2, torch.cat([f, flat])).shape == (13, 12)
    assert torch.equal(winding_sums(p, v2, torch.cat([twice[:1], f, twice[1:]])), want)
    assert winding_table(v2, torch.cat([twice[:1], f, twice[1:]])).shape == (12, 12)
    assert torch.equal(winding_table(v2, torch.cat([twice, f])), winding_table(v, f))
    with pytest.raises(ValueError):
        winding_sums(p, v, twice)                                             # nothing is left


def test_empty_inputs_and_bad_arguments():
    from dgs_amd.mesh_metrics import contains, winding_number, winding_sums_torch, winding_table
    v, f = cube()
    w = winding_number(torch.zeros(0, 3), v, f)
    assert w.shape == (0,) and w.dtype == torch.float64 and contains(torch.zeros(0, 3), v, f).shape == (0,)
    with pytest.raises(ValueError, match="no faces"):
        winding_number(torch.zeros(2, 3), v, f[:0])
    with pytest.raises(ValueError, match="no faces"):
        winding_sums_torch(torch.zeros(2, 3), winding_table(v, f)[:0])
    with pytest.raises(ValueError):
        winding_number(torch.zeros(2, 2), v, f)
    with pytest.raises(ValueError):
        winding_number(torch.zeros(2, 3), v, f.float())
    with pytest.raises(ValueError, match="outside"):
        winding_number(torch.zeros(2, 3), v, f + 1)
    t = winding_table(v.double(), f.int())
    assert t.dtype == torch.float32 and t.shape == (12, 12) and torch.equal(t[:, :3], v[f[:, 0]])
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    assert torch.equal(t[:, 9:], n)


# ---- 5. volume and orientation --------------------------------------------------------------------------------------------------
def test_mesh_volume_and_is_outward():
    from dgs_amd.mesh_metrics import is_outward, mesh_volume
    v, f = ref.icosphere(3)
    vol, ball = mesh_volume(v, f), 4 * math.pi / 3
    assert isinstance(vol, float) and 0.99 * ball < vol < ball               # inscribed: a little less than the ball
    assert mesh_volume(*ref.flipped((v, f))) == pytest.approx(-vol, rel=1e-12)
    assert is_outward(v, f) is True and is_outward(*ref.flipped((v, f))) is False
    assert mesh_volume(v * 2 + 5, f) == pytest.approx(8 * vol, rel=1e-6)     # closed: no dependence on the origin
    assert mesh_volume(*cube()) == 1.0 and is_outward(*ref.torus())


# ---- 6. signed distance ---------------------------------------------------------------------------------------------------------
def test_signed_distance_on_an_icosphere():
    """Signs are exact (the queries keep SHELL from the sphere); magnitudes agree with the analytic sphere to the polyhedron's
    sagitta 1 - sqrt(1 - rho^2), rho = L / sqrt(3) the circumradius bound of a face with longest edge L, plus fp32 rounding."""
    from dgs_amd.mesh_metrics import signed_distance
    v, f = ref.icosphere(3)
    p, inside = ref.sphere_box(600, 73)
    assert 50 < int(inside.sum()) < 550
    sd = signed_distance(p, v, f)
    t = v.double()[f]
    L = float(torch.stack([(t[:, 0] - t[:, 1]).norm(dim=1), (t[:, 1] - t[:, 2]).norm(dim=1), (t[:, 2] - t[:, 0]).norm(dim=1)]).max())
    sagitta = 1 - math.sqrt(1 - L * L / 3)
    want = torch.from_numpy(sphere_distance(p.double().numpy()))
    print("longest edge %.4f, sagitta %.5f, max | |sd| - analytic | = %.5f" % (L, sagitta, float((sd.double().abs() - want).abs().max())))
    assert torch.equal(sd < 0, inside) and not bool((sd == 0).any())
    assert bool(((sd.double().abs() - want).abs() <= sagitta + 1e-6).all())
    assert torch.equal(signed_distance(p, *ref.flipped((v, f))), sd.abs())    # wound inward, a mesh contains nothing


# ---- 7. volumetric IoU ----------------------------------------------------------------------------------------------------------
def test_volume_iou_of_two_overlapping_spheres():
    """Two unit icospheres (level 3), centres d = 0.5 apart: lens volume pi (4R + d) (2R - d)^2 / 12.  Bound on the IoU: 4 binomial
    standard deviations at the number of samples in the union, plus the relative volume deficit of the icosphere."""
    from dgs_amd.mesh_metrics import mesh_volume, volume_iou
    v, f = ref.icosphere(3)
    a, b = (v.numpy(), f.numpy()), ((v + torch.tensor([0.5, 0.0, 0.0])).numpy(), f.numpy())
    n = 50_000
    m = volume_iou(a, b, n_samples=n, seed=0, device="cpu")
    assert set(m) == IOU_KEYS and m["iou_samples"] == n and all(isinstance(m[k], float) for k in IOU_KEYS - {"iou_samples"})
    R, d = 1.0, 0.5
    lens, ball = math.pi * (4 * R + d) * (2 * R - d) ** 2 / 12, 4 * math.pi * R ** 3 / 3
    iou = lens / (2 * ball - lens)
    deficit = 1 - mesh_volume(v, f) / ball
    box = 2.5 * 2 * 2
    n_union = round((m["volume_pred"] + m["volume_gt"] - m["volume_intersection"]) / box * n)
    bound = 4 * math.sqrt(iou * (1 - iou) / n_union) + deficit
    print("iou %.5f, closed form %.5f, bound %.5f (union %d samples, deficit %.5f); volumes %s" % (m["iou"], iou, bound, n_union, deficit, m))
    assert 0 < deficit < 0.01 and 20_000 < n_union < 35_000
    assert abs(m["iou"] - iou) <= bound
    for key, vol in (("volume_pred", ball), ("volume_gt", ball), ("volume_intersection", lens)):
        share = vol / box
        assert abs(m[key] - vol) <= box * 4 * math.sqrt(share * (1 - share) / n) + deficit * vol, key
    assert m["iou"] == m["volume_intersection"] / (m["volume_pred"] + m["volume_gt"] - m["volume_intersection"]) or \
        m["iou"] == pytest.approx(m["volume_intersection"] / (m["volume_pred"] + m["volume_gt"] - m["volume_intersection"]), rel=1e-12)


def test_volume_iou_of_a_mesh_with_itself_and_of_disjoint_meshes():
    from dgs_amd.mesh_metrics import volume_iou
    v, f = ref.icosphere(2)
    a, far = (v, f), (v + torch.tensor([3.0, 0.0, 0.0]), f)
    m = volume_iou(a, a, n_samples=2000, seed=1, device="cpu")
    assert m["iou"] == 1.0 and m["volume_pred"] == m["volume_gt"] == m["volume_intersection"] > 0
    m = volume_iou(a, far, n_samples=2000, seed=1, device="cpu")
    assert m["iou"] == 0.0 and m["volume_intersection"] == 0.0 and m["volume_pred"] > 0 and m["volume_gt"] > 0
    shift = np.eye(4)
    shift[:3, 3] = [-3.0, 0.0, 0.0]
    assert volume_iou(a, far, n_samples=2000, seed=1, device="cpu", gt_transform=shift)["iou"] == 1.0
    both_inward = volume_iou(ref.flipped(a), ref.flipped(a), n_samples=500, device="cpu")
    assert both_inward["iou"] == 0.0 and both_inward["volume_pred"] == 0.0     # nothing inside either: the union is empty
    assert volume_iou(a, a, n_samples=2000, seed=1, device="cpu") == volume_iou(a, a, n_samples=2000, seed=1, device="cpu")
    assert volume_iou(a, far, n_samples=2000, seed=2, device="cpu")["volume_pred"] != volume_iou(a, far, n_samples=2000, seed=1, device="cpu")["volume_pred"]


# ---- 8. wiring ------------------------------------------------------------------------------------------------------------------
def _write_pairs(tmp_path):
    """Two tiny pairs: frame_<i>.ply against a .ply and an .obj ground truth."""
    from dgs_amd.io import write_mesh_ply
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    os.makedirs(str(gt))
    gv, gf = ref.icosphere(1)
    for i in range(2):
        v, f = ref.icosphere(1, 1.0 + 0.1 * i)
        write_mesh_ply(str(pred / ("frame_%d.ply" % i)), v.numpy(), f.numpy().astype(np.int32))
    write_mesh_ply(str(gt / "gt0.ply"), gv.numpy(), gf.numpy().astype(np.int32))
    with open(str(gt / "gt1.obj"), "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in gv) + "".join("f %d %d %d\n" % tuple(int(x) + 1 for x in t) for t in gf))
    return str(pred), str(gt)


def test_mesh_distance_with_and_without_iou():
    from dgs_amd.mesh_metrics import mesh_distance, volume_iou
    pred, gt = ref.icosphere(1), ref.icosphere(1, 1.1)
    pred, gt = (pred[0].numpy(), pred[1].numpy()), (gt[0].numpy(), gt[1].numpy())
    kw = dict(n_samples=500, seed=3, thresholds=(0.02, 0.08), device="cpu")
    plain = mesh_distance(pred, gt, **kw)
    assert mesh_distance(pred, gt, iou_samples=0, **kw) == plain and not IOU_KEYS & set(plain)
    assert set(plain) == {"accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall", "fscore", "normal_consistency", "n_samples",
                          "pred_faces", "gt_faces", "pred_vertices", "gt_vertices"}                    # the parent's keys
    with_iou = mesh_distance(pred, gt, iou_samples=400, **kw)
    assert {k: v for k, v in with_iou.items() if k not in IOU_KEYS} == plain and set(with_iou) - set(plain) == IOU_KEYS
    assert {k: with_iou[k] for k in IOU_KEYS} == volume_iou(pred, gt, n_samples=400, seed=3, device="cpu")
    assert with_iou["iou_samples"] == 400 and 0.5 < with_iou["iou"] < 0.95    # (1 / 1.1)^3 = 0.75
    with pytest.raises(ValueError, match="iou_samples"):
        mesh_distance(pred, gt, iou_samples=-1, **kw)


def test_evaluate_meshes_and_cli_with_iou(tmp_path):
    from dgs_amd.mesh_metrics import _parser, evaluate_meshes, main
    pred, gt = _write_pairs(tmp_path)
    kw = dict(n_samples=500, seed=3, thresholds=(0.02, 0.08), device="cpu")
    plain = evaluate_meshes(pred, gt, **kw)
    plain_bytes = open(os.path.join(pred, "mesh_metrics.json"), "rb").read()
    assert evaluate_meshes(pred, gt, iou_samples=0, **kw) == plain and "iou_samples" not in plain["settings"]
    assert open(os.path.join(pred, "mesh_metrics.json"), "rb").read() == plain_bytes
    assert set(plain["settings"]) == {"n_samples", "seed", "thresholds", "device", "mode", "gt_transform"}
    res = evaluate_meshes(pred, gt, iou_samples=400, **kw)
    on_disk = json.load(open(os.path.join(pred, "mesh_metrics.json")))
    assert on_disk == json.loads(json.dumps(res))
    assert set(res["mean"]) == set(plain["mean"]) | IOU_KEYS and all(set(r) == set(p) | IOU_KEYS for r, p in zip(res["frames"], plain["frames"]))
    assert res["settings"] == dict(plain["settings"], iou_samples=400)
    for r, p in zip(res["frames"], plain["frames"]):
        assert {k: v for k, v in r.items() if k not in IOU_KEYS} == p and r["iou_samples"] == 400
    for k in IOU_KEYS:
        assert res["mean"][k] == pytest.approx(sum(r[k] for r in res["frames"]) / 2, rel=1e-12)
    assert res["frames"][0]["iou"] == 1.0 and 0.5 < res["frames"][1]["iou"] < 0.95   # frame 0 is its ground truth, frame 1 is 10 % larger
    assert _parser().parse_args([pred, gt, "--iou", "123"]).iou == 123 and _parser().parse_args([pred, gt]).iou == 0
    os.remove(os.path.join(pred, "mesh_metrics.json"))
    main([pred, gt, "--samples", "500", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu", "--iou", "400"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == on_disk
    main([pred, gt, "--samples", "500", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu"])
    assert open(os.path.join(pred, "mesh_metrics.json"), "rb").read() == plain_bytes


# ---- 9. C ABI -------------------------------------------------------------------------------------------------------------------
def test_winding_sum_refuses_bad_sizes_before_any_launch():
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    err = lib.dgs_mesh_ops_last_error
    lay = (ctypes.c_int * 4)()
    assert lib.dgs_winding_layout(lay) == 0 and all(int(x) > 0 for x in lay) and int(lay[3]) == 12
    assert _mesh_ops.winding_layout() == tuple(int(x) for x in lay)
    Q, T, C, ROW = _mesh_ops.winding_layout()
    assert Q % 256 == 0 and C % T == 0
    host = (ctypes.c_float * 64)()                                            # never dereferenced: every call below is refused first
    table = ctypes.c_void_p((ctypes.addressof(host) + 15) // 16 * 16)
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    pts, out = (ctypes.c_float * 6)(), (ctypes.c_longlong * 2)()
    assert lib.dgs_winding_sum(2, p(pts), 0, table, 1, p(out), None) < 0 and b"n_tri" in err() and b"dgs_winding_sum" in err()
    assert lib.dgs_winding_sum(2, p(pts), 1 << 31, table, 1, p(out), None) < 0 and b"2^31" in err()
    assert lib.dgs_winding_sum(-1, p(pts), 2, table, 1, p(out), None) < 0 and b"n_query" in err()
    assert lib.dgs_winding_sum(2, p(pts), 2, table, 0, p(out), None) < 0 and b"tri_chunk" in err()
    assert lib.dgs_winding_sum(2, p(pts), 2, None, 1, p(out), None) < 0 and b"null" in err()
    assert lib.dgs_winding_sum(2, None, 2, table, 1, p(out), None) < 0 and b"null" in err()
    assert lib.dgs_winding_sum(2, p(pts), 2, table, 1, None, None) < 0 and b"null" in err()
    assert lib.dgs_winding_sum(2, p(pts), 2, ctypes.c_void_p(table.value + 4), 1, p(out), None) < 0 and b"aligned" in err()
    assert lib.dgs_winding_sum(2, p(pts), 65536, table, 1, p(out), None) < 0 and b"65535 slices" in err()
    assert lib.dgs_winding_sum(0, None, 2, table, 1, None, None) == 0         # no queries: nothing to launch
    assert lib.dgs_winding_layout(None) < 0 and b"null" in err()
    assert lib.dgs_mesh_ops_abi_version() == 2
