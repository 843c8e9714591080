"""Mesh geometry metrics on the CPU: the PyTorch statement of the nearest-neighbour search against a float64 brute force, the
surface sampler, Chamfer / F-score / normal consistency on spheres whose distances are known, the OBJ reader, evaluate_meshes and
the argument checks of the C ABI.  The helpers here (uv_sphere, brute_force64, concentric_spheres, the cached CPU results) are
also what tests/test_mesh_metrics_gpu.py compares the HIP path with."""
import ctypes
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from test_mesh_cpu import C_S, R_S, fusion_inputs, sphere_box

S_SAMPLES = 20_000
SPHERE_C = (0.1, -0.2, 0.3)
U32 = 2.0 ** -24          # unit roundoff of fp32


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def uv_sphere(radius, centre, nu=64, nv=32):
    """(vertices [2 + nu (nv - 1), 3] float32, faces [2 nu (nv - 1), 3] int32), normals outward: nu segments around, nv pole to pole."""
    th = np.pi * np.arange(1, nv) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.broadcast_to(np.cos(th)[:, None], (nv - 1, nu))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * radius + np.asarray(centre, np.float64)
    rid = lambda j, i: 1 + j * nu + (i % nu)
    south = 1 + nu * (nv - 1)
    f = []
    for i in range(nu):
        f.append((0, rid(0, i), rid(0, i + 1)))
        for j in range(nv - 2):
            f.append((rid(j, i), rid(j + 1, i), rid(j + 1, i + 1)))
            f.append((rid(j, i), rid(j + 1, i + 1), rid(j, i + 1)))
        f.append((south, rid(nv - 2, i + 1), rid(nv - 2, i)))
    return v.astype(np.float32), np.asarray(f, np.int32)


def mesh_area(v, f):
    p = np.asarray(v, np.float64)[np.asarray(f, np.int64)]
    return float(0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1).sum())


def brute_force64(query, ref, chunk=512):
    """Squared distances in float64 of the given (fp32) points -> (min d2 [Nq], second smallest d2 [Nq] (inf if Nr = 1), d2 of
    every pair as a function idx -> d2(q, idx)).  Chunked over the queries."""
    q, r = query.detach().cpu().double(), ref.detach().cpu().double()
    mins, seconds = [], []
    for s in range(0, q.shape[0], chunk):
        d = ((q[s:s + chunk, None, :] - r[None, :, :]) ** 2).sum(-1)
        two = torch.topk(d, min(2, r.shape[0]), dim=1, largest=False).values
        mins.append(two[:, 0])
        seconds.append(two[:, 1] if r.shape[0] > 1 else torch.full_like(two[:, 0], float("inf")))
    at = lambda idx: ((q - r[idx.cpu()]) ** 2).sum(-1)
    cat = lambda xs: torch.cat(xs) if xs else torch.zeros(0, dtype=torch.float64)
    return cat(mins), cat(seconds), at


def cloud(n, seed, cluster=0.25):
    """n points in [-1, 1]^3, a share of them in a tight cluster (radius 1e-3) around (0.5, -0.25, 0.125)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, 3, generator=g) * 2 - 1
    k = int(n * cluster)
    if k:
        p[:k] = torch.tensor([0.5, -0.25, 0.125]) + (torch.rand(k, 3, generator=g) * 2 - 1) * 1e-3
    return p[torch.randperm(n, generator=g)].contiguous()


def concentric_spheres():
    return uv_sphere(1.0, SPHERE_C), uv_sphere(1.1, SPHERE_C)


@functools.lru_cache(maxsize=None)
def concentric_cpu(n_samples=S_SAMPLES):
    """mesh_distance of the two spheres on the CPU path, computed once per sample count for the tests of both files."""
    from dgs_amd.mesh_metrics import mesh_distance
    inner, outer = concentric_spheres()
    return mesh_distance(inner, outer, n_samples=n_samples, seed=0, thresholds=(0.05, 0.15), device="cpu")


def fused_sphere_bound(h):
    """h + sqrt(A / S): every vertex of the fused mesh lies within one voxel of the sphere (tests/test_mesh_cpu.py), and sqrt(A / S)
    is twice the expected spacing 0.5 sqrt(A / S) of S samples on a surface of area A."""
    return h + math.sqrt(4 * math.pi * R_S ** 2 / S_SAMPLES)


def analytic_sphere():
    return uv_sphere(R_S, C_S, 128, 64)


# ---- nearest --------------------------------------------------------------------------------------------------------------------
def test_nearest_torch_against_float64_brute_force():
    from dgs_amd.mesh_metrics import nearest
    q, r = cloud(700, 1), cloud(900, 2)
    d2, idx = nearest(q, r)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int64 and d2.shape == idx.shape == (700,)
    m, second, at = brute_force64(q, r)
    unique = second > m * (1 + 1e-5)
    excluded = 1.0 - float(unique.double().mean())
    print("excluded (float64 minimum not unique by 1e-5): %.4f" % excluded)
    assert excluded <= 0.01
    i64 = ((q.double()[:, None, :] - r.double()[None, :, :]) ** 2).sum(-1).argmin(1)
    assert torch.equal(idx[unique], i64[unique])
    d_at = at(idx)
    assert bool(((d2.double() - d_at).abs() <= 6 * U32 * d_at).all()) and bool((d_at <= m * (1 + 12 * U32)).all())
    # float64 tensors run in float64
    d2_64, idx_64 = nearest(q.double(), r.double())
    assert d2_64.dtype == torch.float64 and torch.equal(idx_64[unique], i64[unique])


def test_nearest_ties_go_to_the_lowest_index():
    from dgs_amd.mesh_metrics import nearest
    g = torch.Generator().manual_seed(3)
    base = torch.rand(40, 3, generator=g)
    group = torch.cat([torch.randperm(40, generator=g), torch.randint(0, 40, (200,), generator=g)])
    group = group[torch.randperm(240, generator=g)]
    ref = base[group].contiguous()
    expected = torch.tensor([int(torch.nonzero(group == i)[0]) for i in range(40)])
    assert int((torch.bincount(group) > 1).sum()) > 30
    d2, idx = nearest(base, ref)
    assert torch.equal(d2, torch.zeros(40)) and torch.equal(idx, expected)
    # ... and off the points themselves: equal distances to all copies of the nearest point
    d2, idx = nearest(base + 1e-4, ref)
    assert torch.equal(idx, expected)


def test_nearest_edge_sizes():
    from dgs_amd.mesh_metrics import nearest
    q, r = cloud(5, 4), cloud(7, 5)
    d2, idx = nearest(q, r[:1])
    assert torch.equal(idx, torch.zeros(5, dtype=torch.int64))
    d = q - r[:1]
    assert torch.equal(d2, d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    d2, idx = nearest(q[:1], r)
    assert d2.shape == (1,) and int(idx) == int(((q[:1].double() - r.double()) ** 2).sum(-1).argmin())
    d2, idx = nearest(q[:0], r)
    assert d2.shape == (0,) and idx.shape == (0,) and idx.dtype == torch.int64
    with pytest.raises(ValueError):
        nearest(q, r[:0])
    bad = q.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError):
        nearest(bad, r)
    with pytest.raises(ValueError):
        nearest(q, torch.full((3, 3), float("inf")))


# ---- sample_surface -------------------------------------------------------------------------------------------------------------
def _barycentrics(p, a, b, c):
    """Float64 barycentric coordinates of the projection of p into the plane of (a, b, c), and the distance to that plane."""
    e0, e1, w = b - a, c - a, p - a
    n = np.cross(e0, e1)
    nn = (n * n).sum(-1)
    l1 = (np.cross(w, e1) * n).sum(-1) / nn
    l2 = (np.cross(e0, w) * n).sum(-1) / nn
    return np.stack([1 - l1 - l2, l1, l2], -1), np.abs((w * n).sum(-1)) / np.sqrt(nn)


def test_sample_surface_is_deterministic_and_lies_in_its_faces():
    from dgs_amd.mesh_metrics import sample_surface
    v, f = uv_sphere(0.7, (0.3, 0.1, -0.2), 16, 8)
    v, f = torch.from_numpy(v), torch.from_numpy(f)
    p, fid, nrm = sample_surface(v, f, 5000, 7)
    assert p.dtype == torch.float32 and fid.dtype == torch.int64 and nrm.dtype == torch.float32
    assert p.shape == (5000, 3) and fid.shape == (5000,) and nrm.shape == (5000, 3)
    p2, fid2, nrm2 = sample_surface(v, f, 5000, 7)
    assert torch.equal(p, p2) and torch.equal(fid, fid2) and torch.equal(nrm, nrm2)
    p3, fid3, _ = sample_surface(v, f, 5000, 8)
    assert not torch.equal(p, p3) and not torch.equal(fid, fid3)
    tri = v.double().numpy()[f.long().numpy()[fid.numpy()]]
    bary, dist = _barycentrics(p.double().numpy(), tri[:, 0], tri[:, 1], tri[:, 2])
    print("min barycentric %.3e, max plane distance %.3e" % (bary.min(), dist.max()))
    assert bary.min() >= -1e-6 and dist.max() <= 1e-6
    n64 = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(nrm.numpy() - n64).max() <= 1e-6
    assert ((p.double().numpy() - np.array([0.3, 0.1, -0.2])) * n64).sum(-1).min() > 0        # outward
    assert int(torch.unique(fid).numel()) == f.shape[0]                                         # every face is drawn at this count


def test_sample_surface_is_area_weighted_and_skips_zero_area_faces():
    from dgs_amd.mesh_metrics import sample_surface
    # face 0: area 4.5; face 1: no area (two corners coincide); face 2: area 0.5; face 3: no area (collinear), the last one
    v = torch.tensor([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [5.0, 0.0, 1.0], [6.0, 0.0, 1.0], [5.0, 1.0, 1.0], [7.0, 0.0, 1.0]])
    f = torch.tensor([[0, 1, 2], [0, 1, 1], [3, 4, 5], [3, 4, 6]])
    n = 20_000
    _, fid, _ = sample_surface(v, f, n, 0)
    counts = torch.bincount(fid, minlength=4).tolist()
    sigma = math.sqrt(n * 0.9 * 0.1)
    print("draws per face:", counts, "expected %d +- %.0f" % (0.9 * n, 4 * sigma))
    assert counts[1] == 0 and counts[3] == 0 and counts[0] + counts[2] == n
    assert abs(counts[0] - 0.9 * n) <= 4 * sigma
    with pytest.raises(ValueError):
        sample_surface(v, f[[1, 3]], 10, 0)          # total area 0
    with pytest.raises(ValueError):
        sample_surface(v, f[:0], 10, 0)              # no faces


# ---- spheres --------------------------------------------------------------------------------------------------------------------
def test_two_concentric_spheres():
    """Radii 1.0 and 1.1: both directed means lie between the faceted outer sphere's inradius minus 1 (0.0995) and sqrt(0.1^2 +
    spacing^2) with twice the sample spacing (0.103).  A torch prototype of the sampler gave 0.10090 / 0.10092."""
    m = concentric_cpu()
    print(json.dumps(m))
    assert 0.0995 <= m["accuracy"] <= 0.103 and 0.0995 <= m["completeness"] <= 0.103
    assert m["chamfer"] == m["accuracy"] + m["completeness"]
    assert 2 * 0.0995 ** 2 <= m["chamfer_sq"] <= 2 * 0.1114 ** 2
    assert m["precision"]["0.05"] == 0.0 and m["recall"]["0.05"] == 0.0 and m["fscore"]["0.05"] == 0.0
    assert m["precision"]["0.15"] == 1.0 and m["recall"]["0.15"] == 1.0 and m["fscore"]["0.15"] == 1.0
    assert m["normal_consistency"] >= 0.99
    assert m["n_samples"] == S_SAMPLES and m["pred_faces"] == m["gt_faces"] == 2 * 64 * 31 and m["pred_vertices"] == 2 + 64 * 31


def test_sphere_against_itself_measures_the_sampling_floor():
    """Two independent uniform samplings (seed, seed + 1) of S points on a surface of area A: the expected distance from a point to
    the nearest of S uniform points in the plane is 0.5 sqrt(A / S).  Prototype at S = 20 000: 0.012549 / 0.012513 against 0.012533."""
    from dgs_amd.mesh_metrics import mesh_distance
    sphere = uv_sphere(1.0, SPHERE_C)
    m = mesh_distance(sphere, sphere, n_samples=S_SAMPLES, seed=0, thresholds=(0.05,), device="cpu")
    floor = 0.5 * math.sqrt(mesh_area(*sphere) / S_SAMPLES)
    print("accuracy %.6f, completeness %.6f, floor %.6f" % (m["accuracy"], m["completeness"], floor))
    assert abs(m["accuracy"] - floor) <= 0.05 * floor and abs(m["completeness"] - floor) <= 0.05 * floor
    assert m["fscore"]["0.05"] == 1.0 and m["normal_consistency"] >= 0.99


def test_gt_transform_moves_the_ground_truth():
    from dgs_amd.mesh_metrics import mesh_distance
    inner = uv_sphere(1.0, SPHERE_C, 16, 8)
    moved = (inner[0] - np.float32(2.0), inner[1])
    shift = np.eye(4)
    shift[:3, 3] = 2.0
    a = mesh_distance(inner, inner, n_samples=500, device="cpu")
    b = mesh_distance(inner, moved, n_samples=500, device="cpu", gt_transform=shift)
    assert abs(a["chamfer"] - b["chamfer"]) <= 1e-5 and mesh_distance(inner, moved, n_samples=500, device="cpu")["accuracy"] > 1.0


def test_fused_sphere_against_the_analytic_sphere():
    """The mesh of tests/test_mesh_cpu.py's fused sphere (N = 96, 24 views) against a UV sphere of the true radius and centre: both
    directed means <= h + sqrt(A / S) (fused_sphere_bound)."""
    from dgs_amd.mesh import TSDFVolume
    from dgs_amd.mesh_metrics import mesh_distance
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = fusion_inputs(24, 200)
    vol = TSDFVolume(origin, h, (N, N, N), "cpu").integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    v, f, _ = vol.extract()
    m = mesh_distance((v, f), analytic_sphere(), n_samples=S_SAMPLES, seed=0, thresholds=(0.005, 0.01, 0.02), device="cpu")
    bound = fused_sphere_bound(vol.voxel_size)
    print("fused sphere vs analytic: accuracy %.6f, completeness %.6f (bound %.6f, h %.6f), fscore %s, normal consistency %.4f"
          % (m["accuracy"], m["completeness"], bound, vol.voxel_size, m["fscore"], m["normal_consistency"]))
    assert m["accuracy"] <= bound and m["completeness"] <= bound


# ---- files ----------------------------------------------------------------------------------------------------------------------
OBJ_TEXT = """# a comment
mtllib nothing.mtl
o thing
v 0 0 0
v 1.5 0 0 0.25
v 1.5 2.5e-1 0
v 0 1 -3
vt 0.5 0.5
vn 0 0 1
f 1/1/1 2/1/1 3/1/1
# a quad, then a face with relative indices
f 1//1 2//1 3//1 4//1
v 9 9 9
f -1 -2/1 1/1/1
f 1 3 5
"""


def test_read_mesh_obj(tmp_path):
    from dgs_amd.io import read_mesh_obj, write_mesh_ply
    from dgs_amd.mesh_metrics import read_mesh
    path = str(tmp_path / "m.obj")
    open(path, "w").write(OBJ_TEXT)
    v, f = read_mesh_obj(path)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v, np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 0.25, 0], [0, 1, -3], [9, 9, 9]], np.float32))
    assert np.array_equal(f, np.array([[0, 1, 2], [0, 1, 2], [0, 2, 3], [4, 3, 0], [0, 2, 4]], np.int32))
    v2, f2 = read_mesh(path)
    assert np.array_equal(v, v2) and np.array_equal(f, f2)
    ply = str(tmp_path / "m.ply")
    write_mesh_ply(ply, v, f, np.full((5, 3), 0.5))
    v3, f3 = read_mesh(ply)
    assert np.array_equal(v, v3) and np.array_equal(f, f3) and f3.dtype == np.int32
    with pytest.raises(ValueError):
        read_mesh(str(tmp_path / "m.stl"))
    open(path, "w").write("v 0 0 0\nv 1 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        read_mesh_obj(path)


def test_read_mesh_obj_against_the_reference_reader(tmp_path):
    """tests/golden/obj_golden.npz: a triangle-only OBJ (its text is stored) and what the reference's load_obj made of it."""
    from dgs_amd.io import read_mesh_obj
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj_golden.npz"))
    path = str(tmp_path / "golden.obj")
    open(path, "wb").write(g["obj_text"].tobytes())
    v, f = read_mesh_obj(path)
    assert g["vertices"].shape[0] > 10 and g["faces"].shape[0] > 10
    assert np.array_equal(v, g["vertices"].astype(np.float32)) and np.array_equal(f, g["faces"])


def _write_frames(tmp_path, n):
    from dgs_amd.io import write_mesh_ply
    pred, gt = tmp_path / "pred", tmp_path / "gt"
    os.makedirs(str(gt))
    for i in range(n):
        v, f = uv_sphere(1.0 + 0.05 * i, SPHERE_C, 16, 8)
        write_mesh_ply(str(pred / ("frame_%d.ply" % i)), v, f)
        gv, gf = uv_sphere(1.0, SPHERE_C, 16, 8)
        # natural order: mesh2 < mesh10; the second one is an OBJ
        name = ["mesh2.ply", "mesh10.obj", "mesh11.ply"][i]
        if name.endswith(".obj"):
            with open(str(gt / name), "w") as fh:
                fh.write("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in gv) + "".join("f %d %d %d\n" % tuple(int(x) + 1 for x in t) for t in gf))
        else:
            write_mesh_ply(str(gt / name), gv, gf)
    return str(pred), str(gt)


def test_evaluate_meshes_and_cli(tmp_path):
    from dgs_amd.mesh_metrics import evaluate_meshes, main
    pred, gt = _write_frames(tmp_path, 3)
    res = evaluate_meshes(pred, gt, n_samples=2000, seed=3, thresholds=(0.02, 0.08), device="cpu")
    on_disk = json.load(open(os.path.join(pred, "mesh_metrics.json")))
    assert on_disk == json.loads(json.dumps(res))
    assert [r["frame"] for r in res["frames"]] == [0, 1, 2] and [r["gt"] for r in res["frames"]] == ["mesh2.ply", "mesh10.obj", "mesh11.ply"]
    keys = {"accuracy", "completeness", "chamfer", "chamfer_sq", "normal_consistency", "precision@0.02", "recall@0.02", "fscore@0.02",
            "precision@0.08", "recall@0.08", "fscore@0.08", "n_samples", "pred_faces", "gt_faces", "pred_vertices", "gt_vertices"}
    assert set(res["mean"]) == keys and all(set(r) == keys | {"frame", "pred", "gt"} for r in res["frames"])
    for k in keys:
        assert res["mean"][k] == pytest.approx(sum(r[k] for r in res["frames"]) / 3, rel=1e-12)
    acc = [r["accuracy"] for r in res["frames"]]
    assert acc[0] < acc[1] < acc[2] and abs(acc[2] - 0.1) < 0.02          # the frames were paired with their own ground truth
    assert res["settings"]["n_samples"] == 2000 and res["settings"]["thresholds"] == [0.02, 0.08]
    os.remove(os.path.join(pred, "mesh_metrics.json"))
    main([pred, gt, "--samples", "2000", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == on_disk
    os.remove(os.path.join(gt, "mesh11.ply"))
    with pytest.raises(ValueError, match=r"3 frame.*2 ground-truth"):
        evaluate_meshes(pred, gt, n_samples=100, device="cpu")


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_nn_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    assert lib.dgs_mesh_ops_abi_version() == 2
    buf = (ctypes.c_float * 6)()
    out = (ctypes.c_ulonglong * 2)()
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    assert lib.dgs_nn_search(2, p(buf), 0, p(buf), 1, p(out), None) < 0
    assert b"n_ref" in lib.dgs_mesh_ops_last_error()
    assert lib.dgs_nn_search(2, p(buf), 2, p(buf), 0, p(out), None) < 0
    assert b"ref_chunk" in lib.dgs_mesh_ops_last_error()
    assert lib.dgs_nn_search(2, p(buf), 2, None, 1, p(out), None) < 0
    assert b"null" in lib.dgs_mesh_ops_last_error()
    assert lib.dgs_nn_search(2, None, 2, p(buf), 1, p(out), None) < 0
    assert lib.dgs_nn_search(-1, p(buf), 2, p(buf), 1, p(out), None) < 0
    assert lib.dgs_nn_search(2, p(buf), 1 << 31, p(buf), 1, p(out), None) < 0
    assert b"2^31" in lib.dgs_mesh_ops_last_error()
    assert lib.dgs_nn_search(0, None, 2, p(buf), 1, None, None) == 0            # no queries: nothing to launch
    lay = (ctypes.c_int * 3)()
    assert lib.dgs_nn_layout(lay) == 0 and all(int(x) > 0 for x in lay)
    assert _mesh_ops.nn_layout() == tuple(int(x) for x in lay)
