"""Exact point-to-surface distances on the CPU: the PyTorch statement of dgs_tri_search on closed-form cases (one query per Voronoi
region, faces without area, ties), against a float64 brute force written another way (tests/mesh_surface_ref.py: Ericson's regions)
on random soups and needles, mesh_distance(mode="surface") on the spheres of tests/test_mesh_metrics_cpu.py, the plumbing of the
mode through evaluate_meshes and the CLI, and the argument checks of the C ABI."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_surface_ref as ref
from test_mesh_cpu import fusion_inputs, sphere_box
from test_mesh_metrics_cpu import S_SAMPLES, SPHERE_C, _write_frames, analytic_sphere, concentric_spheres, uv_sphere

KEYS = {"accuracy", "completeness", "chamfer", "chamfer_sq", "precision", "recall", "fscore", "normal_consistency", "n_samples",
        "pred_faces", "gt_faces", "pred_vertices", "gt_vertices"}


# ---- closed-form cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_one_query_per_voronoi_region(dtype):
    from dgs_amd.mesh_metrics import closest_face
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=dtype)
    q = torch.tensor([[0.2, 0.2, 0.5], [-1, -1, 0], [2, -1, 0], [-1, 2, 0], [0.5, -1, 1], [-1, 0.5, 0], [1, 1, 0]], dtype=dtype)
    want = torch.tensor([0.5, math.sqrt(2), math.sqrt(2), math.sqrt(2), math.sqrt(2), 1.0, math.sqrt(0.5)], dtype=torch.float64)
    d2, face = closest_face(q, v, torch.tensor([[0, 1, 2]]))
    assert d2.dtype == dtype and face.dtype == torch.int64 and d2.shape == face.shape == (7,)
    assert torch.equal(face, torch.zeros(7, dtype=torch.int64))
    eps = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -52
    assert float((d2.double().sqrt() - want).abs().max()) <= 4 * eps * 3.0         # coordinates up to 2: a few roundings of size eps * L
    # every corner order of the same triangle gives the same distances
    for perm in ([1, 2, 0], [2, 0, 1], [0, 2, 1]):
        d2_p, _ = closest_face(q, v, torch.tensor([perm]))
        assert float((d2_p.double().sqrt() - want).abs().max()) <= 4 * eps * 3.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_faces_without_area_act_as_their_segments_or_point(dtype):
    from dgs_amd.mesh_metrics import closest_face, triangle_table
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 3, 3]], dtype=dtype)
    d2, _ = closest_face(torch.tensor([[1, 1, 0]], dtype=dtype), v, torch.tensor([[0, 1, 2]]))
    assert float(d2) == 1.0
    d2, _ = closest_face(torch.tensor([[3, 3, 4]], dtype=dtype), v, torch.tensor([[3, 3, 3]]))
    assert float(d2) == 1.0
    dv, df, dp, want = ref.degenerates()
    table = triangle_table(dv.to(dtype), df)
    assert table.shape == (5, 36) and table.dtype == dtype and not bool(torch.isnan(table).any())
    assert torch.equal(table[:4, 33], torch.zeros(4, dtype=dtype)) and float(table[4, 33]) == 1.0           # rn
    assert float(table[1, 30:33].abs().max()) == 0.0 and float(table[2, 30]) == 0.0 and float(table[3, 31]) == 0.0   # r_k of empty edges
    d2, face = closest_face(dp.to(dtype), dv.to(dtype), df)
    assert not bool(torch.isnan(d2).any())
    assert torch.equal(d2.double().sqrt(), want) and torch.equal(face, torch.tensor([0, 1, 2, 2, 3, 3, 0]))


def test_equal_distances_go_to_the_lowest_face():
    from dgs_amd.mesh_metrics import closest_face
    v, f = ref.soup(40, 3)
    pick = torch.tensor([7, 3, 7, 12, 3, 7])
    q = ref.queries(60, 4, v, f[pick])
    d2, face = closest_face(q, v, f[pick])
    first = {7: 0, 3: 1, 12: 3}
    d2_u, face_u = closest_face(q, v, f[torch.tensor([7, 3, 12])])
    assert torch.equal(d2, d2_u)
    assert torch.equal(face, torch.tensor([first[[7, 3, 12][int(i)]] for i in face_u]))
    d2, face = closest_face(q, v, f[torch.tensor([5, 5, 5])])
    assert torch.equal(face, torch.zeros(60, dtype=torch.int64))


def test_the_row_length_is_the_kernels():
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import TRI_ROW, TRI_VALUES
    lay = (ctypes.c_int * 4)()
    lib = _mesh_ops.load()
    assert lib.dgs_tri_layout(lay) == 0 and all(int(x) > 0 for x in lay)
    assert _mesh_ops.tri_layout() == tuple(int(x) for x in lay)
    assert lay[3] == TRI_ROW and TRI_VALUES == 34 and TRI_ROW % 4 == 0 and TRI_ROW >= TRI_VALUES
    assert lay[1] * lay[3] * 4 <= 64 * 1024                      # a round fits the LDS a workgroup may always claim


# ---- against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_statement_against_float64_brute_force(which):
    """fp32 statement against Ericson's regions in float64: |d32 - d64(face)| <= C 2^-24 L kappa and d64(face) <= min64 + the two
    faces' tolerances; and the constant measured over ALL pairs of the set is within the recorded C_MEASURED (C is four times it)."""
    from dgs_amd.mesh_metrics import closest_face
    name, p, v, f = ref.cpu_sets()[which]
    d2, face = closest_face(p, v, f)
    assert d2.dtype == torch.float32 and not bool(torch.isnan(d2).any()) and int(face.min()) >= 0 and int(face.max()) < f.shape[0]
    d64, unit = ref.brute_force64(p, v, f)
    ref.check_against_float64(d2, face, d64, unit, name)
    measured = ref.measure_c(p, v, f)
    print("%s: constant over all %d pairs %.3f (recorded largest %.2f)" % (name, d64.numel(), measured, ref.C_MEASURED))
    assert measured <= ref.C_MEASURED
    # float64 tensors run in float64 and agree with the brute force to float64 accuracy
    d2_64, face_64 = closest_face(p.double(), v.double(), f)
    at = d64.gather(1, face_64[:, None])[:, 0]
    assert d2_64.dtype == torch.float64
    assert bool(((d2_64.sqrt() - at).abs() <= 1e-7 * unit.gather(1, face_64[:, None])[:, 0]).all())


def test_closest_face_refuses_bad_input():
    from dgs_amd.mesh_metrics import closest_face
    v, f = ref.soup(5, 1)
    q = ref.queries(9, 2, v, f)
    with pytest.raises(ValueError, match="no faces"):
        closest_face(q, v, f[:0])
    bad = q.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        closest_face(bad, v, f)
    bad = v.clone()
    bad[0, 0] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        closest_face(q, bad, f)
    with pytest.raises(ValueError, match="outside"):
        closest_face(q, v[:10], f)
    with pytest.raises(ValueError):
        closest_face(q, v, f.float())
    d2, face = closest_face(q[:0], v, f)
    assert d2.shape == (0,) and face.shape == (0,) and face.dtype == torch.int64


# ---- the metric -----------------------------------------------------------------------------------------------------------------
def test_samples_mode_is_the_default_and_unchanged():
    from dgs_amd.mesh_metrics import mesh_distance
    inner, outer = (uv_sphere(r, SPHERE_C, 16, 8) for r in (1.0, 1.1))
    a = mesh_distance(inner, outer, n_samples=700, seed=2, device="cpu")
    b = mesh_distance(inner, outer, n_samples=700, seed=2, device="cpu", mode="samples")
    assert a == b and set(a) == KEYS
    c = mesh_distance(inner, outer, n_samples=700, seed=2, device="cpu", mode="surface")
    assert set(c) == KEYS and c != a and c["accuracy"] < a["accuracy"]
    with pytest.raises(ValueError, match="mode"):
        mesh_distance(inner, outer, n_samples=10, device="cpu", mode="exact")


def test_sphere_against_itself_measures_zero():
    """Samples mode measures the floor 0.0125 here (tests/test_mesh_metrics_cpu.py); the surface mode measures the rounding of a
    point that lies on a face: below 1e-5."""
    from dgs_amd.mesh_metrics import mesh_distance
    sphere = uv_sphere(1.0, SPHERE_C)
    m = mesh_distance(sphere, sphere, n_samples=S_SAMPLES, seed=0, thresholds=(0.005,), device="cpu", mode="surface")
    print(json.dumps(m))
    assert 0.0 <= m["accuracy"] < 1e-5 and 0.0 <= m["completeness"] < 1e-5
    assert m["precision"]["0.005"] == 1.0 and m["recall"]["0.005"] == 1.0 and m["fscore"]["0.005"] == 1.0
    assert m["normal_consistency"] > 0.999
    assert m["n_samples"] == S_SAMPLES and m["pred_faces"] == m["gt_faces"] == 2 * 64 * 31


def _shell():
    """[rho_out - 1, 1.1 - rho_in] of the concentric spheres, rho the smallest float64 distance from the centre to a mesh, and the
    fp32 slack of one distance: C 2^-24 L kappa with L <= 2.2 and the largest kappa of the two meshes."""
    inner, outer = concentric_spheres()
    centre = torch.tensor([SPHERE_C], dtype=torch.float64)
    rho, kappa = [], 0.0
    for v, f in (inner, outer):
        v, f = torch.from_numpy(v).double(), torch.from_numpy(f).long()
        d64, unit = ref.brute_force64(centre, v, f)
        rho.append(float(d64.min()))
        kappa = max(kappa, float((unit / (ref.U32 * (v[f] - centre).norm(dim=-1).max(dim=1).values)).max()))
    return rho[1] - 1.0, 1.1 - rho[0], ref.C * ref.U32 * 2.2 * kappa


def test_concentric_spheres_lie_in_their_shell():
    """A radial ray from a point of one sphere reaches the other, star-shaped surface inside its shell, so every directed distance
    lies in [rho_out - 1, 1.1 - rho_in]; the F-score is exactly 0 below that interval and exactly 1 above it."""
    from dgs_amd.mesh_metrics import closest_face, mesh_distance, sample_surface
    inner, outer = concentric_spheres()
    lo, hi, slack = _shell()
    S = S_SAMPLES // 4
    print("shell [%.6f, %.6f], slack %.2e" % (lo, hi, slack))
    assert 0.09 < lo < 0.1 < hi < 0.11 and slack < 1e-4
    t = lambda m: (torch.from_numpy(m[0]), torch.from_numpy(m[1]).long())
    (iv, jf), (ov, of) = t(inner), t(outer)
    pp, _, _ = sample_surface(iv, jf, S, 0)
    gp, _, _ = sample_surface(ov, of, S, 1)
    for pts, v, f in ((pp, ov, of), (gp, iv, jf)):
        d = closest_face(pts, v, f)[0].double().sqrt()
        print("directed distances %.6f ... %.6f" % (float(d.min()), float(d.max())))
        assert float(d.min()) >= lo - slack and float(d.max()) <= hi + slack
    below, above = lo - 2 * slack, hi + 2 * slack
    m = mesh_distance(inner, outer, n_samples=S, seed=0, thresholds=(below, above), device="cpu", mode="surface")
    kb, ka = "%g" % below, "%g" % above
    assert m["precision"][kb] == 0.0 and m["recall"][kb] == 0.0 and m["fscore"][kb] == 0.0
    assert m["precision"][ka] == 1.0 and m["recall"][ka] == 1.0 and m["fscore"][ka] == 1.0
    assert lo - slack <= m["accuracy"] <= hi + slack and lo - slack <= m["completeness"] <= hi + slack
    assert m["chamfer"] == m["accuracy"] + m["completeness"] and m["normal_consistency"] > 0.999


def test_fused_sphere_against_the_analytic_sphere_without_the_floor():
    """tests/test_mesh_cpu.py's fused sphere (N = 96, 24 views) against the UV sphere of the true radius and centre at S = 2000
    samples (the CPU statement stays at seconds): the surface mode's accuracy is below the samples mode's and below one voxel.
    Measured: accuracy 0.000612, completeness 0.000613 = 0.036 h, where the samples mode reads 0.0216 at this S (0.00694 at
    S = 20 000, nearly all of it the sampling floor)."""
    from dgs_amd.mesh import TSDFVolume
    from dgs_amd.mesh_metrics import mesh_distance
    N, S = 96, 2000
    origin, h = sphere_box(N)
    depth, rgb, proj = fusion_inputs(24, 200)
    vol = TSDFVolume(origin, h, (N, N, N), "cpu").integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    v, f, _ = vol.extract()
    gt = analytic_sphere()
    surface = mesh_distance((v, f), gt, n_samples=S, seed=0, device="cpu", mode="surface")
    samples = mesh_distance((v, f), gt, n_samples=S, seed=0, device="cpu")
    print("fused sphere vs analytic, S = %d, h = %.6f: surface mode accuracy %.6f completeness %.6f fscore %s normal consistency %.4f; "
          "samples mode accuracy %.6f completeness %.6f" % (S, vol.voxel_size, surface["accuracy"], surface["completeness"], surface["fscore"],
                                                            surface["normal_consistency"], samples["accuracy"], samples["completeness"]))
    assert surface["accuracy"] < samples["accuracy"] and surface["accuracy"] < vol.voxel_size
    assert surface["completeness"] < samples["completeness"] and surface["completeness"] < vol.voxel_size
    assert set(surface) == set(samples) == KEYS


def test_zero_area_faces_are_dropped_from_the_searched_mesh():
    """A mesh with zero-area faces sprinkled in measures what the mesh without them measures, and every hit has a normal."""
    from dgs_amd.mesh_metrics import mesh_distance
    v, f = uv_sphere(1.0, SPHERE_C, 16, 8)
    junk = np.array([[0, 0, 5], [3, 3, 3], [7, 9, 7]], np.int32)
    dirty = (v, np.concatenate([junk[:1], f[:50], junk[1:], f[50:]]))
    a = mesh_distance((v, f), (v * np.float32(1.05), f), n_samples=800, device="cpu", mode="surface")
    b = mesh_distance(dirty, (v * np.float32(1.05), dirty[1]), n_samples=800, device="cpu", mode="surface")
    assert math.isfinite(b["normal_consistency"])
    for k in ("accuracy", "completeness", "chamfer", "chamfer_sq", "normal_consistency", "precision", "recall", "fscore"):
        assert a[k] == b[k], k


def test_evaluate_meshes_and_cli_record_the_mode(tmp_path):
    from dgs_amd.mesh_metrics import evaluate_meshes, main
    pred, gt = _write_frames(tmp_path, 3)
    samples = evaluate_meshes(pred, gt, n_samples=1500, seed=3, thresholds=(0.02, 0.08), device="cpu")
    assert samples["settings"]["mode"] == "samples"
    res = evaluate_meshes(pred, gt, n_samples=1500, seed=3, thresholds=(0.02, 0.08), device="cpu", mode="surface")
    on_disk = json.load(open(os.path.join(pred, "mesh_metrics.json")))
    assert on_disk == json.loads(json.dumps(res)) and res["settings"]["mode"] == "surface"
    assert set(res["settings"]) == set(samples["settings"]) and set(res["mean"]) == set(samples["mean"])
    assert all(set(r) == set(s) for r, s in zip(res["frames"], samples["frames"]))
    acc = [r["accuracy"] for r in res["frames"]]
    assert acc[0] < 1e-5 and abs(acc[1] - 0.05) < 0.01 and abs(acc[2] - 0.1) < 0.01      # frame i is a sphere of radius 1 + 0.05 i
    assert all(r["accuracy"] < s["accuracy"] for r, s in zip(res["frames"], samples["frames"]))
    os.remove(os.path.join(pred, "mesh_metrics.json"))
    main([pred, gt, "--samples", "1500", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu", "--mode", "surface"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == on_disk
    main([pred, gt, "--samples", "1500", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == json.loads(json.dumps(samples))


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_tri_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    assert lib.dgs_mesh_ops_abi_version() == 2
    raw = (ctypes.c_float * (2 * 36 + 8))()
    base = ctypes.addressof(raw)
    table = ctypes.c_void_p(base + (-base) % 16)                    # a 16-byte aligned table of two rows inside `raw`
    pts = (ctypes.c_float * 6)()
    out = (ctypes.c_ulonglong * 2)()
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    err = lib.dgs_mesh_ops_last_error
    assert lib.dgs_tri_search(2, p(pts), 0, table, 1, p(out), None) < 0 and b"n_tri" in err()
    assert lib.dgs_tri_search(2, p(pts), 1 << 31, table, 1, p(out), None) < 0 and b"2^31" in err()
    assert lib.dgs_tri_search(-1, p(pts), 2, table, 1, p(out), None) < 0 and b"n_query" in err()
    assert lib.dgs_tri_search(2, p(pts), 2, table, 0, p(out), None) < 0 and b"tri_chunk" in err()
    assert lib.dgs_tri_search(2, p(pts), 2, None, 1, p(out), None) < 0 and b"null" in err()
    assert lib.dgs_tri_search(2, None, 2, table, 1, p(out), None) < 0 and b"null" in err()
    assert lib.dgs_tri_search(2, p(pts), 2, table, 1, None, None) < 0 and b"null" in err()
    assert lib.dgs_tri_search(2, p(pts), 2, ctypes.c_void_p(table.value + 4), 1, p(out), None) < 0 and b"aligned" in err()
    assert lib.dgs_tri_search(2, p(pts), 65536, table, 1, p(out), None) < 0 and b"65535 slices" in err()
    assert lib.dgs_tri_search(0, None, 2, table, 1, None, None) == 0           # no queries: nothing to launch
    assert lib.dgs_tri_layout(None) < 0 and b"null" in err()
