"""Times of mesh simplification on a device-extracted mesh of about 10^6 faces -> profiles/mesh_simplify_timing.json.

    python tools/mesh_simplify_timing.py [--grid 288] [--cells 2 3] [--reps 10] [--samples 100000] [--pixels 800] [--out ...]

The mesh is the analytic sphere |p| = 0.9 in a volume of --grid^3 points over [-1.3, 1.3]^3, extracted by the HIP marching
tetrahedra (its vertices and faces come in cell order, as every extracted frame's do).  For every cell size (in voxels), timed with
device events after a warm-up of each:
  accumulate_vertices   dgs_simplify_accumulate without faces: the clear and the vertex launch
  accumulate            dgs_simplify_accumulate: the clear, the vertex launch and the face launch (faces = the difference)
  solve                 dgs_simplify_solve
  simplify_mesh         the whole function: cells (a sort), the launches, the faces, the compaction
  statement             the baseline: the same sums and the same solve written with index_add_ (mesh_simplify._accumulate_torch and
                        _solve_torch) on the same device, alternating with the kernels; results compared bit for bit
and downstream, on the original and on the simplified mesh: mesh_distance(mode="surface") against the original mesh, and
render_mesh from one camera."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def measure(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms, out = [], None
    for _ in range(reps):
        t, out = timed(fn)
        ms.append(t)
    return stats(ms), out


def sphere_mesh(N, dev):
    from dgs_amd.mesh import TSDFVolume
    h = 2.6 / (N - 1)
    vol = TSDFVolume((-1.3,) * 3, h, (N, N, N), dev)
    ax = torch.arange(N, dtype=torch.float32, device=dev) * vol.voxel_size + vol.origin[0]
    G = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    vol.tsdf = (G.norm(dim=-1) - 0.9).contiguous()
    vol.weight = torch.ones_like(vol.tsdf)
    vol.color = (G / 2.6 + 0.5).clamp(0, 1).contiguous()
    return vol.extract() + (vol.voxel_size,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--cells", type=float, nargs="*", default=[2.0, 3.0], help="cell sizes in voxels")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify_timing.json"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops, mesh_simplify
    from dgs_amd.cameras import make_camera, pose_spherical
    from dgs_amd.mesh_metrics import mesh_distance
    from dgs_amd.mesh_render import render_mesh
    dev = torch.device("cuda:0")
    v, f, c, h = sphere_mesh(a.grid, dev)
    cam = make_camera(pose_spherical(30.0, -30.0, 4.0), 0.6911, 0.6911, a.pixels, a.pixels, 0.0)
    result = {"device": torch.cuda.get_device_name(0), "mesh": "sphere r = 0.9, %d^3" % a.grid, "vertices": int(v.shape[0]), "faces": int(f.shape[0]),
              "layout": _mesh_ops.simplify_layout(), "entries": []}
    full_distance = measure(lambda: mesh_distance((v, f), (v, f), n_samples=a.samples, device=dev, mode="surface"), 3)[0]
    full_render = measure(lambda: render_mesh(cam, v, f, c), a.reps)[0]
    for k in a.cells:
        cell = float(np.float32(k * h))
        cell_t = torch.full((1,), cell, dtype=torch.float32, device=dev)
        cluster, centre, _ = mesh_simplify._cells(v, cell_t, v.amin(0) - cell_t * 0.5)
        cl32, none = cluster.to(torch.int32), f[:0]
        acc_v = lambda: _mesh_ops.simplify_accumulate(v, c, none, cl32, centre, cell)
        acc = lambda: _mesh_ops.simplify_accumulate(v, c, f, cl32, centre, cell)
        rows = acc()
        solve = lambda: _mesh_ops.simplify_solve(rows, centre, cell, True, True)
        ref_acc = lambda: mesh_simplify._accumulate_torch(v, c, f.long(), cluster, centre, cell_t)
        ref_solve = lambda: mesh_simplify._solve_torch(rows, centre, cell_t, True, True)
        whole = lambda: mesh_simplify.simplify_mesh(v, f, c, cell_size=cell)
        acc(), ref_acc()
        torch.cuda.synchronize()
        hip_ms, ref_ms = [], []
        for _ in range(a.reps):                          # alternating: both see the same state of the machine
            hip_ms.append(timed(acc)[0])
            t, ref_rows = timed(ref_acc)
            ref_ms.append(t)
        same = bool(torch.equal(ref_rows, rows))
        (sv, sc), (rv, rc) = solve(), ref_solve()
        same = same and bool(torch.equal(sv.view(torch.int32), rv.view(torch.int32)) and torch.equal(sc.view(torch.int32), rc.view(torch.int32)))
        e = {"cell_voxels": k, "cell": cell, "clusters": int(centre.shape[0]), "results_bit_identical": same,
             "accumulate_vertices": measure(acc_v, a.reps)[0], "accumulate": stats(hip_ms), "solve": measure(solve, a.reps)[0],
             "statement_accumulate": stats(ref_ms), "statement_solve": measure(ref_solve, a.reps)[0]}
        e["speedup_accumulate"] = e["statement_accumulate"]["median_ms"] / e["accumulate"]["median_ms"]
        e["simplify_mesh"], (lv, lf, lc) = measure(whole, a.reps)
        e["vertices_out"], e["faces_out"] = int(lv.shape[0]), int(lf.shape[0])
        e["distance_surface_full"], e["render_full"] = full_distance, full_render
        e["distance_surface_simplified"], d = measure(lambda: mesh_distance((lv, lf), (v, f), n_samples=a.samples, device=dev, mode="surface"), 3)
        e["chamfer_to_full"] = float(d["chamfer"])
        e["render_simplified"] = measure(lambda: render_mesh(cam, lv, lf, lc), a.reps)[0]
        result["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
