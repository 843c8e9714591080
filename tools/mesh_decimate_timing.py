"""Times and quality of mesh decimation on meshes of about 10^6 faces -> profiles/mesh_decimate_timing.json.

    python tools/mesh_decimate_timing.py [--grid 288] [--sheet 708] [--ratios 0.5 0.25 0.1] [--oversubscribe 1 2 4 8 16 64] [--out ...]
                                         [--device cuda:0] [--no-statement]

Two meshes: the analytic sphere |p| = 0.9 in a volume of --grid^3 points, extracted by the marching tetrahedra (vertices and faces in
cell order, as every extracted frame's are), and a marching-tetrahedra-like sheet, the height field z = 0.1 sin(5 x) cos(4 y) over
--sheet^2 grid points in row order, two triangles a cell.  For each:
  rounds      per ratio: the rounds decimate_mesh needs, the faces it reaches, the time of the whole call (one warm-up, then once),
              and the rms distance of the result's vertices and face centroids to the analytic surface
  phases      over the rounds to the smallest ratio, ms per round: tables (the sorts, run lengths and prefix sums of step a), edges
              (dgs_decimate_edges), throttle (kthvalue), select (dgs_decimate_select), prefix (the sort of the selected keys),
              apply (dgs_decimate_apply), compact (the surviving faces); the device is synchronised after every phase
  prepare     ms of step 0 and 1 (the frame, the mean face area, dgs_decimate_quadrics), once a call
  statement   the whole call to the first ratio with the PyTorch statement on the same device, and whether the two results are
              bit-identical
  quality     the table behind mesh_decimate.OVERSUBSCRIBE: for every value, rounds to the middle ratio and the rms distance there
--device cpu runs the rounds and the quality table without a device (small --grid / --sheet), e.g. to look at the table's shape."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def sync(dev):
    if dev.type != "cpu":
        torch.cuda.synchronize()


def sphere_mesh(N, dev):
    from dgs_amd.mesh import TSDFVolume
    h = 2.6 / (N - 1)
    vol = TSDFVolume((-1.3,) * 3, h, (N, N, N), dev)
    ax = torch.arange(N, dtype=torch.float32, device=dev) * vol.voxel_size + vol.origin[0]
    G = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)
    vol.tsdf = (G.norm(dim=-1) - 0.9).contiguous()
    vol.weight = torch.ones_like(vol.tsdf)
    vol.color = (G / 2.6 + 0.5).clamp(0, 1).contiguous()
    return vol.extract()


def sheet_height(x, y):
    return 0.1 * np.sin(5.0 * x) * np.cos(4.0 * y)


def sheet_mesh(N, dev):
    ax = torch.arange(N, dtype=torch.float64) / (N - 1)
    x, y = torch.meshgrid(ax, ax, indexing="ij")
    v = torch.stack((x, y, 0.1 * torch.sin(5.0 * x) * torch.cos(4.0 * y)), -1).reshape(-1, 3).float()
    i, j = torch.meshgrid(torch.arange(N - 1), torch.arange(N - 1), indexing="ij")
    a = (i * N + j).reshape(-1)
    f = torch.stack((torch.stack((a, a + N, a + N + 1), -1), torch.stack((a, a + N + 1, a + 1), -1)), 1).reshape(-1, 3).to(torch.int32)
    c = torch.stack((x, y, 0.5 * torch.ones_like(x)), -1).reshape(-1, 3).float()
    return v.to(dev), f.to(dev), c.to(dev)


def rms_to_surface(name, v, f):
    """The rms distance of vertices and face centroids to the analytic surface (the sheet: the vertical residual over the slope)."""
    p, fn = v.double().cpu().numpy(), f.cpu().numpy().astype(np.int64)
    p = np.concatenate((p[np.unique(fn)], p[fn].mean(1)))
    if name == "sphere":
        d = np.linalg.norm(p, axis=1) - 0.9
    else:
        gx, gy = 0.5 * np.cos(5.0 * p[:, 0]) * np.cos(4.0 * p[:, 1]), -0.4 * np.sin(5.0 * p[:, 0]) * np.sin(4.0 * p[:, 1])
        d = (p[:, 2] - sheet_height(p[:, 0], p[:, 1])) / np.sqrt(1.0 + gx * gx + gy * gy)
    return float(np.sqrt(np.mean(d * d)))


def run(mesh, ratio, oversubscribe=None, clock=None, preserve_boundary=True):
    """decimate_mesh's loop with a round count -> (rounds, vertices, faces); the output tensors through the function itself."""
    from dgs_amd import mesh_decimate as md
    v, f, c = mesh
    target = int(ratio * f.shape[0])
    st, q_bits, scale, centre = md.prepare(v, f, c, preserve_boundary)
    if clock:
        clock("prepare")
    rounds = 0
    for _ in range(md.default_max_rounds(f.shape[0], target)):
        if st.faces.shape[0] <= target:
            break
        n = md.decimate_round(st, target, q_bits, float("inf"), preserve_boundary, oversubscribe, clock)[0]
        rounds += 1
        if n == 0:
            break
    new_v = torch.where(st.moved[:, None], centre + st.pos * (1.0 / scale), v)
    return rounds, new_v, st.faces


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--sheet", type=int, default=708)
    ap.add_argument("--ratios", type=float, nargs="*", default=[0.5, 0.25, 0.1])
    ap.add_argument("--oversubscribe", type=float, nargs="*", default=[1, 2, 4, 8, 16, 64])
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--no-statement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate_timing.json"))
    a = ap.parse_args()
    from dgs_amd import mesh_decimate as md, mesh_topology
    dev = torch.device(a.device)
    result = {"device": torch.cuda.get_device_name(0) if dev.type != "cpu" else "cpu", "oversubscribe": md.OVERSUBSCRIBE, "meshes": []}
    if dev.type != "cpu":
        from dgs_amd import _mesh_ops
        result["layout"] = _mesh_ops.decimate_layout()

    def wall(fn):
        sync(dev)
        t = time.perf_counter()
        out = fn()
        sync(dev)
        return (time.perf_counter() - t) * 1e3, out

    for name, mesh in (("sphere", sphere_mesh(a.grid, dev)), ("sheet", sheet_mesh(a.sheet, dev))):
        v, f, c = mesh
        e = {"mesh": name, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "q_bits": md.quadric_bits(f.shape[0]),
             "rms_input": rms_to_surface(name, v, f), "rounds": [], "quality": []}
        md.decimate_mesh(v, f, c, ratio=0.9)                                                # warm-up: the library, the allocator
        for ratio in a.ratios:
            ms, out = wall(lambda: md.decimate_mesh(v, f, c, ratio=ratio))
            rounds, rv, rf = run(mesh, ratio)
            assert rf.shape[0] == out[1].shape[0]
            e["rounds"].append({"ratio": ratio, "rounds": rounds, "faces_out": int(out[1].shape[0]), "decimate_mesh_ms": ms, "ms_per_round": ms / max(rounds, 1),
                                "rms": rms_to_surface(name, out[0], out[1])})
            print(json.dumps({"mesh": name, **e["rounds"][-1]}), flush=True)
        phases, last = {}, [0.0]

        def clock(phase):
            sync(dev)
            now = time.perf_counter()
            phases[phase] = phases.get(phase, 0.0) + (now - last[0]) * 1e3
            last[0] = now

        sync(dev)
        last[0] = time.perf_counter()
        rounds = run(mesh, min(a.ratios), clock=clock)[0]
        e["prepare_ms"] = phases.pop("prepare")                                             # the frame, the mean face area, dgs_decimate_quadrics: once a call
        e["phases_ms_per_round"] = {k: t / max(rounds, 1) for k, t in phases.items()}
        e["phases_rounds"] = rounds
        print(json.dumps({"mesh": name, "phases_ms_per_round": e["phases_ms_per_round"], "rounds": rounds}), flush=True)
        if dev.type != "cpu" and not a.no_statement:
            ratio = a.ratios[0]
            want = md.decimate_mesh(v, f, c, ratio=ratio, return_map=True)
            mesh_topology._STATEMENT_EVERYWHERE = True
            try:
                ms, got = wall(lambda: md.decimate_mesh(v, f, c, ratio=ratio, return_map=True))
            finally:
                mesh_topology._STATEMENT_EVERYWHERE = False
            same = all((x is None and y is None) or (x.shape == y.shape and torch.equal(x.view(torch.int32) if x.is_floating_point() else x,
                                                                                         y.view(torch.int32) if y.is_floating_point() else y))
                       for x, y in zip(want, got))
            e["statement"] = {"ratio": ratio, "decimate_mesh_ms": ms, "results_bit_identical": bool(same)}
            print(json.dumps({"mesh": name, "statement": e["statement"]}), flush=True)
        mid = a.ratios[len(a.ratios) // 2]
        for k in a.oversubscribe:
            ms, (rounds, qv, qf) = wall(lambda: run(mesh, mid, oversubscribe=float(k)))
            e["quality"].append({"oversubscribe": k, "ratio": mid, "rounds": rounds, "faces_out": int(qf.shape[0]), "ms": ms, "rms": rms_to_surface(name, qv, qf)})
            print(json.dumps({"mesh": name, **e["quality"][-1]}), flush=True)
        result["meshes"].append(e)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
