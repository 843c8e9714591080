"""Times of the closest-triangle search behind mesh_distance(mode="surface") -> profiles/mesh_surface_timing.md.

    python tools/mesh_surface_timing.py [--queries 100000] [--faces 400000 1600000] [--reps 10] [--out profiles/mesh_surface_timing.md]

For every face count F: --queries points uniform in [-1, 1]^3 against F random triangles (first corner uniform in [-1, 1]^3, edges
uniform in [-0.02, 0.02]^3; seeded; the kernel is branch-free, its time does not depend on the data).  dgs_tri_search
(dgs_amd._mesh_ops.closest_face on a prepared table: the memset of the output included, the table not) and the PyTorch statement
of the same arithmetic (dgs_amd.mesh_metrics.closest_face_torch) run on the same device in the same process, ALTERNATING, timed with
device events after a warm-up run of each.  The PyTorch statement makes about a hundred elementwise passes over [chunk, F]
intermediates (--torch-elements elements each), so it runs on the first --torch-queries queries only and its time is SCALED by
queries / torch-queries (its cost is linear in the queries: whole chunks of the same size); the table says so.  Bit-identity is
checked on those queries.  Reported per size: milliseconds (median, min, max), the ratio, pairs per second, and the kernel's rate
against the VALU issue bound for VALU_PER_PAIR instructions per pair (counted in the ISA of tri_search_kernel's inner loop: 368 VALU
instructions per table row and four queries -- 164 + 12 v_mul, 80 v_add, 72 v_sub, 12 + 5 v_cmp, 12 v_cndmask, 4 v_min, 4 v_min3, 3
address / index -- next to 9 LDS reads).  Then one mesh_distance(mode="surface") next to mode="samples" on two UV spheres of about
--faces[0] faces each, end to end (host clock around a synchronised call: sampling, table, both searches, reductions)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

VALU_PER_PAIR = 368.0 / 4.0
# one wave64 VALU instruction occupies a SIMD for 2 cycles: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz
LANE_INSTRUCTIONS_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return "%.2f (%.2f-%.2f, %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def uv_sphere(radius, nu, nv):
    th, ph = np.pi * np.arange(1, nv) / nv, 2 * np.pi * np.arange(nu) / nu
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None, :], np.sin(th)[:, None] * np.sin(ph)[None, :],
                     np.broadcast_to(np.cos(th)[:, None], (nv - 1, nu))], -1).reshape(-1, 3)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring, [[0.0, 0.0, -1.0]]]) * radius
    j, i = np.meshgrid(np.arange(nv - 2), np.arange(nu), indexing="ij")
    rid = lambda j, i: 1 + j * nu + (i % nu)
    quads = np.concatenate([np.stack([rid(j, i), rid(j + 1, i), rid(j + 1, i + 1)], -1).reshape(-1, 3),
                            np.stack([rid(j, i), rid(j + 1, i + 1), rid(j, i + 1)], -1).reshape(-1, 3)])
    i = np.arange(nu)
    south = 1 + nu * (nv - 1)
    caps = np.concatenate([np.stack([np.zeros_like(i), rid(0, i), rid(0, i + 1)], -1),
                           np.stack([np.full_like(i, south), rid(nv - 2, i + 1), rid(nv - 2, i)], -1)])
    return v.astype(np.float32), np.concatenate([quads, caps]).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--faces", type=int, nargs="*", default=[400_000, 1_600_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-queries", type=int, nargs="*", default=[10_000, 2_500])
    ap.add_argument("--torch-elements", type=int, default=1 << 26)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_surface_timing.md"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import closest_face_torch, mesh_distance, triangle_table
    dev = torch.device("cuda:0")
    q_block, t_round, t_chunk, row = _mesh_ops.tri_layout()
    bound = LANE_INSTRUCTIONS_PER_S / VALU_PER_PAIR
    nq = a.queries
    lines = ["# Closest-triangle search of the mesh metrics: `dgs_tri_search` against the PyTorch statement", "",
             "`tools/mesh_surface_timing.py` on %s; %d queries uniform in [-1, 1]^3 against F random triangles, seed 0; device events, the "
             "two alternating in one process after a warm-up run of each; layout: %d queries per workgroup, %d triangles per LDS round, "
             "slices of %d triangles, %d floats per row.  The PyTorch statement runs on the first q queries only, with %d-element "
             "intermediates; its column is that time scaled by %d / q.  VALU issue bound: %.3g lane-instructions/s / %.1f "
             "instructions per pair = %.3g pairs/s." %
             (torch.cuda.get_device_name(0), nq, q_block, t_round, t_chunk, row, a.torch_elements, nq, LANE_INSTRUCTIONS_PER_S, VALU_PER_PAIR, bound), "",
             "| queries x F | workgroups | HIP ms (median, min-max, runs) | PyTorch ms on q queries (median, min-max, runs) | q | PyTorch ms scaled | ratio | "
             "bit-identical on the q queries | HIP pairs/s | share of the VALU bound |", "|---|---|---|---|---|---|---|---|---|---|"]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    for n_faces, tq in zip(a.faces, a.torch_queries):
        g = torch.Generator().manual_seed(0)
        pts = (torch.rand(nq, 3, generator=g) * 2 - 1).to(dev)
        corner = torch.rand(n_faces, 3, generator=g) * 2 - 1
        tri = torch.stack([corner, corner + (torch.rand(n_faces, 3, generator=g) - 0.5) * 0.04, corner + (torch.rand(n_faces, 3, generator=g) - 0.5) * 0.04], 1)
        table = triangle_table(tri.reshape(-1, 3).to(dev), torch.arange(3 * n_faces, device=dev).reshape(-1, 3))
        sub = pts[:tq].contiguous()
        chunk = max(1, a.torch_elements // n_faces)
        run_hip = lambda: _mesh_ops.closest_face(pts, table)
        run_torch = lambda: closest_face_torch(sub, table, chunk=chunk)
        first, _ = timed(run_hip)
        t_first, _ = timed(run_torch)
        hip_ms, torch_ms, out_t = [], [], None
        for i in range(a.reps):
            ms, out_h = timed(run_hip)
            hip_ms.append(ms)
            if i < a.torch_reps:
                ms, out_t = timed(run_torch)
                torch_ms.append(ms)
        same = bool(torch.equal(out_h[0][:tq], out_t[0]) and torch.equal(out_h[1][:tq], out_t[1]))
        h, t = statistics.median(hip_ms), statistics.median(torch_ms) * nq / tq
        rate = float(nq) * n_faces / (h * 1e-3)
        wgs = ((nq + q_block - 1) // q_block) * ((n_faces + t_chunk - 1) // t_chunk)
        row_text = "| %d x %d | %d | %s | %s | %d | %.0f | %.0fx | %s | %.3g | %.0f %% |" % (
            nq, n_faces, wgs, stats(hip_ms), stats(torch_ms), tq, t, t / h, "yes" if same else "NO", rate, 100.0 * rate / bound)
        print(row_text, "(first HIP call %.2f ms, first PyTorch run %.1f ms)" % (first, t_first), flush=True)
        lines.append(row_text)
        del pts, table, sub, out_h, out_t
        torch.cuda.empty_cache()
        flush()

    # one metric call, end to end
    nu = int(round((a.faces[0] / 4) ** 0.5)) * 2
    inner, outer = uv_sphere(1.0, nu, nu // 2), uv_sphere(1.01, nu, nu // 2)
    lines += ["", "`mesh_distance` end to end on two UV spheres (radii 1.0 / 1.01, %d faces each), %d samples, host clock around a "
              "synchronised call after one warm-up call of each mode:" % (inner[1].shape[0], nq), "",
              "| mode | ms (median, min-max, calls) | accuracy | completeness |", "|---|---|---|---|"]
    for mode in ("samples", "surface"):
        ms = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = mesh_distance(inner, outer, n_samples=nq, device="cuda:0", mode=mode)
            torch.cuda.synchronize()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
        lines.append("| %s | %s | %.6f | %.6f |" % (mode, stats(ms), m["accuracy"], m["completeness"]))
        print(lines[-1], flush=True)
        flush()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
