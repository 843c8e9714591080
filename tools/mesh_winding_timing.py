"""Times of the winding-number sums behind contains / volume_iou -> profiles/mesh_winding_timing.json.

    python tools/mesh_winding_timing.py [--queries 100000] [--faces 400000 1600000] [--reps 10] [--out profiles/mesh_winding_timing.json]

For every face count F: --queries points uniform in [-1, 1]^3 against F random triangles (first corner uniform in [-1, 1]^3, edges
uniform in [-0.02, 0.02]^3; seeded; the kernel is branch-free, its time does not depend on the data) -- the inputs of
tools/mesh_surface_timing.py.  dgs_winding_sum (dgs_amd._mesh_ops.winding_sums on a prepared table: the memset of the output
included, the table not) and the PyTorch statement of the same arithmetic (dgs_amd.mesh_metrics.winding_sums_torch) run on the
same device in the same process, ALTERNATING, timed with device events after a warm-up run of each; medians of --reps.  The
statement makes about a hundred elementwise passes over [chunk, F] intermediates, so it runs on the first --torch-queries queries
only and its time is SCALED by queries / torch-queries (its cost is linear in the queries); bit-identity is checked on those
queries.  Reported per size: milliseconds, the ratio, pairs per second, and the kernel's rate against the VALU issue bound for
VALU_PER_PAIR instructions per pair (counted in the ISA of winding_sum_kernel's inner loop: 594 VALU instructions per table row and
four queries -- 172 v_mul, 92 v_add, 48 v_sub, 44 v_fma / v_fmac of the square-root and division refinements, 84 v_cndmask, 72
v_cmp, 12 v_sqrt, 4 v_rcp, 16 v_div_*, 8 min / max, 4 v_rndne, 4 v_cvt, 34 integer -- next to 3 LDS reads).  Then volume_iou end to
end (host clock around a synchronised call) on two UV spheres of about --iou-faces faces each with --queries samples."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

from mesh_surface_timing import LANE_INSTRUCTIONS_PER_S, timed, uv_sphere

VALU_PER_PAIR = 594.0 / 4.0


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--faces", type=int, nargs="*", default=[400_000, 1_600_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--torch-queries", type=int, nargs="*", default=[2_000, 500])
    ap.add_argument("--iou-faces", type=int, default=400_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding_timing.json"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import volume_iou, winding_sums_torch, winding_table
    dev = torch.device("cuda:0")
    layout = _mesh_ops.winding_layout()
    bound = LANE_INSTRUCTIONS_PER_S / VALU_PER_PAIR
    nq = a.queries
    result = {"device": torch.cuda.get_device_name(0), "queries": nq, "layout": layout, "valu_per_pair": VALU_PER_PAIR,
              "valu_bound_pairs_per_s": bound, "entries": []}

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)

    for n_faces, tq in zip(a.faces, a.torch_queries):
        g = torch.Generator().manual_seed(0)
        pts = (torch.rand(nq, 3, generator=g) * 2 - 1).to(dev)
        corner = torch.rand(n_faces, 3, generator=g) * 2 - 1
        tri = torch.stack([corner, corner + (torch.rand(n_faces, 3, generator=g) - 0.5) * 0.04, corner + (torch.rand(n_faces, 3, generator=g) - 0.5) * 0.04], 1)
        table = winding_table(tri.reshape(-1, 3).to(dev), torch.arange(3 * n_faces, device=dev).reshape(-1, 3))
        sub = pts[:tq].contiguous()
        run_hip = lambda: _mesh_ops.winding_sums(pts, table)
        run_torch = lambda: winding_sums_torch(sub, table)
        first, _ = timed(run_hip)                                # warm-up of both (the library, the allocator)
        t_first, _ = timed(run_torch)
        hip_ms, torch_ms, out_t = [], [], None
        for i in range(a.reps):                                  # alternating
            ms, out_h = timed(run_hip)
            hip_ms.append(ms)
            if i < a.torch_reps:
                ms, out_t = timed(run_torch)
                torch_ms.append(ms)
        h, t = statistics.median(hip_ms), statistics.median(torch_ms) * nq / tq
        rate = float(nq) * n_faces / (h * 1e-3)
        e = {"faces": n_faces, "workgroups": ((nq + layout[0] - 1) // layout[0]) * ((n_faces + layout[2] - 1) // layout[2]),
             "dgs_winding_sum": stats(hip_ms), "first_call_ms": first, "statement_queries": tq, "statement_on_those": stats(torch_ms),
             "statement_first_run_ms": t_first, "statement_scaled_ms": t, "ratio": t / h,
             "bit_identical_on_those": bool(torch.equal(out_h[:tq], out_t)), "pairs_per_s": rate, "share_of_valu_bound": rate / bound}
        result["entries"].append(e)
        print(json.dumps(e), flush=True)
        flush()
        del pts, table, sub, out_h, out_t
        torch.cuda.empty_cache()

    # the whole metric, end to end
    nu = int(round((a.iou_faces / 4) ** 0.5)) * 2
    inner, outer = uv_sphere(1.0, nu, nu // 2), uv_sphere(1.05, nu, nu // 2)
    ms = []
    for i in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = volume_iou(inner, outer, n_samples=nq, device="cuda:0")
        torch.cuda.synchronize()
        if i:
            ms.append((time.perf_counter() - t0) * 1e3)
    result["volume_iou"] = dict({"faces_each": int(inner[1].shape[0]), "samples": nq, "host_clock": stats(ms)}, **m)
    print(json.dumps(result["volume_iou"]), flush=True)
    flush()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
