"""Times of the all-pairs nearest-neighbour search behind the mesh metrics -> profiles/mesh_metrics_timing.md.

    python tools/mesh_metrics_timing.py [--sizes 100000 1000000] [--reps 10] [--out profiles/mesh_metrics_timing.md]

For every size N: N query points against N reference points, uniform in [-1, 1]^3 from a seeded generator (random data: the sizes a
mesh_distance call with n_samples = N searches).  dgs_nn_search (dgs_amd._mesh_ops.nearest) and the PyTorch statement of the same
arithmetic (dgs_amd.mesh_metrics.nearest_torch) run on the same device in the same process, ALTERNATING, timed with device events
after warm-up runs of each.  A timed sample of the kernel is as many back-to-back calls as fill about 50 ms (the memset of the
output included), so that a sample measures the kernel and not the clock; the PyTorch statement takes long enough alone, and at sizes
where one run of it takes seconds it is repeated --torch-reps-large times instead of --reps.  Its [chunk, N] intermediates hold
--torch-elements elements (default 2^26, 256 MB in fp32).  Reported per size: milliseconds (median, min, max), the ratio of the
medians, whether the two results are bit-identical, the kernel's rate in pair evaluations per second, and that rate against the
VALU issue bound for the inner loop's instruction count per pair (VALU_PER_PAIR, counted in the ISA: 3 v_sub, 3 v_mul, 2 v_add, 1
v_cmp, 2 v_cndmask = 11, plus 5 v_mov per 16 pairs for the indices and the LDS address)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch

VALU_PER_PAIR = 11.0 + 5.0 / 16.0
# one wave64 VALU instruction occupies a SIMD for 2 cycles: 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz (= the 157.3 TFLOP/s fp32 vector peak / 2)
LANE_INSTRUCTIONS_PER_S = 256 * 4 * 32 * 2.4e9


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, out


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps-large", type=int, default=2)
    ap.add_argument("--torch-elements", type=int, default=1 << 26)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_metrics_timing.md"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import nearest_torch
    dev = torch.device("cuda:0")
    q_block, r_tile, r_chunk = _mesh_ops.nn_layout()
    bound = LANE_INSTRUCTIONS_PER_S / VALU_PER_PAIR
    lines = ["# Nearest-neighbour search of the mesh metrics: `dgs_nn_search` against the PyTorch statement", "",
             "`tools/mesh_metrics_timing.py` on %s; N queries against N reference points, uniform in [-1, 1]^3, seed 0; device events, "
             "the two alternating in one process after warm-up; layout: %d queries per workgroup, %d reference points per LDS round, "
             "slices of %d points.  VALU issue bound: %.3g lane-instructions/s / %.2f instructions per pair = %.3g pairs/s." %
             (torch.cuda.get_device_name(0), q_block, r_tile, r_chunk, LANE_INSTRUCTIONS_PER_S, VALU_PER_PAIR, bound), "",
             "| N | workgroups | HIP ms (median, min-max, samples x calls) | PyTorch ms (median, min-max, runs) | ratio | bit-identical | HIP pairs/s | share of the VALU bound |",
             "|---|---|---|---|---|---|---|---|"]
    for n in a.sizes:
        g = torch.Generator().manual_seed(0)
        q = (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)
        r = (torch.rand(n, 3, generator=g) * 2 - 1).to(dev)
        chunk = max(1, a.torch_elements // n)
        run_hip = lambda: _mesh_ops.nearest(q, r)
        run_torch = lambda: nearest_torch(q, r, chunk=chunk)
        first, _ = timed(run_hip)                       # warm-up of both (code objects, allocator); the first call sizes a sample
        once, _ = timed(run_hip)
        t_first, _ = timed(run_torch)
        inner = max(1, int(round(50.0 / max(once, 1e-3))))
        torch_reps = a.reps if t_first < 1000.0 else a.torch_reps_large
        hip_ms, torch_ms, out_t = [], [], None
        for i in range(a.reps):
            ms, out_h = timed(run_hip, inner)
            hip_ms.append(ms)
            if i < torch_reps:
                ms, out_t = timed(run_torch)
                torch_ms.append(ms)
        same = bool(torch.equal(out_h[0], out_t[0]) and torch.equal(out_h[1], out_t[1]))
        h, t = stats(hip_ms), stats(torch_ms)
        rate = float(n) * n / (h["median"] * 1e-3)
        wgs = ((n + q_block - 1) // q_block) * ((n + r_chunk - 1) // r_chunk)
        row = "| %d | %d | %.3f (%.3f-%.3f, %d x %d) | %.1f (%.1f-%.1f, %d) | %.1fx | %s | %.3g | %.0f %% |" % (
            n, wgs, h["median"], h["min"], h["max"], h["n"], inner, t["median"], t["min"], t["max"], t["n"], t["median"] / h["median"],
            "yes" if same else "NO", rate, 100.0 * rate / bound)
        print(row, "(first HIP call %.3f ms, first PyTorch run %.1f ms)" % (first, t_first), flush=True)
        lines.append(row)
        del q, r, out_h, out_t
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
