"""Times of the earth mover's distance (dgs_emd_auction behind dgs_amd.mesh_metrics.emd) -> a JSON file.

    python tools/mesh_emd_timing.py [--sizes 2048 4096 8192] [--duplicates 2048] [--reps 3] [--scipy-max 4096] [--out FILE]
    python tools/mesh_emd_timing.py --once 4096      # one warm-up and one run of that size, nothing else: the body of a kernel trace

For every size n: n points on the unit sphere against n points on a sphere of radius 1.05 (seeded normal directions), and for
--duplicates the duplicate-heavy construction of tests/test_mesh_emd_cpu.py (half of b one repeated point, a quarter of a another).
Timed: dgs_amd._mesh_ops.emd_auction alone (the host loop of launches and its one read per batch; inputs resident, the quantum
computed before), with a host clock around the call -- the call ends in a device synchronise by construction.  One warm-up run, then
--reps timed ones.  Reported per case: wall milliseconds (median, min, max), rounds, rounds per second, microseconds per round,
primal - dual, and -- up to --scipy-max points -- the seconds scipy.optimize.linear_sum_assignment takes on the same integer matrix on
the host with primal - OPT and OPT - dual.  The yardstick stands in for a reference implementation (the upstream project has no EMD);
it is never the code under test."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch


def sphere_points(n, seed, radius=1.0):
    x = torch.randn((n, 3), generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True) * radius).contiguous()


def duplicate_heavy(n, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.rand((n, 3), generator=g), torch.rand((n, 3), generator=g)
    b[:n // 2] = b[0]
    a[:n // 4] = a[0]
    return a, b


def run_case(name, a, b, reps, with_scipy):
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import _emd_costs, _emd_quantum
    n = a.shape[0]
    q, inv_q = _emd_quantum(a, b)
    ad, bd = a.cuda(), b.cuda()
    lay = _mesh_ops.emd_layout()
    scratch = torch.empty(lay[4] + n * lay[5], dtype=torch.uint8, device="cuda")
    run = lambda: _mesh_ops.emd_auction(ad, bd, inv_q, 50_000_000, scratch=scratch)
    first = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        out = run()
        ms.append((time.perf_counter() - t) * 1e3)
        assert torch.equal(out[0], first[0]) and out[2:] == first[2:]
    _, _, primal, dual, rounds, max_cost = first
    row = {"case": name, "n": n, "q": q, "rounds": rounds, "max_cost": max_cost, "primal_minus_dual": primal - dual,
           "emd_gap": (primal - dual) * q / n, "ms": {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}}
    row["rounds_per_s"] = rounds / (row["ms"]["median"] * 1e-3)
    row["us_per_round"] = row["ms"]["median"] * 1e3 / rounds
    if with_scipy:
        from scipy.optimize import linear_sum_assignment
        cost = _emd_costs(a, b, inv_q).numpy()
        t = time.perf_counter()
        rows, cols = linear_sum_assignment(cost)
        row["scipy_s"] = time.perf_counter() - t
        opt = int(cost[rows, cols].sum())
        row["primal_minus_opt"], row["opt_minus_dual"] = primal - opt, opt - dual
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 4096, 8192])
    ap.add_argument("--duplicates", type=int, nargs="*", default=[2048])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-max", type=int, default=4096)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_emd_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_emd_timing: a HIP device is needed (a time taken elsewhere says nothing)")
    if a.once:
        run_case("sphere vs 1.05 x sphere", sphere_points(a.once, 1), sphere_points(a.once, 2, 1.05), 1, False)
        return
    from dgs_amd import _mesh_ops
    rows = [run_case("sphere vs 1.05 x sphere", sphere_points(n, 1), sphere_points(n, 2, 1.05), a.reps, n <= a.scipy_max) for n in a.sizes]
    rows += [run_case("duplicate-heavy", *duplicate_heavy(n, 7), a.reps, n <= a.scipy_max) for n in a.duplicates]
    out = {"device": torch.cuda.get_device_name(0), "layout": list(_mesh_ops.emd_layout()), "source_hash": _mesh_ops.source_hash(), "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
