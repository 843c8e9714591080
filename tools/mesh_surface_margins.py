"""The constant of the closest-face tolerance -> profiles/mesh_surface_margins.md.

    python tools/mesh_surface_margins.py [--out profiles/mesh_surface_margins.md]

Runs on the CPU.  For every input set of tests/mesh_surface_ref.py -- the sets of tests/test_mesh_surface_cpu.py and every (Nq, Nf)
case of tests/test_mesh_surface_gpu.py -- it evaluates the PyTorch statement of dgs_tri_search in fp32 for ALL pairs and compares
the distances with the float64 brute force: the largest |d32 - d64| / (2^-24 L kappa).  The tests bound their errors by four times
the largest of these values (mesh_surface_ref.C_MEASURED, C); this tool is how C_MEASURED is obtained, and it fails if the value in
the test helper is not the one it measures."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_surface_margins.md"))
    a = ap.parse_args()
    import mesh_surface_ref as ref
    from dgs_amd import _mesh_ops
    layout = _mesh_ops.tri_layout()
    rows = [(name, p.shape[0], f.shape[0], ref.measure_c(p, v, f)) for name, p, v, f in ref.cpu_sets()]
    for nq, nf in ref.gpu_cases(layout):
        p, v, f = ref.case(nq, nf)
        rows.append(("GPU case", nq, nf, ref.measure_c(p, v, f)))
        print(rows[-1], flush=True)
    worst = max(r[3] for r in rows)
    lines = ["# Closest-face search: the constant of the tolerance against float64", "",
             "`tools/mesh_surface_margins.py`, on the CPU.  Per input set: the PyTorch statement of `dgs_tri_search` "
             "(`mesh_metrics._pair_d2`, fp32) for all pairs against the float64 brute force of `tests/mesh_surface_ref.py` "
             "(Ericson's Voronoi regions): the largest `|d32 - d64| / (2^-24 L kappa)`, L the largest float64 distance from the "
             "query to a corner, kappa = |AB| |AC| / |n| of the face.  Layout Q, T, C, row = %s." % (layout,), "",
             "| input set | queries | faces | largest constant |", "|---|---|---|---|"]
    lines += ["| %s | %d | %d | %.3f |" % r for r in rows]
    lines += ["", "Largest over all sets: **%.3f**.  `tests/mesh_surface_ref.py` records C_MEASURED = %.2f and bounds every error by "
              "C = 4 x C_MEASURED = %.2f: the device's elementwise code may round the last bit of an operation differently from the "
              "CPU's, and a factor 4 covers that over the ~100 operations of a pair." % (worst, ref.C_MEASURED, ref.C)]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("largest %.4f, recorded %.2f; wrote %s" % (worst, ref.C_MEASURED, a.out))
    if not (worst <= ref.C_MEASURED <= worst + 0.01):
        raise SystemExit("mesh_surface_ref.C_MEASURED = %.2f is not the measured %.4f rounded up to 0.01" % (ref.C_MEASURED, worst))


if __name__ == "__main__":
    main()
