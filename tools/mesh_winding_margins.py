"""The tolerance of the winding number against float64 -> profiles/mesh_winding_margins.md.

    python tools/mesh_winding_margins.py [--out profiles/mesh_winding_margins.md]

Runs on the CPU.  For every input set of tests/mesh_winding_ref.py -- the sets of tests/test_mesh_winding_cpu.py and every (Nq, Nf)
case of tests/test_mesh_winding_gpu.py -- it evaluates the PyTorch statement of dgs_winding_sum in fp32 and compares W with the
float64 brute force of the same fp32 inputs: the largest |W32 - W64|.  The tests bound their errors by four times the largest of
these values, separately for the shape sets (mesh_winding_ref.W_MEASURED, W_TOL: queries at a distance from the surface) and for
the triangle soups, the GPU cases among them (W_MEASURED_SOUP, W_TOL_SOUP: queries down to the surface).  It also sweeps the statement's atan polynomial, evaluated in fp32, against
float64 atan on r = k / 2,000,000 (mesh_winding_ref.POLY_MEASURED).  This tool is how both numbers are obtained, and it fails if a
value in the test helper is not the one it measures."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def rounded_up(x, digits=2):
    """x rounded up to `digits` significant digits, as a float."""
    from decimal import ROUND_CEILING, Decimal
    d = Decimal(repr(x))
    return float(d.quantize(Decimal(1).scaleb(d.adjusted() - digits + 1), rounding=ROUND_CEILING))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_winding_margins.md"))
    a = ap.parse_args()
    import mesh_winding_ref as ref
    from dgs_amd import _mesh_ops
    layout = _mesh_ops.winding_layout()
    rows = [(name, p.shape[0], f.shape[0], ref.measure(p, v, f), soup) for name, p, v, f, soup in ref.cpu_sets()]
    for r in rows:
        print(r, flush=True)
    for nq, nf in ref.gpu_cases(layout):
        p, v, f = ref.case(nq, nf)
        rows.append(("GPU case", nq, nf, ref.measure(p, v, f), True))
        print(rows[-1], flush=True)
    worst, worst_soup = max(r[3] for r in rows if not r[4]), max(r[3] for r in rows if r[4])
    poly = ref.polynomial_error()
    lines = ["# Winding number: the tolerance against float64", "",
             "`tools/mesh_winding_margins.py`, on the CPU.  Per input set: W from the PyTorch statement of `dgs_winding_sum` "
             "(`mesh_metrics.winding_sums_torch`, fp32 pairs, integer sum) against the float64 brute force of `tests/mesh_winding_ref.py` "
             "(the triple-product form with `torch.atan2`) on the same fp32 inputs: the largest `|W32 - W64|` over the queries.  "
             "Layout Q, T, C, row = %s." % (layout,), "",
             "| input set | queries | faces | largest abs(W32 - W64) |", "|---|---|---|---|"]
    lines += ["| %s | %d | %d | %.3e |" % r[:4] for r in rows]
    lines += ["", "Largest over the shape sets and the cap (queries at least 0.05 from the surface): **%.3e**; over the soups and the GPU "
              "cases (a third of the queries within 0.02 of a face): **%.3e**.  `tests/mesh_winding_ref.py` records W_MEASURED = %.1e, "
              "W_MEASURED_SOUP = %.1e and bounds the errors by W_TOL = 4 x W_MEASURED = %.1e and W_TOL_SOUP = 4 x W_MEASURED_SOUP = %.1e: the "
              "fp32 side is bit-defined, the factor covers another libm's or a device's rounding of the float64 side."
              % (worst, worst_soup, ref.W_MEASURED, ref.W_MEASURED_SOUP, ref.W_TOL, ref.W_TOL_SOUP), "",
              "The atan polynomial (8 terms, first coefficient 1), evaluated in fp32 by Horner as the statement does, against float64 "
              "`atan` on r = k / 2,000,000, k = 0 .. 2,000,000: largest error **%.3e rad** (recorded POLY_MEASURED = %.1e)." % (poly, ref.POLY_MEASURED)]
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    got = (rounded_up(worst), rounded_up(worst_soup), rounded_up(poly))
    print("measured (shapes, soups, polynomial) %r, rounded up to two digits %r; wrote %s" % ((worst, worst_soup, poly), got, a.out))
    if (ref.W_MEASURED, ref.W_MEASURED_SOUP, ref.POLY_MEASURED) != got:
        raise SystemExit("mesh_winding_ref records (W_MEASURED, W_MEASURED_SOUP, POLY_MEASURED) = %r, not %r"
                         % ((ref.W_MEASURED, ref.W_MEASURED_SOUP, ref.POLY_MEASURED), got))


if __name__ == "__main__":
    main()
