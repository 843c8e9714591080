"""Times of mesh smoothing on a device-extracted mesh of about 10^6 faces and on a sheet with shuffled ids
-> profiles/mesh_smooth_timing.json.

    python tools/mesh_smooth_timing.py [--grid 288] [--sheet 742] [--reps 10] [--iterations 10] [--out ...]

Two meshes: the analytic sphere |p| = 0.9 in a volume of --grid^3 points over [-1.3, 1.3]^3, extracted by the HIP marching
tetrahedra (vertices numbered by grid key: a row's neighbours lie near each other), and a --sheet x --sheet triangulated sheet
whose vertex ids are a random permutation (a row's neighbours lie anywhere: the bad case for the gather).  For each, timed with
device events after a warm-up of each:
  adjacency     mesh_smooth.vertex_adjacency: the sort / unique of the packed pairs and the prefix sum
  step          dgs_smooth_steps with one step of mode laplacian on [V,3] (an odd count: the launch and the final copy)
  steps_20      dgs_smooth_steps with the 20 steps of taubin x 10 (per-step time = this / 20: no copy)
  smooth_mesh   the whole function at taubin x --iterations: checks, adjacency, steps
  index_add     the same filter the way a user would write it today: per step zeros.index_add_(0, i, x[j]) over the directed edge
                list, a division by the degree and the update, on the same device, alternating with the kernel in the same loop
and the bytes of a step, V (2 * 4 C + 8) + E (4 + 4 C) -- every array once --, against the measured time."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

from mesh_simplify_timing import measure, sphere_mesh, stats, timed

HBM_PEAK_BYTES_PER_S = 8.0e12          # the specification's figure; about 6.3e12 has been measured for a float4 copy


def shuffled_sheet(m, dev, seed=0):
    ij = torch.stack(torch.meshgrid(torch.arange(m), torch.arange(m), indexing="ij"), -1).reshape(-1, 2)
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(m * m, generator=g) * 0.25
    v = torch.cat((ij.float(), z[:, None]), 1)
    q = (torch.arange(m - 1)[:, None] * m + torch.arange(m - 1)[None, :]).reshape(-1)
    f = torch.cat((torch.stack((q, q + m, q + m + 1), 1), torch.stack((q, q + m + 1, q + 1), 1)))
    perm = torch.randperm(m * m, generator=g)                 # new id -> old id
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(m * m)
    return v[perm].contiguous().to(dev), inv[f].to(torch.int32).contiguous().to(dev)


def index_add_filter(v, i, j, inv_deg, has, factors):
    x = v
    for s in factors:
        acc = torch.zeros_like(x).index_add_(0, i, x[j])
        x = torch.where(has, x + s * (acc * inv_deg - x), x)
    return x


def entry(name, v, f, a):
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_smooth import MODE_LAPLACIAN, smooth_mesh, vertex_adjacency
    V = int(v.shape[0])
    e = {"mesh": name, "vertices": V, "faces": int(f.shape[0])}
    e["adjacency"], (off, nb) = measure(lambda: vertex_adjacency(V, f), a.reps)
    E = int(nb.numel())
    deg = off[1:] - off[:-1]
    e["entries"], e["mean_degree"], e["max_degree"] = E, E / V, int(deg.max())
    taubin = [0.5, -0.53] * a.iterations
    tmp = torch.empty_like(v)
    x1, x20 = v.clone(), v.clone()
    e["step"] = measure(lambda: _mesh_ops.smooth_steps(off, nb, x1.copy_(v), MODE_LAPLACIAN, [0.5], None, tmp), a.reps)[0]
    e["copy_of_input"] = measure(lambda: x1.copy_(v), a.reps)[0]        # both timings above and below include this restore
    row = torch.repeat_interleave(torch.arange(V, device=v.device), deg)
    col = nb.long()
    inv_deg = (1.0 / deg.clamp(min=1).float())[:, None]
    has = (deg > 0)[:, None]
    hip = lambda: _mesh_ops.smooth_steps(off, nb, x20.copy_(v), MODE_LAPLACIAN, taubin, None, tmp)
    ref = lambda: index_add_filter(v, row, col, inv_deg, has, taubin)
    hip(), ref()
    torch.cuda.synchronize()
    hip_ms, ref_ms = [], []
    for _ in range(a.reps):                                  # alternating: both see the same state of the machine
        hip_ms.append(timed(hip)[0])
        t, ref_x = timed(ref)
        ref_ms.append(t)
    e["steps_%d" % len(taubin)], e["index_add_%d" % len(taubin)] = stats(hip_ms), stats(ref_ms)
    e["max_abs_difference_to_index_add"] = float((ref_x - x20).abs().max())
    per_step = (e["steps_%d" % len(taubin)]["median_ms"] - e["copy_of_input"]["median_ms"]) / len(taubin)
    e["per_step_ms"] = per_step
    e["speedup_over_index_add"] = e["index_add_%d" % len(taubin)]["median_ms"] / e["steps_%d" % len(taubin)]["median_ms"]
    C = 3
    e["step_bytes"] = V * (2 * 4 * C + 8) + E * (4 + 4 * C)
    e["step_bytes_per_s"] = e["step_bytes"] / (per_step * 1e-3)
    e["step_fraction_of_hbm_peak"] = e["step_bytes_per_s"] / HBM_PEAK_BYTES_PER_S
    e["smooth_mesh"], out = measure(lambda: smooth_mesh(v, f, method="taubin", iterations=a.iterations), a.reps)
    e["results_bit_identical_to_raw_steps"] = bool(torch.equal(out[0].view(torch.int32), x20.view(torch.int32)))
    e["adjacency_share_of_smooth_mesh"] = e["adjacency"]["median_ms"] / e["smooth_mesh"]["median_ms"]
    e["steps_share_of_smooth_mesh"] = per_step * len(taubin) / e["smooth_mesh"]["median_ms"]
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=288)
    ap.add_argument("--sheet", type=int, default=742)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_timing.json"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "layout": _mesh_ops.smooth_layout(), "filter": "taubin x %d" % a.iterations,
              "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "entries": []}
    v, f, c, h = sphere_mesh(a.grid, dev)
    meshes = [("sphere r = 0.9, %d^3, extracted on the device" % a.grid, v, f),
              ("sheet %d x %d, vertex ids shuffled" % (a.sheet, a.sheet),) + shuffled_sheet(a.sheet, dev)]
    for name, mv, mf in meshes:
        e = entry(name, mv.contiguous(), mf, a)
        result["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
