"""Times of the component step of mesh extraction -> profiles/mesh_clean_timing.json.

    python tools/mesh_clean_timing.py [--sizes 256 512] [--views 60] [--reps 10] [--pixels 800] [--sheet 900] [--out profiles/mesh_clean_timing.json]

For every grid size: the mesh of tools/mesh_timing.py (DynamicTruth at t = 0.25, fused and extracted on the device), then
  * dgs_cc_labels alone (the three launches, through the ctypes call into a preallocated label array) and through its wrapper
    (dgs_amd._mesh_ops.cc_labels: the id check with its host read and the allocation included),
  * dgs_amd.mesh_clean.filter_components end to end on the device tensors, against
  * dgs_amd.mesh.keep_largest_components on the same device tensors, its device-to-host copy included,
the last two ALTERNATING in one process.  Then the same on an n x n sheet whose vertex ids are permuted (the numbering of a
ground-truth OBJ: not spatially sorted), where the NumPy side runs --sheet-host-reps times (default 1: it takes over a minute).
Device events, one warm-up run of each, medians over --reps."""
import argparse
import ctypes
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

from mesh_timing import cameras, stats, timed, truth_model


def same(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu())) for x, y in zip(a, b))


def permuted_sheet(n, seed=0):
    ii, jj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack((ii, jj, np.zeros_like(ii)), -1).reshape(-1, 3).astype(np.float32)
    a = (ii[:-1, :-1] * n + jj[:-1, :-1]).reshape(-1)
    f = np.concatenate((np.stack((a, a + 1, a + n), -1), np.stack((a + 1, a + n + 1, a + n), -1)))
    perm = np.random.default_rng(seed).permutation(n * n)
    vp = np.empty_like(v)
    vp[perm] = v
    return vp, perm[f].astype(np.int32)


def measure(name, v, f, c, reps, host_reps):
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh import keep_largest_components
    from dgs_amd.mesh_clean import filter_components
    lib = _mesh_ops.load()
    dev = v.device
    label = torch.empty(v.shape[0], dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def raw():
        rc = lib.dgs_cc_labels(v.shape[0], f.data_ptr(), f.shape[0], 3, label.data_ptr(), stream)
        assert rc == 0
        return label

    raw(), _mesh_ops.cc_labels(f, v.shape[0])
    dev_out = filter_components(v, f, c)                  # warm-up of both sides
    host_out = keep_largest_components(v, f, c) if host_reps > 1 else None      # (a single host repetition is its own warm-up)
    torch.cuda.synchronize()
    raw_ms = [timed(raw)[0] for _ in range(reps)]
    wrap_ms = [timed(lambda: _mesh_ops.cc_labels(f, v.shape[0]))[0] for _ in range(reps)]
    assert torch.equal(label, _mesh_ops.cc_labels(f, v.shape[0]))
    dev_ms, host_ms = [], []
    for r in range(reps):
        dev_ms.append(timed(lambda: filter_components(v, f, c))[0])
        if r < host_reps:
            ms, host_out = timed(lambda: keep_largest_components(v, f, c))
            host_ms.append(ms)
    e = {"mesh": name, "vertices": int(v.shape[0]), "faces": int(f.shape[0]), "components": int(torch.unique(label).numel()),
         "cc_labels_call": stats(raw_ms), "cc_labels_wrapper": stats(wrap_ms), "filter_components_device": stats(dev_ms),
         "faces_kept": int(dev_out[1].shape[0])}
    if host_ms:
        e["keep_largest_components_host_with_copy"] = stats(host_ms)
        e["speedup_filter"] = statistics.median(host_ms) / statistics.median(dev_ms)
        e["results_bit_identical"] = same(dev_out, host_out)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--sheet", type=int, default=900, help="side of the permuted sheet (0: skip it)")
    ap.add_argument("--sheet-host-reps", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_timing.json"))
    a = ap.parse_args()
    from dgs_amd.mesh import TSDFVolume, views_at_time
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "scene": "DynamicTruth(t=0.25)", "pixels": a.pixels, "views": a.views, "entries": []}

    def record(e):
        result["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)

    if a.sizes:
        t = 0.25
        depth, rgb, proj = views_at_time(truth_model(t, dev), None, cameras(a.views, a.pixels, t), t, torch.zeros(3, device=dev))
        side, lo = 2.8, (-1.3, -1.4, -1.4)
        for N in a.sizes:
            h = side / (N - 1)
            vol = TSDFVolume(lo, h, (N, N, N), dev).integrate(depth, rgb, proj, trunc=5 * h)
            v, f, c = vol.extract()
            del vol
            torch.cuda.empty_cache()
            record(measure("DynamicTruth %d^3" % N, v, f, c, a.reps, a.reps))
            del v, f, c
        del depth, rgb, proj
    if a.sheet:
        v, f = permuted_sheet(a.sheet)
        record(measure("%d x %d sheet, vertex ids permuted" % (a.sheet, a.sheet), torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), None,
                       a.reps, a.sheet_host_reps))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
