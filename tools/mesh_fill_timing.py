"""Times of mesh hole filling on extracted meshes -> profiles/mesh_fill_timing.json.

    python tools/mesh_fill_timing.py [--sizes 256 512] [--views 60] [--pixels 800] [--holes 48] [--reps 10] [--max-edges 128] [--out ...]

The meshes of tools/mesh_timing.py: DynamicTruth(t = 0.25) rendered from --views cameras, fused at --sizes^3 and extracted on the
device; then --holes discs of faces (everything within 1 .. 12 rings of a seed vertex) are taken out.  Reported per mesh, device
events, one warm-up, medians of --reps:
  fill_holes   the whole function with the HIP kernels and with the PyTorch statement on the same device, alternating, and whether
               the two results are bit-identical
  kernels      dgs_fill_rank, dgs_fill_rim and dgs_fill_emit alone, on the tables of the same call
  phases       the phases of one call, the device synchronised after each: loops (the sorts, run lengths, dgs_cc_labels and
               dgs_fill_rank), layout (prefix sums, the host read, the output buffers), rim, emit -- the split between the PyTorch
               tables and the kernels
  loops        how many loops the mesh has, how many were closed, the longest closed one, what the fill added"""
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

from mesh_timing import cameras, stats, timed, truth_model


def punch(v, f, c, n_holes, seed=0):
    """Take n_holes discs of faces out of the mesh, on its device: the faces whose corners all lie within r rings of a seed."""
    from dgs_amd.mesh_topology import _compact
    V, fl = v.shape[0], f.long()
    g = torch.Generator().manual_seed(seed)
    seeds = torch.randint(0, V, (n_holes,), generator=g).tolist()
    gone = torch.zeros(f.shape[0], dtype=torch.bool, device=f.device)
    for k, s in enumerate(seeds):
        mark = torch.zeros(V, dtype=torch.bool, device=f.device)
        mark[s] = True
        for _ in range(1 + k % 12):
            mark[fl[mark[fl].any(1)].reshape(-1)] = True
        gone |= mark[fl].all(1)
    return _compact(v, f[~gone], c, torch.ones(int((~gone).sum()), dtype=torch.bool, device=f.device))


def same(a, b):
    bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x
    return all((x is None and y is None) or (x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y))) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--holes", type=int, default=48)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--max-edges", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_fill_timing.json"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops, mesh_fill as mf, mesh_topology
    from dgs_amd.mesh import TSDFVolume, views_at_time
    from dgs_amd.mesh_topology import _frame
    dev = torch.device("cuda:0")
    t = 0.25
    model = truth_model(t, dev)
    side, lo = 2.8, (-1.3, -1.4, -1.4)
    depth, rgb, proj = views_at_time(model, None, cameras(a.views, a.pixels, t), t, torch.zeros(3, device=dev))
    result = {"device": torch.cuda.get_device_name(0), "scene": "DynamicTruth(t=0.25)", "views": a.views, "pixels": a.pixels,
              "max_hole_edges": a.max_edges, "layout": _mesh_ops.fill_layout(), "entries": []}
    for N in a.sizes:
        h = side / (N - 1)
        vol = TSDFVolume(lo, h, (N, N, N), dev).integrate(depth, rgb, proj, trunc=5 * h)
        v, f, c = punch(*vol.extract(), a.holes)
        del vol
        V, F = v.shape[0], f.shape[0]
        sizes = mf.boundary_loops(V, f)[1].diff()
        fill = lambda: mf.fill_holes(v, f, c, max_hole_edges=a.max_edges)

        def statement():
            mesh_topology._STATEMENT_EVERYWHERE = True
            try:
                return mf.fill_holes(v, f, c, max_hole_edges=a.max_edges)
            finally:
                mesh_topology._STATEMENT_EVERYWHERE = False

        want, got = fill(), statement()                      # warm-up of both (the library, the allocator)
        torch.cuda.synchronize()
        hip_ms, torch_ms = [], []
        for _ in range(a.reps):                              # alternating
            hip_ms.append(timed(fill)[0])
            torch_ms.append(timed(statement)[0])
        # the kernels alone, on the tables of the same call
        tab = mf.rank_inputs(V, mf._proper(f.long()), a.max_edges)
        succ = tab["succ"].to(torch.int32)
        lv, off, _ = mf._loops(V, mf._proper(f.long()), a.max_edges)
        centre, scale = _frame(v)
        centre = [float(x) for x in centre.tolist()]
        lay = mf.ring_layout(V, off)
        rim_loop = torch.repeat_interleave(torch.arange(off.shape[0] - 1, dtype=torch.int32, device=dev), off.diff())
        vout = torch.cat((v, torch.empty((lay["n_new"], 3), device=dev)))
        cout = torch.cat((c, torch.empty((lay["n_new"], 3), device=dev)))
        fout = torch.empty((lay["n_new_faces"], 3), dtype=torch.int32, device=dev)
        S, SC, rows = _mesh_ops.fill_rim(v, c, lv, rim_loop, off, centre, scale)
        calls = {"dgs_fill_rank": lambda: _mesh_ops.fill_rank(succ, tab["leader"], tab["n_rounds"]),
                 "dgs_fill_rim": lambda: _mesh_ops.fill_rim(v, c, lv, rim_loop, off, centre, scale),
                 "dgs_fill_emit": lambda: _mesh_ops.fill_emit(V, lay, lv, off, rows, S, SC, centre, scale, vout, cout, fout)}
        kernels = {}
        for name, call in calls.items():
            call()
            torch.cuda.synchronize()
            kernels[name] = stats([timed(call)[0] for _ in range(a.reps)])
        phases, last = {}, [0.0]

        def clock(phase):
            torch.cuda.synchronize()
            now = time.perf_counter()
            phases[phase] = phases.get(phase, 0.0) + (now - last[0]) * 1e3
            last[0] = now

        runs = []
        for _ in range(a.reps):
            phases.clear()
            torch.cuda.synchronize()
            last[0] = time.perf_counter()
            mf.fill_holes(v, f, c, max_hole_edges=a.max_edges, clock=clock)
            runs.append(dict(phases))
        split = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
        closed = sizes[(sizes <= a.max_edges)]
        e = {"grid": N, "vertices": V, "faces": F, "boundary_half_edges": int(tab["succ"].shape[0]), "loops": int(sizes.shape[0]),
             "loops_closed": int(closed.shape[0]), "longest_closed": int(closed.max()) if closed.numel() else 0, "rank_rounds": tab["n_rounds"],
             "new_vertices": int(want[0].shape[0] - V), "new_faces": int(want[1].shape[0] - F),
             "loops_left": int(mf.boundary_loops(want[0].shape[0], want[1])[1].shape[0] - 1),
             "fill_holes_hip": stats(hip_ms), "fill_holes_statement": stats(torch_ms),
             "speedup": statistics.median(torch_ms) / statistics.median(hip_ms), "results_bit_identical": bool(same(want, got)),
             "kernels": kernels, "phases_ms": split}
        result["entries"].append(e)
        print(json.dumps(e), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
        del v, f, c, want, got
        torch.cuda.empty_cache()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
