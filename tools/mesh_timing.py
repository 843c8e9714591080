"""Times of mesh extraction at sizes a user would run -> profiles/mesh_timing.json.

    python tools/mesh_timing.py [--sizes 256 512] [--views 60 100] [--reps 10] [--pixels 800] [--out profiles/mesh_timing.json]

For every (grid size, view count): DynamicTruth at t = 0.25 rendered from cameras spread over the sphere (dgs_amd.mesh.views_at_time),
then TSDFVolume.integrate on the HIP path and the PyTorch statement of the same arithmetic (dgs_amd.mesh.integrate_torch) on the
same device in the same process, ALTERNATING, timed with device events after a warm-up run of each; then TSDFVolume.extract on the
HIP path (events around the whole call, its host read included).  The NumPy extraction runs on the host and is timed once, at
grids up to 256^3 only.  Reported per entry: milliseconds (median, min, max), voxel-views per second, the algorithmic bytes (20 B
written per voxel: tsdf + weight + 3 colour floats; 4 B * V * H * W of depth read once) and the share of the 8 TB/s HBM peak
those bytes imply at the median time."""
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

PEAK_BYTES_PER_S = 8.0e12


def cameras(n, size, t):
    from dgs_amd.cameras import make_camera, pose_spherical
    out = []
    for k in range(n):
        theta = -180.0 + 360.0 * ((k * 0.6180339887) % 1.0)
        phi = -70.0 + 140.0 * ((k * 0.7548776662) % 1.0)
        out.append(make_camera(pose_spherical(theta, phi, 4.0), 0.6911, 0.6911, size, size, t))
    return out


def truth_model(t, device):
    from dgs_amd.model import SurfelModel
    from dgs_amd.synthetic import DynamicTruth, SurfelScene
    xyz, scales, rot, opac, shs = DynamicTruth().state(t)
    scene = SurfelScene(xyz, scales.log(), rot, torch.logit(opac), shs[:, :1].contiguous(), shs[:, 1:].contiguous(), torch.zeros(xyz.shape[0], 8))
    return SurfelModel(scene).to(device)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="*", default=[60, 100])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pixels", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.json"))
    a = ap.parse_args()
    from dgs_amd.mesh import TSDFVolume, _march_numpy, integrate_torch, views_at_time
    dev = torch.device("cuda:0")
    t = 0.25
    model = truth_model(t, dev)
    side, lo = 2.8, (-1.3, -1.4, -1.4)
    result = {"device": torch.cuda.get_device_name(0), "scene": "DynamicTruth(t=0.25)", "pixels": a.pixels, "peak_bytes_per_s": PEAK_BYTES_PER_S,
              "entries": []}
    for V in a.views:
        depth, rgb, proj = views_at_time(model, None, cameras(V, a.pixels, t), t, torch.zeros(3, device=dev))
        for N in a.sizes:
            h = side / (N - 1)
            trunc = 5 * h
            vol = TSDFVolume(lo, h, (N, N, N), dev)

            def run_hip():
                vol.reset()
                return vol.integrate(depth, rgb, proj, trunc=trunc)

            def run_torch():
                z = torch.zeros((N, N, N), dtype=torch.float32, device=dev)
                return integrate_torch(z, z.clone(), torch.zeros((N, N, N, 3), dtype=torch.float32, device=dev), vol.origin, vol.voxel_size, depth, rgb,
                                       proj, trunc, 6.0)

            run_hip(), run_torch()                       # warm-up of both (allocator, code objects)
            torch.cuda.synchronize()
            hip_ms, torch_ms = [], []
            for _ in range(a.reps):
                hip_ms.append(timed(run_hip)[0])
                ms, out = timed(run_torch)
                torch_ms.append(ms)
            same = bool(torch.equal(out[1], vol.weight) and torch.equal(out[0], vol.tsdf))
            del out
            vol.extract()
            torch.cuda.synchronize()
            ext_ms, mesh = [], None
            for _ in range(a.reps):
                ms, mesh = timed(vol.extract)
                ext_ms.append(ms)
            numpy_ms = None
            if N <= 256:
                t0 = time.perf_counter()
                _march_numpy(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.color.cpu().numpy(), vol.origin, vol.voxel_size)
                numpy_ms = (time.perf_counter() - t0) * 1e3
            n_vox = N ** 3
            nbytes = 20 * n_vox + 4 * V * a.pixels * a.pixels
            e = {"grid": N, "views": V, "voxel_views": n_vox * V, "integrate_hip": stats(hip_ms), "integrate_torch": stats(torch_ms),
                 "speedup_integrate": statistics.median(torch_ms) / statistics.median(hip_ms), "results_bit_identical": same,
                 "hip_voxel_views_per_s": n_vox * V / (statistics.median(hip_ms) * 1e-3), "torch_voxel_views_per_s": n_vox * V / (statistics.median(torch_ms) * 1e-3),
                 "algorithmic_bytes": nbytes, "hip_share_of_peak": nbytes / (statistics.median(hip_ms) * 1e-3) / PEAK_BYTES_PER_S,
                 "extract_hip": stats(ext_ms), "extract_numpy_host_ms": numpy_ms, "vertices": int(mesh[0].shape[0]), "faces": int(mesh[1].shape[0])}
            result["entries"].append(e)
            print(json.dumps(e), flush=True)
            del vol, mesh
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
