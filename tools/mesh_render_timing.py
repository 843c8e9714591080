"""Times of the mesh rasterizer behind dgs_amd.mesh_render -> profiles/mesh_render_timing.md.

    python tools/mesh_render_timing.py [--size 800] [--nu 1000] [--reps 20] [--warmup 3] [--torch-faces 8192] [--out profiles/mesh_render_timing.md]

Three things, each timed with device events after --warmup runs, on one device in one process:
  1. render_mesh on a UV sphere of 2 nu (nu / 2 - 1) faces (about 10^6 at the default) at size x size under an orbit camera: the whole
     call (table in PyTorch, list split, two raster launches, resolve); the wrappers on a prepared table (_mesh_ops.raster +
     _mesh_ops.resolve: the split of the faces into the two lists -- two nonzero calls, each a host synchronisation --, the output
     allocations and the launches); and the C calls alone on prepared lists and outputs (dgs_mesh_raster for both paths with the
     clear + dgs_mesh_resolve with three channels: the clear and three launches between the two events);
  2. the same for the two-triangle quad that is larger than the image: every pixel tested twice by the large-box path;
  3. the PyTorch statement (rasterize_torch + interpolate) on the device on the first --torch-faces faces of the sphere, and that time
     SCALED by faces / torch-faces (it walks the faces in chunks of equal size; the table says so).  Bit-identity with the kernels
     is checked on that subset."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return "%.3f (%.3f-%.3f, %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


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
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--nu", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-faces", type=int, default=8192)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render_timing.md"))
    a = ap.parse_args()
    from dgs_amd import _mesh_ops
    from dgs_amd.cameras import Camera, make_camera, pose_spherical
    from dgs_amd.mesh_render import interpolate, raster_table, rasterize_torch, render_mesh
    dev = torch.device("cuda:0")
    S = a.size
    area, threads, row, cmax = _mesh_ops.raster_layout()
    lines = ["# Mesh rasterizer: `dgs_mesh_raster` + `dgs_mesh_resolve` against the PyTorch statement", "",
             "`tools/mesh_render_timing.py` on %s at %d x %d; device events, %d runs after %d warm-up runs, one device, one process; layout: boxes of at most %d pixels "
             "on the one-lane-per-face path, %d threads per workgroup, %d floats per table row." % (torch.cuda.get_device_name(0), S, S, a.reps, a.warmup, area, threads, row),
             "", "| mesh | faces | small / large path | covered pixels | render_mesh ms (median, min-max, runs) | wrappers ms (list split, allocations, launches) | C calls alone ms (clear, raster x 2, resolve) | table (PyTorch) ms |",
             "|---|---|---|---|---|---|---|---|"]

    def measure(name, cam, v, f, c):
        bg = torch.ones(3, device=dev)
        f32 = f.to(torch.int32).contiguous()
        table, box = raster_table(v, f, cam)
        b = box.long()
        ar = (b[:, 1] - b[:, 0] + 1).clamp(min=0) * (b[:, 3] - b[:, 2] + 1).clamp(min=0)
        n_small, n_large = int(((ar > 0) & (ar <= area)).sum()), int((ar > area).sum())
        best = torch.empty(S * S, dtype=torch.int64, device=dev)
        # the C calls alone, on prepared lists and outputs: nothing but the clear and the three launches is between the two events
        lists = [torch.nonzero((ar > 0) & (ar <= area)).reshape(-1).to(torch.int32), torch.nonzero(ar > area).reshape(-1).to(torch.int32)]
        face_id, depth = torch.empty((S, S), dtype=torch.int32, device=dev), torch.empty((S, S), dtype=torch.float32, device=dev)
        bary, image = torch.empty((S, S, 3), dtype=torch.float32, device=dev), torch.empty((3, S, S), dtype=torch.float32, device=dev)
        lib, stream = _mesh_ops.load(), _mesh_ops._stream(dev)

        def kernels():
            for path, lst in enumerate(lists):
                rc = lib.dgs_mesh_raster(table.shape[0], table.data_ptr(), lst.data_ptr() if lst.numel() else None, lst.numel(), path, S, S,
                                         best.data_ptr(), 1 - path, stream)
                assert rc == 0, lib.dgs_mesh_ops_last_error()
            rc = lib.dgs_mesh_resolve(S, S, best.data_ptr(), table.shape[0], table.data_ptr(), f32.data_ptr(), v.shape[0], c.data_ptr(), 3, bg.data_ptr(),
                                      face_id.data_ptr(), depth.data_ptr(), bary.data_ptr(), image.data_ptr(), stream)
            assert rc == 0, lib.dgs_mesh_ops_last_error()

        whole = lambda: render_mesh(cam, v, f, c)
        wrappers = lambda: _mesh_ops.resolve(_mesh_ops.raster(table, box, S, S, best), table, f32, S, S, c, bg)
        tab = lambda: raster_table(v, f, cam)
        res = {}
        for key, fn in (("whole", whole), ("wrappers", wrappers), ("kernels", kernels), ("table", tab)):
            for _ in range(a.warmup):
                timed(fn)
            res[key] = [timed(fn)[0] for _ in range(a.reps)]
        assert torch.equal(face_id, whole()["face"])
        out = whole()
        lines.append("| %s | %d | %d / %d | %d | %s | %s | %s | %s |" % (name, f.shape[0], n_small, n_large, int((out["face"] >= 0).sum()), stats(res["whole"]),
                                                                      stats(res["wrappers"]), stats(res["kernels"]), stats(res["table"])))
        print(lines[-1], flush=True)
        return table, box, res

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    cam = make_camera(pose_spherical(30.0, -30.0, 2.6), 0.6911, 0.6911, S, S, 0.0).to(dev)
    v, f = uv_sphere(0.8, a.nu, a.nu // 2)
    v, f = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    c = (0.5 + 0.45 * torch.sin(3.0 * v / 0.8)).contiguous()
    table, box, res = measure("UV sphere", cam, v, f, c)
    flush()
    # the statement on a subset of the sphere
    n = min(a.torch_faces, f.shape[0])
    sub_t, sub_b, sub_f = table[:n].contiguous(), box[:n].contiguous(), f[:n].contiguous()

    def statement():
        face, depth, bary = rasterize_torch(sub_t, sub_b, S, S)
        return face, depth, bary, interpolate(c, sub_f, sub_t, face, bary, depth, torch.ones(3))

    timed(statement)
    t_ms = []
    for _ in range(a.torch_reps):
        ms, st = timed(statement)
        t_ms.append(ms)
    hip = _mesh_ops.resolve(_mesh_ops.raster(sub_t, sub_b, S, S), sub_t, sub_f.to(torch.int32).contiguous(), S, S, c, torch.ones(3, device=dev))
    same = bool(torch.equal(hip[0], st[0]) and torch.equal(hip[1].view(torch.int32), st[1].view(torch.int32)) and torch.equal(hip[2], st[2])
                and torch.equal(hip[3], st[3]))
    scaled = statistics.median(t_ms) * f.shape[0] / n
    lines += ["", "PyTorch statement (`rasterize_torch` + `interpolate`) on the device, first %d faces of the sphere: %s ms; scaled by %d / %d: "
              "%.0f ms, %.0fx the C calls' %.3f ms; bit-identical to the kernels on those faces: %s." %
              (n, stats(t_ms), f.shape[0], n, scaled, scaled / statistics.median(res["kernels"]), statistics.median(res["kernels"]), "yes" if same else "NO"), ""]
    print(lines[-2], flush=True)
    flush()
    # the quad, in a camera whose screen coordinates are the vertex coordinates over their depth
    m = torch.zeros(4, 4)
    m[0, 0], m[2, 0], m[1, 1], m[2, 1], m[2, 3] = 2.0 / S, 1.0 / S - 1.0, 2.0 / S, 1.0 / S - 1.0, 1.0
    qcam = Camera(S, S, 1.0, 1.0, torch.eye(4), m, torch.zeros(3), torch.zeros(1)).to(dev)
    qv = torch.tensor([[-0.75 * S, -1.25 * S, 1.0], [1.8 * S, -1.25 * S, 1.0], [1.8 * S, 2.1 * S, 1.0], [-0.75 * S, 2.1 * S, 1.0]], device=dev) * 2.0
    qf = torch.tensor([[0, 1, 2], [0, 2, 3]], device=dev)
    lines += ["| mesh | faces | small / large path | covered pixels | render_mesh ms (median, min-max, runs) | wrappers ms (list split, allocations, launches) | C calls alone ms (clear, raster x 2, resolve) | table (PyTorch) ms |",
              "|---|---|---|---|---|---|---|---|"]
    measure("quad larger than the image", qcam, qv, qf, torch.rand(4, 3, device=dev))
    flush()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
