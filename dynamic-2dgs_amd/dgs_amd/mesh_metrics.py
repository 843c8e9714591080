"""Geometry metrics between two triangle meshes: how far the surface written by dgs_amd.mesh is from a ground-truth surface.  The
reference's meshes are judged on the DG-Mesh benchmark by the Chamfer distance to a ground-truth mesh per frame (its tree carries
the reader of those, read_gt_mesh.py: load_obj); this module samples both surfaces, finds every sample's nearest neighbour in the
other set and reports the directed means, Chamfer distance, precision / recall / F-score and normal consistency.

  nearest          all-pairs nearest neighbour; HIP device: dgs_nn_search of libdgs_mesh_ops.so (include/dgs_mesh_ops.h states the
                   arithmetic and the tie rule); CPU tensors: nearest_torch, the PyTorch statement of the same arithmetic
  sample_surface   area-weighted uniform samples of a mesh, the same points on every device
  mesh_distance    the metrics of one pair of meshes
  read_mesh        .ply (io.read_mesh_ply) or .obj (io.read_mesh_obj)
  evaluate_meshes  frame_<i>.ply of a directory against the i-th ground-truth mesh of another -> mesh_metrics.json

On a HIP device a missing library is an error, never a reason to run the PyTorch statement instead."""
import json
import math
import os
import re

import numpy as np
import torch

_PAIR_BUDGET = 1 << 24   # elements of one [chunk, Nr] intermediate of nearest_torch


# ---- nearest neighbour ----------------------------------------------------------------------------------------------------------
def nearest_torch(query, ref, chunk=None):
    """The arithmetic of dgs_nn_search in PyTorch, in the dtype and on the device of the tensors, chunked over the queries:
    d2 = (dx * dx + dy * dy) + dz * dz as elementwise operations (one rounding each), the minimum over the reference set, and
    among equal distances the lowest index -- written out, not left to what torch.min returns.
    -> (d2 [Nq], idx [Nq] int64).  Also the comparator of the GPU tests and the baseline of tools/mesh_metrics_timing.py."""
    nq, nr = query.shape[0], ref.shape[0]
    if nr < 1:
        raise ValueError("nearest: the reference set is empty")
    if chunk is None:
        chunk = max(1, _PAIR_BUDGET // nr)
    rx, ry, rz = ref[:, 0].unsqueeze(0), ref[:, 1].unsqueeze(0), ref[:, 2].unsqueeze(0)
    index = torch.arange(nr, dtype=torch.int64, device=ref.device).unsqueeze(0)
    d2 = torch.empty(nq, dtype=query.dtype, device=query.device)
    idx = torch.empty(nq, dtype=torch.int64, device=query.device)
    for s in range(0, nq, chunk):
        q = query[s:s + chunk]
        dx, dy, dz = q[:, 0:1] - rx, q[:, 1:2] - ry, q[:, 2:3] - rz
        d = dx * dx + dy * dy + dz * dz
        m = d.min(dim=1, keepdim=True).values
        d2[s:s + chunk] = m[:, 0]
        idx[s:s + chunk] = torch.where(d == m, index, nr).min(dim=1).values
    return d2, idx


def _points(x, what):
    if not torch.is_tensor(x) or x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
        raise ValueError("nearest: %s must be a floating-point tensor [N,3]" % what)
    if not bool(torch.isfinite(x).all()):
        raise ValueError("nearest: %s holds non-finite coordinates" % what)
    return x


@torch.no_grad()
def nearest(query, ref, ref_chunk=None):
    """(d2 [Nq], idx [Nq] int64): squared distance to, and index of, the nearest point of ref [Nr,3] for every point of query
    [Nq,3]; equal distances go to the lowest index.  HIP tensors (fp32): the kernel, ref_chunk = its slice of the reference set per
    workgroup (the result does not depend on it); CPU tensors: nearest_torch in their dtype.  Nr = 0 and non-finite coordinates
    raise ValueError before anything is launched."""
    _points(query, "query"), _points(ref, "ref")
    if ref.shape[0] < 1:
        raise ValueError("nearest: the reference set is empty")
    if query.device != ref.device:
        raise ValueError("nearest: query and ref live on different devices")
    if query.device.type == "cpu":
        return nearest_torch(query, ref)
    from . import _mesh_ops
    return _mesh_ops.nearest(query.float().contiguous(), ref.float().contiguous(), ref_chunk)


# ---- sampling -------------------------------------------------------------------------------------------------------------------
def _mesh_tensors(mesh, device):
    v, f = mesh[0], mesh[1]
    v = (v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v))).to(device)
    f = (f.detach() if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))).to(device)
    return v.reshape(-1, 3), f.reshape(-1, 3).long()


@torch.no_grad()
def sample_surface(vertices, faces, n, seed):
    """n points uniform over the surface of the mesh -> (points [n,3] f32, face_ids [n] int64, normals [n,3] f32 -- the unit normal
    of each point's face) on the device of `vertices`.  The uniforms are [n,3] float64 from a CPU torch.Generator().manual_seed(seed),
    so every device samples the same points; face areas and their cumulative sum are float64.  Face: searchsorted(cum, u0 * total,
    right=True) clamped to Nf - 1 (a zero-area face spans an empty interval and is never drawn); point: (1 - sqrt(u1)) A +
    sqrt(u1) (1 - u2) B + sqrt(u1) u2 C.  ValueError for a mesh without faces or with total area 0."""
    dev = vertices.device
    v = vertices.detach().reshape(-1, 3).double()
    f = faces.detach().reshape(-1, 3).long().to(dev)
    if f.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cross = torch.cross(b - a, c - a, dim=1)
    twice = (cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1] + cross[:, 2] * cross[:, 2]).sqrt()
    cum = torch.cumsum(0.5 * twice, 0)
    total = cum[-1]
    if not float(total) > 0.0 or not math.isfinite(float(total)):
        raise ValueError("sample_surface: the total area of the mesh is %r" % float(total))
    u = torch.rand((int(n), 3), dtype=torch.float64, generator=torch.Generator().manual_seed(int(seed))).to(dev)
    fid = torch.searchsorted(cum, (u[:, 0] * total).contiguous(), right=True).clamp(max=f.shape[0] - 1)
    fid = _skip_empty(fid, twice)
    s = u[:, 1].sqrt().unsqueeze(1)
    t = u[:, 2].unsqueeze(1)
    pts = (1 - s) * a[fid] + s * (1 - t) * b[fid] + s * t * c[fid]
    nrm = cross[fid] / twice[fid].unsqueeze(1)
    return pts.float(), fid, nrm.float()


def _skip_empty(fid, twice):
    """The clamp of searchsorted can only land on the last face; should that one have no area (u0 * total rounding up to the total),
    the draw goes to the last face that has some."""
    if bool((twice[fid] > 0).all()):
        return fid
    good = torch.nonzero(twice > 0).reshape(-1)
    pos = torch.searchsorted(good, fid, right=True).clamp(min=1) - 1
    return torch.where(twice[fid] > 0, fid, good[pos])


# ---- metrics of one pair --------------------------------------------------------------------------------------------------------
def _tkey(tau):
    return "%g" % tau


@torch.no_grad()
def mesh_distance(pred, gt, n_samples=100_000, seed=0, thresholds=(0.005, 0.01, 0.02), device="cuda:0", gt_transform=None):
    """Metrics between the surfaces of pred and gt, each a (vertices [Nv,3], faces [Nf,3]) pair of arrays or tensors.  n_samples
    points are drawn on pred with `seed` and on gt with `seed + 1` (sample_surface), then `nearest` runs both ways on `device`.
    gt_transform: optional [4,4] (column-vector convention, x' = M[:3,:3] x + M[:3,3]) applied to the ground-truth vertices first.

    Conventions: distances are Euclidean, in the units of the meshes, NOT squared unless the name says so; nothing is halved.
      accuracy            mean over the pred samples of the distance to the nearest gt sample
      completeness        mean over the gt samples of the distance to the nearest pred sample
      chamfer             accuracy + completeness
      chamfer_sq          the same sum with squared distances
      precision[tau]      share of the pred samples within tau of gt (<=);  recall[tau]: share of the gt samples within tau of pred
      fscore[tau]         2 P R / (P + R), 0 where P + R = 0
      normal_consistency  mean |n . n'| of a sample's face normal and its nearest neighbour's, averaged over the two directions
      n_samples, pred_faces, gt_faces, pred_vertices, gt_vertices
    The per-threshold entries are dicts keyed by '%g' % tau.  Sample-to-sample distances carry the sampling floor: a surface against
    itself measures about 0.5 sqrt(area / n_samples) per direction, not 0."""
    dev = torch.device(device)
    pv, pf = _mesh_tensors(pred, dev)
    gv, gf = _mesh_tensors(gt, dev)
    if gt_transform is not None:
        m = torch.as_tensor(np.asarray(gt_transform, dtype=np.float64), device=dev)
        gv = (gv.double() @ m[:3, :3].T + m[:3, 3]).to(gv.dtype)
    pp, _, pn = sample_surface(pv, pf, n_samples, seed)
    gp, _, gn = sample_surface(gv, gf, n_samples, seed + 1)
    d2_pg, i_pg = nearest(pp, gp)
    d2_gp, i_gp = nearest(gp, pp)
    d_pg, d_gp = d2_pg.double().sqrt(), d2_gp.double().sqrt()
    out = {"accuracy": float(d_pg.mean()), "completeness": float(d_gp.mean())}
    out["chamfer"] = out["accuracy"] + out["completeness"]
    out["chamfer_sq"] = float(d2_pg.double().mean()) + float(d2_gp.double().mean())
    out["precision"], out["recall"], out["fscore"] = {}, {}, {}
    for tau in thresholds:
        p, r = float((d_pg <= tau).double().mean()), float((d_gp <= tau).double().mean())
        out["precision"][_tkey(tau)], out["recall"][_tkey(tau)] = p, r
        out["fscore"][_tkey(tau)] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    nc_p = (pn.double() * gn[i_pg].double()).sum(1).abs().mean()
    nc_g = (gn.double() * pn[i_gp].double()).sum(1).abs().mean()
    out["normal_consistency"] = 0.5 * (float(nc_p) + float(nc_g))
    out.update(n_samples=int(n_samples), pred_faces=int(pf.shape[0]), gt_faces=int(gf.shape[0]), pred_vertices=int(pv.shape[0]),
               gt_vertices=int(gv.shape[0]))
    return out


# ---- files ----------------------------------------------------------------------------------------------------------------------
def read_mesh(path):
    """(vertices [Nv,3] float32, faces [Nf,3] int32) of a .ply (io.read_mesh_ply) or .obj (io.read_mesh_obj) file."""
    from . import io as dio
    ext = os.path.splitext(path)[1].lower()
    if ext == ".ply":
        v, f, _ = dio.read_mesh_ply(path)
        return v, f
    if ext == ".obj":
        return dio.read_mesh_obj(path)
    raise ValueError("read_mesh: %s is neither .ply nor .obj" % path)


def _natural(name):
    return [int(t) if t.isdigit() else t.lower() for t in re.split(r"(\d+)", name)]


def _flat(m):
    """The scalar entries of a mesh_distance result: 'fscore' {'0.01': x} -> 'fscore@0.01': x."""
    out = {}
    for k, v in m.items():
        if isinstance(v, dict):
            out.update({"%s@%s" % (k, t): x for t, x in v.items()})
        else:
            out[k] = v
    return out


def evaluate_meshes(pred_dir, gt_dir, n_samples=100_000, seed=0, thresholds=(0.005, 0.01, 0.02), device="cuda:0", gt_transform=None, log=None):
    """frame_<i>.ply of pred_dir against the i-th ground-truth mesh of gt_dir (its .obj / .ply files in natural sort order), for
    every i.  A different number of frames and ground-truth meshes is an error.  Writes <pred_dir>/mesh_metrics.json:
    {"frames": [{"frame": i, "pred": ..., "gt": ..., <metrics>}], "mean": {<metric>: mean over the frames}, "settings": ...} with
    the per-threshold metrics flattened to 'fscore@0.01', and returns that dict."""
    frames = {}
    for name in os.listdir(pred_dir):
        m = re.fullmatch(r"frame_(\d+)\.ply", name)
        if m:
            frames[int(m.group(1))] = name
    gts = sorted((n for n in os.listdir(gt_dir) if os.path.splitext(n)[1].lower() in (".obj", ".ply")), key=_natural)
    if len(frames) != len(gts) or sorted(frames) != list(range(len(frames))):
        raise ValueError("evaluate_meshes: %d frame_<i>.ply files in %s (i = %s) but %d ground-truth meshes in %s"
                         % (len(frames), pred_dir, sorted(frames)[:3] + (["..."] if len(frames) > 3 else []), len(gts), gt_dir))
    if not frames:
        raise ValueError("evaluate_meshes: no frame_<i>.ply in %s" % pred_dir)
    rows = []
    for i in range(len(gts)):
        m = _flat(mesh_distance(read_mesh(os.path.join(pred_dir, frames[i])), read_mesh(os.path.join(gt_dir, gts[i])), n_samples=n_samples,
                                seed=seed, thresholds=thresholds, device=device, gt_transform=gt_transform))
        rows.append(dict({"frame": i, "pred": frames[i], "gt": gts[i]}, **m))
        if log is not None:
            log("frame %d (%s vs %s): chamfer %.6f, accuracy %.6f, completeness %.6f, normal consistency %.4f"
                % (i, frames[i], gts[i], m["chamfer"], m["accuracy"], m["completeness"], m["normal_consistency"]))
    keys = [k for k in rows[0] if k not in ("frame", "pred", "gt")]
    result = {"frames": rows, "mean": {k: sum(r[k] for r in rows) / len(rows) for k in keys},
              "settings": {"n_samples": int(n_samples), "seed": int(seed), "thresholds": [float(t) for t in thresholds], "device": str(device),
                           "gt_transform": None if gt_transform is None else np.asarray(gt_transform, dtype=np.float64).tolist()}}
    with open(os.path.join(pred_dir, "mesh_metrics.json"), "w") as fh:
        json.dump(result, fh, indent=1)
    return result


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_metrics",
                                 description="Chamfer distance, F-score and normal consistency of frame_<i>.ply against ground-truth meshes.")
    ap.add_argument("pred_dir")
    ap.add_argument("gt_dir")
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.005, 0.01, 0.02])
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    return evaluate_meshes(a.pred_dir, a.gt_dir, n_samples=a.samples, seed=a.seed, thresholds=tuple(a.thresholds), device=a.device, log=print)


if __name__ == "__main__":
    main()
