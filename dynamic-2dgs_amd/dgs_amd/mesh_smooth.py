"""Mesh smoothing on the tensors' own device: simple, Laplacian and Taubin filters, without open3d.

  smooth_mesh(method="simple")     <- open3d's TriangleMesh.filter_smooth_simple(number_of_iterations)
  smooth_mesh(method="laplacian")  <- filter_smooth_laplacian(number_of_iterations, lambda_filter)
  smooth_mesh(method="taubin")     <- filter_smooth_taubin(number_of_iterations, lambda_filter, mu)

An extracted surface is the zero set of a trilinear TSDF sampled at one voxel: it carries a staircase of about a voxel, and every
frame carries another one.  A step moves every vertex towards the mean of its neighbours; "laplacian" shrinks the shape as it
smooths, "taubin" follows every shrinking step (lam) with an inflating one (mu < -lam) and keeps the volume to first order.

UNIFORM (umbrella) WEIGHTS ONLY -- a stated departure from any distance- or cotangent-weighted variant: every neighbour counts the
same.  The order of a row's sum follows the vertex ids, so the last bits of the result depend on the vertex numbering; renumbering
a mesh changes them and nothing else.

include/dgs_mesh_ops.h states the step.  Its sum is sequential in row order and every operation is rounded on its own, so the HIP
kernel (dgs_smooth_steps) and the PyTorch statement below (smooth_steps_torch) give the same bits.  HIP tensors run the kernel, CPU
tensors the statement; the adjacency before them (a sort of packed 64-bit keys and a prefix sum) is PyTorch on the tensors' device
either way."""
import math

import numpy as np
import torch

from .mesh_topology import _check_mesh, _faces_checked, undirected_edges

_METHODS = ("simple", "laplacian", "taubin")
MODE_LAPLACIAN, MODE_SIMPLE = 0, 1


# ---- adjacency ------------------------------------------------------------------------------------------------------------------
def vertex_adjacency(n_vertices, faces):
    """(offsets [V+1] int64, neighbours [E] int32) on the device of faces [F,3]: row i = neighbours[offsets[i]:offsets[i+1]] lists
    the distinct vertices j != i that share a face with i, ascending.  From the six directed pairs of every face, packed as
    i << 32 | j: pairs with i == j are dropped (a face may name a vertex twice), unique() sorts and removes the repeats (repeated
    faces do not repeat a neighbour), a prefix sum of the row lengths gives the offsets.  ValueError: a face index outside [0, V),
    E >= 2^31."""
    f = _faces_checked("vertex_adjacency", n_vertices, faces)
    V, dev = int(n_vertices), faces.device
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    i = torch.cat((a, b, b, c, c, a))
    j = torch.cat((b, a, c, b, a, c))
    keep = i != j
    key = torch.unique((i[keep] << 32) | j[keep])               # sorted: by i, then by j
    if key.numel() >= 2 ** 31:
        raise ValueError("vertex_adjacency: %d entries do not fit int32 row indices" % key.numel())
    degree = torch.bincount(key >> 32, minlength=V) if key.numel() else torch.zeros(V, dtype=torch.int64, device=dev)
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(degree, 0)
    return offsets, (key & 0xFFFFFFFF).to(torch.int32)


def boundary_vertices(n_vertices, faces):
    """bool [V] on the device of faces: the endpoints of the undirected edges that lie in exactly one face (the runs of
    mesh_topology.undirected_edges of length 1; an edge from a vertex to itself is no edge).  ValueError: a face index outside [0, V)."""
    f = _faces_checked("boundary_vertices", n_vertices, faces)
    V, dev = int(n_vertices), faces.device
    mark = torch.zeros(V, dtype=torch.bool, device=dev)
    key, _, start, count = undirected_edges(f)
    edge = key[start]
    once = edge[(count == 1) & ((edge >> 32) != (edge & 0xFFFFFFFF))]
    mark[once >> 32] = True
    mark[once & 0xFFFFFFFF] = True
    return mark


# ---- the statement --------------------------------------------------------------------------------------------------------------
def _slots(offsets, neighbours):
    """The rows cut into slots: [(rows int64, ids int64)] for k = 0, 1, ...: the rows longer than k and their k-th neighbour.  One
    stable sort of the entries by their position in the row and one host read of the slot sizes."""
    V, E = offsets.numel() - 1, neighbours.numel()
    if E == 0:
        return []
    degree = offsets[1:] - offsets[:-1]
    row = torch.repeat_interleave(torch.arange(V, device=offsets.device), degree)
    slot = torch.arange(E, device=offsets.device) - offsets[row]
    order = torch.argsort(slot, stable=True)                    # within a slot: rows ascending, each at most once
    sizes = torch.bincount(slot).tolist()
    rows, ids = row[order], neighbours.long()[order]
    out, at = [], 0
    for n in sizes:
        out.append((rows[at:at + n], ids[at:at + n]))
        at += n
    return out


def smooth_steps_torch(offsets, neighbours, x, mode, factors, pinned=None):
    """The steps of include/dgs_mesh_ops.h on x [V,C] (fp32, or fp64 for a reference) -> a new tensor.  A row is walked slot by
    slot: for slot k, acc = where(k < d, acc + x[neighbours[offsets[:-1] + k]], acc), vectorised over the vertices -- written as an
    indexed update of the rows longer than k, which touches the same entries -- so every row is summed in its own order, the
    kernel's.  factors: one Python number per step, taken as fp32."""
    V, dev, dt = x.shape[0], x.device, x.dtype
    slots = _slots(offsets, neighbours)
    d = (offsets[1:] - offsets[:-1])
    den = (d if mode == MODE_LAPLACIAN else d + 1).to(dt)[:, None]          # float(d), float(d + 1): one rounding of an integer
    still = d == 0
    if pinned is not None:
        still = still | pinned.bool()
    still = still[:, None]
    for s in factors:
        acc = torch.zeros_like(x)
        for rows, ids in slots:
            acc[rows] = acc[rows] + x[ids]
        if mode == MODE_LAPLACIAN:
            s_t = torch.full((1,), float(np.float32(s)), dtype=dt, device=dev)   # a tensor, not a number: the product is the dtype's own
            new = x + s_t * (acc / den - x)
        else:
            new = (x + acc) / den
        x = torch.where(still, x, new)
    return x


def _factors(method, iterations, lam, mu):
    """(mode, [factor per step])"""
    if method == "simple":
        return MODE_SIMPLE, [0.0] * iterations
    if method == "laplacian":
        return MODE_LAPLACIAN, [lam] * iterations
    return MODE_LAPLACIAN, [lam, mu] * iterations


# ---- the function ---------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def smooth_mesh(vertices, faces, colors=None, method="taubin", iterations=10, lam=0.5, mu=-0.53, pin_boundary=False, pinned=None,
                smooth_colors=False):
    """open3d's filter_smooth_simple / _laplacian / _taubin with uniform weights -> (vertices [V,3] fp32, faces, colors) on the
    tensors' device.  Faces are returned as given, colours too unless smooth_colors is set: then they ride through the same steps
    as channels 3..5 and are clamped to [0, 1] at the end.
      method        "simple": iterations steps p <- (p + sum of neighbours) / (d + 1);  "laplacian": iterations steps
                    p <- p + lam (mean of neighbours - p);  "taubin" (default): iterations times (a step with lam, a step with mu)
      pin_boundary  hold the vertices of boundary_vertices() where they are (an open mesh otherwise shrinks from its rim)
      pinned        bool [V]: further vertices to hold
    A vertex without neighbours stays.  iterations=0 returns the input's bits.
    ValueError: a method outside the three, iterations negative or not an integer, lam or mu not finite (as fp32), vertices not fp32
    or not finite, pinned of another shape or dtype, a face index out of range.  HIP tensors run the kernel of libdgs_mesh_ops.so
    -- a missing library is an error --, CPU tensors the PyTorch statement above: the results are bit-identical.  They depend on
    the vertex numbering in their last bits (the order of a row's sum follows the ids)."""
    _check_mesh("smooth_mesh", vertices, faces, colors)
    if vertices.dtype != torch.float32:
        raise ValueError("smooth_mesh: vertices must be fp32 [V,3]")
    if method not in _METHODS:
        raise ValueError("smooth_mesh: method must be 'simple', 'laplacian' or 'taubin', not %r" % (method,))
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError("smooth_mesh: iterations must be a non-negative integer")
    iterations = int(iterations)
    fac = {}
    for name, val in (("lam", lam), ("mu", mu)):
        if isinstance(val, bool) or not isinstance(val, (int, float, np.floating, np.integer)):
            raise ValueError("smooth_mesh: %s must be a number" % name)
        with np.errstate(over="ignore"):
            fac[name] = float(np.float32(val))
        if not math.isfinite(fac[name]):
            raise ValueError("smooth_mesh: %s must be finite (as fp32)" % name)
    V, dev = vertices.shape[0], vertices.device
    if pinned is not None and not (torch.is_tensor(pinned) and pinned.dtype == torch.bool and pinned.shape == (V,) and pinned.device == dev):
        raise ValueError("smooth_mesh: pinned must be a bool tensor [V] on the device of the vertices")
    if smooth_colors and (colors is None or colors.dtype != torch.float32 or colors.shape != vertices.shape):
        raise ValueError("smooth_mesh: smooth_colors needs fp32 colors [V,3]")
    f = _faces_checked("smooth_mesh", V, faces)
    if V and not bool(torch.isfinite(vertices).all()):
        raise ValueError("smooth_mesh: non-finite vertex coordinates")
    mode, factors = _factors(method, iterations, fac["lam"], fac["mu"])
    keep_c = None if colors is None else colors.clone()
    if not factors or V == 0:
        return vertices.clone(), faces.clone(), keep_c
    offsets, neighbours = vertex_adjacency(V, f)
    hold = pinned
    if pin_boundary:
        rim = boundary_vertices(V, f)
        hold = rim if hold is None else hold | rim
    x = torch.cat((vertices, colors), 1).contiguous() if smooth_colors else vertices.contiguous().clone()
    if dev.type == "cpu":
        x = smooth_steps_torch(offsets, neighbours, x, mode, factors, hold)
    else:
        from . import _mesh_ops   # a missing library is an error, never a reason to run the PyTorch statement instead
        cap = _mesh_ops.smooth_layout()[3]
        hold8 = None if hold is None else hold.to(torch.uint8)
        tmp = torch.empty_like(x)
        for at in range(0, len(factors), cap):                                  # (cap is even: a taubin pair is never cut)
            _mesh_ops.smooth_steps(offsets, neighbours, x, mode, factors[at:at + cap], hold8, tmp)
    if smooth_colors:
        return x[:, :3].contiguous(), faces.clone(), x[:, 3:].clamp(0.0, 1.0).contiguous()
    return x, faces.clone(), keep_c


# ---- shell ----------------------------------------------------------------------------------------------------------------------
def main(argv=None):
    import argparse
    import os
    from . import io as dio
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.mesh_smooth",
                                 description="Smooth a triangle mesh (open3d's filter_smooth_simple / _laplacian / _taubin, uniform weights).")
    ap.add_argument("input", help=".ply or .obj")
    ap.add_argument("output", help=".ply")
    ap.add_argument("--method", choices=_METHODS, default="taubin")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--mu", type=float, default=-0.53)
    ap.add_argument("--pin-boundary", action="store_true", help="hold the vertices of open edges where they are")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    ext = os.path.splitext(a.input)[1].lower()
    if ext == ".ply":
        v, f, c = dio.read_mesh_ply(a.input)
    elif ext == ".obj":
        (v, f), c = dio.read_mesh_obj(a.input), None
    else:
        raise ValueError("%s is neither .ply nor .obj" % a.input)
    dev = torch.device(a.device)
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    v, f, c = smooth_mesh(to(v), to(f), to(c), method=a.method, iterations=a.iterations, lam=a.lam, mu=a.mu, pin_boundary=a.pin_boundary)
    dio.write_mesh_ply(a.output, v, f, c)
    print("%s -> %s: %d vertices, %d faces, %s x %d" % (a.input, a.output, v.shape[0], f.shape[0], a.method, a.iterations))


if __name__ == "__main__":
    main()
