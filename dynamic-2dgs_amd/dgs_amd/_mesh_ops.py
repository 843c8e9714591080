"""ctypes binding of libdgs_mesh_ops.so (include/dgs_mesh_ops.h): TSDF fusion, marching tetrahedra, the all-pairs nearest-neighbour
and closest-triangle searches, the auction solver of the earth mover's distance, the z-buffer triangle rasterizer, the connected components, the
quadric vertex clustering, the smoothing steps, the edge collapse rounds and the hole filling for gfx950, used by dgs_amd.mesh,
dgs_amd.mesh_metrics, dgs_amd.mesh_render, dgs_amd.mesh_clean, dgs_amd.mesh_simplify, dgs_amd.mesh_smooth, dgs_amd.mesh_decimate and
dgs_amd.mesh_fill when the data lives on a HIP device.  CPU tensors use the PyTorch /
NumPy statements in those modules."""
import ctypes
import os

import torch

import _dgs_build
from . import _ops

_CSRC = _ops._CSRC
# -ffp-contract=off: the fuser's accept / reject decisions sit on thresholds; with every operation rounded on its own the kernel
# and the PyTorch statement of the same arithmetic take the same side of every one of them
HIPCC_FLAGS = list(_ops.HIPCC_FLAGS) + ["-ffp-contract=off"]
# name -> (restype, argtypes) of every function include/dgs_mesh_ops.h declares, grouped like csrc/mesh_ops.hip.  Written by hand:
# tests/test_cabi_exports.py compares names, arities and return types with the header.
_ci, _vp, _cf, _ll, _cd = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_longlong, ctypes.c_double
_SEARCH = [_ll, _vp, _ll, _vp, _ll, _vp, _vp]         # n_query, query, n_set, set, chunk, best, stream
_LAYOUT = [ctypes.POINTER(_ci)]
_SIGNATURES = {
    "dgs_mesh_ops_abi_version": (_ci, []),
    "dgs_mesh_ops_last_error": (ctypes.c_char_p, []),
    # fusion and marching tetrahedra
    "dgs_tsdf_integrate": (_ci, [_ci, _ci, _ci, _cf, _cf, _cf, _cf, _ci, _ci, _ci, _vp, _vp, _vp, _cf, _cf, _cf, _ci, _vp, _vp, _vp, _vp]),
    "dgs_mt_classify": (_ci, [_ci, _ci, _ci] + [_vp] * 6),
    "dgs_mt_emit": (_ci, [_ci, _ci, _ci, _cf, _cf, _cf, _cf, _vp, _vp, _ll, _vp, _vp, _vp, _ll] + [_vp] * 7),
    # the two searches
    "dgs_nn_search": (_ci, _SEARCH),
    "dgs_nn_layout": (_ci, _LAYOUT),
    "dgs_tri_search": (_ci, _SEARCH),
    "dgs_tri_layout": (_ci, _LAYOUT),
    # earth mover's distance (its kernels close mesh_search_kernels.h)
    "dgs_emd_auction": (_ci, [_ll, _vp, _vp, _cf, _ll, _vp, _ll, _vp, _vp, _vp, _vp]),
    "dgs_emd_layout": (_ci, _LAYOUT),
    # triangle rasterizer
    "dgs_mesh_raster": (_ci, [_ll, _vp, _vp, _ll, _ci, _ci, _ci, _vp, _ci, _vp]),
    "dgs_mesh_resolve": (_ci, [_ci, _ci, _vp, _ll, _vp, _vp, _ll, _vp, _ci] + [_vp] * 6),
    "dgs_mesh_raster_layout": (_ci, _LAYOUT),
    # connected components
    "dgs_cc_labels": (_ci, [_ll, _vp, _ll, _ci, _vp, _vp]),
    "dgs_cc_layout": (_ci, _LAYOUT),
    # quadric vertex clustering (its kernels close mesh_cc_kernels.h)
    "dgs_simplify_accumulate": (_ci, [_ll, _vp, _vp, _ll, _vp, _vp, _ll, _vp, _cf, _vp, _vp]),
    "dgs_simplify_solve": (_ci, [_ll, _vp, _vp, _cf, _ci, _vp, _vp, _vp]),
    "dgs_simplify_layout": (_ci, _LAYOUT),
    # Laplacian / Taubin smoothing (its kernel closes mesh_cc_kernels.h)
    "dgs_smooth_steps": (_ci, [_ll, _vp, _vp, _ll, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp]),
    "dgs_smooth_layout": (_ci, _LAYOUT),
    # quadric edge collapse in rounds (its kernels close mesh_cc_kernels.h)
    "dgs_decimate_quadrics": (_ci, [_ll, _vp, _ll, _vp, _cf, _ci, _vp, _vp]),
    "dgs_decimate_edges": (_ci, [_ll, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _ll, _vp, _vp, _ll, _ci, _cf, _vp, _vp, _vp, _vp]),
    "dgs_decimate_select": (_ci, [_ll, _ll] + [_vp] * 7),
    "dgs_decimate_apply": (_ci, [_ll] + [_vp] * 6 + [_ll, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp]),
    "dgs_decimate_layout": (_ci, _LAYOUT),
    # hole filling: list ranking, loop sums and smoothed rims, ring emission (its kernels close mesh_cc_kernels.h)
    "dgs_fill_rank": (_ci, [_ll, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "dgs_fill_rim": (_ci, [_ll, _vp, _vp, _ll, _vp, _vp, _ll, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp]),
    "dgs_fill_emit": (_ci, [_ll, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp]),
    "dgs_fill_layout": (_ci, _LAYOUT),
}
_SOURCES = ["mesh_ops.hip", "mesh_common.h", "mesh_fusion_kernels.h", "mesh_search_kernels.h", "mesh_raster_kernels.h", "mesh_cc_kernels.h"]
_LIB = _dgs_build.NativeLibrary(
    os.path.join(_CSRC, "libdgs_mesh_ops.so"), os.path.join(_CSRC, _SOURCES[0]),
    [os.path.join(_CSRC, n) for n in _SOURCES] + [os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "dgs_mesh_ops.h")],
    HIPCC_FLAGS, _SIGNATURES, ("dgs_mesh_ops_abi_version", 2), "dgs_mesh_ops_last_error")
LIB_PATH = _LIB.path
_deps, source_hash, build, load = _LIB.deps, _LIB.source_hash, _LIB.build, _LIB.load
_stream = _dgs_build.stream


def exported_symbols():
    return tuple(_SIGNATURES)


def _check(lib, rc, what):
    _LIB.check(rc, what)


def _f32(t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError("%s: a contiguous fp32 HIP tensor is expected" % what)
    return t


def tsdf_integrate(dims, origin, voxel, depth, rgb, proj, trunc, depth_trunc, prior_weight, accumulate, tsdf, weight, color):
    """dgs_tsdf_integrate on the volume tensors tsdf / weight [Nx,Ny,Nz] and color [Nx,Ny,Nz,3] (in place)."""
    lib = load()
    dev = tsdf.device
    V, H, W = depth.shape
    n = dims[0] * dims[1] * dims[2]
    if rgb.shape != (V, 3, H, W) or proj.shape != (V, 16) or tsdf.numel() != n or weight.numel() != n or color.numel() != 3 * n:
        raise RuntimeError("tsdf_integrate: depth [V,H,W], rgb [V,3,H,W], proj [V,16] and a volume of the given dims are expected")
    for t, what in ((depth, "depth"), (rgb, "rgb"), (proj, "proj"), (tsdf, "tsdf"), (weight, "weight"), (color, "color")):
        _f32(t, what)
        if t.device != dev:
            raise RuntimeError("tsdf_integrate: %s lives on another device than the volume" % what)
    with torch.cuda.device(dev):
        rc = lib.dgs_tsdf_integrate(dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], voxel, V, H, W, depth.data_ptr(), rgb.data_ptr(),
                                    proj.data_ptr(), trunc, depth_trunc, prior_weight, 1 if accumulate else 0, tsdf.data_ptr(),
                                    weight.data_ptr(), color.data_ptr(), _stream(dev))
    _check(lib, rc, "dgs_tsdf_integrate")


def marching_tetrahedra(dims, origin, voxel, tsdf, weight, color=None):
    """(vertices [Nv,3] f32, faces [Nf,3] int32, colors [Nv,3] f32 or None) of the volume, in the order of include/dgs_mesh_ops.h.
    PyTorch does the plumbing between the two passes: two prefix sums, the lists of active cells and of vertex-carrying grid
    points, and the one host read of the two totals that sizes the outputs."""
    lib = load()
    dev = tsdf.device
    Nx, Ny, Nz = dims
    n = Nx * Ny * Nz
    _f32(tsdf, "tsdf"), _f32(weight, "weight")
    if color is not None:
        _f32(color, "color")
    cell_tris = torch.empty(n, dtype=torch.int32, device=dev)
    point_verts = torch.empty(n, dtype=torch.int32, device=dev)
    point_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib, lib.dgs_mt_classify(Nx, Ny, Nz, tsdf.data_ptr(), weight.data_ptr(), cell_tris.data_ptr(), point_verts.data_ptr(),
                                        point_mask.data_ptr(), _stream(dev)), "dgs_mt_classify")
    tri_incl = torch.cumsum(cell_tris, 0, dtype=torch.int64)
    vert_incl = torch.cumsum(point_verts, 0, dtype=torch.int64)
    n_tris, n_verts = (int(x) for x in torch.stack((tri_incl[-1], vert_incl[-1])).tolist())
    if n_verts >= 2 ** 31 or n_tris >= 2 ** 31:
        raise RuntimeError("marching_tetrahedra: %d vertices / %d triangles do not fit the int32 face indices" % (n_verts, n_tris))
    vertices = torch.empty((n_verts, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((n_tris, 3), dtype=torch.int32, device=dev)
    colors = torch.empty((n_verts, 3), dtype=torch.float32, device=dev) if color is not None else None
    if n_tris:
        cells = torch.nonzero(cell_tris).reshape(-1)
        points = torch.nonzero(point_mask).reshape(-1)
        with torch.cuda.device(dev):
            rc = lib.dgs_mt_emit(Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel, tsdf.data_ptr(), None if color is None else color.data_ptr(),
                                 cells.numel(), cells.data_ptr(), cell_tris.data_ptr(), tri_incl.data_ptr(), points.numel(), points.data_ptr(),
                                 point_mask.data_ptr(), vert_incl.data_ptr(), vertices.data_ptr(), None if colors is None else colors.data_ptr(),
                                 faces.data_ptr(), _stream(dev))
        _check(lib, rc, "dgs_mt_emit")
    return vertices, faces, colors


def _layout(name, n):
    lib = load()
    out = (ctypes.c_int * n)()
    _check(lib, getattr(lib, name)(out), name)
    return tuple(int(v) for v in out)


def _search(who, entry, layout, chunk, query, qname, ref, rname, cols, expected):
    """nearest and closest_face: device and dtype checks, the chunk default (layout[2]), the `best` buffer, the call and the
    unpacking of the packed minimum."""
    lib = load()
    dev = query.device
    _f32(query, qname), _f32(ref, rname)
    if ref.device != dev:
        raise RuntimeError("%s: %s lives on another device than %s" % (who, rname, qname))
    if query.dim() != 2 or query.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != cols:
        raise RuntimeError("%s: %s are expected" % (who, expected))
    chunk = layout[2] if chunk is None else int(chunk)
    best = torch.empty(query.shape[0], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(query.shape[0], query.data_ptr(), ref.shape[0], ref.data_ptr(), chunk, best.data_ptr(), _stream(dev))
    _check(lib, rc, entry)
    # the packed values are below 2^63 (d2 >= 0: sign bit clear), so the signed shift and mask are the unsigned ones
    return (best >> 32).to(torch.int32).view(torch.float32), best & 0xFFFFFFFF


def nn_layout():
    """(queries per workgroup, reference points per LDS round, default ref_chunk) of dgs_nn_search."""
    return _layout("dgs_nn_layout", 3)


def nearest(query, ref, ref_chunk=None):
    """dgs_nn_search: (d2 [Nq] f32, idx [Nq] int64) of the nearest point of ref [Nr,3] for every point of query [Nq,3]; equal
    distances go to the lowest index.  The result does not depend on ref_chunk (default: nn_layout()[2])."""
    return _search("nearest", "dgs_nn_search", nn_layout(), ref_chunk, query, "query", ref, "ref", 3, "query [Nq,3] and ref [Nr,3]")


def tri_layout():
    """(queries per workgroup, triangles per LDS round, default tri_chunk, floats per table row) of dgs_tri_search."""
    return _layout("dgs_tri_layout", 4)


def closest_face(points, table, tri_chunk=None):
    """dgs_tri_search: (d2 [Nq] f32, face [Nq] int64) of the closest triangle of table [Nf,row] (mesh_metrics.triangle_table) for
    every point of points [Nq,3]; equal distances go to the lowest face.  The result does not depend on tri_chunk (default:
    tri_layout()[2])."""
    layout = tri_layout()
    return _search("closest_face", "dgs_tri_search", layout, tri_chunk, points, "points", table, "table", layout[3],
                   "points [Nq,3] and table [Nf,%d]" % layout[3])


def emd_layout():
    """(threads per workgroup, objects per LDS round of the dense bidding kernel, largest bidder count of the sparse bidding kernel,
    entries of the result array, fixed bytes of scratch, bytes of scratch per point) of dgs_emd_auction."""
    return _layout("dgs_emd_layout", 6)


EMD_CAP, EMD_OVERFLOW = -3, -4   # statuses of dgs_emd_auction: max_rounds reached; a bid that does not fit 40 bits


def emd_auction(a, b, inv_q, max_rounds, scratch=None):
    """dgs_emd_auction on persons a [n,3] and objects b [n,3] (fp32 HIP tensors) -> (assignment [n] int32, prices [n] int64, primal,
    dual, rounds, max cost).  inv_q: mesh_metrics._emd_quantum.  scratch: an optional uint8 HIP tensor to reuse (emd_layout gives
    its size).  RuntimeError when max_rounds is reached (the message names the phase, eps and the bidders left) or a bid overflows."""
    lib = load()
    dev = a.device
    _f32(a, "a"), _f32(b, "b")
    if b.device != dev:
        raise RuntimeError("emd_auction: b lives on another device than a")
    if a.dim() != 2 or a.shape[1] != 3 or b.shape != a.shape:
        raise RuntimeError("emd_auction: a [n,3] and b [n,3] are expected")
    n = a.shape[0]
    lay = emd_layout()
    need = lay[4] + n * lay[5]
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not (scratch.is_cuda and scratch.device == dev and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= need):
        raise RuntimeError("emd_auction: scratch must be a contiguous uint8 tensor of at least %d bytes on the device of a" % need)
    assignment = torch.empty(n, dtype=torch.int32, device=dev)
    prices = torch.empty(n, dtype=torch.int64, device=dev)
    result = (ctypes.c_longlong * lay[3])()
    with torch.cuda.device(dev):
        rc = lib.dgs_emd_auction(n, a.data_ptr(), b.data_ptr(), float(inv_q), int(max_rounds), scratch.data_ptr(), scratch.numel(),
                                 assignment.data_ptr(), prices.data_ptr(), ctypes.cast(result, ctypes.c_void_p), _stream(dev))
    _check(lib, rc, "dgs_emd_auction")
    return assignment, prices, int(result[0]), int(result[1]), int(result[2]), int(result[3])


def raster_layout():
    """(largest box area of the one-lane-per-face path, threads per workgroup, floats per table row, largest C) of dgs_mesh_raster."""
    return _layout("dgs_mesh_raster_layout", 4)


def raster(table, box, H, W, best=None):
    """dgs_mesh_raster for every face of table [Nf,row] (mesh_render.raster_table) with a non-empty box [Nf,4] int32: the faces are
    split by box area into the two paths' lists (a compare + nonzero) and each path is launched once, the first call clearing
    `best`.  -> best [H*W] int64 (the packed minima; -1 = all-ones where nothing was drawn).  A `best` passed in is reused: it is
    fully re-initialised."""
    lib = load()
    dev = table.device
    layout = raster_layout()
    _f32(table, "table")
    if table.dim() != 2 or table.shape[1] != layout[2] or box.shape != (table.shape[0], 4) or box.dtype != torch.int32 or box.device != dev:
        raise RuntimeError("raster: table [Nf,%d] fp32 and box [Nf,4] int32 on one device are expected" % layout[2])
    if best is None:
        best = torch.empty(H * W, dtype=torch.int64, device=dev)
    elif not (best.is_cuda and best.device == dev and best.dtype == torch.int64 and best.is_contiguous() and best.numel() == H * W):
        raise RuntimeError("raster: best must be a contiguous int64 tensor of H * W elements on the table's device")
    b = box.long()
    area = (b[:, 1] - b[:, 0] + 1).clamp(min=0) * (b[:, 3] - b[:, 2] + 1).clamp(min=0)
    small = torch.nonzero((area > 0) & (area <= layout[0])).reshape(-1).to(torch.int32)
    large = torch.nonzero(area > layout[0]).reshape(-1).to(torch.int32)
    with torch.cuda.device(dev):
        for path, lst, clear in ((0, small, 1), (1, large, 0)):
            rc = lib.dgs_mesh_raster(table.shape[0], table.data_ptr(), lst.data_ptr() if lst.numel() else None, lst.numel(), path, H, W,
                                     best.data_ptr(), clear, _stream(dev))
            _check(lib, rc, "dgs_mesh_raster")
    return best


def resolve(best, table, faces, H, W, attr=None, background=None):
    """dgs_mesh_resolve -> (face_id [H,W] int32, depth [H,W], bary [H,W,3], image [C,H,W] or None).  faces [Nf,3] int32; attr
    [Nv,C] fp32 with background [C], or None for no image."""
    lib = load()
    dev = table.device
    _f32(table, "table")
    if not (faces.is_cuda and faces.dtype == torch.int32 and faces.is_contiguous() and faces.shape == (table.shape[0], 3)):
        raise RuntimeError("resolve: faces must be a contiguous int32 HIP tensor [Nf,3]")
    face_id = torch.empty((H, W), dtype=torch.int32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    bary = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    C, image, nv = 0, None, 0
    if attr is not None:
        _f32(attr, "attr"), _f32(background, "background")
        nv, C = attr.shape
        if background.numel() != C:
            raise RuntimeError("resolve: background must hold one value per channel")
        image = torch.empty((C, H, W), dtype=torch.float32, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        rc = lib.dgs_mesh_resolve(H, W, best.data_ptr(), table.shape[0], ptr(table), ptr(faces), nv, ptr(attr), C, ptr(background),
                                  face_id.data_ptr(), depth.data_ptr(), bary.data_ptr(), ptr(image), _stream(dev))
    _check(lib, rc, "dgs_mesh_resolve")
    return face_id, depth, bary, image


def cc_layout():
    """(threads per workgroup, groups per thread) of dgs_cc_labels: a workgroup takes their product of groups."""
    return _layout("dgs_cc_layout", 2)


def cc_labels(groups, n_nodes):
    """dgs_cc_labels -> label [n_nodes] int32 on the device of groups [G,k] (int32, contiguous, k in {2, 3}): the smallest node id of
    every node's component.  An id outside [0, n_nodes) is a ValueError (one aminmax, read on the host)."""
    lib = load()
    dev = groups.device
    if not (groups.is_cuda and groups.dtype == torch.int32 and groups.is_contiguous()):
        raise RuntimeError("cc_labels: a contiguous int32 HIP tensor is expected")
    if groups.dim() != 2 or groups.shape[1] not in (2, 3):
        raise RuntimeError("cc_labels: groups [G,2] or [G,3] are expected")
    n_nodes = int(n_nodes)
    if n_nodes < 0 or n_nodes >= 2 ** 31:
        raise ValueError("cc_labels: n_nodes must be in [0, 2^31)")
    if groups.shape[0]:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(groups)).tolist())
        if lo < 0 or hi >= n_nodes:
            raise ValueError("cc_labels: node ids in [%d, %d] but n_nodes is %d" % (lo, hi, n_nodes))
    label = torch.empty(n_nodes, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_cc_labels(n_nodes, groups.data_ptr() if groups.shape[0] else None, groups.shape[0], groups.shape[1],
                               label.data_ptr() if n_nodes else None, _stream(dev))
    _check(lib, rc, "dgs_cc_labels")
    return label


def simplify_layout():
    """(threads per workgroup, items per thread, Q, W_MAX, exponent of lambda) of dgs_simplify_accumulate / dgs_simplify_solve."""
    return _layout("dgs_simplify_layout", 5)


def simplify_accumulate(vertices, colors, faces, cluster, centres, cell):
    """dgs_simplify_accumulate -> rows [C,16] int64 on the device of vertices [V,3]: colors [V,3] or None, faces [F,3] int32, cluster
    [V] int32 (the cell of every vertex), centres [C,3], cell a float."""
    lib = load()
    dev = vertices.device
    _f32(vertices, "vertices"), _f32(centres, "centres")
    if colors is not None:
        _f32(colors, "colors")
    for t, what in ((faces, "faces"), (cluster, "cluster")):
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
            raise RuntimeError("simplify_accumulate: %s must be a contiguous int32 HIP tensor" % what)
    V, F, C = vertices.shape[0], faces.shape[0], centres.shape[0]
    if vertices.shape != (V, 3) or faces.shape != (F, 3) or cluster.shape != (V,) or centres.shape != (C, 3) or (colors is not None and colors.shape != (V, 3)):
        raise RuntimeError("simplify_accumulate: vertices [V,3], colors [V,3], faces [F,3], cluster [V] and centres [C,3] are expected")
    if any(t is not None and t.device != dev for t in (colors, faces, cluster, centres)):
        raise RuntimeError("simplify_accumulate: every tensor must live on the device of vertices")
    rows = torch.empty((C, 16), dtype=torch.int64, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        rc = lib.dgs_simplify_accumulate(V, ptr(vertices), ptr(colors), F, ptr(faces), ptr(cluster), C, ptr(centres), float(cell), ptr(rows), _stream(dev))
    _check(lib, rc, "dgs_simplify_accumulate")
    return rows


def simplify_solve(rows, centres, cell, quadric=True, with_colors=False):
    """dgs_simplify_solve -> (vertices [C,3] f32, colors [C,3] f32 or None) from the rows of simplify_accumulate."""
    lib = load()
    dev = rows.device
    _f32(centres, "centres")
    C = centres.shape[0]
    if not (rows.is_cuda and rows.dtype == torch.int64 and rows.is_contiguous() and rows.shape == (C, 16)) or centres.shape != (C, 3) or centres.device != dev:
        raise RuntimeError("simplify_solve: rows [C,16] int64 and centres [C,3] fp32 on one HIP device are expected")
    vertices = torch.empty((C, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((C, 3), dtype=torch.float32, device=dev) if with_colors else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        rc = lib.dgs_simplify_solve(C, ptr(rows), ptr(centres), float(cell), 1 if quadric else 0, ptr(vertices), ptr(colors), _stream(dev))
    _check(lib, rc, "dgs_simplify_solve")
    return vertices, colors


def smooth_layout():
    """(threads per workgroup, vertices per workgroup, largest C, largest n_steps of one call) of dgs_smooth_steps."""
    return _layout("dgs_smooth_layout", 4)


def smooth_steps(offsets, neighbours, x, mode, factors, pinned=None, tmp=None):
    """dgs_smooth_steps, in place on x [V,C] (fp32, contiguous, C in [1, 8]) -> x: one step per entry of factors (Python numbers,
    taken as fp32) of mode 0 (laplacian) or 1 (simple) over the rows offsets [V+1] int64 / neighbours [E] int32
    (mesh_smooth.vertex_adjacency).  pinned: [V] uint8 or bool, or None; tmp: an optional buffer like x to reuse.  At most
    smooth_layout()[3] steps a call."""
    lib = load()
    dev = x.device
    _f32(x, "x")
    if x.dim() != 2:
        raise RuntimeError("smooth_steps: x [V,C] is expected")
    V, C = x.shape
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.shape == (V + 1,)):
        raise RuntimeError("smooth_steps: offsets must be a contiguous int64 HIP tensor [V+1]")
    if not (neighbours.is_cuda and neighbours.dtype == torch.int32 and neighbours.is_contiguous() and neighbours.dim() == 1):
        raise RuntimeError("smooth_steps: neighbours must be a contiguous int32 HIP tensor [E]")
    if pinned is not None:
        if not (pinned.is_cuda and pinned.dtype in (torch.uint8, torch.bool) and pinned.is_contiguous() and pinned.shape == (V,)):
            raise RuntimeError("smooth_steps: pinned must be a contiguous uint8 or bool HIP tensor [V]")
    if tmp is None:
        tmp = torch.empty_like(x)
    elif not (tmp.is_cuda and tmp.dtype == torch.float32 and tmp.is_contiguous() and tmp.shape == x.shape) or tmp.data_ptr() == x.data_ptr():
        raise RuntimeError("smooth_steps: tmp must be another contiguous fp32 HIP tensor of the shape of x")
    if any(t is not None and t.device != dev for t in (offsets, neighbours, pinned, tmp)):
        raise RuntimeError("smooth_steps: every tensor must live on the device of x")
    host = (ctypes.c_float * max(len(factors), 1))(*[float(s) for s in factors])
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        rc = lib.dgs_smooth_steps(V, ptr(offsets), ptr(neighbours), neighbours.numel(), C, int(mode), ctypes.cast(host, ctypes.c_void_p), len(factors),
                                  ptr(pinned), ptr(x), ptr(tmp), _stream(dev))
    _check(lib, rc, "dgs_smooth_steps")
    return x


def decimate_layout():
    """(threads per workgroup, items per thread, Q_MAX, Q_BUDGET, W_MAX, exponent of lambda, least valence of an interior opposite
    vertex, fixed-point bits of mean_len) of the dgs_decimate_* calls."""
    return _layout("dgs_decimate_layout", 8)


def _dec(t, dtype, shape, what):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise RuntimeError("%s must be a contiguous %s HIP tensor %s" % (what, str(dtype).replace("torch.", ""), list(shape)))
    return t


_ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None


def decimate_quadrics(pos, faces, mean_len, q_bits):
    """dgs_decimate_quadrics -> rows [V,10] int64 on the device of pos [V,3] (the frame) for faces [F,3] int32."""
    lib = load()
    dev = pos.device
    V, F = pos.shape[0], faces.shape[0]
    _dec(pos, torch.float32, (V, 3), "decimate_quadrics: pos"), _dec(faces, torch.int32, (F, 3), "decimate_quadrics: faces")
    if faces.device != dev:
        raise RuntimeError("decimate_quadrics: every tensor must live on the device of pos")
    rows = torch.empty((V, 10), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_decimate_quadrics(V, _ptr(pos), F, _ptr(faces), float(mean_len), int(q_bits), _ptr(rows), _stream(dev))
    _check(lib, rc, "dgs_decimate_quadrics")
    return rows


def decimate_edges(pos, rows, faces, tab, q_bits, max_cost):
    """dgs_decimate_edges -> (cost [E] fp32, place [E,3] fp32, valid [E] bool) for the tables of mesh_decimate.round_tables."""
    lib = load()
    dev = pos.device
    V, F, E = pos.shape[0], faces.shape[0], tab["edges"].shape[1]
    _dec(pos, torch.float32, (V, 3), "decimate_edges: pos"), _dec(rows, torch.int64, (V, 10), "decimate_edges: rows")
    _dec(faces, torch.int32, (F, 3), "decimate_edges: faces"), _dec(tab["edges"], torch.int32, (5, E), "decimate_edges: edges")
    _dec(tab["flags"], torch.uint8, (V,), "decimate_edges: flags")
    _dec(tab["adj_offsets"], torch.int64, (V + 1,), "decimate_edges: adj_offsets"), _dec(tab["vf_offsets"], torch.int64, (V + 1,), "decimate_edges: vf_offsets")
    adj, vf = tab["adj"], tab["vf"]
    _dec(adj, torch.int32, (adj.numel(),), "decimate_edges: adj"), _dec(vf, torch.int32, (vf.numel(),), "decimate_edges: vf")
    if any(t.device != dev for t in (rows, faces, tab["edges"], tab["flags"], tab["adj_offsets"], adj, tab["vf_offsets"], vf)):
        raise RuntimeError("decimate_edges: every tensor must live on the device of pos")
    cost = torch.empty(E, dtype=torch.float32, device=dev)
    place = torch.empty((E, 3), dtype=torch.float32, device=dev)
    valid = torch.empty(E, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_decimate_edges(V, _ptr(pos), _ptr(rows), _ptr(tab["flags"]), F, _ptr(faces), E, _ptr(tab["edges"]), _ptr(tab["adj_offsets"]),
                                    _ptr(adj), adj.numel(), _ptr(tab["vf_offsets"]), _ptr(vf), vf.numel(), int(q_bits), float(max_cost), _ptr(cost),
                                    _ptr(place), _ptr(valid), _stream(dev))
    _check(lib, rc, "dgs_decimate_edges")
    return cost, place, valid.bool()


def decimate_select(n_vertices, edges, cost, compete):
    """dgs_decimate_select -> (m1 [V] int64, m2 [V] int64, selected [E] bool) for edges [5,E] int32, cost [E] fp32, compete [E] bool."""
    lib = load()
    dev = cost.device
    V, E = int(n_vertices), edges.shape[1]
    _dec(edges, torch.int32, (5, E), "decimate_select: edges"), _dec(cost, torch.float32, (E,), "decimate_select: cost")
    _dec(compete, torch.bool, (E,), "decimate_select: compete")
    if edges.device != dev or compete.device != dev:
        raise RuntimeError("decimate_select: every tensor must live on the device of cost")
    m1 = torch.empty(V, dtype=torch.int64, device=dev)
    m2 = torch.empty(V, dtype=torch.int64, device=dev)
    selected = torch.empty(E, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_decimate_select(V, E, _ptr(edges), _ptr(cost), _ptr(compete), _ptr(m1), _ptr(m2), _ptr(selected), _stream(dev))
    _check(lib, rc, "dgs_decimate_select")
    return m1, m2, selected.bool()


def decimate_apply(pos, rows, colors, moved, faces, tab, place, sel):
    """dgs_decimate_apply, in place on pos [V,3], rows [V,10], colors [V,3] or None, moved [V] bool and faces [F,3] int32 (re-indexed)
    -> (vmap [V] int32, faces, keep [F] bool) for the selected edge ids sel [S] int32."""
    lib = load()
    dev = pos.device
    V, F, E, S = pos.shape[0], faces.shape[0], tab["edges"].shape[1], sel.shape[0]
    _dec(pos, torch.float32, (V, 3), "decimate_apply: pos"), _dec(rows, torch.int64, (V, 10), "decimate_apply: rows")
    _dec(moved, torch.bool, (V,), "decimate_apply: moved"), _dec(faces, torch.int32, (F, 3), "decimate_apply: faces")
    _dec(tab["edges"], torch.int32, (5, E), "decimate_apply: edges"), _dec(tab["flags"], torch.uint8, (V,), "decimate_apply: flags")
    _dec(place, torch.float32, (E, 3), "decimate_apply: place"), _dec(sel, torch.int32, (S,), "decimate_apply: sel")
    if colors is not None:
        _dec(colors, torch.float32, (V, 3), "decimate_apply: colors")
    if any(t is not None and t.device != dev for t in (rows, colors, moved, faces, tab["edges"], tab["flags"], place, sel)):
        raise RuntimeError("decimate_apply: every tensor must live on the device of pos")
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_decimate_apply(V, _ptr(pos), _ptr(rows), _ptr(colors), _ptr(tab["flags"]), _ptr(moved), _ptr(vmap), E, _ptr(tab["edges"]),
                                    _ptr(place), S, _ptr(sel), F, _ptr(faces), _ptr(keep), _stream(dev))
    _check(lib, rc, "dgs_decimate_apply")
    return vmap, faces, keep.bool()


def fill_layout():
    """(threads per workgroup, items per thread, fixed-point bits of the position, Newell and colour sums, columns of a ring row, taps
    of the smoothed rim, largest n_rounds) of the dgs_fill_* calls."""
    return _layout("dgs_fill_layout", 8)


def fill_rank(succ, leader, n_rounds, buf_a=None, buf_b=None, rank=None):
    """dgs_fill_rank -> rank [n] int32 (the position in hole order; -1 where leader is -1) for succ, leader [n] int32.  buf_a, buf_b
    [n] int64 and rank may be passed in to be reused; after the call the packed entries lie in buf_a (n_rounds even) or buf_b."""
    lib = load()
    dev = succ.device
    n = succ.shape[0]
    _dec(succ, torch.int32, (n,), "fill_rank: succ"), _dec(leader, torch.int32, (n,), "fill_rank: leader")
    buf_a = torch.empty(n, dtype=torch.int64, device=dev) if buf_a is None else _dec(buf_a, torch.int64, (n,), "fill_rank: buf_a")
    buf_b = torch.empty(n, dtype=torch.int64, device=dev) if buf_b is None else _dec(buf_b, torch.int64, (n,), "fill_rank: buf_b")
    rank = torch.empty(n, dtype=torch.int32, device=dev) if rank is None else _dec(rank, torch.int32, (n,), "fill_rank: rank")
    if any(t.device != dev for t in (leader, buf_a, buf_b, rank)):
        raise RuntimeError("fill_rank: every tensor must live on the device of succ")
    with torch.cuda.device(dev):
        rc = lib.dgs_fill_rank(n, _ptr(succ), _ptr(leader), int(n_rounds), _ptr(buf_a), _ptr(buf_b), _ptr(rank), _stream(dev))
    _check(lib, rc, "dgs_fill_rank")
    return rank


def fill_rim(vertices, colors, loop_vertices, rim_loop, loop_offsets, centre, scale):
    """dgs_fill_rim -> (S [B,3] fp64, SC [B,3] fp64 or None, rows [L,16] int64) for the rims loop_vertices / rim_loop [B] int32,
    loop_offsets [L+1] int64 of vertices [V,3] (colors [V,3] or None); centre: three Python numbers, scale: a power of two."""
    lib = load()
    dev = vertices.device
    V, B, L = vertices.shape[0], loop_vertices.shape[0], loop_offsets.shape[0] - 1
    _dec(vertices, torch.float32, (V, 3), "fill_rim: vertices"), _dec(loop_vertices, torch.int32, (B,), "fill_rim: loop_vertices")
    _dec(rim_loop, torch.int32, (B,), "fill_rim: rim_loop"), _dec(loop_offsets, torch.int64, (L + 1,), "fill_rim: loop_offsets")
    if colors is not None:
        _dec(colors, torch.float32, (V, 3), "fill_rim: colors")
    if any(t is not None and t.device != dev for t in (colors, loop_vertices, rim_loop, loop_offsets)):
        raise RuntimeError("fill_rim: every tensor must live on the device of vertices")
    S = torch.empty((B, 3), dtype=torch.float64, device=dev)
    SC = torch.empty((B, 3), dtype=torch.float64, device=dev) if colors is not None else None
    rows = torch.empty((L, 16), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_fill_rim(V, _ptr(vertices), _ptr(colors), B, _ptr(loop_vertices), _ptr(rim_loop), L, _ptr(loop_offsets), float(centre[0]),
                              float(centre[1]), float(centre[2]), float(scale), _ptr(S), _ptr(SC), _ptr(rows), _stream(dev))
    _check(lib, rc, "dgs_fill_rim")
    return S, SC, rows


def fill_emit(n_old, lay, loop_vertices, loop_offsets, rows, S, SC, centre, scale, vertices_out, colors_out, faces_out):
    """dgs_fill_emit for the layout lay (mesh_fill.ring_layout: "rings" [NR,10], "vert_ring" [n_new], "face_ring" [n_new_faces], all
    int32): writes rows n_old .. n_old + n_new of vertices_out [n_old + n_new,3] fp32 (rows 0 .. n_old hold the input vertices) and of
    colors_out (or None, with SC None) and all of faces_out [n_new_faces,3] int32."""
    lib = load()
    dev = vertices_out.device
    rings, vert_ring, face_ring = lay["rings"], lay["vert_ring"], lay["face_ring"]
    NR, NV, NF, B, L = rings.shape[0], vert_ring.shape[0], face_ring.shape[0], loop_vertices.shape[0], loop_offsets.shape[0] - 1
    n_old = int(n_old)
    _dec(rings, torch.int32, (NR, fill_layout()[5]), "fill_emit: rings"), _dec(vert_ring, torch.int32, (NV,), "fill_emit: vert_ring")
    _dec(face_ring, torch.int32, (NF,), "fill_emit: face_ring"), _dec(loop_vertices, torch.int32, (B,), "fill_emit: loop_vertices")
    _dec(loop_offsets, torch.int64, (L + 1,), "fill_emit: loop_offsets"), _dec(rows, torch.int64, (L, 16), "fill_emit: rows")
    _dec(S, torch.float64, (B, 3), "fill_emit: S"), _dec(vertices_out, torch.float32, (n_old + NV, 3), "fill_emit: vertices_out")
    _dec(faces_out, torch.int32, (NF, 3), "fill_emit: faces_out")
    if (SC is None) != (colors_out is None):
        raise RuntimeError("fill_emit: SC and colors_out come together")
    if SC is not None:
        _dec(SC, torch.float64, (B, 3), "fill_emit: SC"), _dec(colors_out, torch.float32, (n_old + NV, 3), "fill_emit: colors_out")
    if any(t is not None and t.device != dev for t in (rings, vert_ring, face_ring, loop_vertices, loop_offsets, rows, S, SC, colors_out, faces_out)):
        raise RuntimeError("fill_emit: every tensor must live on the device of vertices_out")
    with torch.cuda.device(dev):
        rc = lib.dgs_fill_emit(n_old, NV, _ptr(vert_ring), NF, _ptr(face_ring), NR, _ptr(rings), L, _ptr(loop_offsets), B, _ptr(loop_vertices),
                               _ptr(rows), _ptr(S), _ptr(SC), float(centre[0]), float(centre[1]), float(centre[2]), float(scale),
                               _ptr(vertices_out), _ptr(colors_out), _ptr(faces_out), _stream(dev))
    _check(lib, rc, "dgs_fill_emit")
    return vertices_out, colors_out, faces_out
