"""ctypes binding of libdgs_mesh_ops.so (include/dgs_mesh_ops.h): TSDF fusion, marching tetrahedra, the all-pairs nearest-neighbour
and closest-triangle searches, the winding-number sums, the auction solver of the earth mover's distance, the z-buffer triangle rasterizer, the connected components, the
quadric vertex clustering, the smoothing steps, the edge collapse rounds and the hole filling for gfx950, used by dgs_amd.mesh,
dgs_amd.mesh_metrics, dgs_amd.mesh_render, dgs_amd.mesh_clean, dgs_amd.mesh_simplify, dgs_amd.mesh_smooth, dgs_amd.mesh_decimate and
dgs_amd.mesh_fill when the data lives on a HIP device.  CPU tensors use the PyTorch / NumPy statements in those modules."""
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
    # fusion and marching tetrahedra (mesh_fusion_kernels.h)
    "dgs_tsdf_integrate": (_ci, [_ci, _ci, _ci, _cf, _cf, _cf, _cf, _ci, _ci, _ci, _vp, _vp, _vp, _cf, _cf, _cf, _ci, _vp, _vp, _vp, _vp]),
    "dgs_mt_classify": (_ci, [_ci, _ci, _ci] + [_vp] * 6),
    "dgs_mt_emit": (_ci, [_ci, _ci, _ci, _cf, _cf, _cf, _cf, _vp, _vp, _ll, _vp, _vp, _vp, _ll] + [_vp] * 7),
    # the two searches and the winding sums (mesh_search_kernels.h)
    "dgs_nn_search": (_ci, _SEARCH),
    "dgs_nn_layout": (_ci, _LAYOUT),
    "dgs_tri_search": (_ci, _SEARCH),
    "dgs_tri_layout": (_ci, _LAYOUT),
    "dgs_winding_sum": (_ci, _SEARCH),
    "dgs_winding_layout": (_ci, _LAYOUT),
    # earth mover's distance (its kernels close mesh_search_kernels.h)
    "dgs_emd_auction": (_ci, [_ll, _vp, _vp, _cf, _ll, _vp, _ll, _vp, _vp, _vp, _vp]),
    "dgs_emd_layout": (_ci, _LAYOUT),
    # triangle rasterizer (mesh_raster_kernels.h)
    "dgs_mesh_raster": (_ci, [_ll, _vp, _vp, _ll, _ci, _ci, _ci, _vp, _ci, _vp]),
    "dgs_mesh_resolve": (_ci, [_ci, _ci, _vp, _ll, _vp, _vp, _ll, _vp, _ci] + [_vp] * 6),
    "dgs_mesh_raster_layout": (_ci, _LAYOUT),
    # connected components (mesh_cc_kernels.h)
    "dgs_cc_labels": (_ci, [_ll, _vp, _ll, _ci, _vp, _vp]),
    "dgs_cc_layout": (_ci, _LAYOUT),
    # quadric vertex clustering (mesh_simplify_kernels.h)
    "dgs_simplify_accumulate": (_ci, [_ll, _vp, _vp, _ll, _vp, _vp, _ll, _vp, _cf, _vp, _vp]),
    "dgs_simplify_solve": (_ci, [_ll, _vp, _vp, _cf, _ci, _vp, _vp, _vp]),
    "dgs_simplify_layout": (_ci, _LAYOUT),
    # Laplacian / Taubin smoothing (mesh_smooth_kernels.h)
    "dgs_smooth_steps": (_ci, [_ll, _vp, _vp, _ll, _ci, _ci, _vp, _ci, _vp, _vp, _vp, _vp]),
    "dgs_smooth_layout": (_ci, _LAYOUT),
    # quadric edge collapse in rounds (mesh_decimate_kernels.h)
    "dgs_decimate_quadrics": (_ci, [_ll, _vp, _ll, _vp, _cf, _ci, _vp, _vp]),
    "dgs_decimate_edges": (_ci, [_ll, _vp, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _ll, _vp, _vp, _ll, _ci, _cf, _vp, _vp, _vp, _vp]),
    "dgs_decimate_select": (_ci, [_ll, _ll] + [_vp] * 7),
    "dgs_decimate_apply": (_ci, [_ll] + [_vp] * 6 + [_ll, _vp, _vp, _ll, _vp, _ll, _vp, _vp, _vp]),
    "dgs_decimate_layout": (_ci, _LAYOUT),
    # hole filling: list ranking, loop sums and smoothed rims, ring emission (mesh_fill_kernels.h)
    "dgs_fill_rank": (_ci, [_ll, _vp, _vp, _ci, _vp, _vp, _vp, _vp]),
    "dgs_fill_rim": (_ci, [_ll, _vp, _vp, _ll, _vp, _vp, _ll, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp]),
    "dgs_fill_emit": (_ci, [_ll, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _ll, _vp, _vp, _vp, _vp, _cd, _cd, _cd, _cd, _vp, _vp, _vp, _vp]),
    "dgs_fill_layout": (_ci, _LAYOUT),
}
_SOURCES = ["mesh_ops.hip", "mesh_common.h", "mesh_fusion_kernels.h", "mesh_search_kernels.h", "mesh_raster_kernels.h", "mesh_cc_kernels.h",
            "mesh_simplify_kernels.h", "mesh_smooth_kernels.h", "mesh_decimate_kernels.h", "mesh_fill_kernels.h"]
_LIB = _dgs_build.NativeLibrary(
    os.path.join(_CSRC, "libdgs_mesh_ops.so"), os.path.join(_CSRC, _SOURCES[0]),
    [os.path.join(_CSRC, n) for n in _SOURCES] + [os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "dgs_mesh_ops.h")],
    HIPCC_FLAGS, _SIGNATURES, ("dgs_mesh_ops_abi_version", 2), "dgs_mesh_ops_last_error")
LIB_PATH = _LIB.path
_deps, source_hash, build, load = _LIB.deps, _LIB.source_hash, _LIB.build, _LIB.load
_stream = _dgs_build.stream
_f32, _i32, _i64, _f64, _u8 = torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8


def exported_symbols():
    return tuple(_SIGNATURES)


# ---- what every wrapper below is made of ----------------------------------------------------------------------------------------
def _check(rc, what):
    _LIB.check(rc, what)


def _tensor(t, dtype, shape, what):
    """t, after the check that it is a contiguous HIP tensor of `dtype` (one, or a tuple to choose from) and of `shape` (None: any
    shape; an entry None: any size there).  what: "function: argument"."""
    if (t.is_cuda and t.is_contiguous() and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and
            (shape is None or t.shape == shape or (len(t.shape) == len(shape) and all(s is None or s == n for s, n in zip(shape, t.shape))))):
        return t
    kind = " or ".join(str(d).replace("torch.", "") for d in (dtype if type(dtype) is tuple else (dtype,)))
    size = "" if shape is None else " [%s]" % ", ".join("*" if s is None else str(s) for s in shape)
    raise RuntimeError("%s must be a contiguous %s HIP tensor%s" % (what, kind, size))


def _same_device(who, name, dev, *others):
    """Every tensor of others (None: skipped) lives on dev, the device of the argument `name`."""
    if any(t is not None and t.device != dev for t in others):
        raise RuntimeError("%s: every tensor must live on the device of %s" % (who, name))


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _call(dev, entry, *args):
    """The entry point on `dev`: its arguments, then the device's current stream; a negative status raises with the library's message."""
    with torch.cuda.device(dev):
        rc = getattr(load(), entry)(*args, _stream(dev))
    _check(rc, entry)


def _layout(name, n):
    out = (ctypes.c_int * n)()
    _check(getattr(load(), name)(out), name)
    return tuple(int(v) for v in out)


# ---- fusion and marching tetrahedra ---------------------------------------------------------------------------------------------
def tsdf_integrate(dims, origin, voxel, depth, rgb, proj, trunc, depth_trunc, prior_weight, accumulate, tsdf, weight, color):
    """dgs_tsdf_integrate on the volume tensors tsdf / weight [Nx,Ny,Nz] and color [Nx,Ny,Nz,3] (in place)."""
    dev = tsdf.device
    V, H, W = depth.shape
    n = dims[0] * dims[1] * dims[2]
    if rgb.shape != (V, 3, H, W) or proj.shape != (V, 16) or tsdf.numel() != n or weight.numel() != n or color.numel() != 3 * n:
        raise RuntimeError("tsdf_integrate: depth [V,H,W], rgb [V,3,H,W], proj [V,16] and a volume of the given dims are expected")
    for t, what in ((depth, "depth"), (rgb, "rgb"), (proj, "proj"), (tsdf, "tsdf"), (weight, "weight"), (color, "color")):
        _tensor(t, _f32, None, "tsdf_integrate: " + what)
    _same_device("tsdf_integrate", "the volume", dev, depth, rgb, proj, weight, color)
    _call(dev, "dgs_tsdf_integrate", dims[0], dims[1], dims[2], origin[0], origin[1], origin[2], voxel, V, H, W, depth.data_ptr(), rgb.data_ptr(),
          proj.data_ptr(), trunc, depth_trunc, prior_weight, 1 if accumulate else 0, tsdf.data_ptr(), weight.data_ptr(), color.data_ptr())


def marching_tetrahedra(dims, origin, voxel, tsdf, weight, color=None):
    """(vertices [Nv,3] f32, faces [Nf,3] int32, colors [Nv,3] f32 or None) of the volume, in the order of include/dgs_mesh_ops.h.
    PyTorch does the plumbing between the two passes: two prefix sums, the lists of active cells and of vertex-carrying grid
    points, and the one host read of the two totals that sizes the outputs."""
    dev = tsdf.device
    Nx, Ny, Nz = dims
    n = Nx * Ny * Nz
    _tensor(tsdf, _f32, None, "marching_tetrahedra: tsdf"), _tensor(weight, _f32, None, "marching_tetrahedra: weight")
    if color is not None:
        _tensor(color, _f32, None, "marching_tetrahedra: color")
    cell_tris = torch.empty(n, dtype=_i32, device=dev)
    point_verts = torch.empty(n, dtype=_i32, device=dev)
    point_mask = torch.empty(n, dtype=_u8, device=dev)
    _call(dev, "dgs_mt_classify", Nx, Ny, Nz, tsdf.data_ptr(), weight.data_ptr(), cell_tris.data_ptr(), point_verts.data_ptr(), point_mask.data_ptr())
    tri_incl = torch.cumsum(cell_tris, 0, dtype=_i64)
    vert_incl = torch.cumsum(point_verts, 0, dtype=_i64)
    n_tris, n_verts = (int(x) for x in torch.stack((tri_incl[-1], vert_incl[-1])).tolist())
    if n_verts >= 2 ** 31 or n_tris >= 2 ** 31:
        raise RuntimeError("marching_tetrahedra: %d vertices / %d triangles do not fit the int32 face indices" % (n_verts, n_tris))
    vertices = torch.empty((n_verts, 3), dtype=_f32, device=dev)
    faces = torch.empty((n_tris, 3), dtype=_i32, device=dev)
    colors = torch.empty((n_verts, 3), dtype=_f32, device=dev) if color is not None else None
    if n_tris:
        cells = torch.nonzero(cell_tris).reshape(-1)
        points = torch.nonzero(point_mask).reshape(-1)
        _call(dev, "dgs_mt_emit", Nx, Ny, Nz, origin[0], origin[1], origin[2], voxel, tsdf.data_ptr(), None if color is None else color.data_ptr(),
              cells.numel(), cells.data_ptr(), cell_tris.data_ptr(), tri_incl.data_ptr(), points.numel(), points.data_ptr(), point_mask.data_ptr(),
              vert_incl.data_ptr(), vertices.data_ptr(), None if colors is None else colors.data_ptr(), faces.data_ptr())
    return vertices, faces, colors


# ---- the searches, the winding sums and the earth mover's distance ----------------------------------------------------------------------------
def _search(who, entry, layout, chunk, query, qname, ref, rname, cols, expected):
    """nearest and closest_face: device and dtype checks, the chunk default (layout[2]), the `best` buffer, the call and the
    unpacking of the packed minimum."""
    dev = query.device
    _tensor(query, _f32, None, "%s: %s" % (who, qname)), _tensor(ref, _f32, None, "%s: %s" % (who, rname))
    _same_device(who, qname, dev, ref)
    if query.dim() != 2 or query.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != cols:
        raise RuntimeError("%s: %s are expected" % (who, expected))
    chunk = layout[2] if chunk is None else int(chunk)
    best = torch.empty(query.shape[0], dtype=_i64, device=dev)
    _call(dev, entry, query.shape[0], query.data_ptr(), ref.shape[0], ref.data_ptr(), chunk, best.data_ptr())
    # the packed values are below 2^63 (d2 >= 0: sign bit clear), so the signed shift and mask are the unsigned ones
    return (best >> 32).to(_i32).view(_f32), best & 0xFFFFFFFF


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


def winding_layout():
    """(queries per workgroup, triangles per LDS round, default tri_chunk, floats per table row) of dgs_winding_sum."""
    return _layout("dgs_winding_layout", 4)


def winding_sums(points, table, tri_chunk=None):
    """dgs_winding_sum: sums [Nq] int64, the fixed-point winding sums of table [Nf,row] (mesh_metrics.winding_table) at every point
    of points [Nq,3]; W = sums / (2 pi 2^28).  The result does not depend on tri_chunk (default: winding_layout()[2], raised where
    that would make more than 65535 slices)."""
    who, layout, dev = "winding_sums", winding_layout(), points.device
    _tensor(points, _f32, None, who + ": points"), _tensor(table, _f32, None, who + ": table")
    _same_device(who, "points", dev, table)
    if points.dim() != 2 or points.shape[1] != 3 or table.dim() != 2 or table.shape[1] != layout[3]:
        raise RuntimeError("%s: points [Nq,3] and table [Nf,%d] are expected" % (who, layout[3]))
    chunk = max(layout[2], -(-table.shape[0] // 65535)) if tri_chunk is None else int(tri_chunk)
    sums = torch.empty(points.shape[0], dtype=_i64, device=dev)
    _call(dev, "dgs_winding_sum", points.shape[0], points.data_ptr(), table.shape[0], table.data_ptr(), chunk, sums.data_ptr())
    return sums


def emd_layout():
    """(threads per workgroup, objects per LDS round of the dense bidding kernel, largest bidder count of the sparse bidding kernel,
    entries of the result array, fixed bytes of scratch, bytes of scratch per point) of dgs_emd_auction."""
    return _layout("dgs_emd_layout", 6)


EMD_CAP, EMD_OVERFLOW = -3, -4   # statuses of dgs_emd_auction: max_rounds reached; a bid that does not fit 40 bits


def emd_auction(a, b, inv_q, max_rounds, scratch=None):
    """dgs_emd_auction on persons a [n,3] and objects b [n,3] (fp32 HIP tensors) -> (assignment [n] int32, prices [n] int64, primal,
    dual, rounds, max cost).  inv_q: mesh_metrics._emd_quantum.  scratch: an optional uint8 HIP tensor to reuse (emd_layout gives
    its size).  RuntimeError when max_rounds is reached (the message names the phase, eps and the bidders left) or a bid overflows."""
    dev = a.device
    _tensor(a, _f32, None, "emd_auction: a"), _tensor(b, _f32, None, "emd_auction: b")
    _same_device("emd_auction", "a", dev, b)
    if a.dim() != 2 or a.shape[1] != 3 or b.shape != a.shape:
        raise RuntimeError("emd_auction: a [n,3] and b [n,3] are expected")
    n = a.shape[0]
    lay = emd_layout()
    need = lay[4] + n * lay[5]
    if scratch is None:
        scratch = torch.empty(need, dtype=_u8, device=dev)
    elif not (scratch.is_cuda and scratch.device == dev and scratch.dtype == _u8 and scratch.is_contiguous() and scratch.numel() >= need):
        raise RuntimeError("emd_auction: scratch must be a contiguous uint8 tensor of at least %d bytes on the device of a" % need)
    assignment = torch.empty(n, dtype=_i32, device=dev)
    prices = torch.empty(n, dtype=_i64, device=dev)
    result = (ctypes.c_longlong * lay[3])()
    _call(dev, "dgs_emd_auction", n, a.data_ptr(), b.data_ptr(), float(inv_q), int(max_rounds), scratch.data_ptr(), scratch.numel(),
          assignment.data_ptr(), prices.data_ptr(), ctypes.cast(result, ctypes.c_void_p))
    return assignment, prices, int(result[0]), int(result[1]), int(result[2]), int(result[3])


# ---- triangle rasterizer --------------------------------------------------------------------------------------------------------
def raster_layout():
    """(largest box area of the one-lane-per-face path, threads per workgroup, floats per table row, largest C) of dgs_mesh_raster."""
    return _layout("dgs_mesh_raster_layout", 4)


def raster(table, box, H, W, best=None):
    """dgs_mesh_raster for every face of table [Nf,row] (mesh_render.raster_table) with a non-empty box [Nf,4] int32: the faces are
    split by box area into the two paths' lists (a compare + nonzero) and each path is launched once, the first call clearing
    `best`.  -> best [H*W] int64 (the packed minima; -1 = all-ones where nothing was drawn).  A `best` passed in is reused: it is
    fully re-initialised."""
    dev = table.device
    layout = raster_layout()
    _tensor(table, _f32, None, "raster: table")
    if table.dim() != 2 or table.shape[1] != layout[2] or box.shape != (table.shape[0], 4) or box.dtype != _i32 or box.device != dev:
        raise RuntimeError("raster: table [Nf,%d] fp32 and box [Nf,4] int32 on one device are expected" % layout[2])
    if best is None:
        best = torch.empty(H * W, dtype=_i64, device=dev)
    else:
        _tensor(best, _i64, None, "raster: best")
        if best.device != dev or best.numel() != H * W:
            raise RuntimeError("raster: best must be a contiguous int64 tensor of H * W elements on the table's device")
    b = box.long()
    area = (b[:, 1] - b[:, 0] + 1).clamp(min=0) * (b[:, 3] - b[:, 2] + 1).clamp(min=0)
    small = torch.nonzero((area > 0) & (area <= layout[0])).reshape(-1).to(_i32)
    large = torch.nonzero(area > layout[0]).reshape(-1).to(_i32)
    for path, lst, clear in ((0, small, 1), (1, large, 0)):
        _call(dev, "dgs_mesh_raster", table.shape[0], table.data_ptr(), _ptr(lst), lst.numel(), path, H, W, best.data_ptr(), clear)
    return best


def resolve(best, table, faces, H, W, attr=None, background=None):
    """dgs_mesh_resolve -> (face_id [H,W] int32, depth [H,W], bary [H,W,3], image [C,H,W] or None).  faces [Nf,3] int32; attr
    [Nv,C] fp32 with background [C], or None for no image."""
    dev = table.device
    _tensor(table, _f32, None, "resolve: table"), _tensor(faces, _i32, (table.shape[0], 3), "resolve: faces")
    face_id = torch.empty((H, W), dtype=_i32, device=dev)
    depth = torch.empty((H, W), dtype=_f32, device=dev)
    bary = torch.empty((H, W, 3), dtype=_f32, device=dev)
    C, image, nv = 0, None, 0
    if attr is not None:
        _tensor(attr, _f32, None, "resolve: attr"), _tensor(background, _f32, None, "resolve: background")
        nv, C = attr.shape
        if background.numel() != C:
            raise RuntimeError("resolve: background must hold one value per channel")
        image = torch.empty((C, H, W), dtype=_f32, device=dev)
    _call(dev, "dgs_mesh_resolve", H, W, best.data_ptr(), table.shape[0], _ptr(table), _ptr(faces), nv, _ptr(attr), C, _ptr(background),
          face_id.data_ptr(), depth.data_ptr(), bary.data_ptr(), _ptr(image))
    return face_id, depth, bary, image


# ---- connected components -------------------------------------------------------------------------------------------------------
def cc_layout():
    """(threads per workgroup, groups per thread) of dgs_cc_labels: a workgroup takes their product of groups."""
    return _layout("dgs_cc_layout", 2)


def cc_labels(groups, n_nodes):
    """dgs_cc_labels -> label [n_nodes] int32 on the device of groups [G,k] (int32, contiguous, k in {2, 3}): the smallest node id of
    every node's component.  An id outside [0, n_nodes) is a ValueError (one aminmax, read on the host)."""
    dev = groups.device
    _tensor(groups, _i32, None, "cc_labels: groups")
    if groups.dim() != 2 or groups.shape[1] not in (2, 3):
        raise RuntimeError("cc_labels: groups [G,2] or [G,3] are expected")
    n_nodes = int(n_nodes)
    if n_nodes < 0 or n_nodes >= 2 ** 31:
        raise ValueError("cc_labels: n_nodes must be in [0, 2^31)")
    if groups.shape[0]:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(groups)).tolist())
        if lo < 0 or hi >= n_nodes:
            raise ValueError("cc_labels: node ids in [%d, %d] but n_nodes is %d" % (lo, hi, n_nodes))
    label = torch.empty(n_nodes, dtype=_i32, device=dev)
    _call(dev, "dgs_cc_labels", n_nodes, _ptr(groups), groups.shape[0], groups.shape[1], _ptr(label))
    return label


# ---- quadric vertex clustering --------------------------------------------------------------------------------------------------
def simplify_layout():
    """(threads per workgroup, items per thread, Q, W_MAX, exponent of lambda) of dgs_simplify_accumulate / dgs_simplify_solve."""
    return _layout("dgs_simplify_layout", 5)


def simplify_accumulate(vertices, colors, faces, cluster, centres, cell):
    """dgs_simplify_accumulate -> rows [C,16] int64 on the device of vertices [V,3]: colors [V,3] or None, faces [F,3] int32, cluster
    [V] int32 (the cell of every vertex), centres [C,3], cell a float."""
    dev = vertices.device
    V, F, C = vertices.shape[0], faces.shape[0], centres.shape[0]
    _tensor(vertices, _f32, (V, 3), "simplify_accumulate: vertices"), _tensor(centres, _f32, (C, 3), "simplify_accumulate: centres")
    _tensor(faces, _i32, (F, 3), "simplify_accumulate: faces"), _tensor(cluster, _i32, (V,), "simplify_accumulate: cluster")
    if colors is not None:
        _tensor(colors, _f32, (V, 3), "simplify_accumulate: colors")
    _same_device("simplify_accumulate", "vertices", dev, colors, faces, cluster, centres)
    rows = torch.empty((C, 16), dtype=_i64, device=dev)
    _call(dev, "dgs_simplify_accumulate", V, _ptr(vertices), _ptr(colors), F, _ptr(faces), _ptr(cluster), C, _ptr(centres), float(cell), _ptr(rows))
    return rows


def simplify_solve(rows, centres, cell, quadric=True, with_colors=False):
    """dgs_simplify_solve -> (vertices [C,3] f32, colors [C,3] f32 or None) from the rows of simplify_accumulate."""
    dev = rows.device
    C = centres.shape[0]
    _tensor(rows, _i64, (C, 16), "simplify_solve: rows"), _tensor(centres, _f32, (C, 3), "simplify_solve: centres")
    _same_device("simplify_solve", "rows", dev, centres)
    vertices = torch.empty((C, 3), dtype=_f32, device=dev)
    colors = torch.empty((C, 3), dtype=_f32, device=dev) if with_colors else None
    _call(dev, "dgs_simplify_solve", C, _ptr(rows), _ptr(centres), float(cell), 1 if quadric else 0, _ptr(vertices), _ptr(colors))
    return vertices, colors


# ---- Laplacian / Taubin smoothing -----------------------------------------------------------------------------------------------
def smooth_layout():
    """(threads per workgroup, vertices per workgroup, largest C, largest n_steps of one call) of dgs_smooth_steps."""
    return _layout("dgs_smooth_layout", 4)


def smooth_steps(offsets, neighbours, x, mode, factors, pinned=None, tmp=None):
    """dgs_smooth_steps, in place on x [V,C] (fp32, contiguous, C in [1, 8]) -> x: one step per entry of factors (Python numbers,
    taken as fp32) of mode 0 (laplacian) or 1 (simple) over the rows offsets [V+1] int64 / neighbours [E] int32
    (mesh_smooth.vertex_adjacency).  pinned: [V] uint8 or bool, or None; tmp: an optional buffer like x to reuse.  At most
    smooth_layout()[3] steps a call."""
    dev = x.device
    _tensor(x, _f32, (None, None), "smooth_steps: x")
    V, C = x.shape
    _tensor(offsets, _i64, (V + 1,), "smooth_steps: offsets"), _tensor(neighbours, _i32, (None,), "smooth_steps: neighbours")
    if pinned is not None:
        _tensor(pinned, (_u8, torch.bool), (V,), "smooth_steps: pinned")
    if tmp is None:
        tmp = torch.empty_like(x)
    elif _tensor(tmp, _f32, (V, C), "smooth_steps: tmp").data_ptr() == x.data_ptr():
        raise RuntimeError("smooth_steps: tmp must be another tensor than x")
    _same_device("smooth_steps", "x", dev, offsets, neighbours, pinned, tmp)
    host = (ctypes.c_float * max(len(factors), 1))(*[float(s) for s in factors])
    _call(dev, "dgs_smooth_steps", V, _ptr(offsets), _ptr(neighbours), neighbours.numel(), C, int(mode), ctypes.cast(host, ctypes.c_void_p), len(factors),
          _ptr(pinned), _ptr(x), _ptr(tmp))
    return x


# ---- quadric edge collapse in rounds --------------------------------------------------------------------------------------------
def decimate_layout():
    """(threads per workgroup, items per thread, Q_MAX, Q_BUDGET, W_MAX, exponent of lambda, least valence of an interior opposite
    vertex, fixed-point bits of mean_len) of the dgs_decimate_* calls."""
    return _layout("dgs_decimate_layout", 8)


def decimate_quadrics(pos, faces, mean_len, q_bits):
    """dgs_decimate_quadrics -> rows [V,10] int64 on the device of pos [V,3] (the frame) for faces [F,3] int32."""
    dev = pos.device
    V, F = pos.shape[0], faces.shape[0]
    _tensor(pos, _f32, (V, 3), "decimate_quadrics: pos"), _tensor(faces, _i32, (F, 3), "decimate_quadrics: faces")
    _same_device("decimate_quadrics", "pos", dev, faces)
    rows = torch.empty((V, 10), dtype=_i64, device=dev)
    _call(dev, "dgs_decimate_quadrics", V, _ptr(pos), F, _ptr(faces), float(mean_len), int(q_bits), _ptr(rows))
    return rows


def decimate_edges(pos, rows, faces, tab, q_bits, max_cost):
    """dgs_decimate_edges -> (cost [E] fp32, place [E,3] fp32, valid [E] bool) for the tables of mesh_decimate.round_tables."""
    dev = pos.device
    V, F, E = pos.shape[0], faces.shape[0], tab["edges"].shape[1]
    adj, vf = tab["adj"], tab["vf"]
    _tensor(pos, _f32, (V, 3), "decimate_edges: pos"), _tensor(rows, _i64, (V, 10), "decimate_edges: rows")
    _tensor(faces, _i32, (F, 3), "decimate_edges: faces"), _tensor(tab["edges"], _i32, (5, E), "decimate_edges: edges")
    _tensor(tab["flags"], _u8, (V,), "decimate_edges: flags")
    _tensor(tab["adj_offsets"], _i64, (V + 1,), "decimate_edges: adj_offsets"), _tensor(tab["vf_offsets"], _i64, (V + 1,), "decimate_edges: vf_offsets")
    _tensor(adj, _i32, (None,), "decimate_edges: adj"), _tensor(vf, _i32, (None,), "decimate_edges: vf")
    _same_device("decimate_edges", "pos", dev, rows, faces, tab["edges"], tab["flags"], tab["adj_offsets"], adj, tab["vf_offsets"], vf)
    cost = torch.empty(E, dtype=_f32, device=dev)
    place = torch.empty((E, 3), dtype=_f32, device=dev)
    valid = torch.empty(E, dtype=_u8, device=dev)
    _call(dev, "dgs_decimate_edges", V, _ptr(pos), _ptr(rows), _ptr(tab["flags"]), F, _ptr(faces), E, _ptr(tab["edges"]), _ptr(tab["adj_offsets"]),
          _ptr(adj), adj.numel(), _ptr(tab["vf_offsets"]), _ptr(vf), vf.numel(), int(q_bits), float(max_cost), _ptr(cost), _ptr(place), _ptr(valid))
    return cost, place, valid.bool()


def decimate_select(n_vertices, edges, cost, compete):
    """dgs_decimate_select -> (m1 [V] int64, m2 [V] int64, selected [E] bool) for edges [5,E] int32, cost [E] fp32, compete [E] bool."""
    dev = cost.device
    V, E = int(n_vertices), edges.shape[1]
    _tensor(edges, _i32, (5, E), "decimate_select: edges"), _tensor(cost, _f32, (E,), "decimate_select: cost")
    _tensor(compete, torch.bool, (E,), "decimate_select: compete")
    _same_device("decimate_select", "cost", dev, edges, compete)
    m1 = torch.empty(V, dtype=_i64, device=dev)
    m2 = torch.empty(V, dtype=_i64, device=dev)
    selected = torch.empty(E, dtype=_u8, device=dev)
    _call(dev, "dgs_decimate_select", V, E, _ptr(edges), _ptr(cost), _ptr(compete), _ptr(m1), _ptr(m2), _ptr(selected))
    return m1, m2, selected.bool()


def decimate_apply(pos, rows, colors, moved, faces, tab, place, sel):
    """dgs_decimate_apply, in place on pos [V,3], rows [V,10], colors [V,3] or None, moved [V] bool and faces [F,3] int32 (re-indexed)
    -> (vmap [V] int32, faces, keep [F] bool) for the selected edge ids sel [S] int32."""
    dev = pos.device
    V, F, E, S = pos.shape[0], faces.shape[0], tab["edges"].shape[1], sel.shape[0]
    _tensor(pos, _f32, (V, 3), "decimate_apply: pos"), _tensor(rows, _i64, (V, 10), "decimate_apply: rows")
    _tensor(moved, torch.bool, (V,), "decimate_apply: moved"), _tensor(faces, _i32, (F, 3), "decimate_apply: faces")
    _tensor(tab["edges"], _i32, (5, E), "decimate_apply: edges"), _tensor(tab["flags"], _u8, (V,), "decimate_apply: flags")
    _tensor(place, _f32, (E, 3), "decimate_apply: place"), _tensor(sel, _i32, (S,), "decimate_apply: sel")
    if colors is not None:
        _tensor(colors, _f32, (V, 3), "decimate_apply: colors")
    _same_device("decimate_apply", "pos", dev, rows, colors, moved, faces, tab["edges"], tab["flags"], place, sel)
    vmap = torch.empty(V, dtype=_i32, device=dev)
    keep = torch.empty(F, dtype=_u8, device=dev)
    _call(dev, "dgs_decimate_apply", V, _ptr(pos), _ptr(rows), _ptr(colors), _ptr(tab["flags"]), _ptr(moved), _ptr(vmap), E, _ptr(tab["edges"]),
          _ptr(place), S, _ptr(sel), F, _ptr(faces), _ptr(keep))
    return vmap, faces, keep.bool()


# ---- hole filling ---------------------------------------------------------------------------------------------------------------
def fill_layout():
    """(threads per workgroup, items per thread, fixed-point bits of the position, Newell and colour sums, columns of a ring row, taps
    of the smoothed rim, largest n_rounds) of the dgs_fill_* calls."""
    return _layout("dgs_fill_layout", 8)


def fill_rank(succ, leader, n_rounds, buf_a=None, buf_b=None, rank=None):
    """dgs_fill_rank -> rank [n] int32 (the position in hole order; -1 where leader is -1) for succ, leader [n] int32.  buf_a, buf_b
    [n] int64 and rank may be passed in to be reused; after the call the packed entries lie in buf_a (n_rounds even) or buf_b."""
    dev = succ.device
    n = succ.shape[0]
    _tensor(succ, _i32, (n,), "fill_rank: succ"), _tensor(leader, _i32, (n,), "fill_rank: leader")
    buf_a = torch.empty(n, dtype=_i64, device=dev) if buf_a is None else _tensor(buf_a, _i64, (n,), "fill_rank: buf_a")
    buf_b = torch.empty(n, dtype=_i64, device=dev) if buf_b is None else _tensor(buf_b, _i64, (n,), "fill_rank: buf_b")
    rank = torch.empty(n, dtype=_i32, device=dev) if rank is None else _tensor(rank, _i32, (n,), "fill_rank: rank")
    _same_device("fill_rank", "succ", dev, leader, buf_a, buf_b, rank)
    _call(dev, "dgs_fill_rank", n, _ptr(succ), _ptr(leader), int(n_rounds), _ptr(buf_a), _ptr(buf_b), _ptr(rank))
    return rank


def fill_rim(vertices, colors, loop_vertices, rim_loop, loop_offsets, centre, scale):
    """dgs_fill_rim -> (S [B,3] fp64, SC [B,3] fp64 or None, rows [L,16] int64) for the rims loop_vertices / rim_loop [B] int32,
    loop_offsets [L+1] int64 of vertices [V,3] (colors [V,3] or None); centre: three Python numbers, scale: a power of two."""
    dev = vertices.device
    V, B, L = vertices.shape[0], loop_vertices.shape[0], loop_offsets.shape[0] - 1
    _tensor(vertices, _f32, (V, 3), "fill_rim: vertices"), _tensor(loop_vertices, _i32, (B,), "fill_rim: loop_vertices")
    _tensor(rim_loop, _i32, (B,), "fill_rim: rim_loop"), _tensor(loop_offsets, _i64, (L + 1,), "fill_rim: loop_offsets")
    if colors is not None:
        _tensor(colors, _f32, (V, 3), "fill_rim: colors")
    _same_device("fill_rim", "vertices", dev, colors, loop_vertices, rim_loop, loop_offsets)
    S = torch.empty((B, 3), dtype=_f64, device=dev)
    SC = torch.empty((B, 3), dtype=_f64, device=dev) if colors is not None else None
    rows = torch.empty((L, 16), dtype=_i64, device=dev)
    _call(dev, "dgs_fill_rim", V, _ptr(vertices), _ptr(colors), B, _ptr(loop_vertices), _ptr(rim_loop), L, _ptr(loop_offsets), float(centre[0]),
          float(centre[1]), float(centre[2]), float(scale), _ptr(S), _ptr(SC), _ptr(rows))
    return S, SC, rows


def fill_emit(n_old, lay, loop_vertices, loop_offsets, rows, S, SC, centre, scale, vertices_out, colors_out, faces_out):
    """dgs_fill_emit for the layout lay (mesh_fill.ring_layout: "rings" [NR,10], "vert_ring" [n_new], "face_ring" [n_new_faces], all
    int32): writes rows n_old .. n_old + n_new of vertices_out [n_old + n_new,3] fp32 (rows 0 .. n_old hold the input vertices) and of
    colors_out (or None, with SC None) and all of faces_out [n_new_faces,3] int32."""
    dev = vertices_out.device
    rings, vert_ring, face_ring = lay["rings"], lay["vert_ring"], lay["face_ring"]
    NR, NV, NF, B, L = rings.shape[0], vert_ring.shape[0], face_ring.shape[0], loop_vertices.shape[0], loop_offsets.shape[0] - 1
    n_old = int(n_old)
    _tensor(rings, _i32, (NR, fill_layout()[5]), "fill_emit: rings"), _tensor(vert_ring, _i32, (NV,), "fill_emit: vert_ring")
    _tensor(face_ring, _i32, (NF,), "fill_emit: face_ring"), _tensor(loop_vertices, _i32, (B,), "fill_emit: loop_vertices")
    _tensor(loop_offsets, _i64, (L + 1,), "fill_emit: loop_offsets"), _tensor(rows, _i64, (L, 16), "fill_emit: rows")
    _tensor(S, _f64, (B, 3), "fill_emit: S"), _tensor(vertices_out, _f32, (n_old + NV, 3), "fill_emit: vertices_out")
    _tensor(faces_out, _i32, (NF, 3), "fill_emit: faces_out")
    if (SC is None) != (colors_out is None):
        raise RuntimeError("fill_emit: SC and colors_out come together")
    if SC is not None:
        _tensor(SC, _f64, (B, 3), "fill_emit: SC"), _tensor(colors_out, _f32, (n_old + NV, 3), "fill_emit: colors_out")
    _same_device("fill_emit", "vertices_out", dev, rings, vert_ring, face_ring, loop_vertices, loop_offsets, rows, S, SC, colors_out, faces_out)
    _call(dev, "dgs_fill_emit", n_old, NV, _ptr(vert_ring), NF, _ptr(face_ring), NR, _ptr(rings), L, _ptr(loop_offsets), B, _ptr(loop_vertices),
          _ptr(rows), _ptr(S), _ptr(SC), float(centre[0]), float(centre[1]), float(centre[2]), float(scale), _ptr(vertices_out), _ptr(colors_out),
          _ptr(faces_out))
    return vertices_out, colors_out, faces_out
