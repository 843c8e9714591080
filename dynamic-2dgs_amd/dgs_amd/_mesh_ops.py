"""ctypes binding of libdgs_mesh_ops.so (include/dgs_mesh_ops.h): TSDF fusion, marching tetrahedra, the all-pairs nearest-neighbour
and closest-triangle searches, the z-buffer triangle rasterizer and the connected components for gfx950, used by dgs_amd.mesh,
dgs_amd.mesh_metrics, dgs_amd.mesh_render and dgs_amd.mesh_clean when the data lives on a HIP device.  CPU tensors use the PyTorch /
NumPy statements in those modules."""
import ctypes
import os

import torch

from . import _ops

_CSRC = _ops._CSRC
LIB_PATH = os.path.join(_CSRC, "libdgs_mesh_ops.so")
# -ffp-contract=off: the fuser's accept / reject decisions sit on thresholds; with every operation rounded on its own the kernel
# and the PyTorch statement of the same arithmetic take the same side of every one of them
HIPCC_FLAGS = list(_ops.HIPCC_FLAGS) + ["-ffp-contract=off"]
_lib = None
_EXPORTS = ("dgs_mesh_ops_abi_version", "dgs_mesh_ops_last_error", "dgs_tsdf_integrate", "dgs_mt_classify", "dgs_mt_emit",
            "dgs_nn_search", "dgs_nn_layout", "dgs_tri_search", "dgs_tri_layout", "dgs_mesh_raster", "dgs_mesh_resolve",
            "dgs_mesh_raster_layout", "dgs_cc_labels", "dgs_cc_layout")


def _deps():
    hdr = os.path.join(os.path.dirname(os.path.dirname(_CSRC)), "include", "dgs_mesh_ops.h")
    return [os.path.join(_CSRC, "mesh_ops.hip"), hdr]


def source_hash():
    import _dgs_build
    return _dgs_build.source_hash(_deps(), HIPCC_FLAGS)


def build(force=False, verbose=False):
    """hipcc, in-tree; rebuilt whenever the hash of sources + flags differs from the one recorded with the binary."""
    import _dgs_build
    cmd = ["hipcc"] + HIPCC_FLAGS + [os.path.join(_CSRC, "mesh_ops.hip"), "-o", LIB_PATH]
    return _dgs_build.build(LIB_PATH, cmd, _deps(), HIPCC_FLAGS, _CSRC, force=force, verbose=verbose)[0]


def exported_symbols():
    return _EXPORTS


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not found; build it with __graft_entry__.build()" % LIB_PATH)
        from diff_surfel_rasterization._C import _refuse_stale
        _refuse_stale(LIB_PATH, source_hash, build)   # never run a binary built from other sources than the tree's
        lib = ctypes.CDLL(LIB_PATH)
        vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
        lib.dgs_mesh_ops_abi_version.restype = ci
        lib.dgs_mesh_ops_last_error.restype = ctypes.c_char_p
        lib.dgs_tsdf_integrate.restype = ci
        lib.dgs_tsdf_integrate.argtypes = [ci, ci, ci, cf, cf, cf, cf, ci, ci, ci, vp, vp, vp, cf, cf, cf, ci, vp, vp, vp, vp]
        lib.dgs_mt_classify.restype = ci
        lib.dgs_mt_classify.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp]
        lib.dgs_mt_emit.restype = ci
        lib.dgs_mt_emit.argtypes = [ci, ci, ci, cf, cf, cf, cf, vp, vp, ll, vp, vp, vp, ll, vp, vp, vp, vp, vp, vp, vp]
        lib.dgs_nn_search.restype = ci
        lib.dgs_nn_search.argtypes = [ll, vp, ll, vp, ll, vp, vp]
        lib.dgs_nn_layout.restype = ci
        lib.dgs_nn_layout.argtypes = [ctypes.POINTER(ci)]
        lib.dgs_tri_search.restype = ci
        lib.dgs_tri_search.argtypes = [ll, vp, ll, vp, ll, vp, vp]
        lib.dgs_tri_layout.restype = ci
        lib.dgs_tri_layout.argtypes = [ctypes.POINTER(ci)]
        lib.dgs_mesh_raster.restype = ci
        lib.dgs_mesh_raster.argtypes = [ll, vp, vp, ll, ci, ci, ci, vp, ci, vp]
        lib.dgs_mesh_resolve.restype = ci
        lib.dgs_mesh_resolve.argtypes = [ci, ci, vp, ll, vp, vp, ll, vp, ci, vp, vp, vp, vp, vp, vp]
        lib.dgs_mesh_raster_layout.restype = ci
        lib.dgs_mesh_raster_layout.argtypes = [ctypes.POINTER(ci)]
        lib.dgs_cc_labels.restype = ci
        lib.dgs_cc_labels.argtypes = [ll, vp, ll, ci, vp, vp]
        lib.dgs_cc_layout.restype = ci
        lib.dgs_cc_layout.argtypes = [ctypes.POINTER(ci)]
        if lib.dgs_mesh_ops_abi_version() != 2:
            raise RuntimeError("libdgs_mesh_ops.so ABI version mismatch (want 2, library says %d): rebuild it" % lib.dgs_mesh_ops_abi_version())
        _lib = lib
    return _lib


def _check(lib, rc, what):
    if rc < 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.dgs_mesh_ops_last_error().decode()))


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


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


def nn_layout():
    """(queries per workgroup, reference points per LDS round, default ref_chunk) of dgs_nn_search."""
    lib = load()
    out = (ctypes.c_int * 3)()
    _check(lib, lib.dgs_nn_layout(out), "dgs_nn_layout")
    return tuple(int(v) for v in out)


def nearest(query, ref, ref_chunk=None):
    """dgs_nn_search: (d2 [Nq] f32, idx [Nq] int64) of the nearest point of ref [Nr,3] for every point of query [Nq,3]; equal
    distances go to the lowest index.  The result does not depend on ref_chunk (default: nn_layout()[2])."""
    lib = load()
    dev = query.device
    _f32(query, "query"), _f32(ref, "ref")
    if ref.device != dev:
        raise RuntimeError("nearest: ref lives on another device than query")
    if query.dim() != 2 or query.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != 3:
        raise RuntimeError("nearest: query [Nq,3] and ref [Nr,3] are expected")
    chunk = nn_layout()[2] if ref_chunk is None else int(ref_chunk)
    best = torch.empty(query.shape[0], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_nn_search(query.shape[0], query.data_ptr(), ref.shape[0], ref.data_ptr(), chunk, best.data_ptr(), _stream(dev))
    _check(lib, rc, "dgs_nn_search")
    # the packed values are below 2^63 (d2 >= 0: sign bit clear), so the signed shift and mask are the unsigned ones
    return (best >> 32).to(torch.int32).view(torch.float32), best & 0xFFFFFFFF


def tri_layout():
    """(queries per workgroup, triangles per LDS round, default tri_chunk, floats per table row) of dgs_tri_search."""
    lib = load()
    out = (ctypes.c_int * 4)()
    _check(lib, lib.dgs_tri_layout(out), "dgs_tri_layout")
    return tuple(int(v) for v in out)


def closest_face(points, table, tri_chunk=None):
    """dgs_tri_search: (d2 [Nq] f32, face [Nq] int64) of the closest triangle of table [Nf,row] (mesh_metrics.triangle_table) for
    every point of points [Nq,3]; equal distances go to the lowest face.  The result does not depend on tri_chunk (default:
    tri_layout()[2])."""
    lib = load()
    dev = points.device
    _f32(points, "points"), _f32(table, "table")
    if table.device != dev:
        raise RuntimeError("closest_face: table lives on another device than points")
    layout = tri_layout()
    if points.dim() != 2 or points.shape[1] != 3 or table.dim() != 2 or table.shape[1] != layout[3]:
        raise RuntimeError("closest_face: points [Nq,3] and table [Nf,%d] are expected" % layout[3])
    chunk = layout[2] if tri_chunk is None else int(tri_chunk)
    best = torch.empty(points.shape[0], dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.dgs_tri_search(points.shape[0], points.data_ptr(), table.shape[0], table.data_ptr(), chunk, best.data_ptr(), _stream(dev))
    _check(lib, rc, "dgs_tri_search")
    # the packed values are below 2^63 (d2 >= 0: sign bit clear), so the signed shift and mask are the unsigned ones
    return (best >> 32).to(torch.int32).view(torch.float32), best & 0xFFFFFFFF


def raster_layout():
    """(largest box area of the one-lane-per-face path, threads per workgroup, floats per table row, largest C) of dgs_mesh_raster."""
    lib = load()
    out = (ctypes.c_int * 4)()
    _check(lib, lib.dgs_mesh_raster_layout(out), "dgs_mesh_raster_layout")
    return tuple(int(v) for v in out)


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
    lib = load()
    out = (ctypes.c_int * 2)()
    _check(lib, lib.dgs_cc_layout(out), "dgs_cc_layout")
    return tuple(int(v) for v in out)


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
