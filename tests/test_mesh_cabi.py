"""libdgs_mesh_ops.so builds, loads and exports every function include/dgs_mesh_ops.h declares (no compute: runs without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER, LIB = "dgs_mesh_ops.h", "libdgs_mesh_ops.so"


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    return sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", text)) - set(re.findall(r"\(\s*\*\s*(dgs_[a-z0-9_]+)\s*\)", text)))


def test_mesh_library_exports_every_declared_symbol():
    from dgs_amd import _mesh_ops
    path = _mesh_ops.build()   # rebuilds only when the hash of the sources + flags differs from the recorded one
    assert os.path.basename(path) == LIB
    names = declared_functions(HEADER)
    assert len(names) >= 5, names
    handle = ctypes.CDLL(path)
    missing = [n for n in names if not hasattr(handle, n)]
    assert not missing, "%s does not export %s" % (LIB, missing)
    handle.dgs_mesh_ops_abi_version.restype = ctypes.c_int
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert handle.dgs_mesh_ops_abi_version() == int(re.search(r"#define DGS_MESH_OPS_ABI_VERSION (\d+)", text).group(1))


def test_mesh_binding_list_matches_header():
    from dgs_amd import _mesh_ops
    assert sorted(_mesh_ops.exported_symbols()) == declared_functions(HEADER)
    lib = _mesh_ops.load()   # refuses a binary built from other sources than the tree's
    for name in _mesh_ops.exported_symbols():
        getattr(lib, name)


def test_mesh_library_is_separate_from_the_training_libraries():
    """The new kernels live in a third library: the inputs of the two existing ones do not name its sources."""
    from dgs_amd import _mesh_ops, _ops
    from diff_surfel_rasterization import _C
    mine = {os.path.basename(p) for p in _mesh_ops._deps()}
    assert mine == {"mesh_ops.hip", "mesh_common.h", "mesh_fusion_kernels.h", "mesh_search_kernels.h", "mesh_raster_kernels.h",
                    "mesh_cc_kernels.h", "mesh_simplify_kernels.h", "mesh_smooth_kernels.h", "mesh_decimate_kernels.h",
                    "mesh_fill_kernels.h", HEADER}
    assert not mine & {os.path.basename(p) for p in _ops._deps() + _C._deps()}
    assert "-ffp-contract=off" in _mesh_ops.HIPCC_FLAGS and set(_ops.HIPCC_FLAGS) <= set(_mesh_ops.HIPCC_FLAGS)


def test_arguments_are_validated_before_any_launch():
    """Bad sizes are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    assert lib.dgs_tsdf_integrate(4, 4, 4, 0.0, 0.0, 0.0, 0.1, 1, 1, 8, None, None, None, 0.5, 6.0, 0.0, 0, None, None, None, None) < 0
    assert b"2 x 2" in lib.dgs_mesh_ops_last_error()
    assert lib.dgs_mt_classify(1, 4, 4, None, None, None, None, None, None) < 0
    assert b">= 2" in lib.dgs_mesh_ops_last_error()
