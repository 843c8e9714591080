"""The two C-ABI libraries load and export every function their headers declare (no compute: runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-2dgs_amd", "csrc")
CASES = [("dgs_surfel_rasterizer.h", "libdgs_surfel_rasterizer.so"), ("dgs_train_ops.h", "libdgs_train_ops.so")]


def declared_functions(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    # prototypes: "<type> name(args);" -- skip typedef'd function pointers "(*name)"
    return sorted(set(re.findall(r"\b(dgs_[a-z0-9_]+)\s*\(", text)) - set(re.findall(r"\(\s*\*\s*(dgs_[a-z0-9_]+)\s*\)", text)))


@pytest.mark.parametrize("header,lib", CASES)
def test_library_exports_every_declared_symbol(header, lib):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dynamic-2dgs_amd"))
    from dgs_amd import _ops
    from diff_surfel_rasterization import _C
    path = (_C if "rasterizer" in lib else _ops).build()  # rebuilds only when a source is newer than the library
    assert os.path.basename(path) == lib
    names = declared_functions(header)
    assert len(names) >= 5, names
    handle = ctypes.CDLL(path)
    missing = [n for n in names if not hasattr(handle, n)]
    assert not missing, "%s does not export %s" % (lib, missing)


def test_python_bindings_list_matches_headers():
    """The symbol lists __graft_entry__.build() checks are the headers' declarations."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dynamic-2dgs_amd"))
    from dgs_amd import _ops
    from diff_surfel_rasterization import _C
    assert sorted(_ops.exported_symbols()) == declared_functions("dgs_train_ops.h")
    assert set(declared_functions("dgs_surfel_rasterizer.h")) <= set(_C.exported_symbols()) | {"dgs_alloc_fn"}


def _ops_module():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dynamic-2dgs_amd"))
    from dgs_amd import _ops
    return _ops


def _binding_module(name):
    import importlib
    _ops_module()   # (puts the package directory on sys.path)
    return importlib.import_module(name)


@pytest.mark.parametrize("module,source,header", [("dgs_amd._ops", "train_ops.hip", "dgs_train_ops.h"),
                                                  ("diff_surfel_rasterization._C", "surfel_rasterizer.hip", "dgs_surfel_rasterizer.h"),
                                                  ("dgs_amd._mesh_ops", "mesh_ops.hip", "dgs_mesh_ops.h")],
                         ids=["train_ops", "rasterizer", "mesh_ops"])
def test_library_deps_are_the_include_closure(module, source, header):
    """A binding module's _deps() (what the stale-binary hash covers) is exactly the set of files its .hip file reaches through
    relative #include "..." lines, plus its public header: a header missing from the list would hide kernel edits from the hash,
    a listed header that is no longer included fails too."""
    todo, seen = [os.path.join(CSRC, source)], set()
    while todo:
        path = os.path.normpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', open(path).read(), flags=re.M):
            todo.append(os.path.join(os.path.dirname(path), inc))
    want = seen | {os.path.join(ROOT, "include", header)}
    deps = [os.path.normpath(p) for p in _binding_module(module)._deps()]
    assert len(deps) == len(set(deps))
    assert set(deps) == want, (sorted(set(deps) - want), sorted(want - set(deps)))


def _prototypes(header):
    """{name: (return type, number of parameters)} of the header's dgs_* prototypes."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s\*]+)(dgs_[a-z0-9_]+)\s*\(", text):
        depth, commas, i = 1, 0, m.end()
        while depth:
            c = text[i]
            depth += (c == "(") - (c == ")")
            commas += c == "," and depth == 1
            i += 1
        args = text[m.end():i - 1].strip()
        assert text[i:].lstrip().startswith(";"), m.group(2)
        out[m.group(2)] = (" ".join(m.group(1).replace("*", " * ").split()), 0 if args in ("", "void") else commas + 1)
    return out


@pytest.mark.parametrize("module,header", [("dgs_amd._ops", "dgs_train_ops.h"), ("diff_surfel_rasterization._C", "dgs_surfel_rasterizer.h"),
                                           ("dgs_amd._mesh_ops", "dgs_mesh_ops.h")], ids=["train_ops", "rasterizer", "mesh_ops"])
def test_binding_table_matches_header_arity(module, header):
    """Every prototype of a library's header has a table entry with as many argtypes as the prototype has parameters and the restype
    of its return type, and the table has no other entry: ctypes passes a call of the wrong arity without complaint."""
    table = _binding_module(module)._SIGNATURES
    protos = _prototypes(header)
    assert sorted(protos) == declared_functions(header)
    assert sorted(table) == declared_functions(header)
    restypes = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p, "void": None, "void *": ctypes.c_void_p,
                "dgs_context *": ctypes.c_void_p}   # (an opaque handle)
    wrong = []
    for name, (ret, nargs) in sorted(protos.items()):
        restype, argtypes = table[name]
        if restype is not restypes[ret] or len(argtypes) != nargs:
            wrong.append((name, ret, nargs, restype, len(argtypes)))
    assert not wrong, wrong
