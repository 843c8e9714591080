"""_dgs_build.NativeLibrary, the one build-and-load path of the three native libraries, on a tiny C library built with g++ (no hipcc,
no device): what load() compiles, refuses and declares.  The compiler is a wrapper that logs every run, as in test_build_lock.py."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dynamic-2dgs_amd"))

SOURCE = """#include "tiny.h"
extern "C" int tiny_abi_version(void) { return TINY_ABI; }
extern "C" const char* tiny_last_error(void) { return "tiny went wrong"; }
extern "C" int tiny_add(int a, int b) { return a + b + TINY_BIAS; }
"""
LOGGING_CC = "import subprocess, sys\nopen(sys.argv[1], 'a').write('compile\\n')\nsys.exit(subprocess.call(['g++'] + sys.argv[2:]))\n"
FLAGS = ["-O1", "-shared", "-fPIC"]
SIGNATURES = {"tiny_abi_version": (ctypes.c_int, []), "tiny_last_error": (ctypes.c_char_p, []),
              "tiny_add": (ctypes.c_int, [ctypes.c_int, ctypes.c_int])}


class Tiny:
    """A source tree of two inputs (tiny.cpp, tiny.h) in `root` and the description of its library."""

    def __init__(self, root, abi=2, bias=0, env=None, compiler=None):
        import _dgs_build
        self.root, self.log = str(root), os.path.join(str(root), "compiles.log")
        with open(os.path.join(self.root, "tiny.cpp"), "w") as f:
            f.write(SOURCE)
        with open(os.path.join(self.root, "cc.py"), "w") as f:
            f.write(LOGGING_CC)
        self.header(abi, bias)
        src, hdr = os.path.join(self.root, "tiny.cpp"), os.path.join(self.root, "tiny.h")
        self.lib = _dgs_build.NativeLibrary(os.path.join(self.root, "libtiny.so"), src, [src, hdr], FLAGS, SIGNATURES, ("tiny_abi_version", 2),
                                            "tiny_last_error", env=env,
                                            compiler=compiler or [sys.executable, os.path.join(self.root, "cc.py"), self.log])

    def header(self, abi, bias):
        with open(os.path.join(self.root, "tiny.h"), "w") as f:
            f.write("#define TINY_ABI %d\n#define TINY_BIAS %d\n" % (abi, bias))

    def compiles(self):
        return len(open(self.log).read().split()) if os.path.exists(self.log) else 0


def test_current_library_is_loaded_without_a_compile(tmp_path):
    import _dgs_build
    t = Tiny(tmp_path)
    assert t.lib.build() == t.lib.path and t.compiles() == 1
    assert _dgs_build.recorded_hash(t.lib.path) == t.lib.source_hash() == _dgs_build.source_hash(t.lib.deps(), FLAGS)
    lib = t.lib.load()
    assert t.compiles() == 1
    assert lib.tiny_add(2, 3) == 5
    assert t.lib.load() is lib and t.compiles() == 1          # cached


def test_edited_input_is_rebuilt_once(tmp_path):
    t = Tiny(tmp_path)
    t.lib.build()
    t.header(abi=2, bias=100)                                 # the header, not the main source: every input counts
    assert t.lib.load().tiny_add(2, 3) == 105
    assert t.compiles() == 2
    import _dgs_build
    assert _dgs_build.recorded_hash(t.lib.path) == t.lib.source_hash()


def test_stale_library_that_cannot_be_rebuilt_is_refused(tmp_path):
    import _dgs_build
    t = Tiny(tmp_path)
    t.lib.build()
    have = t.lib.source_hash()
    t.header(abi=2, bias=100)
    want = t.lib.source_hash()
    assert have != want
    broken = _dgs_build.NativeLibrary(t.lib.default_path, t.lib.main, t.lib.inputs, FLAGS, SIGNATURES, ("tiny_abi_version", 2), "tiny_last_error",
                                      compiler=[sys.executable, "-c", "import sys; sys.exit(3)"])
    with pytest.raises(RuntimeError) as ex:
        broken.load()
    msg = str(ex.value)
    assert "was built from other sources" in msg and "cannot be rebuilt here" in msg and have in msg and want in msg
    assert _dgs_build.recorded_hash(t.lib.path) == have       # the old binary and its record are untouched


@pytest.mark.parametrize("record", ["missing", "stale"])
def test_an_override_is_the_callers_own_build(tmp_path, monkeypatch, record):
    other = str(tmp_path / "ab_variant.so")
    with open(str(tmp_path / "variant.cpp"), "w") as f:
        f.write("#define TINY_ABI 2\n#define TINY_BIAS 7\n" + SOURCE.replace('#include "tiny.h"\n', ""))
    subprocess.check_call(["g++"] + FLAGS + [str(tmp_path / "variant.cpp"), "-o", other])
    if record == "stale":
        with open(other + ".srchash", "w") as f:
            f.write("0123456789abcdef\n")
    monkeypatch.setenv("TINY_LIB", other)
    t = Tiny(tmp_path, env="TINY_LIB")
    assert t.lib.path == other and t.lib.default_path != other
    assert t.lib.load().tiny_add(2, 3) == 12                  # the variant, as it is: no hash check ...
    assert t.compiles() == 0                                  # ... and no rebuild
    assert not os.path.exists(t.lib.default_path)


def test_other_abi_version_is_refused(tmp_path):
    t = Tiny(tmp_path, abi=1)
    t.lib.build()
    with pytest.raises(RuntimeError, match=r"libtiny\.so ABI version mismatch \(want 2, library says 1\)"):
        t.lib.load()


def test_missing_library_names_the_build(tmp_path):
    t = Tiny(tmp_path)
    with pytest.raises(RuntimeError) as ex:
        t.lib.load()
    assert t.lib.path in str(ex.value) and "not found; build it with __graft_entry__.build()" in str(ex.value)
    assert t.compiles() == 0


def test_prototypes_and_error_check_come_from_the_table(tmp_path):
    t = Tiny(tmp_path)
    t.lib.build()
    lib = t.lib.load()
    for name, (restype, argtypes) in SIGNATURES.items():
        assert getattr(lib, name).restype is restype and list(getattr(lib, name).argtypes) == argtypes
    with pytest.raises(ctypes.ArgumentError):
        lib.tiny_add("2", 3)
    with pytest.raises(TypeError):
        lib.tiny_add(2)                                       # declared arity: ctypes refuses a short call
    t.lib.check(0, "tiny_add")
    with pytest.raises(RuntimeError, match=r"tiny_add failed \(-3\): tiny went wrong"):
        t.lib.check(-3, "tiny_add")
