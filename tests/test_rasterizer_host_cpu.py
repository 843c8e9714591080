"""The host side of the surfel rasterizer that needs no device: every kernel header compiles on its own, the option surface of a
context (defaults, accepted ranges, 0/1 normalisation, refusals and their texts) and the byte layout of the three scratch buffers.
The expected option values and layout numbers are literals, recorded from the library before its host file was split into stage
functions: they hold that file to what it computed."""
import ctypes
import glob
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamic-2dgs_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))
INT_MAX = 2 ** 31 - 1
INVALID = -1   # DGS_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    """A header includes what it uses: no other header has to come first."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not found")
    main = tmp_path / "alone.hip"
    main.write_text('#include "%s"\n' % header)
    run = subprocess.run(["hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(main)],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout[-4000:]


def test_there_are_kernel_headers_to_check():
    assert len(HEADERS) >= 15 and "surfel_math.h" in HEADERS and "blend_common.h" in HEADERS


@pytest.fixture(scope="module")
def lib():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "dynamic-2dgs_amd"))
    from diff_surfel_rasterization import _C
    return _C.load()


@pytest.fixture
def ctx(lib, monkeypatch):
    for name in ("DGS_LONG_TILES", "DGS_MERGED_OFFSETS", "DGS_ORDER_RIDER", "DGS_ACC_RIDER"):
        monkeypatch.delenv(name, raising=False)
    c = lib.dgs_context_create()
    assert c
    yield c
    lib.dgs_context_destroy(c)


# key: (default, accepted boundary values, refused values); key 2 is only ever set to 0 here (a value > 0 allocates on the device)
BOOLEAN_KEYS = {0: 1, 8: 0, 9: 1, 12: 1, 13: 1, 14: 1}   # key: default
RANGE_KEYS = {
    1: (3, (0, 4), (5, -1, INT_MAX)),
    2: (0, (0,), (-1, -INT_MAX)),
    3: (2, (0, 2), (3, -1, INT_MAX)),
    4: (0, (0, INT_MAX), (-1,)),
    5: (0, (0, INT_MAX), (-1,)),
    6: (0, (0, INT_MAX), (-1,)),
    7: (0, (0, 2), (3, -1, INT_MAX)),
    10: (400, (1, INT_MAX), (0, -1)),
    11: (512, (1, INT_MAX), (0, -1)),
}
SET_REFUSAL = b"dgs_set_option: unknown key / value"
GET_REFUSAL = b"dgs_get_option: unknown key"


def test_option_defaults(lib, ctx):
    want = dict(BOOLEAN_KEYS)
    want.update({k: v[0] for k, v in RANGE_KEYS.items()})
    assert sorted(want) == list(range(15))
    assert [lib.dgs_context_get_option(ctx, k) for k in range(15)] == [want[k] for k in range(15)]
    assert [want[k] for k in range(15)] == [1, 3, 0, 2, 0, 0, 0, 0, 0, 1, 400, 512, 1, 1, 1]


@pytest.mark.parametrize("var,key", [("DGS_LONG_TILES", 9), ("DGS_MERGED_OFFSETS", 12), ("DGS_ORDER_RIDER", 13), ("DGS_ACC_RIDER", 14)])
def test_option_defaults_from_the_environment(lib, monkeypatch, var, key):
    for value, want in (("0", 0), ("1", 1), ("5", 1)):
        monkeypatch.setenv(var, value)
        c = lib.dgs_context_create()
        try:
            got = [lib.dgs_context_get_option(c, k) for k in (9, 12, 13, 14)]
        finally:
            lib.dgs_context_destroy(c)
        assert got == [want if k == key else 1 for k in (9, 12, 13, 14)]


def test_option_boundaries_are_accepted_and_read_back(lib, ctx):
    for key, (default, accepted, _) in RANGE_KEYS.items():
        for value in accepted + (default,):
            assert lib.dgs_context_set_option(ctx, key, value) == 0, (key, value)
            assert lib.dgs_context_get_option(ctx, key) == value, (key, value)
    for key, default in BOOLEAN_KEYS.items():
        for value, want in ((0, 0), (1, 1), (2, 1), (-3, 1), (INT_MAX, 1), (-INT_MAX - 1, 1), (0, 0), (default, default)):
            assert lib.dgs_context_set_option(ctx, key, value) == 0, (key, value)
            assert lib.dgs_context_get_option(ctx, key) == want, (key, value)


def test_option_refusals(lib, ctx):
    for key, (default, _, refused) in RANGE_KEYS.items():
        for value in refused:
            assert lib.dgs_context_set_option(ctx, key, value) == INVALID, (key, value)
            assert lib.dgs_last_error() == SET_REFUSAL
            assert lib.dgs_context_get_option(ctx, key) == default, (key, value)   # a refused value changes nothing
    for key in (15, -1, 1000):
        for value in (0, 1):
            assert lib.dgs_context_set_option(ctx, key, value) == INVALID and lib.dgs_last_error() == SET_REFUSAL
        assert lib.dgs_context_get_option(ctx, key) == INVALID and lib.dgs_last_error() == GET_REFUSAL
    assert lib.dgs_context_set_option(None, 0, 1) == INVALID and lib.dgs_last_error() == b"context is NULL"
    assert lib.dgs_context_get_option(None, 0) == INVALID and lib.dgs_last_error() == b"context is NULL"


def test_leaving_capacity_mode_clears_the_list_promise(lib, ctx):
    assert lib.dgs_context_set_option(ctx, 6, 2048) == 0 and lib.dgs_context_get_option(ctx, 6) == 2048
    assert lib.dgs_context_set_option(ctx, 2, 0) == 0
    assert lib.dgs_context_get_option(ctx, 6) == 0 and lib.dgs_context_get_option(ctx, 2) == 0


# dgs_debug_layout: (offsets..., total).  Geometry depends on P alone, the image buffer on (W, H) alone, binning on R alone.
GEOMETRY = {
    1: (0, 128, 256, 384, 512, 640),
    1000: (0, 96000, 96128, 100224, 180224, 188288),
    200000: (0, 19200000, 19200128, 20000128, 36000128, 37600128),
}
IMAGE = {   # 3088 x 3088 = 37 249 tiles: past the 36 864 whose histogram fits the LDS, so `cursor` has its other size
    (16, 16): (0, 3072, 5120, 5248, 5376, 6400, 11520, 11648, 12800),
    (17, 33): (0, 18432, 30720, 30848, 30976, 32000, 37120, 37248, 43520),
    (800, 800): (0, 7680000, 12800000, 12820096, 12830208, 12841984, 12857856, 12867968, 15428096),
    (1600, 1600): (0, 30720000, 51200000, 51280000, 51320064, 51361024, 51406080, 51446144, 61686272),
    (3088, 3088): (0, 114428928, 190714880, 191012992, 191162112, 191316736, 191475456, 191624576, 191773824),
}
BINNING = {
    0: (0, 128, 256, 384),
    1: (0, 128, 256, 384),
    123457: (0, 493952, 1481728, 1481856),
}


def _layout(lib, which, P, W, H, R, cap=16):
    buf = (ctypes.c_size_t * 16)(*([2 ** 64 - 1] * 16))
    n = lib.dgs_debug_layout(which, P, W, H, R, buf, cap)
    return n, tuple(buf[i] for i in range(16))


def test_debug_layout_offsets_and_totals(lib):
    for which, P, (W, H), R in itertools.product((0, 1, 2), GEOMETRY, IMAGE, BINNING):
        want = (GEOMETRY[P], IMAGE[(W, H)], BINNING[R])[which]
        n, got = _layout(lib, which, P, W, H, R)
        assert n == len(want) and got[:n] == want, (which, P, W, H, R)
        assert all(v == 2 ** 64 - 1 for v in got[n:])
    n, got = _layout(lib, 1, 1, 800, 800, 0, cap=3)    # a short array gets the first `cap` entries
    assert n == 3 and got[:3] == IMAGE[(800, 800)][:3] and got[3] == 2 ** 64 - 1
    assert lib.dgs_debug_layout(3, 1, 16, 16, 0, (ctypes.c_size_t * 16)(), 16) == INVALID
    assert lib.dgs_last_error() == b"dgs_debug_layout: which must be 0, 1 or 2"
