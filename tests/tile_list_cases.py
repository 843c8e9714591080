"""Rasterizer inputs whose per-tile lists are known by construction (tests/test_tile_lists_cpu.py, tests/test_tile_lists_gpu.py).

A scene is built from entries (tile_x, tile_y, depth_bits uint32[n]): one tiny camera-facing surfel per depth at the centre of that
tile.  The view matrix is the identity (world space = camera space), so the depth the rasterizer computes is pv[2] = 0 x + 0 y + 1 z + 0
= z BIT FOR BIT, and with a radius of 3 .. 6 px around pixel 8 of the tile the reference rectangle is exactly that tile.  The expected
lists are then np.lexsort((index, depth_bits, tile)): pure NumPy, no device code and no oracle.  Scenes that also hold multi-tile discs
(`many_tiles`, `rectangles`) take the rectangles from the oracle's radii / means2D through the getRect formula (surfel_math.h
tile_rect) -- reference_lists().

Depth classes control what the per-tile radix sort (tile_sort_kernels.h) does: it sorts only the bits in which a list's depths differ
(nbits from the xor of the list's AND and OR), 8 per pass.  From two entries on, every class pins two of its values so that nbits is
exactly the class's figure whatever the generator drew.
"""
import functools
import math

import numpy as np
import torch

TILE = 16
NEAR = 0.2   # the rasterizer culls z <= 0.2
MAX_TIE_RUN = 1500   # the tie pass is an insertion sort by one thread: quadratic.  A limit on test time, not a property under test.


# ---- depth classes: n -> uint32[n] ---------------------------------------------------------------------------------------------------
def _rng(tag, n, salt):
    return np.random.default_rng([0x711e, tag, n, salt])


def _pin(d, lo, hi):
    """Two pinned values: the xor of the list's AND and OR is lo ^ hi at least, so nbits does not depend on the draw."""
    if len(d) >= 2:
        d[0], d[1] = lo, hi
    return d.astype(np.uint32)


def depths_E(n, salt=0):
    """All equal: nbits = 0, no pass, the list is one tie run."""
    return np.full(n, 0x40490fdb, np.uint32)


def depths_B1(n, salt=0):
    """8 low bits: one pass."""
    d = 0x40000000 | _rng(1, n, salt).integers(0, 1 << 8, n, dtype=np.uint32)
    return _pin(d, 0x40000001, 0x400000fe)


def depths_B2(n, salt=0):
    """16 low bits, one of bits 8-15 set: two passes."""
    g = _rng(2, n, salt)
    d = 0x40000000 | g.integers(0, 1 << 16, n, dtype=np.uint32) | (np.uint32(1) << g.integers(8, 16, n, dtype=np.uint32))
    return _pin(d, 0x40000101, 0x4000fffe)


def depths_B3(n, salt=0):
    """z uniform in [2, 4): the 23 mantissa bits, three passes."""
    d = _rng(3, n, salt).uniform(2.0, 4.0, n).astype(np.float32)
    d = np.minimum(d, np.float32(3.9999998)).view(np.uint32).copy()
    return _pin(d, 0x40000001, 0x407ffffe)


def depths_B4(n, salt=0):
    """z log-uniform in [0.25, 2^20): the exponent's top bits differ, four passes."""
    d = np.exp2(_rng(4, n, salt).uniform(-2.0, 20.0, n)).astype(np.float32)
    d = np.clip(d, np.float32(0.25), np.float32(1048575.9)).view(np.uint32).copy()
    return _pin(d, 0x3e800001, 0x497ffffe)


def depths_H(n, salt=0):
    """7 bits at 16-22: the two low digits are constant, their passes put every key in one bin."""
    d = 0x40000000 | (_rng(5, n, salt).integers(0, 1 << 7, n, dtype=np.uint32) << 16)
    return _pin(d, 0x40010000, 0x407e0000)


def depths_T(n, salt=0, run=0):
    """B3 values from a pool of n / 8: many short tie runs; `run` > 0 makes that many entries one value."""
    g = _rng(6, n, salt)
    pool = depths_B3(max(n // 8, 2), salt + 1000)
    d = pool[g.integers(0, len(pool), n)]
    if run:
        d[2:2 + run] = pool[2]
    return _pin(d, pool[0], pool[1])


CLASSES = {"E": depths_E, "B1": depths_B1, "B2": depths_B2, "B3": depths_B3, "B4": depths_B4, "H": depths_H, "T": depths_T}
# what a list of two or more entries must show: nbits as the kernel computes it, and the most distinct depths it can hold
CLASS_NBITS = {"E": 0, "B1": 8, "B2": 16, "B3": 23, "B4": 31, "H": 23, "T": 23}
CLASS_MAX_DISTINCT = {"E": lambda n: 1, "B1": lambda n: 256, "B2": lambda n: 65536, "B3": lambda n: n, "B4": lambda n: n,
                      "H": lambda n: 128, "T": lambda n: max(n // 8, 2)}


def nbits_of(d):
    """The radix kernel's figure: the bits in which the list differs, from the xor of its AND and its OR."""
    d = np.asarray(d, np.uint32)
    diff = int(np.bitwise_and.reduce(d)) ^ int(np.bitwise_or.reduce(d))
    return diff.bit_length()


def longest_tie_run(d):
    _, c = np.unique(np.asarray(d, np.uint32), return_counts=True)
    return int(c.max()) if len(c) else 0


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """name, W, H, lists = [(tile, class name, depth_bits)] of the single-tile surfels, discs = (px, py, radius_px, depth_bits, opacity)
    arrays of the multi-tile ones (or None), case = the rasterizer inputs, tile_of / depth_bits per surfel index (tile -1: a disc)."""

    def __init__(self, name, W, H, lists, discs=None, shuffle=True, seed=0):
        self.name, self.W, self.H = name, W, H
        self.tiles_x, self.tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        self.ntiles = self.tiles_x * self.tiles_y
        self.lists = lists
        tiles = [t for t, _, _ in lists]
        assert len(set(tiles)) == len(tiles) and all(0 <= t < self.ntiles for t in tiles)
        fx, fy = W / 2.0, H / 2.0   # tanfovx = 1, tanfovy = H / W: focal = W / (2 tanfovx) = H / (2 tanfovy)
        tile = np.concatenate([np.full(len(d), t, np.int64) for t, _, d in lists] or [np.zeros(0, np.int64)])
        bits = np.concatenate([d for _, _, d in lists] or [np.zeros(0, np.uint32)]).astype(np.uint32)
        z = bits.view(np.float32).astype(np.float64)
        px = TILE * (tile % self.tiles_x) + TILE // 2
        py = TILE * (tile // self.tiles_x) + TILE // 2
        scale = 1e-4 * z
        opac = np.full(len(z), 0.9)
        if discs is not None:
            dpx, dpy, drad, dbits, dop = discs
            dz = np.asarray(dbits, np.uint32).view(np.float32).astype(np.float64)
            tile = np.concatenate([tile, np.full(len(dz), -1, np.int64)])
            bits = np.concatenate([bits, np.asarray(dbits, np.uint32)])
            px, py = np.concatenate([px, dpx]), np.concatenate([py, dpy])
            # radius = ceil(3 extent), extent ~ fx scale / z: half a pixel below the target so that ceil lands on it
            scale = np.concatenate([scale, (np.asarray(drad, np.float64) - 0.5) / 3.0 / fx * dz])
            opac = np.concatenate([opac, dop])
            z = np.concatenate([z, dz])
        assert np.all(z > NEAR)
        P = len(z)
        perm = np.random.default_rng([0x5eed, seed]).permutation(P) if shuffle else np.arange(P)
        tile, bits, z, px, py, scale, opac = (a[perm] for a in (tile, bits, z, px, py, scale, opac))
        self.tile_of, self.depth_bits, self.P = tile, bits, P
        xyz = np.stack([(px - W / 2.0) / fx * z, (py - H / 2.0) / fy * z, z], 1).astype(np.float32)   # float64, rounded once
        assert np.array_equal(xyz[:, 2].view(np.uint32), bits)
        rot = np.zeros((P, 4), np.float32)
        rot[:, 0] = 1.0
        znear, zfar = 0.01, 100.0
        proj = np.zeros((4, 4), np.float32)   # ordinary perspective projection, row-vector convention (cameras.projection_matrix, transposed)
        proj[0, 0], proj[1, 1] = 1.0, W / H
        proj[2, 2], proj[3, 2], proj[2, 3] = zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
        self.case = dict(
            means3D=f32(xyz), scales=f32(np.stack([scale, scale], 1)), rotations=f32(rot), opacities=f32(opac[:, None]),
            shs=torch.full((P, 1, 3), 0.5), sh_degree=0, viewmatrix=torch.eye(4), projmatrix=f32(proj), campos=torch.zeros(3),
            bg=torch.zeros(3), tanfovx=1.0, tanfovy=H / W, image_height=H, image_width=W)

    # -- expected lists
    def list_lengths(self):
        """Designed length per tile of the single-tile surfels."""
        return np.bincount(self.tile_of[self.tile_of >= 0], minlength=self.ntiles)

    def class_of_tile(self):
        return {t: (c, len(d)) for t, c, d in self.lists}

    def designed_lists(self):
        """(point_list, ranges) by construction; only for scenes without discs."""
        assert not (self.tile_of < 0).any()
        return lists_from_entries(self.tile_of, np.arange(self.P), self.depth_bits, self.ntiles)


def lists_from_entries(tile, index, depth_bits, ntiles):
    """The reference's order: by tile, then depth bits, then surfel index -> (point_list uint32[R], ranges uint32[T, 2])."""
    tile, index = np.asarray(tile, np.int64), np.asarray(index, np.int64)
    o = np.lexsort((index, np.asarray(depth_bits, np.uint32)[index], tile))
    cnt = np.bincount(tile, minlength=ntiles)
    end = np.cumsum(cnt)
    ranges = np.stack([end - cnt, end], 1).astype(np.uint32)
    return index[o].astype(np.uint32), ranges


def tile_rects(px, py, radii, tiles_x, tiles_y):
    """getRect (surfel_math.h tile_rect) in NumPy: float32 arithmetic, truncation toward zero, clamped to the grid."""
    px, py, r = np.asarray(px, np.float32), np.asarray(py, np.float32), np.asarray(radii).astype(np.float32)
    t = np.float32(TILE)
    x0 = np.clip(np.trunc((px - r) / t).astype(np.int64), 0, tiles_x)
    y0 = np.clip(np.trunc((py - r) / t).astype(np.int64), 0, tiles_y)
    x1 = np.clip(np.trunc((px + r + np.float32(TILE - 1)) / t).astype(np.int64), 0, tiles_x)
    y1 = np.clip(np.trunc((py + r + np.float32(TILE - 1)) / t).astype(np.int64), 0, tiles_y)
    return x0, y0, x1, y1


def reference_lists(scene, means2D, radii):
    """Expected lists of any scene from the oracle's radii and means2D: every visible surfel enters each tile of its rectangle."""
    x0, y0, x1, y1 = tile_rects(means2D[:, 0], means2D[:, 1], radii, scene.tiles_x, scene.tiles_y)
    w, h = np.maximum(x1 - x0, 0), np.maximum(y1 - y0, 0)
    area = np.where(np.asarray(radii) > 0, w * h, 0)
    idx = np.repeat(np.arange(scene.P), area)
    k = np.arange(int(area.sum())) - np.repeat(np.cumsum(area) - area, area)   # position inside the surfel's rectangle
    wi = np.maximum(w[idx], 1)
    tile = (y0[idx] + k // wi) * scene.tiles_x + x0[idx] + k % wi
    pl, ranges = lists_from_entries(tile, idx, scene.depth_bits, scene.ntiles)
    return pl, ranges, area


def _even_tiles(ntiles, taken):
    """Tiles of even linear index on an odd-width grid form a checkerboard: every list has four empty neighbours."""
    return [t for t in range(0, ntiles, 2) if t not in taken]


EDGE_LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048)
EDGE_LONG = {4: ("B2", 2049), 260: ("B4", 6000), 130: ("B3", 4096), 288: ("T", 4097)}   # 4 and 260: one workgroup column of the 256


def _edges(with_long):
    lists = []
    if with_long:
        for t, (c, n) in EDGE_LONG.items():
            lists.append((t, c, depths_T(n, run=600) if c == "T" else CLASSES[c](n)))
    free = iter(_even_tiles(289, set(EDGE_LONG)))   # the same tiles with and without the long lists
    for n in EDGE_LENGTHS:
        for c in ("B1", "B2", "B3", "B4"):
            lists.append((next(free), c, CLASSES[c](n)))
    for c in ("E", "H", "T"):
        for n in (300, 1500):
            lists.append((next(free), c, CLASSES[c](n)))
    return Scene("edges" if with_long else "edges_short", 272, 272, lists, seed=1)


# tiles 10 / 266 and 30 / 286 are 256 apart: one workgroup column of every grid-stride sort kernel takes both lists of a pair
LONG_LISTS = {30: ("B4", 16384), 10: ("B4", 16385), 286: ("B4", 57344), 266: ("B4", 57345), 150: ("T", 4097)}


def _long(with_overlong):
    lists = []
    for t, (c, n) in LONG_LISTS.items():
        if n == 57345 and not with_overlong:
            continue
        lists.append((t, c, depths_T(n, salt=1, run=600) if c == "T" else CLASSES[c](n, salt=t)))
    return Scene("long" if with_overlong else "long_fit", 272, 272, lists, seed=2)


def _disc_arrays(rows):
    a = np.asarray(rows, np.float64).reshape(-1, 5)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3].astype(np.uint32), a[:, 4]


# A disc of radius 16 m (+-7) px centred on pixel 8 of tile t covers tiles t - m .. t + m (2 m + 1 of them); radius 16 m - 8 (+-7)
# centred on the tile's first pixel covers t - m .. t + m - 1 (2 m of them) -- the margins of tile_rect's two divisions.
def _disc(tx, ty, wx, bits, opacity):
    m = wx // 2
    if wx % 2:
        return (TILE * tx + 8, TILE * ty + 8, 16 * m if m else 3, bits, opacity)
    return (TILE * tx, TILE * ty, 16 * m - 8, bits, opacity)


def _many_tiles():
    W = 3088   # 193 x 193 = 37 249 tiles: the first square image past the 36 864 counters of the LDS histogram
    tx = 193
    g = np.random.default_rng(0x3a17)
    lists = [(0, "B4", depths_B4(1, 7)), (5 * tx + 100, "B4", depths_B4(5, 7)), (97 * tx + 41, "B4", depths_B4(300, 7)),
             (tx * tx - 1, "B4", depths_B4(2049, 7))]
    taken = {t for t, _, _ in lists}
    tiles = [int(t) for t in g.permutation(tx * tx) if int(t) not in taken][:200]
    for i, t in enumerate(tiles):
        c = ("B1", "B2", "B3", "B4")[i % 4]
        lists.append((t, c, CLASSES[c](int(g.integers(1, 40)), salt=i)))
    db = depths_B4(12, 99)
    discs = [_disc(50, 60, 2, db[0], 0.6), _disc(120, 30, 3, db[1], 0.5), _disc(20, 150, 4, db[2], 0.4), _disc(96, 96, 5, db[3], 0.7),
             _disc(150, 150, 6, db[4], 0.3), _disc(0, 100, 4, db[5], 0.5), _disc(192, 40, 5, db[6], 0.5), _disc(70, 0, 6, db[7], 0.6),
             _disc(100, 192, 3, db[8], 0.4), _disc(193, 193, 4, db[9], 0.5), _disc(0, 0, 6, db[10], 0.5), _disc(97, 41, 3, db[11], 0.5)]
    return Scene("many_tiles", W, W, lists, _disc_arrays(discs), seed=3)


def _rectangles():
    g = np.random.default_rng(0x4ec7)
    rows = []
    n = 2000
    db = depths_B4(n, 5)
    # designed ones first in every group of eight (count_tiles_lds_kernel gives a workgroup ceil(P / 256) = 8 consecutive surfels: these
    # are the lanes one wave holds), random ones around them
    designed = []
    for t in (4, 5, 8, 12, 13):
        designed.append((t, 8, 8))     # area exactly 64: the last size a single thread walks
    for t in (4, 8, 12):
        designed.append((t, 8, 9))     # 81
    designed += [(0, 8, 16), (17, 8, 16), (8, 0, 16), (8, 17, 16)]    # 8 x 16 halves clipped at each border (128)
    designed += [(4, 0, 9), (4, 16, 9), (0, 4, 9), (16, 4, 9)]        # 9 x 5 = 45 clipped
    designed += [(8, 2, 9), (8, 3, 9), (2, 8, 9)]                     # 9 x 7 = 63, 9 x 8 = 72 clipped
    designed += [(8, 8, 35), (9, 9, 36), (7, 8, 37), (8, 8, 41)]      # the whole screen (289)
    for i in range(n):
        if i % 8 == 0 and i // 8 < len(designed):
            tx, ty, wx = designed[i // 8]
            rows.append(_disc(tx, ty, wx, db[i], 0.0))
        else:
            big = g.random() < 0.4
            r = float(np.exp(g.uniform(math.log(60.0), math.log(300.0)))) if big else float(np.exp(g.uniform(math.log(3.0), math.log(70.0))))
            rows.append((g.uniform(-20.0, 292.0), g.uniform(-20.0, 292.0), r, db[i], 0.0))
    a = np.asarray(rows, np.float64)
    # thin discs, so that pixels walk hundreds of entries.  The generator is one for which no pixel has an entry on the 1/255 alpha
    # threshold to fp32 rounding (two of eight tried have one or two; test_tile_lists_cpu.py holds the scene to it)
    a[:, 4] = np.random.default_rng(1000).uniform(0.02, 0.3, n)
    return Scene("rectangles", 272, 272, [], _disc_arrays(a), shuffle=False, seed=4)


_BUILDERS = {"edges": lambda: _edges(True), "edges_short": lambda: _edges(False), "long": lambda: _long(True),
             "long_fit": lambda: _long(False), "many_tiles": _many_tiles, "rectangles": _rectangles}
SCENES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def scene(name):
    return _BUILDERS[name]()


def oracle_f64(name):
    """The fp64 build's forward (not kept: 1.5 GB of planes on the 3088 x 3088 scene)."""
    from scene_utils import oracle_from_case
    return oracle_from_case(scene(name).case, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The fp32 CPU oracle's forward of a scene, computed once and shared (read-only) by the tests of a module; release() drops them."""
    from scene_utils import oracle_from_case
    return oracle_from_case(scene(name).case, dtype=np.float32)


def release():
    """Drops the cached oracle runs (hundreds of MB on the large scene): the test modules call it when they are done."""
    expected.cache_clear()
    oracle.cache_clear()


@functools.lru_cache(maxsize=None)
def expected(name):
    """(point_list, ranges) of a scene: by construction where every surfel is a single-tile one, else from the oracle's rectangles."""
    s = scene(name)
    if not (s.tile_of < 0).any():
        return s.designed_lists()
    o = oracle(name)
    return reference_lists(s, o.field("means2D"), o.radii)[:2]
