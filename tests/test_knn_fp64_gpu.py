"""-m gpu: the three neighbour-search kernels of csrc/knn_kernels.h (knn_kernel, knn_refine_kernel, knn_refine_mfma_kernel) against
the float64 statement of tests/knn_ref.py, through the entry points the trainer uses (_ops.knn_indices, _ops.knn_indices2) and, for
the arguments Python does not expose (dist2, refused shapes), the C library of _ops.load().

In every test the plain scan is held to float64 by knn_ref.check_answer (range, distinct, entry-for-entry equality on the decided
points, the gap on the others; GAP and the dist2 bound are derived in knn_ref from the kernels' arithmetic, CAP is a condition on
the inputs that tests/test_knn_ref_cpu.py checks without a GPU) and both seeded kernels must be torch.equal to it: equal tensors
satisfy the same check.  Run with -s for one `knn-margin` line per case (profiles/knn_margins.md)."""
import functools

import pytest
import torch

import knn_ref as kr

pytestmark = pytest.mark.gpu
MODES = ("box", "mfma")


def _ops():
    from dgs_amd import _ops
    return _ops


def _id(v):
    return "-".join(str(e) for e in v) if isinstance(v, tuple) else str(v)


@functools.lru_cache(maxsize=None)
def _dev(name, N, M, D):
    """The case's inputs on the GPU: shared, never modified."""
    x, nodes = kr.build(name, N, M, D)
    return x.cuda(), nodes.cuda()


def _plain(x, nodes, K):
    return _ops().knn_indices(x, nodes, K)


def _split(x):
    """x1[N,3] contiguous, x2 = the remaining columns as a true column slice (row stride D), as deform.py passes them."""
    return x[:, :3].contiguous(), x[:, 3:]


def _refine(x, nodes, K, seed, mode):
    x1, x2 = _split(x)
    seed = seed.clone()
    got = _ops().knn_indices2(x1, x2, nodes, K, seed=seed, mode=mode)
    assert got.data_ptr() == seed.data_ptr()
    return got


def _seeds(want, M, tag=0):
    """Everything a seed may hold: the answer, another point's answer, random nodes, one node K times, out-of-range garbage, and
    valid indices plus 2^32 (they must not be truncated to 32 bits before the range check)."""
    N, K = want.shape
    g = torch.Generator().manual_seed(300 + tag)
    s = {"exact": want.clone(), "rolled": torch.roll(want, 1, 0).contiguous(),
         "random": torch.randint(0, M, (N, K), generator=g).cuda(),
         "garbage": torch.randint(-5, 3 * M, (N, K), generator=g).cuda(),
         "plus 2^32": want + (1 << 32)}
    if K > 1:
        s["repeated"] = want[:, :1].repeat(1, K).contiguous()
    return s


def _held(case, want, x, nodes, K, dist2=None, what=""):
    """check_answer + the cap on the undecided share + the margin line."""
    st = kr.check_answer(want, x, nodes, K, dist2=dist2)
    print("knn-margin %-22s %-8s N=%-6d M=%-4d D=%-2d K=%d undecided %.2e dist2_rel %.3e (bound %.3e)"
          % ((what,) + tuple(case) + (st["undecided"], st["dist2_rel"], kr.DIST_REL)))
    assert st["undecided"] <= kr.CAP, st
    return st


def _all_three(case, seeds=None, modes=MODES, nodes_view=None, what=""):
    """The plain scan satisfies check_answer; every (mode, seed) of the seeded kernels equals it bit for bit."""
    name, N, M, D, K = case
    x, nodes = _dev(name, N, M, D)
    nd = nodes if nodes_view is None else nodes_view(nodes)
    want = _plain(x, nd, K)
    _held(case, want, x, nodes, K, what=what)
    for sname, seed in (_seeds(want, M) if seeds is None else seeds(want)).items():
        for mode in modes:
            got = _refine(x, nd, K, seed, mode)
            assert torch.equal(got, want), (case, mode, sname, int((got != want).any(1).sum()))
    return want


# ---- plain scan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.PLAIN_KQ + kr.PLAIN_STAGING + kr.PLAIN_SMALL_N, ids=_id)
def test_plain_scan_every_k_and_q(case):
    """knn_kernel<K, Q> for every K and every Q = ceil(D / 4) (D = 3, 4: Q = 1; 5: 2; 11: 3; 16: 4), three ragged workgroups; node
    counts that take two and three 1024-node staging passes with a remainder of one; point counts around one workgroup."""
    name, N, M, D, K = case
    x, nodes = _dev(name, N, M, D)
    _held(case, _plain(x, nodes, K), x, nodes, K, what="plain")


def _raw_points(x, nodes, K, with_dist2, split):
    """dgs_knn_points / dgs_knn_points2 through the C library: (idx, dist2 or None)."""
    ops = _ops()
    lib = ops.load()
    (N, D), M = x.shape, nodes.shape[0]
    idx = torch.full((N, K), -7, dtype=torch.int64, device=x.device)
    d2 = torch.full((N, K), float("nan"), dtype=torch.float32, device=x.device) if with_dist2 else None
    dp = d2.data_ptr() if with_dist2 else None
    with torch.cuda.device(x.device):
        if split:
            x1, x2 = _split(x)
            rc = lib.dgs_knn_points2(N, M, 3, D - 3, K, x1.data_ptr(), x2.data_ptr(), x2.stride(0), nodes.data_ptr(), idx.data_ptr(), dp,
                                     ops._stream(x.device))
        else:
            rc = lib.dgs_knn_points(N, M, D, K, x.data_ptr(), nodes.data_ptr(), idx.data_ptr(), dp, ops._stream(x.device))
    assert rc == 0, rc
    return idx, d2


@pytest.mark.parametrize("split", [False, True], ids=["points", "points2"])
@pytest.mark.parametrize("case", kr.DIST2, ids=_id)
def test_dist2_output(case, split):
    """The distance output no Python caller asks for: ascending, within 19 * 2^-24 relative of the float64 distance of the
    returned node, and asking for it does not change the indices."""
    name, N, M, D, K = case
    x, nodes = _dev(name, N, M, D)
    idx, d2 = _raw_points(x, nodes, K, True, split)
    bare, _ = _raw_points(x, nodes, K, False, split)
    assert torch.equal(idx, bare) and torch.equal(idx, _plain(x, nodes, K))
    assert bool((d2[:, 1:] >= d2[:, :-1]).all())
    _held(case, idx, x, nodes, K, dist2=d2, what="dist2/" + ("points2" if split else "points"))


@pytest.mark.parametrize("H", kr.SPLIT_H)
def test_split_query_plain_scan(H):
    """knn_indices2(x, feat[:, :H]) with feat 16 columns wide (row stride 16 > H) == knn_indices(cat)."""
    case = ("unit", 1537, 257, 3 + H, 3)
    x, nodes = _dev(*case[:4])
    feat = torch.full((x.shape[0], 16), 7.0, device="cuda")      # columns past H hold values that would change the answer
    feat[:, :H] = x[:, 3:]
    got = _ops().knn_indices2(x[:, :3].contiguous(), feat[:, :H], nodes, 3)
    assert torch.equal(got, _plain(x, nodes, 3))
    _held(case, got, x, nodes, 3, what="split H=%d" % H)


@pytest.mark.parametrize("mode", MODES)
def test_split_query_refine(mode):
    case = ("unit", 4099, 200, 11, 3)
    x, nodes = _dev(*case[:4])
    feat = torch.full((x.shape[0], 16), 7.0, device="cuda")
    feat[:, :8] = x[:, 3:]
    want = _plain(x, nodes, 3)
    _held(case, want, x, nodes, 3, what="split refine " + mode)
    for sname, seed in _seeds(want, 200).items():
        got = _ops().knn_indices2(x[:, :3].contiguous(), feat[:, :8], nodes, 3, seed=seed, mode=mode)
        assert torch.equal(got, want), (mode, sname)


# ---- 3-D culling refine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.BOX_KQ, ids=_id)
def test_box_refine_every_k_and_q(case):
    """knn_refine_kernel<K, Q> for every K and Q, D2 = 0 (no second array: x2 unused) to 13 (D = 16, which the matrix-core
    kernel must refuse: "mfma" takes the same kernel there), every kind of seed."""
    _all_three(case, what="box")


@pytest.mark.parametrize("aligned", [False, True], ids=["unaligned", "aligned"])
@pytest.mark.parametrize("case", kr.BOX_LAYOUT, ids=_id)
def test_box_refine_table_layout(case, aligned):
    """The node table is read as 16-byte vectors plus a scalar tail of M * D mod 4 floats; a table that does not start on a
    16-byte boundary (row 1 of an 11-column table: 44 bytes in) goes through the scalar tail alone."""
    def view(nodes):
        if aligned:
            assert nodes.data_ptr() % 16 == 0
            return nodes
        big = torch.zeros((nodes.shape[0] + 1, nodes.shape[1]), device="cuda")
        big[0] = 1e3
        big[1:] = nodes
        v = big[1:]
        assert v.is_contiguous() and v.data_ptr() % 16 != 0
        return v
    assert (case[2] * case[3]) % 4 != 0
    _all_three(case, modes=("box",), nodes_view=view, what="layout " + ("aligned" if aligned else "unaligned"))


@pytest.mark.parametrize("case,mode", list(zip(kr.BOX_LARGE, ("box", "mfma"))), ids=_id)
def test_box_refine_large_tables(case, mode):
    """The largest table the C ABI promises (2048 nodes, D = 16: 154 KB of dynamic LDS) and a table the matrix-core kernel does not
    take (1025 nodes) requested as "mfma": both must launch and be exact."""
    _all_three(case, modes=(mode,), what="large " + mode)


# ---- matrix-core refine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.MFMA_KTP + kr.MFMA_SMALL_N, ids=_id)
def test_mfma_refine_every_k_and_tp(case):
    """knn_refine_mfma_kernel<K, TP> for every K on both sides of the TP = 4 / 8 / 16 boundaries (256 | 257, 512 | 513 nodes), a
    single tile and one node more, the largest table, 11 and 5 coordinates; point counts around one 32-point group."""
    _all_three(case, modes=("mfma",), what="mfma")


def test_mfma_refine_second_grid_stride_trip():
    """A point count at which every wave takes a second trip of the grid-stride loop (CU count read like the launcher reads it).
    The seeds are wrong everywhere, so a group that is never visited keeps a wrong answer."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, M, K = kr.stride_points(cus), kr.STRIDE_M, kr.STRIDE_K
    assert (N + 31) // 32 > cus * 2 * 8
    x, nodes = _dev("unit", N, M, 11)
    want = _plain(x, nodes, K)
    sample = kr.stride_sample(N).cuda()
    _held(("unit", N, M, 11, K), want[sample], x[sample], nodes, K, what="second trip (sample)")
    seeds = _seeds(want, M)
    for sname in ("rolled", "garbage"):
        got = _refine(x, nodes, K, seeds[sname], "mfma")
        assert torch.equal(got, want), (sname, int((got != want).any(1).nonzero()[0]))
    assert torch.equal(_refine(x, nodes, K, seeds["rolled"], "box"), want)


# ---- scenes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kr.SCENES, ids=_id)
def test_scenes_through_all_three_kernels(case):
    """Inputs off the unit box: a scene 64 units from the origin (the matrix-core filter's budget eps = 1e-4 (|x|^2 + max |n|^2)
    against its dropped terms), hyper coordinates that dominate, padding nodes at FAR (|n|^2 = 3e8), exact ties, the trainer's
    storage order.  Exact seed (the filter as tight as it gets) and a stale one (the points moved by 0.01)."""
    name, N, M, D, K = case
    x, nodes = _dev(name, N, M, D)

    def seeds(want):
        return {"exact": want.clone(), "stale": _plain(kr.moved(kr.build(name, N, M, D)[0]).cuda(), nodes, K)}
    want = _all_three(case, seeds=seeds, what="scene")
    if name == "far_pad":
        assert int(want.max()) < M - 8


def test_non_finite_and_overflowing_points_stay_in_range():
    """Rows 24 .. 39 (both sides of a 32-point group seam) hold NaN, +-inf or 3e19 (finite; its square overflows) in a spatial
    or a hyper coordinate: every distance of such a point is NaN or inf, no node fills a slot, and the contract says index 0.
    All three kernels agree bit for bit, every index is in [0, M), and all other rows are those of the clean run.  The indices
    are only read on the host: nothing here hands them to a kernel that would gather with them."""
    name, N, M, D, K = kr.NONFINITE
    clean_x, nodes = _dev(name, N, M, D)
    x = clean_x.clone()
    nan, inf = float("nan"), float("inf")
    edits = [(0, nan), (5, nan), (1, inf), (2, -inf), (0, 3e19), (9, -3e19), (4, inf), (None, nan)]
    for r in range(24, 40):
        col, v = edits[(r - 24) % 8]
        if col is None:
            x[r] = v
        else:
            x[r, col] = v
    clean = _plain(clean_x, nodes, K)
    results = {"plain": _plain(x, nodes, K)}
    for sname, seed in _seeds(clean, M).items():
        for mode in MODES:
            results[mode + "/" + sname] = _refine(x, nodes, K, seed, mode)
    host = {k: v.cpu() for k, v in results.items()}
    want, clean = host["plain"], clean.cpu()
    keep = torch.ones(N, dtype=torch.bool)
    keep[24:40] = False
    for k, v in host.items():
        assert int(v.min()) >= 0 and int(v.max()) < M, (k, int(v.min()), int(v.max()))
        assert torch.equal(v[keep], clean[keep]), k
        assert torch.equal(v, want), (k, v[24:40].tolist())
    assert int(want[24:40].abs().max()) == 0


# ---- refusals and input checks ----------------------------------------------------------------------------------------------
def test_refused_arguments_leave_idx_untouched():
    ops = _ops()
    lib = ops.load()
    dev = torch.device("cuda:0")
    x = torch.rand(64, 17, device=dev)
    x1, x2 = x[:, :3].contiguous(), x[:, 3:].contiguous()
    nodes = torch.rand(2049 * 17, device=dev)
    idx = torch.full((64, 5), -7, dtype=torch.int64, device=dev)
    st = ops._stream(dev)
    xp, x1p, x2p, s2, nd, ip = x.data_ptr(), x1.data_ptr(), x2.data_ptr(), x2.stride(0), nodes.data_ptr(), idx.data_ptr()
    points = lambda N, M, D, K: lib.dgs_knn_points(N, M, D, K, xp, nd, ip, None, st)
    points2 = lambda N, M, D1, D2, K: lib.dgs_knn_points2(N, M, D1, D2, K, x1p, x2p, s2, nd, ip, None, st)
    refine = lambda N, M, D1, D2, K, mode=0: lib.dgs_knn_refine_mode(N, M, D1, D2, K, x1p, x2p, s2, nd, ip, mode, st)
    with torch.cuda.device(dev):
        refused = {
            "K > M": [points(64, 2, 11, 3), points2(64, 2, 3, 8, 3), refine(64, 2, 3, 8, 3), refine(64, 2, 3, 8, 3, 1)],
            "K = 5": [points(64, 100, 11, 5), points2(64, 100, 3, 8, 5), refine(64, 100, 3, 8, 5), refine(64, 100, 3, 8, 5, 1)],
            "D = 17": [points(64, 100, 17, 3), points2(64, 100, 3, 14, 3), refine(64, 100, 3, 14, 3)],
            "D1 = 2 (refine)": [refine(64, 100, 2, 8, 3), refine(64, 100, 2, 8, 3, 1)],
            "M = 2049 (refine)": [refine(64, 2049, 3, 8, 3), refine(64, 2049, 3, 8, 3, 1)],
            "mode = 2": [refine(64, 100, 3, 8, 3, 2), refine(64, 100, 3, 8, 3, -1)],
        }
        empty = [points(0, 100, 11, 3), points2(0, 100, 3, 8, 3), refine(0, 100, 3, 8, 3), refine(0, 100, 3, 8, 3, 1),
                 lib.dgs_knn_refine(0, 100, 3, 8, 3, x1p, x2p, s2, nd, ip, st)]
    torch.cuda.synchronize()
    for what, rcs in refused.items():
        assert all(rc < 0 for rc in rcs), (what, rcs)
    assert empty == [0] * len(empty), empty
    assert bool((idx == -7).all())


def test_knn_indices2_refuses_inputs_it_would_misread():
    """Both branches of _ops.knn_indices2 hand raw pointers and one row stride to the library: a transposed node table, a strided
    x1, an x2 whose columns are not adjacent and anything but float32 are refused, with or without a seed."""
    ops = _ops()
    x, nodes = _dev("unit", 1537, 257, 11)
    x1, x2 = _split(x)
    want = ops.knn_indices2(x1, x2, nodes, 3)
    bad = {
        "transposed nodes": (x1, x2, nodes.t().contiguous().t()),
        "strided x1": (x[:, :3], x2, nodes),
        "x2 with a column stride": (x1, x[:, 3::2][:, :4], nodes),
        "float64 x1": (x1.double(), x2, nodes),
        "float64 nodes": (x1, x2, nodes.double()),
    }
    for what, (a, b, n) in bad.items():
        assert a.shape[0] == x.shape[0] and n.shape[0] == nodes.shape[0]
        for seed in (None, want.clone()):
            with pytest.raises(RuntimeError, match="fp32 row-major"):
                ops.knn_indices2(a, b, n, 3, seed=seed)
            if seed is not None:
                assert torch.equal(seed, want), what
