"""-m gpu: the control-node skinning kernels (lbs_fwd_kernel, lbs_bwd_kernel<ASM, COH, HT, FIXED>, their reductions and the fold in
the node MLP's backward) against the float64 reference of tests/skinning_ref.py, over every hyper dimension the C ABI accepts and
every variant of the backward.

Tolerance, per column group g of every compared tensor (skinning_ref.column_groups):
    e_k = max |kernel - ref64|,  e_t = max |ref32 - ref64|  (ref32: the same formulas evaluated in float32 on the same device)
    e_k <= R * e_t + 4 * 2^-24 * max |ref64|   (+ 3 N 2^-45 for the fixed-point table: the quantisation of the contributions)
R is measured, not chosen: twice the largest e_k / e_t observed on an MI355X, rounded up to a power of two, one value for the
forward outputs and one for the gradients.  Groups whose e_k lies within the four-ulp floor alone are left out of the maximum
(their e_t is 0 or a few ulp: pass-through gradients, sigmoid(opacity)).

Largest e_k / e_t per column group over all 55 tests (2306 comparisons; MI355X, ROCm build of this tree):

    group          ratio   case                              e_k        e_t        floor
    attrs[11:13]   2.894   idx=distinct H=13 coherent        1.094e-06  3.781e-07  6.441e-07
    scales         2.477   N=64 M=64 H=13 LDS (= coherent)   1.562e-08  6.305e-09  1.501e-08
    radius         2.158   N=2000 M=3 H=8 coherent           9.775e-06  4.530e-06  1.542e-06
    feature        2.131   sweep H=1 (every variant)         3.144e-06  1.475e-06  2.434e-07
    attrs[0:4]     2.109   sweep H=4 LDS                     6.185e-07  2.933e-07  2.003e-07
    weight         1.956   edge=tiny LDS                     3.342e-07  1.708e-07  7.500e-08
    attrs[7:11]    1.772   N=65 M=64 H=13 LDS                2.735e-07  1.543e-07  2.635e-07
    ntab.hyper     1.676   fused_lbs H=8                     3.267e-06  1.949e-06  9.885e-07
    ntab.radius    1.641   fused_lbs H=8                     1.631e-05  9.937e-06  1.068e-05
    d_rot          1.584   fused_lbs H=13                    8.812e-08  5.563e-08  5.683e-08
    nodes.hyper    1.544   N=3000 M=1122 H=8 LDS             2.979e-06  1.929e-06  7.837e-07
    attrs[4:7]     1.510   sweep H=10 coherent               1.321e-06  8.744e-07  1.155e-06
    rotation       1.096   sweep H=8 LDS                     1.122e-06  1.024e-06  9.248e-07
    ntab.weight    0.993   fused_lbs H=0                     8.549e-07  8.612e-07  4.844e-07
    (means3D, rotations, opacity, d_xyz, d_scale, xyz, scaling, opacity gradients: within the floor everywhere)

Forward outputs: largest 2.477 -> R_FWD = 8.  Gradients: largest 2.894 -> R_GRAD = 8.  No group comes near the 16 that would
have wanted an explanation: kernel and float32 PyTorch differ in summation order (and expf vs exp) only.
Float-atomic tables: the immediate and a deferred reduce of two DIFFERENT backward passes were never bit-equal in the node
gradients (nine of nine hyper dimensions) -- another pass is another order of the float atomics, as include/dgs_train_ops.h says;
so bit-equality of the reduce paths is asserted on ONE pass's sums for the float table and across passes for the fixed-point one.
"""
import functools

import pytest
import torch

import skinning_ref as sr

pytestmark = pytest.mark.gpu

R_FWD = 8.0
R_GRAD = 8.0
EPS32 = 2.0 ** -24
PARAMS = ("xyz", "scaling", "rotation", "opacity", "feature", "nodes", "radius_raw", "weight_raw")
GRAD_OF = {"radius_raw": "radius", "weight_raw": "weight"}
SWEEP_H = (0, 1, 2, 4, 5, 8, 9, 10, 13)


def _ops():
    from dgs_amd import _ops
    return _ops


def _knn(inp, H):
    ops = _ops()
    if H == 0:      # nothing to split off: dgs_knn_points2 wants at least one coordinate in its second array
        return ops.knn_indices(inp["xyz"], inp["nodes"], 3)
    return ops.knn_indices2(inp["xyz"], inp["feature"][:, :H], inp["nodes"], 3)


@functools.lru_cache(maxsize=None)
def _case(N, M, H, fstride=None, mask_kind="sigmoid", idx_kind="knn", edge_points=(), seed=0, lbs=False):
    """(inputs on the GPU, (out64, grad64), (out32, grad32)): built once, shared, never modified."""
    inp = sr.to_device(sr.build_inputs(N, M, H, fstride, mask_kind, idx_kind, edge_points, seed), "cuda")
    if "idx" not in inp:
        inp["idx"] = _knn(inp, H) if N > 0 else torch.zeros((0, 3), dtype=torch.int64, device="cuda")
    if lbs:
        inp["ntab"] = torch.cat([inp["nodes"], torch.exp(inp["radius_raw"])[:, None], torch.sigmoid(inp["weight_raw"])], 1).contiguous()
        inp["cot"] = inp["cot_lbs"]
    r64 = sr.skin_reference(inp, H, torch.float64, not lbs)
    r32 = sr.skin_reference(inp, H, torch.float32, not lbs)
    return inp, r64, r32


def _compare(case, got, r64, r32, H, R, fails, extra=0.0, splits=None):
    """Group by group (and row range by row range of the per-surfel tensors: splits) against the float64 reference; prints every figure."""
    for name, ref in r64.items():
        k2, a2, b2 = (t.reshape(t.shape[0], -1).double() for t in (got[name], ref, r32[name]))
        assert k2.shape == a2.shape, (case, name, tuple(k2.shape), tuple(a2.shape))
        ranges = splits if (splits and name not in sr.NODE_GRADS and name != "ntab") else [(0, a2.shape[0])]
        for label, lo, hi in sr.column_groups(name, H):
            for r0, r1 in ranges:
                k, a, b = k2[r0:r1, lo:hi], a2[r0:r1, lo:hi], b2[r0:r1, lo:hi]
                if a.numel() == 0:
                    continue
                e_k, e_t = float((k - a).abs().max()), float((b - a).abs().max())
                floor = 4 * EPS32 * float(a.abs().max())
                ratio = e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf"))
                print("SKIN %-34s %-14s rows %6d:%-6d e_k %.3e e_t %.3e floor %.3e ratio %8.3f %s"
                      % (case, label, r0, r1, e_k, e_t, floor, ratio, "floor" if e_k <= floor + extra else "R"))
                if not e_k <= R * e_t + floor + extra:
                    fails.append("%s %s rows %d:%d: e_k %.3e > %g * e_t %.3e + %.3e" % (case, label, r0, r1, e_k, R, e_t, floor + extra))


def _table_is_zero(table, fixed):
    return not bool(table.view(torch.int64 if fixed else torch.float32).ne(0).any())


_NET = {}


def _mlp():
    """The node MLP only hosts the fold (dgs_mlp_backward_reduce): its own weight gradients are not looked at here."""
    if "mlp" not in _NET:
        from dgs_amd.deform import DeformMLP
        torch.manual_seed(4)
        net = DeformMLP().cuda()
        for p in net.parameters():
            p.grad = torch.zeros_like(p)
        _NET["mlp"] = _ops().DeferredNodeMLP(net)
    return _NET["mlp"]


def _run(inp, H, variant, sink=False, preset=0.0, tables=None, snapshot=None):
    """One forward + backward of fused_deform.  variant: lds | coh | fixed | later | later_fixed | fold | fold_fixed (the last four:
    coherent with reduce_later, finished through the closure / through the node MLP's backward).  sink: False | True | "store".
    snapshot: dict; the unreduced table of a deferred variant is copied into it ("table") -- or, when it already holds one, the
    table is overwritten with it before the reduction (two finishes of ONE set of float sums).
    -> (out, grad) with the gradients as the kernels left them (a preset is not subtracted)."""
    ops = _ops()
    lib = ops.load()
    coherent, fixed = variant != "lds", variant.endswith("fixed")
    deferred = variant.startswith(("later", "fold"))
    p = {k: inp[k].clone().requires_grad_(True) for k in PARAMS}
    attrs = inp["attrs"].clone().requires_grad_(True)
    N, M = p["xyz"].shape[0], p["nodes"].shape[0]
    if deferred:
        sink = sink or True
    if sink:
        for t in p.values():
            t.grad = torch.full_like(t, preset)
    g_out = torch.full_like(attrs, float("nan")) if deferred else None
    later = [] if deferred else None
    tables = ops.CoherentTables() if tables is None else tables
    table = tables.get(lib, torch.device("cuda", torch.cuda.current_device()), M, H)[1] if coherent else None
    out = ops.fused_deform(*[p[k] for k in PARAMS], attrs, inp["idx"], inp["mask"], H, grad_sink=sink, g_attrs_out=g_out,
                           coherent=coherent, reduce_later=later, tables=tables, fixed=fixed)
    torch.autograd.backward(out, inp["cot"])
    if deferred:
        assert len(later) == 1
        if snapshot is not None:
            if "table" in snapshot:
                table.copy_(snapshot["table"])
            else:
                snapshot["table"] = table.clone()
        if variant.startswith("later"):
            later[0]()
        else:
            mlp = _mlp()
            mlp.forward(p["nodes"].detach(), torch.full((M, 1), 0.37, device="cuda"))
            mlp.backward(g_out, fold=later[0].fold_args)
            later[0].done()
    if coherent:      # the persistent table is left all zero by every way of finishing, and nobody thinks otherwise
        torch.cuda.synchronize()
        assert _table_is_zero(table, fixed), variant
        assert tables.get(lib, table.device, M, H)[1].data_ptr() == table.data_ptr() and not tables._dirty
    grad = {GRAD_OF.get(k, k): t.grad.detach() for k, t in p.items()}
    grad["attrs"] = g_out if deferred else attrs.grad.detach()
    names = ("means3D", "scales", "rotations", "opacity")
    return {n: o.detach() for n, o in zip(names, out)}, grad


def _check(case, inp, r64, r32, H, variant, fails, splits=None, **kw):
    out, grad = _run(inp, H, variant, **kw)
    N = inp["xyz"].shape[0]
    _compare(case + " " + variant, out, r64[0], r32[0], H, R_FWD, fails, splits=splits)
    _compare(case + " " + variant, grad, r64[1], r32[1], H, R_GRAD, fails, extra=3 * N * 2.0 ** -45 if variant.endswith("fixed") else 0.0,
             splits=splits)
    return out, grad


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


# ---- a. every hyper dimension, every variant -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", SWEEP_H)
def test_h_sweep_all_variants(H):
    """load_row's 16-byte / scalar split at T = 3 + H in {3 .. 16}, lbs_combine's column groups (G <= 16, <= 24, > 24 from H = 10),
    the generic coherent kernels (HT = 0: every H but 8), the H-generic reduce and fold."""
    N, M = 1500, 192
    inp, r64, r32 = _case(N, M, H, fstride=H + 3, seed=H)
    ops = _ops()
    fails = []
    case = "sweep H=%d" % H
    _check(case, inp, r64, r32, H, "lds", fails)
    for form in ("coh", "fixed"):
        sfx = "_fixed" if form == "fixed" else ""
        tables = ops.CoherentTables()
        first = _check(case, inp, r64, r32, H, form, fails, tables=tables)
        second = _check(case + " again", inp, r64, r32, H, form, fails, tables=tables)   # a second backward on the same table
        snap = {}
        closure = _check(case, inp, r64, r32, H, "later" + sfx, fails, tables=tables, snapshot=snap)
        fold = _check(case, inp, r64, r32, H, "fold" + sfx, fails, tables=tables, snapshot=snap)
        # the two ways of finishing the deferred reduce, on the same sums: bit for bit (lbs_reduce_raw_kernel vs the fold)
        _same(closure[1], fold[1], "H=%d %s closure vs fold" % (H, form))
        _same(closure[0], fold[0], "H=%d %s closure vs fold (outputs)" % (H, form))
        if form == "fixed":
            # integer atomics are order-free: two runs, and the immediate and both deferred reductions, give the same bits
            _same(first[1], second[1], "H=%d fixed twice" % H)
            _same(first[1], closure[1], "H=%d fixed immediate vs deferred" % H)
        else:
            # float atomics: another backward is another summation order, so the immediate reduce is compared on equal terms only
            # through the reference (above); what the wave sums do not touch is still the same bits
            for k in sr.SURFEL_GRADS:
                assert torch.equal(first[1][k], closure[1][k]), k
            eq = all(torch.equal(first[1][k], closure[1][k]) for k in sr.NODE_GRADS)
            print("SKIN %s float immediate == deferred bitwise: %s" % (case, eq))
    assert not fails, "\n".join(fails)


# ---- g. the neighbour search that feeds the sweep --------------------------------------------------------------------------------
@pytest.mark.parametrize("H", SWEEP_H)
def test_knn_feeding_the_sweep(H):
    """knn_indices2 with D1 = 3, D2 = H and a feature row stride of H + 3 against a float64 brute force, on the points whose four
    nearest float64 distances are separated by more than 1e-5 relative (tests/test_skinning_ref_cpu.py: at most 1 % are not).
    H = 0 has no second array (dgs_knn_points2 rejects D2 = 0): the plain entry point serves it."""
    inp = _case(1500, 192, H, fstride=H + 3, seed=H)[0]
    d2, want = sr.knn_bruteforce(inp["xyz"], inp["feature"], inp["nodes"], H)
    ok = sr.knn_decided(d2)
    assert int((~ok).sum()) <= 15
    assert torch.equal(inp["idx"][ok], want[ok][:, :3])


# ---- b. fused_lbs: the ntab layout, T = 3 + H + 2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [0, 8, 13])
def test_fused_lbs(H):
    N, M = 1500, 192
    inp, r64, r32 = _case(N, M, H, fstride=H + 3, seed=H, lbs=True)
    ops = _ops()
    feature, ntab, attrs = (inp[k].clone().requires_grad_(True) for k in ("feature", "ntab", "attrs"))
    out = ops.fused_lbs(inp["xyz"], feature, inp["idx"], ntab, attrs, inp["mask"], H)
    torch.autograd.backward(out, inp["cot"])
    fails = []
    case = "lbs H=%d" % H
    _compare(case, dict(zip(("d_xyz", "d_rot", "d_scale"), [o.detach() for o in out])), r64[0], r32[0], H, R_FWD, fails)
    _compare(case, {"feature": feature.grad, "ntab": ntab.grad, "attrs": attrs.grad}, r64[1], r32[1], H, R_GRAD, fails)
    assert float(ntab.grad[:, :3].abs().max()) == 0.0 and float(feature.grad[:, H:].abs().max()) == 0.0
    assert not fails, "\n".join(fails)


# ---- c. sizes and index patterns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 13])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_small_sizes(N, H):
    inp, r64, r32 = _case(N, 64, H, seed=N)
    fails = []
    for variant in ("lds", "coh"):
        _check("N=%d M=64 H=%d" % (N, H), inp, r64, r32, H, variant, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H", [8, 13])
def test_three_nodes_overflow_every_bucket(H):
    """M = 3: all 512 threads of a round land on the same three nodes -- kLbsSlots = 4 rows parked, 508 through the overflow
    atomics of lbs_deliver, in every round; lbs_combine reduces one node per wave."""
    inp, r64, r32 = _case(2000, 3, H, seed=3)
    fails = []
    for variant in ("lds", "coh", "fixed"):
        _check("N=2000 M=3 H=%d" % H, inp, r64, r32, H, variant, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H", [8, 13])
@pytest.mark.parametrize("idx_kind", ["same", "distinct"])
def test_hand_made_neighbour_lists(idx_kind, H):
    """(i) every lane of a wave has the same three nodes: one pass of lbs_combine's loop per slot; (ii) all 64 lanes differ in all
    three slots: 64 passes, one selected lane each."""
    inp, r64, r32 = _case(1024, 256, H, idx_kind=idx_kind, seed=5)
    fails = []
    for variant in ("lds", "coh", "fixed"):
        _check("idx=%s H=%d" % (idx_kind, H), inp, r64, r32, H, variant, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("H", [8, 13])
def test_lds_second_round(H):
    """N = 256 * 512 + 7: every workgroup's chunk is 513 points -- the round loop of the LDS variant runs twice, the second round
    with one valid thread (seven workgroups) or none."""
    inp, r64, r32 = _case(256 * 512 + 7, 64, H, seed=7)
    fails = []
    _check("N=131079 M=64 H=%d" % H, inp, r64, r32, H, "lds", fails)
    assert not fails, "\n".join(fails)


def _largest_m(H):
    ops = _ops()
    M = 2048
    while not ops.lbs_supported(M, H):
        M -= 1
    return M


@pytest.mark.parametrize("H", [8, 13])
def test_largest_node_count(H):
    """The largest M whose tables fit the 160 KB of LDS (lbs_bwd_lds_bytes), and one more: refused in backward, nothing written."""
    ops = _ops()
    M = _largest_m(H)
    assert 512 < M < 2048 and ops.lbs_supported(M, H) and not ops.lbs_supported(M + 1, H)
    inp, r64, r32 = _case(3000, M, H, seed=9)
    fails = []
    for variant in ("lds", "coh"):
        _check("N=3000 M=%d H=%d" % (M, H), inp, r64, r32, H, variant, fails)
    assert not fails, "\n".join(fails)
    big = sr.to_device(sr.build_inputs(3000, M + 1, H, seed=9), "cuda")
    big["idx"] = _knn(big, H)
    for coherent in (False, True):
        p = {k: big[k].clone().requires_grad_(True) for k in PARAMS}
        for t in p.values():
            t.grad = torch.full_like(t, 0.5)
        attrs = big["attrs"].clone().requires_grad_(True)
        out = ops.fused_deform(*[p[k] for k in PARAMS], attrs, big["idx"], big["mask"], H, grad_sink=True, coherent=coherent,
                               tables=ops.CoherentTables())
        with pytest.raises(RuntimeError, match="do not fit"):
            torch.autograd.backward(out, big["cot"])
        torch.cuda.synchronize()
        for k, t in p.items():
            assert bool((t.grad == 0.5).all()), k


# ---- d. argument edges ----------------------------------------------------------------------------------------------------------
EDGE = dict(N=700, M=64, H=8)


@pytest.mark.parametrize("mask_kind", ["none", "binary"])
def test_mask_none_and_exact_zero_one(mask_kind):
    N, M, H = EDGE["N"], EDGE["M"], EDGE["H"]
    inp, r64, r32 = _case(N, M, H, mask_kind=mask_kind, seed=11)
    if mask_kind == "none":
        assert inp["mask"] is None
    else:
        assert bool((inp["mask"] == 0).any()) and bool((inp["mask"] == 1).any())
        gone = inp["mask"] == 0
        assert torch.equal(r64[0]["means3D"][gone], inp["xyz"][gone].double())
    fails = []
    for variant in ("lds", "coh", "fixed"):
        _check("mask=%s" % mask_kind, inp, r64, r32, H, variant, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", ["lds", "coh"])
def test_wide_feature_rows_and_gradient_sinks(variant):
    """feature with H + 3 columns: the extra columns of its gradient are 0 when returned, untouched when added in place; add mode
    adds to what is there; store mode (feature exactly H wide) overwrites all of it."""
    N, M, H = EDGE["N"], EDGE["M"], EDGE["H"]
    fails = []
    inp, r64, r32 = _case(N, M, H, fstride=H + 3, seed=12)
    _, grad = _check("fstride=H+3", inp, r64, r32, H, variant, fails)
    assert float(grad["feature"][:, H:].abs().max()) == 0.0
    # add mode: (0.5 + g) - 0.5 carries one rounding of the sum at its own magnitude on top of the kernel's error
    out, grad = _run(inp, H, variant, sink=True, preset=0.5)
    assert bool((grad["feature"][:, H:] == 0.5).all())
    assert bool((grad["nodes"][:, :3] == 0.5).all())          # detached node positions: nothing is added
    got = {k: (g if k == "attrs" else g - 0.5) for k, g in grad.items()}
    got["feature"] = got["feature"].clone()
    got["feature"][:, H:] = 0.0
    got["nodes"] = got["nodes"].clone()
    got["nodes"][:, :3] = 0.0
    for k in got:
        one = {k: got[k]}
        scale = 0.5 + float(r64[1][k].abs().max())
        _compare("add 0.5 " + variant, one, {k: r64[1][k]}, {k: r32[1][k]}, H, R_GRAD, fails, extra=2 * EPS32 * scale)
    # store mode: every element of every gradient is written
    inp, r64, r32 = _case(N, M, H, seed=13)
    _, grad = _check("store over NaN", inp, r64, r32, H, variant, fails, sink="store", preset=float("nan"))
    for k, g in grad.items():
        assert bool(torch.isfinite(g).all()), k
    assert float(grad["nodes"][:, :3].abs().max()) == 0.0
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", ["lds", "coh"])
@pytest.mark.parametrize("edge", ["tiny", "far", "pad"])
def test_degenerate_points(edge, variant):
    """tiny: ten points with rotation = 0 and mask = 0 -- F.normalize's clamp: output 0, gradient g / 1e-12 (compared on their own:
    twelve orders of magnitude above the rest).  far: twenty points 50 units out -- exp(-dist / 2 r^2) underflows, the weights
    fall to the 1e-7 floor.  pad: eight nodes parked at ControlNodes.FAR."""
    N, M, H = EDGE["N"], EDGE["M"], EDGE["H"]
    inp, r64, r32 = _case(N, M, H, mask_kind="binary", edge_points=(edge,), seed=14)
    splits = {"tiny": [(0, 10), (10, N)], "far": [(0, 20), (20, 40), (40, N)], "pad": None}[edge]
    fails = []
    out, grad = _check("edge=%s" % edge, inp, r64, r32, H, variant, fails, splits=splits)
    if edge == "tiny":
        assert float(out["rotations"][:10].abs().max()) == 0.0
        assert float(r64[0]["rotations"][:10].abs().max()) == 0.0
        assert torch.equal(r64[1]["rotation"][:10], inp["cot"][2][:10].double() / 1e-12)
    if edge == "far":
        w = r64[1]["feature"][20:40]
        assert float(w.abs().max()) == 0.0 and float(grad["feature"][20:40].abs().max()) == 0.0
    if edge == "pad":
        assert int(inp["idx"].max()) < M - 8
        assert float(grad["attrs"][-8:].abs().max()) == 0.0 and float(grad["nodes"][-8:].abs().max()) == 0.0
    assert not fails, "\n".join(fails)


# ---- f. an empty surfel set -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["lds", "coh", "fixed", "later"])
def test_no_surfels(variant):
    """N == 0 (the trainer prunes): forward and backward succeed; the node gradients are 0 (store) or untouched (add), g_attrs is
    0, the persistent table stays zero."""
    M, H = 64, 8
    inp = _case(0, M, H, seed=15)[0]
    for sink, preset in (("store", float("nan")), (True, 0.5)) if variant != "later" else ((True, 0.5),):
        out, grad = _run(inp, H, variant, sink=sink, preset=preset)     # (checks the table)
        assert all(o.shape[0] == 0 for o in out.values())
        want = 0.0 if sink == "store" else 0.5
        for k in ("nodes", "radius", "weight"):
            assert bool((grad[k] == want).all()), (k, sink)
        assert bool((grad["attrs"] == 0).all())
    if variant in ("lds", "coh"):
        out, grad = _run(inp, H, variant)
        for k in sr.NODE_GRADS:
            assert bool((grad[k] == 0).all()), k
    if variant == "lds":
        lbs = _case(0, M, H, seed=15, lbs=True)[0]
        feature, ntab, attrs = (lbs[k].clone().requires_grad_(True) for k in ("feature", "ntab", "attrs"))
        o = _ops().fused_lbs(lbs["xyz"], feature, lbs["idx"], ntab, attrs, lbs["mask"], H)
        torch.autograd.backward(o, lbs["cot"])
        assert bool((ntab.grad == 0).all()) and bool((attrs.grad == 0).all())
