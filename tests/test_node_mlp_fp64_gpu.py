"""-m gpu: the control-node MLP kernels (mlp_pack_kernel, mlp_fwd_kernel, mlp_bwd_kernel, mlp_wgrad_kernel of csrc/node_mlp.h)
against the float64 reference of tests/node_mlp_ref.py: stage by stage on the kernels' own intermediate buffers, and end to end.

The C ABI (dgs_mlp_forward / dgs_mlp_backward) is called with buffers the test owns -- packed, saved, scratch, attrs, the 28
gradients -- every one filled with NaN before the call: an element that is read before it is written, or promised and never
written, shows as NaN.  _ops.DeferredNodeMLP and _ops.fused_node_mlp (the trainer's paths) run next to it on the same inputs
and must give the same bits.

Tolerance, per column group g of every compared tensor (node_mlp_ref.column_groups):
    e_k = max |kernel - ref64|,  e_t = max |ref32 - ref64|  (ref32: the same function in float32 on the same device and inputs)
    e_k <= R * e_t + 4 * 2^-24 * max |ref64|
R is measured, not chosen: twice the largest e_k / e_t observed on an MI355X over the groups whose e_k exceeds the four-ulp
floor, rounded up to a power of two; one value for forward quantities, one for gradients.

Largest e_k / e_t per column group over all 37 tests (3730 comparisons; MI355X, ROCm build of this tree), stage = one kernel stage
from the kernel's own previous buffer, e2e = the whole network; groups whose e_k lies within the four-ulp floor are left out:

    group              ratio   case                     e_k        e_t        floor
    local_rotation.b   7.472   M=320 (stage = e2e)      9.089e-06  1.216e-06  4.533e-06
    d_xyz.b            6.108   M=2048 (stage = e2e)     1.983e-05  3.247e-06  1.213e-05
    T2.b               5.768   M=1024 stage             9.493e-06  1.646e-06  5.220e-06
    L4.b               5.746   M=2048 stage             1.722e-05  2.998e-06  4.914e-06
    L6.b               5.257   M=2048 stage             1.285e-05  2.444e-06  5.651e-06
    L0.b               4.467   M=2048 stage             8.764e-06  1.962e-06  3.130e-06
    d_rotation.b       4.313   M=1024 (stage = e2e)     1.155e-05  2.678e-06  5.851e-06
    L7.b               3.975   M=2048 stage             1.185e-05  2.981e-06  7.076e-06
    L2.b               3.871   M=2048 stage             8.900e-06  2.299e-06  4.885e-06
    d_scaling.b        3.738   M=320 (stage = e2e)      4.324e-06  1.157e-06  2.063e-06
    T1.b               3.673   M=2048 stage             4.451e-06  1.212e-06  1.671e-06
    L1.b               3.283   M=2048 stage             1.059e-05  3.225e-06  3.895e-06
    L3.b               2.707   M=2048 stage             8.641e-06  3.193e-06  4.633e-06
    L5.b               2.504   M=2048 stage             9.985e-06  3.987e-06  5.860e-06
    T1.w[1:13]         1.316   M=2048 e2e               4.836e-06  3.676e-06  1.717e-06
    d_scaling.w        1.260   M=2048 e2e               1.218e-04  9.666e-05  2.794e-05
    d_xyz.w            1.114   M=1024 stage             2.947e-05  2.647e-05  1.786e-05
    T1.w[0:1]          1.076   M=2048 e2e               2.250e-06  2.091e-06  8.006e-07
    T2.w               1.034   head d_scaling e2e       8.145e-07  7.876e-07  4.976e-07
    attrs[4:7]         0.998   xs=16 t=per_node e2e     7.316e-07  7.334e-07  3.110e-07
    attrs[11:13]       0.916   far_inside e2e           1.024e-03  1.117e-03  2.167e-04
    attrs[7:11]        0.862   xs=16 t=column e2e       5.958e-07  6.911e-07  3.634e-07
    attrs[0:4]         0.837   M=256 e2e                7.710e-07  9.212e-07  3.746e-07
    h7                 0.694   far_inside stage         1.638e-03  2.359e-03  1.250e-03
    h0                 0.640   far_inside stage         1.777e-03  2.779e-03  1.517e-03
    h5                 0.595   M=256 stage              1.038e-06  1.744e-06  8.672e-07
    (every other weight gradient and dz3: below 1; et, inp, t1, the other h and dz, dt1, dt2: within the floor everywhere)

Forward quantities: largest 0.998 -> R_FWD = 2.  Gradients: largest 7.472 -> R_GRAD = 16.  No group reaches the 16 that would
want an explanation; the fourteen largest are the fourteen bias gradients: mlp_wgrad_kernel adds a wave's M / 4 rows of dZ one
after the other into one float (bsum), PyTorch's sum is pairwise -- summation order, growing with M.
ReLU masks: in all 37 tests the kernel's masks were the float64 reference's own (0 units differ).  Padding nodes: the gradients
were bit-equal to those of the same call with the rows at ordinary places (the kernels multiply by the zero dZ).
No case of this file has exposed a bug in the kernels.
"""
import ctypes
import functools

import pytest
import torch

import node_mlp_ref as nr

pytestmark = pytest.mark.gpu

R_FWD = 2.0
R_GRAD = 16.0
EPS32 = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
NAN = float("nan")


def _ops():
    from dgs_amd import _ops
    return _ops


# ---- the kernels through the C ABI, on buffers of the test's own -------------------------------------------------------------------
def _nan(n):
    return torch.full((int(n),), NAN, dtype=F32, device="cuda")


def _ptrs(tensors):
    return (ctypes.c_void_p * 28)(*[t.data_ptr() for t in tensors])


def _rb(inp, null_bias):
    return None if null_bias else (ctypes.c_float * 4)(*[float(v) for v in inp["rot_bias"].cpu()])


def _forward(inp, null_bias=False, select=None):
    """dgs_mlp_forward (or _select) over NaN-filled packed / saved / attrs."""
    ops = _ops()
    lib = ops.load()
    M = inp["x"].shape[0]
    dev = inp["x"].device
    out = {"packed": _nan(lib.dgs_mlp_packed_floats()), "saved": _nan(lib.dgs_mlp_saved_floats(M)), "attrs": _nan(M * 13).view(M, 13)}
    assert out["saved"].numel() == nr.sv_total(M)
    x, t = inp["x"], inp["t"]
    args = (M, x.data_ptr(), x.stride(0), t.data_ptr(), t.stride(0), _ptrs(inp["params"]), _rb(inp, null_bias),
            out["packed"].data_ptr(), out["saved"].data_ptr(), out["attrs"].data_ptr())
    with torch.cuda.device(dev):
        if select is None:
            rc = lib.dgs_mlp_forward(*args, ops._stream(dev))
        else:
            table, counter, override, stride, offset, row_out = select
            rc = lib.dgs_mlp_forward_select(*args, table.data_ptr(), table.shape[0], table.shape[1], counter.data_ptr(),
                                            override.data_ptr(), stride, offset, row_out.data_ptr(), ops._stream(dev))
    assert rc == 0, lib.dgs_train_ops_last_error()
    return out


def _preset(inp, seed=9):
    """Fixed-seed random gradient buffers for the add mode (not a constant: a sum added to the wrong element shows)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g).cuda() for p in inp["params"]]


def _backward(inp, fwd, preset=None):
    """dgs_mlp_backward over a NaN-filled scratch; store mode over NaN-filled gradients, add mode over clones of `preset`."""
    ops = _ops()
    lib = ops.load()
    M = inp["x"].shape[0]
    dev = inp["x"].device
    scratch = _nan(lib.dgs_mlp_scratch_floats(M))
    assert scratch.numel() == nr.sc_total(M)
    grads = [torch.full_like(p, NAN) for p in inp["params"]] if preset is None else [g.clone() for g in preset]
    cot = inp["cot"].contiguous()
    with torch.cuda.device(dev):
        rc = lib.dgs_mlp_backward(M, cot.data_ptr(), fwd["packed"].data_ptr(), fwd["saved"].data_ptr(), scratch.data_ptr(), _ptrs(grads),
                                  0 if preset is None else 1, ops._stream(dev))
    assert rc == 0, lib.dgs_train_ops_last_error()
    return {"scratch": scratch, "grads": grads}


def _net(inp):
    from dgs_amd.deform import DeformMLP
    net = DeformMLP().cuda()
    params = _ops().node_mlp_params(net)
    with torch.no_grad():
        for p, v in zip(params, inp["params"]):
            p.copy_(v)
    return net, params


def _trainer_paths(case, inp, fwd, bwd, preset, null_bias):
    """_ops.DeferredNodeMLP and _ops.fused_node_mlp on the same inputs: the same bits as the C ABI calls."""
    ops = _ops()
    net, params = _net(inp)
    rb = (0.0, 0.0, 0.0, 0.0) if null_bias else tuple(float(v) for v in inp["rot_bias"].cpu())
    for p, g in zip(params, preset if preset is not None else [torch.full_like(p, NAN) for p in params]):
        p.grad = g.clone()
    d = ops.DeferredNodeMLP(net)
    attrs = d.forward(inp["x"], inp["t"], rot_bias=rb)
    assert torch.equal(attrs, fwd["attrs"]), case + ": DeferredNodeMLP attrs"
    d.backward(inp["cot"].contiguous(), store=preset is None)
    for n, p, g in zip(nr.PARAM_NAMES, params, bwd["grads"]):
        assert torch.equal(p.grad, g), "%s: DeferredNodeMLP %s" % (case, n)
    for p in params:
        p.grad = None
    if preset is not None:
        for p, g in zip(params, preset):
            p.grad = g.clone()
    attrs = ops.fused_node_mlp(net, inp["x"], inp["t"], rot_bias=rb, grad_sink=preset is not None)
    assert torch.equal(attrs.detach(), fwd["attrs"]), case + ": fused_node_mlp attrs"
    (attrs * inp["cot"]).sum().backward()      # the cotangent autograd hands the kernel is inp["cot"] itself
    for n, p, g in zip(nr.PARAM_NAMES, params, bwd["grads"]):
        assert torch.equal(p.grad, g), "%s: fused_node_mlp %s" % (case, n)


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
def _cmp(case, name, got, r64, r32, R, fails, extra=0.0, what=""):
    """Column group by column group against the float64 reference; prints every figure."""
    k2, a2, b2 = (nr.as_rows(name, t).double() for t in (got, r64, r32))
    assert k2.shape == a2.shape == b2.shape, (case, name, tuple(k2.shape), tuple(a2.shape))
    for label, lo, hi in nr.column_groups(name):
        k, a, b = k2[:, lo:hi], a2[:, lo:hi], b2[:, lo:hi]
        e_k, e_t = float((k - a).abs().max()), float((b - a).abs().max())
        floor = 4 * EPS32 * float(a.abs().max())
        ratio = e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf"))
        print("MLP %-22s %-6s %-17s e_k %.3e e_t %.3e floor %.3e ratio %8.3f %s"
              % (case, what, label, e_k, e_t, floor, ratio, "floor" if e_k <= floor + extra else "R"))
        if not e_k <= R * e_t + floor + extra:      # (a NaN in e_k fails here)
            fails.append("%s %s %s: e_k %.3e > %g * e_t %.3e + %.3e" % (case, what, label, e_k, R, e_t, floor + extra))


def _stage(case, name, got, fn, fails, R, extra=0.0):
    """One kernel stage: fn(dtype) evaluates it from the kernel's own previous buffers."""
    _cmp(case, name, got, fn(F64), fn(F32), R, fails, extra=extra, what="stage")


def _zero(t, what):
    assert bool((t == 0).all()), what + ": not exactly 0"


def _check(case, inp, preset=None, null_bias=False):
    """Forward + backward through the C ABI and checks 1 (stage by stage), 2 (end to end) and 3 (finiteness) of the module docstring.
    -> (fwd, bwd, views of saved, views of scratch)"""
    fails = []
    M = inp["x"].shape[0]
    P = inp["params"]
    fwd = _forward(inp, null_bias=null_bias)
    bwd = _backward(inp, fwd, preset=preset)
    torch.cuda.synchronize()
    sv, sc = nr.split_saved(fwd["saved"], M), nr.split_scratch(bwd["scratch"], M)
    # 3. nothing is NaN or Inf anywhere: every element of every buffer was written
    for n, t in [("packed", fwd["packed"]), ("saved", fwd["saved"]), ("attrs", fwd["attrs"]), ("scratch", bwd["scratch"])] \
            + list(zip(nr.PARAM_NAMES, bwd["grads"])):
        assert bool(torch.isfinite(t).all()), "%s: %s holds %d non-finite elements" % (case, n, int((~torch.isfinite(t)).sum()))
    rot = torch.zeros(4, device="cuda") if null_bias else inp["rot_bias"]
    inp = dict(inp, rot_bias=rot)

    # 1. stage by stage, forward: each stage from the kernel's own previous buffer
    x3, t = inp["x"][:, :3].float(), inp["t"].float()
    k_et, k_inp = sv["et16"][:, :13], sv["inp96"][:, :93]
    _zero(sv["et16"][:, 13:], case + " saved et columns 13..15")
    _zero(sv["inp96"][:, 93:], case + " saved input columns 93..95")
    _stage(case, "et", k_et, lambda d: nr.stage_posenc(t, 6, d), fails, R_FWD)
    _stage(case, "inp", k_inp, lambda d: torch.cat([nr.stage_posenc(x3, 10, d), nr.stage_linear(sv["t1"], P[2], P[3], d, relu=False)], -1),
           fails, R_FWD)
    _stage(case, "t1", sv["t1"], lambda d: nr.stage_linear(k_et, P[0], P[1], d), fails, R_FWD)
    for l in range(8):
        if l == 5:
            fn = lambda d: nr.stage_skip(k_inp, sv["h4"], P[14], P[15], d)
        else:
            src = k_inp if l == 0 else sv["h%d" % (l - 1)]
            fn = lambda d, src=src, l=l: nr.stage_linear(src, P[4 + 2 * l], P[5 + 2 * l], d)
        _stage(case, "h%d" % l, sv["h%d" % l], fn, fails, R_FWD)
    _stage(case, "attrs", fwd["attrs"], lambda d: nr.stage_heads(sv["h7"], P, rot, d), fails, R_FWD)

    # backward: the masks are the kernel's own saved activations
    km = [sv[n] > 0 for n in nr.MASK_NAMES]
    cot = inp["cot"]
    _stage(case, "dz7", sc["dz7"], lambda d: nr.stage_dgrad(cot, nr.head_matrix(P, d), km[8], d), fails, R_GRAD)
    for l in range(7, 0, -1):
        cols = (nr.IN, nr.IN + nr.W) if l == 5 else None
        _stage(case, "dz%d" % (l - 1), sc["dz%d" % (l - 1)],
               lambda d, l=l, cols=cols: nr.stage_dgrad(sc["dz%d" % l], P[4 + 2 * l], km[l], d, cols), fails, R_GRAD)
    k_dt2 = sc["dt2_32"][:, :30]
    _zero(sc["dt2_32"][:, 30:], case + " scratch dt2 columns 30, 31")
    _stage(case, "dt2", k_dt2, lambda d: nr.stage_dt2(sc["dz5"], P[14], sc["dz0"], P[4], d), fails, R_GRAD)
    _stage(case, "dt1", sc["dt1"], lambda d: nr.stage_dgrad(k_dt2, P[2], km[0], d), fails, R_GRAD)

    # weight gradients: every one of the 28 tensors from the kernel's own dZ and X
    got = bwd["grads"] if preset is None else [g.double() - p.double() for g, p in zip(bwd["grads"], preset)]
    extra = [0.0] * 28 if preset is None else [EPS32 * float(p.abs().max()) for p in preset]
    srcs = [(sc["dt1"], k_et), (k_dt2, sv["t1"]), (sc["dz0"], k_inp)]
    srcs += [(sc["dz%d" % l], torch.cat([k_inp, sv["h4"]], -1) if l == 5 else sv["h%d" % (l - 1)]) for l in range(1, 8)]
    srcs += [(cot[:, lo:hi], sv["h7"]) for lo, hi in nr.HEAD_COLS]
    for i, (dz, X) in enumerate(srcs):
        for j in (0, 1):
            _stage(case, nr.PARAM_NAMES[2 * i + j], got[2 * i + j], lambda d, dz=dz, X=X, j=j: nr.stage_wgrad(dz, X, d)[j], fails, R_GRAD,
                   extra=extra[2 * i + j])

    # 2. end to end, with the kernel's masks imposed on the reference's backward
    s64, a64, g64 = nr.mlp_reference(inp, F64, masks=km)
    s32, a32, g32 = nr.mlp_reference(inp, F32, masks=km)
    _cmp(case, "attrs", fwd["attrs"], a64, a32, R_FWD, fails, what="e2e")
    for i, n in enumerate(nr.PARAM_NAMES):
        _cmp(case, n, got[i], g64[i], g32[i], R_GRAD, fails, extra=extra[i], what="e2e")
    differ = 0
    for n, k in zip(nr.MASK_NAMES, km):
        own = s64[n] > 0
        bad = k != own
        differ += int(bad.sum())
        if bool(bad.any()):      # an undecided unit: both activations lie within the layer's forward tolerance of zero
            e_t = float((s32[n].double() - s64[n]).abs().max())
            tol = R_FWD * e_t + 4 * EPS32 * float(s64[n].abs().max())
            worst = float(torch.maximum(sv[n].double(), s64[n])[bad].max())
            print("MLP %-22s masks  %-17s %d differ, activation <= %.3e, tolerance %.3e" % (case, n, int(bad.sum()), worst, tol))
            if not worst <= tol:
                fails.append("%s mask %s: a unit with activation %.3e > %.3e differs" % (case, n, worst, tol))
    print("MLP %-22s masks  %d of %d differ from the float64 reference's own" % (case, differ, 9 * 256 * M))
    if differ > nr.MASK_CAP:
        fails.append("%s: %d masks differ from the float64 reference's own (cap %d)" % (case, differ, nr.MASK_CAP))
    assert not fails, "\n".join(fails)
    _trainer_paths(case, inp, fwd, bwd, preset, null_bias)
    return fwd, bwd, sv, sc


@functools.lru_cache(maxsize=None)
def _case(key):
    """The inputs of node_mlp_ref.GPU_CASES[key] on the GPU: built once, shared, never modified."""
    return nr.to_device(nr.case_inputs(key), "cuda")


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", nr.SWEEP_M)
def test_row_count_sweep(M):
    """Every shape of mlp_wgrad_kernel's tail (rows = M / 4 per wave, phases of 32 rows in two register sets): half a phase (64),
    one phase (128), one and a half (192), a full trip (256), a partial second trip (320), the production size and one above."""
    _check("M=%d" % M, _case("M%d" % M))


@pytest.mark.parametrize("M", [64, 320])
@pytest.mark.parametrize("regime", ["init", "trained"])
def test_regimes(regime, M):
    """init: the heads as constructed (std 1e-4, 1e-5, 1e-5, 1e-8, zero biases) -- each head is a column group of its own."""
    _check("%s M=%d" % (regime, M), _case("%s%d" % (regime, M)))


@pytest.mark.parametrize("head", range(4))
def test_one_head_at_a_time(head):
    """The cotangent lives in one head's columns: dz7 and that head's gradients against their own scale; the other heads get
    exactly nothing."""
    base = _case("M64")
    lo, hi = nr.HEAD_COLS[head]
    cot = torch.zeros_like(base["cot"])
    cot[:, lo:hi] = base["cot"][:, lo:hi]
    fwd, bwd, sv, sc = _check("head %s" % nr.HEAD_NAMES[head], dict(base, cot=cot))
    assert float(sc["dz7"].abs().max()) > 0
    for h in range(4):
        if h != head:
            _zero(bwd["grads"][20 + 2 * h], "%s.w with the cotangent in %s" % (nr.HEAD_NAMES[h], nr.HEAD_NAMES[head]))
            _zero(bwd["grads"][21 + 2 * h], "%s.b with the cotangent in %s" % (nr.HEAD_NAMES[h], nr.HEAD_NAMES[head]))
        else:
            assert float(bwd["grads"][20 + 2 * h].abs().max()) > 0 and float(bwd["grads"][21 + 2 * h].abs().min()) > 0


@pytest.mark.parametrize("M", [64, 320])
def test_add_mode(M):
    """accumulate = 1 over fixed-seed random gradient buffers: result - preset within the tolerance plus 2^-24 of the preset's
    magnitude (the rounding of the one addition); the store-mode result over NaN is what test_row_count_sweep holds."""
    inp = _case("M%d" % M)
    _check("add M=%d" % M, inp, preset=_preset(inp))


@pytest.mark.parametrize("t_kind", nr.T_KINDS)
@pytest.mark.parametrize("x_stride", [3, 11, 16])
def test_strides_and_rot_bias(x_stride, t_kind):
    """x_stride 3, 11, 16 x t_stride 0, 1, 3, rot_bias = (0.3, -0.2, 0.5, 0.1); and rot_bias = NULL, which means zeros."""
    inp = _case("x%d_%s" % (x_stride, t_kind))
    assert inp["x"].stride(0) == x_stride and inp["t"].stride(0) == {"broadcast": 0, "per_node": 1, "column": 3}[t_kind]
    case = "xs=%d t=%s" % (x_stride, t_kind)
    with_bias = _check(case, inp)[0]
    null = _check(case + " NULL", inp, null_bias=True)[0]
    assert torch.equal(null["attrs"][:, 4:], with_bias["attrs"][:, 4:]) and torch.equal(null["saved"], with_bias["saved"])
    assert not torch.equal(null["attrs"][:, :4], with_bias["attrs"][:, :4])


@pytest.mark.parametrize("key", ["far_group", "far_inside"])
def test_padding_nodes(key):
    """Rows parked at ControlNodes.FAR with zero cotangent rows -- a whole workgroup (120..127 of 128), and rows inside
    workgroups that straddle the MFMA row groups (3, 59..62 of 64): everything finite, the far rows' attrs compared like any
    others, and the 28 gradients those of the same call with the rows at ordinary places."""
    inp = _case(key)
    far = list(nr.GPU_CASES[key]["far_rows"])
    assert float(inp["x"][far, :3].min()) == nr.FAR and float(inp["cot"][far].abs().max()) == 0.0
    fwd, bwd, sv, sc = _check(key, inp)
    for n in ["dz%d" % l for l in range(8)] + ["dt1", "dt2_32"]:
        _zero(sc[n][far], "%s %s of the far rows" % (key, n))
    near = dict(inp, x=inp["x"].clone())
    near["x"][far, :3] = torch.tensor([0.3, -0.5, 0.7], device="cuda")
    bwd2 = _backward(near, _forward(near))
    g64 = nr.mlp_reference(inp, F64, masks=[sv[n] > 0 for n in nr.MASK_NAMES])[2]
    bitwise = True
    for n, a, b, r in zip(nr.PARAM_NAMES, bwd["grads"], bwd2["grads"], g64):
        bitwise = bitwise and torch.equal(a, b)
        assert float((a - b).abs().max()) <= 4 * EPS32 * float(r.abs().max()), n
    print("MLP %-22s far rows against rows at ordinary places: gradients bit-equal: %s" % (key, bitwise))


def test_dead_layer():
    """L3's bias at -100: h3 is 0, dz3 and everything below it on that path exactly 0 (L0..L3 and L4's weights get exactly 0);
    the skip concat still carries gradient from L5 to the input, i.e. to the time net."""
    fwd, bwd, sv, sc = _check("dead L3", _case("dead_l3"))
    _zero(sv["h3"], "h3")
    for l in range(4):
        _zero(sc["dz%d" % l], "dz%d" % l)
        _zero(bwd["grads"][4 + 2 * l], "L%d.w" % l)
        _zero(bwd["grads"][5 + 2 * l], "L%d.b" % l)
    _zero(bwd["grads"][12], "L4.w")
    assert float(sc["dz4"].abs().max()) > 0 and float(sc["dt2_32"].abs().max()) > 0
    for i in range(4):
        assert float(bwd["grads"][i].abs().max()) > 0, nr.PARAM_NAMES[i]


def test_exact_zero_pre_activations():
    """L6's weights and bias 0: every pre-activation of the layer is exactly 0, and with a mask of `> 0` dz6 is exactly 0, as in
    PyTorch (relu'(0) = 0) -- nothing flows below the heads' own layer."""
    fwd, bwd, sv, sc = _check("zero L6", _case("zero_l6"))
    _zero(sv["h6"], "h6")
    for l in range(7):
        _zero(sc["dz%d" % l], "dz%d" % l)
    _zero(sc["dt1"], "dt1")
    _zero(sc["dt2_32"], "dt2")
    for i in range(19):      # .. L7.w = dz7^T h6
        _zero(bwd["grads"][i], nr.PARAM_NAMES[i])
    assert float(sc["dz7"].abs().max()) > 0 and float(bwd["grads"][19].abs().max()) > 0      # L7.b


def test_same_row_everywhere():
    """All 64 rows the same node and time: each output element is the same chain of operations on the same operands whatever
    row slot (workgroup, MFMA row group, register) it sits in -- every row of attrs and of every saved layer is row 0's bits."""
    inp = _case("same_row")
    fwd, bwd, sv, sc = _check("same row", inp)
    for n, t in list(sv.items()) + [("attrs", fwd["attrs"])]:
        assert torch.equal(t, t[:1].expand_as(t)), n


def test_determinism():
    """No atomics, fixed order (the header's promise): two runs give the same bits in every buffer."""
    inp = _case("M320")
    runs = []
    for _ in range(2):
        fwd = _forward(inp)
        bwd = _backward(inp, fwd)
        runs.append([fwd["packed"], fwd["saved"], fwd["attrs"], bwd["scratch"]] + bwd["grads"])
    names = ["packed", "saved", "attrs", "scratch"] + list(nr.PARAM_NAMES)
    for n, a, b in zip(names, *runs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), n


def test_select_rider():
    """dgs_mlp_forward_select: the pack launch's extra workgroup picks the step's view -- row (counter * stride + offset) mod
    nrows, or the override word (then reset to -1); counter += 1 -- and the MLP's own outputs are dgs_mlp_forward's bits."""
    inp = _case("M64")
    plain = _forward(inp)
    V, F = 5, 7
    table = torch.arange(V * F, dtype=F32, device="cuda").view(V, F) + 0.5
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    override = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    stride, offset = 2, 1                      # world size 2, rank 1
    for step, forced in enumerate([None, None, 3, None, 9, None]):
        if forced is not None:
            override.fill_(forced)
        row_out = torch.full((F,), NAN, device="cuda")
        got = _forward(inp, select=(table, counter, override, stride, offset, row_out))
        want = forced % V if forced is not None else (step * stride + offset) % V
        assert torch.equal(row_out, table[want]), (step, row_out)
        assert int(counter.item()) == step + 1 and int(override.item()) == -1
        for n in ("packed", "saved", "attrs"):
            assert torch.equal(got[n], plain[n]), n


@pytest.mark.parametrize("M", [0, 63, 96])
def test_bad_row_counts_are_refused(M):
    """M = 0, 63, 96: -1 from both entry points, nothing launched (the NaN-filled buffers stay NaN)."""
    ops = _ops()
    lib = ops.load()
    inp = _case("M128")
    bufs = [_nan(lib.dgs_mlp_packed_floats()), _nan(nr.sv_total(128)), _nan(128 * 13), _nan(nr.sc_total(128))]
    grads = [torch.full_like(p, NAN) for p in inp["params"]]
    dev = inp["x"].device
    x, t, cot = inp["x"], inp["t"], inp["cot"]
    with torch.cuda.device(dev):
        assert lib.dgs_mlp_forward(M, x.data_ptr(), x.stride(0), t.data_ptr(), t.stride(0), _ptrs(inp["params"]), None, bufs[0].data_ptr(),
                                   bufs[1].data_ptr(), bufs[2].data_ptr(), ops._stream(dev)) == -1
        assert lib.dgs_mlp_backward(M, cot.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[3].data_ptr(), _ptrs(grads), 0,
                                    ops._stream(dev)) == -1
    torch.cuda.synchronize()
    for b in bufs + grads:
        assert bool(torch.isnan(b).all())


def test_null_pointers_are_refused():
    ops = _ops()
    lib = ops.load()
    inp = _case("M64")
    M = 64
    bufs = [_nan(lib.dgs_mlp_packed_floats()), _nan(nr.sv_total(M)), _nan(M * 13), _nan(nr.sc_total(M))]
    grads = [torch.full_like(p, NAN) for p in inp["params"]]
    dev = inp["x"].device
    x, t, cot = inp["x"], inp["t"], inp["cot"]
    fargs = [x.data_ptr(), t.data_ptr(), _ptrs(inp["params"]), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr()]
    bargs = [cot.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[3].data_ptr(), _ptrs(grads)]
    with torch.cuda.device(dev):
        for i in range(len(fargs)):
            a = list(fargs)
            a[i] = None
            assert lib.dgs_mlp_forward(M, a[0], x.stride(0), a[1], t.stride(0), a[2], None, a[3], a[4], a[5], ops._stream(dev)) == -1, i
        for i in range(len(bargs)):
            a = list(bargs)
            a[i] = None
            assert lib.dgs_mlp_backward(M, a[0], a[1], a[2], a[3], a[4], 0, ops._stream(dev)) == -1, i
    torch.cuda.synchronize()
    for b in bufs + grads:
        assert bool(torch.isnan(b).all())
