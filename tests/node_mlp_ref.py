"""Plain-PyTorch reference of the control-node MLP kernels (mlp_pack_kernel, mlp_fwd_kernel, mlp_bwd_kernel, mlp_wgrad_kernel in
csrc/node_mlp.h), written from the formulas: positional encodings, the 13 -> 256 -> 30 time net, eight 256-wide ReLU layers with
the skip concat [input, H4] in front of L5, four linear heads -- and its backward by hand, layer by layer, so that every
intermediate the kernels keep (`saved`, `scratch`) has a counterpart and the ReLU masks can be imposed from outside.  Usable at
any floating-point precision and on any device: float64 is the reference of tests/test_node_mlp_fp64_gpu.py, float32 its
yardstick.  tests/test_node_mlp_ref_cpu.py ties it to DeformMLP.forward + torch.autograd, which the goldens pin against the
original project.  A helper module: no tests in here."""
import contextlib

import torch

W = 256                # hidden width
XCH, TOUT, TCH = 63, 30, 13
IN, IN_PAD, T_PAD, HEADS = 93, 96, 16, 13
FAR = 1.0e4            # where ControlNodes parks its padding nodes (ControlNodes.FAR)
LAYERS = ("T1", "T2", "L0", "L1", "L2", "L3", "L4", "L5", "L6", "L7")
HEAD_NAMES = ("local_rotation", "d_xyz", "d_rotation", "d_scaling")       # the order of _ops.node_mlp_params and of attrs
HEAD_COLS = ((0, 4), (4, 7), (7, 11), (11, 13))
PARAM_NAMES = tuple(n + s for n in LAYERS + HEAD_NAMES for s in (".w", ".b"))
MASK_NAMES = ("t1",) + tuple("h%d" % l for l in range(8))                # the nine ReLU layers: T1, L0..L7
REGIMES = ("init", "spread", "trained")
T_KINDS = ("broadcast", "per_node", "column")


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def build_inputs(M, regime="spread", x_stride=11, t_kind="per_node", far_rows=(), seed=4, rot_bias=(1.0, 0.0, 0.0, 0.0)):
    """Fixed-seed float32 inputs on the CPU: x[M, x_stride] (0.8 randn, first three columns used), t (broadcast: an expanded
    [1, 1]; per_node: [M, 1]; column: column 1 of an [M, 3] tensor), params (the 28 tensors in the order of
    _ops.node_mlp_params), cot[M, 13], rot_bias[4].  far_rows: rows parked at FAR, with zero cotangent rows."""
    from dgs_amd.deform import DeformMLP
    assert regime in REGIMES and t_kind in T_KINDS
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = DeformMLP()
        heads = (net.local_rotation, net.gaussian_warp, net.gaussian_rotation, net.gaussian_scaling)
        with torch.no_grad():
            if regime != "init":
                for head in (net.gaussian_warp, net.gaussian_rotation, net.gaussian_scaling, net.local_rotation):
                    head.weight.normal_(0, 0.05)
                    head.bias.normal_(0, 0.1)
                for lin in list(net.linear) + [net.timenet[0], net.timenet[2]]:
                    lin.bias.normal_(0, 0.05)
            if regime == "trained":
                for head in heads:
                    head.weight.mul_(3e3)
        x = torch.randn(M, x_stride) * 0.8
        if t_kind == "broadcast":
            t = torch.full((1, 1), 0.37).expand(M, 1)
        elif t_kind == "per_node":
            t = torch.rand(M, 1)
        else:
            t = torch.rand(M, 3)[:, 1:2]
        cot = torch.randn(M, HEADS)
    far = list(far_rows)
    if far:
        x[far, :3] = FAR
        cot[far] = 0.0
    mods = [net.timenet[0], net.timenet[2]] + list(net.linear) + list(heads)
    params = []
    for m in mods:
        params += [m.weight.detach().clone(), m.bias.detach().clone()]
    return {"x": x, "t": t, "params": params, "cot": cot, "rot_bias": torch.tensor(rot_bias, dtype=torch.float32)}


def to_device(inp, device):
    """The same inputs on `device`, strides kept (a broadcast t stays stride 0, a column t stride 3)."""
    out = dict(inp)
    t = inp["t"]
    if t.stride(0) == 0:
        out["t"] = t[:1].contiguous().to(device).expand(t.shape[0], 1)
    elif t.stride(0) == 1:
        out["t"] = t.contiguous().to(device)
    else:
        base = torch.zeros(t.shape[0], t.stride(0))
        base[:, 1:2] = t
        out["t"] = base.to(device)[:, 1:2]
    out["x"] = inp["x"].to(device)
    out["params"] = [p.to(device) for p in inp["params"]]
    out["cot"] = inp["cot"].to(device)
    out["rot_bias"] = inp["rot_bias"].to(device)
    return out


# ---- products --------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def exact_matmul():
    """float32 products as float32: TF32 and every reduced-precision GEMM mode off for the span."""
    mm, cd = torch.backends.cuda.matmul, torch.backends.cudnn
    old = (mm.allow_tf32, cd.allow_tf32, mm.allow_fp16_reduced_precision_reduction, mm.allow_bf16_reduced_precision_reduction,
           torch.get_float32_matmul_precision())
    mm.allow_tf32 = cd.allow_tf32 = False
    mm.allow_fp16_reduced_precision_reduction = mm.allow_bf16_reduced_precision_reduction = False
    torch.set_float32_matmul_precision("highest")
    try:
        yield
    finally:
        mm.allow_tf32, cd.allow_tf32, mm.allow_fp16_reduced_precision_reduction, mm.allow_bf16_reduced_precision_reduction = old[:4]
        torch.set_float32_matmul_precision(old[4])


def _mm(a, b):
    with exact_matmul():
        return a @ b


# ---- the stages, one kernel stage each -------------------------------------------------------------------------------------------
def stage_posenc(v32, n_freqs, dtype):
    """[v, sin(2^0 v), cos(2^0 v), ..]: the arguments are the float32 input times 2^k (exact), then converted to `dtype`."""
    assert v32.dtype == torch.float32
    outs = [v32.to(dtype)]
    for k in range(n_freqs):
        a = (v32 * float(2 ** k)).to(dtype)
        outs += [torch.sin(a), torch.cos(a)]
    return torch.cat(outs, -1)


def stage_linear(X, Wt, b, dtype, relu=True):
    """Z = X W^T + b (W as PyTorch stores it, [out][in]), with or without the ReLU."""
    z = _mm(X.to(dtype), Wt.to(dtype).t()) + b.to(dtype)
    return torch.relu(z) if relu else z


def stage_skip(inp, h4, Wt, b, dtype):
    """L5 = ReLU([input | H4] W^T + b): the concatenation order of the original (the kernels hold [H4 | input])."""
    return stage_linear(torch.cat([inp.to(dtype), h4.to(dtype)], -1), Wt, b, dtype)


def stage_heads(h7, params, rot_bias, dtype):
    """attrs[M, 13] = [local_rotation + rot_bias | d_xyz | d_rotation | d_scaling]."""
    out = [stage_linear(h7, params[20 + 2 * h], params[21 + 2 * h], dtype, relu=False) for h in range(4)]
    out[0] = out[0] + rot_bias.to(dtype)
    return torch.cat(out, -1)


def head_matrix(params, dtype):
    """The four head weights as one [13][256] matrix."""
    return torch.cat([params[20 + 2 * h].to(dtype) for h in range(4)], 0)


def stage_dgrad(dz, Wt, mask, dtype, cols=None):
    """dX = (dZ W)[:, cols] * mask: the gradient of a layer's input (mask None: no ReLU in between)."""
    Wd = Wt.to(dtype)
    if cols is not None:
        Wd = Wd[:, cols[0]:cols[1]]
    dx = _mm(dz.to(dtype), Wd)
    return dx if mask is None else dx * mask.to(dtype)


def stage_dt2(dz5, W5, dz0, W0, dtype):
    """The gradient of the time net's output: the time columns of the input as L5 sees it, plus those as L0 sees it."""
    return stage_dgrad(dz5, W5, None, dtype, (XCH, IN)) + stage_dgrad(dz0, W0, None, dtype, (XCH, IN))


def stage_wgrad(dz, X, dtype):
    """dW = dZ^T X, db = sum_m dZ."""
    d = dz.to(dtype)
    return _mm(d.t(), X.to(dtype)), d.sum(0)


# ---- the whole network -----------------------------------------------------------------------------------------------------------
def masks_of(stages):
    """The nine ReLU masks (T1, L0..L7) of a set of post-ReLU activations."""
    return [stages[n] > 0 for n in MASK_NAMES]


def mlp_reference(inp, dtype, masks=None):
    """-> (stages, attrs, grads) at precision `dtype` on the device of inp["x"].
    stages: et[M,13], inp[M,93] (posenc(xyz) 63 | time net 30), t1, h0..h7, dz0..dz7, dt2[M,30], dt1 -- the kernels' names.
    grads: the 28 parameter gradients of sum(attrs * cot), in the order of the parameters.
    masks: None (the backward uses the masks of its own forward), or nine boolean tensors to impose in their place."""
    P = inp["params"]
    x3 = inp["x"][:, :3].float()
    t = inp["t"].float()
    s = {}
    s["et"] = stage_posenc(t, 6, dtype)
    s["t1"] = stage_linear(s["et"], P[0], P[1], dtype)
    t2 = stage_linear(s["t1"], P[2], P[3], dtype, relu=False)
    s["inp"] = torch.cat([stage_posenc(x3, 10, dtype), t2], -1)
    h = s["inp"]
    for l in range(8):
        if l == 5:
            h = stage_skip(s["inp"], h, P[14], P[15], dtype)
        else:
            h = stage_linear(h, P[4 + 2 * l], P[5 + 2 * l], dtype)
        s["h%d" % l] = h
    attrs = stage_heads(s["h7"], P, inp["rot_bias"], dtype)

    m = masks_of(s) if masks is None else list(masks)
    assert len(m) == 9
    mT1, mL = m[0], m[1:]
    g = inp["cot"].to(dtype)
    grads = [None] * 28
    for h_, (lo, hi) in enumerate(HEAD_COLS):
        grads[20 + 2 * h_], grads[21 + 2 * h_] = stage_wgrad(g[:, lo:hi], s["h7"], dtype)
    dz = stage_dgrad(g, head_matrix(P, dtype), mL[7], dtype)
    s["dz7"] = dz
    for l in range(7, 0, -1):
        Wl = P[4 + 2 * l]
        if l == 5:
            X = torch.cat([s["inp"], s["h4"]], -1)
            nxt = stage_dgrad(dz, Wl, mL[4], dtype, (IN, IN + W))
        else:
            X = s["h%d" % (l - 1)]
            nxt = stage_dgrad(dz, Wl, mL[l - 1], dtype)
        grads[4 + 2 * l], grads[5 + 2 * l] = stage_wgrad(dz, X, dtype)
        dz = s["dz%d" % (l - 1)] = nxt
    grads[4], grads[5] = stage_wgrad(s["dz0"], s["inp"], dtype)
    s["dt2"] = stage_dt2(s["dz5"], P[14], s["dz0"], P[4], dtype)
    grads[2], grads[3] = stage_wgrad(s["dt2"], s["t1"], dtype)
    s["dt1"] = stage_dgrad(s["dt2"], P[2], mT1, dtype)
    grads[0], grads[1] = stage_wgrad(s["dt1"], s["et"], dtype)
    return s, attrs, grads


# ---- the buffer layouts of node_mlp.h (floats) -----------------------------------------------------------------------------------
def sv_inp(M):
    return 0                                   # [M][96]: posenc(xyz) 63 | time 30 | 3 zeros


def sv_et(M):
    return M * IN_PAD                          # [M][16]: posenc(t) 13 | 3 zeros


def sv_t1(M):
    return sv_et(M) + M * T_PAD                # [M][256]


def sv_h(M, l):
    return sv_t1(M) + M * W * (1 + l)          # L0..L7 outputs [M][256]


def sv_total(M):
    return sv_h(M, 8)


def sc_dz(M, l):
    return M * W * l                           # dZ of L0..L7 [M][256]


def sc_dt1(M):
    return M * W * 8


def sc_dt2(M):
    return sc_dt1(M) + M * W                   # [M][32]: 30 | 2 zeros


def sc_total(M):
    return sc_dt2(M) + M * 32


def split_saved(saved, M):
    """Views of the `saved` buffer: inp96[M,96], et16[M,16], t1, h0..h7."""
    assert saved.numel() == sv_total(M)
    out = {"inp96": saved[sv_inp(M):sv_et(M)].view(M, IN_PAD), "et16": saved[sv_et(M):sv_t1(M)].view(M, T_PAD),
           "t1": saved[sv_t1(M):sv_h(M, 0)].view(M, W)}
    for l in range(8):
        out["h%d" % l] = saved[sv_h(M, l):sv_h(M, l + 1)].view(M, W)
    return out


def split_scratch(scratch, M):
    """Views of the `scratch` buffer: dz0..dz7, dt1, dt2_32[M,32]."""
    assert scratch.numel() == sc_total(M)
    out = {"dz%d" % l: scratch[sc_dz(M, l):sc_dz(M, l + 1)].view(M, W) for l in range(8)}
    out["dt1"] = scratch[sc_dt1(M):sc_dt2(M)].view(M, W)
    out["dt2_32"] = scratch[sc_dt2(M):sc_total(M)].view(M, 32)
    return out


# ---- what is compared separately -------------------------------------------------------------------------------------------------
def column_groups(name):
    """(label, lo, hi) column ranges of tensor `name` (viewed as [rows, columns]; a bias is one row) whose scales differ."""
    if name == "attrs":
        return [("attrs[%d:%d]" % c, c[0], c[1]) for c in HEAD_COLS]
    if name == "inp":
        return [("inp[0:63]", 0, XCH), ("inp[63:93]", XCH, IN)]
    if name == "L0.w":
        return [("L0.w[0:63]", 0, XCH), ("L0.w[63:93]", XCH, IN)]
    if name == "L5.w":
        return [("L5.w[0:63]", 0, XCH), ("L5.w[63:93]", XCH, IN), ("L5.w[93:349]", IN, IN + W)]
    if name == "T1.w":
        return [("T1.w[0:1]", 0, 1), ("T1.w[1:13]", 1, TCH)]
    return [(name, 0, None)]


def as_rows(name, t):
    """The [rows, columns] view column_groups speaks of."""
    return t.reshape(1, -1) if t.dim() == 1 else t.reshape(t.shape[0], -1)


# ---- the inputs of tests/test_node_mlp_fp64_gpu.py -------------------------------------------------------------------------------
# Every (M, regime, seed, ...) the GPU test runs; tests/test_node_mlp_ref_cpu.py holds each of them to the decided-mask cap.
MASK_CAP = 4
SWEEP_M = (64, 128, 192, 256, 320, 1024, 2048)
BIAS = (0.3, -0.2, 0.5, 0.1)
GPU_CASES = {"M%d" % M: dict(M=M) for M in SWEEP_M}
GPU_CASES.update({"%s%d" % (r, M): dict(M=M, regime=r) for r in ("init", "trained") for M in (64, 320)})
GPU_CASES.update({"x%d_%s" % (xs, tk): dict(M=64, x_stride=xs, t_kind=tk, rot_bias=BIAS) for xs in (3, 11, 16) for tk in T_KINDS})
GPU_CASES.update({"far_group": dict(M=128, far_rows=tuple(range(120, 128))), "far_inside": dict(M=64, far_rows=(3, 59, 60, 61, 62)),
                  "dead_l3": dict(M=64), "zero_l6": dict(M=64), "same_row": dict(M=64)})


def case_inputs(key):
    """build_inputs of GPU_CASES[key] (CPU tensors), with the hand-made changes of the cases that have some."""
    inp = build_inputs(**GPU_CASES[key])
    if key == "dead_l3":
        inp["params"][11].fill_(-100.0)        # L3's bias: the whole layer is dead (the skip concat still feeds L5)
    if key == "zero_l6":
        inp["params"][16].zero_()              # L6's weights and bias: every pre-activation is exactly 0
        inp["params"][17].zero_()
    if key == "same_row":
        inp["x"] = inp["x"][:1].expand(64, -1).contiguous()
        inp["t"] = inp["t"][:1].expand(64, -1).contiguous()
    return inp
