"""The float64 reference of tests/test_node_mlp_fp64_gpu.py (tests/node_mlp_ref.py) against DeformMLP.forward + torch.autograd,
its per-stage functions against its whole, and the two properties of the GPU test's inputs that the GPU test relies on: ReLU
masks that float32 and float64 agree on (the cap of node_mlp_ref.MASK_CAP differing units), and padding nodes at
ControlNodes.FAR that stay finite and leave every gradient untouched.  No GPU."""
import functools

import pytest
import torch

import node_mlp_ref as nr


@functools.lru_cache(maxsize=None)
def _ref(key, dtype=torch.float64):
    """(inputs, stages, attrs, grads) of a GPU case: computed once, shared, never modified."""
    inp = nr.case_inputs(key)
    return (inp,) + nr.mlp_reference(inp, dtype)


def _rel(got, want, name, tol, fails):
    for label, lo, hi in nr.column_groups(name):
        g, w = nr.as_rows(name, got)[:, lo:hi], nr.as_rows(name, want)[:, lo:hi]
        err, scale = float((g - w).abs().max()), float(w.abs().max())
        if not err <= tol * scale:
            fails.append("%s: err %.3e scale %.3e" % (label, err, scale))


@pytest.mark.parametrize("t_kind", nr.T_KINDS)
@pytest.mark.parametrize("regime", nr.REGIMES)
def test_reference_matches_autograd(regime, t_kind):
    """mlp_reference(float64) = DeformMLP().double() + torch.autograd to 1e-11 of every column group's own scale."""
    from dgs_amd.deform import DeformMLP
    inp = nr.build_inputs(64, regime, 11, t_kind, seed=4, rot_bias=nr.BIAS)
    assert inp["t"].stride(0) == {"broadcast": 0, "per_node": 1, "column": 3}[t_kind]
    net = DeformMLP().double()
    mods = [net.timenet[0], net.timenet[2]] + list(net.linear) + [net.local_rotation, net.gaussian_warp, net.gaussian_rotation,
                                                                 net.gaussian_scaling]
    with torch.no_grad():
        for i, m in enumerate(mods):
            m.weight.copy_(inp["params"][2 * i])
            m.bias.copy_(inp["params"][2 * i + 1])
    o = net(inp["x"][:, :3].double(), inp["t"].double())
    want = torch.cat([o["local_rotation"] + inp["rot_bias"].double(), o["d_xyz"], o["d_rotation"], o["d_scaling"]], -1)
    (want * inp["cot"].double()).sum().backward()
    _, attrs, grads = nr.mlp_reference(inp, torch.float64)
    fails = []
    _rel(attrs, want.detach(), "attrs", 1e-11, fails)
    for i, m in enumerate(mods):
        _rel(grads[2 * i], m.weight.grad, nr.PARAM_NAMES[2 * i], 1e-11, fails)
        _rel(grads[2 * i + 1], m.bias.grad, nr.PARAM_NAMES[2 * i + 1], 1e-11, fails)
    assert not fails, "\n".join(fails)
    if regime == "init":      # the start-up regime is what the per-head groups are for: five orders of magnitude between the heads
        assert float(inp["params"][26].abs().max()) < 1e-7 < 1e-5 < float(inp["params"][20].abs().max())


@pytest.mark.parametrize("key", ["M64", "init64", "dead_l3", "zero_l6"])
def test_own_masks_change_nothing(key):
    inp, stages, attrs, grads = _ref(key)
    s2, a2, g2 = nr.mlp_reference(inp, torch.float64, masks=nr.masks_of(stages))
    assert torch.equal(attrs, a2)
    for n in stages:
        assert torch.equal(stages[n], s2[n]), n
    for n, a, b in zip(nr.PARAM_NAMES, grads, g2):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("key", ["M64", "trained64", "x16_column"])
def test_stages_reproduce_the_whole(key):
    """Every per-stage function, fed the whole reference's previous entries, gives the matching entry (1e-12 of its scale)."""
    inp, s, attrs, grads = _ref(key)
    P, f64 = inp["params"], torch.float64
    m = nr.masks_of(s)
    fails = []

    def same(got, want, name):
        err, scale = float((got - want).abs().max()), float(want.abs().max())
        if not err <= 1e-12 * scale:
            fails.append("%s: err %.3e scale %.3e" % (name, err, scale))

    same(nr.stage_posenc(inp["t"].float(), 6, f64), s["et"], "et")
    same(nr.stage_posenc(inp["x"][:, :3], 10, f64), s["inp"][:, :63], "inp[0:63]")
    same(nr.stage_linear(s["et"], P[0], P[1], f64), s["t1"], "t1")
    same(nr.stage_linear(s["t1"], P[2], P[3], f64, relu=False), s["inp"][:, 63:], "inp[63:93]")
    same(nr.stage_linear(s["inp"], P[4], P[5], f64), s["h0"], "h0")
    for l in (1, 2, 3, 4, 6, 7):
        same(nr.stage_linear(s["h%d" % (l - 1)], P[4 + 2 * l], P[5 + 2 * l], f64), s["h%d" % l], "h%d" % l)
    same(nr.stage_skip(s["inp"], s["h4"], P[14], P[15], f64), s["h5"], "h5")
    same(nr.stage_heads(s["h7"], P, inp["rot_bias"], f64), attrs, "attrs")
    same(nr.stage_dgrad(inp["cot"], nr.head_matrix(P, f64), m[8], f64), s["dz7"], "dz7")
    for l in (7, 6, 4, 3, 2, 1):
        same(nr.stage_dgrad(s["dz%d" % l], P[4 + 2 * l], m[l], f64), s["dz%d" % (l - 1)], "dz%d" % (l - 1))
    same(nr.stage_dgrad(s["dz5"], P[14], m[5], f64, (nr.IN, nr.IN + nr.W)), s["dz4"], "dz4")
    same(nr.stage_dt2(s["dz5"], P[14], s["dz0"], P[4], f64), s["dt2"], "dt2")
    same(nr.stage_dgrad(s["dt2"], P[2], m[0], f64), s["dt1"], "dt1")
    xs = {0: s["inp"], 5: torch.cat([s["inp"], s["h4"]], -1)}
    for l in range(8):
        dw, db = nr.stage_wgrad(s["dz%d" % l], xs.get(l, s["h%d" % max(l - 1, 0)]), f64)
        same(dw, grads[4 + 2 * l], "L%d.w" % l)
        same(db, grads[5 + 2 * l], "L%d.b" % l)
    for h, (lo, hi) in enumerate(nr.HEAD_COLS):
        dw, db = nr.stage_wgrad(inp["cot"][:, lo:hi], s["h7"], f64)
        same(dw, grads[20 + 2 * h], nr.HEAD_NAMES[h] + ".w")
        same(db, grads[21 + 2 * h], nr.HEAD_NAMES[h] + ".b")
    for i, (dz, x) in enumerate((("dt1", "et"), ("dt2", "t1"))):
        dw, db = nr.stage_wgrad(s[dz], s[x], f64)
        same(dw, grads[2 * i], nr.LAYERS[i] + ".w")
        same(db, grads[2 * i + 1], nr.LAYERS[i] + ".b")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("key", sorted(nr.GPU_CASES))
def test_masks_are_decided(key):
    """A property of the INPUTS: float32 and float64 disagree on the sign of at most MASK_CAP of the 9 * 256 * M pre-activations.
    The GPU test imposes the kernel's masks on the float64 backward and allows that many to differ from the reference's own."""
    inp, s64 = _ref(key)[:2]
    s32 = nr.mlp_reference(inp, torch.float32)[0]
    differ = sum(int((a != b).sum()) for a, b in zip(nr.masks_of(s32), nr.masks_of(s64)))
    print("MLP %-12s M %4d: %d of %d masks differ between float32 and float64" % (key, inp["x"].shape[0], differ, 9 * 256 * inp["x"].shape[0]))
    assert differ <= nr.MASK_CAP


def test_layouts_and_groups():
    """The buffer layouts as csrc/node_mlp.h states them, and column groups that tile every tensor."""
    M = 128
    assert nr.sv_total(M) == M * (96 + 16 + 9 * 256) and nr.sc_total(M) == M * (9 * 256 + 32)
    sv = nr.split_saved(torch.arange(nr.sv_total(M), dtype=torch.float64), M)
    assert sv["et16"][0, 0] == M * 96 and sv["t1"][0, 0] == M * 112 and sv["h7"][M - 1, 255] == nr.sv_total(M) - 1
    sc = nr.split_scratch(torch.arange(nr.sc_total(M), dtype=torch.float64), M)
    assert sc["dz7"][0, 0] == 7 * M * 256 and sc["dt1"][0, 0] == 8 * M * 256 and sc["dt2_32"][M - 1, 31] == nr.sc_total(M) - 1
    inp = nr.build_inputs(64)
    assert len(inp["params"]) == len(nr.PARAM_NAMES) == 28
    for name, p in zip(nr.PARAM_NAMES, inp["params"]):
        cols = nr.as_rows(name, p).shape[1]
        groups = nr.column_groups(name)
        assert groups[0][1] == 0 and (groups[-1][2] or cols) == cols
        assert all(a[2] == b[1] for a, b in zip(groups, groups[1:]))
    assert [p.shape[1] for p in inp["params"][0:20:2]] == [13, 256, 93] + [256] * 4 + [349, 256, 256]
    assert [p.shape[0] for p in inp["params"][20::2]] == [4, 3, 4, 2]


@pytest.mark.parametrize("key", ["far_group", "far_inside"])
def test_far_rows(key):
    """Padding nodes: finite at both precisions (sin and cos of arguments up to 5.12e6), and -- their cotangent rows being zero --
    without any effect on the gradients: the same case with the rows deleted gives the same float64 numbers."""
    inp, s64, a64, g64 = _ref(key)
    far = list(nr.GPU_CASES[key]["far_rows"])
    s32, a32, g32 = nr.mlp_reference(inp, torch.float32)
    for stages, attrs, grads in ((s64, a64, g64), (s32, a32, g32)):
        assert all(bool(torch.isfinite(v).all()) for v in list(stages.values()) + [attrs] + grads)
    assert float(inp["x"][far, :3].min()) == nr.FAR and float(inp["cot"][far].abs().max()) == 0.0
    for n in ["dz%d" % l for l in range(8)] + ["dt1", "dt2"]:
        assert float(s64[n][far].abs().max()) == 0.0, n
    # (a) the rows moved to ordinary places, cotangent rows still zero: the same sums over the same rows, bit for bit
    near = dict(inp, x=inp["x"].clone())
    near["x"][far, :3] = torch.tensor([0.3, -0.5, 0.7])
    for n, a, b in zip(nr.PARAM_NAMES, g64, nr.mlp_reference(near, torch.float64)[2]):
        assert torch.equal(a, b), "%s: %.3e" % (n, float((a - b).abs().max()))
    # (b) the rows deleted: the same terms, but a sum over another row count runs in another order (a BLAS blocks M = 59 unlike
    # M = 64), so "equal" is equal up to the reordering of n terms: |difference| <= 2 n 2^-53 sum |terms|, with the sum of the
    # absolute terms bounded by M max|dZ| max|X| <= M max|dZ| max(1, max|H|) per tensor
    M = inp["x"].shape[0]
    keep = [r for r in range(M) if r not in far]
    cut = dict(inp, x=inp["x"][keep], t=inp["t"][keep], cot=inp["cot"][keep])
    gcut = nr.mlp_reference(cut, torch.float64)[2]
    zmax = max(float(s64[n].abs().max()) for n in s64 if n.startswith("d"))
    zmax = max(zmax, float(inp["cot"].abs().max()))
    keep_t = torch.tensor(keep)
    xmax = max(1.0, max(float(s64[n][keep_t].abs().max()) for n in s64 if not n.startswith("d")))
    bound = 2 * M * 2.0 ** -53 * M * zmax * xmax
    for n, a, b in zip(nr.PARAM_NAMES, g64, gcut):
        assert float((a - b).abs().max()) <= bound, "%s: %.3e > %.3e" % (n, float((a - b).abs().max()), bound)
