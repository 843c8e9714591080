"""Plain-PyTorch reference of the control-node skinning kernels (lbs_fwd_kernel / lbs_bwd_kernel and their reductions in
csrc/skinning_kernels.h), written from the formulas of include/dgs_train_ops.h, for any hyper dimension 0 <= H <= 13 and at any
floating-point precision: float64 is the reference of tests/test_skinning_fp64_gpu.py, float32 its yardstick (what a straight
float32 evaluation of the same formulas loses against float64).  tests/test_skinning_ref_cpu.py ties it to ControlNodes.forward,
which the goldens pin against the original project.  A helper module: no tests in here."""
import math

import torch
import torch.nn.functional as F

K = 3
FAR = 1.0e4            # where ControlNodes parks its padding nodes (ControlNodes.FAR)
SURFEL_GRADS = ("xyz", "scaling", "rotation", "opacity", "feature")
NODE_GRADS = ("nodes", "radius", "weight", "attrs")


def _rotate(q, v):
    """Rotation matrix of the (not necessarily unit) real-first quaternion q[..., 4] applied to v[..., 3]."""
    r, i, j, k = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    x, y, z = v.unbind(-1)
    return torch.stack([(1 - s * (j * j + k * k)) * x + s * (i * j - k * r) * y + s * (i * k + j * r) * z,
                        s * (i * j + k * r) * x + (1 - s * (i * i + k * k)) * y + s * (j * k - i * r) * z,
                        s * (i * k - j * r) * x + s * (j * k + i * r) * y + (1 - s * (i * i + j * j)) * z], -1)


def skin_reference(inputs, H, dtype, assembled):
    """Outputs and autograd gradients of the skinning at precision `dtype`, on the device of inputs["xyz"].

    inputs: xyz[N,3], feature[N,>=max(H,1)], idx[N,3] int64, attrs[M,13], mask ([N], [N,1] or None),
            nodes[M,3+H] + radius_raw[M] + weight_raw[M,1]  (dgs_deform_*)   or   ntab[M,3+H+2] (dgs_lbs_*: activated radius, weight),
            cot: the cotangents of the outputs, in their order;  assembled also: scaling[N,2], rotation[N,4], opacity[N,1].
    assembled=False: out d_xyz, d_rot, d_scale;   True: means3D, scales, rotations, opacity (dgs_deform_forward).
    -> (out, grad): dicts of detached tensors.  grad: feature, attrs, and nodes / radius / weight or ntab; assembled adds xyz,
    scaling, rotation, opacity.  attrs is a leaf: its gradient is an output of its own."""
    def leaf(name):
        return inputs[name].detach().to(dtype).clone().requires_grad_(True)

    x = inputs["xyz"].detach().to(dtype)
    idx = inputs["idx"]
    feature, attrs = leaf("feature"), leaf("attrs")
    leaves = {"feature": feature, "attrs": attrs}
    if "ntab" in inputs:
        ntab = leaves["ntab"] = leaf("ntab")
        node_xyz, node_hyper, radius, weight = ntab[:, :3].detach(), ntab[:, 3:3 + H], ntab[:, 3 + H], ntab[:, 3 + H + 1]
    else:
        nodes, rr, wr = leaf("nodes"), leaf("radius_raw"), leaf("weight_raw")
        leaves.update(nodes=nodes, radius=rr, weight=wr)
        node_xyz, node_hyper = nodes[:, :3].detach(), nodes[:, 3:3 + H]
        radius, weight = torch.exp(rr), torch.sigmoid(wr).reshape(-1)
    mask = inputs.get("mask")
    mask = None if mask is None else mask.detach().to(dtype).reshape(-1, 1)

    # blend weights: squared distance over 3 + H coordinates (node xyz detached), Gaussian kernel, normalised over the K neighbours
    dl = x[:, None, :] - node_xyz[idx]                                  # [N,K,3]
    dh = feature[:, None, :H] - node_hyper[idx]                         # [N,K,H]
    dist = (dl * dl).sum(-1) + (dh * dh).sum(-1)
    w = torch.exp(-dist / (2 * radius[idx] ** 2)) * weight[idx] + 1e-7
    w = w / w.sum(-1, keepdim=True)
    # local frame: rotate x - node by the node's quaternion, back to the world, plus the node's translation
    a = attrs[idx]                                                      # [N,K,13]
    moved = _rotate(a[..., 0:4], dl) + node_xyz[idx] + a[..., 4:7]
    d_xyz = (w[..., None] * moved).sum(1) - x
    d_rot = (w[..., None] * a[..., 7:11]).sum(1)
    d_scale = (w[..., None] * a[..., 11:13]).sum(1)
    if mask is not None:
        d_xyz, d_rot, d_scale = d_xyz * mask, d_rot * mask, d_scale * mask
    if assembled:
        xyz = leaves["xyz"] = leaf("xyz")
        scaling, rotation, opacity = leaf("scaling"), leaf("rotation"), leaf("opacity")
        leaves.update(scaling=scaling, rotation=rotation, opacity=opacity)
        out = {"means3D": xyz + d_xyz, "scales": torch.exp(scaling) + d_scale, "rotations": F.normalize(rotation + d_rot),
               "opacity": torch.sigmoid(opacity)}
    else:
        out = {"d_xyz": d_xyz, "d_rot": d_rot, "d_scale": d_scale}
    cot = [c.detach().to(dtype) for c in inputs["cot"]]
    assert len(cot) == len(out)
    loss = sum((o * c).sum() for o, c in zip(out.values(), cot))
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    grad = {n: (torch.zeros_like(leaves[n]) if g is None else g).detach() for n, g in zip(names, grads)}
    return {k: v.detach() for k, v in out.items()}, grad


def column_groups(name, H):
    """Column ranges a tensor is compared by (the scales of the groups differ by orders of magnitude): list of (label, lo, hi)."""
    if name == "attrs":
        return [("attrs[0:4]", 0, 4), ("attrs[4:7]", 4, 7), ("attrs[7:11]", 7, 11), ("attrs[11:13]", 11, 13)]
    if name == "nodes":
        return [("nodes.hyper", 3, 3 + H)]
    if name == "ntab":
        return [("ntab.hyper", 3, 3 + H), ("ntab.radius", 3 + H, 4 + H), ("ntab.weight", 4 + H, 5 + H)]
    if name == "feature":
        return [("feature", 0, H)]
    return [(name, 0, None)]


def knn_bruteforce(xyz, feature, nodes, H, k=4, chunk=8192):
    """float64 brute force over the 3 + H coordinates: (dist2[N,k] ascending, idx[N,k])."""
    xq = torch.cat([xyz.double(), feature[:, :H].double()], 1)
    nd = nodes[:, :3 + H].double()
    k = min(k, nd.shape[0])
    ds, js = [], []
    for s in range(0, xq.shape[0], chunk):
        d = ((xq[s:s + chunk, None, :] - nd[None]) ** 2).sum(-1)
        v, j = torch.topk(d, k, dim=-1, largest=False, sorted=True)
        ds.append(v)
        js.append(j)
    if not ds:
        return xq.new_zeros((0, k)), torch.zeros((0, k), dtype=torch.int64, device=xq.device)
    return torch.cat(ds), torch.cat(js)


def knn_decided(dist2, gap=1e-5):
    """Points whose neighbour ranking float32 arithmetic can be held to: the relative gap between every consecutive pair of the
    (up to four) smallest float64 distances exceeds `gap`."""
    lo, hi = dist2[:, :-1], dist2[:, 1:]
    return ((hi - lo) > gap * hi).all(1)


def build_inputs(N, M, H, fstride=None, mask_kind="sigmoid", idx_kind="knn", edge_points=(), seed=0):
    """Fixed-seed float32 CPU inputs of one skinning case (move them with to_device()).

    Positions lie in a unit box, hyper coordinates are about 0.05 (nodes: 0.01 + 0.02 noise, as ControlNodes.init_from_points
    leaves them plus the perturbation of the existing tests); the kernel radius starts at the node spacing (0.1 at least, as
    init_from_points gives for a unit scene) with 0.2 of log-normal spread, the weight logit is 0.5 randn; the attribute table has a
    quaternion far from the identity and d_xyz about 0.1.
    fstride: columns of `feature` (default max(H, 1): the C ABI wants a non-NULL feature even at H = 0).
    mask_kind: "none" | "sigmoid" | "binary" (sigmoid values with exact 0 and exact 1 mixed in).
    idx_kind: "knn" (idx is left out: the caller runs the neighbour search under test, or knn_bruteforce) |
              "same" (all 64 lanes of a wave share their three nodes) | "distinct" (the 64 lanes of a wave differ in all three slots).
    edge_points: any of "tiny" (ten points with rotation = 0 and mask = 0: F.normalize's clamp branch), "far" (twenty points 50
              units from every node: the Gaussian underflows in float32, w falls to its 1e-7 floor), "pad" (the last eight nodes
              parked at ControlNodes.FAR)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    fstride = max(H, 1) if fstride is None else fstride
    assert fstride >= max(H, 1)
    xyz = torch.rand(N, 3, generator=g)
    feature = 0.05 * rn(N, fstride)
    node_xyz = torch.rand(M, 3, generator=g)
    nodes = torch.cat([node_xyz, 0.01 + 0.02 * rn(M, H)], 1)
    # hand-made neighbour lists pair points with nodes anywhere in the box: a kernel wide enough to keep their weights alive
    r0 = max(0.1, 0.5 * M ** (-1.0 / 3.0)) if idx_kind == "knn" else 0.7
    radius_raw = math.log(r0) + 0.2 * rn(M)
    weight_raw = 0.5 * rn(M, 1)
    attrs = torch.cat([torch.tensor([1.0, 0.0, 0.0, 0.0]) + 0.5 * rn(M, 4), 0.1 * rn(M, 3), 0.1 * rn(M, 4), 0.02 * rn(M, 2)], 1)
    scaling = math.log(0.02) + 0.3 * rn(N, 2)
    rotation = rn(N, 4)
    opacity = rn(N, 1)
    mask = None
    if mask_kind != "none":
        mask = torch.sigmoid(rn(N))
        if mask_kind == "binary":
            mask[0::5] = 0.0
            mask[1::5] = 1.0
    if "pad" in edge_points:
        assert M > 8 + K
        nodes[-8:, :3] = FAR
    if "far" in edge_points:
        assert N >= 40
        xyz[20:40] += 50.0
    if "tiny" in edge_points:
        assert N >= 10 and mask is not None
        rotation[:10] = 0.0
        mask[:10] = 0.0
    inp = {"xyz": xyz, "feature": feature, "nodes": nodes.contiguous(), "radius_raw": radius_raw, "weight_raw": weight_raw, "attrs": attrs,
           "mask": mask, "scaling": scaling, "rotation": rotation, "opacity": opacity,
           "cot": [rn(N, 3), rn(N, 2), rn(N, 4), rn(N, 1)], "cot_lbs": [rn(N, 3), rn(N, 4), rn(N, 2)]}
    n = torch.arange(N)
    if idx_kind == "same":
        assert M >= 3
        inp["idx"] = torch.stack([(3 * (n // 64) + k) % M for k in range(K)], 1)
    elif idx_kind == "distinct":
        assert M >= 3 * 64
        inp["idx"] = torch.stack([(n % 64 + 64 * k + 7 * (n // 64)) % M for k in range(K)], 1)
    else:
        assert idx_kind == "knn"
    return inp


def to_device(inputs, device):
    mv = lambda v: v.to(device) if torch.is_tensor(v) else ([t.to(device) for t in v] if isinstance(v, list) else v)
    return {k: mv(v) for k, v in inputs.items()}
