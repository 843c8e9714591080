"""float64 statement of the neighbour search (knn_kernel, knn_refine_kernel, knn_refine_mfma_kernel in csrc/knn_kernels.h), the one
assertion helper the tests hold an answer to, the named input builders and the list of cases tests/test_knn_fp64_gpu.py runs
(tests/test_knn_ref_cpu.py checks their preconditions on the CPU).  A helper module: no tests in here.

The contract (include/dgs_train_ops.h): idx[N,K] int64, the K nearest rows of `nodes` under squared L2 in ascending order, ties to
the lower index, every stored index in [0, M) whatever the inputs hold.

GAP -- how close two float64 distances may be before float32 arithmetic is allowed to rank them either way.  The kernels compute
    a = sum_c (x_c - n_c)^2   over the 4 Q <= 16 zero-padded coordinates, in float32:
      * one rounding per difference (the operands are float32 values: the difference is otherwise exact),
      * its square carries that error twice plus its own rounding: three roundings per square,
      * at most 15 additions join the 16 terms; all terms are >= 0, so every addition adds one relative rounding to the sum,
    at most (1 + 3 + 15) 2^-24 = 19 * 2^-24 = 1.13e-6 relative per distance (DIST_REL), with or without FMA contraction (an FMA
    drops the rounding of the product, never adds one).  Two distances that differ by more than twice that, 2.3e-6 relative, keep
    their order in float32.  The project's constant for this (skinning_ref.knn_decided) is 1e-5: above the bound, kept.
"""
import functools

import torch

FAR = 1.0e4                  # ControlNodes.FAR: where padding nodes are parked
DIST_REL = 19 * 2.0 ** -24   # relative error of one float32 distance (docstring)
GAP = 1e-5                   # >= 2 * DIST_REL = 2.3e-6
CAP = 5e-3                   # largest undecided share a case may have (a condition on the inputs: test_knn_ref_cpu.py)
assert GAP >= 2 * DIST_REL


def distances_float64(x, nodes, chunk=8192):
    """Chunks of the [N,M] float64 squared distances of float32 inputs (differences and squares are exact in float64 up to 2^-53)."""
    xq, nd = x.double(), nodes.double()
    for s in range(0, xq.shape[0], chunk):
        xs = xq[s:s + chunk]
        d = torch.zeros((xs.shape[0], nd.shape[0]), dtype=torch.float64, device=xq.device)
        for c in range(xq.shape[1]):
            t = xs[:, c, None] - nd[None, :, c]
            d += t * t
        yield s, d


def knn_float64(x, nodes, K):
    """Brute force in float64: (dist2[N,K+1], idx[N,K+1]), the K + 1 smallest (all M when K + 1 > M) ascending; equal distances
    are ordered by index (stable sort)."""
    kk = min(K + 1, nodes.shape[0])
    ds, js = [], []
    for _, d in distances_float64(x, nodes):
        v, j = torch.sort(d, dim=1, stable=True)
        ds.append(v[:, :kk])
        js.append(j[:, :kk])
    if not ds:
        return (torch.zeros((0, kk), dtype=torch.float64, device=x.device), torch.zeros((0, kk), dtype=torch.int64, device=x.device))
    return torch.cat(ds), torch.cat(js)


def decided(d, gap=GAP):
    """[N] bool: every consecutive pair of the K + 1 smallest float64 distances is either exactly equal (a duplicated node row:
    the float32 distances are bit-identical too, and the index decides) or further apart than gap * the larger one (float32
    cannot swap them, see GAP above)."""
    lo, hi = d[:, :-1], d[:, 1:]
    return ((hi == lo) | ((hi - lo) > gap * hi)).all(1)


def check_answer(idx, x, nodes, K, dist2=None, gap=GAP):
    """Asserts that idx is a correct answer of the neighbour search for (x, nodes, K); no point is left unchecked.
      * int64 [N,K], every entry in [0, M), K distinct entries per row;
      * decided points (decided()): idx equals the float64 answer entry for entry, in order;
      * the other points: the float64 distances of the returned nodes ascend to within `gap` relative and each is within `gap`
        relative of the float64 k-th smallest (the k-th smallest of values perturbed by DIST_REL lies within DIST_REL of the true
        k-th smallest, and the node's own distance within another DIST_REL);
      * dist2, when given: float32 [N,K], every entry within DIST_REL relative of the float64 distance of the returned node.
    -> {"undecided": share of the points, "dist2_rel": largest relative deviation of dist2 (0.0 without)}."""
    N, M = x.shape[0], nodes.shape[0]
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (N, K), (idx.dtype, tuple(idx.shape))
    stats = {"undecided": 0.0, "dist2_rel": 0.0}
    if dist2 is not None:
        assert dist2.dtype == torch.float32 and tuple(dist2.shape) == (N, K)
    if N == 0:
        return stats
    assert int(idx.min()) >= 0 and int(idx.max()) < M, ("index out of range", int(idx.min()), int(idx.max()), M)
    srt = torch.sort(idx, dim=1).values
    dup = (srt[:, 1:] == srt[:, :-1]).any(1)
    assert not bool(dup.any()), ("repeated index in a row", int(dup.nonzero()[0]), idx[dup][0].tolist())
    d, j = knn_float64(x, nodes, K)
    dec = decided(d, gap)
    wrong = dec & (idx != j[:, :K]).any(1)
    if bool(wrong.any()):
        p = int(wrong.nonzero()[0])
        raise AssertionError("%d decided points differ from float64; first: point %d got %s want %s (d64 %s)"
                             % (int(wrong.sum()), p, idx[p].tolist(), j[p, :K].tolist(), d[p].tolist()))
    xq, nd = x.double(), nodes.double()
    dr = ((xq[:, None, :] - nd[idx]) ** 2).sum(-1)                       # [N,K] float64 distances of the returned nodes
    und = ~dec
    if bool(und.any()):
        du, dk = dr[und], d[und][:, :K]
        assert bool((du[:, 1:] >= du[:, :-1] * (1 - gap)).all()), "undecided point: returned nodes not ascending within gap"
        assert bool(((du - dk).abs() <= gap * torch.maximum(du, dk)).all()), "undecided point: not the k-th smallest within gap"
    stats["undecided"] = float(und.double().mean())
    if dist2 is not None:
        dev = (dist2.double() - dr).abs()
        assert bool((dev <= DIST_REL * dr).all()), ("dist2 off", float((dev / dr.clamp_min(1e-300)).max()))
        stats["dist2_rel"] = float((dev / dr.clamp_min(1e-300))[dr > 0].max()) if bool((dr > 0).any()) else 0.0
    return stats


# ---- input builders ---------------------------------------------------------------------------------------------------------
def _morton_order(p):
    q = ((p + 1) * 511.5).long().clamp(0, 1023)
    code = torch.zeros(p.shape[0], dtype=torch.long)
    for b in range(10):
        for c in range(3):
            code |= ((q[:, c] >> b) & 1) << (3 * b + c)
    return torch.argsort(code)


BUILDERS = ("unit", "hyper", "offset", "ties", "far_pad", "morton")


def tie_rows(M):
    """(lo, hi) of the `ties` builder: node row hi is a copy of row lo = 3.  hi is the LAST row of its group of four (the plain scan
    takes the nodes four at a time behind one gate) and row hi - 1 lies close to row lo: for points around them a node of hi's
    own group enters the list just before hi is offered and pushes row lo to the K-th place, where only the index decides between
    lo and hi.  With hi first in its group a scan that takes the higher index on a tie goes unnoticed (measured: a `<=` in the
    plain scan's insertion passed every case while the duplicate sat at M // 2 = 256)."""
    assert M > 8
    return 3, (M // 2) | 3


@functools.lru_cache(maxsize=None)
def build(name, N, M, D, seed=0):
    """(x[N,D], nodes[M,D]): fixed-seed float32 CPU tensors, D = 3 spatial + (D - 3) hyper coordinates.  Shared: never modify.
      unit     positions in [-1, 1]^3, hyper coordinates 0.05 randn on both sides
      hyper    hyper coordinates 0.7 randn on the points, 0.05 on the nodes: the non-spatial part dominates the distance
      offset   unit shifted by +64 on every spatial axis (a scene that is not centred: |x|^2 ~ 1e4, neighbour distances ~ 1e-2)
      ties     node row hi is a copy of row lo (tie_rows: a distant index) with row hi - 1 close by, and the first min(N, M) points
               lie exactly on the nodes (hyper 0.3 randn)
      far_pad  unit with the last eight nodes parked at FAR
      morton   nodes along a Morton curve, points in the order of their nearest node (the trainer's storage order), hyper 0.01"""
    assert name in BUILDERS and D >= 3
    g = torch.Generator().manual_seed(7000 + 101 * BUILDERS.index(name) + seed)
    H = D - 3
    fx, fn = {"hyper": (0.7, 0.05), "ties": (0.3, 0.3), "morton": (0.01, 0.01)}.get(name, (0.05, 0.05))
    x3 = torch.rand(N, 3, generator=g) * 2 - 1
    n3 = torch.rand(M, 3, generator=g) * 2 - 1
    xh = fx * torch.randn(N, H, generator=g)
    nh = fn * torch.randn(M, H, generator=g)
    if name == "morton":
        n3 = n3[_morton_order(n3)]
        x3 = x3[torch.argsort(torch.cdist(x3, n3).argmin(1), stable=True)]
    x, nodes = torch.cat([x3, xh], 1), torch.cat([n3, nh], 1)
    if name == "offset":
        x[:, :3] += 64.0
        nodes[:, :3] += 64.0
    if name == "ties":
        lo, hi = tie_rows(M)
        nodes[hi - 1] = nodes[lo] + 0.1 * torch.randn(D, generator=g)
        nodes[hi] = nodes[lo]
        x[:min(N, M)] = nodes[:min(N, M)]
    if name == "far_pad":
        assert M > 12
        nodes[-8:, :3] = FAR
    return x.contiguous(), nodes.contiguous()


def moved(x, seed=0, sigma=0.01):
    """x with its spatial coordinates moved by sigma randn: the plain scan of this is a stale seed."""
    g = torch.Generator().manual_seed(9000 + seed)
    y = x.clone()
    y[:, :3] += sigma * torch.randn(x.shape[0], 3, generator=g)
    return y


# ---- the cases of tests/test_knn_fp64_gpu.py: (builder, N, M, D, K) -----------------------------------------------------------
KS = (1, 2, 3, 4)
PLAIN_KQ = [("unit", 1537, 257, D, K) for K in KS for D in (3, 4, 5, 11, 16)]           # three workgroups of 512 points, ragged
PLAIN_STAGING = [("unit", 1537, M, 11, 3) for M in (1025, 2049)]                        # more than one 1024-node pass, remainder
PLAIN_SMALL_N = [("unit", N, 33, 11, 3) for N in (1, 2, 511, 512, 513)]
DIST2 = [(b, 1537, 257, D, 4) for b in ("unit", "ties") for D in (11, 16)]
SPLIT_H = (1, 8, 13)
SPLIT = [("unit", 1537, 257, 3 + H, 3) for H in SPLIT_H] + [("unit", 4099, 200, 11, 3)]
BOX_KQ = [("unit", 4099, 200, 3 + D2, K) for K in KS for D2 in (0, 1, 8, 13)]
BOX_LAYOUT = [("unit", 4099, M, 11, 3) for M in (201, 202, 203)]                        # M * 11 = 3, 2, 1 (mod 4)
BOX_LARGE = [("unit", 2049, 2048, 16, 4), ("unit", 2049, 1025, 11, 3)]
MFMA_KTP = [("unit", 4099, M, D, K) for D in (11, 5) for M in (32, 33, 256, 257, 512, 513, 1000, 1024) for K in KS]
MFMA_SMALL_N = [("unit", N, 77, 11, 3) for N in (1, 31, 32, 33)]
SCENES = [(b, 20000, 512, 11, 3) for b in ("offset", "hyper", "far_pad", "ties", "morton")] + [("ties", 20000, 512, 11, 4)]
NONFINITE = ("unit", 4099, 200, 11, 3)
STRIDE_M, STRIDE_K, STRIDE_SAMPLE = 64, 3, 4096


def stride_points(cus):
    """Point count at which every wave of knn_refine_mfma_kernel takes a second trip of its grid-stride loop: the launcher keeps
    per_cu = 2 workgroups of 8 waves resident per CU at this node count, one group of 32 points per wave and trip."""
    return 32 * (cus * 2 * 8) + 33


def stride_sample(N):
    """Indices of the STRIDE_SAMPLE points the second-trip test holds to float64: evenly spread, plus the last 64 points."""
    head = torch.linspace(0, N - 65, STRIDE_SAMPLE - 64).long()
    return torch.cat([head, torch.arange(N - 64, N)])


def all_cases(cus=256):
    """Every (builder, N, M, D, K) the GPU file runs (the second-trip case at the point count of a `cus`-CU device)."""
    cases = (PLAIN_KQ + PLAIN_STAGING + PLAIN_SMALL_N + DIST2 + SPLIT + BOX_KQ + BOX_LAYOUT + BOX_LARGE + MFMA_KTP + MFMA_SMALL_N
             + SCENES + [NONFINITE, ("unit", stride_points(cus), STRIDE_M, 11, STRIDE_K)])
    return sorted(set(cases))
