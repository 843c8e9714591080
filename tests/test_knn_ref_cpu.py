"""Preconditions of tests/test_knn_fp64_gpu.py that need no GPU: the inputs of every case leave float64 a decided answer on all
but CAP of the points, the `ties` builder really ties, the checker of tests/knn_ref.py rejects every kind of wrong answer, and the
PyTorch path of deform.knn_indices passes it."""
import pytest
import torch

import knn_ref as kr

_SHAPES = sorted({c[:4] for c in kr.all_cases()})


@pytest.mark.parametrize("name,N,M,D", _SHAPES)
def test_inputs_of_the_gpu_cases_are_decided(name, N, M, D):
    """At most CAP = 5e-3 of the points of a case may be undecided at GAP (they are still checked, but only to within GAP): a
    condition on the inputs alone.  A case above the cap gets another seed or size, never another cap.  The second-trip case is
    taken at the point count of a 256-CU device and on the sample the GPU test checks (which asserts the cap again on its own)."""
    Ks = sorted({c[4] for c in kr.all_cases() if c[:4] == (name, N, M, D)})
    x, nodes = kr.build(name, N, M, D)
    if M == kr.STRIDE_M:
        x = x[kr.stride_sample(N)]
    d, _ = kr.knn_float64(x, nodes, max(Ks))
    for K in Ks:
        share = float((~kr.decided(d[:, :K + 1])).double().mean())
        print("undecided %-8s N=%-6d M=%-4d D=%-2d K=%d  %.2e" % (name, N, M, D, K, share))
        assert share <= kr.CAP, (name, N, M, D, K, share)


def test_far_is_where_control_nodes_park_their_padding():
    from dgs_amd.deform import ControlNodes
    assert kr.FAR == ControlNodes.FAR


@pytest.mark.parametrize("K", [3, 4])
def test_ties_builder_has_exact_ties_resolved_by_index(K):
    _, N, M, D, _ = kr.SCENES[3]
    x, nodes = kr.build("ties", N, M, D)
    lo, hi = kr.tie_rows(M)
    assert hi % 4 == 3 and hi >= M // 2
    assert torch.equal(nodes[lo], nodes[hi])
    dl = ((x.double() - nodes[lo].double()) ** 2).sum(1)
    dh = ((x.double() - nodes[hi].double()) ** 2).sum(1)
    assert torch.equal(dl, dh)                                   # an exact float64 tie on every point
    d, j = kr.knn_float64(x, nodes, K)
    assert bool((d[:M, 0] == 0).all())                           # the first M points lie on their nodes
    assert j[lo, :2].tolist() == [lo, hi] and j[hi, :2].tolist() == [lo, hi]
    both = ((j == lo).any(1) & (j == hi).any(1)).nonzero().flatten()
    assert both.numel() > 20                                     # the tie is inside the K + 1 smallest of enough points ...
    pos_lo = (j[both] == lo).float().argmax(1)
    pos_hi = (j[both] == hi).float().argmax(1)
    assert bool((pos_hi == pos_lo + 1).all())                    # ... and the reference puts the lower index first
    edge = ((j[:, K - 1] == lo) & (j[:, K] == hi)).sum()         # ... also across the K / K + 1 boundary, where only the index
    assert int(edge) > 0                                         # decides which of the two is returned
    # ... and on some of those a node of hi's own group of four (scanned just before hi) is among the K - 1 nearer ones, with all
    # of them scanned before hi: the plain scan then meets hi while lo sits in the last slot with the same distance
    near = j[:, :K - 1]
    bite = (j[:, K - 1] == lo) & (j[:, K] == hi) & (near < hi).all(1) & (near >= hi - 3).any(1) & kr.decided(d)
    print("ties K=%d: tie inside the K+1 smallest on %d points, across the boundary on %d, behind the scan's gate on %d"
          % (K, both.numel(), int(edge), int(bite.sum())))
    assert int(bite.sum()) >= 3


def _mutation_case():
    x, nodes = kr.build("unit", 2000, 100, 11)
    K = 3
    d, j = kr.knn_float64(x, nodes, K)
    p = int(kr.decided(d).nonzero()[7])                          # one decided point
    dist2 = ((x[:, None, :] - nodes[j[:, :K]]) ** 2).sum(-1)
    return x, nodes, K, j, p, dist2


def test_checker_accepts_the_reference_and_rejects_every_mutation():
    x, nodes, K, j, p, dist2 = _mutation_case()
    M = nodes.shape[0]
    good = j[:, :K].contiguous()
    st = kr.check_answer(good, x, nodes, K, dist2=dist2)
    assert st["undecided"] <= kr.CAP and st["dist2_rel"] <= kr.DIST_REL

    def mutated(fn):
        bad = good.clone()
        fn(bad)
        return bad

    def swap(b):
        b[p, 0], b[p, 1] = good[p, 1], good[p, 0]

    mutations = {
        "last neighbour replaced by the (K+1)-th": lambda b: b.__setitem__((p, K - 1), j[p, K]),
        "two slots swapped": swap,
        "one index duplicated": lambda b: b.__setitem__((p, 1), good[p, 0]),
        "one index set to M": lambda b: b.__setitem__((p, 2), M),
        "one index set to -1": lambda b: b.__setitem__((p, 0), -1),
    }
    for what, fn in mutations.items():
        bad = mutated(fn)
        assert not torch.equal(bad, good), what
        with pytest.raises(AssertionError):
            kr.check_answer(bad, x, nodes, K)
            pytest.fail("the checker accepted: " + what)
    off = dist2.clone()
    off[p, 1] *= 1 + 1e-5
    with pytest.raises(AssertionError):
        kr.check_answer(good, x, nodes, K, dist2=off)
    with pytest.raises(AssertionError):
        kr.check_answer(good.int(), x, nodes, K)
    with pytest.raises(AssertionError):
        kr.check_answer(good[:, :2].contiguous(), x, nodes, K)


def test_checker_holds_undecided_points_to_the_gap():
    """Two nodes 1e-7 relative apart in distance from one point: either order passes, a node that is clearly farther does not."""
    nodes = torch.tensor([[0.5, 0.0, 0.0], [-0.5, 0.0, 0.0], [0.0, 0.9, 0.0], [0.0, 0.0, 2.0]], dtype=torch.float32)
    nodes[1, 0] = torch.nextafter(torch.tensor(-0.5), torch.tensor(-1.0))      # one ulp farther: 1.2e-7 relative in the distance
    x = torch.zeros(1, 3)
    d, _ = kr.knn_float64(x, nodes, 2)
    assert not bool(kr.decided(d)[0]) and float(d[0, 0]) < float(d[0, 1])
    kr.check_answer(torch.tensor([[0, 1]]), x, nodes, 2)
    kr.check_answer(torch.tensor([[1, 0]]), x, nodes, 2)
    for bad in ([0, 2], [2, 0], [1, 3]):
        with pytest.raises(AssertionError):
            kr.check_answer(torch.tensor([bad]), x, nodes, 2)


@pytest.mark.parametrize("name", ["unit", "ties"])
def test_pytorch_knn_indices_passes_the_checker(name):
    """The CPU path of deform.knn_indices (K arg-min passes over the |x|^2 + |n|^2 - 2 x.n expansion) is a correct answer too."""
    from dgs_amd.deform import knn_indices
    x, nodes = kr.build(name, 2000, 100, 11)
    for K in (1, 3, 4):
        kr.check_answer(knn_indices(x, nodes, K), x, nodes, K)
