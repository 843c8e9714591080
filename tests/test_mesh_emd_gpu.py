"""-m gpu: dgs_emd_auction against emd_torch, the PyTorch statement of the same schedule run on the CPU -- assignment, prices, primal,
dual and rounds EQUAL -- at the sizes where the kernels change path (taken from dgs_emd_layout: a wave, a workgroup, the bidder
count S at which the host switches between the sparse and the dense bidding kernel, the LDS round T of the dense one), on the
price-war inputs, against the exact solver, twice, on a side stream, after a run that hit the cap, and inside mesh_distance."""
import functools

import pytest
import torch

from test_mesh_emd_cpu import CASES, case_inputs, check_certificate, cube, sphere_points, statement
from test_mesh_metrics_cpu import concentric_spheres

pytestmark = pytest.mark.gpu


def _layout():
    from dgs_amd import _mesh_ops
    return _mesh_ops.emd_layout()


THREADS, T, S = _layout()[:3]
# n <= S never leaves the sparse kernel; n = S + 1 starts every phase in the dense one (a single, ragged LDS round) and switches on the
# way down; n = T - 1, T, T + 1 and 2 T + 1 put the dense kernel's LDS rounds at full, full + 1 and two full + 1
SIZES = [2, 3, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, S - 1, S, S + 1, T - 1, T, T + 1, 2 * T + 1]


@functools.lru_cache(maxsize=None)
def reference(n):
    """Inputs of one size (on the CPU and on the device) and what emd_torch makes of them.  Computed once, never modified."""
    from dgs_amd.mesh_metrics import _emd_quantum, emd_torch
    a, b = cube(n, 1000 + n)
    q, inv_q = _emd_quantum(a, b)
    return (a, b, a.cuda(), b.cuda(), q, inv_q) + tuple(emd_torch(a, b, inv_q=inv_q))


def check_equal(got, want, what):
    assignment, prices, primal, dual, rounds = got[:5]
    w_assignment, w_prices, w_primal, w_dual, w_rounds = want
    print("%s: rounds %d (statement %d), primal %d (%d), dual %d (%d)" % (what, rounds, w_rounds, primal, w_primal, dual, w_dual))
    assert assignment.dtype == torch.int32 and prices.dtype == torch.int64
    assert rounds == w_rounds
    assert torch.equal(prices.cpu(), w_prices)
    assert torch.equal(assignment.cpu().long(), w_assignment)
    assert primal == w_primal and dual == w_dual


@pytest.mark.parametrize("n", SIZES)
def test_auction_equals_the_statement_at_the_edge_sizes(n):
    from dgs_amd import _mesh_ops
    a, b, ad, bd, q, inv_q, *want = reference(n)
    got = _mesh_ops.emd_auction(ad, bd, inv_q, 2_000_000)
    check_equal(got, want, "n %d" % n)


@pytest.mark.parametrize("name", ["n1", "duplicates512", "coincident300", "same_point5"])
def test_auction_equals_the_statement_on_price_wars(name):
    """Mass eviction (half of the objects one point), a war over equal costs, every cost 0, and the trivial matching."""
    from dgs_amd import _mesh_ops
    a, b = case_inputs(name)
    q, inv_q, *want = statement(name)
    got = _mesh_ops.emd_auction(a.cuda(), b.cuda(), inv_q, 2_000_000)
    check_equal(got, want, name)
    assert got[4] == CASES[name][1]


def test_device_result_against_the_exact_solver():
    """Sphere against 1.05 x another sphere, n = 1024: the bounds of the CPU test on what the device returned."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import _emd_quantum, emd
    a, b = sphere_points(1024, 1), sphere_points(1024, 2, 1.05)
    q, inv_q = _emd_quantum(a, b)
    assignment, prices, primal, dual, rounds, _ = _mesh_ops.emd_auction(a.cuda(), b.cuda(), inv_q, 2_000_000)
    check_certificate(a, b, inv_q, assignment, prices, primal, dual)
    m = emd(a.cuda(), b.cuda())
    assert torch.equal(m["assignment"].cpu(), assignment.cpu().long()) and m["emd_rounds"] == rounds and m["emd_samples"] == 1024
    assert m["emd"] == pytest.approx(float((a.double() - b.double()[assignment.cpu().long()]).norm(dim=1).mean()), rel=1e-14, abs=0.0)
    assert m["emd_gap"] == (primal - dual) * q / 1024 and 0 <= m["emd_gap"] <= q


def test_two_runs_are_bit_identical():
    from dgs_amd import _mesh_ops
    a, b, ad, bd, q, inv_q, *want = reference(S + 1)
    first = _mesh_ops.emd_auction(ad, bd, inv_q, 2_000_000)
    second = _mesh_ops.emd_auction(ad, bd, inv_q, 2_000_000)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]) and first[2:] == second[2:]


def test_auction_on_a_side_stream():
    from dgs_amd import _mesh_ops
    a, b, ad, bd, q, inv_q, *want = reference(THREADS + 1)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = _mesh_ops.emd_auction(ad, bd, inv_q, 2_000_000)
    stream.synchronize()
    check_equal(got, want, "side stream")


def test_the_cap_returns_an_error_and_the_buffers_serve_a_clean_run():
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_metrics import emd
    a, b, ad, bd, q, inv_q, *want = reference(THREADS + 1)
    lay = _mesh_ops.emd_layout()
    scratch = torch.empty(lay[4] + (THREADS + 1) * lay[5], dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"max_rounds = 10 reached in phase 0 \(eps \d+\) with \d+ of %d still unassigned" % (THREADS + 1)):
        _mesh_ops.emd_auction(ad, bd, inv_q, 10, scratch=scratch)
    with pytest.raises(RuntimeError, match="max_rounds = 10 reached"):
        emd(ad, bd, max_rounds=10)
    check_equal(_mesh_ops.emd_auction(ad, bd, inv_q, 2_000_000, scratch=scratch), want, "after the cap")
    # exactly as many rounds as the statement needs are enough
    check_equal(_mesh_ops.emd_auction(ad, bd, inv_q, want[4], scratch=scratch), want, "max_rounds = rounds")
    with pytest.raises(RuntimeError, match="max_rounds"):
        _mesh_ops.emd_auction(ad, bd, inv_q, want[4] - 1, scratch=scratch)


def test_mesh_distance_with_emd_on_the_device_equals_the_cpu_path():
    """The samples are the same points on both devices (tests/test_mesh_metrics_gpu.py asserts it), the auction is bit-identical:
    the same rounds, and the same emd to the round-off of a float64 mean."""
    from dgs_amd.mesh_metrics import mesh_distance
    inner, outer = concentric_spheres()
    kw = dict(n_samples=1500, seed=0, thresholds=(0.05, 0.15), emd_samples=1024)
    cpu = mesh_distance(inner, outer, device="cpu", **kw)
    dev = mesh_distance(inner, outer, device="cuda:0", **kw)
    print({k: (cpu[k], dev[k]) for k in ("emd", "emd_gap", "emd_samples", "emd_rounds")})
    assert dev["emd_rounds"] == cpu["emd_rounds"] and dev["emd_samples"] == cpu["emd_samples"] == 1024
    assert dev["emd_gap"] == cpu["emd_gap"]
    assert dev["emd"] == pytest.approx(cpu["emd"], rel=1e-14, abs=0.0)
