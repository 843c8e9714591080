"""Earth mover's distance on the CPU: emd_torch (the PyTorch statement of dgs_emd_auction) against an exact solver on the same
integer cost matrix (scipy.optimize.linear_sum_assignment), the cap on the rounds, the argument checks, the metric inside
mesh_distance / evaluate_meshes / the command line, a known answer, and the argument checks of the C ABI.  The inputs (CASES,
case_inputs) and the cached statement results (statement) are also what tests/test_mesh_emd_gpu.py compares the HIP path with."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from test_mesh_metrics_cpu import SPHERE_C, _write_frames, uv_sphere


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def cube(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3), generator=g), torch.rand((n, 3), generator=g)


def sphere_points(n, seed, radius=1.0):
    x = torch.randn((n, 3), generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True) * radius).contiguous()


def shifted_permutation(n, seed):
    """Points on the unit sphere against a permutation of themselves shifted by a fixed vector."""
    s = sphere_points(n, seed)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 1))
    return s, (s[perm] + torch.tensor([0.05, 0.02, -0.03])).contiguous()


def duplicate_heavy(n, seed):
    """Half of b is one repeated point, a quarter of a another: mass eviction and price wars."""
    a, b = cube(n, seed)
    b[:n // 2] = b[0]
    a[:n // 4] = a[0]
    return a, b


def coincident(n):
    """All points of a set coincide, the two sets apart: every cost is the same (the diagonal of the union is not 0)."""
    return torch.full((n, 3), 0.25), torch.full((n, 3), 0.75)


# name -> (inputs, rounds of the statement -- recorded from emd_torch; a change of the schedule shows up here first)
CASES = {
    "n1": (lambda: cube(1, 1), 0),
    "n2": (lambda: cube(2, 2), 10),
    "n3": (lambda: cube(3, 3), 20),
    "cube64": (lambda: cube(64, 64), 280),
    "cube257": (lambda: cube(257, 257), 934),
    "shifted512": (lambda: shifted_permutation(512, 5), 543),
    "duplicates512": (lambda: duplicate_heavy(512, 7), 42293),
    "coincident300": (lambda: coincident(300), 14624),
    "same_point5": (lambda: (torch.full((5, 3), 0.5), torch.full((5, 3), 0.5)), 5),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def statement(name):
    """(q, inv_q, assignment, prices, primal, dual, rounds) of emd_torch on a case.  Computed once, never modified."""
    from dgs_amd.mesh_metrics import _emd_quantum, emd_torch
    a, b = case_inputs(name)
    q, inv_q = _emd_quantum(a, b)
    return (q, inv_q) + tuple(emd_torch(a, b, inv_q=inv_q))


def exact_optimum(a, b, inv_q):
    """The optimum of the assignment problem on the integer matrix of the pinned expression, by scipy."""
    from scipy.optimize import linear_sum_assignment
    from dgs_amd.mesh_metrics import _emd_costs
    cost = _emd_costs(a, b, inv_q).numpy()
    rows, cols = linear_sum_assignment(cost)
    return int(cost[rows, cols].sum()), cost


def check_certificate(a, b, inv_q, assignment, prices, primal, dual):
    """sigma is a permutation, primal and dual are what they claim to be, and 0 <= primal - OPT <= n, 0 <= OPT - dual <= n: the
    bounds eps-complementary slackness with eps = 1 gives, no slack."""
    n = a.shape[0]
    opt, cost = exact_optimum(a, b, inv_q)
    sigma = assignment.cpu().numpy().astype(np.int64)
    p = prices.cpu().numpy().astype(np.int64)
    assert sorted(sigma.tolist()) == list(range(n))
    assert primal == int(cost[np.arange(n), sigma].sum())
    assert dual == int((cost + p[None, :]).min(axis=1).sum()) - int(p.sum())
    print("n %d: primal - OPT = %d, OPT - dual = %d (both in [0, %d]), largest price %d" % (n, primal - opt, opt - dual, n, int(p.max())))
    assert 0 <= primal - opt <= n
    assert 0 <= opt - dual <= n


# ---- the statement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_emd_torch_against_the_exact_solver(name, monkeypatch):
    from dgs_amd import mesh_metrics
    a, b = case_inputs(name)
    q, inv_q, assignment, prices, primal, dual, rounds = statement(name)
    check_certificate(a, b, inv_q, assignment, prices, primal, dual)
    assert rounds == CASES[name][1]
    n = a.shape[0]

    def cached(a_, b_, max_rounds, inv_q_):
        """emd() on top of the statement's cached result (the slow cases run their thousands of rounds once per session)."""
        assert torch.equal(a_, a) and torch.equal(b_, b) and inv_q_ == inv_q and max_rounds == 2_000_000
        return assignment, prices, primal, dual, rounds

    monkeypatch.setattr(mesh_metrics, "emd_torch", cached)
    m = mesh_metrics.emd(a, b)
    assert torch.equal(m["assignment"], assignment) and m["emd_rounds"] == rounds and m["emd_samples"] == n
    # the float64 mean of the matched distances (to the round-off of a differently ordered float64 sum)
    assert m["emd"] == pytest.approx(float((a.double() - b.double()[assignment]).norm(dim=1).mean()), rel=1e-14, abs=0.0)
    assert m["emd_gap"] == (primal - dual) * q / n and 0 <= m["emd_gap"] <= q
    if name == "same_point5":
        assert q == 0.0 and inv_q == 0.0 and m["emd"] == 0.0 and m["emd_gap"] == 0.0
    if name == "coincident300":
        assert q > 0.0


def test_the_cap_on_the_rounds_raises():
    from dgs_amd.mesh_metrics import emd
    a, b = cube(512, 512)
    with pytest.raises(RuntimeError, match=r"max_rounds = 10 reached in phase 0 \(eps \d+\) with \d+ of 512 still unassigned"):
        emd(a, b, max_rounds=10)


def test_emd_argument_checks():
    from dgs_amd.mesh_metrics import emd
    a, b = cube(8, 0)
    with pytest.raises(ValueError, match="same size"):
        emd(a, b[:7])
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        emd(a[:, :2], b[:, :2])
    with pytest.raises(ValueError, match=r"\[N,3\]"):
        emd(a.reshape(-1), b.reshape(-1))
    with pytest.raises(ValueError, match="non-finite"):
        emd(a, torch.full_like(b, float("nan")))
    with pytest.raises(ValueError):
        emd(a[:0], b[:0])
    with pytest.raises(ValueError, match="max_rounds"):
        emd(a, b, max_rounds=0)


# ---- inside the mesh metrics ----------------------------------------------------------------------------------------------------
def test_mesh_distance_with_and_without_emd():
    from dgs_amd.mesh_metrics import emd, mesh_distance, sample_surface
    pred, gt = uv_sphere(1.0, SPHERE_C, 16, 8), uv_sphere(1.1, SPHERE_C, 16, 8)
    kw = dict(n_samples=1000, seed=3, thresholds=(0.02, 0.08), device="cpu")
    plain = mesh_distance(pred, gt, **kw)
    assert mesh_distance(pred, gt, emd_samples=0, **kw) == plain and not any(k.startswith("emd") for k in plain)
    with_emd = mesh_distance(pred, gt, emd_samples=256, **kw)
    assert {k: v for k, v in with_emd.items() if not k.startswith("emd")} == plain
    assert set(with_emd) - set(plain) == {"emd", "emd_gap", "emd_samples", "emd_rounds"}
    t = lambda m: (torch.from_numpy(m[0]), torch.from_numpy(m[1]))
    pp, _, _ = sample_surface(*t(pred), 1000, 3)
    gp, _, _ = sample_surface(*t(gt), 1000, 4)
    m = emd(pp[:256], gp[:256])
    assert all(with_emd[k] == m[k] for k in ("emd", "emd_gap", "emd_samples", "emd_rounds")) and with_emd["emd_samples"] == 256
    # no pair of a matching is shorter than the person's nearest object: the one-to-one mean is at least the directed nearest mean
    nearest = (pp[:256, None, :].double() - gp[None, :256, :].double()).norm(dim=2).min(dim=1).values.mean()
    assert with_emd["emd"] >= float(nearest) * (1 - 1e-12)
    with pytest.raises(ValueError, match="emd_samples"):
        mesh_distance(pred, gt, emd_samples=1001, **kw)
    with pytest.raises(ValueError, match="emd_samples"):
        mesh_distance(pred, gt, emd_samples=-1, **kw)


def test_evaluate_meshes_and_cli_with_emd(tmp_path):
    from dgs_amd.mesh_metrics import evaluate_meshes, main
    pred, gt = _write_frames(tmp_path, 3)
    kw = dict(n_samples=1000, seed=3, thresholds=(0.02, 0.08), device="cpu")
    plain = evaluate_meshes(pred, gt, **kw)
    assert evaluate_meshes(pred, gt, emd_samples=0, **kw) == plain and "emd_samples" not in plain["settings"]
    res = evaluate_meshes(pred, gt, emd_samples=256, **kw)
    on_disk = json.load(open(os.path.join(pred, "mesh_metrics.json")))
    assert on_disk == json.loads(json.dumps(res))
    new = {"emd", "emd_gap", "emd_samples", "emd_rounds"}
    assert set(res["mean"]) == set(plain["mean"]) | new and all(set(r) == set(p) | new for r, p in zip(res["frames"], plain["frames"]))
    assert res["settings"] == dict(plain["settings"], emd_samples=256)
    for r, p in zip(res["frames"], plain["frames"]):
        assert {k: v for k, v in r.items() if k not in new} == p and r["emd_samples"] == 256
    for k in new:
        assert res["mean"][k] == pytest.approx(sum(r[k] for r in res["frames"]) / 3, rel=1e-12)
    emds = [r["emd"] for r in res["frames"]]
    assert emds[0] < emds[1] < emds[2]                                        # the spheres grow away from the ground truth
    os.remove(os.path.join(pred, "mesh_metrics.json"))
    main([pred, gt, "--samples", "1000", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu", "--emd", "256"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == on_disk
    main([pred, gt, "--samples", "1000", "--seed", "3", "--thresholds", "0.02", "0.08", "--device", "cpu"])
    assert json.load(open(os.path.join(pred, "mesh_metrics.json"))) == json.loads(json.dumps(plain))


def test_a_translated_copy_costs_at_most_the_translation():
    """Samples p against p + t (the same sample indices): the identity is a matching of mean length mean |b_i - a_i|, and the
    matching found is within n quanta of the optimum of the quantised problem (primal <= OPT + n).  A cost is within one quantum
    of its pair's true distance / q: half a quantum from rint, and less than half from the fp32 evaluation (three roundings into
    d2's terms and two sums, the sqrt, 1 / q and the product: under 6 * 2^-24 relative, of at most 2^20 quanta = 0.375).  Hence
    sum d(i, sigma(i)) / q <= primal + n <= OPT + 2 n <= sum c(i, i) + 2 n <= sum d(i, i) / q + 3 n, i.e.
    emd <= mean |b_i - a_i| + 3 q.  No tolerance beyond that."""
    from dgs_amd.mesh_metrics import _emd_quantum, emd, sample_surface
    v, f = uv_sphere(1.0, SPHERE_C, 16, 8)
    p, _, _ = sample_surface(torch.from_numpy(v), torch.from_numpy(f), 300, 0)
    b = (p + torch.tensor([0.03, -0.04, 0.12])).contiguous()                  # |t| = 0.13
    identity = float((b.double() - p.double()).norm(dim=1).mean())
    q, _ = _emd_quantum(p, b)
    m = emd(p, b)
    print("emd %.9f, identity matching %.9f, q %.3e, gap %.3e" % (m["emd"], identity, q, m["emd_gap"]))
    assert m["emd"] <= identity + 3 * q
    assert identity <= 0.13 * (1 + 1e-6)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_emd_arguments_are_validated_before_any_launch():
    """Bad arguments are refused by the host wrapper (status < 0 and a message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    assert lib.dgs_mesh_ops_abi_version() == 2
    lay = _mesh_ops.emd_layout()
    assert len(lay) == 6 and all(x > 0 for x in lay)
    pts = (ctypes.c_float * 12)()
    out = (ctypes.c_longlong * 4)()
    scratch = (ctypes.c_ulonglong * ((lay[4] + 4 * lay[5]) // 8))()
    result = (ctypes.c_longlong * lay[3])()
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    call = lambda n, a, b, inv_q, max_rounds, s, s_bytes, assignment, prices, res: lib.dgs_emd_auction(
        n, a, b, inv_q, max_rounds, s, s_bytes, assignment, prices, res, None)
    good = (4, p(pts), p(pts), 1.0, 100, p(scratch), ctypes.sizeof(scratch), p(out), p(out), p(result))
    for position, message in ((1, b"null"), (2, b"null"), (5, b"null"), (7, b"null"), (8, b"null"), (9, b"null")):
        args = list(good)
        args[position] = None
        assert call(*args) < 0
        assert message in lib.dgs_mesh_ops_last_error(), position
    for change, message in (((0, -1), b"negative n"), ((0, 1 << 24), b"2^24"), ((4, 0), b"max_rounds"), ((4, -5), b"max_rounds"),
                            ((3, -1.0), b"inv_q"), ((3, float("inf")), b"inv_q"), ((3, float("nan")), b"inv_q"),
                            ((6, ctypes.sizeof(scratch) - 1), b"scratch")):
        args = list(good)
        args[change[0]] = change[1]
        assert call(*args) < 0
        assert message in lib.dgs_mesh_ops_last_error(), change
    args = list(good)
    args[5] = ctypes.c_void_p(ctypes.addressof(scratch) + 4)                  # misaligned
    assert call(*args) < 0 and b"aligned" in lib.dgs_mesh_ops_last_error()
    assert call(0, None, None, 1.0, 100, None, 0, None, None, p(result)) == 0   # no points: nothing to launch
    assert list(result) == [0] * lay[3]
