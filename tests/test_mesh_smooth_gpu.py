"""-m gpu: dgs_smooth_steps and dgs_amd.mesh_smooth on a HIP device against the CPU statement.  Every comparison is exact: the
integer adjacency, and the fp32 bit patterns of vertices and colours."""
import pytest
import torch

from test_mesh_cpu import fusion_inputs, sphere_box
from test_mesh_simplify_cpu import analytic_mesh, same_bits
from test_mesh_smooth_cpu import noisy_sphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check_adjacency(V, f):
    """vertex_adjacency and boundary_vertices built on the device against the CPU's; -> the CPU's (offsets, neighbours)."""
    from dgs_amd.mesh_smooth import boundary_vertices, vertex_adjacency
    off, nb = vertex_adjacency(V, f)
    d_off, d_nb = vertex_adjacency(V, f.to(DEV))
    assert d_off.is_cuda and d_nb.is_cuda and d_off.dtype == off.dtype and d_nb.dtype == nb.dtype
    assert torch.equal(d_off.cpu(), off) and torch.equal(d_nb.cpu(), nb)
    assert torch.equal(boundary_vertices(V, f.to(DEV)).cpu(), boundary_vertices(V, f))
    return off, nb


def check_mesh(v, f, c=None, **kw):
    """smooth_mesh on the device against the CPU run; -> the CPU result."""
    from dgs_amd.mesh_smooth import smooth_mesh
    want = smooth_mesh(v, f, c, **kw)
    kw = {k: (x.to(DEV) if torch.is_tensor(x) else x) for k, x in kw.items()}
    got = smooth_mesh(v.to(DEV), f.to(DEV), None if c is None else c.to(DEV), **kw)
    assert all(x.is_cuda for x in got if x is not None)
    same_bits(got, want)
    return want


def check_steps(off, nb, x, mode, factors, pinned=None):
    """The raw binding, in place on a device copy of x, against the statement; a second call on the same buffers (x restored, tmp
    as the first call left it) gives the same bits.  -> the statement's result."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_smooth import smooth_steps_torch
    want = smooth_steps_torch(off, nb, x, mode, factors, pinned)
    d_off, d_nb, d_pin = off.to(DEV), nb.to(DEV), None if pinned is None else pinned.to(DEV)
    buf, tmp = x.to(DEV), torch.full(x.shape, float("nan"), device=DEV)
    out = _mesh_ops.smooth_steps(d_off, d_nb, buf, mode, factors, d_pin, tmp)
    assert out is buf                                              # the result is in x, for an odd and for an even count
    same_bits((buf,), (want,))
    buf.copy_(x.to(DEV))
    _mesh_ops.smooth_steps(d_off, d_nb, buf, mode, factors, d_pin, tmp)
    same_bits((buf,), (want,))
    return want


# ---- the analytic shapes and an extracted mesh -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["sphere", "cube"])
def test_analytic_shapes(shape):
    v, f, c, h = analytic_mesh(shape)
    if shape == "sphere":
        v = noisy_sphere()[4]
    off, nb = check_adjacency(v.shape[0], f)
    assert 4 <= int((off[1:] - off[:-1]).min()) and int((off[1:] - off[:-1]).max()) <= 10
    for method in ("taubin", "laplacian", "simple"):
        out = check_mesh(v, f, c, method=method, iterations=10)
        assert not torch.equal(out[0], v)
        check_mesh(v, f.long(), c, method=method, iterations=3, smooth_colors=True, pin_boundary=True)
    # an open mesh, so that pin_boundary pins something: the half x >= 0
    half = f[(v[f.long()][:, :, 0] >= 0).all(1)]
    from dgs_amd.mesh_smooth import boundary_vertices
    assert 0 < int(boundary_vertices(v.shape[0], half).sum()) < v.shape[0]
    check_adjacency(v.shape[0], half)
    for method in ("taubin", "laplacian", "simple"):
        a = check_mesh(v, half, c, method=method, iterations=4, pin_boundary=True, smooth_colors=True)
        b = check_mesh(v, half, c, method=method, iterations=4, lam=0.3, mu=-0.34)
        assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], c)


@pytest.fixture(scope="module")
def device_mesh():
    """The recipe of tests/test_mesh_simplify_gpu.py: the sphere and the plate of tests/test_mesh_cpu.py fused at 96^3 from 24 views
    of 200^2 and extracted on the device; here as CPU tensors."""
    from dgs_amd.mesh import TSDFVolume
    N = 96
    origin, h = sphere_box(N)
    depth, rgb, proj = (x.to(DEV) for x in fusion_inputs(24, 200, plate=True))
    v, f, c = TSDFVolume(origin, h, (N,) * 3, DEV).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0).extract()
    assert v.is_cuda and f.shape[0] > 10000
    return v.cpu(), f.cpu(), c.cpu(), h


def test_a_mesh_extracted_on_the_device(device_mesh):
    """taubin x 10, then simplify_mesh of the result: both stages bit-identical to the CPU."""
    from dgs_amd.mesh_simplify import simplify_mesh
    v, f, c, h = device_mesh
    check_adjacency(v.shape[0], f)
    sv, sf, sc = check_mesh(v, f, c, method="taubin", iterations=10)
    assert not torch.equal(sv, v) and torch.isfinite(sv).all()
    want = simplify_mesh(sv, sf, sc, cell_size=2 * h)
    got = simplify_mesh(sv.to(DEV), sf.to(DEV), sc.to(DEV), cell_size=2 * h)
    same_bits(got, want)
    print("extracted mesh: %d vertices, %d -> %d faces" % (v.shape[0], f.shape[0], want[1].shape[0]))
    assert want[1].shape[0] * 6 < f.shape[0]


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def test_layout_boundaries():
    """V at 1, at one workgroup - 1, + 0, + 1 and at a ragged second workgroup, with random faces; the last vertex has neighbours and
    must move."""
    from dgs_amd import _mesh_ops
    per_group = _mesh_ops.smooth_layout()[1]
    g = torch.Generator().manual_seed(3)
    one = check_mesh(torch.rand((1, 3), generator=g), torch.zeros((1, 3), dtype=torch.int32), method="laplacian", iterations=3)
    assert one[0].shape == (1, 3)
    for V in (per_group - 1, per_group, per_group + 1, 2 * per_group - 37):
        v, c = torch.rand((V, 3), generator=g), torch.rand((V, 3), generator=g)
        f = torch.randint(0, V, (2 * V, 3), generator=g, dtype=torch.int32)
        f[-1] = torch.tensor([V - 1, 0, V // 2])
        check_adjacency(V, f)
        for method in ("taubin", "simple"):
            out = check_mesh(v, f, c, method=method, iterations=2, smooth_colors=True)
            assert not torch.equal(out[0][-1], v[-1]) and not torch.equal(out[2][-1], c[-1])


# ---- rows --------------------------------------------------------------------------------------------------------------------------
def test_row_shapes_in_one_mesh():
    """An isolated vertex, a vertex of degree 1, a fan whose hub has degree 5 000, repeated faces and a face naming a vertex twice.
    Vertex 0 is the hub, 1..5000 its rim, 5001 hangs on the rim by the face (5000, 5001, 5001), 5002 is isolated."""
    n = 5000
    g = torch.Generator().manual_seed(8)
    rim = torch.arange(1, n + 1)
    fan = torch.stack((torch.zeros(n, dtype=torch.int64), rim, torch.roll(rim, -1)), 1)
    f = torch.cat((fan, fan[:50], torch.tensor([[n, n + 1, n + 1], [7, 7, 7]]))).to(torch.int32)
    v, c = torch.rand((n + 3, 3), generator=g), torch.rand((n + 3, 3), generator=g)
    off, nb = check_adjacency(n + 3, f)
    d = (off[1:] - off[:-1]).tolist()
    assert d[0] == n and d[n + 1] == 1 and d[n + 2] == 0 and d[n] == 4 and d[1] == 3
    for method, it in (("taubin", 2), ("laplacian", 3), ("simple", 2)):
        out = check_mesh(v, f, c, method=method, iterations=it, smooth_colors=True)
        assert torch.equal(out[0][n + 2], v[n + 2]) and not torch.equal(out[0][n + 1], v[n + 1]) and not torch.equal(out[0][0], v[0])
    pin = torch.zeros(n + 3, dtype=torch.bool)
    pin[0] = True
    out = check_mesh(v, f, None, method="laplacian", iterations=2, pinned=pin)
    assert torch.equal(out[0][0], v[0])


# ---- the raw binding ---------------------------------------------------------------------------------------------------------------
def random_rows(V, n_faces, seed):
    from dgs_amd.mesh_smooth import vertex_adjacency
    g = torch.Generator().manual_seed(seed)
    return vertex_adjacency(V, torch.randint(0, V, (n_faces, 3), generator=g, dtype=torch.int32)) + (g,)


def test_step_counts():
    """1, 2 and 7 steps, then the layout's cap: an odd count ends with the copy, and the result is in x every time."""
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_smooth import MODE_LAPLACIAN, MODE_SIMPLE
    cap = _mesh_ops.smooth_layout()[3]
    V = 300
    off, nb, g = random_rows(V, 500, seed=12)
    x = torch.rand((V, 3), generator=g)
    pinned = torch.rand(V, generator=g) < 0.1
    for n in (1, 2, 7):
        check_steps(off, nb, x, MODE_LAPLACIAN, [0.5, -0.53, 0.25, 0.1, -0.2, 0.7, 0.33][:n], pinned)
        check_steps(off, nb, x, MODE_SIMPLE, [0.0] * n)
    out = check_steps(off, nb, x, MODE_LAPLACIAN, [0.5, -0.53] * (cap // 2))
    assert torch.isfinite(out).all()
    with pytest.raises(RuntimeError, match="n_steps"):
        _mesh_ops.smooth_steps(off.to(DEV), nb.to(DEV), x.to(DEV), MODE_LAPLACIAN, [0.1] * (cap + 1))
    # smooth_mesh takes more steps than one call does
    from dgs_amd.mesh_smooth import smooth_mesh, smooth_steps_torch
    f = torch.randint(0, 40, (60, 3), generator=g, dtype=torch.int32)
    v = torch.rand((40, 3), generator=g)
    got = smooth_mesh(v.to(DEV), f.to(DEV), method="laplacian", iterations=cap + 3, lam=0.05)
    same_bits(got, smooth_mesh(v, f, method="laplacian", iterations=cap + 3, lam=0.05))


@pytest.mark.parametrize("C", [1, 3, 6, 8])
def test_channels(C):
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_smooth import MODE_LAPLACIAN, MODE_SIMPLE
    V = 2 * _mesh_ops.smooth_layout()[1] + 11
    off, nb, g = random_rows(V, 3 * V, seed=20 + C)
    x = torch.randn((V, C), generator=g) * 100.0
    pinned = torch.rand(V, generator=g) < 0.2
    a = check_steps(off, nb, x, MODE_LAPLACIAN, [0.5, -0.53, 0.9], pinned)
    b = check_steps(off, nb, x, MODE_SIMPLE, [0.0, 0.0])
    assert not torch.equal(a, x) and not torch.equal(b, x) and torch.equal(a[pinned], x[pinned])
    with pytest.raises(RuntimeError):
        _mesh_ops.smooth_steps(off.to(DEV), nb.to(DEV), torch.zeros((V, 9), device=DEV), MODE_SIMPLE, [0.0])
