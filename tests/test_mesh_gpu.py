"""-m gpu: the HIP fuser and the HIP marching tetrahedra against the PyTorch / NumPy statements, a moving scene through the product
rasterizer, and extract_meshes on a short fit.  The margins quoted here are derived in profiles/mesh_parity_margins.md."""
import math
import os

import numpy as np
import pytest
import torch

from test_mesh_cpu import (C_S, R_S, assert_closed_sphere, fusion_inputs, marching_tets_reference, mesh_report, sphere_box,
                           spread_cameras)

pytestmark = pytest.mark.gpu
N6, VIEWS6, SIZE6 = 96, 24, 200


def _cpu_margin(prior_weight):
    """What float32 does to the PyTorch statement on these inputs, measured against its float64 run on the CPU: the share of voxels
    whose weight differs (an accept / reject decision on a threshold to rounding) and the largest tsdf / colour deviation elsewhere."""
    from dgs_amd.mesh import TSDFVolume
    origin, h = sphere_box(N6)
    out = []
    for dt in (torch.float64, torch.float32):
        depth, rgb, proj = fusion_inputs(VIEWS6, SIZE6, plate=True, dtype=dt)
        out.append(TSDFVolume(origin, h, (N6,) * 3, "cpu", prior_weight=prior_weight, dtype=dt).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0))
    v64, v32 = out
    flips = v64.weight != v32.weight.double()
    share = float(flips.double().mean())
    dev_t = float((v64.tsdf - v32.tsdf.double()).abs()[~flips].max())
    return share, dev_t, int(flips.sum())


@pytest.fixture(scope="module")
def fused():
    """The volume of test 6 on the device, fused by the HIP kernel in one call (prior_weight 0), and its inputs."""
    from dgs_amd.mesh import TSDFVolume
    origin, h = sphere_box(N6)
    depth, rgb, proj = (x.cuda() for x in fusion_inputs(VIEWS6, SIZE6, plate=True))
    vol = TSDFVolume(origin, h, (N6,) * 3, "cuda:0").integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    return vol, (depth, rgb, proj), origin, h


# ---- 6 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior_weight", [0.0, 1.0])
def test_hip_fuser_matches_the_pytorch_statement(prior_weight):
    """Measured on an MI355X (profiles/mesh_parity_margins.md): no weight differs, the colour is bit-identical and the tsdf agrees to
    3.0e-7 (prior 0) / 2.4e-7 (prior 1); the asserted caps come from the float32-vs-float64 runs of the PyTorch statement on the CPU."""
    from dgs_amd.mesh import TSDFVolume, integrate_torch
    share64, dev64, n64 = _cpu_margin(prior_weight)
    print("prior %g: float32 vs float64 on the CPU: %d voxels (share %.3e) differ in weight, max |dtsdf| elsewhere %.3e" % (prior_weight, n64, share64, dev64))
    assert share64 <= 2.5e-5, "the inputs put too many decisions on a threshold: change the inputs, not the cap"
    cap, bound = min(4 * share64, 1e-4), 8 * dev64
    origin, h = sphere_box(N6)
    depth, rgb, proj = (x.cuda() for x in fusion_inputs(VIEWS6, SIZE6, plate=True))
    hip = TSDFVolume(origin, h, (N6,) * 3, "cuda:0", prior_weight=prior_weight).integrate(depth, rgb, proj, trunc=5 * h, depth_trunc=6.0)
    ref = TSDFVolume(origin, h, (N6,) * 3, "cuda:0", prior_weight=prior_weight)
    t, w, c = integrate_torch(ref.tsdf, ref.weight, ref.color, ref.origin, ref.voxel_size, depth, rgb, proj, 5 * ref.voxel_size, 6.0)
    torch.cuda.synchronize()
    assert float((hip.weight - prior_weight).max()) > 5 and float(hip.weight.min()) == prior_weight      # the kernel did fuse, and left unseen voxels alone
    flips = hip.weight != w
    share = float(flips.double().mean())
    d_t = float((hip.tsdf - t).abs()[~flips].max())
    d_c = float((hip.color - c).abs()[~flips].max())
    print("prior %g: HIP vs PyTorch on the device: %d voxels (share %.3e, cap %.3e) differ in weight; elsewhere max |dtsdf| %.3e, max |dcolour| %.3e "
          "(bound %.3e)" % (prior_weight, int(flips.sum()), share, cap, d_t, d_c, bound))
    assert share <= cap
    assert torch.equal(hip.weight[~flips], w[~flips])
    assert d_t <= bound and d_c <= bound
    # three accumulate chunks == one call, bit for bit
    chunked = TSDFVolume(origin, h, (N6,) * 3, "cuda:0", prior_weight=prior_weight)
    for s in range(0, VIEWS6, 8):
        chunked.integrate(depth[s:s + 8], rgb[s:s + 8], proj[s:s + 8], trunc=5 * h, depth_trunc=6.0)
    assert torch.equal(chunked.tsdf, hip.tsdf) and torch.equal(chunked.weight, hip.weight) and torch.equal(chunked.color, hip.color)


def test_hip_fuser_is_safe_for_cameras_anywhere():
    """A camera inside the grid, one with everything behind it, a degenerate projection (all zeros) and one of NaNs: the kernel forms
    tap addresses only after the frustum test and only from clamped pixel indices, so such views are rejected as a whole and the
    result equals the PyTorch statement's bit for bit (grid dimensions that are no multiples of the brick: partial bricks too)."""
    from dgs_amd.cameras import make_camera, pose_spherical
    from dgs_amd.mesh import TSDFVolume, integrate_torch
    W = H = 32
    cams = [make_camera(pose_spherical(10.0, -30.0, 0.05), 2.0, 2.0, W, H, 0.0), make_camera(pose_spherical(-60.0, 20.0, 3.0), 0.7, 0.7, W, H, 0.0)]
    proj = torch.stack([c.full_proj_transform.reshape(16) for c in cams] + [torch.zeros(16), torch.full((16,), float("nan"))]).cuda()
    proj[1] = -proj[1]                                    # everything behind the camera
    g = torch.Generator().manual_seed(3)
    depth = (torch.rand(4, H, W, generator=g) * 3.0).cuda()
    rgb = torch.rand(4, 3, H, W, generator=g).cuda()
    vols = []
    for use_hip in (True, False):
        vol = TSDFVolume((-0.5, -0.5, -0.5), 1.0 / 37, (38, 35, 33), "cuda:0")
        if use_hip:
            vol.integrate(depth, rgb, proj, trunc=0.2, depth_trunc=6.0)
        else:
            vol.tsdf, vol.weight, vol.color = integrate_torch(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size, depth, rgb, proj, 0.2, 6.0)
        vols.append(vol)
    torch.cuda.synchronize()
    hip, ref = vols
    assert float(hip.weight.max()) == 1.0 and 0 < float(hip.weight.mean()) < 1      # only the camera inside the grid is accepted anywhere
    assert torch.equal(hip.weight, ref.weight) and torch.equal(hip.tsdf, ref.tsdf) and torch.equal(hip.color, ref.color)
    assert bool(torch.isfinite(hip.tsdf).all()) and bool(torch.isfinite(hip.color).all())


# ---- 7 --------------------------------------------------------------------------------------------------------------------------
def test_hip_marching_tetrahedra_matches_the_numpy_statement(fused):
    from dgs_amd.mesh import keep_largest_components
    vol, _, _, _ = fused
    v, f, c = vol.extract()
    torch.cuda.synchronize()
    assert v.is_cuda and f.dtype == torch.int32 and c.shape == v.shape
    V, F = v.cpu().numpy(), f.cpu().numpy()
    Vr, Fr, keys = marching_tets_reference(vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.origin, vol.voxel_size)
    print("HIP marching tetrahedra: %d vertices, %d faces (NumPy statement: %d, %d)" % (len(V), len(F), len(Vr), len(Fr)))
    assert V.shape == Vr.shape and F.shape == Fr.shape and len(F) > 100000
    assert np.array_equal(F, Fr)
    err = np.abs(V - Vr) / np.maximum(1.0, np.abs(Vr))
    print("max vertex deviation %.3e (allowed %.3e)" % (err.max(), 8 * 2.0 ** -24))
    assert err.max() <= 8 * 2.0 ** -24
    assert float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    # the CPU path of the same class on the same volume: identical arrays
    from dgs_amd.mesh import TSDFVolume
    cpu = TSDFVolume(vol.origin, vol.voxel_size, vol.dims, "cpu")
    cpu.tsdf, cpu.weight, cpu.color = vol.tsdf.cpu(), vol.weight.cpu(), vol.color.cpu()
    v2, f2, c2 = cpu.extract()
    assert np.array_equal(f2.numpy(), F) and np.array_equal(v2.numpy(), V) and np.abs(c2.numpy() - c.cpu().numpy()).max() <= 1e-6
    # the sphere is the largest component (the plate is a one-sided sheet that leaves the box): closed, oriented, chi = 2
    vs, fs, _ = keep_largest_components(V, F, None, n_keep=1)
    assert_closed_sphere(vs.numpy(), fs.numpy())
    dist = np.abs(np.linalg.norm(vs.numpy().astype(np.float64) - C_S, axis=1) - R_S) / vol.voxel_size
    print("sphere component: %d vertices, distance max %.3f h (views that see the plate's rim in front of the sphere interpolate between "
          "two valid depths there: this is the fusion's error, the same on both paths)" % (vs.shape[0], dist.max()))
    assert fs.shape[0] < F.shape[0]                       # the plate is in the mesh as well


# ---- 8 --------------------------------------------------------------------------------------------------------------------------
H8 = 0.02
ORIGIN8, DIMS8 = (-1.3, -0.8, -1.0), (140, 81, 101)
# the CPU path with the oracle rasterizer at the same size (profiles/mesh_parity_margins.md), in voxels: {t: (max, p95)}
ORACLE_DIST8 = {0.25: (0.7493, 0.3599), 0.75: (0.8173, 0.3649)}


def truth_model(t, device):
    """DynamicTruth().state(t) as a SurfelModel (no deformation: the state already is the scene at time t)."""
    from dgs_amd.model import SurfelModel
    from dgs_amd.synthetic import DynamicTruth, SurfelScene
    xyz, scales, rot, opac, shs = DynamicTruth().state(t)
    scene = SurfelScene(xyz, scales.log(), rot, torch.logit(opac), shs[:, :1].contiguous(), shs[:, 1:].contiguous(), torch.zeros(xyz.shape[0], 8))
    return SurfelModel(scene).to(device)


def truth_mesh(t, device, rasterizer_cls=None):
    from dgs_amd.mesh import TSDFVolume, views_at_time
    model = truth_model(t, device)
    cams = spread_cameras(40, 200, 200, t=t)
    depth, rgb, proj = views_at_time(model, None, cams, t, torch.zeros(3, device=device), alpha_min=0.5, rasterizer_cls=rasterizer_cls)
    assert depth.shape == (40, 200, 200) and rgb.shape == (40, 3, 200, 200) and proj.shape == (40, 16) and depth.device.type == torch.device(device).type
    vol = TSDFVolume(ORIGIN8, H8, DIMS8, device).integrate(depth, rgb, proj, trunc=5 * H8, depth_trunc=6.0)
    v, f, c = vol.extract()
    return v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()


def sphere_side(V, F):
    """The largest connected component among the faces whose vertices all have x < 0.1, and the other components' face counts."""
    from dgs_amd.mesh import vertex_components
    left = V[:, 0] < 0.1
    fl = left[F]
    assert not (fl.any(1) & ~fl.all(1)).any(), "a face mixes the sphere's side and the plate's"
    Fs = F[fl.all(1)]
    lab = vertex_components(V.shape[0], Fs)[Fs[:, 0]]
    ids, counts = np.unique(lab, return_counts=True)
    main = Fs[lab == ids[np.argmax(counts)]]
    return main, sorted(counts.tolist())[:-1]


def test_mesh_of_a_moving_scene_through_the_product_rasterizer():
    from dgs_amd.mesh import keep_largest_components
    centroid = {}
    for t in (0.25, 0.75):
        V, F, C = truth_mesh(t, "cuda:0")
        main, others = sphere_side(V, F)
        used = np.unique(main)
        assert_closed_sphere(V, main, "t = %g" % t)
        centre = np.array([-0.55, 0.0, 0.25 * math.sin(2 * math.pi * t)])
        dist = np.abs(np.linalg.norm(V[used].astype(np.float64) - centre, axis=1) - 0.55) / H8
        centroid[t] = V[used].astype(np.float64).mean(0)
        print("t = %g: %d vertices, %d faces; sphere component %d faces, other components on its side %s; distance max %.4f h, p95 %.4f h "
              "(oracle: %.4f, %.4f); centroid %s" % (t, len(V), len(F), len(main), others, dist.max(), np.quantile(dist, 0.95), *ORACLE_DIST8[t], centroid[t]))
        assert dist.max() <= ORACLE_DIST8[t][0] + 0.5 and np.quantile(dist, 0.95) <= ORACLE_DIST8[t][1] + 0.5
        # colours: the sphere's are 0.5 + 0.45 sin(4 n + phase) of the outward normal n
        n = (V[used].astype(np.float64) - centre) / 0.55
        want = 0.5 + 0.45 * np.sin(4.0 * n + np.array([0.0, 2.0, 4.0]))
        assert np.abs(C[used] - want).mean() < 0.08
        # floaters smaller than the filter's default minimum are gone after it
        vk, fk, _ = keep_largest_components(V, F, C)
        small = [n_ for n_ in others if n_ < 50]
        if small:
            main_k, others_k = sphere_side(vk.numpy(), fk.numpy())
            assert len(main_k) == len(main) and not [n_ for n_ in others_k if n_ < 50]
    dz = centroid[0.25][2] - centroid[0.75][2]
    print("centroid z(0.25) - z(0.75) = %.5f" % dz)
    assert abs(dz - 0.5) <= 2 * H8                         # the mesh is of time t, not of one fixed state


# ---- 9 --------------------------------------------------------------------------------------------------------------------------
def test_extract_meshes_on_a_short_fit(tmp_path):
    from dgs_amd.fit import fit
    from dgs_amd.io import read_mesh_ply
    from dgs_amd.mesh import extract_meshes, main
    from dgs_amd.synthetic import write_dynamic_dnerf
    data, model = str(tmp_path / "scene"), str(tmp_path / "model")
    write_dynamic_dnerf(data, n_train=24, n_test=3, H=128, W=128, device="cuda:0")
    fit(data, model, iterations=300, device="cuda:0", num_pts=5000, node_num=128, seed=0, warm_up=100, regularize_from=180, densify_from=100,
        densify_interval=50, opacity_reset_interval=10_000)
    logs = []
    files = extract_meshes(model, data, times=[0.2, 0.7], voxel_size=0.03, device="cuda:0", log=logs.append)
    assert [os.path.relpath(p, model) for p in files] == ["train/ours_300/frame_0.ply", "train/ours_300/frame_1.ply"] and len(logs) == 2
    for p in files:
        v, f, c = read_mesh_ply(p)
        print(p, v.shape, f.shape)
        assert v.shape[0] > 0 and f.shape[0] > 0 and c.shape == v.shape
        assert f.min() >= 0 and f.max() < v.shape[0] and np.isfinite(v).all()
        assert np.abs(v).max() < 3.0
    # default times: the test split's; the command line goes the same way
    main([model, data, "--voxel-size", "0.05", "--out-dir", str(tmp_path / "cli")])
    assert sorted(os.listdir(str(tmp_path / "cli"))) == ["frame_0.ply", "frame_1.ply", "frame_2.ply"]
