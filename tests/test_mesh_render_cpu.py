"""-m "not gpu": the PyTorch statement of the mesh rasterizer (dgs_amd.mesh_render) on the CPU against a float64 brute force and
against closed forms, the images built on it, render_meshes on a hand-written dataset, and the argument checks of the C ABI."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_raster_ref as ref

U32 = ref.U32


def _camera_on_axis(size, radius=4.0):
    """A camera looking at the origin from distance `radius`; the principal point is the screen point ((size - 1) / 2, same)."""
    return ref.orbit_camera(size, size, theta=20.0, phi=-40.0, radius=radius)


def _origin_sphere(nu=32, nv=16, radius=0.8):
    v, f, c = ref.sphere(nu, nv, radius, (0.0, 0.0, 0.0))
    return v, f, c


# ---- the statement against float64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ref.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ref.CASES)
def test_statement_against_float64_brute_force(name, size):
    """Observed (fp32 statement on the CPU, all cases): depth 1.3e-6 relative at most (cap 32 * 2^-24 = 1.9e-6), barycentrics at
    most 0.25 of their bound, colours at most 0.06 of theirs; at most 4 pixels of a case fall into the exclusion set."""
    from dgs_amd.mesh_render import rasterize
    H, W = size
    cam, v, f, c, r64 = ref.case(name, H, W)
    out = rasterize(v, f, cam, attr=c)
    assert out["face"].dtype == torch.int32 and out["depth"].dtype == torch.float32 and out["image"].shape == (3, H, W)
    ref.compare_with_float64("%s %dx%d" % (name, H, W), out, out["image"], r64, W, H)


def test_closed_sphere_is_watertight():
    """No uncovered pixel with four covered 4-neighbours: neighbouring faces leave no crack."""
    from dgs_amd.mesh_render import rasterize
    for name in ("sphere", "sphere unwelded", "sphere coarse"):
        for H, W in ref.SIZES:
            cam, v, f, _, _ = ref.case(name, H, W)
            hit = (rasterize(v, f, cam)["face"] >= 0).numpy()
            hole = ~hit[1:-1, 1:-1] & hit[:-2, 1:-1] & hit[2:, 1:-1] & hit[1:-1, :-2] & hit[1:-1, 2:]
            assert hit.sum() > 100 and not hole.any(), (name, H, W, np.argwhere(hole)[:4])


def test_welded_and_unwelded_meshes_give_identical_maps():
    from dgs_amd.mesh_render import rasterize
    for H, W in ref.SIZES:
        cam, v, f, c, _ = ref.case("sphere", H, W)
        _, v2, f2, c2, _ = ref.case("sphere unwelded", H, W)
        a, b = rasterize(v, f, cam, attr=c), rasterize(v2, f2, cam, attr=c2)
        assert torch.equal(a["face"], b["face"]) and torch.equal(a["depth"].view(torch.int32), b["depth"].view(torch.int32))
        assert torch.equal(a["image"], b["image"])


def test_equal_depths_go_to_the_lowest_face():
    from dgs_amd.mesh_render import rasterize
    cam = ref.pixel_camera(16, 20)
    tri = torch.tensor([[2.3, 1.7, 1.0], [17.1, 3.2, 1.0], [6.4, 13.9, 1.0]]) * 2.0
    far = tri * 1.5                                                         # the same screen triangle, farther away
    v = torch.cat([far, tri, tri, tri])
    f = torch.arange(12).reshape(4, 3)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]):
        out = rasterize(v, f[order], cam)
        hit = out["face"] >= 0
        want = min(i for i, o in enumerate(order) if o != 0)                # the first of the three coincident near faces
        assert int(hit.sum()) > 40 and bool((out["face"][hit] == want).all()), order
        assert float((out["depth"][hit] - 2.0).abs().max()) <= 4 * 2.0 * U32


def test_dropped_faces_are_never_drawn():
    from dgs_amd.mesh_render import raster_table, rasterize
    H, W = 16, 20
    cam = ref.pixel_camera(H, W)
    px = lambda x, y, z: [x * z, y * z, z]
    v = torch.tensor([px(2, 2, 1.0), px(15, 3, 1.0), px(6, 13, 0.005),      # a corner behind near (w = 0.005 <= 0.01)
                      px(2, 5, 1.0), px(8, 5, 1.0), px(14, 5, 1.0),         # zero area: collinear (one image row)
                      px(3, 9, 1.0), px(3, 9, 1.0), px(12, 4, 1.0),         # a repeated vertex
                      px(-30, 2, 1.0), px(-10, 3, 1.0), px(-20, 14, 1.0),   # entirely off-screen (left)
                      px(5, 40, 1.0), px(15, 45, 1.0), px(8, 60, 1.0)])     # entirely off-screen (below)
    f = torch.arange(15).reshape(5, 3)
    table, box = raster_table(v, f, cam)
    assert box.tolist() == [[0, -1, 0, -1]] * 5
    assert table[:3, 15].tolist() == [0.0, 0.0, 0.0] and table[3:, 15].abs().tolist() == [1.0, 1.0]
    out = rasterize(v, f, cam, attr=torch.ones(15, 1), background=torch.tensor([0.25]))
    assert bool((out["face"] == -1).all()) and bool((out["depth"] == 0).all()) and bool((out["image"] == 0.25).all())
    # the same faces next to a visible one: only that one is drawn
    v2 = torch.cat([v, torch.tensor([px(4, 3, 2.0), px(16, 5, 2.0), px(9, 12, 2.0)])])
    f2 = torch.cat([f, torch.tensor([[15, 16, 17]])])
    out = rasterize(v2, f2, cam)
    assert set(out["face"].unique().tolist()) == {-1, 5}
    # a corner exactly at near is dropped, one just above is drawn
    for z, drawn in ((0.01, False), (0.0100001, True)):
        v3 = torch.tensor([px(2, 2, 1.0), px(15, 3, 1.0), px(6, 13, z)])
        assert bool((rasterize(v3, torch.tensor([[0, 1, 2]]), cam)["face"] >= 0).any()) == drawn


def test_a_pixel_whose_depth_is_nan_is_not_covered():
    """An edge function that overflows to an infinity passes the sign tests and gives b = inf / inf: the coverage rule q > 0 keeps
    such a pixel empty, next to a face that is drawn as usual."""
    from dgs_amd.mesh_render import VALUES, _pair, _pixels, raster_table, rasterize
    H, W = 16, 20
    cam = ref.pixel_camera(H, W)
    v, f = ref.overflowing_face()
    table, box = raster_table(v, f, cam)
    assert box.tolist() == [[0, W - 1, 0, H - 1]] and float(table[0, 15]) == 1.0          # a valid face over the whole image
    _, _, px, py = _pixels(H, W, "cpu", torch.float32)
    col = table[:, :VALUES].t().contiguous().unsqueeze(2)
    e0 = col[12] * (col[2] * (py[None] - col[1]) - col[3] * (px[None] - col[0]))
    inside, _, z = _pair(col, px[None], py[None])
    assert bool(torch.isinf(e0).all()) and bool(torch.isnan(z).all()) and not bool(inside.any())
    out = rasterize(v, f, cam, attr=torch.ones(3, 2), background=torch.tensor([0.25, 0.5]))
    assert bool((out["face"] == -1).all()) and bool((out["depth"] == 0).all()) and bool((out["image"][1] == 0.5).all())
    v2 = torch.cat([v, torch.tensor([[4.0, 3.0, 1.0], [16.0, 5.0, 1.0], [9.0, 12.0, 1.0]]) * 2.0])
    out = rasterize(v2, torch.tensor([[0, 1, 2], [3, 4, 5]]), cam, attr=torch.rand(6, 3, generator=torch.Generator().manual_seed(0)))
    assert set(out["face"].unique().tolist()) == {-1, 1} and bool(torch.isfinite(out["image"]).all()) and bool(torch.isfinite(out["depth"]).all())


def test_half_off_screen_face_is_drawn_inside_the_image_only():
    from dgs_amd.mesh_render import raster_table, rasterize
    H, W = 16, 20
    cam = ref.pixel_camera(H, W)
    v = torch.tensor([[-12.5, 3.5, 1.0], [11.5, -9.5, 1.0], [9.5, 30.5, 1.0]])
    f = torch.tensor([[0, 1, 2]])
    _, box = raster_table(v, f, cam)
    assert box.tolist() == [[0, 11, 0, H - 1]]
    r64 = ref.brute_force64(v, f, cam)
    out = rasterize(v, f, cam)
    keep = ~r64["excluded"]
    assert np.array_equal((out["face"].numpy() >= 0)[keep], (r64["face"] >= 0)[keep]) and 50 < int((out["face"] >= 0).sum()) < H * W
    assert not bool((out["face"][:, 12:] >= 0).any())


# ---- closed forms ---------------------------------------------------------------------------------------------------------------
def test_sphere_against_its_projected_disc_and_centre_depth():
    from dgs_amd.mesh_render import rasterize
    size, d, R, nu, nv = 97, 4.0, 0.8, 32, 16
    cam = _camera_on_axis(size, d)
    v, f, _ = _origin_sphere(nu, nv, R)
    out = rasterize(v, f, cam)
    hit = (out["face"] >= 0).numpy()
    focal = size / (2 * math.tan(cam.FoVx / 2))
    rho = focal * R / math.sqrt(d * d - R * R)                              # the silhouette of the exact sphere: a circle round the centre
    shrink = math.cos(math.pi / nu) * math.cos(math.pi / nv)                # the inscribed polyhedron reaches at least this far
    c = (size - 1) / 2
    yy, xx = np.mgrid[0:size, 0:size]
    r = np.hypot(xx - c, yy - c)
    disc, core = r <= rho, r <= focal * R * shrink / math.sqrt(d * d - (R * shrink) ** 2) - 1e-3
    boundary = int(disc.sum() - core.sum())
    print("disc %d pixels, covered %d, boundary ring %d" % (disc.sum(), hit.sum(), boundary))
    assert not (hit & ~(r <= rho + 1e-3)).any() and not (core & ~hit).any()
    assert abs(int(hit.sum()) - int(disc.sum())) <= boundary
    sagitta = R * (1 - shrink)
    centre_depth = float(out["depth"][size // 2, size // 2])
    print("centre depth %.6f, distance - radius %.6f, facet sagitta %.6f" % (centre_depth, d - R, sagitta))
    assert abs(centre_depth - (d - R + 0.5 * sagitta)) <= 0.5 * sagitta + 1e-5


def test_vertex_normals_of_a_sphere_point_outwards():
    from dgs_amd.mesh_render import vertex_normals
    nu, nv = 32, 16
    v, f, _ = _origin_sphere(nu, nv, 0.8)
    n = vertex_normals(v, f)
    assert n.dtype == torch.float32 and n.shape == v.shape
    cos = (n.double() * (v.double() / 0.8)).sum(1)
    assert float((n.norm(dim=1) - 1).abs().max()) <= 1e-6
    assert float(cos.min()) >= math.cos(max(2 * math.pi / nu, math.pi / nv))    # within one facet angle of the outward normal
    assert torch.equal(n, vertex_normals(v, f))                                 # deterministic
    # a vertex no face touches gets the zero vector
    assert vertex_normals(torch.cat([v, torch.zeros(1, 3)]), f)[-1].tolist() == [0.0, 0.0, 0.0]


def test_shape_image_is_brightest_where_the_normal_faces_the_camera():
    from dgs_amd.mesh_render import rasterize, render_mesh_shape
    size = 97
    cam = _camera_on_axis(size)
    v, f, _ = _origin_sphere()
    img = render_mesh_shape(cam, v, f)
    hit = rasterize(v, f, cam)["face"] >= 0
    assert img.shape == (3, size, size) and torch.equal(img[0], img[1]) and torch.equal(img[0], img[2])
    assert bool((img[0][~hit] == 1.0).all())                                # exactly white outside the silhouette
    inside = torch.where(hit, img[0], torch.zeros_like(img[0]))
    y, x = divmod(int(inside.argmax()), size)
    assert abs(y - size // 2) <= 2 and abs(x - size // 2) <= 2
    assert abs(float(inside.max()) - (0.5 + 0.3 + 0.04)) <= 2e-3            # n = l = v = r at the centre
    assert float(img[0][hit].min()) >= 0.5 - 1e-6                           # ambient everywhere
    rim = hit & ~(torch.roll(hit, 3, 0) & torch.roll(hit, -3, 0) & torch.roll(hit, 3, 1) & torch.roll(hit, -3, 1))
    assert float(img[0][rim].max()) < float(inside.max()) - 0.1             # darker towards the silhouette


def test_supersample_is_the_block_mean_of_the_larger_render():
    from dgs_amd.mesh_render import render_mesh, render_mesh_shape
    H, W = 37, 53
    cam, v, f, c, _ = ref.case("sphere coarse", H, W)
    big = render_mesh(cam._replace(image_height=2 * H, image_width=2 * W), v, f, c)
    ss = render_mesh(cam, v, f, c, supersample=2)
    mean = lambda x: x.reshape(x.shape[0], H, 2, W, 2).mean(dim=(2, 4))
    assert torch.equal(ss["render"], mean(big["render"])) and torch.equal(ss["alpha"], mean(big["alpha"]))
    assert float((ss["render"] - torch.nn.functional.avg_pool2d(big["render"][None], 2)[0]).abs().max()) <= 1e-6
    assert ss["render"].shape == (3, H, W) and ss["face"].shape == (H, W) and ss["depth"].shape == (1, H, W)
    partial = (ss["alpha"] > 0) & (ss["alpha"] < 1)
    assert bool(partial.any()) and bool((ss["depth"][ss["alpha"] > 0] > 3.0).all())      # edges are blended; depth is a mean over hits only
    one = render_mesh(cam, v, f, c)
    assert bool(((one["alpha"] == 0) | (one["alpha"] == 1)).all()) and bool((one["render"][:, one["alpha"][0] == 0] == 1.0).all())
    assert render_mesh_shape(cam, v, f, supersample=2).shape == (3, H, W)
    with pytest.raises(ValueError):
        render_mesh(cam, v, f, c, supersample=0)


def test_zero_faces_and_bad_meshes():
    from dgs_amd.mesh_render import rasterize, render_mesh
    cam = ref.pixel_camera(5, 7)
    out = render_mesh(cam, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int64), torch.zeros(0, 3))
    assert bool((out["render"] == 1).all()) and bool((out["face"] == -1).all()) and bool((out["alpha"] == 0).all())
    v = torch.tensor([[1.0, 1.0, 1.0], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0]])
    for bad_v, bad_f in ((v, torch.tensor([[0, 1, 3]])), (v, torch.tensor([[0.0, 1.0, 2.0]])), (v * float("nan"), torch.tensor([[0, 1, 2]])),
                         (v[:, :2], torch.tensor([[0, 1, 2]]))):
        with pytest.raises(ValueError):
            rasterize(bad_v, bad_f, cam)


# ---- the product step -----------------------------------------------------------------------------------------------------------
def _write_dataset(path, n_test, size=24):
    """A hand-written D-NeRF dataset: transforms_{train,test}.json and tiny RGBA PNGs."""
    from PIL import Image
    from dgs_amd.cameras import pose_spherical
    g = np.random.default_rng(5)
    for split, n in (("train", 2), ("test", n_test)):
        os.makedirs(os.path.join(path, split), exist_ok=True)
        frames = []
        for k in range(n):
            rgba = g.integers(0, 256, (size, size, 4), dtype=np.uint8)
            rgba[..., 3] = np.where(np.hypot(*np.mgrid[0:size, 0:size] - size / 2) < size / 3, 255, 0)
            Image.fromarray(rgba, "RGBA").save(os.path.join(path, split, "r_%03d.png" % k))
            frames.append({"file_path": "./%s/r_%03d" % (split, k), "time": k / max(n - 1, 1),
                           "transform_matrix": pose_spherical(-120.0 + 70.0 * k, -25.0 - 5.0 * k, 4.0).tolist()})
        with open(os.path.join(path, "transforms_%s.json" % split), "w") as fh:
            json.dump({"camera_angle_x": 0.6911, "frames": frames}, fh)


def _write_meshes(mesh_dir, n):
    from dgs_amd.io import write_mesh_ply
    for i in range(n):
        v, f, c = ref.sphere(16, 8, 0.6 + 0.1 * i, (0.1 * i, 0.0, 0.05))
        write_mesh_ply(os.path.join(mesh_dir, "frame_%d.ply" % i), v, f.int(), c)


def test_render_meshes_and_cli(tmp_path):
    from PIL import Image
    from dgs_amd.evaluate import to_uint8
    from dgs_amd.io import load_dnerf, read_mesh_ply
    from dgs_amd.mesh_render import main, render_mesh, render_meshes
    data, model = str(tmp_path / "data"), str(tmp_path / "model")
    mesh_dir = os.path.join(model, "train", "ours_7")
    _write_dataset(data, 3)
    _write_meshes(mesh_dir, 3)
    res = render_meshes(mesh_dir, data, device="cpu")
    # out_dir defaults to the model directory; evaluate()'s and evaluate_meshes' files are not touched (none exist here)
    assert sorted(os.listdir(model)) == ["mesh_image", "mesh_render_per_view.json", "mesh_render_results.json", "mesh_shape", "train"]
    names = ["%05d.png" % i for i in range(3)]
    assert sorted(os.listdir(os.path.join(model, "mesh_image"))) == names and sorted(os.listdir(os.path.join(model, "mesh_shape"))) == names
    results = json.load(open(os.path.join(model, "mesh_render_results.json")))
    per_view = json.load(open(os.path.join(model, "mesh_render_per_view.json")))
    assert set(results) == {"PSNR", "SSIM", "MS-SSIM"} and set(per_view) == {"PSNR", "SSIM", "MS-SSIM"}
    assert results["MS-SSIM"] is None and all(per_view["MS-SSIM"][n] is None for n in names)      # 24 pixels a side < 161
    assert all(sorted(per_view[k]) == names for k in per_view)
    assert results["PSNR"] == pytest.approx(np.mean([per_view["PSNR"][n] for n in names])) and 0 < results["PSNR"] < 60 and -1 <= results["SSIM"] <= 1
    assert res["results"]["PSNR"] == results["PSNR"] and math.isnan(res["results"]["MS-SSIM"])
    # the PNG of frame 1 is to_uint8 of the render of frame_1.ply from test camera 1
    test = load_dnerf(data, white_background=True)["test"]
    v, f, c = (torch.from_numpy(x) for x in read_mesh_ply(os.path.join(mesh_dir, "frame_1.ply")))
    want = render_mesh(test[1].camera, v, f, c)["render"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(model, "mesh_image", names[1]))), to_uint8(want))
    assert float(want.min()) < 0.9 and float(want[:, 0, 0].min()) == 1.0                          # the mesh is in view, on white
    # the shell form writes the same numbers
    other = str(tmp_path / "other")
    cli = main([mesh_dir, data, "--device", "cpu", "--out-dir", other])
    assert cli["results"]["PSNR"] == res["results"]["PSNR"] and cli["per_view"]["SSIM"] == res["per_view"]["SSIM"]
    assert json.load(open(os.path.join(other, "mesh_render_per_view.json"))) == per_view
    assert sorted(os.listdir(os.path.join(other, "mesh_shape"))) == names
    # --float scores the float renders, --black-background draws on black
    flt = main([mesh_dir, data, "--device", "cpu", "--out-dir", other, "--float", "--black-background", "--supersample", "2"])
    assert flt["results"]["PSNR"] != res["results"]["PSNR"]
    assert np.asarray(Image.open(os.path.join(other, "mesh_image", names[0])))[0, 0].tolist() == [0, 0, 0]
    # a directory that is not <model>/train/ours_<it> receives the files itself
    loose = str(tmp_path / "loose")
    _write_meshes(loose, 3)
    render_meshes(loose, data, device="cpu")
    assert os.path.exists(os.path.join(loose, "mesh_render_results.json")) and os.path.isdir(os.path.join(loose, "mesh_image"))
    # count mismatch
    os.remove(os.path.join(loose, "frame_2.ply"))
    with pytest.raises(ValueError, match="test cameras"):
        render_meshes(loose, data, device="cpu")


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_row_length_is_the_kernels():
    from dgs_amd import _mesh_ops
    from dgs_amd.mesh_render import ROW
    layout = _mesh_ops.raster_layout()
    assert layout[2] == ROW and ROW * 4 % 16 == 0 and layout[1] % 64 == 0 and layout[0] >= 1 and layout[3] >= 6
    assert _mesh_ops.load().dgs_mesh_raster_layout(None) < 0


def test_raster_arguments_are_validated_before_any_launch():
    """Every bad argument is refused by the host wrapper (status < 0 and its message), without touching a device."""
    from dgs_amd import _mesh_ops
    lib = _mesh_ops.load()
    err = lambda: lib.dgs_mesh_ops_last_error()
    raw = (ctypes.c_float * (2 * 24 + 8))()
    base = ctypes.addressof(raw)
    table = ctypes.c_void_p(base + (-base) % 16)                            # a 16-byte aligned table of two rows inside `raw`
    odd = ctypes.c_void_p(table.value + 4)
    lst, best = (ctypes.c_int * 2)(), (ctypes.c_ulonglong * 16)()
    fac, att, bg, img = (ctypes.c_int * 6)(), (ctypes.c_float * 9)(), (ctypes.c_float * 9)(), (ctypes.c_float * 16 * 9)()
    p = lambda x: ctypes.cast(x, ctypes.c_void_p)
    raster = lambda **k: lib.dgs_mesh_raster(*[k.get(n, d) for n, d in (("n_faces", 2), ("table", table), ("list", p(lst)), ("n_list", 2), ("path", 0),
                                                                       ("H", 4), ("W", 4), ("best", p(best)), ("clear", 1), ("stream", None))])
    for kw, msg in (({"H": 0}, b"H and W"), ({"W": -3}, b"H and W"), ({"H": 1 << 16, "W": 1 << 15}, b"too large"), ({"n_faces": 1 << 31}, b"2^31"),
                    ({"n_faces": -1}, b"negative n_faces"), ({"table": None}, b"null pointer"), ({"table": odd}, b"aligned"),
                    ({"list": None}, b"null pointer"), ({"best": None}, b"null pointer"), ({"n_list": -1}, b"negative n_list"),
                    ({"n_list": 1 << 31}, b"n_list"), ({"path": 2}, b"path")):
        assert raster(**kw) < 0 and msg in err(), (kw, err())
    resolve = lambda **k: lib.dgs_mesh_resolve(*[k.get(n, d) for n, d in (("H", 4), ("W", 4), ("best", p(best)), ("n_faces", 2), ("table", table),
                                                                         ("faces", p(fac)), ("n_vertices", 3), ("attr", p(att)), ("C", 3),
                                                                         ("background", p(bg)), ("face_id", None), ("depth", None), ("bary", None),
                                                                         ("image", p(img)), ("stream", None))])
    cmax = _mesh_ops.raster_layout()[3]
    for kw, msg in (({"H": 0}, b"H and W"), ({"W": 0}, b"H and W"), ({"n_faces": 1 << 31}, b"2^31"), ({"table": odd}, b"aligned"),
                    ({"table": None}, b"null pointer"), ({"C": cmax + 1}, b"C must be"), ({"C": -1}, b"C must be"), ({"best": None}, b"null pointer"),
                    ({"faces": None}, b"null pointer"), ({"attr": None}, b"null pointer"), ({"background": None}, b"null pointer"),
                    ({"image": None}, b"null pointer"), ({"n_vertices": 1 << 31}, b"n_vertices"), ({"n_vertices": -1}, b"n_vertices")):
        assert resolve(**kw) < 0 and msg in err(), (kw, err())
