"""The PyTorch statement of the image metrics (dgs_amd/evaluate.py: the CPU path of image_metrics and, in float64, the reference of
the HIP kernel in tests/test_image_metrics_gpu.py) and the writer of evaluate(), without a GPU.
  reference pin   utils/loss_utils.py ssim and the psnr formula of utils/image_utils.py, recorded by
                  tests/golden/make_image_metrics_golden.py on make_loss_golden.images, as floats and after the 8-bit round trip
  MS-SSIM         no library to pin against (pytorch_msssim is not installed): closed forms instead
  pooled level    avg_pool2d(x, 2, padding=(H % 2, W % 2)) written out by hand
  writer          folders, file names, JSON layout; the numbers are those of the PNGs read back"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import image_metrics_ref as ir

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
F64 = torch.float64
W5 = 0.1333


def _ev():
    from dgs_amd import evaluate
    return evaluate


def test_reference_pin():
    from make_loss_golden import images
    ev = _ev()
    g = np.load(os.path.join(HERE, "golden", "image_metrics_golden.npz"))
    sizes = [tuple(int(v) for v in s) for s in g["sizes"]]
    assert (3, 40, 52) in sizes and any(min(h, w) < 11 for _, h, w in sizes)
    for i, (C, H, W) in enumerate(sizes):
        a, b = images(C, H, W)
        for tag, quantize in (("float", False), ("u8", True)):
            m = ev.image_metrics_torch(a.double(), b.double(), quantize=quantize)
            assert m["ssim"].dtype == F64 and m["ssim"].shape == ()
            assert float(m["ssim"]) == pytest.approx(float(g["ssim_%s_%d" % (tag, i)]), abs=1e-6), (C, H, W, tag)
            assert float(m["psnr"]) == pytest.approx(float(g["psnr_%s_%d" % (tag, i)]), abs=1e-6 * float(g["psnr_%s_%d" % (tag, i)])), (C, H, W, tag)
            assert float(m["mse"]) == pytest.approx(10 ** (-float(m["psnr"]) / 10), rel=1e-12)
            assert math.isnan(float(m["ms_ssim"]))                           # smaller than 161
            # the CPU path of image_metrics is this function; float32 agrees with float64 to float32 accuracy
            m32 = ev.image_metrics(a, b, quantize=quantize)
            assert float(m32["ssim"]) == pytest.approx(float(m["ssim"]), abs=2e-5) and float(m32["psnr"]) == pytest.approx(float(m["psnr"]), abs=1e-4)


def test_quantisation_is_the_png_round_trip():
    ev = _ev()
    x = torch.tensor([-0.3, 0.0, 0.5 / 255, 0.4999 / 255, 1.0 / 255, 0.5, 0.999, 1.0, 1.7, float("nan")])
    q = ev.quantize_torch(x)
    want = torch.tensor([0, 0, 1, 0, 1, 128, 255, 255, 255], dtype=torch.float32) / 255
    assert torch.equal(q[:-1], want) and math.isnan(float(q[-1]))
    u = ev.to_uint8(x[None, None, :-1])
    assert u.reshape(-1).tolist() == [0, 0, 1, 0, 1, 128, 255, 255, 255]


@pytest.mark.parametrize("size,chain", [(161, (161, 81, 41, 21, 11)), (176, (176, 88, 44, 22, 11))])
def test_ms_ssim_closed_forms(size, chain):
    ev = _ev()
    assert [h for h, _ in ev._levels(size, size + 15)] == list(chain)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, size, size, generator=gen, dtype=F64)
    m = ev.image_metrics_torch(x, x.clone())
    assert torch.equal(m["ms_ssim"], torch.ones(2, dtype=F64)) and torch.equal(m["ssim"], torch.ones(2, dtype=F64))
    assert bool(torch.isinf(m["psnr"]).all()) and bool((m["mse"] == 0).all())
    if size % 2 == 0:
        # constant images, even sizes (no zero padding enters the pyramid): every cs is C2 / C2, the last level's ssim is the
        # luminance term alone
        for a, b in ((0.3, 0.6), (0.75, 0.25), (0.0, 1.0)):
            m = ev.image_metrics_torch(torch.full((1, 3, size, size), a, dtype=F64), torch.full((1, 3, size, size), b, dtype=F64))
            want = ((2 * a * b + ir.C1) / (a * a + b * b + ir.C1)) ** W5
            assert float(m["ms_ssim"][0]) == pytest.approx(want, abs=1e-12), (a, b)
            assert float(m["mse"][0]) == pytest.approx((a - b) ** 2, rel=1e-12)


def test_ms_ssim_is_undefined_at_160():
    ev = _ev()
    gen = torch.Generator().manual_seed(6)
    x, y = torch.rand(1, 1, 160, 200, generator=gen, dtype=F64), torch.rand(1, 1, 160, 200, generator=gen, dtype=F64)
    m = ev.image_metrics_torch(x, y)
    assert math.isnan(float(m["ms_ssim"][0])) and math.isfinite(float(m["ssim"][0]))
    m = ev.image_metrics_torch(torch.rand(1, 1, 161, 161, generator=gen, dtype=F64), torch.rand(1, 1, 161, 161, generator=gen, dtype=F64))
    assert 0.0 <= float(m["ms_ssim"][0]) < 1.0
    assert math.isnan(float(ev.image_metrics_torch(x, y, ms_ssim=False)["ms_ssim"][0]))
    with pytest.raises(ValueError):
        ev.metric_sums_torch(x[..., :10, :], y[..., :10, :], "valid")


@pytest.mark.parametrize("H,W", [(7, 10), (10, 7), (7, 9), (1, 1), (8, 12)])
def test_pooled_level(H, W):
    ev = _ev()
    x = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(H * 100 + W), dtype=F64)
    got = ev.pool_torch(x)
    PH, PW = (H + 1) // 2, (W + 1) // 2
    assert got.shape == (2, 3, PH, PW)
    padded = torch.zeros(2, 3, 2 * PH, 2 * PW, dtype=F64)
    padded[..., H % 2:, W % 2:] = x
    want = (padded[..., 0::2, 0::2] + padded[..., 0::2, 1::2] + padded[..., 1::2, 0::2] + padded[..., 1::2, 1::2]) / 4
    assert torch.allclose(got, want, rtol=0, atol=1e-15)


def test_same_window_is_losses_ssim():
    from dgs_amd.losses import ssim_torch
    ev = _ev()
    a, b = ir.make_batch(2, 3, 23, 31)
    se, s, cs = ev.metric_sums_torch(a.double(), b.double(), "same")
    for i in range(2):
        assert float(s[i].sum()) / (3 * 23 * 31) == pytest.approx(float(ssim_torch(a[i].double(), b[i].double())), abs=1e-7)
    assert torch.allclose(se, ((a.double() - b.double()) ** 2).sum((-2, -1)))
    assert bool((cs > s).all())                                              # the luminance term is below 1 on distinct images


def test_writer(tmp_path):
    ev = _ev()
    H = W = 176
    gen = torch.Generator().manual_seed(11)
    items = []
    for i in range(3):
        gt = torch.rand(3, H, W, generator=gen, dtype=F64)
        rgb = (0.7 * gt + 0.3 * torch.rand(3, H, W, generator=gen, dtype=F64)) * 1.05 - 0.02          # leaves [0, 1]: the writer clamps
        items.append((torch.cat([rgb, torch.rand(1, H, W, generator=gen, dtype=F64)]), gt, torch.rand(1, H, W, generator=gen, dtype=F64)))
    model = str(tmp_path)
    mean, per_view = ev.write_split(model, "test", "ours_7", iter(items), batch=2)
    ev.write_results(model, {"ours_7": mean}, {"ours_7": per_view})
    base = os.path.join(model, "test", "ours_7")
    names = ["%05d.png" % i for i in range(3)]
    from PIL import Image
    for sub, mode in (("renders", "RGBA"), ("gt", "RGB"), ("depth", "RGB")):
        assert sorted(os.listdir(os.path.join(base, sub))) == names
        im = Image.open(os.path.join(base, sub, names[0]))
        assert im.mode == mode and im.size == (W, H)
    assert np.array_equal(np.asarray(Image.open(os.path.join(base, "gt", names[1]))), ev.to_uint8(items[1][1]))
    results, views = json.load(open(os.path.join(model, "results.json"))), json.load(open(os.path.join(model, "per_view.json")))
    assert list(results) == ["ours_7"] and sorted(results["ours_7"]) == ["MS-SSIM", "PSNR", "SSIM"]
    assert list(views) == ["ours_7"] and sorted(views["ours_7"]) == ["MS-SSIM", "PSNR", "SSIM"]
    back = ir.png_metrics(base)
    for key, k in (("PSNR", "psnr"), ("SSIM", "ssim"), ("MS-SSIM", "ms_ssim")):
        assert sorted(views["ours_7"][key]) == names
        for n in names:
            assert views["ours_7"][key][n] == pytest.approx(back[n][k], rel=1e-12), (key, n)      # float64 items: the same statement on the same pixels
        assert results["ours_7"][key] == pytest.approx(np.mean([views["ours_7"][key][n] for n in names]), rel=1e-12)
    assert 0.3 < results["ours_7"]["MS-SSIM"] < 1.0
    # quantize=False scores the float tensors: close to, and different from, the files' numbers
    mean_f, _ = ev.write_split(model, "test", "ours_7", iter(items), save_images=False, quantize=False)
    assert mean_f["PSNR"] != mean["PSNR"] and mean_f["PSNR"] == pytest.approx(mean["PSNR"], abs=0.05)
    # below 161 pixels MS-SSIM is null in the files
    small = [(r[:, :40, :40], g[:, :40, :40], d[:, :40, :40]) for r, g, d in items[:1]]
    mean_s, per_s = ev.write_split(model, "train", "ours_7", iter(small))
    ev.write_results(model, {"train/ours_7": mean_s}, {"train/ours_7": per_s})
    assert json.load(open(os.path.join(model, "results.json")))["train/ours_7"]["MS-SSIM"] is None
    assert os.path.exists(os.path.join(model, "train", "ours_7", "depth", "00000.png"))
