"""-m gpu: evaluate() end to end.  A small synthetic D-NeRF dataset (8 train and 3 test views at 176 x 176, so that MS-SSIM is
defined), a fit of a few hundred iterations, evaluate(): the files exist under the reference's names, per_view.json has one entry per
test frame, every number equals the float64 statement applied to the PNGs read back (tolerance and R of
tests/test_image_metrics_gpu.py; yardstick: the statement in float32 on the device, on the same pixels), results.json holds the means
of the per-view values, and the held-out PSNR is finite and above that of the untrained model on the same frames."""
import gc
import json
import math
import os

import numpy as np
import pytest
import torch

import image_metrics_ref as ir
from test_image_metrics_gpu import EPS32, R_METRIC

pytestmark = pytest.mark.gpu


def test_evaluate_a_short_fit(tmp_path):
    from diff_surfel_rasterization import _C
    try:
        _evaluate_a_short_fit(tmp_path)
    finally:
        _C.set_capacity(0)          # fit() leaves the rasterizer in capacity mode (the captured step's list size)
        gc.collect()                # the trainer, its captured graph and the restored models go before the next test starts
        torch.cuda.empty_cache()


def _evaluate_a_short_fit(tmp_path):
    from dgs_amd import evaluate as ev
    from dgs_amd import io as dio
    from dgs_amd.fit import fit
    from dgs_amd.model import SurfelModel
    from dgs_amd.synthetic import write_dynamic_dnerf
    dev = torch.device("cuda:0")
    data, model = str(tmp_path / "scene"), str(tmp_path / "model")
    write_dynamic_dnerf(data, n_train=8, n_test=3, H=176, W=176, device=dev)
    fit(data, model, iterations=300, device=dev, num_pts=5000, node_num=128, seed=0, warm_up=100, regularize_from=180, densify_from=100,
        densify_interval=50, opacity_reset_interval=10_000)
    logs = []
    out = ev.evaluate(model, data, device=dev, log=logs.append)
    base = os.path.join(model, "test", "ours_300")
    names = ["%05d.png" % i for i in range(3)]
    for sub in ("renders", "gt", "depth"):
        assert sorted(os.listdir(os.path.join(base, sub))) == names, sub
    results, views = json.load(open(os.path.join(model, "results.json"))), json.load(open(os.path.join(model, "per_view.json")))
    assert results == out["results"] and views == out["per_view"]
    assert list(results) == ["ours_300"] and sorted(results["ours_300"]) == ["MS-SSIM", "PSNR", "SSIM"]
    assert len(logs) == 3 + 1
    # every number against the float64 statement on the files
    r64 = ir.png_metrics(base)
    fails = []
    for n in names:
        a, b = ir.read_png(os.path.join(base, "renders", n))[:3].float().to(dev), ir.read_png(os.path.join(base, "gt", n))[:3].float().to(dev)
        r32 = {k: float(v) for k, v in ev.image_metrics_torch(a, b).items()}
        for key, k in (("PSNR", "psnr"), ("SSIM", "ssim"), ("MS-SSIM", "ms_ssim")):
            assert sorted(views["ours_300"][key]) == names
            got, want = views["ours_300"][key][n], r64[n][k]
            e_k, e_t, floor = abs(got - want), abs(r32[k] - want), 4 * EPS32 * abs(want)
            print("EVAL %s %-8s got %.9f ref64 %.9f e_k %.3e e_t %.3e floor %.3e" % (n, key, got, want, e_k, e_t, floor))
            if not e_k <= R_METRIC * e_t + floor:
                fails.append("%s %s: e_k %.3e > %g * e_t %.3e + %.3e" % (n, key, e_k, R_METRIC, e_t, floor))
    assert not fails, "\n".join(fails)
    for key in ("PSNR", "SSIM", "MS-SSIM"):
        assert results["ours_300"][key] == pytest.approx(np.mean([views["ours_300"][key][n] for n in names]), rel=1e-12)
        assert math.isfinite(results["ours_300"][key])
    assert 0.0 < results["ours_300"]["SSIM"] < 1.0 and 0.0 < results["ours_300"]["MS-SSIM"] < 1.0
    # ... and the fit has learnt something: the untrained model (the random initial point cloud fit() starts from) on the same frames
    loaded = dio.load_dnerf(data)
    pc = loaded["point_cloud"]
    untrained = SurfelModel(dio.scene_from_point_cloud(pc.points, pc.colors, device=dev), active_sh_degree=0).to(dev)
    bg = torch.zeros(3, device=dev)
    before = [float(ev.image_metrics(r[:3], g, quantize=True, ms_ssim=False)["psnr"]) for r, g, _ in ev.render_split(untrained, None, loaded["test"], bg)]
    print("EVAL held-out PSNR untrained %.3f -> after 300 iterations %.3f" % (np.mean(before), results["ours_300"]["PSNR"]))
    assert len(before) == 3 and results["ours_300"]["PSNR"] > np.mean(before)
    # the float scores (no round trip) are close to the files' and not equal to them; no images are written again
    os.remove(os.path.join(base, "renders", names[0]))
    flt = ev.evaluate(model, data, device=dev, save_images=False, quantize=False)
    assert not os.path.exists(os.path.join(base, "renders", names[0]))
    assert flt["results"]["ours_300"]["PSNR"] == pytest.approx(results["ours_300"]["PSNR"], abs=0.05)
    assert flt["results"]["ours_300"]["PSNR"] != results["ours_300"]["PSNR"]
