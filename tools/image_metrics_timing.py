"""Times of the image metrics of an evaluation run -> profiles/image_metrics_timing.json.

    python tools/image_metrics_timing.py [--size 800] [--batch 20] [--reps 10] [--out profiles/image_metrics_timing.json]

dgs_amd.evaluate.image_metrics (dgs_image_metrics: one launch for the same-window sums, five for the MS-SSIM chain) against the PyTorch
statement of the same formulas in float32 on the same device (image_metrics_torch), for a batch of B RGB images of size x size from
a seeded generator, with and without the MS-SSIM chain.  Both run in one process, ALTERNATING, timed with device events after one
warm-up call of each; reported: the median, minimum and maximum of --reps calls, the ratio of the medians, the largest difference of
the four numbers between the two, and the bytes the algorithm has to move (every launch reads its two inputs once and writes its
pooled outputs once; the per-workgroup slots are left out) against the time."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dynamic-2dgs_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def algorithmic_bytes(B, C, H, W, chain):
    """fp32 bytes: the same-window launch reads both images; each chain level reads both of its images and writes both pooled ones."""
    from dgs_amd.evaluate import _levels
    total = 2 * B * C * H * W * 4
    if chain:
        lv = _levels(H, W)
        for l, (h, w) in enumerate(lv):
            total += 2 * B * C * h * w * 4
            if l < 4:
                total += 2 * B * C * lv[l + 1][0] * lv[l + 1][1] * 4
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_timing.json"))
    a = ap.parse_args()
    from dgs_amd import _ops
    from dgs_amd.evaluate import image_metrics, image_metrics_torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    B, C, H, W = a.batch, 3, a.size, a.size
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(B, C, H, W, generator=g)
    pred = (0.8 * gt + 0.2 * torch.rand(B, C, H, W, generator=g)).to(dev)
    gt = gt.to(dev)
    result = {"device": torch.cuda.get_device_name(0), "shape": [B, C, H, W], "layout": list(_ops.image_metrics_layout()), "method":
              "device events, one warm-up call of each, then %d calls of each, alternating, in one process" % a.reps, "cases": {}}
    for chain in (False, True):
        run_hip = lambda: image_metrics(pred, gt, quantize=True, ms_ssim=chain)
        run_torch = lambda: image_metrics_torch(pred, gt, quantize=True, ms_ssim=chain)
        timed(run_hip)
        timed(run_torch)
        hip_ms, torch_ms = [], []
        for _ in range(a.reps):
            ms, out_h = timed(run_hip)
            hip_ms.append(ms)
            ms, out_t = timed(run_torch)
            torch_ms.append(ms)
        keys = ["psnr", "ssim"] + (["ms_ssim"] if chain else [])
        h, t = stats(hip_ms), stats(torch_ms)
        nbytes = algorithmic_bytes(B, C, H, W, chain)
        case = {"hip": h, "torch_float32": t, "ratio_of_medians": t["median_ms"] / h["median_ms"], "launches": 2 * (6 if chain else 1),
                "algorithmic_bytes": nbytes, "hip_bytes_per_s": nbytes / (h["median_ms"] * 1e-3),
                "max_abs_difference": {k: float((out_h[k] - out_t[k]).abs().max()) for k in keys}}
        result["cases"]["ms_ssim" if chain else "psnr_ssim"] = case
        print(json.dumps({("ms_ssim" if chain else "psnr_ssim"): case}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
