"""Generates tests/golden/image_metrics_golden.npz by IMPORTING the reference's utils/loss_utils.py: ssim (the way
make_loss_golden.py does) and evaluating the psnr formula of utils/image_utils.py:32-34 (that module itself imports lpips and piq,
which are not installed) on the deterministic images of make_loss_golden.images, as floats and after the 8-bit round trip of
torchvision.utils.save_image + a PNG reader.  Only the images' parameters and the outputs are stored.
Run from the repo root:  python tests/golden/make_image_metrics_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_loss_golden import images, import_reference  # noqa: E402

SIZES = ((3, 40, 52), (3, 7, 9), (1, 61, 117))       # (C, H, W); the second is smaller than the 11 x 11 window


def round_trip(x):
    """save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8), read back as to_tensor reads it (/ 255)."""
    return x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).to(torch.float32) / 255


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def main():
    lu, _ = import_reference()
    out = {"sizes": np.asarray(SIZES, dtype=np.int64)}
    for i, (C, H, W) in enumerate(SIZES):
        a, b = images(C, H, W)
        for tag, (x, y) in (("float", (a, b)), ("u8", (round_trip(a), round_trip(b)))):
            # the float32 pixels, evaluated by the reference's code in float64 (its window keeps its float32 values): in float32 its
            # own rounding is 2e-6 of the SSIM of these smooth images, more than the 1e-6 the test pins
            x, y = x.double(), y.double()
            out["ssim_%s_%d" % (tag, i)] = np.float64(lu.ssim(x[None], y[None]).item())
            out["psnr_%s_%d" % (tag, i)] = np.float64(psnr(x[None], y[None]).item())
    np.savez_compressed(os.path.join(HERE, "image_metrics_golden.npz"), **out)
    print({k: (v.tolist() if v.shape else float(v)) for k, v in out.items()})


if __name__ == "__main__":
    main()
