"""How good does a fitted scene look on the views it was not trained on?  What the reference answers with render.py (render the
test split, write renders/ gt/ depth/ PNGs, print PSNR, SSIM, MS-SSIM, LPIPS) and metrics.py (read the PNGs back, write
results.json and per_view.json), as one call: evaluate().

  image_metrics        <- utils/image_utils.py psnr, utils/loss_utils.py ssim (what metrics.py reports) and the published multi-scale
                          SSIM as render.py:69 calls it (pytorch_msssim.ms_ssim, data_range 1, default weights)
  render_split         <- render.py:48-79 render_set
  evaluate             <- render.py render_sets + metrics.py evaluate

On a HIP device the sums behind the three numbers come from libdgs_train_ops.so (dgs_image_metrics, csrc/metric_kernels.h): one
launch for the whole batch per window / pyramid level, per-plane sums in float64, bit-identical from run to run.  On CPU tensors
image_metrics_torch states the same formulas in PyTorch at any precision; in float64 it is the reference of the kernel's tests.

Per plane (one channel of one image), with g the 11-tap sigma = 1.5 window (the fp32 values of losses._window_1d; a float64
evaluation renormalises them to sum to 1 in float64, which moves each by less than 2^-24 of itself: with the fp32 values taken as
they are, s11 - mu1^2 of a CONSTANT image is 6e-8 a^2 instead of 0), C1 = 0.01^2, C2 = 0.03^2:
  mu1 = g*a, mu2 = g*b, s11 = g*(a a) - mu1^2, s22 = g*(b b) - mu2^2, s12 = g*(a b) - mu1 mu2
  cs = (2 s12 + C2) / (s11 + s22 + C2),  ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs
  psnr    = 20 log10(1 / sqrt(mean over C,H,W of (a - b)^2))
  ssim    = mean over C,H,W of the ssim map on the zero-padded H x W domain ("same")
  ms_ssim = mean over C of  prod_{l=1..4} relu(mean cs_l)^{w_l} * relu(mean ssim_5)^{w_5},  level l on the (H_l - 10) x (W_l - 10)
            domain without padding ("valid"), level l + 1 = avg_pool2d(level l, 2, padding=(H_l % 2, W_l % 2)); defined for
            min(H, W) > 160, NaN otherwise (null in the JSON files)
pytorch_msssim and piq are not installed where this package is built and tested, so the lines above -- not a run of those libraries --
are the contract.  Not built: piq.ssim with its automatic down-sampling (render.py:67) and both LPIPS variants (their networks'
weights are not available); the JSON files have no LPIPS key.

Shell form:  python -m dgs_amd.evaluate MODEL DATA [--splits test ...] [--iteration N] [--no-images] [--float]
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from .losses import _window_1d

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MS_SSIM_MIN_SIDE = 161        # (side - 1) / 2^4 >= 10: the fifth level still holds an 11 x 11 window
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- the PyTorch statement ------------------------------------------------------------------------------------------------------
def quantize_torch(x):
    """The 8-bit round trip of torchvision.utils.save_image and a PNG reader: floor(clamp(x, 0, 1) * 255 + 0.5) / 255, evaluated in
    float32 whatever the dtype of x (which level a pixel lands on is decided there: in the writer and in the kernel), returned in
    the dtype of x."""
    y = x.to(torch.float32)
    return (torch.floor(y.clamp(0, 1) * 255 + 0.5) / torch.tensor(255.0, dtype=torch.float32, device=x.device)).to(x.dtype)


def pool_torch(x):
    """The next level of the MS-SSIM pyramid: 2 x 2 means at stride 2 behind one row / column of zeros on an odd axis."""
    return F.avg_pool2d(x, 2, padding=(x.shape[-2] % 2, x.shape[-1] % 2))


def _window(device, dtype):
    w = _window_1d(11, 1.5, device, torch.float32).to(dtype)
    return w / w.sum() if dtype == torch.float64 else w


def _band(n, w, pad):
    """[n + 2 pad - 10, n]: row i holds the window over columns i - pad .. i - pad + 10 (a banded matrix product instead of a
    convolution: any dtype on any device)."""
    rows = n + 2 * pad - 10
    i, j = torch.arange(rows, device=w.device)[:, None], torch.arange(n, device=w.device)[None, :]
    d = j - i + pad
    ok = (d >= 0) & (d <= 10)
    return torch.where(ok, w[d.clamp(0, 10)], torch.zeros((), dtype=w.dtype, device=w.device))


def metric_sums_torch(a, b, window="same"):
    """(SE, S, CS), each [B,C] in the dtype of a: the three sums of dgs_image_metrics for a, b [B,C,H,W]."""
    pad = {"same": 5, "valid": 0}[window]
    H, W = a.shape[-2:]
    if H + 2 * pad < 11 or W + 2 * pad < 11:
        raise ValueError("the valid window needs H >= 11 and W >= 11")
    w = _window(a.device, a.dtype)
    tv, th = _band(H, w, pad), _band(W, w, pad).T
    blur = lambda x: tv @ x @ th
    mu1, mu2, s11, s22, s12 = blur(a), blur(b), blur(a * a), blur(b * b), blur(a * b)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    sg1, sg2, sg12 = s11 - mu1_sq, s22 - mu2_sq, s12 - mu12
    cs = (2 * sg12 + C2) / (sg1 + sg2 + C2)
    ssim = (2 * mu12 + C1) / (mu1_sq + mu2_sq + C1) * cs
    return ((a - b) ** 2).sum((-2, -1)), ssim.sum((-2, -1)), cs.sum((-2, -1))


def _levels(H, W):
    """[(H_l, W_l)] of the five MS-SSIM levels."""
    out = [(H, W)]
    for _ in range(4):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _finish(shape, se, s_same, level_sums):
    """Sums -> the result dict.  se, s_same: [B,C] float64; level_sums: None or five (S, CS) [B,C] float64, one per level."""
    B, C, H, W = shape
    mse = se.sum(1) / float(C * H * W)
    out = {"mse": mse, "psnr": 20.0 * torch.log10(1.0 / torch.sqrt(mse)), "ssim": s_same.sum(1) / float(C * H * W)}
    if level_sums is None:
        out["ms_ssim"] = torch.full_like(mse, float("nan"))
    else:
        prod = torch.ones_like(se)
        for l, ((h, w), (s, cs)) in enumerate(zip(_levels(H, W), level_sums)):
            mean = (s if l == 4 else cs) / float((h - 10) * (w - 10))
            prod = prod * torch.relu(mean) ** MS_SSIM_WEIGHTS[l]
        out["ms_ssim"] = prod.mean(1)
    return out


def _batched(pred, gt):
    if pred.shape != gt.shape or pred.dim() not in (3, 4):
        raise ValueError("image_metrics expects two [C,H,W] or [B,C,H,W] tensors of equal shape")
    return (pred[None], gt[None], True) if pred.dim() == 3 else (pred, gt, False)


def image_metrics_torch(pred, gt, quantize=False, ms_ssim=True):
    """image_metrics in PyTorch, evaluated in the dtype of pred; the results are float64."""
    a, b, single = _batched(pred, gt.to(pred.dtype))
    if quantize:
        a, b = quantize_torch(a), quantize_torch(b)
    B, C, H, W = a.shape
    se, s_same, _ = metric_sums_torch(a, b, "same")
    levels = None
    if ms_ssim and min(H, W) >= MS_SSIM_MIN_SIDE:
        levels = []
        for l in range(5):
            _, s, cs = metric_sums_torch(a, b, "valid")
            levels.append((s.double(), cs.double()))
            if l < 4:
                a, b = pool_torch(a), pool_torch(b)
    out = _finish((B, C, H, W), se.double(), s_same.double(), levels)
    return {k: v[0] for k, v in out.items()} if single else out


def image_metrics(pred, gt, quantize=False, ms_ssim=True):
    """Per image: {"psnr", "ssim", "ms_ssim", "mse"} as float64 tensors [B] (0-dim for [C,H,W] inputs) on the inputs' device.
    quantize: both images go through the 8-bit round trip first (the numbers metrics.py computes from the written PNGs).
    HIP tensors: dgs_image_metrics, one launch for the same-window sums and five for the MS-SSIM chain, each level's launch writing
    the next level's images.  CPU tensors: image_metrics_torch."""
    if not pred.is_cuda:
        return image_metrics_torch(pred, gt, quantize, ms_ssim)
    from . import _ops
    a, b, single = _batched(pred.float(), gt.float())
    B, C, H, W = a.shape
    same, _, _ = _ops.image_metric_sums(a, b, "same", quantize)
    levels = None
    if ms_ssim and min(H, W) >= MS_SSIM_MIN_SIDE:
        levels = []
        for l in range(5):
            sums, pa, pb = _ops.image_metric_sums(a, b, "valid", quantize and l == 0, pooled=l < 4)
            levels.append((sums[..., 1], sums[..., 2]))
            a, b = pa, pb
    out = _finish((B, C, H, W), same[..., 0], same[..., 1], levels)
    return {k: v[0] for k, v in out.items()} if single else out


# ---- renders --------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def render_split(surfels, deform, frames, bg, rasterizer_cls=None):
    """render.py:48-79 for the frames (dgs_amd.io.Frame) of one split, each at its own time: yields per frame
    (render [4,H,W] = colour and alpha clamped to [0, 1], ground truth [3,H,W], depth / (depth.max() + 1e-5) [1,H,W]) on the model's
    device.  deform=None renders the surfels as they are."""
    from .render import render
    dev = surfels.get_xyz.device
    for fr in frames:
        cam = fr.camera.to(dev)
        d = {}
        if deform is not None:
            dv = deform(surfels.get_xyz.detach(), deform.expand_time(cam.fid), surfels.feature, surfels.motion_mask)
            d = {"d_xyz": dv["d_xyz"], "d_rotation": dv["d_rotation"], "d_scaling": dv["d_scaling"]}
        out = render(cam, surfels, bg, rasterizer_cls=rasterizer_cls, **d)
        rendering = torch.clamp(torch.cat([out["render"], out["alpha"]]), 0.0, 1.0)
        depth = out["depth"]
        yield rendering, fr.image.to(dev), depth / (depth.max() + 1e-5)


def to_uint8(x):
    """[C,H,W] in [0, 1] -> [H,W,C] uint8, rounded as torchvision.utils.save_image rounds."""
    return torch.floor(x.detach().float().clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()


def save_png(x, path):
    """8-bit PNG of a [C,H,W] tensor; one channel is written as three equal ones (save_image's make_grid does that)."""
    from PIL import Image
    u = to_uint8(x)
    if u.shape[2] == 1:
        u = np.repeat(u, 3, axis=2)
    Image.fromarray(u, {3: "RGB", 4: "RGBA"}[u.shape[2]]).save(path)


def _json_number(v):
    v = float(v)
    return v if math.isfinite(v) else None


def write_split(model_path, split, method, items, save_images=True, quantize=True, batch=8, log=None):
    """items: iterable of (render [>=3,H,W], gt [3,H,W], depth [1,H,W]).  Writes <model>/<split>/<method>/{renders,gt,depth}/%05d.png
    (save_images) and returns ({"PSNR", "SSIM", "MS-SSIM"} means, the same keys -> {file name: value}) over the items, metrics in
    batches of `batch` images of one size."""
    base = os.path.join(model_path, split, method)
    dirs = {k: os.path.join(base, k) for k in ("renders", "gt", "depth")}
    if save_images:
        for p in dirs.values():
            os.makedirs(p, exist_ok=True)
    per_view = {"SSIM": {}, "PSNR": {}, "MS-SSIM": {}}
    pending = []

    def flush():
        if not pending:
            return
        m = image_metrics(torch.stack([p[1] for p in pending]), torch.stack([p[2] for p in pending]), quantize=quantize)
        m = {k: v.cpu().tolist() for k, v in m.items()}
        for i, (name, _, _) in enumerate(pending):
            per_view["PSNR"][name], per_view["SSIM"][name], per_view["MS-SSIM"][name] = m["psnr"][i], m["ssim"][i], m["ms_ssim"][i]
            if log is not None:
                log("%s/%s %s: PSNR %.4f SSIM %.6f MS-SSIM %.6f" % (split, method, name, m["psnr"][i], m["ssim"][i], m["ms_ssim"][i]))
        del pending[:]

    for idx, (rendering, gt, depth) in enumerate(items):
        name = "%05d.png" % idx
        if save_images:
            save_png(rendering, os.path.join(dirs["renders"], name))
            save_png(gt, os.path.join(dirs["gt"], name))
            save_png(depth, os.path.join(dirs["depth"], name))
        image, target = rendering[:3].clamp(0, 1), gt[:3].to(rendering.dtype).clamp(0, 1)
        if pending and (pending[0][1].shape != image.shape or len(pending) >= batch):
            flush()
        pending.append((name, image, target))
    flush()
    if not per_view["PSNR"]:
        raise ValueError("write_split: no frames in split %r" % split)
    mean = {k: float(np.mean(list(v.values()))) for k, v in per_view.items()}
    return mean, per_view


def write_results(model_path, results, per_view):
    """<model>/results.json and <model>/per_view.json in the layout of metrics.py:84-95; NaN is written as null."""
    clean = lambda d: {k: (clean(v) if isinstance(v, dict) else _json_number(v)) for k, v in d.items()}
    for name, d in (("results.json", results), ("per_view.json", per_view)):
        with open(os.path.join(model_path, name), "w") as fp:
            json.dump(clean(d), fp, indent=True)


def evaluate(model_path, data_path, splits=("test",), iteration=-1, device="cuda:0", white_background=False, save_images=True, quantize=True,
             batch=8, log=None):
    """restore() the checkpoint, render every frame of the given splits of the dataset at its own time, write the PNGs and score them.
    Files: <model>/<split>/ours_<it>/{renders,gt,depth}/00000.png ... (save_images), <model>/results.json = {method: {"SSIM", "PSNR",
    "MS-SSIM"}} and <model>/per_view.json = {method: {metric: {file name: value}}}; the method key is ours_<it> for the test split
    (what metrics.py scans) and <split>/ours_<it> for any other.  quantize=True scores the images as the 8-bit files hold them,
    False the float renders.  Returns {"results": ..., "per_view": ...} as written."""
    from . import io as dio
    from .fit import restore
    device = torch.device(device)
    it = dio.search_for_max_iteration(os.path.join(model_path, "point_cloud")) if iteration == -1 else iteration
    surfels, deform = restore(model_path, iteration=it, device=device)
    data = dio.load_dnerf(data_path, white_background=white_background)
    bg = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], device=device)
    results, per_view = {}, {}
    for split in splits:
        frames = data.get(split)
        if not frames:
            raise ValueError("evaluate: the dataset at %s has no %r split" % (data_path, split))
        method = "ours_{}".format(it)
        key = method if split == "test" else split + "/" + method
        results[key], per_view[key] = write_split(model_path, split, method, render_split(surfels, deform, frames, bg), save_images=save_images,
                                                  quantize=quantize, batch=batch, log=log)
        if log is not None:
            log("[ITER %s] %s: PSNR %.4f SSIM %.6f MS-SSIM %.6f" % (it, split, results[key]["PSNR"], results[key]["SSIM"], results[key]["MS-SSIM"]))
    write_results(model_path, results, per_view)
    return {"results": results, "per_view": per_view}


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m dgs_amd.evaluate", description="Render the held-out views of a fitted scene and score them: "
                                 "PSNR, SSIM, MS-SSIM into results.json and per_view.json.")
    ap.add_argument("model_path")
    ap.add_argument("data_path")
    ap.add_argument("--splits", nargs="+", default=["test"])
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--white-background", action="store_true")
    ap.add_argument("--no-images", action="store_true", help="do not write the PNGs")
    ap.add_argument("--float", action="store_true", help="score the float renders instead of their 8-bit files")
    a = ap.parse_args(argv)
    return evaluate(a.model_path, a.data_path, splits=tuple(a.splits), iteration=a.iteration, device=a.device, white_background=a.white_background,
                    save_images=not a.no_images, quantize=not a.float, batch=8, log=print)


if __name__ == "__main__":
    main()
