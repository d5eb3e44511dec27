"""Time of the SSIM kernel (metrics.ssim: s360_ssim, two launches) at the evaluation shapes, beside the CPU computation it replaces.

  [18,3,256,256]  the six cube faces of the three target panoramas of one evaluation step
  [6,3,512,512]   one panorama's faces at configs[4]'s face size

GPU: HIP events around `--iters` back-to-back calls on one stream after `--warmup` calls, repeated `--reps` times (median and range
of the per-call time).  CPU: the reference's compute_ssim loops over images and channels through skimage, i.e.
scipy.ndimage.gaussian_filter on float32 images, single thread; restated here with scipy when it is installed (skimage is
not needed), else the numpy statement of tests/ssim_reference.py (all images at once).  Also prints the kernel's largest
deviation from the float64 statement on the timed inputs.  One JSON line per shape on stdout.
usage: ssim_timing.py [--iters 200] [--warmup 20] [--reps 5] [--cpu-reps 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ssim_reference as R  # noqa: E402
from splatter360_amd import metrics  # noqa: E402

SHAPES = ((18, 3, 256, 256), (6, 3, 512, 512))


def scipy_ssim(x: np.ndarray, y: np.ndarray):
    """skimage.metrics.structural_similarity(x, y, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) for one
    [C,H,W] float32 image, restated on scipy.ndimage (what skimage.filters.gaussian calls); None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    f = lambda a: ndimage.gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
    cn, c1, c2 = 121.0 / 120.0, 0.01 ** 2, 0.03 ** 2
    out = []
    for a, b in zip(x, y):
        ux, uy, uxx, uyy, uxy = f(a), f(b), f(a * a), f(b * b), f(a * b)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        out.append(s[5:-5, 5:-5].mean(dtype=np.float64))
    return float(np.mean(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_timing.py needs a GPU (no CPU fallback)")
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    for shape in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(0)
        x = torch.rand(shape, generator=g)
        y = (x + 0.05 * torch.randn(shape, generator=g)).clamp(-0.1, 1.1)
        xd, yd = x.to(dev), y.to(dev)
        for _ in range(a.warmup):
            metrics.ssim(xd, yd)
        torch.cuda.synchronize()
        per_call = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                metrics.ssim(xd, yd)
            e1.record()
            e1.synchronize()
            per_call.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        got = metrics.ssim(xd, yd).cpu().numpy().astype(np.float64)
        xn, yn = x.numpy(), y.numpy()
        dev64 = float(np.abs(got - R.ssim(xn, yn)).max())
        have_scipy = scipy_ssim(xn[0], yn[0]) is not None
        how = "scipy.ndimage per image" if have_scipy else "numpy statement (tests/ssim_reference.py), batched"
        cpu_s = []
        for _ in range(a.cpu_reps):
            t = time.perf_counter()
            if have_scipy:
                for i in range(shape[0]):
                    scipy_ssim(xn[i], yn[i])
            else:
                R.ssim(xn, yn, np.float32)
            cpu_s.append(time.perf_counter() - t)
        rec = dict(shape=list(shape), what="metrics.ssim per call, host overhead included", gpu_us_per_call_median=round(float(np.median(per_call)), 2),
                   gpu_us_per_call_range=[round(min(per_call), 2), round(max(per_call), 2)], iters=a.iters, reps=a.reps,
                   cpu_s_median=round(float(np.median(cpu_s)), 4), cpu_method=how + ", 1 thread",
                   max_abs_dev_from_float64=dev64, device=torch.cuda.get_device_name(dev))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
