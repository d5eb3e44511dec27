"""numpy statement of the SSIM that the reference's evaluation step computes (src/evaluation/metrics.py:38-54):
skimage.metrics.structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) per image.

skimage's algorithm, restated without skimage or scipy (the GPU tests import this module):
- the moments x, y, x*x, y*y, x*y are filtered with scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5, mode="reflect"):
  separable 11-tap passes, axis 0 then axis 1, each pass accumulated in float64 and stored in the image's type;
  scipy's "reflect" is numpy's "symmetric" padding;
- vx = cov_norm (uxx - ux^2), vy, vxy likewise, cov_norm = 121 / 120 (sample covariance);
- S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = 0.01^2, C2 = 0.03^2;
- per channel the float64 mean of S cropped by 5 pixels on every side, per image the mean over channels.

dtype=np.float32 is skimage's own arithmetic for float32 images; dtype=np.float64 is the yardstick the kernel is held to.
"""
from __future__ import annotations

import numpy as np

SIGMA, TRUNCATE, WIN = 1.5, 3.5, 11
RADIUS = int(TRUNCATE * SIGMA + 0.5)          # scipy.ndimage.gaussian_filter1d's radius: 5
PAD = (WIN - 1) // 2                          # skimage's crop: 5
K1, K2 = 0.01, 0.03


def gaussian_weights() -> np.ndarray:
    """The 11 float64 weights scipy.ndimage._gaussian_kernel1d builds for sigma 1.5, radius 5."""
    x = np.arange(-RADIUS, RADIUS + 1)
    phi = np.exp(-0.5 / (SIGMA * SIGMA) * x.astype(np.float64) ** 2)
    return phi / phi.sum()


def _filter(img: np.ndarray, dtype, pad_mode: str) -> np.ndarray:
    """Separable Gaussian over the last two axes; each pass accumulates in float64 and is stored as `dtype`."""
    w = gaussian_weights()
    r = RADIUS
    widths = [(0, 0)] * (img.ndim - 2) + [(r, r), (r, r)]
    p = np.pad(img, widths, mode=pad_mode)
    h, wd = img.shape[-2], img.shape[-1]
    acc = np.zeros(p.shape[:-2] + (h, p.shape[-1]), np.float64)
    for k in range(2 * r + 1):
        acc += w[k] * p[..., k:k + h, :]
    t = acc.astype(dtype)
    acc = np.zeros(img.shape, np.float64)
    for k in range(2 * r + 1):
        acc += w[k] * t[..., :, k:k + wd]
    return acc.astype(dtype)


def ssim_map(x: np.ndarray, y: np.ndarray, dtype=np.float64, pad_mode: str = "symmetric") -> np.ndarray:
    """S per pixel for images [..., H, W] (full size; the border depends on the padding, the interior does not)."""
    x = np.asarray(x).astype(dtype)
    y = np.asarray(y).astype(dtype)
    f = lambda a: _filter(a, dtype, pad_mode)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    cov_norm = dtype(WIN * WIN / (WIN * WIN - 1.0))
    c1, c2 = dtype(K1 * K1), dtype(K2 * K2)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    a1, a2 = dtype(2) * ux * uy + c1, dtype(2) * vxy + c2
    b1, b2 = ux * ux + uy * uy + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2)


def ssim(x: np.ndarray, y: np.ndarray, dtype=np.float64, pad_mode: str = "symmetric") -> np.ndarray:
    """Mean SSIM per image of [N, C, H, W] arrays -> float64 [N]."""
    if x.shape != y.shape or x.ndim != 4:
        raise ValueError(f"expected two [N,C,H,W] arrays of one shape, got {x.shape} and {y.shape}")
    if min(x.shape[-2:]) < WIN:
        raise ValueError("win_size exceeds image extent")
    s = ssim_map(x, y, dtype, pad_mode)[..., PAD:-PAD, PAD:-PAD]
    per_channel = s.reshape(s.shape[0], s.shape[1], -1).mean(axis=-1, dtype=np.float64)
    return per_channel.mean(axis=1)
