"""A numpy statement of the training step's context-depth loss (the reference's src/model/model_wrapper_erp.py:242-287 with
erode and compute_l1_sphere_loss of src/model/model_wrapper_helper.py), written for this project.

  erode(x, k)            1 - (max over the k x k window of 1 - x), the window padded by reflection ((k - 1) / 2 on each side,
                         index -1 -> 1, H -> H - 2), NaN wherever the window holds one
  row_weights(H)         sin((h + 0.5) pi / H) in float32
  l1_sphere(p, t, m)     float32 terms |t - p| * (w_h * m) and w_h * m, float64 sums, the sums rounded to float32, the
                         denominator clamped away from 0 by 1e-10, the quotient in float32; also the float64 quotient
  l1_sphere_grads        the autograd chain: grad_p = -(((g / den') * (w_h m)) * sign(t - p)), grad_t = -grad_p, sign(NaN) = 0
  closure                mask = depth > near; target = far where depth < fill_below; erode the mask when it has a hole;
                         weight * loss
"""
import numpy as np

F32 = np.float32


def _reflect(i: np.ndarray, n: int) -> np.ndarray:
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def _max_nan(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.maximum(a, b)).astype(a.dtype)


def erode(x: np.ndarray, ksize: int = 5) -> np.ndarray:
    """x[..., H, W] float32 -> the eroded planes (float32)."""
    x = np.asarray(x, F32)
    h, w = x.shape[-2:]
    pad = (ksize - 1) // 2
    assert ksize % 2 == 1 and pad < h and pad < w
    inv = (F32(1) - x).astype(F32)
    ry = _reflect(np.arange(-pad, h + pad), h)
    rx = _reflect(np.arange(-pad, w + pad), w)
    padded = inv[..., ry, :][..., rx]
    m = np.full(x.shape, -np.inf, F32)
    for dy in range(ksize):
        for dx in range(ksize):
            m = _max_nan(m, padded[..., dy:dy + h, dx:dx + w])
    return (F32(1) - m).astype(F32)


def row_weights(h: int) -> np.ndarray:
    r = (np.arange(h, dtype=F32) + F32(0.5)) * F32(np.pi)
    return np.sin((r / F32(h)).astype(F32)).astype(F32)


def clamp_away(den):
    den = np.asarray(den, F32)
    return np.where(den >= 0, np.maximum(den, F32(1e-10)), np.where(np.isnan(den), den, np.minimum(den, F32(-1e-10)))).astype(F32)


def l1_sphere(p, t, m, keep_batch=False, weights=None):
    """p, t, m [B,V,H,W] -> dict(loss32, den32 (clamped), loss64 (float64 quotient of the float64 sums, clamped den), num64, den64)."""
    p, t, m = (np.asarray(a, F32) for a in (p, t, m))
    h = p.shape[2]
    w = row_weights(h) if weights is None else np.asarray(weights, F32)
    wm = (w[None, None, :, None] * m).astype(F32)
    term = (np.abs(t - p).astype(F32) * wm).astype(F32)
    axes = (1, 2, 3) if keep_batch else (0, 1, 2, 3)
    num = term.astype(np.float64).sum(axis=axes)
    den = wm.astype(np.float64).sum(axis=axes)
    denc = clamp_away(den.astype(F32))
    with np.errstate(all="ignore"):
        loss32 = (num.astype(F32) / denc).astype(F32)
        d64 = np.where(den >= 0, np.maximum(den, 1e-10), np.where(np.isnan(den), den, np.minimum(den, -1e-10)))
        loss64 = num / d64
    return dict(loss32=loss32, den32=denc, loss64=loss64, num64=num, den64=den)


def l1_sphere_grads(p, t, m, g, den, weights=None):
    """The autograd chain of l1_sphere given the incoming gradient g (scalar or [B]) and the clamped denominator den
    (scalar or [B]) -> (grad_p, grad_t), float32."""
    p, t, m = (np.asarray(a, F32) for a in (p, t, m))
    h = p.shape[2]
    w = row_weights(h) if weights is None else np.asarray(weights, F32)
    wm = (w[None, None, :, None] * m).astype(F32)
    with np.errstate(all="ignore"):
        q = (np.asarray(g, F32) / np.asarray(den, F32)).astype(F32).reshape(-1, 1, 1, 1)
        d = (t - p).astype(F32)
        s = ((F32(0) < d).astype(F32) - (d < F32(0)).astype(F32)).astype(F32)
        x = ((q * wm).astype(F32) * s).astype(F32)
    return (-x).astype(F32), x


def closure(pred, depth, far, near=0.1, fill_below=1e-7, weight=0.1, ksize=5, conditional=True):
    """The reference's compute_context_depth_loss on [B,V,H,W] -> dict(loss (float32, weighted), mask, target, den32)."""
    depth = np.asarray(depth, F32)
    mask = (depth > F32(near)).astype(F32)
    target = np.where(depth < F32(fill_below), F32(far), depth).astype(F32)
    if not conditional or not mask.all():
        mask = erode(mask, ksize)
    r = l1_sphere(pred, target, mask)
    return dict(loss=(r["loss32"] * F32(weight)).astype(F32), mask=mask, target=target, den32=r["den32"])
