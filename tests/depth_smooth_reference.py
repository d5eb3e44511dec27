"""The statement of the depth-smoothness loss (the reference's LossDepth, src/loss/loss_depth.py:26-60), written for this project:
the kernels of csrc/s360_depth_smooth.hip and every test of them are held to `statement`.

    statement(depth, ln, lf, image, sigma, second, g)   numpy, float64 arithmetic on the float32 inputs -> loss, grad, A
    torch_statement(...)                                the reference's lines in plain torch (any dtype / device): the float32
                                                        chain the kernels replace, used as the on-device comparison and timing
    make_case(shape, vn, seed)                          inputs with the edge cases the tests need

ln = log(near), lf = log(far) are inputs (float32 [B,Vn], taken with torch's .log()); view v uses bound v // (V // Vn).
"""
import numpy as np


def _sgn(t):
    """torch's sign: sign(0) = 0, and sign(NaN) = 0 (numpy's would be NaN)."""
    return (t > 0).astype(np.float64) - (t < 0).astype(np.float64)


def _bounds(x, v):
    """[B,Vn] float32 -> [B,V,1,1] float64, view v using bound v // (V // Vn)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    assert x.ndim == 2 and v % x.shape[1] == 0
    return np.repeat(x, v // x.shape[1], axis=1)[:, :, None, None]


def _diff(a, axis):
    hi = [slice(None)] * a.ndim
    lo = [slice(None)] * a.ndim
    hi[axis], lo[axis] = slice(1, None), slice(None, -1)
    return a[tuple(hi)] - a[tuple(lo)], tuple(hi), tuple(lo)


def _axis_terms(n, image, sigma, second, axis):
    """Along one axis (-1: W, -2: H): the terms t, their weights e, and per term the stencil (offset, coefficient) pairs."""
    t, hi, lo = _diff(n, axis)                                   # n[x + 1] - n[x]
    if second:
        t = t[hi] - t[lo]                                         # (n[x + 2] - n[x + 1]) - (n[x + 1] - n[x])
    e = np.ones_like(t)
    if sigma is not None:
        c = _diff(image, axis)[0].max(axis=2)                     # signed difference, largest over the channels; NaN stays NaN
        if second:
            c = np.maximum(c[hi], c[lo])
        e = np.exp(-c * np.float64(np.float32(sigma)))
        t = t * e
    return t, e, (((0, 1.0), (1, -2.0), (2, 1.0)) if second else ((0, -1.0), (1, 1.0)))


def statement(depth, ln, lf, image=None, sigma=None, second=False, g=1.0):
    """-> dict(loss float32 0-d, grad float32 [B,V,H,W], A float64 [B,V,H,W], loss64, grad64, tx, ty).

    Everything is float64 arithmetic on the float32 inputs (sigma and g are rounded to float32 first: they cross the C ABI as
    floats), in the order written; the loss and each gradient are rounded to float32 once."""
    d = np.asarray(depth, np.float32).astype(np.float64)
    b, v, h, w = d.shape
    ln, lf = _bounds(ln, v), _bounds(lf, v)
    img = None if sigma is None else np.asarray(image, np.float32).astype(np.float64)
    g = np.float64(np.float32(g))
    with np.errstate(all="ignore"):
        m = np.minimum(d, lf)
        c = np.maximum(m, ln)
        span = lf - ln
        n = (c - ln) / span                                       # a division, not a reciprocal multiply
        grad_n, a_n, sums, terms = np.zeros_like(d), np.zeros_like(d), [], []
        for axis in (-1, -2):
            t, e, stencil = _axis_terms(n, img, sigma, second, axis)
            count = np.float64(t.size)
            sums.append(np.abs(t).sum(dtype=np.float64) / count)
            terms.append(t)
            s_acc, a_acc = np.zeros_like(d), np.zeros_like(d)
            length = t.shape[axis]
            for off, coef in stencil:                             # the term that starts at x touches pixel x + off
                sl = [slice(None)] * 4
                sl[axis] = slice(off, off + length)
                s_acc[tuple(sl)] += coef * _sgn(t) * e
                a_acc[tuple(sl)] += abs(coef) * np.abs(_sgn(t)) * e
            grad_n += s_acc / count
            a_n += a_acc / count
        loss64 = sums[0] + sums[1]
        gate = np.where(d > lf, 0.0, np.where(d == lf, 0.5, 1.0)) * np.where(m < ln, 0.0, np.where(m == ln, 0.5, 1.0))
        grad64 = g * grad_n * gate / span
        big_a = np.abs(g) * a_n * np.abs(gate / span)
    return {"loss": np.float32(loss64), "grad": grad64.astype(np.float32), "A": big_a, "loss64": loss64, "grad64": grad64,
            "tx": terms[0], "ty": terms[1]}


def torch_statement(depth, near, far, image=None, sigma=None, second=False, weight=1.0, return_terms=False):
    """The reference's lines (loss_depth.py:34-60) in plain torch, in depth's dtype on depth's device.  near, far [B,Vn] with
    Vn in {1, V} broadcast as the reference's do; any other divisor of V is repeated per view first."""
    import torch
    v = depth.shape[1]
    if near.shape[1] not in (1, v):
        near, far = (x.repeat_interleave(v // x.shape[1], dim=1) for x in (near, far))
    near = near[..., None, None].log()
    far = far[..., None, None].log()
    n = depth.minimum(far).maximum(near)
    n = (n - near) / (far - near)
    dx, dy = n.diff(dim=-1), n.diff(dim=-2)
    if second:
        dx, dy = dx.diff(dim=-1), dy.diff(dim=-2)
    if sigma is not None:
        cx, cy = image.diff(dim=-1).amax(dim=2), image.diff(dim=-2).amax(dim=2)
        if second:
            cx = cx[..., :, 1:].maximum(cx[..., :, :-1])
            cy = cy[..., 1:, :].maximum(cy[..., :-1, :])
        dx = dx * torch.exp(-cx * sigma)
        dy = dy * torch.exp(-cy * sigma)
    loss = weight * (dx.abs().mean() + dy.abs().mean())
    return (loss, dx, dy) if return_terms else loss


MODES = (("d1", False, None), ("d2", True, None), ("d1_bilateral", False, 2.0), ("d2_bilateral", True, 2.0))   # name, second, sigma


def torch_log(x, device="cpu"):
    """torch's float32 .log() of a numpy array on `device`: the bounds as the reference (and the Python layer) takes them there."""
    import torch
    return torch.from_numpy(np.asarray(x, np.float32)).to(device).log().cpu().numpy()


def make_case(shape, vn, seed, channels=3, device="cpu"):
    """depth [B,V,H,W], near, far [B,Vn], image [B,V,C,H,W] (float32 numpy).  The depth spreads over [log near - 0.8,
    log far + 0.8], so some pixels lie outside both bounds; where the planes are large enough it also holds a pixel exactly at
    log(far) and one exactly at log(near) (torch's float32 logs on `device`), two equal neighbours along each axis (all in plane [0, 0]), from two views on
    a constant plane (the last view of the last batch element) and from three views on a plane wholly beyond far (the view
    before it)."""
    rng = np.random.default_rng(seed)
    b, v, h, w = shape
    near = (0.3 + 0.4 * rng.random((b, vn))).astype(np.float32)
    far = (20.0 + 80.0 * rng.random((b, vn))).astype(np.float32)
    ln, lf = torch_log(near, device), torch_log(far, device)
    per = v // vn
    lo, hi = np.repeat(ln, per, axis=1)[:, :, None, None], np.repeat(lf, per, axis=1)[:, :, None, None]
    depth = (lo - 0.8 + (hi - lo + 1.6) * rng.random(shape)).astype(np.float32)
    image = rng.random((b, v, channels, h, w)).astype(np.float32)
    if h >= 3 and w >= 3:
        depth[0, 0, 1, 1] = hi[0, 0, 0, 0]                        # exactly log(far): the tie of minimum
        depth[0, 0, h - 1, 0] = lo[0, 0, 0, 0]                    # exactly log(near): the tie of maximum
        depth[0, 0, 0, w - 2] = depth[0, 0, 0, w - 1] = 0.5 * (lo[0, 0, 0, 0] + hi[0, 0, 0, 0])    # equal neighbours along W
        depth[0, 0, h - 2, w - 1] = depth[0, 0, h - 1, w - 1]     # equal neighbours along H
        depth[0, 0, 0, 0], depth[0, 0, 1, 0] = lo[0, 0, 0, 0] - 0.5, hi[0, 0, 0, 0] + 0.5           # outside both bounds
    if v >= 2:
        depth[b - 1, v - 1] = 0.5 * (lo[b - 1, v - 1] + hi[b - 1, v - 1])     # a constant plane
    if v >= 3:
        depth[b - 1, v - 2] = hi[b - 1, v - 2] + 1.0 + rng.random((h, w)).astype(np.float32)   # a plane wholly beyond far
    return {"depth": depth, "near": near, "far": far, "image": image}
