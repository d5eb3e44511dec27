"""The training step's context-depth loss on the GPU: erode, compute_l1_sphere_loss and their closure (csrc/s360_depth_loss.hip).

The reference supervises the context views' predicted depth on every default training step (src/model/model_wrapper_erp.py:242-287,
`wo_depth_supervise: false`): the mask `depth > 0.1`, the far fill of `depth < 1e-7`, an erosion of the mask (only when it has
holes, which needs `mask.all()` on the host) and 0.1 x compute_l1_sphere_loss (src/model/model_wrapper_helper.py:4-24, :63-90).
Here `erode` and `compute_l1_sphere_loss` keep the reference's contracts, and `context_depth_loss` runs the whole closure in two
kernel launches forward and one backward, with the erosion unconditional and no host synchronisation.  Float32 GPU tensors only;
there is no CPU path (plugin.install(depth_loss=True) keeps the replaced functions for everything else).
"""
from __future__ import annotations

import ctypes as C
from typing import Union

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from ._call import _check_cuda_f32, call, invoke, ptr

FUSED_MAX_KSIZE = 17
_WEIGHTS = {}


def row_weights(height: int, device) -> Tensor:
    """sin((h + 0.5) pi / H) per ERP row, float32, with the reference's own torch expression (model_wrapper_helper.py:77-78) on
    `device`, so that every term is the reference's to the bit.  Cached per (height, device)."""
    device = torch.device(device)
    key = (int(height), device)
    w = _WEIGHTS.get(key)
    if w is None:
        w = torch.arange(0, height, dtype=torch.float32, device=device)
        w = torch.sin((w + 0.5) * torch.pi / height)
        _WEIGHTS[key] = w
    return w


def erode(bin_img: Tensor, ksize: int = 5) -> Tensor:
    """The reference's erode (model_wrapper_helper.py:4-24): 1 - max_pool(reflect_pad(1 - x)) over ksize x ksize, for [C,H,W]
    or [N,C,H,W] float32 GPU tensors; bit-identical to torch's expression for any input, NaN and inf included.  No autograd
    (the reference's mask carries none).  ValueError for an even ksize, a pad (ksize - 1) / 2 >= H or W, or another rank."""
    if bin_img.dim() not in (3, 4):
        raise ValueError(f"erode expects a [C,H,W] or [N,C,H,W] tensor, got shape {tuple(bin_img.shape)}")
    _check_cuda_f32("erode", bin_img)
    ksize = int(ksize)
    h, w = int(bin_img.shape[-2]), int(bin_img.shape[-1])
    pad = (ksize - 1) // 2
    if ksize < 1 or ksize % 2 == 0:
        raise ValueError(f"erode needs an odd ksize, got {ksize}")
    if pad >= h or pad >= w:
        raise ValueError(f"erode: reflect padding {pad} needs H, W > {pad}, got {h}x{w}")
    x = bin_img.detach().contiguous()
    out = torch.empty_like(x)
    planes = x.numel() // max(h * w, 1)
    if planes == 0:
        return out
    call("s360_erode", x.device, ptr(x), ptr(out), planes, h, w, ksize)
    return out


def _forward(pred, target, mask, keep_batch, far, near, fill, ksize):
    b, v, h, w = (int(s) for s in pred.shape)
    n = b if keep_batch else 1
    loss = torch.empty(n, dtype=torch.float32, device=pred.device)
    den = torch.empty(n, dtype=torch.float32, device=pred.device)
    wts = row_weights(h, pred.device)
    nbytes = C.c_size_t(0)
    args = (ptr(wts), b, v, h, w, int(keep_batch), ptr(far), C.c_float(near), C.c_float(fill), int(ksize))
    invoke("s360_l1_sphere_forward", None, None, ptr(mask), *args, None, None, None, C.byref(nbytes), None)
    ws = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=pred.device)
    call("s360_l1_sphere_forward", pred.device, ptr(pred), ptr(target), ptr(mask), *args, ptr(loss), ptr(den), ptr(ws), C.byref(nbytes))
    return loss, den


def _backward(g, pred, target, mask, den, keep_batch, far, near, fill, ksize, need_target):
    b, v, h, w = (int(s) for s in pred.shape)
    g = g.to(torch.float32).reshape(-1).contiguous()
    gp = torch.empty_like(pred)
    gt = torch.empty_like(pred) if need_target else None
    call("s360_l1_sphere_backward", pred.device, ptr(pred), ptr(target), ptr(mask), ptr(row_weights(h, pred.device)), b, v, h, w,
         int(keep_batch), ptr(far), C.c_float(near), C.c_float(fill), int(ksize), ptr(g), ptr(den), ptr(gp), ptr(gt))
    return gp, gt


class _L1Sphere(torch.autograd.Function):
    """loss(pred, target; mask) with the reference's autograd chain; mask None = the fused closure (mask from target)."""

    @staticmethod
    def forward(ctx, pred, target, mask, far, keep_batch, near, fill, ksize):
        pred, target = pred.detach().contiguous(), target.detach().contiguous()
        mask = mask.detach().contiguous() if mask is not None else None
        loss, den = _forward(pred, target, mask, keep_batch, far, near, fill, ksize)
        ctx.save_for_backward(pred, target, mask, far, den)
        ctx.opts = (keep_batch, near, fill, ksize)
        return loss if keep_batch else loss.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, target, mask, far, den = ctx.saved_tensors
        keep_batch, near, fill, ksize = ctx.opts
        need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_p or need_t):
            return (None,) * 8
        gp, gt = _backward(g, pred, target, mask, den, keep_batch, far, near, fill, ksize, need_t)
        return (gp if need_p else None), gt, None, None, None, None, None, None


def _check_bvhw(what: str, *ts: Tensor) -> None:
    if ts[0].dim() != 4:
        raise ValueError(f"{what} expects [B,V,H,W] tensors, got shape {tuple(ts[0].shape)}")
    for t in ts[1:]:
        if t.shape != ts[0].shape:
            raise ValueError(f"{what} expects tensors of one [B,V,H,W] shape, got {tuple(ts[0].shape)} and {tuple(t.shape)}")


def compute_l1_sphere_loss(y_pred: Tensor, y_true: Tensor, mask: Tensor = None, keep_batch: bool = False) -> Tensor:
    """The reference's compute_l1_sphere_loss (model_wrapper_helper.py:63-90): sum |t - p| sin(phi_h) m / clamp_away_from(sum
    sin(phi_h) m, 0, 1e-10) over [B,V,H,W] -> 0-d tensor (keep_batch: [B]) in y_pred's dtype.  Differentiable in y_pred and
    y_true (torch's chain, once).  mask=None raises NotImplementedError, as the reference does.  Float32 GPU tensors of one
    shape; the mask takes no gradient.  Two kernels forward, one backward, on the current stream; no host synchronisation."""
    if mask is None:
        raise NotImplementedError
    _check_bvhw("compute_l1_sphere_loss", y_pred, y_true, mask)
    _check_cuda_f32("compute_l1_sphere_loss", y_pred, y_true, mask)
    if mask.requires_grad:
        raise ValueError("compute_l1_sphere_loss: the mask takes no gradient")
    if y_pred.numel() == 0:
        raise ValueError("compute_l1_sphere_loss: empty tensors")
    return _L1Sphere.apply(y_pred, y_true, mask, None, bool(keep_batch), 0.0, 0.0, 1)


def context_depth_loss(pred_depth: Tensor, depth_sphere: Tensor, far: Union[Tensor, float], *, near_threshold: float = 0.1,
                       fill_below: float = 1e-7, weight: float = 0.1, ksize: int = 5) -> Tensor:
    """The reference's compute_context_depth_loss closure (model_wrapper_erp.py:242-287) on [B,V,H,W] float32 GPU tensors:

        mask = erode(depth_sphere > near_threshold)        # unconditional: eroding an all-ones mask gives all ones
        target = where(depth_sphere < fill_below, far, depth_sphere)
        weight * compute_l1_sphere_loss(pred_depth, target, mask)

    in two kernels forward and one backward (the eroded mask is recomputed from the depth there), with no host
    synchronisation: `far` is read on the device (a 0-d or 1-element tensor, e.g. batch['context']['far'][0, 0], or a
    number).  Unlike the reference, depth_sphere is NOT modified in place (the reference writes far into it); it takes no
    gradient.  `weight` is a plain torch multiply after the loss, as in the reference, so the gradient scales the same way."""
    _check_bvhw("context_depth_loss", pred_depth, depth_sphere)
    _check_cuda_f32("context_depth_loss", pred_depth, depth_sphere)
    ksize = int(ksize)
    h, w = int(pred_depth.shape[2]), int(pred_depth.shape[3])
    if ksize < 1 or ksize % 2 == 0 or ksize > FUSED_MAX_KSIZE:
        raise ValueError(f"context_depth_loss needs an odd ksize <= {FUSED_MAX_KSIZE}, got {ksize}")
    if (ksize - 1) // 2 >= h or (ksize - 1) // 2 >= w:
        raise ValueError(f"context_depth_loss: reflect padding {(ksize - 1) // 2} needs H, W > {(ksize - 1) // 2}, got {h}x{w}")
    if pred_depth.numel() == 0:
        raise ValueError("context_depth_loss: empty tensors")
    if isinstance(far, Tensor):
        if far.numel() != 1:
            raise ValueError(f"context_depth_loss: far must hold one value, got shape {tuple(far.shape)}")
        if far.device != pred_depth.device:
            raise ValueError(f"context_depth_loss: far is on {far.device}, the depths on {pred_depth.device}")
        far_t = far.detach().reshape(1).to(torch.float32).contiguous()
    else:
        far_t = torch.full((1,), float(far), dtype=torch.float32, device=pred_depth.device)
    loss = _L1Sphere.apply(pred_depth, depth_sphere.detach(), None, far_t, False, float(near_threshold), float(fill_below), ksize)
    return weight * loss
