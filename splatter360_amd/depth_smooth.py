"""The training step's edge-aware depth-smoothness loss on the GPU: the reference's LossDepth (csrc/s360_depth_smooth.hip).

The reference's third registered loss (src/loss/loss_depth.py:26-60, config/loss/depth.yaml) normalises the rendered depth
between log(near) and log(far), takes first or second differences along both image axes, optionally weights them with
exp(-sigma x the largest signed colour difference) of the target image, and adds the two means of the absolute values: about a
dozen elementwise and reduction launches forward and more backward.  Here the forward is two kernel launches and the backward
one, in float64 per pixel, with nothing saved between them but the inputs and no host synchronisation.  Float32 GPU tensors
only; there is no CPU path (plugin.install(depth_smoothness=True) keeps the replaced method for everything else).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from ._call import call, invoke, ptr


def _args(depth, ln, lf, image, sigma, flags):
    b, v, h, w = (int(s) for s in depth.shape)
    c = int(image.shape[2]) if image is not None else 0
    return (ptr(depth), ptr(ln), ptr(lf), ptr(image), b, v, int(ln.shape[1]), c, h, w, C.c_float(sigma), int(flags))


def _forward(depth, ln, lf, image, sigma, flags) -> Tensor:
    loss = torch.empty((), dtype=torch.float32, device=depth.device)
    args = _args(depth, ln, lf, image, sigma, flags)
    nbytes = C.c_size_t(0)
    invoke("s360_depth_smooth_forward", *args, None, None, C.byref(nbytes), None)
    ws = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=depth.device)
    call("s360_depth_smooth_forward", depth.device, *args, ptr(loss), ptr(ws), C.byref(nbytes))
    return loss


def _backward(g, depth, ln, lf, image, sigma, flags) -> Tensor:
    g = g.to(torch.float32).reshape(1).contiguous()
    grad = torch.empty_like(depth)
    call("s360_depth_smooth_backward", depth.device, *_args(depth, ln, lf, image, sigma, flags), ptr(g), ptr(grad))
    return grad


class _DepthSmooth(torch.autograd.Function):
    """loss(depth; log near, log far, image) with the reference's autograd chain in depth."""

    @staticmethod
    def forward(ctx, depth, ln, lf, image, sigma, flags):
        depth = depth.detach().contiguous()
        ctx.save_for_backward(depth, ln, lf, image)
        ctx.opts = (sigma, flags)
        return _forward(depth, ln, lf, image, sigma, flags)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        depth, ln, lf, image = ctx.saved_tensors
        return _backward(g, depth, ln, lf, image, *ctx.opts), None, None, None, None, None


def depth_smoothness_loss(depth: Tensor, near: Tensor, far: Tensor, image: Optional[Tensor] = None, *,
                          sigma_image: Optional[float] = None, use_second_derivative: bool = False, weight: float = 1.0) -> Tensor:
    """The reference's LossDepth.forward (src/loss/loss_depth.py:34-60) on float32 GPU tensors -> a 0-d float32 tensor:

        n = (depth.minimum(log far).maximum(log near) - log near) / (log far - log near)
        dx, dy = n.diff(-1), n.diff(-2)                      # use_second_derivative: the diff of the diff
        sigma_image is not None:  dx *= exp(-sigma_image * max over channels of image.diff(-1)), dy likewise with diff(-2)
                                  (second derivative: the larger of the two adjacent colour differences)
        weight * (dx.abs().mean() + dy.abs().mean())

    depth [B,V,H,W]; near, far [B,Vn] with Vn dividing V (view v uses bound v // (V // Vn): Vn = 1 and Vn = V are the
    reference's broadcasts, Vn = V // 6 is one bound per panorama of six faces); image [B,V,C,H,W], read only with sigma_image
    and never given a gradient.  The logs are torch's own .log() on the device, so the bounds are the reference's to the bit;
    everything after them is float64 per pixel, rounded to float32 once.  Differentiable in depth only (torch's chain, once:
    sign(0) = 0, halves at the ties of minimum / maximum).  `weight` is a plain torch multiply on the result, as in the
    reference.  Two kernels forward, one backward, on the current stream; no host synchronisation, so near <= 0 or near == far
    are not caught: they give non-finite results, as in the reference.
    RuntimeError for CPU tensors; ValueError for another rank, shape or dtype, H or W <= the derivative order, an image that
    requires grad, or sigma_image without an image."""
    what = "depth_smoothness_loss"
    order = 2 if use_second_derivative else 1
    if sigma_image is not None and image is None:
        raise ValueError(f"{what}: sigma_image needs an image")
    if sigma_image is None:
        image = None
    tensors = [t for t in (depth, near, far, image) if t is not None]
    for t in tensors:
        if not isinstance(t, Tensor):
            raise ValueError(f"{what} takes tensors, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU only (no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} takes float32 tensors, got {t.dtype}")
        if t.device != depth.device:
            raise ValueError(f"{what}: tensors on different devices ({depth.device}, {t.device})")
    if depth.dim() != 4 or depth.numel() == 0:
        raise ValueError(f"{what} expects a non-empty [B,V,H,W] depth, got shape {tuple(depth.shape)}")
    b, v, h, w = (int(s) for s in depth.shape)
    if h <= order or w <= order:
        raise ValueError(f"{what}: a derivative of order {order} needs H, W > {order}, got {h}x{w}")
    if near.dim() != 2 or near.shape != far.shape or near.shape[0] != b or near.shape[1] < 1 or v % int(near.shape[1]) != 0:
        raise ValueError(f"{what} expects near and far of one shape [B,Vn] with Vn dividing V = {v}, got {tuple(near.shape)} and "
                         f"{tuple(far.shape)}")
    flags = _lib.DS_SECOND if use_second_derivative else 0
    if image is not None:
        if image.dim() != 5 or image.shape[2] < 1 or (image.shape[0], image.shape[1], image.shape[3], image.shape[4]) != (b, v, h, w):
            raise ValueError(f"{what} expects an image [B,V,C,H,W] matching the depth {tuple(depth.shape)}, got {tuple(image.shape)}")
        if image.requires_grad:
            raise ValueError(f"{what}: the image takes no gradient")
        image = image.contiguous()
        flags |= _lib.DS_BILATERAL
    ln, lf = near.detach().log().contiguous(), far.detach().log().contiguous()
    loss = _DepthSmooth.apply(depth, ln, lf, image, float(sigma_image) if sigma_image is not None else 0.0, flags)
    return weight * loss
