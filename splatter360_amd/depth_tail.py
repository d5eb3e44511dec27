"""The encoder's fine-depth and opacity tail on the GPU, forward and backward (csrc/s360_depth_tail.hip).

The elementwise stretch of the reference's predictor and encoder that lies between the networks and the Gaussian adapter:

    coarse_disps = 1 / coarse_depths;  pdf_max = F.interpolate(pdf_max, scale_factor=s)                       (depth_predictor_
    fullres_disps = F.interpolate(coarse_disps, scale_factor=s, mode="bilinear", align_corners=True)           multiview_360.py:650-658)
    delta_disps, raw_densities = delta_disps_density.split(gpp, dim=1);  densities = sigmoid(raw_densities)    (:694-719)
    depths = 1 / (fullres_disps + delta_disps).clamp(1 / far, 1 / near),  both "(v b) dpt h w -> b v (h w) srf dpt"
    opacities = 0.5 * (1 - (1 - densities) ** e + densities ** (1 / e)) / gpp                                  (encoder_costvolume.py:228-241, :420)

`fullres_maps` is the first three lines in two launches (two more backward), `fine_depth_tail` the rest in one (one more
backward), writing the [b, v, H W, 1, gpp] tensors the adapter consumes directly; `upsample` and `map_pdf_to_opacity` are the single
statements, which plugin.install(depth_tail=True) puts behind the predictor module's F.interpolate and the encoder's
map_pdf_to_opacity.  The tail differentiates the opacity in the density LOGIT, so its gradient is finite for every finite logit;
torch's float32 autograd of the statement gives NaN once the sigmoid rounds to 0 or 1.  Float32 GPU tensors only; there is no
CPU path (the installed seams keep the replaced functions for everything else).  Float64 arithmetic rounded once, fixed order, no
atomics: forward and backward are bit-identical from run to run.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from ._call import _check_cuda_f32, call, ptr

MODES = {"nearest": 0, "bilinear": 1}


def _scale(scale_factor) -> int:
    if isinstance(scale_factor, bool) or not isinstance(scale_factor, (int, float)) or scale_factor != int(scale_factor) or scale_factor < 1:
        raise ValueError(f"upsample takes an integer scale_factor >= 1, got {scale_factor!r}")
    return int(scale_factor)


def _grad(g):
    return None if g is None else g.to(torch.float32).contiguous()


class _Upsample(torch.autograd.Function):
    """One [n, 1, h, w] map to [n, 1, h s, w s]; saves the input only when it samples the reciprocal."""

    @staticmethod
    def forward(ctx, x, s, mode, reciprocal):
        x = x.detach().contiguous()
        n, _, h, w = (int(d) for d in x.shape)
        out = torch.empty(n, 1, h * s, w * s, dtype=torch.float32, device=x.device)
        call("s360_upsample_forward", x.device, ptr(x), ptr(out), n, h, w, s, mode, int(reciprocal))
        ctx.save_for_backward(*((x,) if reciprocal else ()))
        ctx.args = (n, h, w, s, mode, bool(reciprocal))
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        n, h, w, s, mode, reciprocal = ctx.args
        x = ctx.saved_tensors[0] if reciprocal else None
        g_out = _grad(g_out)
        g_x = torch.empty(n, 1, h, w, dtype=torch.float32, device=g_out.device)
        call("s360_upsample_backward", g_out.device, ptr(g_out), ptr(x), ptr(g_x), n, h, w, s, mode, int(reciprocal))
        return g_x, None, None, None


def upsample(x: Tensor, scale_factor, mode: str = "nearest", reciprocal: bool = False) -> Tensor:
    """F.interpolate(x, scale_factor=s) (mode "nearest": source index Y // s) or F.interpolate(x, scale_factor=s, mode="bilinear",
    align_corners=True) of one [n, 1, h, w] map for an integer s >= 1, in one kernel; reciprocal=True upsamples 1 / x instead,
    without storing it.  The bilinear source coordinate is exact in integers; values are weighed in float64 and rounded once.
    Once-differentiable: the backward is the adjoint as a gather (no atomics), times -1 / x^2 with reciprocal.  Float32 GPU tensors;
    no CPU path; a non-contiguous x is copied."""
    if mode not in MODES:
        raise ValueError(f"upsample knows the modes {sorted(MODES)}, got {mode!r}")
    s = _scale(scale_factor)
    if x.dim() != 4 or x.shape[1] != 1:
        raise ValueError(f"upsample expects an [n, 1, h, w] map, got shape {tuple(x.shape)}")
    _check_cuda_f32("upsample", x)
    if x.numel() == 0:
        raise ValueError("upsample: empty tensor")
    return _Upsample.apply(x, s, MODES[mode], bool(reciprocal))


def fullres_maps(coarse_depths: Tensor, pdf_max: Tensor, upscale_factor) -> tuple:
    """The reference's :650-658 after the depth head: (fullres_disps, pdf_max_full), both [n, 1, h s, w s] —
    the bilinear align_corners=True upsampling of 1 / coarse_depths and the nearest upsampling of pdf_max.  Two launches forward,
    two backward."""
    return upsample(coarse_depths, upscale_factor, "bilinear", reciprocal=True), upsample(pdf_max, upscale_factor, "nearest")


def opacity_exponent(initial, final, warm_up, global_step) -> float:
    """The exponent of the reference's map_pdf_to_opacity (encoder_costvolume.py:236-238) for its cfg.opacity_mapping fields."""
    x = initial + min(global_step / warm_up, 1) * (final - initial)
    return float(2 ** x)


def _exponent(exponent) -> float:
    e = C.c_float(float(exponent)).value                        # the ABI takes a float32, as torch does for a float32 tensor
    if not math.isfinite(e) or e <= 0:
        raise ValueError(f"the opacity exponent must be finite and positive, got {exponent!r}")
    return e


class _FineDepthTail(torch.autograd.Function):
    """(depths, opacities[, densities]) of the full-resolution disparity and the U-Net's delta / density logits; saves its inputs
    only."""

    @staticmethod
    def forward(ctx, fullres, delta_density, lo, hi, v, gpp, exponent, return_densities):
        fullres, delta_density = fullres.detach().contiguous(), delta_density.detach().contiguous()
        n, _, h, w = (int(d) for d in fullres.shape)
        outs = tuple(torch.empty(n // v, v, h * w, 1, gpp, dtype=torch.float32, device=fullres.device) for _ in range(3 if return_densities else 2))
        call("s360_depth_tail_forward", fullres.device, ptr(fullres), ptr(delta_density), ptr(lo), ptr(hi), exponent, gpp, v, ptr(outs[0]),
             ptr(outs[1]), ptr(outs[2] if return_densities else None), n, h, w)
        ctx.save_for_backward(fullres, delta_density, lo, hi)
        ctx.args = (n, h, w, v, gpp, exponent)
        ctx.set_materialize_grads(False)                        # an unused output hands None, which the kernel takes as zero
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *g_outs):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 8
        fullres, delta_density, lo, hi = ctx.saved_tensors
        n, h, w, v, gpp, exponent = ctx.args
        g = [_grad(x) for x in g_outs] + [None] * (3 - len(g_outs))
        g_fullres, g_delta = torch.empty_like(fullres), torch.empty_like(delta_density)
        call("s360_depth_tail_backward", fullres.device, ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(fullres), ptr(delta_density), ptr(lo), ptr(hi),
             exponent, gpp, v, ptr(g_fullres), ptr(g_delta), n, h, w)
        return g_fullres, g_delta, None, None, None, None, None, None


def fine_depth_tail(fullres_disps: Tensor, delta_disps_density: Tensor, near: Tensor, far: Tensor, *, views: int,
                    gaussians_per_pixel: int = 1, exponent: float = 1.0, return_densities: bool = False) -> tuple:
    """The reference's :694-719 with the encoder's map_pdf_to_opacity and / gpp (encoder_costvolume.py:228-241, :420) as one
    kernel: fullres_disps [(v b), 1, H, W], delta_disps_density [(v b), 2 gpp, H, W] (the U-Net's to_disparity output: disparity
    deltas, then density logits), near and far [b, v] ->

        depths = 1 / (fullres_disps + delta_disps).clamp(1 / far, 1 / near),   opacities = map_pdf_to_opacity(sigmoid(raw_densities)) / gpp

    (and densities = sigmoid(raw_densities) with return_densities), each [b, v, H W, 1, gpp]: the reference's
    "(v b) dpt h w -> b v (h w) srf dpt" is done by the store.  `exponent` is opacity_exponent(...) of the step.  Differentiable
    once in the first two arguments; the clamp passes the gradient where 1 / far <= sum <= 1 / near, bounds included, decided on
    the float32 sum as torch decides it (the values come from the unrounded sum); the opacity's gradient is taken in the logit and is finite for every finite logit.
    Float32 GPU tensors; no CPU path."""
    gpp, v = int(gaussians_per_pixel), int(views)
    if fullres_disps.dim() != 4 or fullres_disps.shape[1] != 1:
        raise ValueError(f"fine_depth_tail expects fullres_disps [(v b), 1, H, W], got shape {tuple(fullres_disps.shape)}")
    _check_cuda_f32("fine_depth_tail", fullres_disps, delta_disps_density, near, far)
    n, _, h, w = (int(d) for d in fullres_disps.shape)
    if gpp < 1 or v < 1 or n == 0 or n % v != 0 or h * w == 0:
        raise ValueError(f"fine_depth_tail: views={views}, gaussians_per_pixel={gaussians_per_pixel} do not fit fullres_disps {tuple(fullres_disps.shape)}")
    if tuple(delta_disps_density.shape) != (n, 2 * gpp, h, w):
        raise ValueError(f"fine_depth_tail expects delta_disps_density {(n, 2 * gpp, h, w)}, got {tuple(delta_disps_density.shape)}")
    if tuple(near.shape) != (n // v, v) or tuple(far.shape) != (n // v, v):
        raise ValueError(f"fine_depth_tail expects near and far [b, v] = {(n // v, v)}, got {tuple(near.shape)} and {tuple(far.shape)}")
    # [2, v, b]: the reference's float32 1.0 / far, 1.0 / near in (v b) order (torch forms 1.0 / x as x.reciprocal() * 1.0)
    bounds = torch.stack((far.detach().t(), near.detach().t())).reciprocal()
    return _FineDepthTail.apply(fullres_disps, delta_disps_density, bounds[0].reshape(-1), bounds[1].reshape(-1), v, gpp, _exponent(exponent),
                                bool(return_densities))


class _OpacityMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pdf, exponent):
        pdf = pdf.detach().contiguous()
        out = torch.empty_like(pdf)
        call("s360_opacity_map_forward", pdf.device, ptr(pdf), ptr(out), pdf.numel(), exponent)
        ctx.save_for_backward(pdf)
        ctx.exponent = exponent
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        if g_out is None or not ctx.needs_input_grad[0]:
            return None, None
        (pdf,) = ctx.saved_tensors
        g_out = _grad(g_out)
        g_pdf = torch.empty_like(pdf)
        call("s360_opacity_map_backward", pdf.device, ptr(pdf), ptr(g_out), ptr(g_pdf), pdf.numel(), ctx.exponent)
        return g_pdf, None


def map_pdf_to_opacity(pdf: Tensor, exponent: float) -> Tensor:
    """The reference's map_pdf_to_opacity (encoder_costvolume.py:241) for a tensor of probabilities of any shape and the exponent
    of the step: 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent)), one kernel forward and one backward.  The derivative is
    taken in pdf and mirrors the reference's: infinite at pdf = 0 (exponent > 1) or 1 (exponent < 1).  Float32 GPU tensors; no CPU
    path."""
    _check_cuda_f32("map_pdf_to_opacity", pdf)
    if pdf.numel() == 0:
        raise ValueError("map_pdf_to_opacity: empty tensor")
    return _OpacityMap.apply(pdf, _exponent(exponent))


def _native_interpolate_call(args, kwargs):
    """(input, s, mode) if F.interpolate(*args, **kwargs) is a call `upsample` computes — a float32 GPU [n, 1, h, w] input, an
    integer scale_factor and either the default nearest mode or mode="bilinear", align_corners=True, nothing else — else None."""
    names = ("input", "size", "scale_factor", "mode", "align_corners")
    if len(args) > len(names) or any(k not in names for k in kwargs) or any(n in kwargs for n in names[:len(args)]):
        return None
    call = {"size": None, "scale_factor": None, "mode": "nearest", "align_corners": None, **dict(zip(names, args)), **kwargs}
    x, s, mode = call.get("input"), call["scale_factor"], call["mode"]
    if not (isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 1 and x.numel() > 0):
        return None
    if call["size"] is not None or isinstance(s, bool) or not isinstance(s, (int, float)) or s != int(s) or s < 1:
        return None
    if (mode, call["align_corners"]) not in (("nearest", None), ("bilinear", True)):
        return None
    return x, int(s), mode


class InterpolateProxy:
    """Stands in for the name `F` (torch.nn.functional) of the predictor's module: every attribute is the replaced object's own
    (torch.nn.functional, or the depth head's proxy when both are installed), except that `interpolate` runs `upsample` for the
    calls it computes (_native_interpolate_call) and hands every other call to the replaced interpolate untouched."""

    def __init__(self, replaced):
        self.replaced = replaced

    def __getattr__(self, name):
        if name == "replaced":                                  # not set yet (copying, unpickling): no recursion
            raise AttributeError(name)
        return getattr(self.replaced, name)

    def interpolate(self, *args, **kwargs):
        call = _native_interpolate_call(args, kwargs)
        if call is None:
            return self.replaced.interpolate(*args, **kwargs)
        return upsample(call[0], call[1], call[2])
