"""The tail of the multi-view transformer's TransformerLayer on the GPU, forward and backward (csrc/s360_transformer_ffn.hip).

Behind its attention the reference's TransformerLayer.forward (src/model/encoder/backbone/multiview_transformer.py:407-414) runs

    message = norm1(merge(message))
    message = mlp(cat([source, message], -1))      # Linear 2C -> 8C, GELU, Linear 8C -> C, no biases
    message = norm2(message)
    return source + message

and, with no_ffn, `source + norm1(merge(message))`.  Autograd of those lines keeps the [T, 2C] concatenation and both [T, 8C]
activations per layer (0.6 GB at the ERP shape, T = 65 536).  `ffn_tail` computes the same function with one fused forward kernel and
a three-launch backward that recompute the hidden activations: the autograd node saves source, m, the second Linear's output z
[T, C], one float64 (mean, rstd) pair per token and norm, and the parameters.  `layer_norm_residual` is the no_ffn tail.  The firm
gain is memory; speed against torch's rocBLAS path is what profiles/transformer_ffn_timing.json says it is.  Float32 GPU tensors,
C = 128 and hidden width 1024 (what both backbones use); there is no CPU path (the installed seam keeps the replaced method for
everything else).  Forward and backward are bit-identical from run to run: fixed order, no atomics.

precision="highest" (the default) forms every product from exact float32 products; precision="high" is what
torch.set_float32_matmul_precision('high') asks for: each float32 number as the sum of two bfloat16 numbers and each product of the
forward and the backward as Ah Bh + Ah Bl + Al Bh on the bf16 MFMA, float32 accumulation (the LayerNorm rows stay float64).  The
weights are split once per call into 3 MiB of bf16 planes in a scratch buffer; the token side is split inside the kernels, so the
"high" mode saves what "highest" saves.  A forward run in one precision takes its backward in the same one.
`precision.resolve("torch")` reads torch's setting at call time.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from . import precision as _prec
from ._args import buffers as _buffers, eps as _eps, flat as _flat, high_scratch as _high_scratch, no_scratch as _no_scratch, \
    positive_int as _positive, tensor_rule
from ._call import call, ptr
from .precision import PRECISIONS  # noqa: F401  (the name callers of this module use)

CHANNELS = 128
HIDDEN = 1024
FFN_GRADIENTS = ("g_source", "g_m", "g_norm1_weight", "g_norm1_bias", "g_w1", "g_w2", "g_norm2_weight", "g_norm2_bias")
NORM_GRADIENTS = ("g_x", "g_weight", "g_bias", "g_residual")
_tensor = tensor_rule(ValueError, "{what}: {name} must be a GPU tensor (there is no CPU path), got device {device}")


def scratch_bytes(tokens: int, backward: bool, precision: str = "highest") -> int:
    """The bytes of scratch a forward (backward) call of ffn_tail allocates for `tokens` tokens: "highest" none for the forward
    and s360_ffn_tail_scratch_bytes for the backward; "high" s360_ffn_tail_high_scratch_bytes, the same plus the weights' bf16
    planes, whose size does not depend on tokens.  0 for tokens < 1."""
    _prec.check("ffn_tail", precision)
    tokens = int(tokens)
    if precision == "high":
        return int(_lib.lib().s360_ffn_tail_high_scratch_bytes(tokens, int(bool(backward))))
    return int(_lib.lib().s360_ffn_tail_scratch_bytes(tokens)) if backward else 0


def supported_widths(channels: int, hidden: int = HIDDEN) -> bool:
    return channels == CHANNELS and hidden == HIDDEN


def weight_chunks(tokens: int) -> int:
    """How many token chunks the weight-gradient pass of ffn_tail's backward uses for `tokens` tokens (at most 16, each a multiple
    of 32 tokens but for the last)."""
    tokens = _positive("weight_chunks", "tokens", tokens)
    return int(_lib.lib().s360_ffn_tail_weight_chunks(tokens))


def _rows(what: str, name: str, t) -> int:
    """Tokens of a [..., C] tensor with C = 128."""
    _tensor(what, name, t)
    if t.dim() < 1 or t.shape[-1] != CHANNELS:
        raise ValueError(f"{what} takes {name} [..., C] with C = {CHANNELS}, got shape {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{what}: {name} is empty, shape {tuple(t.shape)}")
    return t.numel() // CHANNELS


def _checked_ffn(what: str, source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps) -> int:
    tokens = _rows(what, "source", source)
    _tensor(what, "m", m, source.shape, device=source.device)
    _tensor(what, "w1", w1, device=source.device)
    _tensor(what, "w2", w2, device=source.device)
    if tuple(w1.shape) != (HIDDEN, 2 * CHANNELS) or tuple(w2.shape) != (CHANNELS, HIDDEN):
        raise ValueError(f"{what} takes w1 [{HIDDEN}, {2 * CHANNELS}] and w2 [{CHANNELS}, {HIDDEN}] (hidden width {HIDDEN}), got "
                         f"{tuple(w1.shape)} and {tuple(w2.shape)}")
    for name, t in (("norm1_weight", norm1_weight), ("norm1_bias", norm1_bias), ("norm2_weight", norm2_weight), ("norm2_bias", norm2_bias)):
        _tensor(what, name, t, (CHANNELS,), device=source.device)
    _eps(what, eps)
    return tokens


def _checked_norm(what: str, x, weight, bias, residual, eps) -> int:
    tokens = _rows(what, "x", x)
    _tensor(what, "residual", residual, x.shape, device=x.device)
    _tensor(what, "weight", weight, (CHANNELS,), device=x.device)
    _tensor(what, "bias", bias, (CHANNELS,), device=x.device)
    _eps(what, eps)
    return tokens


def ffn_tail_forward(source: Tensor, m: Tensor, norm1_weight: Tensor, norm1_bias: Tensor, w1: Tensor, w2: Tensor, norm2_weight: Tensor,
                     norm2_bias: Tensor, eps: float = 1e-5, *, precision: str = "highest", scratch: Optional[Tensor] = None) -> tuple:
    """s360_ffn_tail_forward (precision "high": s360_ffn_tail_high_forward) -> (out in source's shape, z [T, C] float32, stats
    [2, T, 2] float64).  `scratch`: a uint8 buffer of scratch_bytes(T, False, "high") bytes for the "high" call to use in place
    of one it allocates; refused (ValueError) with any other precision, whose forward has no scratch."""
    _prec.check("ffn_tail", precision)
    _no_scratch("ffn_tail_forward", precision, scratch)
    tokens = _checked_ffn("ffn_tail_forward", source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps)
    args = [_flat(t) for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias)]
    out = torch.empty(source.shape, dtype=torch.float32, device=source.device)
    z = torch.empty(tokens, CHANNELS, dtype=torch.float32, device=source.device)
    stats = torch.empty(2, tokens, 2, dtype=torch.float64, device=source.device)
    common = (*(ptr(t) for t in args), tokens, CHANNELS, HIDDEN, C.byref(C.c_double(float(eps))), ptr(out), ptr(z), ptr(stats))
    if precision == "high":
        scratch = _high_scratch("ffn_tail_forward", scratch_bytes(tokens, False, "high"), source.device, scratch, _tensor)
        call("s360_ffn_tail_high_forward", source.device, *common, ptr(scratch), scratch.numel())
    else:
        call("s360_ffn_tail_forward", source.device, *common)
    return out, z, stats


def ffn_tail_backward(source: Tensor, m: Tensor, norm1_weight: Tensor, norm1_bias: Tensor, w1: Tensor, w2: Tensor, norm2_weight: Tensor,
                      norm2_bias: Tensor, z: Tensor, stats: Tensor, g_out: Tensor, eps: float = 1e-5, *, buffers: Optional[dict] = None,
                      precision: str = "highest", scratch: Optional[Tensor] = None) -> tuple:
    """s360_ffn_tail_backward (precision "high": s360_ffn_tail_high_backward, with z and stats of a "high" forward) -> the
    gradients in FFN_GRADIENTS' order (the order of ffn_tail's arguments).  `buffers`: {name: contiguous float32 buffer} for any of
    them to write into; the others are allocated.  `scratch`: as in ffn_tail_forward, scratch_bytes(T, True, "high") bytes, refused with
    any other precision (the "highest" backward allocates its own)."""
    what = "ffn_tail_backward"
    _prec.check("ffn_tail", precision)
    _no_scratch(what, precision, scratch)
    tokens = _checked_ffn(what, source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps)
    _tensor(what, "g_out", g_out, source.shape, device=source.device)
    _tensor(what, "z", z, (tokens, CHANNELS), device=source.device)
    _tensor(what, "stats", stats, (2, tokens, 2), dtype=torch.float64, device=source.device)
    ins = [_flat(t) for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, z, stats, g_out)]
    shapes = [t.shape for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias)]
    outs = dict(zip(FFN_GRADIENTS, _buffers(what, FFN_GRADIENTS, shapes, [torch.float32] * 8, source.device, buffers, _tensor)))
    if precision == "high":
        scratch = _high_scratch(what, scratch_bytes(tokens, True, "high"), source.device, scratch, _tensor)
    else:
        scratch = _prec.scratch(_lib.lib().s360_ffn_tail_scratch_bytes(tokens), source.device)
    order = ("g_source", "g_m", "g_w1", "g_w2", "g_norm1_weight", "g_norm1_bias", "g_norm2_weight", "g_norm2_bias")
    call("s360_ffn_tail_high_backward" if precision == "high" else "s360_ffn_tail_backward", source.device, *(ptr(t) for t in ins), tokens, CHANNELS, HIDDEN, C.byref(C.c_double(float(eps))),
         ptr(scratch), scratch.numel(), *(ptr(outs[n]) for n in order))
    return tuple(outs[n] for n in FFN_GRADIENTS)


def layer_norm_residual_forward(x: Tensor, weight: Tensor, bias: Tensor, residual: Tensor, eps: float = 1e-5) -> tuple:
    """s360_layer_norm_residual_forward -> (out in x's shape, stats [T, 2] float64)."""
    tokens = _checked_norm("layer_norm_residual_forward", x, weight, bias, residual, eps)
    args = [_flat(t) for t in (x, weight, bias, residual)]
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    stats = torch.empty(tokens, 2, dtype=torch.float64, device=x.device)
    call("s360_layer_norm_residual_forward", x.device, *(ptr(t) for t in args), tokens, CHANNELS, C.byref(C.c_double(float(eps))),
         ptr(out), ptr(stats))
    return out, stats


def layer_norm_residual_backward(x: Tensor, weight: Tensor, stats: Tensor, g_out: Tensor, *, buffers: Optional[dict] = None) -> tuple:
    """s360_layer_norm_residual_backward -> (g_x, g_weight, g_bias, g_residual), NORM_GRADIENTS' order."""
    what = "layer_norm_residual_backward"
    tokens = _rows(what, "x", x)
    _tensor(what, "weight", weight, (CHANNELS,), device=x.device)
    _tensor(what, "g_out", g_out, x.shape, device=x.device)
    _tensor(what, "stats", stats, (tokens, 2), dtype=torch.float64, device=x.device)
    ins = [_flat(t) for t in (x, weight, stats, g_out)]
    shapes = [t.shape for t in (x, weight, weight, x)]
    outs = dict(zip(NORM_GRADIENTS, _buffers(what, NORM_GRADIENTS, shapes, [torch.float32] * 4, x.device, buffers, _tensor)))
    scratch = _prec.scratch(_lib.lib().s360_ffn_tail_scratch_bytes(tokens), x.device)
    call("s360_layer_norm_residual_backward", x.device, *(ptr(t) for t in ins), tokens, CHANNELS, ptr(scratch), scratch.numel(),
         ptr(outs["g_x"]), ptr(outs["g_residual"]), ptr(outs["g_weight"]), ptr(outs["g_bias"]))
    return tuple(outs[n] for n in NORM_GRADIENTS)


class _FFNTail(torch.autograd.Function):
    """Saves source, m, z [T, C], the statistics and the parameters: nothing of size [T, 2C] or [T, 8C] and, in the "high" mode,
    none of the bf16 planes (the backward splits the weights again)."""

    @staticmethod
    def forward(ctx, source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps, precision):
        args = [_flat(t) for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias)]
        out, z, stats = ffn_tail_forward(*args, eps, precision=precision)
        ctx.save_for_backward(*args, z, stats)
        ctx.eps, ctx.precision = eps, precision
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        *args, z, stats = ctx.saved_tensors
        return (*ffn_tail_backward(*args, z, stats, g_out.to(torch.float32), ctx.eps, precision=ctx.precision), None, None)


class _LayerNormResidual(torch.autograd.Function):
    """Saves x, the weight and one (mean, rstd) pair per token."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, eps):
        x, weight = _flat(x), _flat(weight)
        out, stats = layer_norm_residual_forward(x, weight, bias, residual, eps)
        ctx.save_for_backward(x, weight, stats)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, weight, stats = ctx.saved_tensors
        return (*layer_norm_residual_backward(x, weight, stats, g_out.to(torch.float32)), None)


def ffn_tail(source: Tensor, m: Tensor, norm1_weight: Tensor, norm1_bias: Tensor, w1: Tensor, w2: Tensor, norm2_weight: Tensor,
             norm2_bias: Tensor, eps: float = 1e-5, precision: str = "highest") -> Tensor:
    """source + LN2(gelu(cat([source, LN1(m)], -1) w1^T) w2^T): the reference's TransformerLayer.forward :408-414 behind
    `message = self.merge(message)`, m being that message.

    source, m [..., C] with any leading dimensions; norm1 / norm2 weight and bias [C] (nn.LayerNorm's affine parameters, biased
    variance, eps); w1 [8C, 2C] and w2 [C, 8C] (nn.Linear's layout, no biases); GELU in the erf form.  Returns a tensor of
    source's shape.  Differentiable (once) in all eight tensors.  Float32 GPU tensors, C = 128 and 8C = 1024; no CPU path; a
    non-contiguous input is copied once.  precision "highest": exact float32 products; "high": bf16x3 products on the bf16 MFMA,
    forward and backward (the module's docstring)."""
    _prec.check("ffn_tail", precision)
    _checked_ffn("ffn_tail", source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps)
    return _FFNTail.apply(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, float(eps), precision)


def layer_norm_residual(x: Tensor, weight: Tensor, bias: Tensor, residual: Tensor, eps: float = 1e-5) -> Tensor:
    """residual + LN(x) weight + bias over the last axis: the tail of the reference's TransformerLayer with no_ffn (:408, :414).
    x, residual [..., C]; weight, bias [C].  Differentiable (once) in all four.  Float32 GPU tensors, C = 128."""
    _checked_norm("layer_norm_residual", x, weight, bias, residual, eps)
    return _LayerNormResidual.apply(x, weight, bias, residual, float(eps))
