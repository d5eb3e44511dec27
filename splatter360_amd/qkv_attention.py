"""The U-Nets' multi-head QKV attention on the GPU, forward and backward (csrc/s360_qkv_attention.hip).

The reference's AttentionBlocks (src/model/encoder/costvolume/ldm_unet/unet.py:310-380) run QKVAttentionLegacy (:527-565) — or
QKVAttention (:572-599) with use_new_attention_order — on the output of a 1x1 convolution, qkv [N, heads 3 ch, T]: with
use_cross_view_self_attn the views move from the batch rows into the sequence ("(v b) n t -> b n (v t)"), a float32
[b heads, L, L] weight tensor and its softmax are formed (268 MB each per batch element at the hm3d shape: 4 heads, L = 4 096),
autograd keeps them, and the reference's checkpoint forms them again in the backward.  `qkv_attention` computes the same function
with one fused kernel pair that reads qkv where it lies — channel-major, heads interleaved, the joint sequence spread over the
(v b) rows — and writes `a` and g_qkv where they belong: no score-sized tensor and no permuted copy exists, forward or backward,
and the autograd node saves qkv and one float64 log-sum-exp per (batch element, head, joint token).  The firm gain is memory;
speed against torch's rocBLAS path is what profiles/qkv_attention_timing.json says it is.  Float32 GPU tensors with ch = 32
(what both U-Nets use); there is no CPU path (the installed seam keeps the replaced methods for everything else).  Forward and backward are
bit-identical from run to run: fixed order, no atomics.

precision="highest" (the default) forms every product from exact float32 products; precision="high" is what
torch.set_float32_matmul_precision('high') asks for, as in window_attention.py: each float32 number as the sum of two bfloat16
numbers and each product A B as Ah Bh + Ah Bl + Al Bh on the bf16 MFMA, accumulated in float32 (csrc: the k_qah_* kernels).  Its
planes live in a scratch tensor of `scratch_bytes(...)` bytes that a call allocates and drops; the autograd node keeps qkv and lse
in either mode.  `precision.resolve("torch")` reads torch's setting at call time.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from . import precision as _prec
from ._args import buffers as _buffers, positive_int as _positive, tensor_rule
from ._call import call, ptr
from .precision import PRECISIONS  # noqa: F401  (the name callers of this module use)

ORDERS = {"legacy": _lib.QKV_LEGACY, "new": _lib.QKV_NEW}
HEAD_CHANNELS = (32,)
_tensor = tensor_rule(ValueError, "{what}: {name} must be a GPU tensor (there is no CPU path), got device {device}")


def supported_head_channels(ch: int) -> bool:
    return ch in HEAD_CHANNELS


def scratch_bytes(rows: int, views: int, heads: int, tokens: int, backward: bool) -> int:
    """s360_qkv_attention_high_scratch_bytes: the bytes of bf16 planes a "high" forward (backward) call needs."""
    return int(_lib.lib().s360_qkv_attention_high_scratch_bytes(int(rows), int(views), int(heads), HEAD_CHANNELS[0], int(tokens),
                                                                int(bool(backward))))


def _scratch(qkv: Tensor, views: int, heads: int, backward: bool) -> Tensor:
    return _prec.scratch(scratch_bytes(int(qkv.shape[0]), views, heads, int(qkv.shape[2]), backward), qkv.device)


def _checked(what: str, qkv, n_heads, n_frames, cross_view, order) -> tuple:
    """The shape checks of a call, then the tensor rule (the order they have always had); returns (rows, views, heads, ch, tokens, order code)."""
    if order not in ORDERS:
        raise ValueError(f"{what} knows the orders {sorted(ORDERS)}, got order={order!r}")
    if not isinstance(qkv, Tensor):
        raise ValueError(f"{what}: qkv must be a tensor, got {type(qkv).__name__}")
    if qkv.dim() != 3:
        raise ValueError(f"{what} expects qkv [N, heads * 3 * ch, T], got shape {tuple(qkv.shape)}")
    _positive(what, "n_heads", n_heads)
    _positive(what, "n_frames", n_frames)
    rows, width, tokens = (int(s) for s in qkv.shape)
    if qkv.numel() == 0:
        raise ValueError(f"{what}: qkv is empty, shape {tuple(qkv.shape)}")
    if width % (3 * n_heads) != 0:
        raise ValueError(f"{what}: qkv has {width} channel rows, not a multiple of 3 * n_heads = {3 * n_heads}")
    ch = width // (3 * n_heads)
    if not supported_head_channels(ch):
        raise ValueError(f"{what} takes qkv with ch = {HEAD_CHANNELS[0]} channels per head, got ch = {ch}")
    views = n_frames if cross_view else 1
    if rows % views != 0:
        raise ValueError(f"{what}: n_frames = {n_frames} must divide the {rows} rows of qkv for cross-view attention")
    _tensor(what, "qkv", qkv)
    return rows, views, n_heads, ch, tokens, ORDERS[order]


def attention_forward(qkv: Tensor, n_heads: int, *, n_frames: int = 1, cross_view: bool = False, order: str = "legacy",
                      precision: str = "highest", _dims=None) -> tuple:
    """s360_qkv_attention_forward (precision "high": s360_qkv_attention_high_forward) -> (out [N, heads ch, T] float32,
    lse [N / views, heads, views T] float64).  `_dims` is not for callers: the autograd node sets it (_checked's
    result) for a qkv that qkv_attention has checked and the node has made contiguous, and with it set nothing is checked here."""
    precision = _prec.check("qkv_attention", precision)
    rows, views, heads, ch, tokens, code = _dims or _checked("attention_forward", qkv, n_heads, n_frames, cross_view, order)
    if _dims is None:
        qkv = qkv.detach().contiguous()
    out = torch.empty(rows, heads * ch, tokens, dtype=torch.float32, device=qkv.device)
    lse = torch.empty(rows // views, heads, views * tokens, dtype=torch.float64, device=qkv.device)
    args = (ptr(qkv), rows, views, heads, ch, tokens, code, ptr(out), ptr(lse))
    if precision == "high":
        scratch = _scratch(qkv, views, heads, False)
        call("s360_qkv_attention_high_forward", qkv.device, *args, ptr(scratch), scratch.numel())
    else:
        call("s360_qkv_attention_forward", qkv.device, *args)
    return out, lse


def attention_backward(qkv: Tensor, lse: Tensor, g_out: Tensor, n_heads: int, *, n_frames: int = 1, cross_view: bool = False,
                       order: str = "legacy", g_qkv: Optional[Tensor] = None, precision: str = "highest", _dims=None) -> Tensor:
    """s360_qkv_attention_backward (precision "high": s360_qkv_attention_high_backward, with the lse of a "high" forward) -> g_qkv
    in qkv's shape and layout.  `g_qkv`: a contiguous float32 buffer of qkv's shape on its device to write into (every element is
    written); allocated when None.  `_dims`: not for callers, as in attention_forward."""
    precision = _prec.check("qkv_attention", precision)
    rows, views, heads, ch, tokens, code = _dims or _checked("attention_backward", qkv, n_heads, n_frames, cross_view, order)
    if _dims is None:
        _tensor("attention_backward", "g_out", g_out, (rows, heads * ch, tokens), device=qkv.device)
        _tensor("attention_backward", "lse", lse, (rows // views, heads, views * tokens), dtype=torch.float64, device=qkv.device)
        qkv, lse, g_out = (t.detach().contiguous() for t in (qkv, lse, g_out))
    if g_qkv is None:
        g_qkv = torch.empty_like(qkv)
    else:                                                     # the kernels move one dword per lane: a float's alignment, as for qkv
        _buffers("attention_backward", ("g_qkv",), (qkv.shape,), (torch.float32,), qkv.device, {"g_qkv": g_qkv}, _tensor, align=4)
        if g_qkv.data_ptr() == qkv.data_ptr():
            raise ValueError("attention_backward: g_qkv must be a buffer of its own, not qkv itself")
    delta = torch.empty_like(lse)
    args = (ptr(qkv), ptr(lse), ptr(g_out), rows, views, heads, ch, tokens, code, ptr(delta), ptr(g_qkv))
    if precision == "high":
        scratch = _scratch(qkv, views, heads, True)
        call("s360_qkv_attention_high_backward", qkv.device, *args, ptr(scratch), scratch.numel())
    else:
        call("s360_qkv_attention_backward", qkv.device, *args)
    return g_qkv


class _QKVAttention(torch.autograd.Function):
    """a of qkv; saves qkv and lse, nothing score-sized (the backward forms Delta from the recomputed probabilities, so not even
    the output is kept) and, in the "high" mode, none of the bf16 planes (the backward splits again)."""

    @staticmethod
    def forward(ctx, qkv, n_heads, n_frames, cross_view, order, precision, dims):
        qkv = qkv.detach().contiguous()
        opts = dict(n_frames=n_frames, cross_view=cross_view, order=order, precision=precision, _dims=dims)
        out, lse = attention_forward(qkv, n_heads, **opts)
        ctx.save_for_backward(qkv, lse)
        ctx.n_heads, ctx.opts = n_heads, opts
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        qkv, lse = ctx.saved_tensors
        return attention_backward(qkv, lse, g_out.to(torch.float32).contiguous(), ctx.n_heads, **ctx.opts), None, None, None, None, None, None


def qkv_attention(qkv: Tensor, n_heads: int, *, n_frames: int = 1, cross_view: bool = False, order: str = "legacy",
                  precision: str = "highest") -> Tensor:
    """The reference's QKVAttentionLegacy(n_heads, n_frames, use_cross_view_self_attn).forward (order "legacy", unet.py:527-565)
    or QKVAttention(n_heads).forward (order "new", :572-599) without its temporaries.

    qkv [N, heads 3 ch, T].  "legacy": head hd owns channel rows [hd 3 ch, (hd + 1) 3 ch), q then k then v; "new": q | k | v chunks of
    heads ch rows, head hd owns [hd ch, (hd + 1) ch) of each.  With cross_view the n_frames views of a batch element, which lie
    in rows u N / n_frames + bi (the reference's (v b) order), form one joint sequence of n_frames T tokens; without it n_frames
    is not used and every row attends within itself.  weight = softmax((q ch^-1/4) . (k ch^-1/4)) over the keys,
    a[c, t] = sum_s weight[t, s] v[c, s].  precision "highest": exact float32 products; "high": bf16x3 products on the bf16 MFMA,
    forward and backward (the module's docstring).  Returns a [N, heads ch, T] in qkv's row order.  Differentiable (once) in qkv.
    Float32 GPU tensors, ch = 32; no CPU path; a non-contiguous qkv is copied once."""
    _prec.check("qkv_attention", precision)
    dims = _checked("qkv_attention", qkv, n_heads, n_frames, cross_view, order)
    return _QKVAttention.apply(qkv, int(n_heads), int(n_frames), bool(cross_view), order, precision, dims)
