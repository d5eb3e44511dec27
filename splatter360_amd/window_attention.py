"""The multi-view transformer's single-head (shifted-)window attention on the GPU, forward and backward
(csrc/s360_window_attention.hip).

The reference's backbone (src/model/encoder/backbone/multiview_transformer.py:60-210, single_head_split_window_attention) rolls
the token grid, splits it into K x K windows, forms a dense [B K^2, Lw, Lk] score tensor, adds a dense shifted-window mask,
takes a softmax, multiplies by v, merges the windows and rolls back; autograd keeps the score-sized tensors of all twelve calls of
a backbone.  `window_attention` computes the same function with one fused kernel pair in which the rolls, the split and merge,
the mask and the softmax are index arithmetic: no score-sized tensor and no mask tensor exists, forward or backward, and the
autograd node saves q, k, v and one float64 log-sum-exp per query.  `full_attention` is single_head_full_attention (:8-16).
`ShiftMask` is what plugin.install(window_attention=True) lets generate_shift_window_attn_mask return in place of the
[K^2, Lw, Lw] tensor.  Float32 GPU tensors with 32 | C, 32 <= C <= 128; there is no CPU path (the installed seam keeps the
replaced functions for everything else).  Forward and backward are bit-identical from run to run: fixed order, no atomics.

precision="highest" (the default) forms every product from exact float32 products; precision="high" is what
torch.set_float32_matmul_precision('high') asks for: each float32 number as the sum of two bfloat16 numbers and each product
A B as Ah Bh + Ah Bl + Al Bh on the bf16 MFMA, accumulated in float32 (precision.py; csrc: the k_wah_* kernels).  Its planes live
in a scratch tensor of `scratch_bytes(...)` bytes that a call allocates and drops; the autograd node keeps q, k, v and lse in either
mode.  `resolve_precision("torch")` (precision.resolve) reads torch's setting at call time.
"""
from __future__ import annotations

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from . import _lib
from . import precision as _prec
from ._args import flat as _flat, tensor_rule
from ._call import call, ptr
from .precision import PRECISIONS, resolve as resolve_precision  # noqa: F401  (the names callers of this module use)

MASK_RULES = {"reference": 0, "aligned": 1}
MIN_CHANNELS, MAX_CHANNELS, CHANNEL_STEP = 32, 128, 32
_tensor = tensor_rule(RuntimeError, "{what} runs on the GPU only (no CPU path)")


def supported_channels(c: int) -> bool:
    return MIN_CHANNELS <= c <= MAX_CHANNELS and c % CHANNEL_STEP == 0


def _rule(mask_rule: str) -> int:
    if mask_rule not in MASK_RULES:
        raise ValueError(f"window_attention knows the mask rules {sorted(MASK_RULES)}, got mask_rule={mask_rule!r}")
    return MASK_RULES[mask_rule]


def scratch_bytes(batch: int, partners: int, height: int, width: int, channels: int, num_splits: int, backward: bool) -> int:
    """s360_window_attention_high_scratch_bytes: the bytes of bf16 planes a "high" forward (backward) call needs."""
    return int(_lib.lib().s360_window_attention_high_scratch_bytes(int(batch), int(partners), int(height), int(width), int(channels),
                                                                   int(num_splits), int(bool(backward))))


def _checked(what: str, q: Tensor, k: Tensor, v: Tensor, height: int, width: int, num_splits: int) -> int:
    """The shape checks of a call, then the tensor rule (so a CPU tensor of a wrong shape gets the shape's message); returns `partners`."""
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if q.dim() != 3:
        raise ValueError(f"{what} expects q [B, L, C], got shape {tuple(q.shape)}")
    if k.dim() not in (3, 4) or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"{what} expects k and v of one shape [B, L, C] or [B, m, L, C], got {tuple(k.shape)} and {tuple(v.shape)}")
    b, l, c = (int(s) for s in q.shape)
    if (int(k.shape[0]), int(k.shape[-2]), int(k.shape[-1])) != (b, l, c):
        raise ValueError(f"{what}: k {tuple(k.shape)} does not match q {tuple(q.shape)}")
    height, width, num_splits = int(height), int(width), int(num_splits)
    if height < 1 or width < 1 or height * width != l:
        raise ValueError(f"{what}: height * width = {height} * {width} is not the token count {l}")
    if num_splits < 1 or height % num_splits or width % num_splits:
        raise ValueError(f"{what}: num_splits = {num_splits} must divide height {height} and width {width}")
    if not supported_channels(c):
        raise ValueError(f"{what} takes {MIN_CHANNELS} <= C <= {MAX_CHANNELS} channels in multiples of {CHANNEL_STEP}, got {c}")
    partners = int(k.shape[1]) if k.dim() == 4 else 0
    if q.numel() == 0 or (k.dim() == 4 and partners < 1):
        raise ValueError(f"{what}: empty tensors")
    for name, t in (("q", q), ("k", k), ("v", v)):
        _tensor(what, name, t, device=q.device)
    return partners


def attention_forward(q: Tensor, k: Tensor, v: Tensor, *, height: int, width: int, num_splits: int, with_shift: bool = False,
                      mask_rule: str = "reference", precision: str = "highest", _partners=None) -> tuple:
    """s360_window_attention_forward (precision "high": s360_window_attention_high_forward) on contiguous float32 GPU tensors ->
    (out [B, L, C] float32, lse [B, L] float64).  `_partners` is not for callers: the autograd node sets it
    for tensors that window_attention has checked and the node has flattened, and with it set nothing is checked here."""
    rule, precision, partners = _rule(mask_rule), _prec.check("window_attention", precision), _partners
    if partners is None:
        partners = _checked("attention_forward", q, k, v, height, width, num_splits)
        q, k, v = (_flat(t) for t in (q, k, v))
    b, l, c = (int(s) for s in q.shape)
    out = torch.empty_like(q)
    lse = torch.empty(b, l, dtype=torch.float64, device=q.device)
    args = (ptr(q), ptr(k), ptr(v), b, partners, int(height), int(width), c, int(num_splits), int(bool(with_shift)), rule, ptr(out), ptr(lse))
    if precision == "high":
        scratch = _prec.scratch(scratch_bytes(b, partners, height, width, c, num_splits, False), q.device)
        call("s360_window_attention_high_forward", q.device, *args, ptr(scratch), scratch.numel())
    else:
        call("s360_window_attention_forward", q.device, *args)
    return out, lse


def attention_backward(q: Tensor, k: Tensor, v: Tensor, lse: Tensor, g_out: Tensor, *, height: int, width: int, num_splits: int,
                       with_shift: bool = False, mask_rule: str = "reference", needs=(True, True, True),
                       precision: str = "highest", _partners=None) -> tuple:
    """s360_window_attention_backward (precision "high": s360_window_attention_high_backward, with the lse of a "high" forward)
    -> (g_q, g_k, g_v) in the inputs' shapes, None where `needs` is False.  `_partners`: not for callers, as in attention_forward."""
    rule, precision, partners = _rule(mask_rule), _prec.check("window_attention", precision), _partners
    if partners is None:
        partners = _checked("attention_backward", q, k, v, height, width, num_splits)
        _tensor("attention_backward", "g_out", g_out, q.shape, device=q.device)
        _tensor("attention_backward", "lse", lse, q.shape[:2], dtype=torch.float64, device=q.device)
        q, k, v, lse, g_out = (_flat(t) for t in (q, k, v, lse, g_out))
    b, l, c = (int(s) for s in q.shape)
    g_q, g_k, g_v = (torch.empty_like(t) if need else None for t, need in zip((q, k, v), needs))
    if g_q is None and g_k is None and g_v is None:
        return None, None, None
    delta = torch.empty(b, l, dtype=torch.float64, device=q.device)
    args = (ptr(q), ptr(k), ptr(v), ptr(lse), ptr(g_out), b, partners, int(height), int(width), c, int(num_splits),
            int(bool(with_shift)), rule, ptr(delta), ptr(g_q), ptr(g_k), ptr(g_v))
    if precision == "high":
        scratch = _prec.scratch(scratch_bytes(b, partners, height, width, c, num_splits, True), q.device)
        call("s360_window_attention_high_backward", q.device, *args, ptr(scratch), scratch.numel())
    else:
        call("s360_window_attention_backward", q.device, *args)
    return g_q, g_k, g_v


class _WindowAttention(torch.autograd.Function):
    """out of (q, k, v); saves q, k, v and lse, nothing score-sized (the backward forms Delta from the recomputed probabilities,
    so not even out is kept) and, in the "high" mode, none of the bf16 planes (the backward splits again)."""

    @staticmethod
    def forward(ctx, q, k, v, opts):
        q, k, v = (_flat(t) for t in (q, k, v))
        out, lse = attention_forward(q, k, v, **opts)
        ctx.save_for_backward(q, k, v, lse)
        ctx.opts = opts
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        q, k, v, lse = ctx.saved_tensors
        grads = attention_backward(q, k, v, lse, _flat(g_out.to(torch.float32)), needs=tuple(ctx.needs_input_grad[:3]), **ctx.opts)
        return (*grads, None)


def window_attention(q: Tensor, k: Tensor, v: Tensor, *, height: int, width: int, num_splits: int, with_shift: bool = False,
                     mask_rule: str = "reference", precision: str = "highest") -> Tensor:
    """The reference's single_head_split_window_attention (multiview_transformer.py:60-210) without its temporaries.

    q [B, L, C] with L = height * width tokens in (y, x) order; k, v [B, L, C] (the same-shape branch) or [B, m, L, C] (the
    multi-view branch: the window's keys are ordered (token, view), view fastest).  Windows are (height / num_splits) x
    (width / num_splits); with_shift rolls the grid by half a window first and masks pairs from different regions with the
    reference's FINITE -100.0.  mask_rule "reference" reproduces the reference's `attn_mask.repeat(b, 1, m)`, which gives key
    column j the region of window token j mod Lw; "aligned" gives it the region of its own token j // m.  The two coincide at
    m <= 1 and without shift.  precision "highest": exact float32 products; "high": bf16x3 products on the bf16 MFMA, forward
    and backward (the module's docstring).  Returns out [B, L, C] in the original token order.  Differentiable (once) in q, k
    and v.  Float32 GPU tensors, C a multiple of 32 in [32, 128]; no CPU path; non-contiguous or misaligned inputs are copied once."""
    _prec.check("window_attention", precision)
    _rule(mask_rule)
    partners = _checked("window_attention", q, k, v, height, width, num_splits)
    return _WindowAttention.apply(q, k, v, dict(height=int(height), width=int(width), num_splits=int(num_splits), with_shift=bool(with_shift),
                                                mask_rule=mask_rule, precision=precision, _partners=partners))


def full_attention(q: Tensor, k: Tensor, v: Tensor, precision: str = "highest") -> Tensor:
    """The reference's single_head_full_attention (multiview_transformer.py:8-16) for Lq == Lk: softmax(q k^T / sqrt(C)) v over all
    tokens of a batch element, as one window without shift."""
    _prec.check("window_attention", precision)
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, Tensor) or t.dim() != 3:
            raise ValueError(f"full_attention expects {name} [B, L, C]")
    if tuple(k.shape) != tuple(q.shape):
        raise ValueError(f"full_attention needs Lq == Lk: q {tuple(q.shape)}, k {tuple(k.shape)}")
    return window_attention(q, k, v, height=1, width=int(q.shape[1]), num_splits=1, precision=precision)


class ShiftMask:
    """The shifted-window mask as a handle: (h, w, wh, ww, sh, sw, device) and nothing of size Lw^2.  `dense()` builds the
    reference's [K^2, Lw, Lw] float32 tensor of generate_shift_window_attn_mask (multiview_transformer.py:19-57) on demand, once (with `build`,
    by calling it)."""

    def __init__(self, h: int, w: int, wh: int, ww: int, sh: int, sw: int, device=None, build=None):
        self.h, self.w, self.wh, self.ww, self.sh, self.sw = (int(x) for x in (h, w, wh, ww, sh, sw))
        self.device = torch.device("cpu") if device is None else torch.device(device)
        self.build = build                                      # () -> the dense tensor (the seam: the replaced generator)
        self._dense = None

    @property
    def num_splits(self) -> int:
        return self.w // self.ww

    def regions(self) -> Tensor:
        """[h, w] int64: the region of every ROLLED position (the reference's slices, negative bounds as Python's)."""
        def axis(n, win, s):
            r = torch.zeros(n, dtype=torch.int64, device=self.device)
            for idx, sl in enumerate((slice(0, -win), slice(-win, -s), slice(-s, None))):
                r[sl] = idx
            return r
        return 3 * axis(self.h, self.wh, self.sh)[:, None] + axis(self.w, self.ww, self.sw)[None, :]

    def dense(self) -> Tensor:
        if self._dense is None and self.build is not None:
            self._dense = self.build()
        if self._dense is None:
            k = self.num_splits
            reg = self.regions().view(k, self.h // k, k, self.w // k).permute(0, 2, 1, 3).reshape(k * k, -1)
            diff = reg.unsqueeze(1) != reg.unsqueeze(2)
            self._dense = torch.where(diff, torch.tensor(-100.0, device=self.device), torch.tensor(0.0, device=self.device))
        return self._dense

    def matches(self, h: int, w: int, num_splits: int) -> bool:
        return (self.h, self.w) == (h, w) and self.h // self.wh == num_splits and self.w // self.ww == num_splits \
            and (self.sh, self.sw) == (self.wh // 2, self.ww // 2)

    def __repr__(self):
        return f"ShiftMask(h={self.h}, w={self.w}, wh={self.wh}, ww={self.ww}, sh={self.sh}, sw={self.sw}, device={self.device})"
