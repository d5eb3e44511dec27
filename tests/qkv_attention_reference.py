"""The yardstick of the fused multi-head QKV attention (splatter360_amd.qkv_attention): the project's own statement of

    qkv [N, heads 3 ch, T];  B = N / views;  joint token s < L = views T of batch element bi is token s mod T of view s // T and
    lives in row (s // T) B + bi  (views = 1 without cross-view: L = T, row = bi)
    order "legacy": head hd owns channel rows [hd 3 ch, (hd + 1) 3 ch), q then k then v
    order "new":    the channel axis is q | k | v chunks of heads ch rows, head hd owns [hd ch, (hd + 1) ch) of each
    weight[t, s] = softmax_s((q ch^-1/4)[:, t] . (k ch^-1/4)[:, s]),   a[c, t] = sum_s weight[t, s] v[c, s]
    a [N, heads ch, T] in the rows' (v b) order

in any dtype (`statement`), the same lines in float32 in the order of operations a stock torch implementation uses
(`reference_lines`, the yardstick of the accuracy rule), deterministic inputs, gradients, and stand-ins for the reference's two
attention classes that the installed seam rebinds.  The statement is held to the reference's recorded outputs
(tests/golden/qkv_attention.npz) by tests/test_qkv_attention_spec.py.  Nothing here needs a GPU.
"""
import math

import numpy as np
import torch
from torch import nn

import group_norm_reference as G

ORDERS = ("legacy", "new")


def split_heads(qkv, heads, views, cross_view, order):
    """(q, k, v), each [B, heads, ch, L]: the joint sequences of every batch element and head."""
    n, width, t = qkv.shape
    nv = views if cross_view else 1
    assert order in ORDERS and width % (3 * heads) == 0 and n % nv == 0
    b, ch = n // nv, width // (3 * heads)
    x = qkv.reshape(nv, b, width, t)                                   # row u B + bi -> [u, bi]
    if order == "legacy":
        x = x.reshape(nv, b, heads, 3, ch, t).permute(3, 1, 2, 4, 0, 5)                 # [3, B, heads, ch, views, T]
    else:
        x = x.reshape(nv, b, 3, heads, ch, t).permute(2, 1, 3, 4, 0, 5)
    x = x.reshape(3, b, heads, ch, nv * t)
    return x[0], x[1], x[2]


def merge_heads(a, views, cross_view):
    """[B, heads, ch, L] -> [N, heads ch, T] in the (v b) row order."""
    b, heads, ch, length = a.shape
    nv = views if cross_view else 1
    t = length // nv
    return a.reshape(b, heads * ch, nv, t).permute(2, 0, 1, 3).reshape(nv * b, heads * ch, t)


def joint(a, heads, views, cross_view):
    """[N, heads ch, T] in the (v b) row order -> [B, heads, ch, L]: merge_heads' inverse."""
    n, width, t = a.shape
    nv = views if cross_view else 1
    return a.reshape(nv, n // nv, heads, width // heads, t).permute(1, 2, 3, 0, 4).reshape(n // nv, heads, width // heads, nv * t)


def statement(qkv, heads, views=1, cross_view=False, order="legacy", dtype=torch.float64):
    """The function in `dtype` (float64: the statement the kernels are held to), pure torch, differentiable."""
    q, k, v = (x.to(dtype) for x in split_heads(qkv, heads, views, cross_view, order))
    scale = q.shape[2] ** -0.25
    weight = torch.softmax(torch.einsum("bhct,bhcs->bhts", q * scale, k * scale), dim=-1)
    return merge_heads(torch.einsum("bhts,bhcs->bhct", weight, v), views, cross_view)


def reference_lines(qkv, heads, views=1, cross_view=False, order="legacy"):
    """The same lines in float32 as a stock torch implementation runs them: heads folded into the batch, q and k scaled by
    ch^-1/4 each, one batched product for the weights, softmax in float32, one batched product with v.  Forms the
    [B heads, L, L] weight tensor; on the device of qkv."""
    q, k, v = split_heads(qkv.float(), heads, views, cross_view, order)
    b, _, ch, length = q.shape
    q, k, v = (x.reshape(b * heads, ch, length) for x in (q, k, v))
    scale = 1 / math.sqrt(math.sqrt(ch))
    weight = torch.einsum("bct,bcs->bts", q * scale, k * scale)
    weight = torch.softmax(weight.float(), dim=-1).type(weight.dtype)
    a = torch.einsum("bts,bcs->bct", weight, v)
    return merge_heads(a.reshape(b, heads, ch, length), views, cross_view)


def random_case(n, heads, t, ch=32, scale=1.0, seed=0, device="cpu"):
    """(qkv [n, heads 3 ch, t], g [n, heads ch, t]) float32, deterministic: standard normal times `scale`, g standard normal."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, heads * 3 * ch, t, generator=gen) * scale
    g = torch.randn(n, heads * ch, t, generator=gen)
    return qkv.to(device), g.to(device)


def gradients(fn, qkv, g, dtype=None):
    """(out, g_qkv) of fn(qkv) with the output gradient g, both detached; in `dtype` if given (inputs cast first)."""
    x = qkv.detach().clone()
    if dtype is not None:
        x, g = x.to(dtype), g.to(dtype)
    x.requires_grad_(True)
    out = fn(x)
    out.backward(g.to(out.dtype))
    return out.detach(), x.grad


def parts(g_qkv, heads, order):
    """(g_q, g_k, g_v) [N, heads, ch, T]: the q, k and v rows of a tensor in qkv's layout."""
    n, width, t = g_qkv.shape
    ch = width // (3 * heads)
    x = g_qkv.reshape(n, heads, 3, ch, t).transpose(1, 2) if order == "legacy" else g_qkv.reshape(n, 3, heads, ch, t)
    return x[:, 0], x[:, 1], x[:, 2]


# ---- stand-ins for the reference's classes (written for this project; attribute names are those the wrappers read) --------------

class StandinQKVAttentionLegacy(nn.Module):
    """Heads split before q, k, v; with use_cross_view_self_attn the n_frames views of the (v b) batch form one sequence."""

    def __init__(self, n_heads, n_frames=2, use_cross_view_self_attn=False):
        super().__init__()
        self.n_heads, self.n_frames, self.use_cross_view_self_attn = n_heads, n_frames, use_cross_view_self_attn
        self.calls = 0

    def forward(self, qkv):
        self.calls += 1
        assert qkv.shape[1] % (3 * self.n_heads) == 0
        a = reference_lines(qkv, self.n_heads, self.n_frames, self.use_cross_view_self_attn, "legacy")
        return a.type(qkv.dtype)


class StandinQKVAttention(nn.Module):
    """q, k, v split before the heads; no cross-view form."""

    def __init__(self, n_heads):
        super().__init__()
        self.n_heads = n_heads
        self.calls = 0

    def forward(self, qkv):
        self.calls += 1
        assert qkv.shape[1] % (3 * self.n_heads) == 0
        return reference_lines(qkv, self.n_heads, 1, False, "new").type(qkv.dtype)


def standin_modules(unet_name, predictor_name, backbone_name):
    """group_norm_reference.standin_modules plus the two attention classes in the unet module, whose AttentionBlock builds its
    `attention` from the module's own QKVAttentionLegacy (QKVAttention with use_new_attention_order), as the reference's does."""
    mods = G.standin_modules(unet_name, predictor_name, backbone_name)
    unet = mods[unet_name]
    for name, base in (("QKVAttentionLegacy", StandinQKVAttentionLegacy), ("QKVAttention", StandinQKVAttention)):
        setattr(unet, name, type(name, (base,), {"__module__": unet.__name__}))       # a fresh class per module: patches do not leak

    def init(self, channels, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True, use_new_attention_order=False):
        G.StandinAttentionBlock.__init__(self, channels, num_head_channels, postnorm, num_frames, use_cross_view_self_attn)
        self.attention = unet.QKVAttention(self.num_heads) if use_new_attention_order else \
            unet.QKVAttentionLegacy(self.num_heads, n_frames=num_frames, use_cross_view_self_attn=use_cross_view_self_attn)

    unet.AttentionBlock = type("AttentionBlock", (unet.AttentionBlock,), {"__module__": unet.__name__, "__init__": init})
    return mods
