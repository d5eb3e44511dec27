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
(tests/golden/qkv_attention.npz) by tests/test_qkv_attention_spec.py.  Further the per-row measure of
tests/test_gpu_qkv_attention_float64.py: `row_scales` (the exact quantities per (batch element, head, joint token) in float64 and
the scale each is summed from: the window attention's formulas, not written a second time), `lines_rows` (the float32 lines' six
quantities), the cases and the maps between the tensors' layouts and the per-row indexing.  Nothing here needs a GPU.
"""
import math

import numpy as np
import torch
from torch import nn

import group_norm_reference as G
import window_attention_reference as W

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


def reference_lines(qkv, heads, views=1, cross_view=False, order="legacy", parts=None):
    """The same lines in float32 as a stock torch implementation runs them: heads folded into the batch, q and k scaled by
    ch^-1/4 each, one batched product for the weights, softmax in float32, one batched product with v.  Forms the
    [B heads, L, L] weight tensor; on the device of qkv.  A dict given as `parts` receives the intermediates, detached:
    "scores" and "probabilities" [B heads, L, L] (queries, keys) and "values" [B heads, ch, L]."""
    q, k, v = split_heads(qkv.float(), heads, views, cross_view, order)
    b, _, ch, length = q.shape
    q, k, v = (x.reshape(b * heads, ch, length) for x in (q, k, v))
    scale = 1 / math.sqrt(math.sqrt(ch))
    weight = torch.einsum("bct,bcs->bts", q * scale, k * scale)
    scores = weight
    weight = torch.softmax(weight.float(), dim=-1).type(weight.dtype)
    if parts is not None:
        parts.update(scores=scores.detach(), probabilities=weight.detach(), values=v.detach())
    a = torch.einsum("bts,bcs->bct", weight, v)
    return merge_heads(a.reshape(b, heads, ch, length), views, cross_view)


def random_case(n, heads, t, ch=32, scale=1.0, seed=0, device="cpu", head_scales=None, row_gains=None, order="legacy"):
    """(qkv [n, heads 3 ch, t], g [n, heads ch, t]) float32, deterministic: standard normal times `scale`, g standard normal.
    head_scales: one further factor per head on its q and k rows (where they lie in `order`); row_gains: one factor per batch
    row on g.  Without them the tensors are those of the plain call, bit for bit."""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, heads * 3 * ch, t, generator=gen) * scale
    g = torch.randn(n, heads * ch, t, generator=gen)
    if head_scales is not None:
        assert len(head_scales) == heads
        f = torch.tensor(head_scales, dtype=torch.float32).view(1, heads, 1, 1)
        for x in parts(qkv, heads, order)[:2]:                                      # views into qkv
            x *= f
    if row_gains is not None:
        assert len(row_gains) == n
        g = g * torch.tensor(row_gains, dtype=torch.float32).view(n, 1, 1)
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


# ---- the per-row measure (tests/test_gpu_qkv_attention_float64.py, pinned by tests/test_qkv_attention_rows.py) ------------------
# Rows are indexed per (batch element, head, joint token): a quantity with channels is [B, heads, L, ch], one without [B, heads, L]
# (the layout of the kernels' lse and delta).  The formulas are window_attention_reference.row_scales' for one unmasked window
# of L tokens, called on [B heads, L, ch] tensors.
ROW_NAMES, UNIT, SCALE_FLOOR = W.ROW_NAMES, W.UNIT, W.SCALE_FLOOR
row_units, worst_rows = W.row_units, W.worst_rows

# name: (N, views, cross_view, heads, T, order); ch = 32.  The nine shapes of tests/test_gpu_qkv_attention.py and the smallest
# shapes that reach what they leave out.
ROW_CASES = {
    "tile": (2, 1, False, 1, 32, "legacy"),           # exactly one tile
    "ragged": (2, 1, False, 2, 35, "legacy"),         # one token past a tile; rows not 16-byte aligned
    "tiny": (1, 1, False, 1, 5, "legacy"),            # less than a tile
    "straddle": (4, 2, True, 4, 48, "legacy"),        # L = 96, B = 2; the second tile spans two views; four interleaved heads
    "views3": (3, 3, True, 1, 20, "legacy"),          # L = 60
    "frames_unused": (4, 2, False, 2, 40, "legacy"),  # n_frames = 2 with cross-view off: the rows stay separate
    "new_order": (2, 2, True, 2, 40, "new"),          # the q | k | v chunk order
    "long": (2, 2, True, 1, 320, "legacy"),           # L = 640: twenty key tiles, the running maximum moves
    "uneven": (2, 2, True, 1, 100, "legacy"),         # L = 200: seven tiles for four waves (2, 2, 2, 1), the last one ragged
    "edge": (2, 2, True, 1, 65, "legacy"),            # L = 130: five tiles for four waves (2, 1, 1, 1); the last owner tile and the
                                                      # last key tile have two valid rows; T odd
    "thin4": (4, 4, True, 2, 5, "legacy"),            # L = 20: one tile spans four views; three of four waves walk nothing
    "one": (2, 2, True, 1, 1, "legacy"),              # T = 1, L = 2
    "mixed": (4, 2, True, 4, 48, "legacy"),           # heads and batch rows of very different magnitude in one tensor (ROW_EXTRAS)
    "new_mixed": (2, 1, False, 4, 35, "new"),         # the new order with four heads of different magnitude and unaligned rows
}
MIXED_HEADS = (6.0, 2.2, 0.8, 0.3)
ROW_EXTRAS = {"mixed": dict(head_scales=MIXED_HEADS, row_gains=(1.0, 1e-1, 1e-2, 1e-3)), "new_mixed": dict(head_scales=MIXED_HEADS)}
# (name, input scale): every case at 1, 3 and 6; the two mixed cases once, their heads carry the scales
ROW_RUNS = [(name, scale) for name in ROW_CASES if name not in ROW_EXTRAS for scale in (1.0, 3.0, 6.0)] + [(name, 1.0) for name in ROW_EXTRAS]


def row_inputs(name, scale=1.0, device="cpu"):
    """(qkv, g) of a run of ROW_RUNS: the one set of inputs the CPU and the GPU tests of the per-row rule share."""
    n, views, cross, heads, t, order = ROW_CASES[name]
    seed = 4000 + 7 * sorted(ROW_CASES).index(name)
    return random_case(n, heads, t, scale=scale, seed=seed, device=device, order=order, **ROW_EXTRAS.get(name, {}))


def out_rows(a, heads, views, cross_view):
    """A tensor in out's layout [N, heads ch, T] -> [B, heads, L, ch]."""
    return joint(a, heads, views, cross_view).transpose(2, 3)


def out_from_rows(x, views, cross_view):
    """[B, heads, L, ch] -> out's layout [N, heads ch, T]: out_rows' inverse."""
    return merge_heads(x.transpose(2, 3), views, cross_view)


def qkv_rows(g_qkv, heads, views, cross_view, order):
    """A tensor in qkv's layout [N, heads 3 ch, T] -> (q, k, v) rows, each [B, heads, L, ch]."""
    return tuple(x.transpose(2, 3) for x in split_heads(g_qkv, heads, views, cross_view, order))


def qkv_from_rows(q, k, v, views, cross_view, order):
    """(q, k, v) rows [B, heads, L, ch] -> qkv's layout [N, heads 3 ch, T]: qkv_rows' inverse."""
    b, heads, length, ch = q.shape
    nv = views if cross_view else 1
    x = torch.stack([t.transpose(2, 3).reshape(b, heads, ch, nv, length // nv) for t in (q, k, v)])     # [3, B, heads, ch, views, T]
    x = x.permute(4, 1, 2, 0, 3, 5) if order == "legacy" else x.permute(4, 1, 0, 2, 3, 5)
    return x.reshape(nv * b, heads * 3 * ch, length // nv)


def vector_to_out(x, views, cross_view):
    """One number per row [B, heads, L] -> [N, heads, T], the rows and tokens of out's layout (a mask over out's elements is
    this, repeated over each head's ch channel rows)."""
    return merge_heads(x.unsqueeze(2), views, cross_view)


def vector_from_out(x, views, cross_view):
    """[N, heads, T] -> [B, heads, L]: vector_to_out's inverse."""
    return joint(x, x.shape[1], views, cross_view).squeeze(2)


def _folded(x):
    """[B, heads, L, ch] -> [B heads, L, ch] (contiguous)."""
    return x.reshape(-1, *x.shape[2:])


def row_scales(qkv, g, heads, views=1, cross_view=False, order="legacy"):
    """(want, scale): two dicts over ROW_NAMES, float64 on the inputs' device.  want: out, g_q, g_k, g_v [B, heads, L, ch], lse and
    delta [B, heads, L]; scale: one number per row, [B, heads, L].  window_attention_reference.row_scales (its docstring has the
    formulas) for one unmasked window of the L joint tokens, every (batch element, head) a batch entry: its scores are
    q . k / sqrt(ch), the statement's (q ch^-1/4) . (k ch^-1/4)."""
    q, k, v = (_folded(x.detach().double()) for x in qkv_rows(qkv, heads, views, cross_view, order))
    gr = out_rows(g.detach().double(), heads, views, cross_view)
    b, _, length, ch = gr.shape
    want, scale = W.row_scales(q, k, v, _folded(gr), 1, False, 1, length)
    unfold = lambda x: x.reshape(b, heads, *x.shape[1:])
    return {n: unfold(x) for n, x in want.items()}, {n: unfold(x) for n, x in scale.items()}


def lines_rows(qkv, g, heads, views=1, cross_view=False, order="legacy"):
    """The float32 yardstick of all six quantities in the per-row indexing, a dict over ROW_NAMES: out and the gradients of
    reference_lines by autograd, lse = torch.logsumexp of its own float32 scores and delta = (P * dP).sum(-1) of its own
    probabilities, with dP = g^T v formed from the same tensors."""
    got = {}
    out, g_qkv = gradients(lambda x: reference_lines(x, heads, views, cross_view, order, parts=got), qkv, g)
    scores, prob, v = got["scores"], got["probabilities"], got["values"]
    gr = joint(g.to(prob.dtype), heads, views, cross_view)                          # [B, heads, ch, L]
    b, _, ch, length = gr.shape
    dp = torch.einsum("bct,bcs->bts", gr.reshape(b * heads, ch, length), v)
    rows = (out_rows(out, heads, views, cross_view), *qkv_rows(g_qkv, heads, views, cross_view, order),
            torch.logsumexp(scores, dim=-1).reshape(b, heads, length), (prob * dp).sum(-1).reshape(b, heads, length))
    return dict(zip(ROW_NAMES, rows))


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
