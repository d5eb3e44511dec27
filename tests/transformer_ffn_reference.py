"""The yardstick of the fused transformer FFN tail (splatter360_amd.transformer_ffn): the project's own statement of what the
reference's TransformerLayer.forward (src/model/encoder/backbone/multiview_transformer.py:334-414) computes behind its attention,

    X = cat([source, LN1(m)], -1);  h = gelu(X W1^T);  z = h W2^T;  out = source + LN2(z)        (no_ffn: out = source + LN1(m))
    LN(x) = (x - mean) / sqrt(var + eps) weight + bias over the last axis, var the BIASED variance; gelu the erf form

generic in C, in any dtype (`statement`, `norm_statement`; float64 is what the kernels are held to), the whole layer with full
attention (`layer_statement`), the same lines in float32 as stock torch runs them (`reference_lines`, `norm_lines`: the yardstick
of the accuracy rule), deterministic inputs, gradients, and a stand-in for the reference's backbone module with a TransformerLayer
written for this project that the installed seam rebinds.  The statement is held to the reference's recorded outputs
(tests/golden/transformer_ffn.npz) by tests/test_transformer_ffn_spec.py.  Nothing here needs a GPU.
"""
import math
import sys

import torch
import torch.nn.functional as F
from torch import nn

import window_attention_reference as W

TAIL_NAMES = ("source", "m", "norm1_weight", "norm1_bias", "w1", "w2", "norm2_weight", "norm2_bias")
NORM_NAMES = ("x", "weight", "bias", "residual")
LAYER_PARAMS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "norm1.weight", "norm1.bias", "mlp.0.weight",
                "mlp.2.weight", "norm2.weight", "norm2.bias")


def layer_norm(x, weight, bias, eps, unbiased=False):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).sum(dim=-1, keepdim=True) / (x.shape[-1] - (1 if unbiased else 0))
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def statement(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps=1e-5, dtype=torch.float64, wrong=None):
    """The tail in `dtype`, pure torch, differentiable, generic in C.  wrong: one of the rules the spec test shows to matter —
    "cat_order", "tanh_gelu", "unbiased_variance", "residual_before_norm2"."""
    source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias = (
        t.to(dtype) for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias))
    unbiased = wrong == "unbiased_variance"
    y = layer_norm(m, norm1_weight, norm1_bias, eps, unbiased)
    x = torch.cat([y, source] if wrong == "cat_order" else [source, y], dim=-1)
    z = gelu(x @ w1.transpose(0, 1), tanh=wrong == "tanh_gelu") @ w2.transpose(0, 1)
    if wrong == "residual_before_norm2":
        return layer_norm(source + z, norm2_weight, norm2_bias, eps, unbiased)
    return source + layer_norm(z, norm2_weight, norm2_bias, eps, unbiased)


def norm_statement(x, weight, bias, residual, eps=1e-5, dtype=torch.float64):
    x, weight, bias, residual = (t.to(dtype) for t in (x, weight, bias, residual))
    return residual + layer_norm(x, weight, bias, eps)


def reference_lines(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps=1e-5):
    """The reference's lines in float32 on the tensors' device: F.layer_norm, the concatenation, two F.linear around F.gelu,
    F.layer_norm, the add.  Forms the [T, 2C] and both [T, 8C] tensors."""
    c = source.shape[-1]
    message = F.layer_norm(m, (c,), norm1_weight, norm1_bias, eps)
    message = F.linear(F.gelu(F.linear(torch.cat([source, message], dim=-1), w1)), w2)
    return source + F.layer_norm(message, (c,), norm2_weight, norm2_bias, eps)


def norm_lines(x, weight, bias, residual, eps=1e-5):
    return residual + F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def gradients(fn, tensors, g, dtype=None):
    """(out, gradient of every tensor) of fn(*tensors) with the output gradient g, all detached; in `dtype` if given."""
    xs = [t.detach().clone().to(dtype or t.dtype).requires_grad_(True) for t in tensors]
    out = fn(*xs)
    out.backward(g.to(out.dtype))
    return (out.detach(), *(x.grad for x in xs))


def random_case(tokens, scale=1.0, seed=0, device="cpu", c=128, lead=None):
    """(the eight tensors of TAIL_NAMES, g), float32, deterministic: source and m standard normal times `scale` (m with an offset
    of its own per token, so that norm1 has a mean to take out), the Linear weights normal with nn.Linear's 1 / sqrt(fan-in)
    deviation, norm weights around 1, g standard normal.  lead: the leading dimensions (their product is `tokens`)."""
    gen = torch.Generator().manual_seed(seed)
    shape = (*(lead or (tokens,)), c)
    assert math.prod(shape[:-1]) == tokens
    source = torch.randn(shape, generator=gen) * scale
    m = (torch.randn(shape, generator=gen) + 0.5 * torch.randn(*shape[:-1], 1, generator=gen)) * scale
    n1w, n2w = (1 + 0.2 * torch.randn(c, generator=gen) for _ in range(2))
    n1b, n2b = (0.2 * torch.randn(c, generator=gen) for _ in range(2))
    w1 = torch.randn(8 * c, 2 * c, generator=gen) / math.sqrt(2 * c)
    w2 = torch.randn(c, 8 * c, generator=gen) / math.sqrt(8 * c)
    g = torch.randn(shape, generator=gen)
    return tuple(t.to(device) for t in (source, m, n1w, n1b, w1, w2, n2w, n2b)), g.to(device)


def norm_case(case):
    """The no_ffn tail's tensors (NORM_NAMES) from a case of random_case: x = m, residual = source."""
    (source, m, n1w, n1b, *_), g = case
    return (m, n1w, n1b, source), g


def layer_statement(params, source, target, no_ffn=False, eps=1e-5, dtype=torch.float64):
    """The whole single-head TransformerLayer with full attention in `dtype` from a {state_dict key: tensor} dict of its
    parameters: projections, softmax(q k^T / sqrt(C)) v, merge, then the tail."""
    p = {k: v.to(dtype) for k, v in params.items()}
    source, target = source.to(dtype), target.to(dtype)
    q, k, v = source @ p["q_proj.weight"].T, target @ p["k_proj.weight"].T, target @ p["v_proj.weight"].T
    m = W.full_lines(q, k, v) @ p["merge.weight"].T
    if no_ffn:
        return norm_statement(m, p["norm1.weight"], p["norm1.bias"], source, eps, dtype)
    return statement(source, m, p["norm1.weight"], p["norm1.bias"], p["mlp.0.weight"], p["mlp.2.weight"], p["norm2.weight"],
                     p["norm2.bias"], eps, dtype)


def layer_params(no_ffn):
    return tuple(k for k in LAYER_PARAMS if not (no_ffn and (k.startswith("mlp") or k.startswith("norm2"))))


# ---- a stand-in for the reference's backbone module (written for this project; attribute names are those the wrapper reads) -----

class StandinTransformerLayer(nn.Module):
    """The reference's TransformerLayer as the seam sees it: the same attributes and submodule names (so the same state_dict
    keys), a forward with its signature that looks the attention functions up in its module's globals at call time, and a
    counter of its calls."""

    def __init__(self, d_model=128, nhead=1, attention_type="swin", no_ffn=False, ffn_dim_expansion=4, with_shift=False,
                 add_per_view_attn=False, **kwargs):
        super().__init__()
        self.dim, self.nhead, self.attention_type, self.no_ffn = d_model, nhead, attention_type, no_ffn
        self.add_per_view_attn, self.with_shift = add_per_view_attn, with_shift
        self.q_proj, self.k_proj, self.v_proj, self.merge = (nn.Linear(d_model, d_model, bias=False) for _ in range(4))
        self.norm1 = nn.LayerNorm(d_model)
        if not no_ffn:
            self.mlp = nn.Sequential(nn.Linear(2 * d_model, 2 * d_model * ffn_dim_expansion, bias=False), nn.GELU(),
                                     nn.Linear(2 * d_model * ffn_dim_expansion, d_model, bias=False))
            self.norm2 = nn.LayerNorm(d_model)
        self.calls = 0

    def forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, attn_num_splits=None, **kwargs):
        self.calls += 1
        g = sys.modules[type(self).__module__].__dict__
        attn_type = kwargs.get("attn_type", self.attention_type)
        query, key, value = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        if attn_type == "swin" and attn_num_splits > 1:
            opts = dict(num_splits=attn_num_splits, with_shift=self.with_shift, h=height, w=width, attn_mask=shifted_window_attn_mask)
            if self.nhead > 1:
                message = g["multi_head_split_window_attention"](query, key, value, num_head=self.nhead, **opts)
            elif self.add_per_view_attn:
                b, l, c = query.shape
                views = key.shape[1]
                message = g["single_head_split_window_attention"](query.unsqueeze(1).expand(b, views, l, c).reshape(-1, l, c),
                                                                  key.reshape(-1, l, c), value.reshape(-1, l, c), **opts)
                message = message.view(b, views, l, c).sum(1)
            else:
                message = g["single_head_split_window_attention"](query, key, value, **opts)
        else:
            message = g["single_head_full_attention"](query, key, value)
        message = self.norm1(self.merge(message))
        if not self.no_ffn:
            message = self.norm2(self.mlp(torch.cat([source, message], dim=-1)))
        return source + message


def standin_module(name):
    """window_attention_reference.standin_module (the attention functions install(window_attention=True) rebinds) plus a
    TransformerLayer class of the module's own: a fresh class per module, so patches do not leak."""
    mod = W.standin_module(name)
    mod.TransformerLayer = type("TransformerLayer", (StandinTransformerLayer,), {"__module__": name})
    return mod


def randomise(layer, seed, scale=1.0):
    """Every parameter of a layer from a seeded generator: Linear weights with deviation scale / sqrt(fan-in), norm weights
    around 1, norm biases around 0."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key, p in layer.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=gen) * scale / math.sqrt(p.shape[1]))
            elif key.endswith("weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))
    return layer
