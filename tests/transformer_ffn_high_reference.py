"""The yardstick of the FFN tail's "high" precision mode (splatter360_amd/transformer_ffn.py, precision="high"): the statement of
tests/transformer_ffn_reference.py with its two products — and, through window_attention_high_reference.HighProduct, the four
products of their backward — as bf16x3 products of split operands, everything else in float64.  What the kernels and this file
share is the specification:

  split(x)   hi = bf16(x), round to nearest even; lo = bf16(x - float32(hi))        (window_attention_high_reference.split)
  product    A B = Ah Bh + Ah Bl + Al Bh (terms=3); Al Bl is dropped.  terms=1 keeps Ah Bh alone: what a kernel that lost its lo
             planes would compute.  Both operands are split from their float32 values: X = [source, float32(LN1(m))] and W1, h =
             float32(gelu(pre)) and W2, and in the backward dz, dpre, X and h again.

Further the whole single-head layer with full attention in the same arithmetic (`layer_split_statement`), and the token counts at
which the "high" kernels' launch geometry takes each of its paths, derived from the kernel file's constants (`geometry_cases`).
Nothing here needs a GPU.
"""
import re

import torch

import test_transformer_ffn_rows as ROWS
import transformer_ffn_reference as R
import window_attention_high_reference as H

KERNEL_FILE = ROWS.CSRC / "s360_transformer_ffn.hip"
OUT_NAMES = ("out", *("g_" + n for n in R.TAIL_NAMES))
EXACT = ("g_norm2_bias",)                                          # holds no product: the sum of g_out over the tokens


def split_statement(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps=1e-5, terms=3):
    """R.statement with high products: float32 tensors (any leading dimensions) -> out in source's shape, float64; differentiable
    (dh = dz W2, dX = dpre W1, g_w1 = dpre^T X and g_w2 = dz^T h are high products of their own split operands)."""
    source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias = (
        t.double() for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias))
    shape, c = source.shape, source.shape[-1]
    s2, m2 = source.reshape(-1, c), m.reshape(-1, c)
    x = torch.cat([s2, R.layer_norm(m2, norm1_weight, norm1_bias, eps)], dim=-1)
    h = R.gelu(H.HighProduct.apply(x, w1.transpose(0, 1), terms))
    z = H.HighProduct.apply(h, w2.transpose(0, 1), terms)
    return (s2 + R.layer_norm(z, norm2_weight, norm2_bias, eps)).reshape(shape)


def layer_split_statement(params, source, target, no_ffn=False, eps=1e-5, terms=3, attention_terms=None):
    """R.layer_statement with the tail's products as high products and, with attention_terms, the full attention's too (the layer
    with both seams installed at "high"); the projections and merge, the layer's own nn.Linears, stay float64."""
    p = {k: v.double() for k, v in params.items()}
    source, target = source.double(), target.double()
    q, k, v = source @ p["q_proj.weight"].T, target @ p["k_proj.weight"].T, target @ p["v_proj.weight"].T
    if attention_terms is None:
        m = R.W.full_lines(q, k, v)
    else:
        m = H.split_statement(q, k, v, 1, False, 1, q.shape[1], terms=attention_terms)
    m = m @ p["merge.weight"].T
    if no_ffn:
        return R.norm_statement(m, p["norm1.weight"], p["norm1.bias"], source, eps)
    return split_statement(source, m, p["norm1.weight"], p["norm1.bias"], p["mlp.0.weight"], p["mlp.2.weight"], p["norm2.weight"],
                           p["norm2.bias"], eps, terms)


errors, check_rule = H.errors, H.check_rule


# ---- the launch geometry of the "high" kernels -------------------------------------------------------------------------------

# The "high" kernels are launched on the "highest" kernels' geometry (high_launches; the spec test pins it), so the constants and
# their restatement are the ones tests/test_transformer_ffn_rows.py reads from the kernel file: one place to edit.
constants, geometry = ROWS.constants, ROWS.geometry


def high_launches():
    """{kernel: grid expression} of the "high" kernels' launches, as the kernel file writes them."""
    text = KERNEL_FILE.read_text()
    return {name: re.sub(r"\s+", " ", grid) for name, grid in
            re.findall(r"hipLaunchKernelGGL\((k_ffh_\w+), dim3\((.*?)\), dim3\(S360_BLOCK\)", text, flags=re.S)}


def geometry_cases():
    """name: the smallest T (with a ragged end) that reaches a path of the launch geometry: a second workgroup of the forward
    and the token pass (one token in it), a third (a full wave and a one-token wave), two tiles per weight chunk (the last chunk
    a full tile and a one-token tile), three (the last chunk 7 tokens), and the token pass's grid stride (two workgroups walk a
    second tile, the last one of 5 tokens)."""
    k = constants()
    ft, tm, chunks, wgs = k["FF_T"], k["FF_T"] * k["FF_WAVES"], k["FF_MAX_CHUNKS"], k["FF_TOKEN_WGS"]
    return {"wg2": tm + 1, "wg3": 2 * tm + ft + 1, "tiles2": chunks * ft + ft + 1, "tiles3": 2 * chunks * ft + ft + 7,
            "stride": (wgs + 1) * tm + 5}
