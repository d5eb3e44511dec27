"""The yardstick of the QKV attention's "high" precision mode (splatter360_amd/qkv_attention.py, precision="high"): the function
of tests/qkv_attention_reference.py with each of its six products as a bf16x3 product of split operands, every sum in float64.
The specification is the window attention's (tests/window_attention_high_reference.py: `split`, `HighProduct`), not written a
second time:

  split(x)   hi = bf16(x), round to nearest even; lo = bf16(x - float32(hi))
  product    A B = Ah Bh + Ah Bl + Al Bh (terms=3); Al Bl is dropped.  terms=1 keeps Ah Bh alone: the single-bf16 product a
             kernel that lost a lo plane would compute.

q and k are split UNSCALED and 1 / sqrt(ch) divides the summed score once; P and dS are split from the values the float64 softmax
and its backward leave, rounded to float32.  Further the cases the CPU and the GPU tests of the mode share.
"""
import torch

import qkv_attention_reference as R
from window_attention_high_reference import HighProduct, bound, check_rule, errors, split  # noqa: F401  (all but HighProduct: for the tests)

# name: (N, views, cross_view, heads, T, order); ch = 32: the nine shapes of tests/test_gpu_qkv_attention.py and two more
SHAPES = {
    "tile": (2, 1, False, 1, 32, "legacy"),
    "ragged": (2, 1, False, 2, 35, "legacy"),
    "tiny": (1, 1, False, 1, 5, "legacy"),
    "straddle": (4, 2, True, 4, 48, "legacy"),
    "views3": (3, 3, True, 1, 20, "legacy"),
    "frames_unused": (4, 2, False, 2, 40, "legacy"),
    "new_order": (2, 2, True, 2, 40, "new"),
    "long": (2, 2, True, 1, 320, "legacy"),
    "uneven": (2, 2, True, 1, 100, "legacy"),
    "t16": (1, 1, False, 1, 16, "legacy"),           # exactly one k-step of the second product
    "t17": (1, 1, False, 1, 17, "legacy"),           # one token past it
}
# the seed rule of tests/test_gpu_qkv_attention.py, over these eleven names
SEEDS = {n: 2000 + 7 * i for i, n in enumerate(sorted(SHAPES))}
SCALES = (1.0, 6.0)
NAMES = ("out", "g_qkv", "g_q", "g_k", "g_v")


def split_statement(qkv, heads, views=1, cross_view=False, order="legacy", terms=3):
    """R.statement with high products: qkv [N, heads 3 ch, T] -> out [N, heads ch, T] float64; differentiable (dP = dO^T V,
    g_q = K dS^T, g_k = Q dS and g_v = dO P are high products too, through HighProduct.backward)."""
    q, k, v = (x.double() for x in R.split_heads(qkv, heads, views, cross_view, order))            # [B, heads, ch, L]
    scores = HighProduct.apply(q.transpose(-1, -2), k, terms) / q.shape[2] ** 0.5                  # [B, heads, L queries, L keys]
    out = HighProduct.apply(torch.softmax(scores, dim=-1), v.transpose(-1, -2), terms)             # [B, heads, L, ch]
    return R.merge_heads(out.transpose(-1, -2), views, cross_view)


def case(name, scale, device="cpu"):
    """(qkv, g) of one run."""
    n, views, cross, heads, t, order = SHAPES[name]
    return R.random_case(n, heads, t, scale=scale, seed=SEEDS[name], device=device)


def with_parts(name, pair):
    """(out, g_qkv) -> (out, g_qkv, g_q, g_k, g_v): NAMES' order."""
    out, g_qkv = pair
    return (out, g_qkv, *R.parts(g_qkv, SHAPES[name][3], SHAPES[name][5]))


def yardsticks(name, scale, device="cpu"):
    """((qkv, g), want, three, lines): the float64 statement, the terms=3 statement and the float32 lines on `device`, each in
    NAMES' order."""
    n, views, cross, heads, t, order = SHAPES[name]
    qkv, g = case(name, scale, device)
    want = R.gradients(lambda x: R.statement(x, heads, views, cross, order), qkv, g, torch.float64)
    three = R.gradients(lambda x: split_statement(x, heads, views, cross, order, terms=3), qkv, g, torch.float64)
    lines = R.gradients(lambda x: R.reference_lines(x, heads, views, cross, order), qkv, g)
    return (qkv, g), with_parts(name, want), with_parts(name, three), with_parts(name, lines)


