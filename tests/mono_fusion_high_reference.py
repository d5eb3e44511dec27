"""The yardstick of the mono-feature fusion's "high" precision mode (splatter360_amd/mono_fusion.py, precision="high"): the
statement of tests/mono_fusion_reference.py with its two products — and, through window_attention_high_reference.HighProduct, the
four products of their backward — as bf16x3 products of split operands, everything else in float64.  What the kernels and this
file share is the specification:

  split(x)   hi = bf16(x), round to nearest even; lo = bf16(x - float32(hi))        (window_attention_high_reference.split)
  product    A B = Ah Bh + Ah Bl + Al Bh (terms=3); Al Bl is dropped.  terms=1 keeps Ah Bh alone: what a kernel that lost its lo
             planes would compute.  Both operands are split from their float32 values: X = [erp_feat, m] with m the float32
             stitch and W1, a = float32(relu(LN(y))) and W2, and in the backward g_out, g_y, X and a again.

Further how far the three-term products move LayerNorm's output (`ln_deviation`) against how far the nearest ReLU decision is from
0 (`ln_margin_abs`), and the launches of the "high" kernels as the kernel file writes them (`high_launches`).  Nothing here needs a
GPU.
"""
import re
from pathlib import Path

import torch

import mono_fusion_reference as R
import window_attention_high_reference as H

KERNEL_FILE = Path(__file__).resolve().parent.parent / "splatter360_amd" / "csrc" / "s360_mono_fusion.hip"
errors, check_rule = H.errors, H.check_rule


def split_statement(erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps=1e-5, terms=3, parts=None, m=None):
    """R.statement with high products: float32 tensors -> out [N, C, H, W], float64; differentiable in erp_feat and the
    parameters (g_a = g_out W2, g_X = g_y W1, g_w1 = g_y^T X and g_w2 = g_out^T a are high products of their own split operands).
    m: R.stitch32 of the case if at hand.  parts: a dict that receives "y", the first high product [T, C], and "ln", LayerNorm's
    output [N, H, W, C]."""
    if m is None:
        m = R.stitch32(mono_cube, grid)
    m = m.to(device=erp_feat.device, dtype=torch.float64)
    erp_feat, w1, ln_weight, ln_bias, w2 = (t.double() for t in (erp_feat, w1, ln_weight, ln_bias, w2))
    n, c, h, w = erp_feat.shape
    x = torch.cat([erp_feat, m], dim=1).permute(0, 2, 3, 1).reshape(n * h * w, -1)
    y = H.HighProduct.apply(x, w1.transpose(0, 1), terms)
    ln = R.layer_norm(y, ln_weight, ln_bias, eps)
    if parts is not None:
        parts["y"] = y
        parts["ln"] = ln.reshape(n, h, w, c)
    out = H.HighProduct.apply(torch.relu(ln), w2.transpose(0, 1), terms)
    return out.reshape(n, h, w, c).permute(0, 3, 1, 2)


def three_rows(tensors, g, eps=1e-5, terms=3):
    """split_statement and its gradients by autograd in the per-row indexing of R.row_statement (R.ROW_NAMES, y taken from
    inside), float64 on the inputs' device: the specification's own rows, the second yardstick of the per-row "high" rule."""
    m = R.stitch32(tensors[1], tensors[2])
    return R._rows_of(lambda *t, parts: split_statement(*t, eps=eps, terms=terms, parts=parts, m=m), tensors, g, torch.float64)[0]


def ln_outputs(tensors, m=None, terms=3):
    """(LayerNorm's output of the float64 statement, of the split statement with `terms` terms), on the CPU."""
    cpu = [t.detach().cpu() for t in tensors]
    p64, ps = {}, {}
    with torch.no_grad():
        R.statement(*cpu, parts=p64, m=m)
        split_statement(*cpu, terms=terms, parts=ps, m=m)
    return p64["ln"], ps["ln"]


def ln_deviation(tensors, m=None) -> float:
    """max |LN_3 - LN_64| over LayerNorm's outputs of the three-term and the float64 statement."""
    ln64, ln3 = ln_outputs(tensors, m)
    return (ln3 - ln64).abs().max().item()


def ln_margin_abs(tensors, m=None) -> float:
    """The smallest |value| over LayerNorm's outputs of the float64 statement: how far the nearest ReLU decision is from 0."""
    return ln_outputs(tensors, m)[0].abs().min().item()


def flipped_decisions(tensors, m=None, terms=3) -> int:
    """How many ReLU decisions of the float64 statement the split statement takes the other way."""
    ln64, lns = ln_outputs(tensors, m, terms)
    return int(((ln64 > 0) != (lns > 0)).sum().item())


def launches(prefix):
    """{kernel: grid expression} of the launches of the kernels k_<prefix>_*, as the kernel file writes them."""
    text = KERNEL_FILE.read_text()
    return {name: re.sub(r"\s+", " ", grid) for name, grid in
            re.findall(rf"hipLaunchKernelGGL\((k_{prefix}_\w+), dim3\((.*?)\), dim3\(S360_BLOCK\)", text, flags=re.S)}


def high_launches():
    return launches("mfh")
