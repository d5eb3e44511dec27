"""The one precision rule of the four operators that have a "high" mode (window_attention, qkv_attention, transformer_ffn,
mono_fusion): every kernel of the package that uses the matrix unit obeys it.

precision="highest" forms every product from exact float32 products; precision="high" is what
torch.set_float32_matmul_precision('high') asks for: each float32 number as the sum of two bfloat16 numbers and each product
A B as Ah Bh + Ah Bl + Al Bh on the bf16 MFMA, accumulated in float32 (csrc/s360_bf16x3.h).  "torch", where an option takes it,
follows torch.get_float32_matmul_precision() at every call.
"""
from __future__ import annotations

import torch
from torch import Tensor

PRECISIONS = ("highest", "high")
_TORCH_PRECISIONS = {"highest": "highest", "high": "high", "medium": "high"}    # never less accurate than asked


def check(operator_name: str, precision: str) -> str:
    """`precision` if it is one of PRECISIONS; ValueError in `operator_name`'s words otherwise."""
    if not isinstance(precision, str) or precision not in PRECISIONS:
        raise ValueError(f"{operator_name} knows the precisions {list(PRECISIONS)}, got precision={precision!r}")
    return precision


def resolve(name: str) -> str:
    """"highest" or "high" as they are; "torch": what torch.get_float32_matmul_precision() says now — 'highest' is "highest",
    'high' and 'medium' are "high" (there is no single-bf16 mode: the result is never less accurate than asked)."""
    if name == "torch":
        return _TORCH_PRECISIONS[torch.get_float32_matmul_precision()]
    return check("window_attention", name)


def seam_option(option_name: str, value) -> str:
    """The value of an install() precision option, checked when the seam is installed: one of PRECISIONS, or "torch", which is
    kept as it is (`resolve` reads torch's float32 matmul precision at every call)."""
    if value != "torch" and value not in PRECISIONS:
        raise ValueError(f"{option_name} is one of {[*PRECISIONS, 'torch']}, got {value!r}")
    return value


def scratch(nbytes: int, device) -> Tensor:
    """The uint8 scratch tensor of one call; the operator's scratch_bytes says how many bytes."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)
