"""The argument vocabulary of the operators' Python wrappers (transformer_ffn, mono_fusion, window_attention, qkv_attention): what
a tensor argument must be, how it reaches the library, how the output buffers and a "high" call's scratch are taken or
allocated.  `what` is the public function the message names.  What a tensor that is not on the GPU raises is the operator's own
(ValueError for the FFN tail and the QKV attention, RuntimeError for the mono fusion and the window attention, each with its
text; callers may rely on either): `tensor_rule` makes the operator's `tensor`, and `buffers` and `high_scratch` take it.  The
QKV attention's kernels move one dword per lane, so its wrapper keeps `.detach().contiguous()` in place of `flat` and asks
`buffers` for a float's alignment."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor

from . import precision as _prec


def tensor_rule(off_gpu, off_gpu_message: str):
    """The operator's `tensor(what, name, t, shape=None, dtype=torch.float32, device=None)`: raises unless t is a GPU tensor of
    that dtype (device, shape).  A tensor that is not on the GPU raises `off_gpu` with `off_gpu_message` formatted with what,
    name and device; a module binds its rule once at import, so a call costs what a function of its own would."""
    def tensor(what: str, name: str, t, shape=None, dtype=torch.float32, device=None) -> None:
        if not isinstance(t, Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise off_gpu(off_gpu_message.format(what=what, name=name, device=t.device))
        if t.dtype != dtype:
            raise ValueError(f"{what}: {name} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")
        if device is not None and t.device != device:
            raise ValueError(f"{what}: {name} is on {t.device}, expected {device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return tensor


def flat(t: Tensor) -> Tensor:
    """Detached, contiguous and 16-byte aligned: a non-contiguous (or misaligned) input is copied once."""
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def buffers(what: str, names: Sequence[str], shapes, dtypes, device, given: Optional[dict], tensor, align: int = 16) -> list:
    """The output buffers of a call: `given` maps names to contiguous, `align`-byte aligned buffers of the right shape and dtype on
    the device to write into (every element is written); the others are allocated."""
    given = dict(given or {})
    unknown = set(given) - set(names)
    if unknown:
        raise ValueError(f"{what}: unknown buffers {sorted(unknown)}; the outputs are {list(names)}")
    out = []
    for name, shape, dtype in zip(names, shapes, dtypes):
        buf = given.get(name)
        if buf is None:
            buf = torch.empty(tuple(shape), dtype=dtype, device=device)
        else:
            tensor(what, name, buf, shape, dtype=dtype, device=device)
            if not buf.is_contiguous() or buf.data_ptr() % align:
                raise ValueError(f"{what}: the buffer {name} must be contiguous and {align}-byte aligned")
        out.append(buf)
    return out


def positive_int(what: str, name: str, v) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{what}: {name} must be a positive integer, got {v!r}")
    return v


def eps(what: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
        raise ValueError(f"{what}: eps must be a positive number, got {v!r}")
    return float(v)


def no_scratch(what: str, precision: str, given) -> None:
    """Only the "high" call takes the caller's scratch: one handed to a "highest" call would go unused, so it is refused."""
    if given is not None and precision != "high":
        raise ValueError(f"{what}: scratch is the buffer of a precision=\"high\" call, got one with precision={precision!r}")


def high_scratch(what: str, nbytes: int, device, given: Optional[Tensor], tensor) -> Tensor:
    """The scratch of a "high" call: `nbytes` (the operator's scratch_bytes) allocated, or the caller's uint8 buffer (the library
    checks its size and alignment)."""
    if given is None:
        return _prec.scratch(nbytes, device)
    tensor(what, "scratch", given, dtype=torch.uint8, device=device)
    if given.dim() != 1 or not given.is_contiguous():
        raise ValueError(f"{what}: scratch must be a contiguous 1-D uint8 buffer")
    return given
