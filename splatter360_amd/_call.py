"""How every operator module calls libs360.so: one pointer helper, one stream helper, one checked call.

The library is reached through `_lib.lib()` at call time (never cached here), so a test that replaces `_lib.lib` sees every call.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _lib


def ptr(t):
    """A tensor's address, or None (NULL for c_void_p and POINTER(...) parameters alike) for a missing tensor."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream(device) -> C.c_void_p:
    """The handle of `device`'s current stream."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def invoke(name: str, *args) -> None:
    """An entry point that returns a status, with the arguments as given: calls without a launch (workspace-size queries, host-only
    entry points) and call sites that hold their own device guard and pass their own stream."""
    _lib.check(getattr(_lib.lib(), name)(*args), name)


def call(name: str, device, *args) -> None:
    """A launch on `device`'s current stream (the ABI's last parameter), under that device's guard."""
    with torch.cuda.device(device):
        invoke(name, *args, stream(device))


def _check_cuda_f32(what: str, *ts: Tensor) -> None:
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU only (no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} takes float32 tensors, got {t.dtype}")
        if t.device != ts[0].device:
            raise ValueError(f"{what}: tensors on different devices ({ts[0].device}, {t.device})")
