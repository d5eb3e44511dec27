"""What the host-side argument rule must leave alone, and what it must stop, at the two attention operators on the GPU
(csrc/s360_window_attention.hip, csrc/s360_qkv_attention.hip through their wrappers), forward and backward in both precisions:
inputs may be one another (self-attention on one tensor); a window input that is contiguous but not 16-byte aligned is copied,
not refused; the QKV attention takes such a tensor where it lies, as its kernels move one dword per lane; and a call refused for
an output that is an input has written nothing.  Every comparison is bit for bit: the runs differ only in where the data lies.
"""
import pytest
import torch

from splatter360_amd import _lib, qkv_attention as qa, window_attention as wa
from splatter360_amd._call import ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("highest", "high")
WINDOW = dict(height=4, width=8, num_splits=2, with_shift=True)          # B = 1, 4 x 8 tokens, C = 32


def _offset_view(t):
    """t's values as a contiguous tensor 4 bytes into a buffer of its own: not 16-byte aligned."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = flat[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _window(q, k, v, g, precision):
    out, lse = wa.attention_forward(q, k, v, precision=precision, **WINDOW)
    return (out, *wa.attention_backward(q, k, v, lse, g, precision=precision, **WINDOW))


def _window_case(seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(1, 32, 32, device=DEV, generator=gen) for _ in range(2))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_attention_takes_one_tensor_as_q_k_and_v(precision):
    q, g = _window_case(1)
    want = _window(q, q.clone(), q.clone(), g, precision)
    got = _window(q, q, q, g, precision)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_window_attention_copies_a_misaligned_input(precision):
    q, g = _window_case(2)
    k, v = q.flip(1).contiguous(), q.roll(3, 1).contiguous()
    want = _window(q, k, v, g, precision)
    got = _window(_offset_view(q), k, v, g, precision)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_qkv_attention_reads_a_misaligned_qkv_where_it_lies(precision):
    gen = torch.Generator(device=DEV).manual_seed(3)
    qkv, g = torch.randn(2, 96, 35, device=DEV, generator=gen), torch.randn(2, 32, 35, device=DEV, generator=gen)      # T = 35: ragged

    def run(x):
        out, lse = qa.attention_forward(x, 1, precision=precision)
        return out, qa.attention_backward(x, lse, g, 1, precision=precision)

    want, got = run(qkv), run(_offset_view(qkv))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_window_forward_refused_for_out_equal_to_k_writes_nothing(precision):
    q, k = _window_case(4)
    v, before = q.flip(1).contiguous(), k.clone()
    lse = torch.empty(1, 32, dtype=torch.float64, device=DEV)
    args = [ptr(q), ptr(k), ptr(v), 1, 0, 4, 8, 32, 2, 1, 0, ptr(k), ptr(lse)]
    name = "s360_window_attention_forward"
    if precision == "high":
        scratch = torch.empty(wa.scratch_bytes(1, 0, 4, 8, 32, 2, False), dtype=torch.uint8, device=DEV)
        args += [ptr(scratch), scratch.numel()]
        name = "s360_window_attention_high_forward"
    assert getattr(_lib.lib(), name)(*args, stream(torch.device(DEV))) == -1                  # S360_E_BADARG
    torch.cuda.synchronize()
    assert torch.equal(k, before)
