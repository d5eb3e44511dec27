"""The specification of the window attention's "high" precision mode, on the CPU: the split, what the three-term product buys
over a single bf16 product (the condition that gives the accuracy bound of tests/test_gpu_window_attention_high.py its meaning),
the argument errors, resolve_precision, the install option and the three C entry points.

Discrimination, measured on one CPU with random_case(seed=5) over the 22 runs below, four tensors each: the terms=1 statement's
error against statement(float64) is at least 280 x (max) and 332 x (mean) the terms=3 statement's; the test asks for 50 x.  The
terms=3 statement's own error is 6 to 100 x (max) and 10 to 48 x (mean) the float32 lines'.
"""
import functools
import re
import sys
from pathlib import Path

import pytest
import torch

import window_attention_high_reference as H
import window_attention_reference as R
from splatter360_amd import _lib, plugin, window_attention as wa

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("out", "g_q", "g_k", "g_v")
# name: (B, m, h, w, K, C), the shapes of tests/test_gpu_window_attention.py
SHAPES = {
    "tile": (2, 0, 8, 16, 2, 128),
    "ragged": (1, 0, 10, 14, 2, 128),
    "multi": (2, 3, 8, 12, 2, 128),
    "c32": (1, 2, 8, 8, 2, 32),
    "long": (1, 0, 32, 64, 2, 128),
    "k1": (2, 0, 4, 5, 1, 128),
}
RUNS = [(name, shift, scale) for name, s in SHAPES.items() for shift in ((False, True) if s[4] > 1 else (False,)) for scale in (1.0, 6.0)]


def test_split_is_two_bfloat16_numbers_within_2_to_the_minus_16():
    gen = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(4096, generator=gen) * s for s in (1e-20, 1e-3, 1.0, 300.0, 1e20)]
                  + [torch.tensor([0.0, -0.0, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 3.0e38, 2.0 ** -126])])
    hi, lo = H.split(x)
    assert hi.dtype == lo.dtype == torch.bfloat16
    for part in (hi, lo):                                       # bf16-exact: the float32 value has 16 zero low bits
        assert (part.to(torch.float32).view(torch.int32) & 0xFFFF).eq(0).all()
    assert torch.equal(hi, x.to(torch.bfloat16))                # round to nearest even: 1 + 2^-8 ties to 1, 1 + 2^-9 rounds down
    assert hi[-4].item() == 1.0 and hi[-3].item() == 1.0
    assert torch.equal(lo, (x - hi.float()).to(torch.bfloat16))
    err = (hi.double() + lo.double() - x.double()).abs()
    assert (err <= 2.0 ** -16 * x.double().abs()).all()
    assert (err > 2.0 ** -20 * x.double().abs()).any()          # and it is a two-term split, not an exact one


@functools.lru_cache(maxsize=None)
def _statements(name, shift, scale):
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=scale, seed=5)
    want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, ksp, shift, h, w), q, k, v, g, torch.float64)
    three, one = (R.gradients(lambda a, bb, cc: H.split_statement(a, bb, cc, ksp, shift, h, w, terms=t), q, k, v, g, torch.float64)
                  for t in (3, 1))
    return want, three, one


@pytest.mark.parametrize("name,shift,scale", RUNS)
def test_three_terms_are_fifty_times_closer_than_one(name, shift, scale):
    want, three, one = _statements(name, shift, scale)
    for n, w64, t3, t1 in zip(NAMES, want, three, one):
        assert t3.dtype == torch.float64 and t3.shape == w64.shape
        (max3, mean3), (max1, mean1) = H.errors(t3, w64), H.errors(t1, w64)
        print(f"{name} shift={int(shift)} scale={scale:g} {n}: terms=1 max {max1:.3e} mean {mean1:.3e} | terms=3 max {max3:.3e} mean {mean3:.3e}"
              f" | ratios {max1 / max3:.0f} {mean1 / mean3:.0f}")
        assert max3 > 0.0 and max1 >= 50.0 * max3 and mean1 >= 50.0 * mean3, (name, shift, scale, n)


def test_an_unknown_precision_is_refused_before_any_tensor_is_touched():
    q, k, v, g = R.random_case(1, 0, 4, 8, c=32, seed=1)
    opts = dict(height=4, width=8, num_splits=2)
    for call in (lambda: wa.window_attention(q, k, v, precision="fast", **opts), lambda: wa.full_attention(q, k, v, precision="fast"),
                 lambda: wa.attention_forward(q, k, v, precision="fast", **opts),
                 lambda: wa.attention_backward(q, k, v, None, g, precision="fast", **opts),
                 lambda: wa.window_attention(None, None, None, precision="medium", **opts)):
        with pytest.raises(ValueError, match=r"'highest', 'high'"):
            call()
    assert wa.PRECISIONS == ("highest", "high")
    for good in wa.PRECISIONS:                                  # a known precision goes on to the device check (no CPU path)
        with pytest.raises(RuntimeError, match="GPU only"):
            wa.window_attention(q, k, v, precision=good, **opts)


def test_resolve_precision_follows_torch_at_call_time():
    assert wa.resolve_precision("highest") == "highest" and wa.resolve_precision("high") == "high"
    with pytest.raises(ValueError, match=r"'highest', 'high'"):
        wa.resolve_precision("medium")
    before = torch.get_float32_matmul_precision()
    try:
        for setting, want in (("highest", "highest"), ("high", "high"), ("medium", "high")):
            torch.set_float32_matmul_precision(setting)
            assert wa.resolve_precision("torch") == want
    finally:
        torch.set_float32_matmul_precision(before)
    assert torch.get_float32_matmul_precision() == before


@pytest.fixture
def standin():
    assert plugin.WINDOW_ATTENTION_MODULE not in sys.modules
    mod = R.standin_module(plugin.WINDOW_ATTENTION_MODULE)
    sys.modules[plugin.WINDOW_ATTENTION_MODULE] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        del sys.modules[plugin.WINDOW_ATTENTION_MODULE]


@pytest.mark.parametrize("precision", ["highest", "high", "torch"])
def test_the_install_option_is_recorded_and_uninstall_restores(standin, precision):
    originals = {n: getattr(standin, n) for n in plugin.WINDOW_ATTENTION_NAMES}
    bound = plugin.install_window_attention(precision=precision)
    assert plugin.WINDOW_ATTENTION_SEAM.options == {"precision": precision}
    for n in (plugin.WINDOW_ATTENTION_SPLIT, plugin.WINDOW_ATTENTION_FULL):
        assert getattr(standin, n) is bound[n] and bound[n].replaced is originals[n] and bound[n].precision == precision
    # CPU tensors still reach the replaced functions, whatever the precision
    q, k, v, _ = R.random_case(1, 0, 4, 8, c=32, seed=1)
    assert torch.equal(standin.layer(q, k, v, 4, 8, 2, False), R.reference_lines(q, k, v, 2, False, 4, 8))
    plugin.uninstall()
    assert all(getattr(standin, n) is originals[n] for n in plugin.WINDOW_ATTENTION_NAMES)


def test_the_default_install_is_highest_and_an_unknown_option_is_refused(standin):
    originals = {n: getattr(standin, n) for n in plugin.WINDOW_ATTENTION_NAMES}
    assert plugin.install_window_attention()[plugin.WINDOW_ATTENTION_SPLIT].precision == "highest"
    plugin.uninstall()
    for bad in (lambda: plugin.install_window_attention(precision="medium"),
                lambda: plugin.install(lazy=True, window_attention=True, window_attention_precision="fast")):
        with pytest.raises(ValueError, match="'highest', 'high', 'torch'"):
            bad()
    assert all(getattr(standin, n) is originals[n] for n in plugin.WINDOW_ATTENTION_NAMES)
    plugin.install(lazy=True, window_attention=True, window_attention_precision="torch")
    assert getattr(standin, plugin.WINDOW_ATTENTION_FULL).precision == "torch"


def test_the_three_entry_points_are_declared_bound_and_sized():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in ("s360_window_attention_high_scratch_bytes", "s360_window_attention_high_forward", "s360_window_attention_high_backward"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 25 and "#define S360_ABI_VERSION 25" in (ROOT / "include" / "s360.h").read_text()
    lib = _lib.lib()
    # host arithmetic: the planes of (q, k, v) are as many bytes as the tensors (bf16 hi + lo = 4 bytes an element) and a
    # transposed plane rounds a window's rows up to a multiple of 4
    b, m, h, w, c, ksp = 2, 3, 8, 12, 128, 2
    nq, nk, lw = b * h * w * c, b * m * h * w * c, h * w // 4
    assert wa.scratch_bytes(b, m, h, w, c, ksp, False) == 4 * (nq + 2 * nk)
    assert wa.scratch_bytes(b, m, h, w, c, ksp, True) == 4 * (3 * nq + 3 * nk) + 4 * nq
    assert wa.scratch_bytes(1, 0, 10, 14, 32, 2, False) == 4 * 140 * 32 * 2 + 4 * 4 * 32 * 36      # Lw = 35 -> 36
    for bad in ((0, 0, 8, 8, 32, 2), (1, 0, 8, 8, 48, 2), (1, 0, 8, 9, 32, 2), (1, -1, 8, 8, 32, 2)):
        assert lib.s360_window_attention_high_scratch_bytes(*bad, 0) == 0
    # refusals that need no device memory: null tensors, then a null scratch behind valid-looking (never read) addresses
    assert lib.s360_window_attention_high_forward(None, None, None, 1, 0, 8, 8, 32, 2, 0, 0, None, None, None, 0, None) == -1
    assert lib.s360_window_attention_high_backward(None, None, None, None, None, 1, 0, 8, 8, 32, 2, 0, 0, None, None, None, None,
                                                   None, 0, None) == -1
