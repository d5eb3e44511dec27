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


# ---- H.check_rule, the accuracy rule the four "high" GPU files share, on tensors whose errors are exact powers of two
def _ruled(e3, e32, kernel, want=None):
    """check_rule on one tensor "t" of 64 elements: `want` (ones), want + e3 as the terms=3 statement, want + e32 as the float32
    lines and want + kernel as the kernel's float32 result; each error a number or a tensor of 64."""
    want = torch.ones(64, dtype=torch.float64) if want is None else want
    three, lines, got = want + e3, (want + e32).float(), (want + kernel).float()
    assert torch.equal(got.double(), want + kernel) and torch.equal(lines.double(), want + e32)       # nothing was rounded away
    H.check_rule("case", ("t",), (want,), (three,), (lines,), (got,))


def _only(i, v):
    x = torch.zeros(64, dtype=torch.float64)
    x[i] = v
    return x


def test_check_rule_passes_the_statement_itself_and_prints_every_figure(capsys):
    _ruled(2.0 ** -10, 2.0 ** -12, 2.0 ** -10)
    line = capsys.readouterr().out
    for field in ("case t: kernel max 9.766e-04 mean 9.766e-04", "e3 max 9.766e-04", "e32 max 2.441e-04", "floor 5.960e-08",
                  "kernel / bound 0.533 0.533", "kernel / e3 1.00 1.00"):
        assert field in line, (field, line)


def test_check_rule_fails_on_the_maximum_alone():
    e3, e32 = 2.0 ** -10, 2.0 ** -12
    _ruled(e3, e32, e3 + _only(5, 1.5 * (e3 + e32) - e3))                    # 1.5 x (e3 + e32) at one element: the bound itself
    with pytest.raises(AssertionError) as failed:
        _ruled(e3, e32, e3 + _only(5, 2.0 ** -9 - e3))                       # 2^-9 = 1.6 x (e3 + e32) there
    tag, ((name, kmax, kmean, bmax, bmean),) = failed.value.args[0]
    assert (tag, name, kmax, bmax) == ("case", "t", 2.0 ** -9, 1.5 * (e3 + e32)) and kmean <= bmean


def test_check_rule_fails_on_the_mean_alone():
    e3 = _only(0, 2.0 ** -10)                                                # max 2^-10, mean 2^-16; the float32 lines exact
    _ruled(e3, 0.0, 2.0 ** -16)
    with pytest.raises(AssertionError) as failed:
        _ruled(e3, 0.0, 2.0 ** -12)                                          # below the maximum's bound at every element
    tag, ((name, kmax, kmean, bmax, bmean),) = failed.value.args[0]
    assert kmax == 2.0 ** -12 <= bmax == 1.5 * 2.0 ** -10 and kmean == 2.0 ** -12 > bmean == 1.5 * 2.0 ** -16


def test_check_rule_fails_on_one_nan_a_wrong_dtype_and_a_wrong_shape():
    want = torch.ones(64, dtype=torch.float64)
    good = want.float()
    bad = good.clone()
    bad[17] = float("nan")
    for got in (bad, good.double(), good[:63], good.view(8, 8)):
        with pytest.raises(AssertionError) as failed:
            H.check_rule("case", ("t",), (want,), (want,), (good,), (got,))
        assert failed.value.args[0] == ("case", "t")
    H.check_rule("case", ("t",), (want,), (want,), (good,), (good,))


def test_check_rule_lets_the_floor_decide_where_both_yardsticks_are_exact():
    want = torch.ones(64, dtype=torch.float64) + _only(0, 2.0 ** 20 - 1.0)   # max|want| = 2^20: the floor is 2^-4
    _ruled(0.0, 0.0, 2.0 ** -4 * (want == 1.0), want)                        # e3 = e32 = 0: only the floor admits 2^-4
    with pytest.raises(AssertionError):
        _ruled(0.0, 0.0, _only(1, 2.0 ** -3), want)
    with pytest.raises(AssertionError):
        _ruled(0.0, 0.0, 2.0 ** -4 * (want == 1.0))                          # the same error with max|want| = 1: floor 2^-24


def test_check_rule_collects_every_failing_tensor_before_it_asserts():
    want = torch.ones(64, dtype=torch.float64)
    exact, off = want.float(), (want + 2.0 ** -10).float()
    with pytest.raises(AssertionError) as failed:
        H.check_rule("case", ("a", "b", "c"), (want,) * 3, (want,) * 3, (exact,) * 3, (off, exact, off))
    assert [f[0] for f in failed.value.args[0][1]] == ["a", "c"]


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
