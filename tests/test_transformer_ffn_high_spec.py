"""The specification of the FFN tail's "high" precision mode, on the CPU: what the three-term product buys over a single bf16
product (the condition that gives the accuracy bound of tests/test_gpu_transformer_ffn_high.py its meaning), the token counts of
that file's geometry cases from the kernel file's constants, the argument errors, the install option and the three C entry points.

Discrimination, measured on one CPU with R.random_case(T, scale, seed=3000 + T) over T in {5, 33, 129, 545} x scale in {1, 6},
out and seven gradients each: the terms=1 statement's error against statement(float64) is at least 233 x (max) and 422 x (mean)
the terms=3 statement's; the test asks for 50 x, the window attention's figure.  g_norm2_bias holds no product and is exact in
both statements.
"""
import functools
import re
import sys
from pathlib import Path

import pytest
import torch

import transformer_ffn_high_reference as HR
import transformer_ffn_reference as R
from splatter360_amd import _lib, plugin, transformer_ffn as tf

ROOT = Path(__file__).resolve().parent.parent
RUNS = [(t, scale) for t in (5, 33, 129, 545) for scale in (1.0, 6.0)]
PLANE_BYTES = 2 * 2 * 2 * (tf.HIDDEN * 2 * tf.CHANNELS + tf.CHANNELS * tf.HIDDEN)       # two layouts x (hi, lo) x 2 bytes, w1 and w2


@functools.lru_cache(maxsize=None)
def _statements(tokens, scale):
    tensors, g = R.random_case(tokens, scale, seed=3000 + tokens)
    want = R.gradients(lambda *t: R.statement(*t), tensors, g, torch.float64)
    three, one = (R.gradients(lambda *t: HR.split_statement(*t, terms=terms), tensors, g, torch.float64) for terms in (3, 1))
    return want, three, one


@pytest.mark.parametrize("tokens,scale", RUNS)
def test_three_terms_are_fifty_times_closer_than_one(tokens, scale):
    want, three, one = _statements(tokens, scale)
    for n, w64, t3, t1 in zip(HR.OUT_NAMES, want, three, one):
        assert t3.dtype == torch.float64 and t3.shape == w64.shape
        if n in HR.EXACT:
            assert torch.equal(t3, w64) and torch.equal(t1, w64), n
            continue
        (max3, mean3), (max1, mean1) = HR.errors(t3, w64), HR.errors(t1, w64)
        print(f"T={tokens} scale={scale:g} {n}: terms=1 max {max1:.3e} mean {mean1:.3e} | terms=3 max {max3:.3e} mean {mean3:.3e}"
              f" | ratios {max1 / max3:.0f} {mean1 / mean3:.0f}")
        assert max3 > 0.0 and max1 >= 50.0 * max3 and mean1 >= 50.0 * mean3, (tokens, scale, n)


def test_the_split_statement_takes_leading_dimensions():
    tensors, g = R.random_case(40, seed=9, lead=(2, 4, 5))
    flat = [t.reshape(-1, 128) if t.dim() == 4 else t for t in tensors]
    a = R.gradients(lambda *t: HR.split_statement(*t), tensors, g, torch.float64)
    b = R.gradients(lambda *t: HR.split_statement(*t), flat, g.reshape(-1, 128), torch.float64)
    assert a[0].shape == (2, 4, 5, 128) and all(torch.equal(x.reshape(y.shape), y) for x, y in zip(a, b))


def test_the_geometry_cases_come_from_the_kernel_file_s_constants():
    """The "high" kernels are launched on the geometry of the "highest" ones, so the token counts at which a path is first taken
    are those of transformer_ffn_reference.ROW_CASES; a change of a constant or of a launch fails here."""
    k, cases = HR.constants(), HR.geometry_cases()
    launches = HR.high_launches()
    assert launches == {"k_ffh_split": "(unsigned)((FFH_W1 + FFH_W2 + S360_BLOCK - 1) / S360_BLOCK)",
                        "k_ffh_forward": "(tokens + FF_TM - 1) / FF_TM", "k_ffh_backward_tokens": "wgs",
                        "k_ffh_backward_weights": "FF_H / (FF_T * FF_WAVES), chunks"}
    text = HR.KERNEL_FILE.read_text()
    high = text[text.index("k_ffh_backward_tokens"):]
    assert "tile += gridDim.x" in high and "const int chunks = ff_chunks(tokens), wgs = ff_token_wgs(tokens);" in high
    assert cases == {n: R.ROW_CASES[n] for n in cases} == {"wg2": 129, "wg3": 289, "tiles2": 545, "tiles3": 1063, "stride": 65669}
    ft, geo = k["FF_T"], {n: HR.geometry(t) for n, t in cases.items()}
    tm = geo["wg2"]["tm"]
    assert geo["wg2"]["token_wgs"] == 2 and HR.geometry(cases["wg2"] - 1)["token_wgs"] == 1
    assert geo["wg3"]["token_wgs"] == 3 and cases["wg3"] - 2 * tm == ft + 1
    assert geo["tiles2"]["chunk_tokens"] == 2 * ft and cases["tiles2"] - (geo["tiles2"]["chunks"] - 1) * 2 * ft == ft + 1
    assert HR.geometry(k["FF_MAX_CHUNKS"] * ft)["chunk_tokens"] == ft
    assert geo["tiles3"]["chunk_tokens"] == 3 * ft and cases["tiles3"] - (geo["tiles3"]["chunks"] - 1) * 3 * ft == 7
    assert HR.geometry(2 * k["FF_MAX_CHUNKS"] * ft)["chunk_tokens"] == 2 * ft
    g = geo["stride"]
    assert g["token_wgs"] == k["FF_TOKEN_WGS"] and g["token_tiles"] == k["FF_TOKEN_WGS"] + 2
    assert cases["stride"] - (g["token_tiles"] - 1) * tm == 5
    assert all(geo[n]["token_tiles"] <= k["FF_TOKEN_WGS"] for n in cases if n != "stride")


def test_an_unknown_precision_is_refused_before_any_tensor_is_touched():
    tensors, g = R.random_case(5, seed=1)
    for call in (lambda: tf.ffn_tail(*tensors, precision="fast"), lambda: tf.ffn_tail_forward(*tensors, precision="fast"),
                 lambda: tf.ffn_tail_backward(*tensors, None, None, g, precision="fast"),
                 lambda: tf.ffn_tail(*(None,) * 8, precision="medium"), lambda: tf.ffn_tail(*tensors, precision=None),
                 lambda: tf.scratch_bytes(5, True, "torch")):
        with pytest.raises(ValueError, match=r"'highest', 'high'"):
            call()
    assert tf.PRECISIONS == ("highest", "high")
    for good in tf.PRECISIONS:                                  # a known precision goes on to the device check (no CPU path)
        with pytest.raises(ValueError, match="GPU"):
            tf.ffn_tail(*tensors, precision=good)


def test_a_scratch_buffer_is_refused_unless_the_precision_is_high():
    """The "highest" forward has no scratch and its backward allocates its own: a caller's buffer would go unused."""
    tensors, g = R.random_case(5, seed=1)
    scratch = torch.empty(16, dtype=torch.uint8)
    for call in (lambda: tf.ffn_tail_forward(*tensors, scratch=scratch), lambda: tf.ffn_tail_forward(*tensors, precision="highest", scratch=scratch),
                 lambda: tf.ffn_tail_backward(*tensors, None, None, g, scratch=scratch)):
        with pytest.raises(ValueError, match='scratch is the buffer of a precision="high" call'):
            call()
    with pytest.raises(ValueError, match="GPU"):                # with "high" it goes on to the device check
        tf.ffn_tail_forward(*tensors, precision="high", scratch=scratch)


@pytest.fixture
def standin():
    assert plugin.TRANSFORMER_FFN_MODULE not in sys.modules
    mod = R.standin_module(plugin.TRANSFORMER_FFN_MODULE)
    sys.modules[plugin.TRANSFORMER_FFN_MODULE] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        del sys.modules[plugin.TRANSFORMER_FFN_MODULE]


def _forward(standin):
    return standin.TransformerLayer.forward


@pytest.mark.parametrize("precision", ["highest", "high", "torch"])
def test_the_install_option_is_recorded_and_uninstall_restores(standin, precision):
    original = _forward(standin)
    bound = plugin.install_transformer_ffn(precision=precision)
    assert plugin.TRANSFORMER_FFN_SEAM.options == {"precision": precision}
    assert _forward(standin) is bound and bound.replaced is original and bound.precision == precision
    # CPU tensors still reach the replaced method, whatever the precision
    layer = R.randomise(standin.TransformerLayer(d_model=128), 3)
    x = torch.randn(1, 6, 128, generator=torch.Generator().manual_seed(4))
    layer(x, x, attn_num_splits=1)
    assert layer.calls == 1 and bound.native_calls == 0
    plugin.uninstall()
    assert _forward(standin) is original


def test_a_second_install_with_another_precision_replaces_the_wrapper(standin):
    """No uninstall() between: the recorded option is the one the bound wrapper runs with, one layer deep; the same option
    again keeps the wrapper (and its call count).  The window attention's seam, on the same mechanism, alike."""
    original = _forward(standin)
    first = plugin.install_transformer_ffn(precision="highest")
    assert plugin.install_transformer_ffn(precision="highest") is first
    plugin.install(lazy=True, transformer_ffn=True, transformer_ffn_precision="high")
    second = _forward(standin)
    assert second is not first and second.precision == "high" and second.replaced is original
    assert plugin.TRANSFORMER_FFN_SEAM.options == {"precision": "high"}
    third = plugin.install_transformer_ffn(precision="torch")
    assert third is _forward(standin) and third.precision == "torch" and third.replaced is original
    plugin.install_window_attention(precision="highest")
    plugin.install_window_attention(precision="high")
    full = getattr(standin, plugin.WINDOW_ATTENTION_FULL)
    assert full.precision == "high" and getattr(full.replaced, "replaced", None) is None
    assert plugin.WINDOW_ATTENTION_SEAM.options == {"precision": "high"}
    plugin.uninstall()
    assert _forward(standin) is original and getattr(getattr(standin, plugin.WINDOW_ATTENTION_FULL), "replaced", None) is None


def test_the_default_install_is_highest_and_an_unknown_option_is_refused(standin):
    original = _forward(standin)
    assert plugin.install_transformer_ffn().precision == "highest"
    plugin.uninstall()
    plugin.install(lazy=True, transformer_ffn=True)
    assert _forward(standin).precision == "highest" and plugin.TRANSFORMER_FFN_SEAM.options == {"precision": "highest"}
    plugin.uninstall()
    for bad in (lambda: plugin.install_transformer_ffn(precision="medium"),
                lambda: plugin.install(lazy=True, transformer_ffn=True, transformer_ffn_precision="fast"),
                lambda: plugin.install(lazy=True, transformer_ffn=True, window_attention=True, transformer_ffn_precision=3)):
        with pytest.raises(ValueError, match="'highest', 'high', 'torch'"):
            bad()
    assert _forward(standin) is original                        # nothing was patched, the attention functions neither
    assert all(getattr(getattr(standin, n), "replaced", None) is None for n in plugin.WINDOW_ATTENTION_NAMES)


def test_the_option_is_independent_of_the_window_attention_s_and_does_not_reach_the_decoder(standin):
    plugin.install(lazy=True, transformer_ffn=True, transformer_ffn_precision="torch", window_attention=True,
                   window_attention_precision="high", views_per_group=3)
    assert _forward(standin).precision == "torch" and getattr(standin, plugin.WINDOW_ATTENTION_FULL).precision == "high"
    assert plugin.TRANSFORMER_FFN_SEAM.options == {"precision": "torch"} and plugin.WINDOW_ATTENTION_SEAM.options == {"precision": "high"}
    assert plugin.DECODER_SEAM.options == {"views_per_group": 3}
    plugin.uninstall()
    plugin.install(lazy=True, window_attention=True, transformer_ffn=True, transformer_ffn_precision="high")
    assert _forward(standin).precision == "high" and getattr(standin, plugin.WINDOW_ATTENTION_FULL).precision == "highest"


def test_the_three_entry_points_are_declared_bound_and_sized():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in ("s360_ffn_tail_high_scratch_bytes", "s360_ffn_tail_high_forward", "s360_ffn_tail_high_backward"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 25 and "#define S360_ABI_VERSION 25" in (ROOT / "include" / "s360.h").read_text()
    lib = _lib.lib()
    # the planes are the same 3 MiB whatever T, forward and backward; "highest" has no forward scratch
    for tokens in (1, 129, 65669):
        assert tf.scratch_bytes(tokens, False) == 0 and tf.scratch_bytes(tokens, True) == lib.s360_ffn_tail_scratch_bytes(tokens) > 0
        for back in (False, True):
            assert tf.scratch_bytes(tokens, back, "high") - tf.scratch_bytes(tokens, back, "highest") == PLANE_BYTES == 3 << 20
            assert tf.scratch_bytes(tokens, back, "high") % 16 == 0
    for bad in (0, -1, -2 ** 31):
        assert lib.s360_ffn_tail_high_scratch_bytes(bad, 0) == 0 and lib.s360_ffn_tail_high_scratch_bytes(bad, 1) == 0
        assert tf.scratch_bytes(bad, True, "high") == 0
    # refusals that need no device memory: null tensors
    assert lib.s360_ffn_tail_high_forward(*(None,) * 8, 1, 128, 1024, None, None, None, None, None, 0, None) == -1
    assert lib.s360_ffn_tail_high_backward(*(None,) * 11, 1, 128, 1024, None, None, 0, *(None,) * 8, None) == -1
