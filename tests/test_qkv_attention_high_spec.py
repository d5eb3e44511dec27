"""The specification of the QKV attention's "high" precision mode, on the CPU: that the accuracy bound of
tests/test_gpu_qkv_attention_high.py tells a three-term product from a single bf16 product, the argument errors, the install
option and the three C entry points.

Discrimination, measured on one CPU over the 11 shapes x 2 scales x 5 tensors below (the GPU test's cases and seeds; the bound
max(1.5 x (e3 + e32), 2^-24 max|want|) with e32 from the float32 lines on the CPU): the terms=1 statement's error against
statement(float64) is at least 13.8 x the bound in the maximum and 19.9 x in the mean (g_q of `tiny` at scale 6, where every row's
weight sits on one key; g_qkv and g_k of that case 15.4 x / 34.0 x and 23.8 x / 25.5 x); in every other case at least 133 x (out of
`uneven` at scale 1) and 225 x (g_k of `views3` at scale 6).  The test asks for 5 x.  The seeds are the rule of
tests/test_gpu_qkv_attention.py, 2000 + 7 x the name's place in sorted order, over the eleven names.
"""
import re
import sys
from pathlib import Path

import pytest
import torch

import qkv_attention_high_reference as H
import qkv_attention_reference as R
from splatter360_amd import _lib, plugin, qkv_attention as qa

ROOT = Path(__file__).resolve().parent.parent
MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)
ENTRIES = ("s360_qkv_attention_high_scratch_bytes", "s360_qkv_attention_high_forward", "s360_qkv_attention_high_backward")


@pytest.mark.parametrize("scale", H.SCALES)
@pytest.mark.parametrize("name", sorted(H.SHAPES))
def test_a_single_bf16_product_is_five_times_beyond_the_gpu_rule_s_bound(name, scale):
    n, views, cross, heads, t, order = H.SHAPES[name]
    (qkv, g), want, three, lines = H.yardsticks(name, scale)
    one = H.with_parts(name, R.gradients(lambda x: H.split_statement(x, heads, views, cross, order, terms=1), qkv, g, torch.float64))
    failures = []
    for nm, w64, t3, l32, t1 in zip(H.NAMES, want, three, lines, one):
        assert t1.dtype == torch.float64 and t1.shape == w64.shape
        (max1, mean1), (bmax, bmean) = H.errors(t1, w64), H.bound(w64, t3, l32)
        print(f"{name} scale={scale:g} {nm}: terms=1 max {max1:.3e} mean {mean1:.3e} | bound max {bmax:.3e} mean {bmean:.3e}"
              f" | ratios {max1 / bmax:.1f} {mean1 / bmean:.1f}")
        if not (bmax > 0.0 and max1 >= 5.0 * bmax and mean1 >= 5.0 * bmean):
            failures.append((nm, max1, mean1, bmax, bmean))
    assert not failures, (name, scale, failures)


def test_three_terms_are_the_statement_up_to_the_split():
    """terms=3 at `straddle`: within 2^-12 of the float64 statement relative to the largest value — the split's 2^-16 per product
    through a softmax at unit scale — and not equal to it."""
    _, want, three, _ = H.yardsticks("straddle", 1.0)
    for w64, t3 in zip(want, three):
        e = H.errors(t3, w64)[0]
        assert 0.0 < e <= 2.0 ** -12 * w64.abs().max().item()


def test_an_unknown_precision_is_refused_before_any_launch(monkeypatch):
    qkv, g = R.random_case(2, 2, 8, seed=1)
    monkeypatch.setattr(qa._lib, "lib", lambda: pytest.fail("a launch was reached"))
    for call in (lambda: qa.qkv_attention(qkv, 2, precision="bogus"), lambda: qa.attention_forward(qkv, 2, precision="bogus"),
                 lambda: qa.attention_backward(qkv, None, g, 2, precision="bogus"),
                 lambda: qa.qkv_attention(None, 2, precision="medium")):
        with pytest.raises(ValueError, match=r"'highest', 'high'"):
            call()
    assert qa.PRECISIONS == ("highest", "high")
    for good in qa.PRECISIONS:                                  # a known precision goes on to the device check (no CPU path)
        with pytest.raises(ValueError, match="GPU tensor"):
            qa.qkv_attention(qkv, 2, precision=good)


@pytest.fixture
def standin():
    assert not any(m in sys.modules for m in MODULES)
    mods = R.standin_modules(*MODULES)
    sys.modules.update(mods)
    try:
        yield mods[MODULES[0]]
    finally:
        plugin.uninstall()
        for m in MODULES:
            del sys.modules[m]


def _recorded(monkeypatch):
    """qa.qkv_attention replaced by a recorder of its keywords that returns the float32 lines."""
    seen = []

    def record(qkv, n_heads, **kw):
        seen.append(kw)
        return R.reference_lines(qkv, n_heads, kw["n_frames"], kw["cross_view"], kw["order"])

    monkeypatch.setattr(qa, "qkv_attention", record)
    monkeypatch.setattr(plugin, "_unet_attention_call", lambda qkv, heads, views: True)     # CPU tensors reach the wrapper's call
    return seen


def test_the_seam_resolves_torch_at_every_call(standin, monkeypatch):
    unet = standin
    originals = {c: getattr(unet, c).forward for c in (plugin.UNET_ATTENTION_LEGACY, plugin.UNET_ATTENTION_NEW)}
    seen = _recorded(monkeypatch)
    plugin.install(lazy=True, unet_attention=True, unet_attention_precision="torch")
    assert all(seam.options == {"precision": "torch"} for seam in plugin.UNET_ATTENTION_SEAMS)
    legacy, new = unet.QKVAttentionLegacy(2, n_frames=2, use_cross_view_self_attn=True), unet.QKVAttention(2)
    wrappers = [getattr(unet, c).__dict__["forward"] for c in originals]
    assert all(w.precision == "torch" and w.replaced is originals[c] and w.native_calls == 0 for w, c in zip(wrappers, originals))
    qkv, _ = R.random_case(2, 2, 8, seed=1)
    before = torch.get_float32_matmul_precision()
    try:
        for setting, want in (("high", "high"), ("highest", "highest"), ("medium", "high")):
            torch.set_float32_matmul_precision(setting)
            del seen[:]
            out = legacy(qkv)
            new(qkv)
            assert [kw["precision"] for kw in seen] == [want, want], setting
            assert seen[0]["order"] == "legacy" and seen[0]["cross_view"] is True and seen[0]["n_frames"] == 2
            assert seen[1]["order"] == "new" and seen[1]["cross_view"] is False
            assert torch.equal(out, R.reference_lines(qkv, 2, 2, True, "legacy"))
    finally:
        torch.set_float32_matmul_precision(before)
    assert [w.native_calls for w in wrappers] == [3, 3] and legacy.calls == 0 and new.calls == 0
    plugin.uninstall()
    assert all(getattr(unet, c).forward is originals[c] for c in originals)


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_a_fixed_option_is_passed_whatever_torch_says_and_a_second_install_replaces_it(standin, monkeypatch, precision):
    unet = standin
    seen = _recorded(monkeypatch)
    bound = plugin.install_unet_attention(precision=precision)
    assert set(bound) == {"QKVAttentionLegacy.forward", "QKVAttention.forward"} and all(w.precision == precision for w in bound.values())
    att = unet.QKVAttention(2)
    qkv, _ = R.random_case(2, 2, 8, seed=1)
    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high" if precision == "highest" else "highest")
        att(qkv)
    finally:
        torch.set_float32_matmul_precision(before)
    other = "high" if precision == "highest" else "highest"
    plugin.install(lazy=True, unet_attention=True, unet_attention_precision=other)
    wrapper = unet.QKVAttention.__dict__["forward"]
    assert wrapper.precision == other and getattr(wrapper.replaced, "replaced", None) is None      # replaced, not stacked
    att(qkv)
    assert [kw["precision"] for kw in seen] == [precision, other]


def test_the_default_install_is_highest_and_an_unknown_option_is_refused(standin):
    unet = standin
    originals = {c: getattr(unet, c).forward for c in (plugin.UNET_ATTENTION_LEGACY, plugin.UNET_ATTENTION_NEW)}
    assert all(w.precision == "highest" for w in plugin.install_unet_attention().values())
    plugin.uninstall()
    plugin.install(lazy=True, unet_attention=True)
    assert unet.QKVAttentionLegacy.__dict__["forward"].precision == "highest"
    plugin.uninstall()
    for bad in (lambda: plugin.install_unet_attention(precision="medium"),
                lambda: plugin.install(lazy=True, unet_attention=True, unet_attention_precision="bogus")):
        with pytest.raises(ValueError, match="'highest', 'high', 'torch'"):
            bad()
    assert all(getattr(unet, c).forward is originals[c] for c in originals)
    # CPU tensors still reach the replaced methods, whatever the precision
    plugin.install(lazy=True, unet_attention=True, unet_attention_precision="high")
    att = unet.QKVAttention(2)
    qkv, _ = R.random_case(2, 2, 8, seed=1)
    assert torch.equal(att(qkv), R.reference_lines(qkv, 2, 1, False, "new")) and att.calls == 1
    assert unet.QKVAttention.__dict__["forward"].native_calls == 0


def test_the_three_entry_points_are_declared_bound_and_sized():
    text = (ROOT / "include" / "s360.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 25 and "#define S360_ABI_VERSION 25" in text
    lib = _lib.lib()
    # host arithmetic: hi + lo are 4 bytes an element, L is rounded up to a multiple of 32; a forward holds three planes of
    # [B, heads, Lpad, 32] pairs (the padded qkv's bytes), a backward seven (1.75 x the padded qkv and g_out)
    for name, (n, views, cross, heads, t, order) in H.SHAPES.items():
        nv = views if cross else 1
        lpad = -(-nv * t // 32) * 32
        plane = 4 * (n // nv) * heads * lpad * 32
        assert qa.scratch_bytes(n, nv, heads, t, False) == 3 * plane, name
        assert qa.scratch_bytes(n, nv, heads, t, True) == 7 * plane, name
    for bad in ((0, 1, 1, 32, 8), (2, 1, 1, 16, 8), (3, 2, 1, 32, 8), (2, 1, 0, 32, 8), (2, 1, 1, 32, 0)):
        assert lib.s360_qkv_attention_high_scratch_bytes(*bad, 0) == 0
    # refusals that need no device memory: a null tensor, then a null scratch behind a valid-looking (never read) address
    assert lib.s360_qkv_attention_high_forward(None, 2, 1, 1, 32, 8, 0, None, None, None, 0, None) == -1
    assert lib.s360_qkv_attention_high_backward(None, None, None, 2, 1, 1, 32, 8, 0, None, None, None, 0, None) == -1
    assert lib.s360_qkv_attention_high_forward(16, 2, 1, 1, 32, 8, 0, 32, 48, None, 1 << 20, None) == -1
    assert lib.s360_qkv_attention_high_forward(16, 2, 1, 1, 16, 8, 0, 32, 48, 64, 1 << 20, None) == -4         # ch = 16: unsupported
