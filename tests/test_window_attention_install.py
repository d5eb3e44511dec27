"""install(window_attention=True) on a stand-in for the reference's backbone module (tests/window_attention_reference.standin_module),
without a GPU: the names are rebound and restored, CPU and float64 calls run the replaced functions and return their bits, and a
ShiftMask handle never reaches torch code.  The GPU half of the seam is in tests/test_gpu_window_attention.py."""
import inspect
import sys

import pytest
import torch

import window_attention_reference as R
from splatter360_amd import plugin, window_attention as wa

REBOUND = (plugin.WINDOW_ATTENTION_SPLIT, plugin.WINDOW_ATTENTION_FULL, plugin.WINDOW_ATTENTION_MASK)


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


def test_the_names_are_the_reference_s():
    assert plugin.WINDOW_ATTENTION_MODULE == "src.model.encoder.backbone.multiview_transformer"
    assert REBOUND == ("single_head_split_window_attention", "single_head_full_attention", "generate_shift_window_attn_mask")
    assert plugin.WINDOW_ATTENTION_MULTI == "multi_head_split_window_attention"
    assert inspect.signature(plugin.install).parameters["window_attention"].default is False


def test_install_rebinds_the_names_and_uninstall_restores_them(standin):
    mod = standin
    originals = {n: getattr(mod, n) for n in plugin.WINDOW_ATTENTION_NAMES}
    assert plugin.install(lazy=True, window_attention=True) is None                # lazy: no decoder registry is imported here
    for n in plugin.WINDOW_ATTENTION_NAMES:
        assert getattr(mod, n) is not originals[n] and getattr(mod, n).replaced is originals[n], n
        assert inspect.signature(getattr(mod, n)).parameters.keys() == inspect.signature(originals[n]).parameters.keys(), n
    patched = {n: getattr(mod, n) for n in plugin.WINDOW_ATTENTION_NAMES}
    assert plugin.install_window_attention() == patched                            # idempotent: no second layer
    plugin.install(lazy=True, window_attention=True)
    assert all(getattr(mod, n) is patched[n] for n in patched)
    plugin.uninstall()
    assert all(getattr(mod, n) is originals[n] for n in originals)


def test_install_without_the_keyword_leaves_the_module_alone(standin):
    originals = {n: getattr(standin, n) for n in plugin.WINDOW_ATTENTION_NAMES}
    plugin.install(lazy=True, depth_head=True)
    assert all(getattr(standin, n) is originals[n] for n in originals)


@pytest.mark.parametrize("m", [0, 1, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_cpu_and_float64_calls_fall_back_and_the_fallback_sees_a_dense_mask(standin, m, dtype):
    mod = standin
    h, w, k = 4, 8, 2
    q, kk, v, _ = (t.to(dtype) for t in R.random_case(2, m, h, w, c=32, seed=4 + m))
    before = [mod.layer(q, kk, v, h, w, k, shift) for shift in (False, True)]
    before_multi = mod.layer(q, kk, v, h, w, k, True, multi_head=True) if m == 0 else None
    before_full = mod.layer(q, kk, v, h, w, 1, False) if m == 0 else None
    plugin.install_window_attention()
    handle = mod.generate_shift_window_attn_mask((h, w), h // k, w // k, h // k // 2, w // k // 2, device=q.device)
    assert isinstance(handle, wa.ShiftMask) and handle.matches(h, w, k) and handle.device == q.device
    assert torch.equal(handle.dense(), R.dense_mask(h, w, k))
    mod.calls.clear()
    after = [mod.layer(q, kk, v, h, w, k, shift) for shift in (False, True)]
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert [c[0] for c in mod.calls] == ["single", "single"]                       # the replaced function ran, once per call
    assert all(isinstance(c[1], torch.Tensor) and not isinstance(c[1], wa.ShiftMask) for c in mod.calls)
    if m == 0:
        mod.calls.clear()
        assert torch.equal(mod.layer(q, kk, v, h, w, k, True, multi_head=True), before_multi)
        assert torch.equal(mod.layer(q, kk, v, h, w, 1, False), before_full)
        assert [c[0] for c in mod.calls] == ["multi", "full"] and isinstance(mod.calls[0][1], torch.Tensor)


def test_fallback_keeps_autograd_and_the_reference_s_own_errors(standin):
    mod = standin
    plugin.install_window_attention()
    q, kk, v, g = R.random_case(1, 0, 4, 4, c=32, seed=9)
    q.requires_grad_(True)
    out = mod.layer(q, kk, v, 4, 4, 2, True)
    out.backward(g)
    assert torch.isfinite(q.grad).all() and q.grad.abs().max().item() > 0
    with pytest.raises(AssertionError):                                             # with_shift without a mask: the replaced function's assertion
        mod.single_head_split_window_attention(q.detach(), kk, v, num_splits=2, with_shift=True, h=4, w=4, attn_mask=None)
    # a dense mask given by the caller is handed on as it is
    mask = R.dense_mask(4, 4, 2)
    mod.calls.clear()
    mod.single_head_split_window_attention(q.detach(), kk, v, num_splits=2, with_shift=True, h=4, w=4, attn_mask=mask)
    assert mod.calls[0][1] is mask


def test_install_before_the_module_is_imported_uses_the_import_hook():
    assert plugin.WINDOW_ATTENTION_MODULE not in sys.modules
    try:
        assert plugin.install_window_attention() is None
        hooks = [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher)]
        assert plugin.WINDOW_ATTENTION_SEAM in hooks
    finally:
        plugin.uninstall()
    assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
