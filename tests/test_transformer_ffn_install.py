"""install(transformer_ffn=True) on a stand-in for the reference's backbone module
(tests/transformer_ffn_reference.standin_module), without a GPU: TransformerLayer.forward is rebound and restored, before and after
the module's import, CPU calls and every form the wrapper does not recognise reach the replaced method and return its bits, and the
seam composes with install(window_attention=True) in both orders.  The GPU half of the seam is in
tests/test_gpu_transformer_ffn.py."""
import inspect
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest
import torch
from torch import nn

import transformer_ffn_reference as R
from splatter360_amd import plugin, transformer_ffn as tf

ROOT = Path(__file__).resolve().parent.parent
MODULE = plugin.TRANSFORMER_FFN_MODULE


@pytest.fixture
def standin():
    assert MODULE not in sys.modules
    mod = R.standin_module(MODULE)
    sys.modules[MODULE] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        del sys.modules[MODULE]


def bound(mod):
    return mod.TransformerLayer.__dict__.get("forward", mod.TransformerLayer.forward)


def test_the_names_are_the_reference_s():
    assert MODULE == "src.model.encoder.backbone.multiview_transformer" == plugin.WINDOW_ATTENTION_MODULE
    seam = plugin.TRANSFORMER_FFN_SEAM
    assert isinstance(seam, plugin._MethodSeam) and (seam.keyword, seam.cls_name, seam.names) == ("transformer_ffn", "TransformerLayer", ("forward",))
    assert plugin.OPTION_SEAMS["transformer_ffn"] == (seam,)
    assert inspect.signature(plugin.install).parameters["transformer_ffn"].default is False


def test_install_rebinds_forward_and_uninstall_restores_it(standin):
    original = bound(standin)
    assert plugin.install(lazy=True, transformer_ffn=True) is None                 # lazy: no decoder registry is imported here
    patched = bound(standin)
    assert patched is not original and patched.replaced is original and patched.native_calls == 0
    assert list(inspect.signature(patched).parameters) == list(inspect.signature(original).parameters)
    assert plugin.install_transformer_ffn() is patched                             # idempotent: no second layer
    plugin.install(lazy=True, transformer_ffn=True)
    assert bound(standin) is patched
    plugin.uninstall()
    assert bound(standin) is original


def test_install_without_the_keyword_leaves_the_method_alone(standin):
    original = bound(standin)
    plugin.install(lazy=True, window_attention=True)
    assert bound(standin) is original


@pytest.mark.parametrize("order", [("transformer_ffn", "window_attention"), ("window_attention", "transformer_ffn")])
def test_it_composes_with_window_attention_in_both_orders(standin, order):
    original = bound(standin)
    full = standin.single_head_full_attention
    for keyword in order:
        plugin.install(lazy=True, **{keyword: True})
    assert bound(standin).replaced is original and standin.single_head_full_attention.replaced is full
    # a CPU call: the wrapper hands it to the replaced method, which finds the window-attention wrapper in the module's globals,
    # which hands the CPU tensors to the stand-in's own function
    layer = R.randomise(standin.TransformerLayer(d_model=128), 2)
    source, target = torch.randn(2, 6, 128, generator=torch.Generator().manual_seed(1)).unbind(0)
    out = layer(source[None], target[None], attn_num_splits=1)
    assert layer.calls == 1 and standin.calls == [("full", None)] and bound(standin).native_calls == 0
    plugin.uninstall()
    assert bound(standin) is original and standin.single_head_full_attention is full
    assert torch.equal(layer(source[None], target[None], attn_num_splits=1), out)


def test_the_state_dict_keys_are_the_reference_s(standin):
    plugin.install_transformer_ffn()
    assert tuple(standin.TransformerLayer(d_model=128).state_dict()) == R.LAYER_PARAMS
    assert tuple(standin.TransformerLayer(d_model=128, no_ffn=True).state_dict()) == R.layer_params(True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("no_ffn", [False, True])
def test_cpu_calls_reach_the_replaced_method(standin, dtype, no_ffn, monkeypatch):
    for name in ("ffn_tail", "layer_norm_residual"):
        monkeypatch.setattr(tf, name, lambda *a, **k: pytest.fail("the kernels were called"))
    layer = R.randomise(standin.TransformerLayer(d_model=128, no_ffn=no_ffn), 3).to(dtype)
    source, target = torch.randn(2, 2, 5, 128, generator=torch.Generator().manual_seed(4)).to(dtype).unbind(0)
    before = layer(source, target, attn_num_splits=1)
    plugin.install_transformer_ffn()
    after = layer(source, target, attn_num_splits=1)
    assert torch.equal(before, after) and after.dtype == dtype and layer.calls == 2 and bound(standin).native_calls == 0


class _Fake:
    """What _transformer_ffn_call reads of a tensor: enough to show the decision without a GPU."""

    def __init__(self, shape=(2, 6, 128), cuda=True, dtype=torch.float32):
        self.shape, self.is_cuda, self.dtype, self.device = torch.Size(shape), cuda, dtype, torch.device("cuda:0" if cuda else "cpu")

    def dim(self):
        return len(self.shape)

    def numel(self):
        return self.shape.numel()


def test_the_fall_through_conditions(standin, monkeypatch):
    """The decision reads attributes, devices, dtypes and shapes only; a float32 GPU call of a plain single-head layer is taken,
    each condition of the list is not."""
    monkeypatch.setattr(plugin, "_is_cuda_f32", lambda t: isinstance(t, _Fake) and t.is_cuda and t.dtype == torch.float32)
    make = standin.TransformerLayer
    ok, x = make(d_model=128), _Fake()
    take = plugin._transformer_ffn_call
    assert take(ok, x, x, {}) and take(make(d_model=128, no_ffn=True), x, x, {})
    assert take(ok, x, _Fake((2, 3, 6, 128)), {})                                   # a [B, N - 1, L, C] target
    assert not take(make(d_model=128, nhead=2), x, x, {})
    assert not take(make(d_model=128, add_per_view_attn=True), x, x, {})
    assert not take(ok, x, x, {"attn_type": "epipolar_full_attn"})
    assert not take(ok, _Fake(cuda=False), x, {}) and not take(ok, x, _Fake(cuda=False), {})
    assert not take(ok, _Fake(dtype=torch.float16), x, {})
    assert not take(make(d_model=64), _Fake((2, 6, 64)), _Fake((2, 6, 64)), {})
    assert not take(ok, _Fake((2, 6, 64)), x, {})                                   # a width that is not the layer's
    assert not take(ok, _Fake((6, 128)), x, {})
    assert not take(make(d_model=128, ffn_dim_expansion=2), x, x, {})               # hidden width 512
    for spoil in ("bias", "tanh", "relu", "four", "norm1", "norm2", "eps"):
        layer = make(d_model=128)
        if spoil == "bias":
            layer.mlp[0] = nn.Linear(256, 1024, bias=True)
        elif spoil == "tanh":
            layer.mlp[1] = nn.GELU(approximate="tanh")
        elif spoil == "relu":
            layer.mlp[1] = nn.ReLU()
        elif spoil == "four":
            layer.mlp.append(nn.Identity())
        elif spoil == "norm1":
            layer.norm1 = nn.LayerNorm(128, elementwise_affine=False)
        elif spoil == "norm2":
            layer.norm2 = nn.LayerNorm(128, elementwise_affine=False)
        else:
            layer.norm2 = nn.LayerNorm(128, eps=1e-6)
        assert not take(layer, x, x, {}), spoil
    no_affine = make(d_model=128, no_ffn=True)
    no_affine.norm1 = nn.LayerNorm(128, elementwise_affine=False)
    assert not take(no_affine, x, x, {})


def test_a_refused_call_keeps_the_reference_s_keywords(standin):
    """attn_type and any further keyword reach the replaced method as they came."""
    seen = {}
    original = bound(standin)

    def spy(self, source, target, **kwargs):
        seen.update(kwargs)
        return original(self, source, target, **kwargs)

    standin.TransformerLayer.forward = spy
    plugin.install_transformer_ffn()
    layer = standin.TransformerLayer(d_model=128)
    x = torch.zeros(1, 4, 128)
    layer(x, x, height=2, width=2, attn_num_splits=1, attn_type="full", extra=3)
    assert seen == dict(height=2, width=2, shifted_window_attn_mask=None, attn_num_splits=1, attn_type="full", extra=3)
    plugin.uninstall()
    assert bound(standin) is spy


SCRIPT = textwrap.dedent("""
    import importlib, sys
    sys.path[:0] = [{root!r}, {tests!r}]
    import transformer_ffn_reference as R
    from splatter360_amd import plugin

    MODULE = plugin.TRANSFORMER_FFN_MODULE
    # before the module's import: a pending hook, placed when the module appears
    assert plugin.install_transformer_ffn() is None
    assert any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.TRANSFORMER_FFN_SEAM for f in sys.meta_path)
    mod = R.standin_module(MODULE)
    original = mod.TransformerLayer.forward
    sys.modules[MODULE] = mod
    importlib.import_module("colorsys")                     # any import asks the pending hooks
    sys.modules.pop("colorsys", None)
    importlib.import_module("colorsys")
    assert mod.TransformerLayer.__dict__["forward"].replaced is original
    assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.TRANSFORMER_FFN_SEAM for f in sys.meta_path)
    plugin.uninstall()
    assert mod.TransformerLayer.forward is original
    # after the module's import: placed at once
    assert plugin.install_transformer_ffn().replaced is original
    plugin.uninstall()
    assert mod.TransformerLayer.forward is original
    print("ok")
""")


def test_the_seam_is_placed_before_and_after_the_module_s_import():
    code = SCRIPT.format(root=str(ROOT), tests=str(ROOT / "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
