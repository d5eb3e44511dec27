"""install(unet_attention=True) on stand-ins for the reference's unet module (tests/qkv_attention_reference.standin_modules),
without a GPU: the two forwards are rebound and restored, before and after the module's import, CPU and half-precision calls reach
the replaced methods and return their bits, and the seam composes with install(group_norm=True).  The GPU half of the seam is in
tests/test_gpu_qkv_attention.py."""
import inspect
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest
import torch

import group_norm_reference as G
import qkv_attention_reference as R
from splatter360_amd import plugin, qkv_attention as qa

ROOT = Path(__file__).resolve().parent.parent
MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)
CLASSES = ("QKVAttentionLegacy", "QKVAttention")


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


def forwards(unet):
    return {c: getattr(unet, c).__dict__.get("forward", getattr(getattr(unet, c), "forward")) for c in CLASSES}


def test_the_names_are_the_reference_s():
    assert plugin.UNET_ATTENTION_MODULE == "src.model.encoder.costvolume.ldm_unet.unet"
    assert [(s.cls_name, s.names) for s in plugin.UNET_ATTENTION_SEAMS] == [(c, ("forward",)) for c in CLASSES]
    assert all(isinstance(s, plugin._MethodSeam) and s.keyword == "unet_attention" for s in plugin.UNET_ATTENTION_SEAMS)
    assert plugin.OPTION_SEAMS["unet_attention"] == plugin.UNET_ATTENTION_SEAMS
    assert inspect.signature(plugin.install).parameters["unet_attention"].default is False


def test_install_rebinds_the_two_forwards_and_uninstall_restores_them(standin):
    originals = forwards(standin)
    assert plugin.install(lazy=True, unet_attention=True) is None                  # lazy: no decoder registry is imported here
    patched = forwards(standin)
    for name in CLASSES:
        assert patched[name] is not originals[name] and patched[name].replaced is originals[name], name
        assert inspect.signature(patched[name]).parameters.keys() == inspect.signature(originals[name]).parameters.keys(), name
    assert plugin.install_unet_attention() == {f"{c}.forward": patched[c] for c in CLASSES}      # idempotent: no second layer
    plugin.install(lazy=True, unet_attention=True)
    assert forwards(standin) == patched
    plugin.uninstall()
    assert forwards(standin) == originals


def test_install_without_the_keyword_leaves_the_module_alone(standin):
    originals = forwards(standin)
    plugin.install(lazy=True, group_norm=True)
    assert forwards(standin) == originals


def test_it_composes_with_group_norm(standin):
    originals = forwards(standin)
    block_forward = standin.AttentionBlock.__dict__.get("_forward", standin.AttentionBlock._forward)
    plugin.install(lazy=True, unet_attention=True, group_norm=True)
    patched = forwards(standin)
    assert all(patched[c].replaced is originals[c] for c in CLASSES)
    assert standin.AttentionBlock.__dict__["_forward"].replaced is block_forward and standin.ResBlock.__dict__["_forward"].replaced is not None
    # the group-norm wrapper of the block calls self.attention: the block's result on the CPU is the replaced methods' bits
    block = G.randomise(standin.AttentionBlock(64, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True), 3)
    x = torch.from_numpy(G.lattice((4, 64, 3, 5), 2, span=255))
    out = block(x)
    assert block.attention.calls == 1 and patched["QKVAttentionLegacy"].native_calls == 0
    plugin.uninstall()
    assert forwards(standin) == originals and torch.equal(block(x), out)


@pytest.mark.parametrize("dtype,device", [(torch.float32, "cpu"), (torch.float16, "cpu"), (torch.float64, "cpu")])
def test_cpu_and_half_precision_calls_reach_the_replaced_methods(standin, dtype, device, monkeypatch):
    monkeypatch.setattr(qa, "qkv_attention", lambda *a, **k: pytest.fail("the kernels were called"))
    legacy = standin.QKVAttentionLegacy(2, n_frames=3, use_cross_view_self_attn=True)
    new = standin.QKVAttention(2)
    qkv, _ = R.random_case(6, 2, 7, seed=4)
    qkv = qkv.to(dtype=dtype, device=device)
    before = (legacy(qkv), new(qkv))
    plugin.install_unet_attention()
    after = (legacy(qkv), new(qkv))
    assert all(torch.equal(x, y) and x.dtype == dtype for x, y in zip(before, after))
    assert legacy.calls == 2 and new.calls == 2
    assert all(f.native_calls == 0 for f in forwards(standin).values())


def test_the_wrapper_decides_on_device_dtype_and_shape_only():
    ok = torch.empty(4, 192, 5, device="meta")                                     # no data: the decision reads no element
    assert not plugin._unet_attention_call(ok, 2, 2)                               # not a CUDA tensor
    assert not plugin._unet_attention_call(torch.zeros(4, 192, 5), 2, 2)
    assert not plugin._unet_attention_call(torch.zeros(4, 192, 5, dtype=torch.float16), 2, 2)


def test_fallback_keeps_the_reference_s_own_errors(standin):
    plugin.install_unet_attention()
    with pytest.raises(AssertionError):                                            # 192 rows are no multiple of 3 x 5: the replaced method's assertion
        standin.QKVAttentionLegacy(5)(torch.zeros(2, 192, 4))


SCRIPT = textwrap.dedent("""
    import importlib, sys, types
    sys.path[:0] = [{root!r}, {tests!r}]
    import qkv_attention_reference as R
    from splatter360_amd import plugin

    MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)
    # before the module's import: pending hooks, placed when the module appears
    assert plugin.install_unet_attention() == {{"QKVAttentionLegacy.forward": None, "QKVAttention.forward": None}}
    hooks = [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher)]
    assert all(s in hooks for s in plugin.UNET_ATTENTION_SEAMS)
    mods = R.standin_modules(*MODULES)
    unet = mods[MODULES[0]]
    originals = {{c: getattr(unet, c).forward for c in ("QKVAttentionLegacy", "QKVAttention")}}
    sys.modules.update(mods)
    importlib.import_module("colorsys")                     # any import asks the pending hooks
    sys.modules.pop("colorsys", None)
    importlib.import_module("colorsys")
    for c, f in originals.items():
        assert getattr(unet, c).__dict__["forward"].replaced is f, c
    assert not any(isinstance(f, plugin._SeamPatcher) and f.seam in plugin.UNET_ATTENTION_SEAMS for f in sys.meta_path)
    plugin.uninstall()
    for c, f in originals.items():
        assert getattr(unet, c).forward is f, c
    # after the module's import: placed at once
    out = plugin.install_unet_attention()
    assert all(out[c + ".forward"].replaced is f for c, f in originals.items())
    plugin.install(lazy=True, unet_attention=True, group_norm=True)
    assert unet.AttentionBlock.__dict__["_forward"].replaced is not None
    assert all(getattr(unet, c).__dict__["forward"] is out[c + ".forward"] for c in originals)
    plugin.uninstall()
    assert all(getattr(unet, c).forward is f for c, f in originals.items())
    print("ok")
""")


def test_the_seam_is_placed_before_and_after_the_module_s_import():
    code = SCRIPT.format(root=str(ROOT), tests=str(ROOT / "tests"))
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
