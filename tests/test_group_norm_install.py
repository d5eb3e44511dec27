"""install(group_norm=True) on stand-ins for the reference's three modules (tests/group_norm_reference.standin_modules), without a
GPU: the four methods are rebound and restored, unrecognised forms reach the replaced methods, and on the CPU the wrapped
forwards reproduce the recorded blocks through the fallback.  The GPU half of the seam is in tests/test_gpu_group_norm.py."""
import inspect
import sys

import numpy as np
import pytest
import torch
from torch import nn

import group_norm_reference as R
from splatter360_amd import group_norm as gn, plugin
from test_group_norm_spec import BLOCK_SEEDS, recorded

MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)
METHODS = (("ResBlock", "_forward", 0), ("AttentionBlock", "_forward", 0), ("DepthPredictorMultiView360", "__init__", 1), ("ResidualBlock", "forward", 2))


@pytest.fixture
def standin():
    assert not any(m in sys.modules for m in MODULES)
    mods = R.standin_modules(*MODULES)
    sys.modules.update(mods)
    try:
        yield [mods[m] for m in MODULES]
    finally:
        plugin.uninstall()
        for m in MODULES:
            del sys.modules[m]


def methods(mods):
    return {f"{c}.{m}": getattr(mods[i], c).__dict__.get(m, getattr(getattr(mods[i], c), m)) for c, m, i in METHODS}


def test_the_names_are_the_reference_s():
    assert plugin.GROUP_NORM_UNET_MODULE == "src.model.encoder.costvolume.ldm_unet.unet"
    assert plugin.COST_VOLUME_MODULE == "src.model.encoder.costvolume.depth_predictor_multiview_360"
    assert plugin.GROUP_NORM_BACKBONE_MODULE == "src.model.encoder.backbone.unimatch.backbone"
    assert [(s.cls_name, s.names) for s in plugin.GROUP_NORM_SEAMS] == [(c, (m,)) for c, m, _ in METHODS]
    assert all(isinstance(s, plugin._MethodSeam) for s in plugin.GROUP_NORM_SEAMS)
    assert plugin.GROUP_NORM_PREDICTOR_NETS == ("corr_refine_net", "refine_unet")
    assert inspect.signature(plugin.install).parameters["group_norm"].default is False


def test_install_rebinds_the_four_methods_and_uninstall_restores_them(standin):
    originals = methods(standin)
    assert plugin.install(lazy=True, group_norm=True) is None                       # lazy: no decoder registry is imported here
    patched = methods(standin)
    for name in originals:
        assert patched[name] is not originals[name] and patched[name].replaced is originals[name], name
    assert plugin.install_group_norm() == patched                                   # idempotent: no second layer
    plugin.install(lazy=True, group_norm=True)
    assert methods(standin) == patched
    plugin.uninstall()
    assert methods(standin) == originals


def test_install_without_the_keyword_leaves_the_modules_alone(standin):
    originals = methods(standin)
    plugin.install(lazy=True, depth_head=True)
    assert methods(standin) == originals


def test_unrecognised_forms_reach_the_replaced_methods(standin, monkeypatch):
    unet, _, backbone = standin
    seen = []
    for cls, name in ((unet.ResBlock, "_forward"), (unet.AttentionBlock, "_forward"), (backbone.ResidualBlock, "forward")):
        def spy(self, *a, _inner=getattr(cls, name), _cls=cls.__name__, **k):
            seen.append(_cls)
            return _inner(self, *a, **k)
        monkeypatch.setattr(cls, name, spy)                                         # what install will find and keep as .replaced
    x = torch.from_numpy(R.lattice((2, 16, 4, 6), 1, span=255))
    blocks = [R.randomise(unet.ResBlock(16, 16, postnorm=False), 1), R.randomise(unet.ResBlock(16, 16, up=True), 2),
              R.randomise(unet.ResBlock(16, 16, down=True), 3), R.randomise(unet.AttentionBlock(16, num_head_channels=16, postnorm=False), 4),
              R.randomise(backbone.ResidualBlock(16, 16, norm_layer=lambda c: nn.InstanceNorm2d(c, affine=True)), 5),
              R.randomise(backbone.ResidualBlock(16, 16, norm_layer=nn.BatchNorm2d), 6).eval()]
    before = [b(x) for b in blocks]
    seen.clear()
    plugin.install_group_norm()
    assert unet.ResBlock.__dict__["_forward"].replaced.__name__ == "spy"
    after = [b(x) for b in blocks]
    assert all(torch.equal(p, q) for p, q in zip(before, after))
    assert seen == ["ResBlock"] * 3 + ["AttentionBlock"] + ["ResidualBlock"] * 2    # prenorm, up, down; prenorm; affine, BatchNorm
    seen.clear()
    R.randomise(unet.ResBlock(16, 16), 7)(x)                                        # the recognised form does not
    assert seen == []


@pytest.mark.parametrize("case", sorted(BLOCK_SEEDS))
def test_wrapped_forwards_reproduce_the_recorded_blocks_on_the_cpu(standin, case, monkeypatch):
    unet, _, backbone = standin
    g = recorded(case)
    seed = BLOCK_SEEDS[case]
    module = {"resblock_same": lambda: unet.ResBlock(32, 32), "resblock_proj": lambda: unet.ResBlock(64, 32),
              "attention": lambda: unet.AttentionBlock(32, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True),
              "residual": lambda: backbone.ResidualBlock(64, 96, stride=2)}[case]()
    R.randomise(module, seed)
    x = torch.from_numpy(g["x"])
    before = module(x)
    plugin.install_group_norm()
    kernel_calls = []
    monkeypatch.setattr(gn, "group_norm_act", lambda *a, **k: kernel_calls.append(1))
    xin = x.clone().requires_grad_(True)
    after = module(xin)
    assert type(module).__dict__["forward" if case == "residual" else "_forward"].replaced is not None
    assert torch.equal(after, before) and not kernel_calls                          # the fallback: torch's own bits, no kernel on the CPU
    after.backward(torch.from_numpy(g["g"]))
    tol = 64 * 2.0 ** -24
    assert np.abs(after.detach().numpy() - g["out64"]).max() <= tol * np.abs(g["out64"]).max()
    assert np.abs(xin.grad.numpy() - g["gx64"]).max() <= tol * np.abs(g["gx64"]).max()


def test_the_predictor_s_constructor_fuses_its_two_heads(standin):
    _, predictor, _ = standin
    plain = predictor.DepthPredictorMultiView360(16)
    plugin.install_group_norm()
    fused, bare = predictor.DepthPredictorMultiView360(16), predictor.DepthPredictorMultiView360(channels=16, bare=True)
    assert list(fused.state_dict()) == list(plain.state_dict())
    for net, act in ((fused.corr_refine_net, "gelu"), (fused.refine_unet, "gelu")):
        assert isinstance(net[1], gn.FusedGroupNormAct) and net[1].activation == act and isinstance(net[2], nn.Identity)
        assert isinstance(net[3][0].in_layers[1], gn.FusedGroupNormAct) and net[3][0].in_layers[1].activation == "silu"
    assert isinstance(bare.refine_unet, nn.Conv2d) and isinstance(bare.corr_refine_net[1], gn.FusedGroupNormAct)
    fused.load_state_dict(plain.state_dict())                                        # a checkpoint of the unfused module loads
    x = torch.randn(2, 5, 4, 6)
    assert torch.equal(fused.refine_unet(x), plain.refine_unet(x)) and torch.equal(fused.corr_refine_net(x), plain.corr_refine_net(x))
    # a fused ResBlock is still recognised by the ResBlock seam (the residual goes into the second norm's call)
    assert plugin._norm_pair(fused.refine_unet[3][0].in_layers) is not None and plugin._norm_pair(plain.refine_unet[3][0].in_layers) is not None
    plugin.uninstall()
    assert not isinstance(predictor.DepthPredictorMultiView360(16).refine_unet[1], gn.FusedGroupNormAct)


def test_install_before_the_modules_are_imported_uses_the_import_hook():
    assert not any(m in sys.modules for m in MODULES)
    try:
        assert plugin.install_group_norm() == {f"{c}.{m}": None for c, m, _ in METHODS}
        hooks = [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher)]
        assert all(s in hooks for s in plugin.GROUP_NORM_SEAMS)
        mods = R.standin_modules(*MODULES)
        originals = {m: methods([mods[n] for n in MODULES]) for m in ("before",)}["before"]
        sys.modules.update(mods)
        try:
            import json  # noqa: F401  (any import asks the pending hooks, which find the modules imported behind their back)
            import importlib
            importlib.import_module("colorsys")
            sys.modules.pop("colorsys", None)
            importlib.import_module("colorsys")
            patched = methods([mods[n] for n in MODULES])
            assert all(patched[k].replaced is originals[k] for k in originals)
        finally:
            plugin.uninstall()
            for m in MODULES:
                del sys.modules[m]
    finally:
        plugin.uninstall()
    assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
