"""`splatter360_amd.install(mono_fusion=True)`: EncoderCostVolume.__init__ rebound in the unchanged reference, on CPU, on the
stand-in encoder module of tests/mono_fusion_reference.py registered under the reference's module name.  On CPU tensors the wrapped
c2e runs its own forward, so the installed encoder returns the uninstalled bits; the handle's algebra (what stays lazy, what
materialises) is exercised directly on CPU handles.  The GPU half (the kernels behind the seam) is in tests/test_gpu_mono_fusion.py."""
import inspect
import sys

import einops
import pytest
import torch
from torch import nn

import mono_fusion_reference as R
import splatter360_amd
from splatter360_amd import mono_fusion as mf, plugin

NAME = plugin.MONO_FUSION_MODULE


@pytest.fixture
def module():
    """The stand-in under the reference's module name; every seam restored and the name released afterwards."""
    assert NAME not in sys.modules
    mod = R.standin_module(NAME)
    sys.modules[NAME] = mod
    try:
        yield mod
    finally:
        splatter360_amd.uninstall()
        sys.modules.pop(NAME, None)


def _init(mod):
    return mod.EncoderCostVolume.__dict__["__init__"]


def _inputs(seed=0, n=2, d=128, cm=64, geometry=(4, 8, 16)):
    fw, h, w = geometry
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, h, w, generator=gen), torch.randn(n, cm, fw, 6 * fw, generator=gen)


def test_names_are_the_references_and_the_keyword_defaults_to_false():
    assert (plugin.MONO_FUSION_MODULE, plugin.MONO_FUSION_CLASS, plugin.MONO_FUSION_METHOD) == \
        ("src.model.encoder.encoder_costvolume", "EncoderCostVolume", "__init__")
    assert (plugin.MONO_FUSION_MODULE, plugin.MONO_FUSION_CLASS) == (plugin.DEPTH_TAIL_MODULE, plugin.DEPTH_TAIL_CLASS)
    assert plugin.MONO_FUSION_NETS == ("rgbd_fusion", "c2e")
    p = inspect.signature(plugin.install).parameters["mono_fusion"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert plugin.OPTION_SEAMS["mono_fusion"] == (plugin.MONO_FUSION_SEAM,)


def test_install_rebinds_is_idempotent_and_uninstall_restores(module):
    original = _init(module)
    splatter360_amd.install(lazy=True, mono_fusion=True)
    bound = _init(module)
    assert bound is not original and bound.replaced is original
    assert plugin.install_mono_fusion() is bound
    splatter360_amd.install(lazy=True, mono_fusion=True)
    assert _init(module) is bound and bound.replaced is original                           # no wrapper around a wrapper
    enc = module.EncoderCostVolume()
    assert isinstance(enc.rgbd_fusion, mf.FusedMonoFusion) and enc.c2e.forward.replaced is not None
    splatter360_amd.uninstall()
    assert _init(module) is original
    plain = module.EncoderCostVolume()
    assert type(plain.rgbd_fusion) is nn.Sequential and getattr(plain.c2e.forward, "replaced", None) is None
    # an encoder without add_mono_feat has no rgbd_fusion: the hook leaves it alone
    splatter360_amd.install(lazy=True, mono_fusion=True)
    bare = module.EncoderCostVolume(add_mono_feat=False)
    assert not hasattr(bare, "rgbd_fusion") and getattr(bare.c2e.forward, "replaced", None) is None


@pytest.mark.parametrize("order", [("depth_tail", "mono_fusion"), ("mono_fusion", "depth_tail")])
def test_composes_with_depth_tail_on_the_same_class_in_either_order(module, order):
    cls = module.EncoderCostVolume
    init, opacity = cls.__dict__["__init__"], cls.__dict__["map_pdf_to_opacity"]
    for keyword in order:
        splatter360_amd.install(lazy=True, **{keyword: True})
    assert cls.__dict__["__init__"].replaced is init and cls.__dict__["map_pdf_to_opacity"].replaced is opacity
    enc = cls()
    assert isinstance(enc.rgbd_fusion, mf.FusedMonoFusion)
    splatter360_amd.uninstall()
    assert cls.__dict__["__init__"] is init and cls.__dict__["map_pdf_to_opacity"] is opacity


def test_state_dict_keys_and_values_are_unchanged(module):
    torch.manual_seed(3)
    plain = module.EncoderCostVolume()
    splatter360_amd.install(lazy=True, mono_fusion=True)
    torch.manual_seed(3)
    fused = module.EncoderCostVolume()
    a, b = plain.state_dict(), fused.state_dict()
    assert list(a) == list(b) == ["c2e.sample_grid", "rgbd_fusion.0.weight", "rgbd_fusion.1.weight", "rgbd_fusion.1.bias", "rgbd_fusion.3.weight"]
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert [k for k, _ in fused.rgbd_fusion.named_parameters()] == ["0.weight", "1.weight", "1.bias", "3.weight"]
    plain.load_state_dict(b)                                                                # both directions load strictly
    fused.load_state_dict(a)
    seq = nn.Sequential(nn.Linear(192, 128, bias=False), nn.LayerNorm(128), nn.ReLU(), nn.Linear(128, 128, bias=False))
    again = mf.FusedMonoFusion.from_sequential(seq)
    assert all(p is q for p, q in zip(seq.parameters(), again.parameters()))                # the same Parameter objects


def test_cpu_forward_through_the_installed_standin_returns_the_uninstalled_bits(module):
    torch.manual_seed(5)
    plain = module.EncoderCostVolume()
    splatter360_amd.install(lazy=True, mono_fusion=True)
    fused = module.EncoderCostVolume()
    fused.load_state_dict(plain.state_dict())
    feats, cube = _inputs()
    outs = []
    for enc in (plain, fused):
        x = feats.clone().requires_grad_(True)
        out = enc(x, cube)
        out.backward(torch.ones_like(out))
        outs.append((out.detach(), x.grad, [p.grad.clone() for p in enc.rgbd_fusion.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(p, q) for p, q in zip(outs[0][2], outs[1][2]))
    assert fused.c2e.calls == 1                                                             # the module's own forward ran
    # with grad enabled (the reference's two gradient-carrying c2e calls) and for other channel counts: the own forward as well
    assert not isinstance(fused.c2e(cube), mf.MonoStitchHandle)
    with torch.no_grad():
        assert not isinstance(fused.c2e(cube), mf.MonoStitchHandle)                         # a CPU tensor


def _handle(module, seed=0):
    enc = module.EncoderCostVolume()
    feats, cube = _inputs(seed)
    with torch.no_grad():
        want = enc.c2e(cube)
    return enc, feats, cube, want, mf.MonoStitchHandle(enc.c2e, cube)


def test_handle_survives_cat_and_rearrange_with_the_installed_einops(module):
    enc, feats, cube, want, h = _handle(module)
    calls = enc.c2e.calls
    assert tuple(h.shape) == tuple(want.shape) and h.dtype == torch.float32 and h.device == cube.device and h.dim() == 4
    assert not h.requires_grad and not h.fusable and "MonoStitchHandle" in repr(h)
    cat = torch.cat([feats, h], dim=1)
    assert isinstance(cat, mf.MonoStitchHandle) and tuple(cat.shape) == (2, 192, 8, 16) and not cat.fusable
    last = einops.rearrange(cat, "bv c h w -> bv h w c")
    assert isinstance(last, mf.MonoStitchHandle) and tuple(last.shape) == (2, 8, 16, 192) and last.fusable
    assert last._s360_erp is feats and last._s360_cube is cube
    assert last.reshape(2, 8, 16, 192) is last and last.view(last.shape) is last and last.permute(0, 1, 2, 3) is last
    assert last.size(-1) == 192 and last.numel() == 2 * 8 * 16 * 192
    assert enc.c2e.calls == calls                                                           # nothing was stitched
    real = last.materialise()
    assert type(real) is torch.Tensor and torch.equal(real, torch.cat([feats, want], dim=1).permute(0, 2, 3, 1))
    # FusedMonoFusion on a CPU handle: the real tensor through nn.Sequential.forward
    fusion = mf.FusedMonoFusion.from_sequential(enc.rgbd_fusion)
    assert torch.equal(fusion(last), enc.rgbd_fusion(real))


def test_any_other_operation_materialises_with_the_references_bits(module):
    enc, feats, cube, want, h = _handle(module, seed=1)
    for got, ref in ((h + 0, want + 0), (h[:, :3], want[:, :3]), (torch.cat([h, want], dim=0), torch.cat([want, want], dim=0)),
                     (torch.cat([want, h], dim=3), torch.cat([want, want], dim=3)),
                     (torch.cat([h, feats], dim=1), torch.cat([want, feats], dim=1)),
                     (torch.cat([feats, h], dim=1).permute(0, 3, 1, 2), torch.cat([feats, want], dim=1).permute(0, 3, 1, 2)),
                     (torch.cat([feats, h], dim=1) * 2, torch.cat([feats, want], dim=1) * 2),
                     (h.permute(0, 2, 3, 1), want.permute(0, 2, 3, 1)), (h.reshape(2, -1), want.reshape(2, -1)), (h.sum(), want.sum())):
        assert type(got) is torch.Tensor and torch.equal(got, ref)
    assert h.contiguous().is_contiguous() and torch.equal(h.contiguous(), want)
