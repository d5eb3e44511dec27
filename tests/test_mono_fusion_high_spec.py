"""The specification of the mono-feature fusion's "high" precision mode, on the CPU: what the three-term product buys over a
single bf16 product (the condition that gives the accuracy bound of tests/test_gpu_mono_fusion_high.py its meaning), the argument
errors, the three C entry points, the install option and the launch geometry.

Discrimination, measured on one CPU over RUNS (out and five gradients each): the terms=1 statement's error against
statement(float64) is at least 397 x (max) and 521 x (mean) the terms=3 statement's; the test asks for 50 x, the window
attention's figure.  The single-bf16 statement also takes 2 to 11 ReLU decisions of the random cases the other way; the three-term
statement takes none.
"""
import functools
import re
import sys
from pathlib import Path

import pytest
import torch

import mono_fusion_high_reference as HR
import mono_fusion_reference as R
from splatter360_amd import _lib, mono_fusion as mf, plugin, precision

ROOT = Path(__file__).resolve().parent.parent
# (N, geometry, Cm, kind, seed): the shapes of tests/test_gpu_mono_fusion.py's cases, the seeds of the "high" GPU file
SHAPES = [(1, "g0", 64, "random", 101), (1, "g1", 64, "random", 111), (3, "g2", 192, "random", 108), (1, "g1", 384, "random", 100),
          (1, "g0", 1024, "random", 101), (2, "g3", 64, "decided", 200)]
RUNS = [(*shape, scale) for shape in SHAPES for scale in (1.0, 6.0)]


@functools.lru_cache(maxsize=None)
def _statements(n, geometry, cm, kind, seed, scale):
    make = R.decided_case if kind == "decided" else R.random_case
    tensors, g = make(n, geometry, cm, scale=scale, seed=seed)
    m = R.stitch32(tensors[1], tensors[2])
    want = R.gradients(lambda *t: R.statement(*t, m=m), tensors, g, torch.float64)
    three, one = (R.gradients(lambda *t: HR.split_statement(*t, terms=terms, m=m), tensors, g, torch.float64) for terms in (3, 1))
    return (tensors, m), want, three, one


@pytest.mark.parametrize("n,geometry,cm,kind,seed,scale", RUNS)
def test_three_terms_are_fifty_times_closer_than_one(n, geometry, cm, kind, seed, scale):
    (tensors, m), want, three, one = _statements(n, geometry, cm, kind, seed, scale)
    for name, w64, t3, t1 in zip(R.RESULTS, want, three, one):
        assert t3.dtype == torch.float64 and t3.shape == w64.shape
        (max3, mean3), (max1, mean1) = HR.errors(t3, w64), HR.errors(t1, w64)
        print(f"{geometry}/{cm} {kind} scale={scale:g} {name}: terms=1 max {max1:.3e} mean {mean1:.3e} | terms=3 max {max3:.3e} mean "
              f"{mean3:.3e} | ratios {max1 / max3:.0f} {mean1 / mean3:.0f}")
        assert max3 > 0.0 and max1 >= 50.0 * max3 and mean1 >= 50.0 * mean3, (geometry, cm, scale, name)
    flips3, flips1 = HR.flipped_decisions(tensors, m), HR.flipped_decisions(tensors, m, terms=1)
    print(f"{geometry}/{cm} {kind} scale={scale:g}: ReLU decisions taken the other way: terms=3 {flips3}, terms=1 {flips1}")
    assert flips3 == 0
    assert flips1 == 0 if kind == "decided" else flips1 >= 1


def test_the_split_statement_is_the_statement_but_for_its_products():
    """With operands of the first product that a single bf16 holds exactly, Ah Bh alone is the product: LayerNorm's output of the
    terms=1 statement is the float64 statement's, to the order of the sums."""
    tensors, _ = R.random_case(1, "g0", 64, seed=7)
    tensors = tuple(t.to(torch.bfloat16).to(torch.float32) if i in (0, 3) else t for i, t in enumerate(tensors))
    m = R.stitch32(tensors[1], tensors[2]).to(torch.bfloat16).to(torch.float32)
    parts1, parts64 = {}, {}
    out = HR.split_statement(*tensors, terms=1, m=m, parts=parts1)
    R.statement(*tensors, m=m, parts=parts64)
    assert out.dtype == torch.float64 and tuple(out.shape) == tuple(tensors[0].shape)
    assert parts1["ln"].shape == parts64["ln"].shape and torch.allclose(parts1["ln"], parts64["ln"], rtol=0, atol=1e-12)


# ---- the argument errors ------------------------------------------------------------------------------------------------------

OPERATOR_MESSAGE = "mono_fusion knows the precisions ['highest', 'high'], got precision='fast'"
OPTION_MESSAGE = "mono_fusion_precision is one of ['highest', 'high', 'torch'], got 'fast'"


def _message(call) -> str:
    with pytest.raises(ValueError) as caught:
        call()
    return str(caught.value)


def test_an_unknown_precision_is_refused_before_any_tensor_is_touched():
    assert mf.PRECISIONS is precision.PRECISIONS
    assert _message(lambda: precision.check("mono_fusion", "fast")) == OPERATOR_MESSAGE
    for call in (lambda: mf.mono_fusion(*(None,) * 7, precision="fast"), lambda: mf.mono_fusion_forward(*(None,) * 7, precision="fast"),
                 lambda: mf.mono_fusion_backward(*(None,) * 10, precision="fast"), lambda: mf.scratch_bytes(1, 64, True, "fast")):
        assert _message(call) == OPERATOR_MESSAGE
    assert "got precision='torch'" in _message(lambda: mf.scratch_bytes(1, 64, True, "torch"))
    tensors, _ = R.random_case(1, "g0", 64)
    for good in mf.PRECISIONS:                                  # a known precision goes on to the device check (no CPU path)
        with pytest.raises(RuntimeError, match="GPU only"):
            mf.mono_fusion(*tensors, precision=good)


def test_the_install_option_s_refusal_is_worded_as_the_other_three():
    assert _message(lambda: precision.seam_option("mono_fusion_precision", "fast")) == OPTION_MESSAGE
    assert _message(lambda: plugin.install_mono_fusion(precision="fast")) == OPTION_MESSAGE
    assert _message(lambda: plugin.install(lazy=True, mono_fusion=True, mono_fusion_precision="fast")) == OPTION_MESSAGE
    for good in (*precision.PRECISIONS, "torch"):
        assert precision.seam_option("mono_fusion_precision", good) == good


def test_a_scratch_buffer_is_refused_unless_the_precision_is_high():
    """The "highest" forward has no scratch and its backward allocates its own: a caller's buffer would go unused."""
    tensors, g = R.random_case(1, "g0", 64)
    scratch = torch.empty(16, dtype=torch.uint8)
    for call in (lambda: mf.mono_fusion_forward(*tensors, scratch=scratch),
                 lambda: mf.mono_fusion_forward(*tensors, precision="highest", scratch=scratch),
                 lambda: mf.mono_fusion_backward(*tensors, None, None, g, scratch=scratch)):
        with pytest.raises(ValueError, match='scratch is the buffer of a precision="high" call'):
            call()
    assert _message(lambda: mf.mono_fusion_forward(*tensors, scratch=scratch)) == \
        'mono_fusion_forward: scratch is the buffer of a precision="high" call, got one with precision=\'highest\''
    with pytest.raises(RuntimeError, match="GPU only"):         # with "high" it goes on to the device check
        mf.mono_fusion_forward(*tensors, precision="high", scratch=scratch)


# ---- the three entry points -----------------------------------------------------------------------------------------------------

def test_the_three_entry_points_are_declared_bound_and_sized():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in ("s360_mono_fusion_high_scratch_bytes", "s360_mono_fusion_high_forward", "s360_mono_fusion_high_backward"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.EXPORTS, name
    assert _lib.ABI_VERSION == 25 and "#define S360_ABI_VERSION 25" in (ROOT / "include" / "s360.h").read_text()
    lib = _lib.lib()
    for cm in (64, 384, 768, 1024):
        planes = 4 * 128 * (4 * 128 + cm)                       # (hi, lo) x 2 bytes of w1_r [C, C + Cm] and three [C, C] planes
        assert planes < 3 * (1 << 19)                           # under 1.5 MiB
        for tokens in (1, 129, 65536):
            assert mf.scratch_bytes(tokens, cm) == mf.scratch_bytes(tokens, cm, True) == lib.s360_mono_fusion_scratch_bytes(tokens, cm) > 0
            assert mf.scratch_bytes(tokens, cm, False) == 0     # the "highest" forward has none
            for back in (False, True):
                high = mf.scratch_bytes(tokens, cm, back, "high")
                assert high - mf.scratch_bytes(tokens, cm, back, "highest") == planes and high % 16 == 0
                assert high == lib.s360_mono_fusion_high_scratch_bytes(tokens, cm, int(back))
    for tokens, cm in ((0, 64), (-1, 64), (-2 ** 31, 384), (128, 96), (128, 0), (128, 1088)):
        assert lib.s360_mono_fusion_high_scratch_bytes(tokens, cm, 0) == 0 and lib.s360_mono_fusion_high_scratch_bytes(tokens, cm, 1) == 0
    # refusals that need no device memory: null tensors
    assert lib.s360_mono_fusion_high_forward(*(None,) * 7, 1, 128, 64, 4, 8, 16, None, None, None, None, None, 0, None) == -1
    assert lib.s360_mono_fusion_high_backward(*(None,) * 10, 1, 128, 64, 4, 8, 16, None, None, 0, *(None,) * 5, None) == -1


def test_the_entry_points_refuse_what_the_highest_ones_refuse():
    """Fake (never dereferenced) 16-byte aligned addresses: the scratch null or misaligned -1, short -2, unsupported widths the
    code of s360_mono_fusion_forward, every refusal before any GPU work."""
    import ctypes as C
    lib = _lib.lib()
    eps = C.byref(C.c_double(1e-5))
    a = [0x10000 * (i + 1) for i in range(20)]
    dims = (1, 128, 64, 4, 8, 16)
    need = [lib.s360_mono_fusion_high_scratch_bytes(128, 64, back) for back in (0, 1)]
    fwd = lambda scratch, nbytes, d=dims: lib.s360_mono_fusion_high_forward(*a[:7], *d, eps, a[7], a[8], a[9], scratch, nbytes, None)   # noqa: E731
    bwd = lambda scratch, nbytes, d=dims: lib.s360_mono_fusion_high_backward(*a[:10], *d, eps, scratch, nbytes, *a[10:15], None)         # noqa: E731
    for call, n in ((fwd, need[0]), (bwd, need[1])):
        assert call(None, n) == -1 and call(a[15] + 8, n) == -1
        assert call(a[15], n - 1) == -2 and call(a[15], 0) == -2
        assert call(a[0], n) == -1                              # the scratch is an input
        for bad in ((1, 96, 64, 4, 8, 16), (1, 128, 96, 4, 8, 16), (1, 128, 1088, 4, 8, 16)):
            assert call(a[15], 1 << 30, bad) == -4
        assert call(a[15], 1 << 30, (0, 128, 64, 4, 8, 16)) == -1
    assert lib.s360_mono_fusion_forward(*a[:7], 1, 128, 96, 4, 8, 16, eps, a[7], a[8], a[9], None) == -4


# ---- the install option ---------------------------------------------------------------------------------------------------------

NAME = plugin.MONO_FUSION_MODULE


@pytest.fixture
def standin():
    assert NAME not in sys.modules
    mod = R.standin_module(NAME)
    sys.modules[NAME] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        sys.modules.pop(NAME, None)


def _init(mod):
    return mod.EncoderCostVolume.__dict__["__init__"]


@pytest.mark.parametrize("option", ["highest", "high", "torch"])
def test_the_install_option_is_recorded_and_uninstall_restores(standin, option):
    original = _init(standin)
    bound = plugin.install_mono_fusion(precision=option)
    assert plugin.MONO_FUSION_SEAM.options == {"precision": option}
    assert _init(standin) is bound and bound.replaced is original and bound.precision == option
    enc = standin.EncoderCostVolume()
    assert isinstance(enc.rgbd_fusion, mf.FusedMonoFusion) and enc.rgbd_fusion.precision == option
    assert list(enc.state_dict()) == ["c2e.sample_grid", "rgbd_fusion.0.weight", "rgbd_fusion.1.weight", "rgbd_fusion.1.bias", "rgbd_fusion.3.weight"]
    plugin.uninstall()
    assert _init(standin) is original
    assert enc.rgbd_fusion.precision == option                  # an encoder built meanwhile keeps its own


def test_the_default_is_highest_and_a_second_install_replaces_the_wrapper_one_layer_deep(standin):
    original = _init(standin)
    assert mf.FusedMonoFusion.precision == "highest"
    plugin.install(lazy=True, mono_fusion=True)
    first = _init(standin)
    assert first.precision == "highest" and plugin.MONO_FUSION_SEAM.options == {"precision": "highest"}
    assert plugin.install_mono_fusion() is first                # the same option keeps the wrapper
    early = standin.EncoderCostVolume()
    plugin.install(lazy=True, mono_fusion=True, mono_fusion_precision="high")
    second = _init(standin)
    assert second is not first and second.precision == "high" and second.replaced is original
    third = plugin.install_mono_fusion(precision="torch")
    assert third is _init(standin) and third.precision == "torch" and third.replaced is original
    late = standin.EncoderCostVolume()
    assert (early.rgbd_fusion.precision, late.rgbd_fusion.precision) == ("highest", "torch")
    plugin.uninstall()
    assert _init(standin) is original


def test_the_option_is_independent_of_the_other_three_and_does_not_reach_the_decoder(standin):
    plugin.install(lazy=True, mono_fusion=True, mono_fusion_precision="high", transformer_ffn=True, transformer_ffn_precision="torch",
                   window_attention=True, unet_attention=True, unet_attention_precision="highest", views_per_group=3)
    assert _init(standin).precision == "high" and plugin.MONO_FUSION_SEAM.options == {"precision": "high"}
    assert plugin.TRANSFORMER_FFN_SEAM.options == {"precision": "torch"} and plugin.WINDOW_ATTENTION_SEAM.options == {"precision": "highest"}
    assert all(seam.options == {"precision": "highest"} for seam in plugin.UNET_ATTENTION_SEAMS)
    assert plugin.DECODER_SEAM.options == {"views_per_group": 3}
    plugin.uninstall()
    plugin.install(lazy=True, mono_fusion=True, transformer_ffn=True, transformer_ffn_precision="high")
    assert _init(standin).precision == "highest" and plugin.TRANSFORMER_FFN_SEAM.options == {"precision": "high"}


def test_a_cpu_forward_through_the_seam_at_high_returns_the_uninstalled_bits(standin):
    """On CPU tensors the wrapped c2e runs its own forward and FusedMonoFusion nn.Sequential's: the precision is not consulted."""
    torch.manual_seed(5)
    plain = standin.EncoderCostVolume()
    plugin.install(lazy=True, mono_fusion=True, mono_fusion_precision="high")
    fused = standin.EncoderCostVolume()
    fused.load_state_dict(plain.state_dict())
    gen = torch.Generator().manual_seed(0)
    feats, cube = torch.randn(2, 128, 8, 16, generator=gen), torch.randn(2, 64, 4, 24, generator=gen)
    assert torch.equal(plain(feats, cube), fused(feats, cube))


# ---- the launch geometry ----------------------------------------------------------------------------------------------------------

def test_the_high_launches_use_the_geometry_of_the_highest_ones():
    """The existing path cases (tests/test_gpu_mono_fusion.py's CASES) cover the "high" kernels because each is launched on the
    grid expression of its "highest" twin; a change of either fails here."""
    high, highest = HR.high_launches(), HR.launches("mf")
    assert highest == {"k_mf_forward": "(unsigned)((tokens + MF_TM - 1) / MF_TM)", "k_mf_backward_tokens": "wgs",
                       "k_mf_backward_weights": "K / MF_KC + MF_C / MF_KC, chunks",
                       "k_mf_reduce": "(nw1 + nw2 + 2 * MF_C + S360_BLOCK - 1) / S360_BLOCK"}
    assert high == {"k_mfh_split": "(unsigned)((MF_C * K + MF_C * MF_C + S360_BLOCK - 1) / S360_BLOCK)",
                    "k_mfh_forward": highest["k_mf_forward"], "k_mfh_backward_tokens": highest["k_mf_backward_tokens"],
                    "k_mfh_backward_weights": highest["k_mf_backward_weights"]}
    text = HR.KERNEL_FILE.read_text()
    tail = text[text.index('extern "C" int s360_mono_fusion_high_backward'):]
    assert "const int K = MF_C + mono_channels, chunks = mf_chunks(tokens), wgs = mf_token_wgs(tokens);" in tail
    assert tail.count("hipLaunchKernelGGL(k_mf_reduce") == 1 and "mf_tiles(tokens), chunks, p_w1, p_w2" in tail
    assert '#include "s360_bf16x3.h"' in text and "__builtin_amdgcn_mfma_f32_32x32x16_bf16" not in text      # the header's arithmetic alone
