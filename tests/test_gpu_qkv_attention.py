"""The fused multi-head QKV attention on the GPU (csrc/s360_qkv_attention.hip through splatter360_amd/qkv_attention.py) against the
float64 statement of tests/qkv_attention_reference.py, with the reference's float32 lines on the same GPU and inputs as the
yardstick.

Accuracy rule (the project's, tests/test_gpu_window_attention.py): for each of out and g_qkv — whole, and its q, k and v rows on
their own so that a failure names the pass — over all elements, the kernel's max and mean absolute error against
statement(float64) are <= max(1.5 x the same figure of reference_lines(float32), 2^-24 max|want|).

Measured on one MI355X (9 shapes x 2 scales x 5 tensors: 90 maxima and 90 means): the kernels' maxima are at most 1.27 x the
float32 lines' (1.44 x in out of `tiny` at scale 6, where both lie under the 2^-24 floor), their means at most 0.89 x (1.32 x
and 1.03 x in out and g_v of that case); the block through the seam (two installs, with and without a checkpoint: 32 tensors) 0.31 to 1.00 x and 0.25 to 1.02 x.
The scores are summed in float64 over float32 chains of 8 channels and stay float64 until the maximum or lse is subtracted; the
products over the keys are float32 chains of one 32-key tile added in float64 — as one float32 chain over all keys, `long` missed
the bound in out (1.82 x).  Delta is sum P dP / sum P over the recomputed P: with the plain sum, `tiny` at scale 6 — every row's
weight on one key, gradients of 3e-6 from dP of 30 — missed the bound in g_q and g_k (2.1e-6 and 2.4e-6 against the lines' 1.1e-6
and 1.4e-6: the rounding of lse, 1e-7, times Delta); with the quotient they are 4.8e-12 and 4.1e-12.  What remains at parity with
the yardstick is a row that two keys share at logits of +-100: dS there follows the rounding of the two scores' 8-channel chains,
as it does the rounding of torch's float32 scores.

tests/test_gpu_qkv_attention_float64.py holds the same kernels to float64 per (batch element, head, token) row, lse and Delta
included, through the C ABI into NaN-filled buffers between sentinels; the two files complement each other (its docstring).  The
`isfinite` assertion of _check_rule below does not alone prove a write: `out` comes from torch.empty, and stale finite memory
passes it; that every element is written, and nothing beside it, is shown there.
"""
import functools
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

import group_norm_reference as G
import qkv_attention_reference as R
from splatter360_amd import plugin, qkv_attention as qa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (N, views, cross_view, heads, T, order); ch = 32
SHAPES = {
    "tile": (2, 1, False, 1, 32, "legacy"),          # exactly one tile
    "ragged": (2, 1, False, 2, 35, "legacy"),        # one token past a tile; rows not 16-byte aligned
    "tiny": (1, 1, False, 1, 5, "legacy"),           # less than a tile
    "straddle": (4, 2, True, 4, 48, "legacy"),       # L = 96, B = 2; the second tile spans two views; the (v b) row order; four interleaved heads
    "views3": (3, 3, True, 1, 20, "legacy"),         # L = 60
    "frames_unused": (4, 2, False, 2, 40, "legacy"),  # n_frames = 2 with cross-view off: the rows stay separate
    "new_order": (2, 2, True, 2, 40, "new"),         # the q | k | v chunk order
    "long": (2, 2, True, 1, 320, "legacy"),          # L = 640: twenty key tiles, the running maximum moves
    "uneven": (2, 2, True, 1, 100, "legacy"),        # L = 200: seven tiles for four waves (2, 2, 2, 1), the last one ragged, T no multiple of 32
}
SCALES = (1.0, 6.0)
NAMES = ("out", "g_qkv", "g_q", "g_k", "g_v")


def _opts(name):
    n, views, cross, heads, t, order = SHAPES[name]
    return heads, dict(n_frames=views, cross_view=cross, order=order)


def _native(name, qkv, g):
    heads, opts = _opts(name)
    x = qkv.detach().clone().requires_grad_(True)
    out = qa.qkv_attention(x, heads, **opts)
    out.backward(g)
    return out.detach(), x.grad


def _with_parts(name, pair):
    out, g_qkv = pair
    return (out, g_qkv, *R.parts(g_qkv, SHAPES[name][3], SHAPES[name][5]))


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    """Inputs, the float64 statement, the float32 lines and the kernels' results of one case: computed once, shared, never
    modified."""
    n, views, cross, heads, t, order = SHAPES[name]
    seed = 2000 + 7 * sorted(SHAPES).index(name)
    qkv, g = R.random_case(n, heads, t, scale=scale, seed=seed, device=DEV)
    want = R.gradients(lambda x: R.statement(x, heads, views, cross, order), qkv, g, torch.float64)
    lines = R.gradients(lambda x: R.reference_lines(x, heads, views, cross, order), qkv, g)
    got = _native(name, qkv, g)
    return (qkv, g), _with_parts(name, want), _with_parts(name, lines), _with_parts(name, got)


def _errors(x, want):
    e = (x.double() - want).abs()
    return e.max().item(), e.mean().item()


def _check_rule(tag, names, want, lines, got):
    failures = []
    for n, w64, l32, x in zip(names, want, lines, got):
        assert x.dtype == torch.float32 and x.shape == w64.shape, (tag, n)
        assert torch.isfinite(x).all(), (tag, n)                                    # no NaN tolerated (alone no proof of a write: the docstring)
        (kmax, kmean), (lmax, lmean) = _errors(x, w64), _errors(l32, w64)
        floor = 2.0 ** -24 * w64.abs().max().item()
        print(f"{tag} {n}: kernel max {kmax:.3e} mean {kmean:.3e} | float32 lines max {lmax:.3e} mean {lmean:.3e} | floor {floor:.3e}"
              f" | ratios {kmax / lmax if lmax else 0:.2f} {kmean / lmean if lmean else 0:.2f}")
        if not (kmax <= max(1.5 * lmax, floor) and kmean <= max(1.5 * lmean, floor)):
            failures.append((n, kmax, kmean, lmax, lmean, floor))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accuracy_against_the_float64_statement(name, scale):
    _, want, lines, got = _run(name, scale)
    _check_rule(f"{name} scale={scale:g}", NAMES, want, lines, got)


@pytest.mark.parametrize("name", ["ragged", "straddle", "long"])
def test_large_logits_stay_finite_and_inside_the_hull_of_v(name):
    """Scale 30: the logits' deviation is about 900 / sqrt(32) x sqrt(32) ~ 900, every row is all but one-hot.  Every out[c, t]
    lies inside [min_s v[c, s], max_s v[c, s]] over the joint sequence of its batch element and head, up to float32 rounding:
    the weights are float32 exponentials, their sum and the weighted sum of v are float32 chains over the handful of keys that
    carry weight, the quotient is rounded once — 8 x 2^-24 x max|v[c, .]| covers those roundings."""
    n, views, cross, heads, t, order = SHAPES[name]
    qkv, g = R.random_case(n, heads, t, scale=30.0, seed=5, device=DEV)
    out, g_qkv = _native(name, qkv, g)
    assert torch.isfinite(out).all() and torch.isfinite(g_qkv).all()
    v = R.split_heads(qkv, heads, views, cross, order)[2]                           # [B, heads, ch, L]
    lo, hi = v.amin(dim=3, keepdim=True), v.amax(dim=3, keepdim=True)
    o = R.joint(out, heads, views, cross)
    margin = 8 * 2.0 ** -24 * v.abs().amax(dim=3, keepdim=True)
    excess = torch.maximum(o - hi, lo - o)
    print(f"{name}: largest excess over the hull {excess.max().item():.3e}, margin {margin.min().item():.3e} .. {margin.max().item():.3e}")
    assert (excess <= margin).all()


def _direct(name, qkv, g, g_qkv=None):
    heads, opts = _opts(name)
    out, lse = qa.attention_forward(qkv, heads, **opts)
    return out, lse, qa.attention_backward(qkv, lse, g, heads, g_qkv=g_qkv, **opts)


@pytest.mark.parametrize("name", ["straddle", "long"])
def test_forward_and_backward_are_deterministic(name):
    (qkv, g), _, _, got = _run(name, 1.0)
    n, views, cross, heads, t, order = SHAPES[name]
    first = _direct(name, qkv, g)
    assert first[1].dtype == torch.float64 and tuple(first[1].shape) == (n // views, heads, views * t)
    assert torch.equal(first[0], got[0]) and torch.equal(first[2], got[1])          # the autograd node runs the same two calls
    again = _direct(name, qkv, g)
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _direct(name, qkv, g)
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_log_sum_exp_is_the_statement_s():
    (qkv, g), _, _, _ = _run("straddle", 1.0)
    n, views, cross, heads, t, order = SHAPES["straddle"]
    _, lse, _ = _direct("straddle", qkv, g)
    q, k, _ = (x.double() for x in R.split_heads(qkv, heads, views, cross, order))
    want = torch.logsumexp(torch.einsum("bhct,bhcs->bhts", q, k) / q.shape[2] ** 0.5, dim=-1)
    assert (lse - want).abs().max().item() <= 1e-5


@pytest.mark.parametrize("name", ["ragged", "straddle"])
def test_every_element_of_the_gradient_is_written(name):
    """The backward writes into a buffer that holds NaN everywhere: the masked tails of the last tiles included, nothing is left."""
    (qkv, g), _, _, got = _run(name, 1.0)
    buf = torch.full_like(qkv, float("nan"))
    _, _, g_qkv = _direct(name, qkv, g, g_qkv=buf)
    assert g_qkv is buf and torch.isfinite(buf).all() and torch.equal(buf, got[1])


def test_no_host_synchronisation():
    (qkv, g), _, _, got = _run("straddle", 1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _native("straddle", qkv, g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_a_non_contiguous_input_is_copied_once():
    (qkv, g), _, _, got = _run("ragged", 1.0)
    nc = torch.cat([qkv, qkv], dim=2)[..., :qkv.shape[2]]
    assert not nc.is_contiguous()
    again = _native("ragged", nc, g)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def test_memory_stays_of_the_order_of_the_input():
    """(2, 2, on, 4, 1024, legacy): L = 2048, qkv is 3 MiB and ONE [heads, L, L] score tensor would be 64 MiB (21 x).  A forward plus
    backward of the native path allocates out, g_out, g_qkv and two float64 vectors per (head, token), about 1.7 x qkv; the
    bound is 3 x."""
    n, views, heads, t = 2, 2, 4, 1024
    qkv, _ = R.random_case(n, heads, t, seed=3, device=DEV)
    qkv.requires_grad_(True)
    nbytes = qkv.numel() * 4
    assert nbytes == 3 * 1024 * 1024 and heads * (views * t) ** 2 * 4 == 64 * 1024 * 1024

    def step():
        out = qa.qkv_attention(qkv, heads, n_frames=views, cross_view=True)
        out.backward(torch.ones_like(out))

    step()                                                                          # warm-up
    qkv.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print(f"forward + backward peak rise {rise / nbytes:.3f} x qkv ({rise} bytes)")
    assert rise <= 3 * nbytes
    assert torch.isfinite(qkv.grad).all() and qkv.grad.abs().max().item() > 0


def test_argument_errors_come_before_any_launch(monkeypatch):
    qkv, _ = R.random_case(4, 2, 8, seed=1, device=DEV)
    monkeypatch.setattr(qa._lib, "lib", lambda: pytest.fail("a launch was reached"))
    with pytest.raises(ValueError, match="n_heads"):
        qa.qkv_attention(qkv, 5)                                                    # 192 rows are no multiple of 15
    with pytest.raises(ValueError, match="n_frames"):
        qa.qkv_attention(qkv, 2, n_frames=3, cross_view=True)
    with pytest.raises(ValueError, match="ch"):
        qa.qkv_attention(qkv, 4)                                                    # ch = 16
    with pytest.raises(ValueError, match="qkv"):
        qa.qkv_attention(qkv.cpu(), 2)
    with pytest.raises(ValueError, match="float32"):
        qa.qkv_attention(qkv.half(), 2)
    with pytest.raises(ValueError, match="order"):
        qa.qkv_attention(qkv, 2, order="other")
    with pytest.raises(ValueError, match="qkv"):
        qa.attention_forward(qkv[0], 2)


# ---- the seam on the GPU -------------------------------------------------------------------------------------------------------

MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)
PARAMS = ("qkv.weight", "qkv.bias", "proj_out.weight", "proj_out.bias", "norm.weight", "norm.bias")


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


def _block64(block, x, g):
    """The postnorm block x + norm(proj_out(attention(qkv(x)))) in float64 from the block's float32 parameters -> (out, g_x,
    parameter gradients in PARAMS' order)."""
    p = {k: v.detach().double().requires_grad_(True) for k, v in block.named_parameters()}
    b, c, *spatial = x.shape
    x64 = x.detach().double().reshape(b, c, -1).requires_grad_(True)
    att = block.attention
    a = R.statement(F.conv1d(x64, p["qkv.weight"], p["qkv.bias"]), att.n_heads, att.n_frames, att.use_cross_view_self_attn, "legacy")
    h = F.group_norm(F.conv1d(a, p["proj_out.weight"], p["proj_out.bias"]), block.norm.num_groups, p["norm.weight"], p["norm.bias"], block.norm.eps)
    out = (x64 + h).reshape(b, c, *spatial)
    out.backward(g.double())
    return (out.detach(), x64.grad.reshape(x.shape), *(p[k].grad for k in PARAMS))


def _block32(block, x, g, through_checkpoint=False):
    block.zero_grad(set_to_none=True)
    xin = x.detach().clone().requires_grad_(True)
    out = checkpoint(block._forward, xin, use_reentrant=True) if through_checkpoint else block(xin)
    out.backward(g)
    named = dict(block.named_parameters())
    return (out.detach(), xin.grad, *(named[k].grad.clone() for k in PARAMS))


@pytest.mark.parametrize("with_group_norm", [False, True])
def test_seam_runs_the_kernel_in_the_attention_block_and_holds_the_rule(standin, with_group_norm):
    """The stand-in AttentionBlock (4 heads of 32, 2 views x 2 batch elements, 6 x 8 = 48 tokens: the `straddle` shape) whose
    attention is the stand-in QKVAttentionLegacy: output, input gradient and parameter gradients against the block in float64,
    with the uninstalled float32 block on the same GPU as the yardstick; then once more through a checkpoint that recomputes the
    forward under enable_grad."""
    unet = standin
    block = G.randomise(unet.AttentionBlock(128, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True), 11).to(DEV)
    assert type(block.attention) is unet.QKVAttentionLegacy and block.num_heads == 4
    gen = torch.Generator().manual_seed(12)
    x, g = (torch.randn(4, 128, 6, 8, generator=gen).to(DEV) for _ in range(2))
    names = ("out", "g_x", *("g_" + k for k in PARAMS))
    want = _block64(block, x, g)
    lines = _block32(block, x, g)
    assert block.attention.calls == 1
    plugin.install(lazy=True, unet_attention=True, group_norm=with_group_norm)
    wrapper = unet.QKVAttentionLegacy.__dict__["forward"]
    assert wrapper.replaced is not None and wrapper.native_calls == 0
    assert (getattr(unet.AttentionBlock.__dict__.get("_forward"), "replaced", None) is not None) == with_group_norm
    got = _block32(block, x, g)
    assert wrapper.native_calls == 1 and block.attention.calls == 1                 # the kernels, once; the replaced method, never
    _check_rule(f"block group_norm={int(with_group_norm)}", names, want, lines, got)
    again = _block32(block, x, g, through_checkpoint=True)
    assert wrapper.native_calls == 3 and block.attention.calls == 1                 # the forward and its recomputation
    _check_rule(f"block group_norm={int(with_group_norm)} checkpoint", names, want, lines, again)
    assert torch.equal(again[0], got[0])
    qkv16 = block.qkv(x.reshape(4, 128, -1)).detach().half()                        # half precision reaches the replaced method
    out16 = block.attention(qkv16)
    assert out16.dtype == torch.float16 and block.attention.calls == 2 and wrapper.native_calls == 3
    block.attention.calls = 1
    plugin.uninstall()
    assert getattr(unet.QKVAttentionLegacy.__dict__["forward"], "replaced", None) is None
    back = _block32(block, x, g)
    assert block.attention.calls == 2 and torch.equal(back[0], lines[0])


def test_seam_on_the_new_order_class_gives_the_direct_api_s_bits(standin):
    unet = standin
    (qkv, g), _, _, _ = _run("new_order", 1.0)
    att = unet.QKVAttention(2)
    plugin.install_unet_attention()
    wrapper = unet.QKVAttention.__dict__["forward"]
    out = att(qkv)
    assert wrapper.native_calls == 1 and att.calls == 0
    assert torch.equal(out, qa.qkv_attention(qkv, 2, order="new"))                  # QKVAttention has no cross-view form
