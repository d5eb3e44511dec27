"""The QKV attention's "high" precision mode on the GPU (the k_qah_* kernels of csrc/s360_qkv_attention.hip through
splatter360_amd/qkv_attention.py, precision="high") against the float64 statement of tests/qkv_attention_reference.py.

Accuracy rule: for each of out and g_qkv — whole, and its q, k and v rows on their own so that a failure names the pass — over
all elements, the kernel's max and mean absolute error against statement(float64) are <= max(1.5 x (e3 + e32), 2^-24 max|want|):
e3 the same figure of split_statement(terms=3) (tests/qkv_attention_high_reference.py: the split's rounding, sums in float64), e32
that of the float32 lines on the same GPU (float32 accumulation) — the kernel has both.  tests/test_qkv_attention_high_spec.py
compares a single-bf16 product with this bound.

Measured on one MI355X (11 shapes x 2 scales x 5 tensors: 110 maxima and 110 means), kernel error / bound: the maxima are at most
0.928 (g_q of `views3` at scale 1) and the means at most 0.696 (g_v of `new_order` at scale 6); typically both are 0.64 to 0.67, the
kernel's error being the terms=3 statement's.  A maximum is not as steady as a mean: where an element of P lies next to a tie of
its lo part's rounding, a P a few float32 steps from the statement's float32(softmax in float64) rounds lo the other way, which
moves one term of g_v by 2^-17 P |g| (a statement fed float32 scores perturbed by 5e-7 of their size on the CPU moved the maximum
of a 17-token case between 8.4e-06 and 1.59e-05).  The kernel's P is therefore exp(sum / sqrt(ch) - lse) with the difference in
float64 and the rounding of the exponent carried into the result (qah_exp).  lse is within 4.7e-06 of the float64 log-sum-exp at
scale 1; at scale 30 the largest excess over the hull is 4.9e-04 against a slack of 1.6e-03; forward + backward peak 4.04 x qkv at
L = 2048, of which the scratch is 2.33 x.  The seeds are the rule of tests/test_gpu_qkv_attention.py over the eleven names.

Hull: an output of the "high" mode is a convex combination of split values vh + vl, each within 2^-16 |v| of v, so it lies
inside the joint sequence's hull of v widened by 2^-16 max|v| (the float32 accumulation adds a few 2^-24 of that, far below).
"""
import ctypes as C
import functools
import sys

import pytest
import torch
from torch.utils.checkpoint import checkpoint

import group_norm_reference as G
import qkv_attention_high_reference as H
import qkv_attention_reference as R
from splatter360_amd import _call, _lib, plugin, qkv_attention as qa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = H.SHAPES


def _opts(name):
    n, views, cross, heads, t, order = SHAPES[name]
    return heads, dict(n_frames=views, cross_view=cross, order=order)


def _native(name, qkv, g, **kw):
    heads, opts = _opts(name)
    x = qkv.detach().clone().requires_grad_(True)
    out = qa.qkv_attention(x, heads, **opts, **kw)
    out.backward(g)
    return out.detach(), x.grad


def _direct(name, qkv, g, g_qkv=None, **kw):
    heads, opts = _opts(name)
    out, lse = qa.attention_forward(qkv, heads, **opts, **kw)
    return out, lse, qa.attention_backward(qkv, lse, g, heads, g_qkv=g_qkv, **opts, **kw)


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    """Inputs, the float64 statement, the terms=3 statement, the float32 lines and the "high" kernels' results of one case:
    computed once, shared, never modified."""
    (qkv, g), want, three, lines = H.yardsticks(name, scale, DEV)
    got = H.with_parts(name, _native(name, qkv, g, precision="high"))
    return (qkv, g), want, three, lines, got


@pytest.mark.parametrize("scale", H.SCALES)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accuracy_against_the_float64_statement(name, scale):
    _, want, three, lines, got = _run(name, scale)
    H.check_rule(f"{name} scale={scale:g}", H.NAMES, want, three, lines, got)


@pytest.mark.parametrize("name", ["straddle", "new_order", "long", "uneven"])
def test_exact_data_come_out_in_the_right_rows_and_channels(name):
    """Key j of every (batch element, head) carries a +-1 code over the 32 channels, the bits of (2654435761 j) mod 2^32 —
    distinct by construction, the multiplier is odd; query i carries 512 code[pi(i)] with pi(i) = (11 i + 7) mod L; v holds
    integers in [-8, 8].  The score of key pi(i) is 512 x 32 / sqrt(32) and two codes differ in at least one channel, 512 x 2 /
    sqrt(32) = 181 below (checked in float64 to be more than 100), so P is the permutation matrix.  All of these are exact in
    bfloat16, so out must be v[:, pi] bit for bit: a swapped row and column, a wrong k order in the second product or a wrong
    head offset moves integers about."""
    n, views, cross, heads, t, order = SHAPES[name]
    nv = views if cross else 1
    b, length = n // nv, nv * t
    j = torch.arange(length, dtype=torch.int64)
    word = (2654435761 * j) % (1 << 32)
    code = (((word.unsqueeze(1) >> torch.arange(32)) & 1) * 2 - 1).float()           # [L, 32]
    assert len({tuple(r) for r in code.tolist()}) == length
    pi = (11 * j + 7) % length
    assert len(set(pi.tolist())) == length and not torch.equal(pi[pi], j)            # a permutation, not its own inverse
    k = code.expand(b, heads, length, 32).contiguous()
    q = 512.0 * k[:, :, pi]
    gen = torch.Generator().manual_seed(11)
    v = torch.randint(-8, 9, (b, heads, length, 32), generator=gen).float()
    scores = q.double() @ k.double().transpose(-1, -2) / 32 ** 0.5
    win = scores.gather(-1, pi.view(1, 1, length, 1).expand(b, heads, length, 1))
    rest = scores.scatter(-1, pi.view(1, 1, length, 1).expand(b, heads, length, 1), float("-inf")).amax(-1, keepdim=True)
    assert (win - rest).min().item() > 100.0
    qkv = R.qkv_from_rows(q, k, v, views, cross, order).contiguous()
    want = R.out_from_rows(v[:, :, pi], views, cross)
    out = qa.qkv_attention(qkv.to(DEV), heads, n_frames=views, cross_view=cross, order=order, precision="high")
    assert torch.equal(out.cpu(), want)


def test_highest_is_the_call_without_the_keyword_and_high_is_not():
    (qkv, g), _, _, _, high = _run("straddle", 1.0)
    plain = _native("straddle", qkv, g)
    highest = _native("straddle", qkv, g, precision="highest")
    assert all(torch.equal(x, y) for x, y in zip(plain, highest))
    assert all(not torch.equal(x, y) for x, y in zip(plain, high[:2]))


@pytest.mark.parametrize("name", ["straddle", "long"])
def test_forward_and_backward_are_deterministic(name):
    (qkv, g), _, _, _, got = _run(name, 1.0)
    again = _native(name, qkv, g, precision="high")
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    again = _native(name, qkv, g, precision="high")
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _native(name, qkv, g, precision="high")
    side.synchronize()
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("name,scale", [("straddle", 1.0), ("uneven", 1.0)])
def test_direct_calls_give_the_autograd_path_s_bits_and_the_statement_s_lse(name, scale):
    (qkv, g), _, _, _, got = _run(name, scale)
    n, views, cross, heads, t, order = SHAPES[name]
    out, lse, g_qkv = _direct(name, qkv, g, precision="high")
    assert torch.equal(out, got[0]) and torch.equal(g_qkv, got[1])
    assert lse.dtype == torch.float64 and tuple(lse.shape) == (n // views, heads, views * t)
    q, k, _ = (x.double() for x in R.split_heads(qkv, heads, views, cross, order))
    want = torch.logsumexp(torch.einsum("bhct,bhcs->bhts", q, k) / q.shape[2] ** 0.5, dim=-1)
    err = (lse - want).abs().max().item()
    print(f"{name} scale={scale:g}: lse max error {err:.3e}")
    assert err <= 1e-3


@pytest.mark.parametrize("name", ["ragged", "straddle"])
def test_every_element_of_the_gradient_is_written(name):
    """The backward writes into a buffer that holds NaN everywhere: the masked tails of the last tiles included, nothing is left."""
    (qkv, g), _, _, _, got = _run(name, 1.0)
    buf = torch.full_like(qkv, float("nan"))
    _, _, g_qkv = _direct(name, qkv, g, g_qkv=buf, precision="high")
    assert g_qkv is buf and torch.isfinite(buf).all() and torch.equal(buf, got[1])


def _abi(name, qkv, g, fill):
    """Forward and backward through the C ABI with scratch buffers of exactly scratch_bytes bytes filled with `fill` ->
    (out, lse, g_qkv, the two scratch tensors)."""
    n, views, cross, heads, t, order = SHAPES[name]
    nv = views if cross else 1
    lib, p = _lib.lib(), _call.ptr
    dims = (n, nv, heads, 32, t, qa.ORDERS[order])
    out = torch.empty(n, heads * 32, t, device=DEV)
    lse = torch.empty(n // nv, heads, nv * t, dtype=torch.float64, device=DEV)
    delta, g_qkv = torch.empty_like(lse), torch.empty_like(qkv)
    s_fwd, s_bwd = (torch.full((qa.scratch_bytes(n, nv, heads, t, back),), fill, dtype=torch.uint8, device=DEV) for back in (False, True))
    with torch.cuda.device(DEV):
        st = _call.stream(torch.device(DEV))
        assert lib.s360_qkv_attention_high_forward(p(qkv), *dims, p(out), p(lse), p(s_fwd), s_fwd.numel(), st) == 0
        assert lib.s360_qkv_attention_high_backward(p(qkv), p(lse), p(g), *dims, p(delta), p(g_qkv), p(s_bwd), s_bwd.numel(), st) == 0
    torch.cuda.synchronize()
    return out, lse, g_qkv, s_fwd, s_bwd


@pytest.mark.parametrize("name", ["ragged", "tiny", "straddle"])
def test_a_poisoned_scratch_changes_nothing(name):
    """0xFF in every byte of the scratch is a bfloat16 NaN in every element: the pre-pass writes all that the main kernels read,
    the padding to a multiple of 32 tokens included."""
    (qkv, g), _, _, _, got = _run(name, 1.0)
    out, lse, g_qkv, _, _ = _abi(name, qkv.contiguous(), g.contiguous(), 0xFF)
    assert torch.equal(out, got[0]) and torch.equal(g_qkv, got[1])
    assert torch.equal(lse, _direct(name, qkv, g, precision="high")[1])


def test_null_short_and_misaligned_scratch_are_refused_and_write_nothing():
    (qkv, g), _, _, _, _ = _run("straddle", 1.0)
    n, views, cross, heads, t, order = SHAPES["straddle"]
    lib, p = _lib.lib(), _call.ptr
    dims = (n, views, heads, 32, t, 0)
    out, g_qkv = torch.full((n, heads * 32, t), 7.0, device=DEV), torch.full_like(qkv, 7.0)
    lse = torch.full((n // views, heads, views * t), 7.0, dtype=torch.float64, device=DEV)
    delta, lse_in = torch.full_like(lse, 7.0), torch.zeros_like(lse)
    with torch.cuda.device(DEV):
        st = _call.stream(torch.device(DEV))
        for back in (False, True):
            need = qa.scratch_bytes(n, views, heads, t, back)
            scratch = torch.full((need + 16,), 7, dtype=torch.uint8, device=DEV)
            for sp, size, code in ((None, need, -1), (p(scratch), need - 1, -2), (C.c_void_p(scratch.data_ptr() + 2), need, -1)):
                if back:
                    rc = lib.s360_qkv_attention_high_backward(p(qkv), p(lse_in), p(g), *dims, p(delta), p(g_qkv), sp, size, st)
                else:
                    rc = lib.s360_qkv_attention_high_forward(p(qkv), *dims, p(out), p(lse), sp, size, st)
                assert rc == code, (back, size, rc)
            torch.cuda.synchronize()
            assert scratch.eq(7).all()
    assert out.eq(7.0).all() and lse.eq(7.0).all() and delta.eq(7.0).all() and g_qkv.eq(7.0).all()


@pytest.mark.parametrize("name", ["ragged", "straddle", "long"])
def test_large_logits_stay_finite_and_inside_the_hull_of_v(name):
    n, views, cross, heads, t, order = SHAPES[name]
    qkv, g = R.random_case(n, heads, t, scale=30.0, seed=5, device=DEV)
    out, g_qkv = _native(name, qkv, g, precision="high")
    assert torch.isfinite(out).all() and torch.isfinite(g_qkv).all()
    v = R.split_heads(qkv, heads, views, cross, order)[2]                           # [B, heads, ch, L]
    lo, hi = v.amin(dim=3, keepdim=True), v.amax(dim=3, keepdim=True)
    o = R.joint(out, heads, views, cross)
    excess = torch.maximum(o - hi, lo - o).max().item()
    slack = 2.0 ** -16 * v.abs().max().item()                                       # the split of v (the module's docstring)
    print(f"{name}: largest excess over the hull {excess:.3e}, the split's slack {slack:.3e}")
    assert excess <= slack


def test_no_host_synchronisation():
    (qkv, g), _, _, _, got = _run("straddle", 1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _native("straddle", qkv, g, precision="high")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


def _peak_delta(fn):
    """Peak bytes REQUESTED from the allocator during fn() (tests/test_gpu_window_attention_high.py has the reason)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_stats(DEV)["requested_bytes.all.current"]
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.memory_stats(DEV)["requested_bytes.all.peak"] - base, out


def test_scratch_stays_within_the_operands():
    """With L padded to 32: a forward's scratch is at most the bytes of qkv, a backward's at most twice those of qkv and g_out."""
    for name, (n, views, cross, heads, t, order) in SHAPES.items():
        nv = views if cross else 1
        lpad = -(-nv * t // 32) * 32
        nq, ng = 4 * (n // nv) * heads * 3 * 32 * lpad, 4 * (n // nv) * heads * 32 * lpad
        fwd, bwd = (qa.scratch_bytes(n, nv, heads, t, back) for back in (False, True))
        print(f"{name}: scratch {fwd} / {bwd} bytes, padded qkv {nq}, padded qkv + g_out {nq + ng}")
        assert 0 < fwd <= nq and fwd < bwd <= 2 * (nq + ng), name


def test_memory_is_today_s_bound_plus_the_scratch():
    """(2, 2, on, 4, 1024, legacy) of tests/test_gpu_qkv_attention.py: qkv is 3 MiB; today's bound for a forward plus backward, 3 x
    qkv, plus the backward's scratch."""
    n, views, heads, t = 2, 2, 4, 1024
    qkv, _ = R.random_case(n, heads, t, seed=3, device=DEV)
    qkv.requires_grad_(True)
    nbytes = qkv.numel() * 4
    scratch = qa.scratch_bytes(n, views, heads, t, True)
    assert nbytes == 3 * 1024 * 1024

    def step():
        out = qa.qkv_attention(qkv, heads, n_frames=views, cross_view=True, precision="high")
        out.backward(torch.ones_like(out))

    step()                                                                          # warm-up
    qkv.grad = None
    rise, _ = _peak_delta(step)
    print(f"forward + backward peak {rise / nbytes:.3f} x qkv, of which scratch {scratch / nbytes:.3f} x qkv")
    assert rise <= 3 * nbytes + scratch
    assert torch.isfinite(qkv.grad).all() and qkv.grad.abs().max().item() > 0


# ---- the seam on the GPU -------------------------------------------------------------------------------------------------------

MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)


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


def _block(block, x, g, through_checkpoint=False):
    block.zero_grad(set_to_none=True)
    xin = x.detach().clone().requires_grad_(True)
    out = checkpoint(block._forward, xin, use_reentrant=True) if through_checkpoint else block(xin)
    out.backward(g)
    return (out.detach(), xin.grad, *(p.grad.clone() for _, p in sorted(block.named_parameters())))


def test_seam_follows_torch_s_setting_at_every_call_and_under_a_checkpoint(standin):
    """The stand-in AttentionBlock of tests/test_gpu_qkv_attention.py (the `straddle` shape) under
    unet_attention_precision="torch": the attention module on its own against the direct calls, bit for bit, then the block with
    and without a checkpoint that recomputes the forward."""
    unet = standin
    (qkv, g), _, _, _, high = _run("straddle", 1.0)
    highest = _native("straddle", qkv, g)
    block = G.randomise(unet.AttentionBlock(128, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True), 11).to(DEV)
    assert type(block.attention) is unet.QKVAttentionLegacy and block.num_heads == 4
    plugin.install(lazy=True, unet_attention=True, unet_attention_precision="torch")
    wrapper = unet.QKVAttentionLegacy.__dict__["forward"]
    assert wrapper.precision == "torch" and wrapper.native_calls == 0

    def through_the_module():
        x = qkv.detach().clone().requires_grad_(True)
        out = block.attention(x)
        out.backward(g)
        return out.detach(), x.grad

    gen = torch.Generator().manual_seed(12)
    x, gx = (torch.randn(4, 128, 6, 8, generator=gen).to(DEV) for _ in range(2))
    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high")
        seam_high = through_the_module()
        block_high = _block(block, x, gx)
        assert wrapper.native_calls == 2
        block_high_checkpoint = _block(block, x, gx, through_checkpoint=True)
        assert wrapper.native_calls == 4                                            # the forward and its recomputation
        torch.set_float32_matmul_precision("highest")
        seam_highest = through_the_module()
        block_highest = _block(block, x, gx)
    finally:
        torch.set_float32_matmul_precision(before)
    assert wrapper.native_calls == 6 and block.attention.calls == 0                 # the replaced method, never
    assert all(torch.equal(a, b) for a, b in zip(seam_high, high[:2]))
    assert all(torch.equal(a, b) for a, b in zip(seam_highest, highest))
    assert torch.equal(block_high[0], block_high_checkpoint[0])                     # as tests/test_gpu_qkv_attention.py: the output's bits
    for a, b in zip(block_high[1:], block_high_checkpoint[1:]):                     # the recomputation ran "high" too
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()
    assert not torch.equal(block_high[0], block_highest[0])
