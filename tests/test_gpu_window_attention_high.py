"""The window attention's "high" precision mode on the GPU (the k_wah_* kernels of csrc/s360_window_attention.hip through
splatter360_amd/window_attention.py, precision="high") against the float64 statement of tests/window_attention_reference.py.

Accuracy rule: for each of out, g_q, g_k, g_v over all elements, the kernel's max and mean absolute error against
statement(float64) are <= max(1.5 x (e3 + e32), 2^-24 max|want|): e3 the same figure of split_statement(terms=3)
(tests/window_attention_high_reference.py: the split's rounding, sums in float64), e32 that of the float32 lines on the same GPU
(float32 accumulation) — the kernel has both.  tests/test_window_attention_high_spec.py shows that a single-bf16 product is 50 x
or more beyond e3, so a kernel that loses a lo plane or a term cannot pass.

Hull: an output of the "high" mode is a convex combination of split values vh + vl, each within 2^-16 |v| of v, so it lies
inside the window's hull of v widened by 2^-16 max|v| (the float32 accumulation adds a few 2^-24 of that, far below).
"""
import ctypes as C
import functools
import sys

import pytest
import torch

import window_attention_high_reference as H
import window_attention_reference as R
from splatter360_amd import _call, _lib, plugin, window_attention as wa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (B, m, h, w, K, C): the eight shapes of tests/test_gpu_window_attention.py and one per remaining channel count
SHAPES = {
    "tile": (2, 0, 8, 16, 2, 128),
    "ragged": (1, 0, 10, 14, 2, 128),
    "tiles3": (2, 1, 16, 24, 2, 128),
    "multi": (2, 3, 8, 12, 2, 128),
    "k1": (2, 0, 4, 5, 1, 128),
    "c32": (1, 2, 8, 8, 2, 32),
    "long": (1, 0, 32, 64, 2, 128),
    "k4": (1, 1, 16, 16, 4, 128),
    "c64": (1, 0, 8, 8, 2, 64),
    "c96": (1, 1, 8, 8, 2, 96),
}
RUNS = [(name, shift, scale, rule) for name, s in SHAPES.items() for shift in ((False, True) if s[4] > 1 else (False,))
        for scale in (1.0, 6.0) for rule in (("reference", "aligned") if name == "multi" and shift else ("reference",))]
NAMES = ("out", "g_q", "g_k", "g_v")


def _native(name, q, k, v, g, shift, rule, needs=(True, True, True), **kw):
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v = (t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), needs))
    if name == "k1":
        out = wa.full_attention(q, k, v, **kw)
    else:
        out = wa.window_attention(q, k, v, height=h, width=w, num_splits=ksp, with_shift=shift, mask_rule=rule, **kw)
    out.backward(g)
    return out.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def _run(name, shift, scale, rule):
    """Inputs, the float64 statement, the terms=3 statement, the float32 lines and the "high" kernels' results of one case:
    computed once, shared, never modified."""
    b, m, h, w, ksp, c = SHAPES[name]
    seed = 2000 + 7 * sorted(SHAPES).index(name) + int(shift)
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=scale, seed=seed, device=DEV)
    want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, ksp, shift, h, w, rule), q, k, v, g, torch.float64)
    three = R.gradients(lambda a, bb, cc: H.split_statement(a, bb, cc, ksp, shift, h, w, rule, terms=3), q, k, v, g, torch.float64)
    mask = R.dense_mask(h, w, ksp, DEV) if shift else None
    lines = R.gradients(lambda a, bb, cc: R.reference_lines(a, bb, cc, ksp, shift, h, w, mask, rule=rule), q, k, v, g)
    got = _native(name, q, k, v, g, shift, rule, precision="high")
    return (q, k, v, g), want, three, lines, got


@pytest.mark.parametrize("name,shift,scale,rule", RUNS)
def test_accuracy_against_the_float64_statement(name, shift, scale, rule):
    _, want, three, lines, got = _run(name, shift, scale, rule)
    H.check_rule(f"{name} shift={int(shift)} scale={scale:g} {rule}", NAMES, want, three, lines, got)


@pytest.mark.parametrize("name,shift", [("ragged", True), ("multi", True), ("long", False), ("long", True)])
def test_exact_data_come_out_in_the_right_rows_and_channels(name, shift):
    """Key j of every window carries a +-1 code e_j, query i carries 128 e_pi(i) with pi(i) = (11 i + 7) mod Lk, a fixed
    permutation that is not its own inverse: the score of key pi(i) is 128 sqrt(C) and every other lies more than 200 below
    (checked in float64), so that P is the permutation matrix even where the finite mask takes 100 off the winner; v holds
    integers in [-8, 8].  All of these are exact in bfloat16, so out must be v[pi(i)] bit for bit: a swapped row and column, a
    wrong k order in the second product or a wrong channel map moves integers about."""
    b, m, h, w, ksp, c = SHAPES[name]
    mm = max(m, 1)
    gen = torch.Generator().manual_seed(11)
    tok, _ = R.window_index(h, w, ksp, shift)
    nw, lw = tok.shape
    lk = lw * mm
    code = (torch.randint(0, 2, (b, nw, lk, c), generator=gen) * 2 - 1).float()
    vals = torch.randint(-8, 9, (b, nw, lk, c), generator=gen).float()
    pi = (11 * torch.arange(lw) + 7) % lk
    assert len(set(pi.tolist())) == lw and not torch.equal(pi, torch.arange(lw))
    assert lk != lw or not torch.equal(pi[pi], torch.arange(lw))                    # not its own inverse: P and P^T differ
    qw = 128.0 * code[:, :, pi]                                                     # [B, K^2, Lw, C]
    scores = qw.double() @ code.double().transpose(-1, -2) / c ** 0.5
    win = scores.gather(-1, pi.view(1, 1, lw, 1).expand(b, nw, lw, 1))
    rest = scores.scatter(-1, pi.view(1, 1, lw, 1).expand(b, nw, lw, 1), float("-inf")).amax(-1, keepdim=True)
    assert (win - rest).min().item() > 200.0
    q = torch.empty(b, h * w, c)
    q[:, tok.reshape(-1)] = qw.reshape(b, nw * lw, c)
    k4, v4 = torch.empty(b, mm, h * w, c), torch.empty(b, mm, h * w, c)
    for src, dst in ((code, k4), (vals, v4)):                                       # key j = p m + u is token tok[p] of view u
        dst[:, :, tok.reshape(-1)] = src.reshape(b, nw, lw, mm, c).permute(0, 3, 1, 2, 4).reshape(b, mm, nw * lw, c)
    want = torch.empty(b, h * w, c)
    want[:, tok.reshape(-1)] = vals[:, :, pi].reshape(b, nw * lw, c)
    k4, v4 = (t if m else t[:, 0] for t in (k4, v4))
    out = wa.window_attention(q.to(DEV), k4.to(DEV), v4.to(DEV), height=h, width=w, num_splits=ksp, with_shift=shift, precision="high")
    assert torch.equal(out.cpu(), want)


def test_highest_is_the_call_without_the_keyword_and_high_is_not():
    (q, k, v, g), _, _, _, high = _run("multi", True, 1.0, "reference")
    plain = _native("multi", q, k, v, g, True, "reference")
    highest = _native("multi", q, k, v, g, True, "reference", precision="highest")
    assert all(torch.equal(x, y) for x, y in zip(plain, highest))
    assert all(not torch.equal(x, y) for x, y in zip(plain, high))


@pytest.mark.parametrize("name,shift", [("multi", True), ("long", True), ("ragged", False)])
def test_forward_and_backward_are_deterministic(name, shift):
    (q, k, v, g), _, _, _, got = _run(name, shift, 1.0, "reference")
    again = _native(name, q, k, v, g, shift, "reference", precision="high")
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _native(name, q, k, v, g, shift, "reference", precision="high")
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, False, True), (False, True, False)])
def test_partial_gradients(needs):
    (q, k, v, g), _, _, _, got = _run("multi", True, 1.0, "reference")
    part = _native("multi", q, k, v, g, True, "reference", needs=needs, precision="high")
    assert torch.equal(part[0], got[0])
    for need, x, full in zip(needs, part[1:], got[1:]):
        assert (x is None) if not need else torch.equal(x, full)
    b, m, h, w, ksp, c = SHAPES["multi"]
    opts = dict(height=h, width=w, num_splits=ksp, with_shift=True, precision="high")
    out, lse = wa.attention_forward(q, k, v, **opts)
    low = wa.attention_backward(q, k, v, lse, g, needs=needs, **opts)
    assert lse.dtype == torch.float64 and tuple(lse.shape) == (b, h * w) and torch.equal(out, got[0])
    for need, x, full in zip(needs, low, got[1:]):
        assert (x is None) if not need else torch.equal(x, full)


@pytest.mark.parametrize("name,shift", [("ragged", True), ("multi", True), ("long", False)])
def test_large_logits_stay_finite_and_inside_the_hull_of_v(name, shift):
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=30.0, seed=5, device=DEV)
    got = _native(name, q, k, v, g, shift, "reference", precision="high")
    assert all(torch.isfinite(t).all() for t in got)
    tok, _ = R.window_index(h, w, ksp, shift, DEV)
    k4 = v if v.dim() == 4 else v.unsqueeze(1)
    vw = k4[:, :, tok]                                                              # [B, m, K^2, Lw, C]
    wlo, whi = vw.amin(dim=(1, 3)), vw.amax(dim=(1, 3))                             # [B, K^2, C]: the window's own hull
    ow = got[0][:, tok]                                                             # [B, K^2, Lw, C]
    excess = torch.maximum(ow - whi.unsqueeze(2), wlo.unsqueeze(2) - ow).max().item()
    slack = 2.0 ** -16 * v.abs().max().item()                                       # the split of v (the module's docstring)
    print(f"{name}: largest excess over the window's hull {excess:.3e}, the split's slack {slack:.3e}")
    assert excess <= slack


def test_no_host_synchronisation():
    (q, k, v, g), _, _, _, got = _run("multi", True, 1.0, "reference")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _native("multi", q, k, v, g, True, "reference", precision="high")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def _peak_delta(fn):
    """Peak bytes REQUESTED from the allocator during fn() (requested_bytes of torch.cuda.memory_stats).  allocated_bytes counts
    whole blocks, and the allocator hands out a cached block whole when the remainder would be 1 MiB or less: at `long`, where q
    is 1 MiB, that is a figure about which blocks earlier tests left free (measured: the 3 MiB scratch counted as 4)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_stats(DEV)["requested_bytes.all.current"]
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.memory_stats(DEV)["requested_bytes.all.peak"] - base, out


def test_scratch_stays_within_twice_the_operands():
    for name, (b, m, h, w, ksp, c) in SHAPES.items():
        nq, nk = 4 * b * h * w * c, 4 * b * max(m, 1) * h * w * c
        fwd, bwd = (wa.scratch_bytes(b, m, h, w, c, ksp, back) for back in (False, True))
        print(f"{name}: scratch {fwd} / {bwd} bytes, operands {nq + 2 * nk} / {2 * nq + 2 * nk}")
        assert 0 < fwd <= 2 * (nq + 2 * nk) and fwd < bwd <= 2 * (2 * nq + 2 * nk), name


def test_memory_is_today_s_bound_plus_the_scratch():
    """`long`: q is 1 MiB.  Today's bounds ("highest": the forward allocates out and lse, < 2 q; the backward three gradients and
    Delta, < 5 q) plus the two scratch figures."""
    b, m, h, w, ksp, c = SHAPES["long"]
    q, k, v, g = (t.requires_grad_(i < 3) for i, t in enumerate(R.random_case(b, m, h, w, c=c, seed=3, device=DEV)))
    nbytes = q.numel() * 4
    s_fwd, s_bwd = (wa.scratch_bytes(b, m, h, w, c, ksp, back) for back in (False, True))

    def forward():
        return wa.window_attention(q, k, v, height=h, width=w, num_splits=ksp, with_shift=True, precision="high")

    forward().backward(g)                                                           # warm-up
    q.grad = k.grad = v.grad = None
    fwd, out = _peak_delta(forward)
    bwd, _ = _peak_delta(lambda: out.backward(g))
    print(f"forward peak {fwd / nbytes:.3f} q (scratch {s_fwd / nbytes:.3f} q), backward peak {bwd / nbytes:.3f} q (scratch {s_bwd / nbytes:.3f} q)")
    assert fwd < 2 * nbytes + s_fwd and bwd < 5 * nbytes + s_bwd
    assert torch.isfinite(q.grad).all() and torch.isfinite(k.grad).all() and torch.isfinite(v.grad).all()


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


def test_seam_follows_torch_s_setting_at_call_time(standin, monkeypatch):
    mod = standin
    (q, k, v, g), _, _, _, high = _run("multi", True, 1.0, "reference")
    highest = _native("multi", q, k, v, g, True, "reference")
    b, m, h, w, ksp, c = SHAPES["multi"]
    launches = []
    forward = wa.attention_forward
    monkeypatch.setattr(wa, "attention_forward", lambda *a, **kw: launches.append(kw.get("precision")) or forward(*a, **kw))
    plugin.install(lazy=True, window_attention=True, window_attention_precision="torch")

    def through_the_layer():
        qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = mod.layer(qq, kk, vv, h, w, ksp, True)
        out.backward(g)
        return out.detach(), qq.grad, kk.grad, vv.grad

    before = torch.get_float32_matmul_precision()
    try:
        torch.set_float32_matmul_precision("high")
        seam_high = through_the_layer()
        torch.set_float32_matmul_precision("highest")
        seam_highest = through_the_layer()
    finally:
        torch.set_float32_matmul_precision(before)
    assert launches == ["high", "highest"] and [c[0] for c in mod.calls] == []       # each kernel once; the replaced function never
    assert all(torch.equal(x, y) for x, y in zip(seam_high, high))
    assert all(torch.equal(x, y) for x, y in zip(seam_highest, highest))


def test_null_and_short_scratch_are_refused_and_write_nothing():
    (q, k, v, g), _, _, _, got = _run("multi", True, 1.0, "reference")
    b, m, h, w, ksp, c = SHAPES["multi"]
    lib = _lib.lib()
    out, g_q = torch.full_like(q, 7.0), torch.full_like(q, 7.0)
    lse = torch.full((b, h * w), 7.0, dtype=torch.float64, device=DEV)
    delta, lse_in = torch.full_like(lse, 7.0), torch.zeros_like(lse)
    dims = (b, m, h, w, c, ksp, 1, 0)
    p = _call.ptr
    with torch.cuda.device(DEV):
        st = _call.stream(torch.device(DEV))
        for back in (False, True):
            need = wa.scratch_bytes(b, m, h, w, c, ksp, back)
            scratch = torch.full((need,), 7, dtype=torch.uint8, device=DEV)
            for sp, size, code in ((None, need, -1), (p(scratch), need - 1, -2), (C.c_void_p(scratch.data_ptr() + 2), need, -1)):
                if back:
                    rc = lib.s360_window_attention_high_backward(p(q), p(k), p(v), p(lse_in), p(g), *dims, p(delta), p(g_q),
                                                                 None, None, sp, size, st)
                else:
                    rc = lib.s360_window_attention_high_forward(p(q), p(k), p(v), *dims, p(out), p(lse), sp, size, st)
                assert rc == code, (back, size, rc)
            torch.cuda.synchronize()
            assert scratch.eq(7).all()
    assert out.eq(7.0).all() and lse.eq(7.0).all() and delta.eq(7.0).all() and g_q.eq(7.0).all()
