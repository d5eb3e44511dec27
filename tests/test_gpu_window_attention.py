"""The fused window attention on the GPU (csrc/s360_window_attention.hip through splatter360_amd/window_attention.py) against the
float64 statement of tests/window_attention_reference.py, with the reference's float32 lines on the same GPU and inputs as the
yardstick.

Accuracy rule (the project's, tests/test_gpu_depth_head.py): for each of out, g_q, g_k, g_v over all elements, the kernel's max
and mean absolute error against statement(float64) are <= max(1.5 x the same figure of reference_lines(float32), 2^-24 max|want|).

Measured on one MI355X (33 cases x 4 tensors: 132 maxima and 132 means): the kernels' maxima are 0.07 to 0.98 x the float32
lines', their means 0.17 to 0.93 x.  The scores and dP are summed in float64 over float32 chains of 8 channels; with one float32
chain over all channels, or four added pairwise, the means were at parity and four maxima missed the bound (1.51 to 1.66 x).
"""
import functools
import sys

import pytest
import torch

import window_attention_reference as R
from splatter360_amd import plugin, window_attention as wa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: (B, m, h, w, K, C)
SHAPES = {
    "tile": (2, 0, 8, 16, 2, 128),        # Lw = 32: exactly one MFMA tile
    "ragged": (1, 0, 10, 14, 2, 128),     # Lw = 35: one row past a tile; odd window, shifts 2 and 3
    "tiles3": (2, 1, 16, 24, 2, 128),     # Lw = 96; a 4-D k with m = 1
    "multi": (2, 3, 8, 12, 2, 128),       # Lk = 72: the (p, u) key order and both mask rules
    "k1": (2, 0, 4, 5, 1, 128),           # no shift, through full_attention
    "c32": (1, 2, 8, 8, 2, 32),
    "long": (1, 0, 32, 64, 2, 128),       # Lw = 512: many key tiles, the running maximum moves
    "k4": (1, 1, 16, 16, 4, 128),         # sixteen windows
}
RUNS = [(name, shift, scale, rule) for name, s in SHAPES.items() for shift in ((False, True) if s[4] > 1 else (False,))
        for scale in (1.0, 6.0) for rule in (("reference", "aligned") if name == "multi" and shift else ("reference",))]
NAMES = ("out", "g_q", "g_k", "g_v")


def _native(name, q, k, v, g, shift, rule, needs=(True, True, True)):
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v = (t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), needs))
    if name == "k1":
        out = wa.full_attention(q, k, v)
    else:
        out = wa.window_attention(q, k, v, height=h, width=w, num_splits=ksp, with_shift=shift, mask_rule=rule)
    out.backward(g)
    return out.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def _run(name, shift, scale, rule):
    """Inputs, the float64 statement, the float32 lines and the kernels' results of one case: computed once, shared, never
    modified."""
    b, m, h, w, ksp, c = SHAPES[name]
    seed = 1000 + 7 * sorted(SHAPES).index(name) + int(shift)
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=scale, seed=seed, device=DEV)
    want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, ksp, shift, h, w, rule), q, k, v, g, torch.float64)
    mask = R.dense_mask(h, w, ksp, DEV) if shift else None
    lines = R.gradients(lambda a, bb, cc: R.reference_lines(a, bb, cc, ksp, shift, h, w, mask, rule=rule), q, k, v, g)
    got = _native(name, q, k, v, g, shift, rule)
    return (q, k, v, g), want, lines, got


def _errors(x, want):
    e = (x.double() - want).abs()
    return e.max().item(), e.mean().item()


def _check_rule(tag, want, lines, got):
    failures = []
    for n, w64, l32, x in zip(NAMES, want, lines, got):
        assert x.dtype == torch.float32 and x.shape == w64.shape, (tag, n)
        (kmax, kmean), (lmax, lmean) = _errors(x, w64), _errors(l32, w64)
        floor = 2.0 ** -24 * w64.abs().max().item()
        print(f"{tag} {n}: kernel max {kmax:.3e} mean {kmean:.3e} | float32 lines max {lmax:.3e} mean {lmean:.3e} | floor {floor:.3e}")
        if not (kmax <= max(1.5 * lmax, floor) and kmean <= max(1.5 * lmean, floor)):
            failures.append((n, kmax, kmean, lmax, lmean, floor))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("name,shift,scale,rule", RUNS)
def test_accuracy_against_the_float64_statement(name, shift, scale, rule):
    _, want, lines, got = _run(name, shift, scale, rule)
    _check_rule(f"{name} shift={int(shift)} scale={scale:g} {rule}", want, lines, got)


def test_the_mask_is_finite():
    """Scores of about +-200 (q, k randn * 7.7: the score's deviation is 59), with shift: rows exist whose unmasked scores all lie
    more than 100 below a masked key's, and there the masked key dominates.  The result follows the float64 statement with the
    finite -100 under the same accuracy rule, and is far from the statement with -inf."""
    name, shift = "tiles3", True
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=7.7, seed=77, device=DEV)
    want = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, ksp, shift, h, w), q, k, v, g, torch.float64)
    minus_inf = R.statement(q, k, v, ksp, shift, h, w, mask_value=float("-inf"))
    assert (minus_inf - want[0]).abs().max().item() > 0.5                          # the case tells the two conventions apart
    mask = R.dense_mask(h, w, ksp, DEV)
    lines = R.gradients(lambda a, bb, cc: R.reference_lines(a, bb, cc, ksp, shift, h, w, mask), q, k, v, g)
    got = _native(name, q, k, v, g, shift, "reference")
    _check_rule("finite mask", want, lines, got)
    assert (got[0].double() - want[0]).abs().max().item() < 1e-2 * (minus_inf - want[0]).abs().max().item()


@pytest.mark.parametrize("name,shift", [("ragged", True), ("multi", True), ("long", False)])
def test_large_logits_stay_finite_and_inside_the_hull_of_v(name, shift):
    b, m, h, w, ksp, c = SHAPES[name]
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=30.0, seed=5, device=DEV)
    got = _native(name, q, k, v, g, shift, "reference")
    assert all(torch.isfinite(t).all() for t in got)
    # every window's keys are a subset of the batch element's rows of v: the hull of all of them contains the window's
    vv = v.reshape(b, -1, c)
    lo, hi = vv.min(dim=1, keepdim=True)[0], vv.max(dim=1, keepdim=True)[0]
    tok, _ = R.window_index(h, w, ksp, shift, DEV)
    k4 = v if v.dim() == 4 else v.unsqueeze(1)
    vw = k4[:, :, tok]                                                              # [B, m, K^2, Lw, C]
    wlo, whi = vw.amin(dim=(1, 3)), vw.amax(dim=(1, 3))                             # [B, K^2, C]: the window's own hull
    ow = got[0][:, tok]                                                             # [B, K^2, Lw, C]
    excess = torch.maximum(ow - whi.unsqueeze(2), wlo.unsqueeze(2) - ow).max().item()
    print(f"{name}: largest excess over the window's hull {excess:.3e}")
    assert excess <= 0.0 and (got[0] >= lo).all() and (got[0] <= hi).all()


def test_a_four_dimensional_k_with_one_partner_is_the_squeezed_k():
    (q, k, v, g), _, _, got = _run("tiles3", True, 1.0, "reference")
    assert k.dim() == 4 and k.shape[1] == 1
    b, m, h, w, ksp, c = SHAPES["tiles3"]
    q, k3, v3 = (t.detach().clone().requires_grad_(True) for t in (q, k[:, 0], v[:, 0]))
    out = wa.window_attention(q, k3, v3, height=h, width=w, num_splits=ksp, with_shift=True)
    out.backward(g)
    assert torch.equal(out, got[0]) and torch.equal(q.grad, got[1])
    assert torch.equal(k3.grad, got[2][:, 0]) and torch.equal(v3.grad, got[3][:, 0])


@pytest.mark.parametrize("name", ["tiles3", "ragged"])
def test_mask_rules_give_the_same_bits_at_one_partner(name):
    (q, k, v, g), _, _, got = _run(name, True, 1.0, "reference")
    again = _native(name, q, k, v, g, True, "aligned")
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_mask_rules_differ_at_three_partners():
    ref, ali = _run("multi", True, 1.0, "reference")[3], _run("multi", True, 1.0, "aligned")[3]
    assert (ref[0] - ali[0]).abs().max().item() > 0.1


@pytest.mark.parametrize("name,shift", [("multi", True), ("long", True), ("ragged", False)])
def test_forward_and_backward_are_deterministic(name, shift):
    (q, k, v, g), _, _, got = _run(name, shift, 1.0, "reference")
    for _ in range(3):
        again = _native(name, q, k, v, g, shift, "reference")
        assert all(torch.equal(x, y) for x, y in zip(got, again))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        again = _native(name, q, k, v, g, shift, "reference")
    side.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, again))


def test_no_host_synchronisation():
    (q, k, v, g), _, _, got = _run("multi", True, 1.0, "reference")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _native("multi", q, k, v, g, True, "reference")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(got, again))


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, False, True), (False, True, False)])
def test_partial_gradients(needs):
    (q, k, v, g), _, _, got = _run("multi", True, 1.0, "reference")
    part = _native("multi", q, k, v, g, True, "reference", needs=needs)
    assert torch.equal(part[0], got[0])
    for need, x, full in zip(needs, part[1:], got[1:]):
        assert (x is None) if not need else torch.equal(x, full)
    b, m, h, w, ksp, c = SHAPES["multi"]
    out, lse = wa.attention_forward(q, k, v, height=h, width=w, num_splits=ksp, with_shift=True)
    low = wa.attention_backward(q, k, v, lse, g, height=h, width=w, num_splits=ksp, with_shift=True, needs=needs)
    assert lse.dtype == torch.float64 and tuple(lse.shape) == (b, h * w) and torch.equal(out, got[0])
    for need, x, full in zip(needs, low, got[1:]):
        assert (x is None) if not need else torch.equal(x, full)


def test_log_sum_exp_is_the_statement_s():
    (q, k, v, g), _, _, _ = _run("ragged", True, 1.0, "reference")
    b, m, h, w, ksp, c = SHAPES["ragged"]
    _, lse = wa.attention_forward(q, k, v, height=h, width=w, num_splits=ksp, with_shift=True)
    tok, region = R.window_index(h, w, ksp, True, DEV)
    qw, kw = q.double()[:, tok], k.double()[:, tok]
    scores = qw @ kw.transpose(-1, -2) / c ** 0.5 + torch.where(region.unsqueeze(2) != region.unsqueeze(1), R.MASK_VALUE, 0.0)
    want = torch.logsumexp(scores, dim=-1)                                          # [B, K^2, Lw]
    assert (lse[:, tok] - want).abs().max().item() <= 1e-5


def test_dtype_and_shape_errors_on_the_gpu():
    q, k, v, g = R.random_case(1, 0, 4, 8, c=32, seed=1, device=DEV)
    opts = dict(height=4, width=8, num_splits=2)
    with pytest.raises(ValueError, match="float32"):
        wa.window_attention(q.half(), k.half(), v.half(), **opts)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.window_attention(q, k.cpu(), v.cpu(), **opts)
    nc = torch.cat([q, q], dim=-1)[..., :32]                                        # non-contiguous: copied once
    assert not nc.is_contiguous() and torch.equal(wa.window_attention(nc, k, v, **opts), wa.window_attention(q, k, v, **opts))


def _peak_delta(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(DEV) - base, out


def test_memory_stays_of_the_order_of_the_inputs():
    """(1, 0, 64, 128, 2): q is 4.2 MB and one score tensor would be 67 MB.  The forward allocates out and lse (< 2 q), the
    backward three gradients and a float64 Delta per query (< 5 q)."""
    b, m, h, w, ksp, c = 1, 0, 64, 128, 2, 128
    q, k, v, g = (t.requires_grad_(i < 3) for i, t in enumerate(R.random_case(b, m, h, w, c=c, seed=3, device=DEV)))
    nbytes = q.numel() * 4
    assert nbytes == 4 * 1024 * 1024 and 4 * (h * w // 4) ** 2 * 4 == 64 * 1024 * 1024

    def forward():
        return wa.window_attention(q, k, v, height=h, width=w, num_splits=ksp, with_shift=True)

    forward().backward(g)                                                           # warm-up
    q.grad = k.grad = v.grad = None
    fwd, out = _peak_delta(forward)
    bwd, _ = _peak_delta(lambda: out.backward(g))
    print(f"forward peak {fwd / nbytes:.3f} q, backward peak {bwd / nbytes:.3f} q")
    assert fwd < 2 * nbytes and bwd < 5 * nbytes
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


def test_installed_mask_generator_allocates_no_mask(standin):
    plugin.install_window_attention()
    h, w, ksp = 64, 128, 2
    delta, handle = _peak_delta(lambda: standin.generate_shift_window_attn_mask((h, w), h // ksp, w // ksp, h // ksp // 2, w // ksp // 2,
                                                                                device=torch.device(DEV)))
    assert isinstance(handle, wa.ShiftMask) and handle.matches(h, w, ksp) and delta < 1024


@pytest.mark.parametrize("name,shift", [("multi", True), ("tiles3", False), ("k1", False)])
def test_seam_runs_the_kernel_once_and_gives_the_direct_api_s_bits(standin, monkeypatch, name, shift):
    mod = standin
    (q, k, v, g), _, lines, got = _run(name, shift, 1.0, "reference")
    b, m, h, w, ksp, c = SHAPES[name]
    launches = []
    forward = wa.attention_forward
    monkeypatch.setattr(wa, "attention_forward", lambda *a, **kw: launches.append(1) or forward(*a, **kw))
    plugin.install_window_attention()

    def through_the_layer(q, k, v):
        q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = mod.layer(q, k, v, h, w, ksp, shift)
        out.backward(g.to(out.dtype))
        return out.detach(), q.grad, k.grad, v.grad

    mod.calls.clear()
    seam = through_the_layer(q, k, v)
    assert len(launches) == 1 and mod.calls == []                                   # the kernel, once; the replaced function, never
    assert all(torch.equal(x, y) for x, y in zip(seam, got))
    # half precision falls back to the replaced function, with a dense mask
    half = through_the_layer(q.half(), k.half(), v.half())
    assert len(launches) == 1 and len(mod.calls) == 1 and half[0].dtype == torch.float16
    assert mod.calls[0][1] is None or (isinstance(mod.calls[0][1], torch.Tensor) and mod.calls[0][1].is_cuda)
    plugin.uninstall()
    mod.calls.clear()
    torch_again = through_the_layer(q, k, v)
    assert len(launches) == 1 and len(mod.calls) == 1
    if ksp == 1:                                                                    # the layer calls the full-attention lines there
        lines = R.gradients(R.full_lines, q, k, v, g)
    assert all(torch.equal(x, y) for x, y in zip(torch_again, lines))
