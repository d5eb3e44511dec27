"""The native softmax depth head (splatter360_amd/depth_head.py, csrc/s360_depth_head.hip) on the GPU against the float64
statement of tests/depth_head_reference.py.

Accuracy rule (the project's "as close to float64 as the float32 statement is", tests/test_gpu_cost_volume.py): for each of depth,
pdf_max and the gradient of the logits (random g_depth and g_pmax), over ALL elements, the kernel's max and mean absolute error
against float64 are <= max(1.5 x the same figure of the torch float32 statement on the same GPU and inputs, 2^-24 max|want|).  The
floor is half a float32 ulp of the largest value: a correctly rounded result cannot fail where torch happens to be exact.

Measured on an MI355X at the hm3d shape (2 x 128 x 128 x 256), logits randn (profiles/depth_head_timing.json, "accuracy"):
depth kernel max 7.0e-08 / mean 1.4e-08, torch float32 8.2e-07 / 9.0e-08; pdf_max kernel 1.4e-08 / 1.5e-09, torch float32
1.7e-07 / 9.2e-09; gradient kernel 5.7e-08 / 7.5e-11, torch float32 4.3e-07 / 1.2e-09.
Call times there, native against the torch statement: forward 40.4 against 167.4 µs, forward + backward 212.7 against
297.8 µs; at D = 32 forward 32.5 against 54.0 µs and forward + backward 207.6 against 150.3 µs (slower: the call is host-bound)."""
import sys

import pytest
import torch

import depth_head_reference as R
from splatter360_amd import cost_volume as cv, depth_head as dh, plugin

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (n, D, h, w): the smallest shapes at which each mechanism can break
SHAPES = {
    "plain": (2, 16, 8, 32),
    "odd": (3, 7, 5, 13),                  # P = 65: one lane past a wave; odd D
    "d1": (1, 1, 4, 4),                    # D = 1: pmax = 1, depth = c, gradient = 0 exactly
    "ragged": (2, 130, 3, 21),             # D no multiple of any split; P no multiple of 4 (the scalar backward)
    "ref_d": (1, 128, 32, 64),             # the reference's D
}
HM3D = (2, 128, 128, 256)
SCALES = (1.0, 30.0)                       # 30: the pdf is nearly one-hot
_CACHE = {}


def _case(shape, scale, sampling):
    """Inputs and the two torch statements of one case, computed once and shared (never modified)."""
    key = (shape, scale, sampling)
    if key not in _CACHE:
        logits, cand, g_depth, g_pmax = R.random_case(shape, scale, sampling, seed=sum(shape) + int(scale) + len(sampling), device=DEV)
        with torch.no_grad():
            want, t32 = R.head(logits, cand, torch.float64), R.head(logits, cand, torch.float32)
        _CACHE[key] = dict(logits=logits, cand=cand, g_depth=g_depth, g_pmax=g_pmax, want=want, t32=t32)
    return _CACHE[key]


def _check(label, got, want, t32):
    """The rule: prints the four figures, then asserts both bars."""
    e_k, e_t = (got.double() - want).abs(), (t32.double() - want).abs()
    floor = 2.0 ** -24 * want.abs().max().item()
    figures = (e_k.max().item(), e_k.mean().item(), e_t.max().item(), e_t.mean().item())
    print(f"{label}: kernel max/mean {figures[0]:.4g} {figures[1]:.4g}; torch f32 max/mean {figures[2]:.4g} {figures[3]:.4g}; floor {floor:.4g}")
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.isfinite(got).all()
    assert figures[0] <= max(1.5 * figures[2], floor) and figures[1] <= max(1.5 * figures[3], floor), (label, figures, floor)


def _native_gradient(logits, cand, g_depth, g_pmax):
    z = logits.clone().requires_grad_(True)
    outs = dh.softmax_depth_head(z, cand)
    pairs = [(o, g) for o, g in zip(outs, (g_depth, g_pmax)) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return z.grad


def _accuracy(name, shape, scale, sampling):
    c = _case(shape, scale, sampling)
    depth, pmax = dh.softmax_depth_head(c["logits"], c["cand"])
    _check(f"{name} x{scale:g} {sampling} depth", depth, c["want"][0], c["t32"][0])
    _check(f"{name} x{scale:g} {sampling} pdf_max", pmax, c["want"][1], c["t32"][1])
    grad = _native_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"])
    want = R.logits_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"], torch.float64)
    t32 = R.logits_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"], torch.float32)
    _check(f"{name} x{scale:g} {sampling} g_logits", grad, want, t32)
    return depth, pmax, grad


@pytest.mark.parametrize("sampling", cv.SAMPLINGS)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_outputs_and_gradient_match_float64_as_closely_as_torch_float32(name, scale, sampling):
    depth, pmax, grad = _accuracy(name, SHAPES[name], scale, sampling)
    if name == "d1":
        c = _case(SHAPES[name], scale, sampling)
        assert (pmax == 1).all() and torch.equal(depth, c["cand"].view(1, 1, 1, 1).expand_as(depth)) and (grad == 0).all()


@pytest.mark.parametrize("scale", SCALES)
def test_hm3d_shape_matches_float64_as_closely_as_torch_float32(scale):
    _accuracy("hm3d", HM3D, scale, "inverse_depth")
    _CACHE.pop((HM3D, scale, "inverse_depth"))                          # 33.5 MB of logits: not kept for the session


def test_large_logits_stay_finite():
    logits, cand, g_depth, g_pmax = R.random_case(SHAPES["ragged"], 1e4, "inverse_depth", seed=11, device=DEV)
    depth, pmax = dh.softmax_depth_head(logits, cand)
    grad = _native_gradient(logits, cand, g_depth, g_pmax)
    assert torch.isfinite(depth).all() and torch.isfinite(pmax).all() and torch.isfinite(grad).all()
    assert (pmax > 0).all() and (pmax <= 1).all()
    lo, hi = cand.min(dim=1)[0].view(-1, 1, 1, 1), cand.max(dim=1)[0].view(-1, 1, 1, 1)
    assert (depth >= lo).all() and (depth <= hi).all()


def test_argmax_is_the_first_maximum():
    c = _case(SHAPES["ragged"], 1.0, "log_depth")
    logits, cand = c["logits"], c["cand"]
    argmax = dh.head_forward(logits, cand)[3]
    assert argmax.dtype == torch.int32 and torch.equal(argmax.long(), logits.argmax(1, keepdim=True))
    top = logits.max().item() + 1.0
    # two equal, largest depths: in one wave's group of loads, in two of its groups, in two waves, at the two ends
    for lo, hi in ((2, 6), (2, 34), (3, 9), (9, 11), (0, 129)):
        tied = logits.clone()
        tied[:, lo] = top
        tied[:, hi] = top
        _, pmax, _, a = dh.head_forward(tied, cand)
        assert (a == lo).all(), (lo, hi)
        with torch.no_grad():
            _check(f"tie {lo} {hi} pdf_max", pmax, R.head(tied, cand, torch.float64)[1], R.head(tied, cand, torch.float32)[1])


@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_forward_and_backward_are_bit_identical_across_runs_and_streams(name):
    c = _case(SHAPES[name], 1.0, "inverse_depth")
    runs = []

    def once():
        depth, pmax = dh.softmax_depth_head(c["logits"], c["cand"])
        runs.append((depth, pmax, _native_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"])))

    for _ in range(3):
        once()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        once()
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for run in runs[1:] for x, y in zip(runs[0], run))


@pytest.mark.parametrize("name", ["plain", "ragged"])
def test_partial_gradients(name):
    """g_depth only, g_pmax only (explicit zeros for the other: what autograd hands when both outputs are used), and one output
    used downstream alone (autograd hands None for the other, which reaches the kernel as a null pointer)."""
    c = _case(SHAPES[name], 30.0, "linear_depth")
    logits, cand, g_depth, g_pmax = c["logits"], c["cand"], c["g_depth"], c["g_pmax"]
    zeros = torch.zeros_like(g_depth)
    for label, gd, gp in (("g_depth only", g_depth, None), ("g_pmax only", None, g_pmax)):
        want = R.logits_gradient(logits, cand, gd, gp, torch.float64)
        t32 = R.logits_gradient(logits, cand, gd, gp, torch.float32)
        with_zeros = _native_gradient(logits, cand, zeros if gd is None else gd, zeros if gp is None else gp)
        with_none = _native_gradient(logits, cand, gd, gp)
        _check(f"{name} {label}, zeros", with_zeros, want, t32)
        _check(f"{name} {label}, None", with_none, want, t32)
        depth, _, lse, argmax = dh.head_forward(logits, cand)
        assert torch.equal(dh.head_backward(logits, cand, lse, depth, argmax, gd, gp), with_none)


def test_no_host_synchronisation_in_forward_and_backward():
    c = _case(SHAPES["plain"], 1.0, "inverse_depth")
    _native_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"])            # warm-up: library load, allocator
    z = c["logits"].clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        depth, pmax = dh.softmax_depth_head(z, c["cand"])
        torch.autograd.backward([depth, pmax], [c["g_depth"], c["g_pmax"]])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_memory_has_no_d_sized_temporary():
    """Forward: the extra peak stays below half the logits' bytes (four [n, h, w] maps).  Backward: below 1.5 x the logits' bytes
    (g_logits plus small tensors)."""
    c = _case(SHAPES["ref_d"], 1.0, "inverse_depth")
    z = c["logits"].clone().requires_grad_(True)
    nbytes = z.numel() * 4
    _native_gradient(c["logits"], c["cand"], c["g_depth"], c["g_pmax"])            # warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    depth, pmax = dh.softmax_depth_head(z, c["cand"])
    torch.cuda.synchronize()
    fwd = torch.cuda.max_memory_allocated(DEV) - base
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    torch.autograd.backward([depth, pmax], [c["g_depth"], c["g_pmax"]])
    torch.cuda.synchronize()
    bwd = torch.cuda.max_memory_allocated(DEV) - base
    print(f"logits {nbytes} B; forward peak delta {fwd} B; backward peak delta {bwd} B")
    assert fwd < 0.5 * nbytes and bwd < 1.5 * nbytes


def test_non_contiguous_logits_and_both_candidate_shapes_give_the_same_bits():
    c = _case(SHAPES["plain"], 1.0, "log_depth")
    logits, cand, g_depth, g_pmax = c["logits"], c["cand"], c["g_depth"], c["g_pmax"]
    want = (*dh.softmax_depth_head(logits, cand), _native_gradient(logits, cand, g_depth, g_pmax))
    channels_last = logits.contiguous(memory_format=torch.channels_last)
    wide = torch.randn(logits.shape[0], logits.shape[1], logits.shape[2], logits.shape[3] + 3, device=DEV)
    wide[..., 1:-2] = logits
    view = wide[..., 1:-2]
    assert not channels_last.is_contiguous() and not view.is_contiguous()
    for z in (channels_last, view):
        got = (*dh.softmax_depth_head(z, cand), _native_gradient(z, cand, g_depth, g_pmax))
        assert all(torch.equal(x, y) for x, y in zip(want, got))
    got = (*dh.softmax_depth_head(logits, cand[:, :, None, None]), _native_gradient(logits, cand[:, :, None, None], g_depth, g_pmax))
    assert all(torch.equal(x, y) for x, y in zip(want, got))


def test_errors():
    logits, cand, _, _ = R.random_case((2, 4, 3, 5), 1.0, "inverse_depth", seed=1, device=DEV)
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits.double(), cand.double())
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits, cand.double())
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits, cand[:1])                          # n
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits, cand[:, :3])                       # D
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits[0], cand)                           # 3-D
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits[:, :, :0], cand)                    # empty
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits[:0], cand[:0])
    with pytest.raises(RuntimeError):
        dh.softmax_depth_head(logits.cpu(), cand.cpu())
    with pytest.raises(RuntimeError):
        dh.softmax_depth_head(logits, cand.cpu())


def test_coarse_depth_head_is_the_head_followed_by_torchs_own_upsampling():
    c = _case(SHAPES["plain"], 1.0, "inverse_depth")
    n, _, h, w = SHAPES["plain"]
    fullres_disps, pdf_max, coarse_depths = dh.coarse_depth_head(c["logits"], c["cand"], 4)
    depth, pmax = dh.softmax_depth_head(c["logits"], c["cand"])
    assert fullres_disps.shape == (n, 1, 4 * h, 4 * w) and pdf_max.shape == (n, 1, 4 * h, 4 * w) and coarse_depths.shape == (n, 1, h, w)
    assert torch.equal(coarse_depths, depth)
    assert torch.equal(pdf_max, torch.nn.functional.interpolate(pmax, scale_factor=4))
    assert torch.equal(fullres_disps, torch.nn.functional.interpolate(1 / depth, scale_factor=4, mode="bilinear", align_corners=True))


def test_installed_seam_runs_the_kernel_once_and_falls_back(monkeypatch):
    c = _case(SHAPES["odd"], 1.0, "inverse_depth")
    logits, cand, g_depth, g_pmax = c["logits"], c["cand"], c["g_depth"], c["g_pmax"]
    c4 = cand[:, :, None, None]
    calls = []
    low_level = dh.head_forward
    monkeypatch.setattr(dh, "head_forward", lambda *a: calls.append(1) or low_level(*a))
    assert plugin.COST_VOLUME_MODULE not in sys.modules
    mod = R.standin_module(plugin.COST_VOLUME_MODULE)
    sys.modules[plugin.COST_VOLUME_MODULE] = mod
    try:
        torchs = mod.depth_head(logits, c4)
        proxy = plugin.install_depth_head()
        assert mod.F is proxy and proxy.replaced is torch.nn.functional
        # the three statements: softmax_depth_head's two tensors, from one run of the low-level forward
        z = logits.clone().requires_grad_(True)
        depth, pmax = mod.depth_head(z, c4)
        assert len(calls) == 1
        direct = dh.softmax_depth_head(logits, cand)
        assert torch.equal(depth, direct[0]) and torch.equal(pmax, direct[1])
        # a loss on both outputs: the direct API's gradient, bit for bit
        torch.autograd.backward([depth, pmax], [g_depth, g_pmax])
        assert torch.equal(z.grad, _native_gradient(logits, cand, g_depth, g_pmax))
        # the indices of torch.max come with the values
        pdf = mod.F.softmax(logits, dim=1)
        assert isinstance(pdf, dh.LazyPdf) and pdf.shape == logits.shape
        coarse = (pdf * c4).sum(1, True)                                                # the other operand order, positional
        both = torch.max(pdf, dim=1, keepdim=True)
        assert torch.equal(coarse, direct[0]) and torch.equal(both.values, direct[1])
        assert both[1].dtype == torch.int64 and torch.equal(both[1], logits.argmax(1, keepdim=True))
        # every other use goes dense and is torch's softmax path
        del calls[:]
        dense = torch.softmax(logits, 1)
        assert torch.equal(mod.F.softmax(logits, dim=1).sum(), dense.sum())
        assert torch.equal(mod.F.softmax(logits, dim=1)[:, 0], dense[:, 0])
        assert torch.equal(torch.max(mod.F.softmax(logits, dim=1), dim=1, keepdim=True)[0], dense.max(1, keepdim=True)[0])     # max first
        flat = mod.depth_head(logits, c4, keepdim=False)
        assert torch.equal(flat[0], (c4 * dense).sum(1)) and torch.equal(flat[1], dense.max(1)[0])
        wrong = mod.depth_head(logits, cand[:, :, None, None].double())                 # float64 candidates: torch's promotion
        assert wrong[0].dtype == torch.float64 and torch.equal(wrong[1], dense.max(1, keepdim=True)[0])
        half = mod.depth_head(logits.half(), c4.half())                                  # AMP halves: the replaced softmax
        assert half[0].dtype == torch.float16
        zd = logits.clone().requires_grad_(True)
        mod.F.softmax(zd, dim=1)[:, 0].sum().backward()                                 # autograd intact on the dense path
        zt = logits.clone().requires_grad_(True)
        torch.softmax(zt, 1)[:, 0].sum().backward()
        assert torch.equal(zd.grad, zt.grad)
        assert calls == []
        plugin.uninstall()
        assert mod.F is torch.nn.functional
        again = mod.depth_head(logits, c4)
        assert torch.equal(again[0], torchs[0]) and torch.equal(again[1], torchs[1]) and calls == []
    finally:
        plugin.uninstall()
        del sys.modules[plugin.COST_VOLUME_MODULE]
