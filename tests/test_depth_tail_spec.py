"""The fine-depth and opacity tail's CPU-checkable parts: the statement of tests/depth_tail_reference.py against the closed form
the backward kernel evaluates, how often float32 and float64 disagree on the clamp, the float32 statement's NaN gradient at
saturated logits (why the kernel differentiates in the logit), and the C ABI's six new symbols.  The install seam is in
tests/test_depth_tail_install.py, the GPU half in tests/test_gpu_depth_tail.py."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import depth_tail_reference as R
from splatter360_amd import _lib, depth_tail as dt

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("s360_upsample_forward", "s360_upsample_backward", "s360_depth_tail_forward", "s360_depth_tail_backward",
         "s360_opacity_map_forward", "s360_opacity_map_backward")


@pytest.mark.parametrize("exponent", [1.0, 4.0, 0.5])
def test_closed_form_gradient_in_the_logit_is_the_statements_autograd_gradient(exponent):
    """float64 autograd of sigmoid -> map_pdf_to_opacity -> / gpp equals (e (1 - p)^e p + (1 / e) p^(1 / e) (1 - p)) / (2 gpp),
    and torch.autograd.gradcheck accepts the statement, on a 2 x 3 x 5 case."""
    gen = torch.Generator().manual_seed(5)
    x = (3.0 * torch.randn(2, 3, 5, generator=gen, dtype=torch.float64)).requires_grad_(True)
    for gpp in (1, 2):
        def statement(z):
            return R.map_pdf_to_opacity(torch.sigmoid(z), exponent) / gpp

        (auto,) = torch.autograd.grad(statement(x).sum(), x)
        want = R.opacity_logit_slope(x.detach(), exponent, gpp)
        assert (auto - want).abs().max().item() <= 1e-14 * max(1.0, want.abs().max().item())
        assert torch.autograd.gradcheck(statement, (x,))


def test_whole_tail_statement_passes_gradcheck():
    fullres, dd, near, far, *_ = R.random_case(1, 2, 3, 5, 1, seed=9)

    def statement(f, d):
        return R.tail(f, d, near, far, 1, 4.0, torch.float64)

    f, d = fullres.double().requires_grad_(True), dd.double().requires_grad_(True)
    total, lo, hi = R.tail_planes(fullres, dd, near, far, 1, 4.0)[3:]
    assert ((total - lo).abs().min().item() > 1e-4) and ((total - hi).abs().min().item() > 1e-4)     # no element sits on the kink
    assert torch.autograd.gradcheck(statement, (f, d))


def test_float32_and_float64_take_the_same_clamp_decision_on_the_random_case():
    """The cap the GPU test relies on: at most 0.1 % of the elements may differ."""
    fullres, dd, near, far, *_ = R.random_case(2, 2, 32, 128, 1, seed=1)
    t64, lo64, hi64 = R.tail_planes(fullres, dd, near, far, 1, 1.0, torch.float64)[3:]
    t32, lo32, hi32 = R.tail_planes(fullres, dd, near, far, 1, 1.0, torch.float32)[3:]
    p64, p32 = R.clamp_pass(t64, lo64, hi64), R.clamp_pass(t32, lo32, hi32)
    differ = (p64 != p32).sum().item()
    print(f"clamp decisions that differ: {differ} of {p64.numel()}")
    assert p64.numel() == 16384 and differ <= 0.001 * p64.numel()
    assert 0.05 < (~p64).float().mean().item() < 0.5 and (t64 < lo64).any() and (t64 > hi64).any()    # both sides are exercised


@pytest.mark.parametrize("x, exponent", [(-120.0, 4.0), (120.0, 0.5)])
def test_float32_statement_has_a_nan_gradient_at_saturated_logits(x, exponent):
    """sigmoid rounds to exactly 0 or 1 in float32; pow's derivative is infinite there and meets sigmoid' = 0.  The closed form in
    the logit is finite at the same point."""
    z = torch.tensor([x], dtype=torch.float32, requires_grad=True)
    R.map_pdf_to_opacity(torch.sigmoid(z), exponent).sum().backward()
    assert torch.isnan(z.grad).all()
    slope = R.opacity_logit_slope(torch.tensor([x], dtype=torch.float64), exponent)
    assert torch.isfinite(slope).all() and slope.item() >= 0


def test_opacity_exponent_is_the_references_expression():
    for initial, final, warm_up, step in ((0.0, 0.0, 1, 0), (0.0, 2.0, 1000, 250), (-1.0, 3.0, 10, 50), (2.0, -1.0, 3, 1)):
        x = initial + min(step / warm_up, 1) * (final - initial)
        assert dt.opacity_exponent(initial, final, warm_up, step) == 2 ** x


def test_abi_has_the_depth_tail_entry_points_and_they_reject_bad_arguments():
    lib = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header)
    assert "s360_depth_tail.hip" in _lib.SOURCES and (ROOT / "splatter360_amd" / "csrc" / "s360_depth_tail.hip").exists()
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25                  # additive: the version stays
    p = C.c_void_p(16)                                                              # never dereferenced: every call below is refused
    nan, inf = float("nan"), float("inf")
    up_f, up_b = lib.s360_upsample_forward, lib.s360_upsample_backward
    assert up_f(None, p, 2, 8, 8, 4, 1, 0, None) == -1 and up_f(p, None, 2, 8, 8, 4, 1, 0, None) == -1
    for n, h, w, s, mode in ((0, 8, 8, 4, 1), (2, 0, 8, 4, 1), (2, 8, -1, 4, 0), (2, 8, 8, 0, 1), (2, 8, 8, -2, 0), (2, 8, 8, 4, 2),
                             (2, 8, 8, 4, -1), (2, 1 << 15, 1 << 15, 4, 0)):
        assert up_f(p, p, n, h, w, s, mode, 0, None) == -1 and up_b(p, p, p, n, h, w, s, mode, 1, None) == -1
    assert up_b(None, p, p, 2, 8, 8, 4, 1, 0, None) == -1 and up_b(p, p, None, 2, 8, 8, 4, 1, 0, None) == -1
    assert up_b(p, None, p, 2, 8, 8, 4, 1, 1, None) == -1                           # reciprocal needs src
    tf, tb = lib.s360_depth_tail_forward, lib.s360_depth_tail_backward
    good = dict(e=1.0, gpp=1, v=2, n=4, H=8, W=8)

    def forward(ptrs=(p, p, p, p, p, p, p), **kw):
        a = {**good, **kw}
        return tf(*ptrs[:4], a["e"], a["gpp"], a["v"], *ptrs[4:], a["n"], a["H"], a["W"], None)

    def backward(ptrs=(p,) * 9, **kw):
        a = {**good, **kw}
        return tb(*ptrs[:7], a["e"], a["gpp"], a["v"], *ptrs[7:], a["n"], a["H"], a["W"], None)

    for bad in (dict(e=0.0), dict(e=-1.0), dict(e=nan), dict(e=inf), dict(gpp=0), dict(gpp=-1), dict(v=0), dict(v=3), dict(n=0),
                dict(H=0), dict(W=-4), dict(H=1 << 15, W=1 << 15)):
        assert forward(**bad) == -1 and backward(**bad) == -1, bad
    for i in range(6):                                                              # densities_out (index 6) may be null
        assert forward(ptrs=tuple(None if j == i else p for j in range(7))) == -1, i
    for i in range(3, 9):                                                           # the three incoming gradients may be null
        assert backward(ptrs=tuple(None if j == i else p for j in range(9))) == -1, i
    of, ob = lib.s360_opacity_map_forward, lib.s360_opacity_map_backward
    assert of(None, p, 8, 1.0, None) == -1 and of(p, None, 8, 1.0, None) == -1
    assert ob(None, p, p, 8, 1.0, None) == -1 and ob(p, None, p, 8, 1.0, None) == -1 and ob(p, p, None, 8, 1.0, None) == -1
    for count, e in ((0, 1.0), (-3, 1.0), (8, 0.0), (8, -2.0), (8, nan), (8, inf)):
        assert of(p, p, count, e, None) == -1 and ob(p, p, p, count, e, None) == -1


def test_python_layer_refuses_what_it_cannot_run():
    fullres, dd, near, far, *_ = R.random_case(1, 2, 4, 8, 1, seed=1)
    depth, pmax, *_ = R.random_maps(2, 3, 5, 4, seed=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        dt.upsample(depth, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        dt.fullres_maps(depth, pmax, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        dt.fine_depth_tail(fullres, dd, near, far, views=2)
    with pytest.raises(RuntimeError, match="GPU only"):
        dt.map_pdf_to_opacity(pmax, 2.0)
    with pytest.raises(ValueError):
        dt.upsample(depth, 1.5)
    with pytest.raises(ValueError):
        dt.upsample(depth, 0)
    with pytest.raises(ValueError):
        dt.upsample(depth, 2, mode="bicubic")
    with pytest.raises(ValueError):
        dt.upsample(depth[0], 2)
    with pytest.raises(ValueError):
        dt.upsample(depth.expand(2, 3, 3, 5), 2)
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres[0], dd, near, far, views=2)
