"""The fine-depth and opacity tail, the upsampling and the opacity map (csrc/s360_depth_tail.hip) held to float64 PER ELEMENT.
tests/test_gpu_depth_tail.py pools each tensor into one maximum and one mean, leaves out the elements where float64 and float32
decide the clamp differently, and takes torch's float64 1 - (1 - sigmoid(x)) ** e as the opacity's `want`, which keeps no digit
of 1 - p from |x| = 37 on and so cannot judge the kernel where it is most careful; its logits (3 N(0, 1)) never get there.  Here
every element of every output and gradient is measured against its own bound

    |got - want| <= 2^-24 |want| + 2^-40 A + 2^-149

with `want` from depth_tail_reference (opacity_elements: a float64 form without cancellation, pinned against 200-bit arithmetic
by tests/test_depth_tail_elements.py; upsample_elements: numpy from exact integer taps; tail_elements: the clamp's pattern from
the float32 sum in numpy, the kernel's stated contract, so NO element is left out) and A the sum of the magnitudes of the element's
terms.  Nearest upsampling is held to bit equality.  Logits 3 N(0, 1) with +-17.5, +-20, +-40, +-88 and +-100 planted; fullres +
delta planted exactly on lo and hi, one float32 ulp on either side of each, and a quarter ulp off each in float64 only.

Every run goes through the C ABI into NaN-filled buffers between sentinels, once 16-byte aligned and once with every float
pointer shifted by one float (the scalar kernels even where the float4 ones would run), and shows: the kernels write all they own
and nothing else; aligned and shifted runs give the same bits; the Python layer gives the ABI's bits.  Each prints
`[dt64] case quantity kernel / torch-float32` (pytest -s; the float32 figure is for the reader, not a bound; nan where torch's
float32 autograd gives NaN) and, with S360_ACCURACY_REPORT=<file>, merges its figures into that file
(profiles/depth_head_tail_float64_accuracy.json).

Measured on one MI355X (69 runs: 30 upsamplings, 24 tails, 15 opacity maps; worst element in bounds, kernel / torch float32
statement; profiles/depth_head_tail_float64_accuracy.json):

    quantity              kernel            torch float32          the case of the largest kernel figure
    upsample out          0.000 to 0.999    0 to 63.3              up/wave/bilinear/recip
    upsample g_src        0.000 to 0.986    0 to 3.45e+04          up/h1/bilinear/recip
    tail depths           0.375 to 1.000    0.375 to 1.41          tail/vec_gpp2
    tail opacities        0.053 to 0.992    0.053 to 1.68e+07      tail/gpp2/e4
    tail densities        0.421 to 0.972    0.421 to 26.6          tail/batch/e4
    tail g_fullres        0.000 to 0.969    0 to 821               tail/gpp2
    tail g_delta (disp.)  0.000 to 0.968    0 to 3.53              tail/gpp2
    tail g_delta (logit)  0.000 to 0.988    0 to 1.68e+07, NaN     tail/batch/e0.5
    opacity map out       0.000 to 0.957    0 to 323               map/n1027/e4
    opacity map g_pdf     0.000 to 0.985    0 to 3.59              map/n1027/e0.5

(1.000 is 0.99999...: depths are one rounding of 1 / fine.  1.68e+07 is 2^24: float32's sigmoid has rounded to 0 or 1 and the
statement's opacity is off by all of itself; its autograd gives NaN in 12 of the 24 tail runs.)  Found by this file: nothing; every
run passes with the kernels as they were, every buffer is fully written with its sentinels intact, aligned and shifted runs agree
bit for bit, the pattern of zeros of the disparity gradient is the float32 sum's at every planted sum, and the gradient of the
opacity map at p = 1 with e = 0.5 is the statement's infinity with its sign.

Planted on a scratch build, arithmetic only (never an index): expm1(e * lq) replaced by exp(e * lq) - 1 in dt_opacity fails 11
of this file's tests — every tail case at e = 1 and e = 0.5 but `single`, and the three null-gradient cases; opacities 2^24 bounds:
all of the value — and passes all 65 tests of the pooled file.  At e = 4 it changes no float32 digit (the root p^(1 / 4) is 1e22
times the lost term at x = -100), as tests/test_depth_tail_elements.py works out.
"""
import ctypes as C
import functools
import json
import math
import os
from pathlib import Path

import pytest
import torch

import depth_tail_reference as R
from splatter360_amd import _lib, depth_tail as dt
from test_gpu_depth_head_float64 import DEV, _assert_owned, _guarded, _placed

pytestmark = pytest.mark.gpu
# (n, h, w, s) and (b, v, H, W, gpp): tests/test_gpu_depth_tail.py's, and gpp = 2 with P % 4 == 0 (float4 loads, scalar channel-last stores)
UP_SHAPES = {"cell": (1, 2, 2, 4), "odd": (2, 3, 5, 4), "h1": (1, 1, 7, 2), "s1": (1, 4, 4, 1), "s3": (3, 5, 13, 3), "wave": (1, 9, 33, 4)}
TAIL_SHAPES = {"two_views": (1, 2, 4, 8, 1), "batch": (2, 2, 5, 13, 1), "gpp2": (1, 3, 3, 21, 2), "single": (1, 1, 1, 1, 1),
               "vec_gpp2": (1, 2, 2, 6, 2)}
EXPONENTS = (1.0, 4.0, 0.5)
MODES = ("nearest", "bilinear")
MAP_LENGTHS = (1, 3, 4, 5, 1027)
REPORT = {}
WHAT = ("tests/test_gpu_depth_tail_float64.py on an MI355X: the upsampling, the fine-depth and opacity tail and the opacity map per "
        "element against float64; worst |got - want| / (2^-24 |want| + 2^-40 A + 2^-149) per quantity, kernel / torch float32 statement "
        "(bound: kernel <= 1; nan: the float32 statement's autograd gives NaN).")


def _report(key, fig):
    """Keep the case's figures; with S360_ACCURACY_REPORT=<file> in the environment merge them into that file (shared with
    tests/test_gpu_depth_head_float64.py: how profiles/depth_head_tail_float64_accuracy.json is made)."""
    REPORT[key] = fig
    path = os.environ.get("S360_ACCURACY_REPORT")
    if path:
        p = Path(path)
        old = json.loads(p.read_text()) if p.exists() else {}
        p.write_text(json.dumps(dict(what={**old.get("what", {}), "dt64": WHAT}, cases={**old.get("cases", {}), **REPORT}), indent=1, sort_keys=True))


def _ptr(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _judge(tag, got, want, cond, t32):
    """Prints and records kernel / torch-float32 for each quantity, then asserts kernel <= 1."""
    fig, failures = {}, []
    for q in got:
        assert got[q].dtype == torch.float32 and got[q].shape == want[q].shape, (tag, q)
        kern = R.worst(got[q].cpu(), want[q], cond[q])
        yard = R.worst(t32[q].cpu(), want[q], cond[q]) if q in t32 else float("nan")
        print(f"[dt64] {tag} {q} {kern:.3f} / {yard:.4g}")
        fig[q] = [round(kern, 4) if math.isfinite(kern) else repr(kern), float(f"{yard:.4g}") if math.isfinite(yard) else None]
        if not kern <= 1.0:                                      # a NaN fails here
            failures.append((q, kern))
    _report(f"dt64/{tag}", fig)
    assert not failures, (tag, failures)


# ------------------------------------------------------------------------------------------------ upsampling
def _up_abi(x, g, s, mode, reciprocal, shift, tag):
    n, _, h, w = x.shape
    xs, gs = _placed(x, shift), _placed(g, shift)
    out_buf, out = _guarded(n * h * s * w * s, torch.float32, shift)
    gx_buf, gx = _guarded(n * h * w, torch.float32, shift)
    lib = _lib.lib()
    _lib.check(lib.s360_upsample_forward(_ptr(xs), _ptr(out), n, h, w, s, dt.MODES[mode], int(reciprocal), _stream()), "forward")
    _lib.check(lib.s360_upsample_backward(_ptr(gs), _ptr(xs) if reciprocal else None, _ptr(gx), n, h, w, s, dt.MODES[mode], int(reciprocal),
                                          _stream()), "backward")
    torch.cuda.synchronize()
    _assert_owned(out_buf, out.numel(), shift, (tag, "out", shift))
    _assert_owned(gx_buf, gx.numel(), shift, (tag, "g_src", shift))
    return dict(out=out.view(n, 1, h * s, w * s), g_src=gx.view(n, 1, h, w))


@functools.lru_cache(maxsize=None)
def _up_case(name):
    n, h, w, s = UP_SHAPES[name]
    return R.random_maps(n, h, w, s, seed=sum(UP_SHAPES[name]), device=DEV)


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(UP_SHAPES))
def test_upsample_every_element_against_float64(name, mode, reciprocal):
    s = UP_SHAPES[name][3]
    depth, pmax, g, _ = _up_case(name)
    tag = f"up/{name}/{mode}{'/recip' if reciprocal else ''}"
    base = tag
    for x in ((depth,) if reciprocal or mode == "bilinear" else (depth, pmax)):
        tag = base + ("/pmax" if x is pmax else "")
        runs = [_up_abi(x, g, s, mode, reciprocal, shift, tag) for shift in (0, 1)]
        assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), (tag, "aligned and shifted runs differ")
        got = runs[0]
        z = x.clone().requires_grad_(True)
        out = dt.upsample(z, s, mode, reciprocal)
        out.backward(g)
        assert torch.equal(out, got["out"]) and torch.equal(z.grad, got["g_src"]), (tag, "the Python layer and the C ABI differ")
        want, cond = {}, {}
        want["out"], cond["out"] = R.upsample_elements(x, s, mode, reciprocal)
        want["g_src"], cond["g_src"] = R.upsample_backward_elements(g, x, s, mode, reciprocal)
        if mode == "nearest" and not reciprocal:                                 # a gather: the source's bits
            assert torch.equal(got["out"].cpu().double(), want["out"]) and torch.equal(got["out"], torch.nn.functional.interpolate(x, scale_factor=s))
        zz = x.clone().requires_grad_(True)
        t_out = R.upsample(zz, s, mode, reciprocal, torch.float32)
        t_out.backward(g)
        _judge(tag, got, want, cond, dict(out=t_out.detach(), g_src=zz.grad))


# ------------------------------------------------------------------------------------------------ the tail
@functools.lru_cache(maxsize=None)
def _tail_case(name):
    b, v, h, w, gpp = TAIL_SHAPES[name]
    fullres, dd, near, far, *grads = R.random_case(b, v, h, w, gpp, seed=sum(TAIL_SHAPES[name]), device=DEV)
    bounds = torch.stack((far.t(), near.t())).reciprocal()                       # as fine_depth_tail forms them: [2, v, b]
    lo, hi = bounds[0].reshape(-1).contiguous(), bounds[1].reshape(-1).contiguous()
    fullres, dd = R.plant(fullres, dd, lo, hi, gpp)
    return fullres, dd, near, far, lo, hi, tuple(grads)


def _tail_abi(fullres, dd, lo, hi, v, gpp, exponent, grads, shift, tag):
    """One forward and one backward of the C ABI; outputs come back in plane layout."""
    n, _, h, w = fullres.shape
    b = n // v
    f, d, l, u = (_placed(t, shift) for t in (fullres, dd, lo, hi))
    g = [_placed(t, shift) for t in grads]
    bufs = {k: _guarded(n * gpp * h * w, torch.float32, shift) for k in ("depths", "opacities", "densities")}
    bufs["g_fullres"] = _guarded(n * h * w, torch.float32, shift)
    bufs["g_dd"] = _guarded(n * 2 * gpp * h * w, torch.float32, shift)
    body = {k: x[1] for k, x in bufs.items()}
    lib = _lib.lib()
    _lib.check(lib.s360_depth_tail_forward(_ptr(f), _ptr(d), _ptr(l), _ptr(u), exponent, gpp, v, _ptr(body["depths"]), _ptr(body["opacities"]),
                                           _ptr(body["densities"]), n, h, w, _stream()), "forward")
    _lib.check(lib.s360_depth_tail_backward(_ptr(g[0]), _ptr(g[1]), _ptr(g[2]), _ptr(f), _ptr(d), _ptr(l), _ptr(u), exponent, gpp, v,
                                            _ptr(body["g_fullres"]), _ptr(body["g_dd"]), n, h, w, _stream()), "backward")
    torch.cuda.synchronize()
    for k, (buf, x) in bufs.items():
        _assert_owned(buf, x.numel(), shift, (tag, k, shift))
    raw = {k: body[k].view(b, v, h * w, 1, gpp) for k in ("depths", "opacities", "densities")}
    g_dd = body["g_dd"].view(n, 2 * gpp, h, w)
    got = {k: R.planes(x, h, w) for k, x in raw.items()}
    got.update(g_fullres=body["g_fullres"].view(n, 1, h, w), g_delta=g_dd[:, :gpp], g_logit=g_dd[:, gpp:])
    return got, raw, g_dd


def _tail_hold(tag, name, exponent, grads):
    b, v, h, w, gpp = TAIL_SHAPES[name]
    fullres, dd, near, far, lo, hi, _ = _tail_case(name)
    runs = [_tail_abi(fullres, dd, lo, hi, v, gpp, exponent, grads, shift, tag) for shift in (0, 1)]
    assert all(torch.equal(runs[0][0][k], runs[1][0][k]) for k in runs[0][0]), (tag, "aligned and shifted runs differ")
    got, raw, g_dd = runs[0]
    f, d = fullres.clone().requires_grad_(True), dd.clone().requires_grad_(True)
    outs = dt.fine_depth_tail(f, d, near, far, views=v, gaussians_per_pixel=gpp, exponent=exponent, return_densities=True)
    pairs = [(o, g) for o, g in zip(outs, grads) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    assert all(torch.equal(o, raw[k]) for o, k in zip(outs, ("depths", "opacities", "densities"))), (tag, "the Python layer and the C ABI differ")
    assert torch.equal(f.grad, got["g_fullres"]) and torch.equal(d.grad, g_dd), (tag, "the Python layer and the C ABI differ")
    want, cond = R.tail_elements(fullres, dd, lo, hi, gpp, exponent, grads)
    with torch.no_grad():
        t_outs = R.tail_planes(fullres, dd, near, far, gpp, exponent, torch.float32)[:3]
    tf, td = fullres.clone().requires_grad_(True), dd.clone().requires_grad_(True)
    pairs = [(o, g) for o, g in zip(R.tail(tf, td, near, far, gpp, exponent, torch.float32), grads) if g is not None]
    t_f, t_d = (torch.zeros_like(x) if y is None else y for x, y in
                zip((tf, td), torch.autograd.grad([o for o, _ in pairs], (tf, td), [g for _, g in pairs], allow_unused=True)))
    t32 = dict(depths=t_outs[0], opacities=t_outs[1], densities=t_outs[2], g_fullres=t_f, g_delta=t_d[:, :gpp], g_logit=t_d[:, gpp:])
    _judge(tag, {k: x.contiguous() for k, x in got.items()}, want, cond, t32)
    # the pattern of zeros of the disparity gradient is the float32 sum's, element for element
    inside = R.clamp_pattern(fullres, dd[:, :gpp], lo, hi)
    if grads[0] is not None:
        assert torch.equal(got["g_delta"].cpu() != 0, inside & (R.planes(grads[0].cpu(), h, w) != 0)), tag
    return got


@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_tail_every_element_against_float64(name, exponent):
    _tail_hold(f"tail/{name}/e{exponent:g}", name, exponent, _tail_case(name)[6])


@pytest.mark.parametrize("name", ["gpp2", "vec_gpp2", "two_views"])
def test_tail_one_gradient_alone_as_null_pointers(name):
    grads = _tail_case(name)[6]
    for i, what in enumerate(("g_depths", "g_opacities", "g_densities")):
        _tail_hold(f"tail/{name}/{what} only", name, 0.5, tuple(g if j == i else None for j, g in enumerate(grads)))


def test_tail_forward_without_densities_leaves_the_other_two_alone():
    fullres, dd, near, far, lo, hi, grads = _tail_case("vec_gpp2")
    b, v, h, w, gpp = TAIL_SHAPES["vec_gpp2"]
    full, _, _ = _tail_abi(fullres, dd, lo, hi, v, gpp, 4.0, grads, 0, "no densities")
    two = dt.fine_depth_tail(fullres, dd, near, far, views=v, gaussians_per_pixel=gpp, exponent=4.0)
    assert len(two) == 2 and torch.equal(R.planes(two[0], h, w), full["depths"]) and torch.equal(R.planes(two[1], h, w), full["opacities"])


# ------------------------------------------------------------------------------------------------ the flat opacity map
def _map_abi(p, g, exponent, shift, tag):
    ps, gs = _placed(p, shift), _placed(g, shift)
    o_buf, o = _guarded(p.numel(), torch.float32, shift)
    g_buf, gp = _guarded(p.numel(), torch.float32, shift)
    lib = _lib.lib()
    _lib.check(lib.s360_opacity_map_forward(_ptr(ps), _ptr(o), p.numel(), exponent, _stream()), "forward")
    _lib.check(lib.s360_opacity_map_backward(_ptr(ps), _ptr(gs), _ptr(gp), p.numel(), exponent, _stream()), "backward")
    torch.cuda.synchronize()
    _assert_owned(o_buf, p.numel(), shift, (tag, "out", shift))
    # the gradient may hold the statement's infinities, never a NaN: the ownership check reads NaN as unwritten
    _assert_owned(g_buf, p.numel(), shift, (tag, "g_pdf", shift))
    return dict(out=o, g_pdf=gp)


@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("length", MAP_LENGTHS)
def test_opacity_map_every_element_against_float64(length, exponent):
    """p in [1 / 256, 1] (pdf_max's range for D <= 256), with p = 1 and p = 1 / 256 planted where they fit; at p = 1 with
    e = 0.5 the gradient is the float64 statement's infinity, sign included."""
    gen = torch.Generator().manual_seed(3 + length)
    p = (1.0 / 256 + (1.0 - 1.0 / 256) * torch.rand(length, generator=gen)).clamp(1.0 / 256, 1.0)
    g = torch.randn(length, generator=gen)
    p[0], g[0] = 1.0, -1.5
    if length > 1:
        p[length - 1], g[length - 1] = 1.0 / 256, 2.5
    if length > 4:
        p[4], g[4] = 1.0, 0.75
    p, g = p.to(DEV), g.to(DEV)
    tag = f"map/n{length}/e{exponent:g}"
    runs = [_map_abi(p, g, exponent, shift, tag) for shift in (0, 1)]
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), (tag, "aligned and shifted runs differ")
    got = runs[0]
    z = p.clone().requires_grad_(True)
    out = dt.map_pdf_to_opacity(z, exponent)
    out.backward(g)
    assert torch.equal(out, got["out"]) and torch.equal(z.grad, got["g_pdf"]), (tag, "the Python layer and the C ABI differ")
    want, cond = {}, {}
    want["out"], cond["out"] = R.opacity_map_elements(p, exponent)
    want["g_pdf"], cond["g_pdf"] = R.opacity_map_elements(p, exponent, g)
    if exponent == 0.5:
        assert want["g_pdf"][0].item() == float("-inf") and got["g_pdf"][0].item() == float("-inf")
        assert length <= 4 or got["g_pdf"][4].item() == float("inf")
    zz = p.clone().requires_grad_(True)
    t_out = R.map_pdf_to_opacity(zz, exponent)
    t_out.backward(g)
    _judge(tag, got, want, cond, dict(out=t_out.detach(), g_pdf=zz.grad))
