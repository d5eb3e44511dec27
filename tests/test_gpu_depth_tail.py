"""The native fine-depth and opacity tail (splatter360_amd/depth_tail.py, csrc/s360_depth_tail.hip) on the GPU against the float64
statement of tests/depth_tail_reference.py.

Accuracy rule (the project's "as close to float64 as the float32 statement is", tests/test_gpu_depth_head.py): for every output
and every gradient, over the compared elements, the kernel's max and mean absolute error against float64 are
<= max(1.5 x the same figure of the torch float32 statement on the same GPU and inputs, 2^-24 max|want|).  The floor is half a
float32 ulp of the largest value: a correctly rounded result cannot fail where torch happens to be exact.

Clamp exclusions: the gradient through the clamp is 0 or not by a comparison of a float32 sum with a float32 bound; float64 adds
without rounding and can decide the other way for a sum within half an ulp of a bound.  For g_fullres_disps and the disparity half
of g_delta the elements where the two statements decide differently are left out (at most 0.1 % of them, which
tests/test_depth_tail_spec.py shows the recipe leaves ample room for), and on the rest the kernel's zero / non-zero pattern equals
the float32 statement's exactly."""
import sys

import pytest
import torch

import depth_tail_reference as R
from splatter360_amd import depth_tail as dt, plugin

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (n, h, w, s): the smallest shapes at which each mechanism of the upsampling can break
UP_SHAPES = {
    "cell": (1, 2, 2, 4),                  # minimal bilinear cell
    "odd": (2, 3, 5, 4),                   # odd sizes
    "h1": (1, 1, 7, 2),                    # h = 1; the fine row (14) is no multiple of 4: the scalar forward
    "s1": (1, 4, 4, 1),                    # s = 1: the output is the input, or 1 / x
    "s3": (3, 5, 13, 3),                   # a scale that is no power of two; fine row 39: scalar
    "wave": (1, 9, 33, 4),                 # a fine row (132) crossing a wave
}
HM3D_UP = (2, 128, 256, 4)
# (b, v, H, W, gpp)
TAIL_SHAPES = {
    "two_views": (1, 2, 4, 8, 1),
    "batch": (2, 2, 5, 13, 1),             # b > 1: the (v b) -> (b v) transposition is visible; H W = 65: the scalar kernels
    "gpp2": (1, 3, 3, 21, 2),              # gpp = 2, odd
    "single": (1, 1, 1, 1, 1),
}
HM3D_TAIL = (1, 2, 512, 1024, 1)
EXPONENTS = (1.0, 4.0, 0.5)                # 2^0, 2^2, 2^-1
MODES = ("nearest", "bilinear")
_UP, _TAIL = {}, {}


def _check(label, got, want, t32, keep=None):
    """The rule: prints the four figures, then asserts both bars.  keep: the compared elements (all by default)."""
    assert got.dtype == torch.float32 and got.shape == want.shape and torch.isfinite(got).all()
    e_k, e_t, ref = (got.double() - want).abs(), (t32.double() - want).abs(), want.abs()
    if keep is not None:
        e_k, e_t, ref = e_k[keep], e_t[keep], ref[keep]
    floor = 2.0 ** -24 * ref.max().item()
    figures = (e_k.max().item(), e_k.mean().item(), e_t.max().item(), e_t.mean().item())
    print(f"{label}: kernel max/mean {figures[0]:.4g} {figures[1]:.4g}; torch f32 max/mean {figures[2]:.4g} {figures[3]:.4g}; floor {floor:.4g}")
    assert figures[0] <= max(1.5 * figures[2], floor) and figures[1] <= max(1.5 * figures[3], floor), (label, figures, floor)


def _up_case(shape):
    if shape not in _UP:
        n, h, w, s = shape
        _UP[shape] = R.random_maps(n, h, w, s, seed=sum(shape), device=DEV)
    return _UP[shape]


def _statement_up_gradient(x, g, s, mode, reciprocal, dtype):
    z = x.detach().to(dtype).requires_grad_(True)
    return torch.autograd.grad(R.upsample(z, s, mode, reciprocal, dtype), z, g.to(dtype))[0]


def _native_up_gradient(x, g, s, mode, reciprocal):
    z = x.clone().requires_grad_(True)
    dt.upsample(z, s, mode, reciprocal).backward(g)
    return z.grad


def _up_accuracy(name, shape, mode, reciprocal):
    s = shape[3]
    x, _, g, _ = _up_case(shape)
    label = f"{name} {mode}{' 1/x' if reciprocal else ''}"
    got = dt.upsample(x, s, mode, reciprocal)
    with torch.no_grad():
        _check(f"{label} out", got, R.upsample(x, s, mode, reciprocal), R.upsample(x, s, mode, reciprocal, torch.float32))
    grad = _native_up_gradient(x, g, s, mode, reciprocal)
    _check(f"{label} g_src", grad, _statement_up_gradient(x, g, s, mode, reciprocal, torch.float64),
           _statement_up_gradient(x, g, s, mode, reciprocal, torch.float32))
    return x, got


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(UP_SHAPES))
def test_upsample_and_its_gradient_match_float64_as_closely_as_torch_float32(name, mode, reciprocal):
    x, got = _up_accuracy(name, UP_SHAPES[name], mode, reciprocal)
    if name == "s1":                                                            # s = 1: no interpolation, one rounding
        assert torch.equal(got, (1 / x.double()).float() if reciprocal else x)


@pytest.mark.parametrize("name", [k for k, v in UP_SHAPES.items() if v[3] in (2, 3, 4)])
def test_nearest_is_bit_equal_to_torchs_interpolate(name):
    x, pmax, _, _ = _up_case(UP_SHAPES[name])
    s = UP_SHAPES[name][3]
    for t in (x, pmax):
        assert torch.equal(dt.upsample(t, s), torch.nn.functional.interpolate(t, scale_factor=s))


def test_upsample_hm3d_shape_matches_float64_as_closely_as_torch_float32():
    _up_accuracy("hm3d", HM3D_UP, "bilinear", True)
    _up_accuracy("hm3d", HM3D_UP, "nearest", False)
    _UP.pop(HM3D_UP)


@pytest.mark.parametrize("name", list(UP_SHAPES))
def test_bilinear_backward_is_the_adjoint_of_the_forward(name):
    """<up(x), g> = <x, up^T(g)>, both sums in float64 from the float32 results.  x and g are positive, so neither sum cancels
    and each side is off by at most one float32 rounding (2^-24 relative) per term: 2^-20 leaves a factor of eight."""
    n, h, w, s = UP_SHAPES[name]
    x, _, g, _ = _up_case(UP_SHAPES[name])
    g = g.abs() + 0.5
    lhs = (dt.upsample(x, s, "bilinear").double() * g.double()).sum().item()
    rhs = (x.double() * _native_up_gradient(x, g, s, "bilinear", False).double()).sum().item()
    print(f"{name}: <up x, g> {lhs!r}  <x, up^T g> {rhs!r}  relative difference {abs(lhs - rhs) / abs(lhs):.3g}")
    assert abs(lhs - rhs) <= 2.0 ** -20 * abs(lhs)


def test_fullres_maps_is_the_two_upsamplings():
    depth, pmax, g_d, g_p = _up_case(UP_SHAPES["odd"])
    d, p = depth.clone().requires_grad_(True), pmax.clone().requires_grad_(True)
    fullres_disps, pdf_max = dt.fullres_maps(d, p, 4)
    assert torch.equal(fullres_disps, dt.upsample(depth, 4, "bilinear", reciprocal=True)) and torch.equal(pdf_max, dt.upsample(pmax, 4))
    torch.autograd.backward([fullres_disps, pdf_max], [g_d, g_p])
    assert torch.equal(d.grad, _native_up_gradient(depth, g_d, 4, "bilinear", True))
    assert torch.equal(p.grad, _native_up_gradient(pmax, g_p, 4, "nearest", False))
    with torch.no_grad():
        want, t32 = R.fullres_maps(depth, pmax, 4), R.fullres_maps(depth, pmax, 4, torch.float32)
    _check("fullres_maps disps", fullres_disps.detach(), want[0], t32[0])
    _check("fullres_maps pdf_max", pdf_max.detach(), want[1], t32[1])


def _tail_case(shape):
    if shape not in _TAIL:
        _TAIL[shape] = R.random_case(*shape, seed=sum(shape), device=DEV)
    return _TAIL[shape]


def _native_tail(case, gpp, exponent, grads=None):
    """(outputs, (g_fullres, g_delta)) of the native tail; grads: three gradients (None entries: unused outputs)."""
    fullres, dd, near, far = case[:4]
    f, d = fullres.clone().requires_grad_(True), dd.clone().requires_grad_(True)
    outs = dt.fine_depth_tail(f, d, near, far, views=near.shape[1], gaussians_per_pixel=gpp, exponent=exponent, return_densities=True)
    if grads is None:
        return outs, None
    pairs = [(o, g) for o, g in zip(outs, grads) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return outs, (f.grad, d.grad)


def _tail_accuracy(name, shape, exponent):
    b, v, h, w, gpp = shape
    case = _tail_case(shape)
    fullres, dd, near, far, *grads = case
    label = f"{name} e={exponent:g}"
    outs, (g_f, g_d) = _native_tail(case, gpp, exponent, grads)
    with torch.no_grad():
        want, t32 = R.tail(fullres, dd, near, far, gpp, exponent), R.tail(fullres, dd, near, far, gpp, exponent, torch.float32)
        p64 = R.clamp_pass(*R.tail_planes(fullres, dd, near, far, gpp, exponent, torch.float64)[3:])
        p32 = R.clamp_pass(*R.tail_planes(fullres, dd, near, far, gpp, exponent, torch.float32)[3:])
    for i, what in enumerate(("depths", "opacities", "densities")):
        assert outs[i].shape == (b, v, h * w, 1, gpp)
        _check(f"{label} {what}", outs[i].detach(), want[i], t32[i])
    want_g = R.tail_gradient(fullres, dd, near, far, gpp, exponent, grads, torch.float64)
    t32_g = R.tail_gradient(fullres, dd, near, far, gpp, exponent, grads, torch.float32)
    keep = p64 == p32                                                           # [n, gpp, H, W]
    differ = (~keep).sum().item()
    print(f"{label}: clamp decisions that differ between float64 and float32: {differ} of {keep.numel()}")
    assert differ <= 0.001 * keep.numel()
    keep_f = keep.all(dim=1, keepdim=True)
    _check(f"{label} g_fullres_disps", g_f, want_g[0], t32_g[0], keep_f)
    _check(f"{label} g_delta disparity", g_d[:, :gpp], want_g[1][:, :gpp], t32_g[1][:, :gpp], keep)
    _check(f"{label} g_delta density", g_d[:, gpp:], want_g[1][:, gpp:], t32_g[1][:, gpp:])
    assert torch.equal((g_d[:, :gpp] != 0)[keep], (t32_g[1][:, :gpp] != 0)[keep])
    assert torch.equal((g_f != 0)[keep_f], (t32_g[0] != 0)[keep_f])
    return outs


@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_tail_and_its_gradients_match_float64_as_closely_as_torch_float32(name, exponent):
    _tail_accuracy(name, TAIL_SHAPES[name], exponent)


def test_tail_hm3d_shape_matches_float64_as_closely_as_torch_float32():
    _tail_accuracy("hm3d", HM3D_TAIL, 4.0)
    _TAIL.pop(HM3D_TAIL)


def test_exponent_one_gives_the_density_over_gpp():
    for name in ("two_views", "gpp2"):
        gpp = TAIL_SHAPES[name][4]
        case = _tail_case(TAIL_SHAPES[name])
        outs, _ = _native_tail(case, gpp, 1.0)
        b, v = case[2].shape
        logits = case[1][:, gpp:]
        with torch.no_grad():
            _check(f"{name} opacity at e = 1", outs[1], R.relayout(torch.sigmoid(logits.double()) / gpp, b, v),
                   R.relayout(torch.sigmoid(logits) / gpp, b, v))


def test_clamp_passes_the_gradient_on_its_bounds_and_blocks_it_one_ulp_outside():
    near, far = torch.tensor([[0.3]], device=DEV), torch.tensor([[7.0]], device=DEV)
    lo, hi = (t.reshape(()) for t in R.bounds(near, far))
    inf = torch.tensor(float("inf"), device=DEV)
    sums = torch.stack((lo, hi, torch.nextafter(lo, -inf), torch.nextafter(hi, inf), 0.5 * (lo + hi)))
    fullres = sums.reshape(1, 1, 1, 5).clone().requires_grad_(True)
    dd = torch.zeros(1, 2, 1, 5, device=DEV, requires_grad=True)                # delta = 0: the sum is fullres exactly
    depths, _ = dt.fine_depth_tail(fullres, dd, near, far, views=1)
    g = torch.tensor([1.0, -2.0, 3.0, 4.0, 0.5], device=DEV).reshape(1, 1, 5, 1, 1)
    depths.backward(g)
    want = (-g.flatten().double() / sums.double() ** 2).float()
    want[2:4] = 0.0
    print("g_fullres at lo, hi, lo - ulp, hi + ulp, middle:", fullres.grad.flatten().tolist())
    assert torch.equal(fullres.grad.flatten(), want) and torch.equal(dd.grad[0, 0].flatten(), want)
    assert (want[:2] != 0).all() and want[4] != 0
    assert torch.equal(depths.flatten(), (1 / torch.stack((lo, hi, lo, hi, 0.5 * (lo + hi))).double()).float())


@pytest.mark.parametrize("exponent", [4.0, 0.5])
def test_saturated_logits_give_finite_outputs_and_gradients(exponent):
    for name in ("batch", "gpp2"):
        b, v, h, w, gpp = TAIL_SHAPES[name]
        fullres, dd, near, far, *grads = _tail_case(TAIL_SHAPES[name])
        values = torch.tensor([120.0, -120.0, 1e4, -1e4, 90.0, -104.0, 30.0], device=DEV)
        dd = dd.clone()
        dd[:, gpp:] = values[torch.arange(dd[:, gpp:].numel(), device=DEV) % len(values)].reshape(dd[:, gpp:].shape)
        outs, (g_f, g_d) = _native_tail((fullres, dd, near, far), gpp, exponent, grads)
        assert all(torch.isfinite(t).all() for t in (*outs, g_f, g_d))
        depths, opacities, densities = outs
        assert (opacities >= 0).all() and (opacities <= torch.tensor(1.0 / gpp, device=DEV)).all()
        assert (densities >= 0).all() and (densities <= 1).all()
        inf = torch.tensor(float("inf"), device=DEV)
        lo_d, hi_d = torch.nextafter(near, -inf)[:, :, None, None, None], torch.nextafter(far, inf)[:, :, None, None, None]
        assert (depths >= lo_d).all() and (depths <= hi_d).all()
        # the gradient is the closed form in the logit (float64 autograd of the statement is NaN here too: its sigmoid is exactly
        # 0 or 1 from |x| = 37 on), rounded once
        x = dd[:, gpp:].double()
        want = (R.planes(grads[1], h, w).double() * R.opacity_logit_slope(x, exponent, gpp)
                + R.planes(grads[2], h, w).double() * torch.sigmoid(x) * torch.sigmoid(-x))
        t32 = R.tail_gradient(fullres, dd, near, far, gpp, exponent, grads, torch.float32)[1][:, gpp:]
        err = (g_d[:, gpp:].double() - want).abs().max().item()
        print(f"{name} e={exponent:g}: float32 statement's density gradient has {torch.isnan(t32).sum().item()} NaN of {t32.numel()}; "
              f"kernel against the closed form: max error {err:.4g}")
        assert err <= 2.0 ** -24 * want.abs().max().item(), err


@pytest.mark.parametrize("name", ["batch", "gpp2"])
def test_layout_is_the_references_einops_pattern(name):
    """fine_depth_tail's [b, v, H W, 1, gpp] tensors against the same kernel run one (view, surface) plane at a time (where no
    relayout happens: b = v = gpp = 1) and put in place by the reference's einops pattern in torch."""
    b, v, h, w, gpp = TAIL_SHAPES[name]
    fullres, dd, near, far, *_ = _tail_case(TAIL_SHAPES[name])
    outs, _ = _native_tail((fullres, dd, near, far), gpp, 4.0)
    planes = [torch.empty(b * v, gpp, h, w, device=DEV) for _ in range(3)]
    for ni in range(b * v):
        vi, bi = divmod(ni, b)
        for k in range(gpp):
            one = dt.fine_depth_tail(fullres[ni:ni + 1], dd[ni:ni + 1, [k, gpp + k]], near[bi:bi + 1, vi:vi + 1], far[bi:bi + 1, vi:vi + 1],
                                     views=1, exponent=4.0, return_densities=True)
            for plane, o in zip(planes, one):
                plane[ni, k] = o.reshape(h, w)
    planes[1] = planes[1] / gpp                                                 # gpp is 1 or 2: exact
    for got, plane in zip(outs, planes):
        assert torch.equal(got, R.relayout(plane, b, v))


def test_forward_and_backward_are_bit_identical_across_runs():
    runs = []
    for _ in range(2):
        depth, pmax, g_d, g_p = _up_case(UP_SHAPES["s3"])
        case = _tail_case(TAIL_SHAPES["gpp2"])
        outs, grads = _native_tail(case, 2, 4.0, case[4:])
        pdf = pmax.clone().requires_grad_(True)
        opacity = dt.map_pdf_to_opacity(pdf, 4.0)
        opacity.backward(g_p[:, :, :5, :13])
        runs.append((dt.upsample(depth, 3, "bilinear", True), _native_up_gradient(depth, g_d, 3, "bilinear", True),
                     dt.upsample(pmax, 3), _native_up_gradient(pmax, g_p, 3, "nearest", False), *outs, *grads, opacity, pdf.grad))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_unused_outputs_hand_null_gradients():
    """One output used downstream alone: autograd hands None for the others, which reaches the kernel as null pointers and
    gives the bits of explicit zeros."""
    gpp = 2
    case = _tail_case(TAIL_SHAPES["gpp2"])
    g_depths, g_opacities, g_densities = case[4:]
    zeros = torch.zeros_like(g_depths)
    for grads in ((g_depths, None, None), (None, g_opacities, None), (None, None, g_densities)):
        with_none = _native_tail(case, gpp, 0.5, grads)[1]
        with_zeros = _native_tail(case, gpp, 0.5, [zeros if g is None else g for g in grads])[1]
        assert all(torch.equal(x, y) for x, y in zip(with_none, with_zeros))
    fullres, dd, near, far = case[:4]
    two = dt.fine_depth_tail(fullres, dd, near, far, views=3, gaussians_per_pixel=gpp, exponent=0.5)
    three = dt.fine_depth_tail(fullres, dd, near, far, views=3, gaussians_per_pixel=gpp, exponent=0.5, return_densities=True)
    assert len(two) == 2 and torch.equal(two[0], three[0]) and torch.equal(two[1], three[1])


@pytest.mark.parametrize("exponent", EXPONENTS)
def test_opacity_map_and_its_gradient_match_float64_and_mirror_its_infinities(exponent):
    gen = torch.Generator().manual_seed(3)
    pdf = (0.001 + 0.998 * torch.rand(3, 5, 7, 1, 1, generator=gen)).to(DEV)     # 105 elements: a float4 body and a ragged end
    g = torch.randn(3, 5, 7, 1, 1, generator=gen).to(DEV)
    z = pdf.clone().requires_grad_(True)
    out = dt.map_pdf_to_opacity(z, exponent)
    out.backward(g)
    z64, z32 = pdf.double().requires_grad_(True), pdf.clone().requires_grad_(True)
    want, t32 = R.map_pdf_to_opacity(z64, exponent), R.map_pdf_to_opacity(z32, exponent)
    want.backward(g.double())
    t32.backward(g)
    _check(f"opacity map e={exponent:g} out", out.detach(), want.detach(), t32.detach())
    _check(f"opacity map e={exponent:g} g_pdf", z.grad, z64.grad, z32.grad)
    ends = torch.tensor([0.0, 1.0, 0.5], device=DEV, requires_grad=True)
    dt.map_pdf_to_opacity(ends, exponent).sum().backward()
    ends64 = torch.tensor([0.0, 1.0, 0.5], dtype=torch.float64, device=DEV, requires_grad=True)
    R.map_pdf_to_opacity(ends64, exponent).sum().backward()
    print(f"opacity map e={exponent:g}: gradient at p = 0, 1, 0.5: {ends.grad.tolist()}; float64 statement {ends64.grad.tolist()}")
    assert torch.equal(ends.grad, ends64.grad.float())


def test_no_host_synchronisation_in_forward_and_backward():
    depth, pmax, g_d, g_p = _up_case(UP_SHAPES["odd"])
    case = _tail_case(TAIL_SHAPES["batch"])
    _native_tail(case, 1, 4.0, case[4:])                                        # warm-up: library load, allocator
    dt.fullres_maps(depth, pmax, 4)
    d, p = depth.clone().requires_grad_(True), pmax.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.autograd.backward(dt.fullres_maps(d, p, 4), [g_d, g_p])
        _native_tail(case, 1, 4.0, case[4:])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_non_contiguous_inputs_give_the_same_bits():
    depth, _, g_d, _ = _up_case(UP_SHAPES["odd"])
    wide = torch.rand(2, 1, 3, 8, device=DEV)
    wide[..., 1:6] = depth
    view = wide[..., 1:6]
    assert not view.is_contiguous()
    assert torch.equal(dt.upsample(view, 4, "bilinear", True), dt.upsample(depth, 4, "bilinear", True))
    assert torch.equal(_native_up_gradient(view, g_d, 4, "bilinear", True), _native_up_gradient(depth, g_d, 4, "bilinear", True))
    case = _tail_case(TAIL_SHAPES["two_views"])
    fullres, dd, near, far = case[:4]
    cl = dd.contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    want, got = _native_tail(case, 1, 4.0, case[4:]), _native_tail((fullres, cl, near, far), 1, 4.0, case[4:])
    assert all(torch.equal(x, y) for x, y in zip((*want[0], *want[1]), (*got[0], *got[1])))


def test_errors():
    fullres, dd, near, far, *_ = _tail_case(TAIL_SHAPES["two_views"])
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres, dd, near, far, views=3)                      # n % v
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres, dd, near, far, views=2, gaussians_per_pixel=2)
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres, dd, near.t(), far.t(), views=2)              # [v, b]
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres, dd, near, far, views=2, exponent=0.0)
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres, dd, near, far, views=2, exponent=float("nan"))
    with pytest.raises(ValueError):
        dt.fine_depth_tail(fullres.double(), dd.double(), near, far, views=2)
    with pytest.raises(RuntimeError):
        dt.fine_depth_tail(fullres, dd.cpu(), near, far, views=2)
    with pytest.raises(ValueError):
        dt.map_pdf_to_opacity(fullres, -1.0)
    with pytest.raises(ValueError):
        dt.upsample(fullres[:0], 2)
    with pytest.raises(ValueError):
        dt.upsample(fullres, 2.5)


def test_installed_seam_runs_the_kernels_and_falls_back():
    depth, pmax, g_d, g_p = _up_case(UP_SHAPES["odd"])
    assert plugin.COST_VOLUME_MODULE not in sys.modules and plugin.DEPTH_TAIL_MODULE not in sys.modules
    pred = R.standin_module(plugin.COST_VOLUME_MODULE, R.PREDICTOR_SOURCE)
    enc_mod = R.standin_module(plugin.DEPTH_TAIL_MODULE, R.ENCODER_SOURCE)
    sys.modules[plugin.COST_VOLUME_MODULE], sys.modules[plugin.DEPTH_TAIL_MODULE] = pred, enc_mod
    try:
        original = enc_mod.EncoderCostVolume.__dict__["map_pdf_to_opacity"]
        enc = enc_mod.EncoderCostVolume(initial=0.0, final=2.0, warm_up=100)
        pdf = pmax.reshape(2, 1, 15, 1, 1).contiguous()
        torchs = (*pred.fullres(depth, pmax, 4), enc.map_pdf_to_opacity(pdf, 50))
        proxy, method = plugin.install_depth_tail()
        assert pred.F is proxy and isinstance(proxy, dt.InterpolateProxy) and proxy.replaced is torch.nn.functional
        assert enc_mod.EncoderCostVolume.__dict__["map_pdf_to_opacity"] is method and method.replaced is original
        # the predictor's two F.interpolate calls: the native results bit for bit, and gradients flow
        d, p = depth.clone().requires_grad_(True), pmax.clone().requires_grad_(True)
        fullres_disps, pdf_max = pred.fullres(d, p, 4)
        assert torch.equal(fullres_disps, dt.upsample(1 / depth, 4, "bilinear")) and torch.equal(pdf_max, dt.upsample(pmax, 4))
        assert type(fullres_disps.grad_fn).__name__ == "_UpsampleBackward" and type(pdf_max.grad_fn).__name__ == "_UpsampleBackward"
        torch.autograd.backward([fullres_disps, pdf_max], [g_d, g_p])
        direct = depth.clone().requires_grad_(True)
        dt.upsample(1 / direct, 4, "bilinear").backward(g_d)
        assert torch.equal(d.grad, direct.grad) and torch.equal(p.grad, _native_up_gradient(pmax, g_p, 4, "nearest", False))
        # the encoder's method: the native opacity map with the method's own exponent
        exponent = dt.opacity_exponent(0.0, 2.0, 100, 50)
        assert exponent == 2.0
        z = pdf.clone().requires_grad_(True)
        opacity = enc.map_pdf_to_opacity(z, 50)
        assert torch.equal(opacity, dt.map_pdf_to_opacity(pdf, exponent)) and type(opacity.grad_fn).__name__ == "_OpacityMapBackward"
        opacity.sum().backward()
        assert torch.isfinite(z.grad).all() and z.grad.abs().max().item() > 0
        with torch.no_grad():
            _check("installed opacity", opacity.detach(), R.map_pdf_to_opacity(pdf.double(), exponent), torchs[2])
        # every other call: the replaced functions
        assert torch.equal(pred.half_pixel(depth, 2), torch.nn.functional.interpolate(depth, scale_factor=2, mode="bilinear", align_corners=False))
        rgb = depth.expand(2, 3, 3, 5)
        assert torch.equal(pred.F.interpolate(rgb, scale_factor=2), torch.nn.functional.interpolate(rgb, scale_factor=2))
        assert torch.equal(pred.F.interpolate(depth, size=(6, 10)), torch.nn.functional.interpolate(depth, size=(6, 10)))
        assert torch.equal(enc.map_pdf_to_opacity(pdf.double(), 50), original(enc, pdf.double(), 50))
        assert torch.equal(enc.map_pdf_to_opacity(pdf.cpu(), 50), original(enc, pdf.cpu(), 50))
        plugin.uninstall()
        assert pred.F is torch.nn.functional and enc_mod.EncoderCostVolume.__dict__["map_pdf_to_opacity"] is original
        again = (*pred.fullres(depth, pmax, 4), enc.map_pdf_to_opacity(pdf, 50))
        assert all(torch.equal(x, y) for x, y in zip(torchs, again))
    finally:
        plugin.uninstall()
        del sys.modules[plugin.COST_VOLUME_MODULE], sys.modules[plugin.DEPTH_TAIL_MODULE]
