"""The per-element measure of the fine-depth and opacity tail and of the upsampling, pinned on the CPU
(tests/depth_tail_reference.py: opacity_elements, upsample_elements, tail_elements, opacity_map_elements, worst).

tests/test_gpu_depth_tail.py pools each tensor into one maximum and one mean absolute error, and its float64 `want` of the
opacity is torch's 1 - (1 - sigmoid(x)) ** e, which cancels: from |x| = 37 on 1 - sigmoid(x) keeps no digit, so that statement cannot
judge the kernel where it is most careful (it forms the opacity through expm1 and softplus).  Here every element is measured
against its own bound, 2^-24 |want| + 2^-40 A + 2^-149 (A: the sum of the magnitudes of the element's terms), and this file shows
without a GPU that

  - the float64 form used as `want` agrees with 200-bit arithmetic (mpmath) to 2^-45 relative over x in [-100, 100] and
    e in {1, 4, 0.5}, for the opacity, its logit slope, p and p (1 - p) — and that torch's float64 statement is millions of bounds
    off at large |x| (printed);
  - the numpy statement of the bilinear upsampling from exact integer taps agrees with float64 F.interpolate to 2^-40 A;
  - a float64 model of the kernels' formulas, rounded once, meets the bound, with the edges planted (logits to +-100, sums on
    and one ulp around the clamp's bounds), and torch's float32 statement does not (printed);
  - three planted defects fail it: the opacity as 1 - (1 - p)^e in float64, the slope with q = 1 - p, and the clamp decided on
    the float64 sum for sums within half an ulp of a bound.  Whether the pooled rule passes each is printed.

tests/test_gpu_depth_tail_float64.py holds the kernels to the same measure.
"""
import functools

import pytest
import torch

import depth_head_reference as R_head
import depth_tail_reference as R

EXPONENTS = (1.0, 4.0, 0.5)
UP_SHAPES = {"cell": (1, 2, 2, 4), "odd": (2, 3, 5, 4), "h1": (1, 1, 7, 2), "s1": (1, 4, 4, 1), "s3": (3, 5, 13, 3), "wave": (1, 9, 33, 4)}
TAIL_SHAPES = {"two_views": (1, 2, 4, 8, 1), "batch": (2, 2, 5, 13, 1), "gpp2": (1, 3, 3, 21, 2), "vec_gpp2": (1, 2, 2, 6, 2)}


def _pin_points():
    gen = torch.Generator().manual_seed(5)
    grid = torch.linspace(-100.0, 100.0, 401, dtype=torch.float64)
    near = torch.tensor([-1e-3, 1e-3, -1e-8, 1e-8, 0.0, 36.7, -36.7, 37.5, -37.5, 17.5, -17.5, 88.0, -88.0], dtype=torch.float64)
    return torch.cat((grid, near, (200.0 * torch.rand(200, generator=gen) - 100.0).float().double()))


@pytest.mark.parametrize("exponent", EXPONENTS)
def test_the_float64_form_agrees_with_200_bit_arithmetic(exponent):
    import mpmath
    mpmath.mp.prec = 200
    x = _pin_points()
    form = R.opacity_elements(x, exponent)
    stated = dict(opacity=R.map_pdf_to_opacity(torch.sigmoid(x), exponent), slope=R.opacity_logit_slope(x, exponent), p=torch.sigmoid(x),
                  pq=torch.sigmoid(x) * (1 - torch.sigmoid(x)))
    e = mpmath.mpf(exponent)
    worst_form, worst_stated = dict.fromkeys(form, 0.0), dict.fromkeys(form, 0.0)
    for i, xi in enumerate(x.tolist()):
        p = 1 / (1 + mpmath.exp(-mpmath.mpf(xi)))
        q = 1 / (1 + mpmath.exp(mpmath.mpf(xi)))
        exact = dict(opacity=(1 - q ** e + p ** (1 / e)) / 2, slope=(e * q ** e * p + p ** (1 / e) * q / e) / 2, p=p, pq=p * q)
        for k, v in exact.items():
            worst_form[k] = max(worst_form[k], float(abs(mpmath.mpf(form[k][i].item()) - v) / v))
            worst_stated[k] = max(worst_stated[k], float(abs(mpmath.mpf(stated[k][i].item()) - v) / v))
    print(f"e={exponent:g}: relative error against 200 bits, in units of 2^-45: the pinned form "
          + " ".join(f"{k} {v * 2.0 ** 45:.3g}" for k, v in worst_form.items())
          + "; torch's float64 statement, in units of 2^-24 (one float32 bound) "
          + " ".join(f"{k} {v * 2.0 ** 24:.3g}" for k, v in worst_stated.items()))
    assert all(v <= 2.0 ** -45 for v in worst_form.values()), worst_form
    if exponent <= 1.0:                                                         # at e = 4 the root p^(1 / 4) hides the lost 1 - (1 - p)^4
        assert worst_stated["opacity"] > 1e6 * 2.0 ** -24                       # why torch's float64 statement is not the `want`
    assert worst_stated["pq"] > 1e6 * 2.0 ** -24


@pytest.mark.parametrize("reciprocal", [False, True])
@pytest.mark.parametrize("name", list(UP_SHAPES))
def test_the_integer_tap_statement_of_the_bilinear_upsampling_agrees_with_float64_interpolate(name, reciprocal):
    n, h, w, s = UP_SHAPES[name]
    x, _, g, _ = R.random_maps(n, h, w, s, seed=sum(UP_SHAPES[name]))
    want, cond = R.upsample_elements(x, s, "bilinear", reciprocal)
    torchs = R.upsample(x, s, "bilinear", reciprocal)
    assert bool(((torchs - want).abs() <= R.COND * cond).all())
    z = x.double().requires_grad_(True)
    (tg,) = torch.autograd.grad(R.upsample(z, s, "bilinear", reciprocal), z, g.double())
    gw, gc = R.upsample_backward_elements(g, x, s, "bilinear", reciprocal)
    assert bool(((tg - gw).abs() <= R.COND * gc).all())
    # the float32 statement, for the reader
    t32 = R.upsample(x, s, "bilinear", reciprocal, torch.float32)
    print(f"{name}{' 1/x' if reciprocal else ''}: float64 interpolate {((torchs - want).abs() / (R.COND * cond + R.TINY)).max().item():.3g} x 2^-40 A; "
          f"torch float32 {R.worst(t32, want, cond):.3g} bounds")
    assert R.worst(want.float(), want, cond) <= 1.0


@pytest.mark.parametrize("name", list(UP_SHAPES))
def test_the_nearest_statement_is_a_gather(name):
    n, h, w, s = UP_SHAPES[name]
    x, _, g, _ = R.random_maps(n, h, w, s, seed=sum(UP_SHAPES[name]))
    want, _ = R.upsample_elements(x, s, "nearest")
    assert torch.equal(want.float(), torch.nn.functional.interpolate(x, scale_factor=s))
    gw, gc = R.upsample_backward_elements(g, x, s, "nearest")
    z = x.double().requires_grad_(True)
    (tg,) = torch.autograd.grad(R.upsample(z, s, "nearest"), z, g.double())
    assert bool(((tg - gw).abs() <= R.COND * gc).all())


@functools.lru_cache(maxsize=None)
def _tail_case(name):
    b, v, h, w, gpp = TAIL_SHAPES[name]
    fullres, dd, near, far, *grads = R.random_case(b, v, h, w, gpp, seed=sum(TAIL_SHAPES[name]))
    lo, hi = (t.reshape(-1) for t in R.bounds(near, far))
    fullres, dd = R.plant(fullres, dd, lo, hi, gpp)
    return fullres, dd, near, far, lo, hi, grads


def _float32_statement(fullres, dd, near, far, gpp, exponent, grads):
    """torch's float32 statement in plane layout; its density gradient is NaN where the sigmoid rounds to 0 or 1."""
    h, w = fullres.shape[2:]
    outs = R.tail_planes(fullres, dd, near, far, gpp, exponent, torch.float32)[:3]
    g_f, g_d = R.tail_gradient(fullres, dd, near, far, gpp, exponent, grads, torch.float32)
    return dict(depths=outs[0], opacities=outs[1], densities=outs[2], g_fullres=g_f, g_delta=g_d[:, :gpp], g_logit=g_d[:, gpp:])


def _pooled(got, want, t32):
    ok = torch.isfinite(t32)
    return R_head.pooled_passes(got[ok], want[ok], t32[ok])


@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_a_float64_model_rounded_once_meets_the_bound_and_torch_float32_does_not(name, exponent):
    fullres, dd, near, far, lo, hi, grads = _tail_case(name)
    gpp = TAIL_SHAPES[name][4]
    want, cond = R.tail_elements(fullres, dd, lo, hi, gpp, exponent, grads)
    model = R.tail_model(fullres, dd, lo, hi, gpp, exponent, grads)
    t32 = _float32_statement(fullres, dd, near, far, gpp, exponent, grads)
    fig = {q: R.worst(model[q], want[q], cond[q]) for q in R.TAIL_QUANTITIES}
    yard = {q: R.worst(t32[q], want[q], cond[q]) for q in R.TAIL_QUANTITIES}
    print(f"{name} e={exponent:g}: model " + " ".join(f"{q} {fig[q]:.3g}" for q in R.TAIL_QUANTITIES)
          + "; torch float32 " + " ".join(f"{q} {yard[q]:.3g}" for q in R.TAIL_QUANTITIES))
    assert all(v <= 1.0 for v in fig.values()), fig
    assert not yard["opacities"] <= 1.0 and not yard["g_logit"] <= 1.0           # float32's sigmoid saturates: no yardstick here


@pytest.mark.parametrize("exponent", EXPONENTS)
@pytest.mark.parametrize("name", list(TAIL_SHAPES))
def test_planted_defects_fail_the_measure(name, exponent):
    """Each defect is asserted at the exponents where it changes a float32 digit at all: at e = 4 the root p^(1 / 4) of the opacity
    is 1e22 times the lost 1 - (1 - p)^4 at x = -100, and at e = 0.5 the slope's first term e (1 - p)^e p (which takes log(1 - p),
    not 1 - p) is 1e8 times the second wherever 1 - p cancels; there the figure is printed and nothing is asserted of it."""
    fullres, dd, near, far, lo, hi, grads = _tail_case(name)
    gpp = TAIL_SHAPES[name][4]
    want, cond = R.tail_elements(fullres, dd, lo, hi, gpp, exponent, grads)
    t32 = _float32_statement(fullres, dd, near, far, gpp, exponent, grads)
    for label, kwargs, q in (("opacity as 1 - (1 - p)^e in float64", dict(opacity="pow"), "opacities"),
                             ("slope with q = 1 - p", dict(slope_q="one_minus_p"), "g_logit"),
                             ("clamp decided on the float64 sum", dict(float64_clamp=True), "g_delta")):
        bad = R.tail_model(fullres, dd, lo, hi, gpp, exponent, grads, **kwargs)
        per_element = R.worst(bad[q], want[q], cond[q])
        pooled = _pooled(bad[q], want[q], t32[q])
        print(f"{name} e={exponent:g}: {label}: {q} {per_element:.4g} bounds; pooled rule (finite float32 elements) {'passes' if pooled else 'fails'}")
        visible = not (q == "opacities" and exponent == 4.0) and not (q == "g_logit" and exponent == 0.5)
        assert per_element > 1.0 or not visible, label
        others = [k for k in R.TAIL_QUANTITIES if k != q and not (q == "g_delta" and k == "g_fullres")]
        assert all(R.worst(bad[k], want[k], cond[k]) <= 1.0 for k in others), label


def test_the_clamp_follows_the_float32_sum_within_half_an_ulp_of_a_bound():
    """fullres = lo with delta = -+ lo 2^-26 (and hi likewise): the float64 sum is outside or inside by a quarter ulp, the float32
    sum is the bound itself, so the gradient passes — the kernel's stated contract, and torch's element for element."""
    fullres, dd, near, far, lo, hi, grads = _tail_case("two_views")
    inside = R.clamp_pattern(fullres, dd[:, :1], lo, hi)
    total64 = fullres.double() + dd[:, :1].double()
    in64 = (total64 >= lo.double().view(-1, 1, 1, 1)) & (total64 <= hi.double().view(-1, 1, 1, 1))
    differ = inside & ~in64
    assert int(differ.sum()) >= 2 and int((~inside & in64).sum()) == 0
    f = fullres.clone().requires_grad_(True)
    (f + dd[:, :1]).clamp(*R.bounds(near, far)).sum().backward()
    assert torch.equal(f.grad != 0, inside)


@pytest.mark.parametrize("exponent", EXPONENTS)
def test_the_opacity_map_measure(exponent):
    gen = torch.Generator().manual_seed(3)
    p = (1.0 / 256 + (1.0 - 1.0 / 256) * torch.rand(1027, generator=gen)).clamp(1.0 / 256, 1.0)
    p[:2] = torch.tensor([1.0, 1.0 / 256])
    g = torch.randn(1027, generator=gen)
    g[0] = -1.5
    want, cond = R.opacity_map_elements(p, exponent)
    gw, gc = R.opacity_map_elements(p, exponent, g)
    assert R.worst(want.float(), want, cond) <= 1.0 and R.worst(gw.float(), gw, gc) <= 1.0
    z = p.clone().requires_grad_(True)
    R.map_pdf_to_opacity(z, exponent).backward(g)
    print(f"opacity map e={exponent:g}: torch float32 value {R.worst(R.map_pdf_to_opacity(p, exponent), want, cond):.3g} bounds, "
          f"gradient {R.worst(z.grad, gw, gc):.3g} bounds; gradient at p = 1: {gw[0].item()}")
    if exponent == 0.5:
        assert gw[0].item() == float("-inf")                                     # g = -1.5 times the statement's +inf
    z64 = p.double().requires_grad_(True)
    R.map_pdf_to_opacity(z64, exponent).backward(g.double())
    assert R.worst(z64.grad, gw, gc) <= 1.0                                      # autograd of the statement: the same infinities
