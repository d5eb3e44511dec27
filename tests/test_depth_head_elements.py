"""The per-element measure of the softmax depth head, pinned on the CPU (tests/depth_head_reference.py: head_elements, worst).

tests/test_gpu_depth_head.py pools each tensor into one maximum and one mean absolute error.  The gradient of the logits is
p_d (...) with p_d from 1 down to 1e-50 and below inside one tensor, so the pooled figures see the few elements of weight near 1.
Here every element is measured against its own bound

    |got - want| <= 2^-24 |want| + 2^-40 A + 2^-149        (A: the sum of the magnitudes of the element's terms)

and this file shows, without a GPU, that the bound is one a correct float64-then-round kernel meets (kernel_model: worst <= 1 on the
four committed shapes at scales 1, 6, 30 and 1e4), that torch's float32 statement lies far outside it (printed), and that three
planted defects fail it — among them the backward WITHOUT its correction of the saved float32 lse and depth, which the pooled rule
passes at scales 1 and 6 on all four shapes (asserted).  tests/test_gpu_depth_head_float64.py holds the kernels to the same measure.
"""
import functools

import pytest
import torch

import depth_head_reference as R

SAMPLING = "inverse_depth"


@functools.lru_cache(maxsize=None)
def _case(name, scale):
    shape = R.ELEMENT_SHAPES[name]
    inputs = R.random_case(shape, scale, SAMPLING, seed=R.element_seed(shape, scale, SAMPLING))
    return (inputs, *R.head_elements(*inputs))


def _figures(got, want, cond):
    return {q: R.worst(got[q], want[q], cond[q]) for q in R.QUANTITIES}


@pytest.mark.parametrize("scale", R.ELEMENT_SCALES)
@pytest.mark.parametrize("name", list(R.ELEMENT_SHAPES))
def test_a_float64_model_rounded_once_meets_the_bound_and_torch_float32_does_not(name, scale):
    inputs, want, cond = _case(name, scale)
    model = R.kernel_model(*inputs)
    fig = _figures(model, want, cond)
    t32 = _figures(R.float32_statement(*inputs), want, cond)
    print(f"{name} x{scale:g}: model " + " ".join(f"{q} {fig[q]:.3g}" for q in R.QUANTITIES)
          + "; torch float32 " + " ".join(f"{q} {t32[q]:.3g}" for q in R.QUANTITIES))
    assert torch.equal(model["argmax"], want["argmax"])
    assert all(fig[q] <= 1.0 for q in R.QUANTITIES), fig
    if scale <= 30.0:                                            # at 1e4 the softmax of few depths is exactly one-hot: nothing to get wrong
        assert t32["g_logits"] > 100.0, t32                      # float32 carries its rounding of |z| into every p_d: no yardstick here


@pytest.mark.parametrize("scale", R.ELEMENT_SCALES)
@pytest.mark.parametrize("name", list(R.ELEMENT_SHAPES))
def test_the_backward_without_its_correction_fails_per_element_and_passes_the_pooled_rule(name, scale):
    """q = 1, r = 0 and pmax = e_a: the saved float32 lse and depth taken at face value."""
    inputs, want, cond = _case(name, scale)
    got = R.kernel_model(*inputs, corrected=False)["g_logits"]
    per_element = R.worst(got, want["g_logits"], cond["g_logits"])
    pooled = R.pooled_passes(got, want["g_logits"], R.logits_gradient(*inputs, torch.float32))
    print(f"{name} x{scale:g}: uncorrected backward {per_element:.4g} bounds; pooled rule {'passes' if pooled else 'fails'}")
    if scale <= 30.0:                                            # at 1e4 the softmax of few depths is exactly one-hot: lse and depth are exact
        assert per_element > 1.0
    if scale in (1.0, 6.0):
        assert pooled


def test_a_zeroed_gradient_column_at_a_low_scale_pixel_fails_per_element():
    inputs = R.mixed_case(SAMPLING)
    want, cond = R.head_elements(*inputs)
    model = R.kernel_model(*inputs)
    fig = _figures(model, want, cond)
    print("mixed: model " + " ".join(f"{q} {fig[q]:.3g}" for q in R.QUANTITIES))
    assert all(fig[q] <= 1.0 for q in R.QUANTITIES), fig
    # row 6: g_depth x 1e-6 (and logits x 30); the column's largest entry is far below the tensor's
    got = model["g_logits"].clone()
    assert want["g_logits"][1, :, 6, 5].abs().max() < 1e-3 * want["g_logits"].abs().max()
    got[1, :, 6, 5] = 0.0
    per_element = R.worst(got, want["g_logits"], cond["g_logits"])
    pooled = R.pooled_passes(got, want["g_logits"], R.logits_gradient(*inputs, torch.float32))
    print(f"mixed: one column zeroed {per_element:.4g} bounds; pooled rule {'passes' if pooled else 'fails'}")
    assert per_element > 1e6


@pytest.mark.parametrize("pair", [(2, 6), (2, 34), (3, 9), (9, 11), (0, 129)])
def test_the_last_maximum_on_a_tie_fails(pair):
    inputs, _, _ = _case("ragged", 1.0)
    logits, cand, g_depth, g_pmax = inputs
    tied = logits.clone()
    top = logits.max().item() + 1.0
    tied[:, pair[0]] = top
    tied[:, pair[1]] = top
    want, cond = R.head_elements(tied, cand, g_depth, g_pmax)
    assert (want["argmax"] == pair[0]).all()
    good = R.kernel_model(tied, cand, g_depth, g_pmax)
    assert torch.equal(good["argmax"], want["argmax"]) and all(v <= 1.0 for v in _figures(good, want, cond).values())
    bad = R.kernel_model(tied, cand, g_depth, g_pmax, last_maximum=True)
    per_element = R.worst(bad["g_logits"], want["g_logits"], cond["g_logits"])
    pooled = R.pooled_passes(bad["g_logits"], want["g_logits"], R.logits_gradient(tied, cand, g_depth, g_pmax, torch.float32))
    print(f"tie {pair}: last maximum {per_element:.4g} bounds; pooled rule {'passes' if pooled else 'fails'}")
    assert (bad["argmax"] == pair[1]).all() and per_element > 1e3


def test_worst_holds_zero_infinity_and_nan_exactly():
    one, zero, inf = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64), torch.full((1,), float("inf"), dtype=torch.float64)
    assert R.worst(torch.zeros(1), zero, zero) == 0.0
    assert R.worst(torch.full((1,), 2.0 ** -149), zero, zero) == float("inf")       # exactly 0 is asked, not merely one bound
    assert R.worst(torch.full((1,), 2.0 ** -149), zero, one * 2.0 ** -109) <= 1.0
    assert R.worst(torch.full((1,), float("inf")), inf, inf) == 0.0
    assert R.worst(torch.full((1,), float("-inf")), inf, inf) == float("inf")
    assert R.worst(torch.full((1,), 1e30), inf, inf) == float("inf")
    assert not R.worst(torch.full((1,), float("nan")), one, one) <= 1.0
    assert R.worst(torch.full((1,), 1.0 + 2.0 ** -23), one, zero) > 1.0 >= R.worst(torch.ones(1), one * (1.0 + 2.0 ** -24), zero)
