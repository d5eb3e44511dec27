"""The per-row measure of tests/test_gpu_window_attention_float64.py, pinned on the CPU so that the GPU test cannot be vacuous:
window_attention_reference.row_scales gives the statement's values, the float32 lines measure a few units of 2^-24 in every
case the GPU test runs (the condition the GPU test asserts of its yardstick), two planted defects pass the pooled rule of
tests/test_gpu_window_attention.py and fail the per-row rule, and a scale of exactly 0 means "nothing of this row's inputs
reaches it".

Measured (float32 lines on the CPU, 8 cases x shift off / on x input scales 1, 3, 6 = 48 runs; worst row, units of 2^-24):
out 0.01 to 1.16, g_q 0.01 to 0.84, g_k 0.20 to 2.13, g_v 0.36 to 2.17, lse 0.50 to 2.73, delta 0.06 to 0.93.
"""
import functools

import pytest
import torch

import window_attention_reference as R

YARDSTICK_LIMIT = 4.0                                           # units; the GPU test's "yardstick not usable" bound
RUNS = [(name, shift, scale) for name in R.ROW_CASES for shift in (False, True) for scale in (1.0, 3.0, 6.0)]


@functools.lru_cache(maxsize=None)
def _run(name, shift, scale, rule="reference"):
    b, m, h, w, ksp, c = R.ROW_CASES[name]
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=scale, seed=2000 + 7 * sorted(R.ROW_CASES).index(name) + int(shift))
    want, sc = R.row_scales(q, k, v, g, ksp, shift, h, w, rule)
    return (q, k, v, g), want, sc


@pytest.mark.parametrize("name,shift,rule", [("c96", True, "reference"), ("m5", True, "reference"), ("m11", True, "aligned"),
                                             ("m11", True, "reference"), ("k3", True, "reference"), ("thin", True, "reference"),
                                             ("edge", False, "reference")])
@pytest.mark.parametrize("scale", [1.0, 6.0])
def test_row_scales_gives_the_statement_s_values(name, shift, rule, scale):
    (q, k, v, g), want, sc = _run(name, shift, scale, rule)
    b, m, h, w, ksp, c = R.ROW_CASES[name]
    ref = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, ksp, shift, h, w, rule), q, k, v, g, torch.float64)
    for n, x in zip(R.ROW_NAMES, ref):
        assert want[n].dtype == torch.float64 and want[n].shape == x.shape
        assert (want[n] - x).abs().max().item() <= 1e-12 * max(1.0, x.abs().max().item()), n
        assert sc[n].shape == x.shape[:-1] and (sc[n] >= 0).all()
    assert want["lse"].shape == want["delta"].shape == sc["lse"].shape == sc["delta"].shape == q.shape[:2]
    # a correctly rounded result is within half a unit: |want| <= scale, row by row
    for n in R.ROW_NAMES:
        mag = want[n].abs().amax(-1) if want[n].dim() > sc[n].dim() else want[n].abs()
        assert (mag <= sc[n] * (1 + 1e-12)).all(), n


@pytest.mark.parametrize("name,shift,scale", RUNS)
def test_the_float32_lines_measure_a_few_units_in_every_case(name, shift, scale):
    (q, k, v, g), want, sc = _run(name, shift, scale)
    b, m, h, w, ksp, c = R.ROW_CASES[name]
    worst = R.worst_rows(R.lines_rows(q, k, v, g, ksp, shift, h, w), want, sc)
    print(f"[wa64-cpu] {name} shift={int(shift)} scale={scale:g} " + " ".join(f"{n}={x:.2f}" for n, x in worst.items()))
    assert set(worst) == set(R.ROW_NAMES) and all(x <= YARDSTICK_LIMIT for x in worst.values()), worst


def test_the_yardstick_s_lse_and_delta_are_the_lines_own():
    """lines_rows' lse and delta come from reference_lines' own float32 scores and probabilities, and asking for them does not
    change what reference_lines returns."""
    (q, k, v, g), want, sc = _run("m5", True, 1.0)
    b, m, h, w, ksp, c = R.ROW_CASES["m5"]
    mask = R.dense_mask(h, w, ksp)
    parts = {}
    plain = R.reference_lines(q, k, v, ksp, True, h, w, mask)
    again = R.reference_lines(q, k, v, ksp, True, h, w, mask, parts=parts)
    assert torch.equal(plain, again) and parts["scores"].dtype == torch.float32
    assert parts["scores"].shape == parts["probabilities"].shape == (b * ksp * ksp, h * w // ksp ** 2, m * h * w // ksp ** 2)
    lines = R.lines_rows(q, k, v, g, ksp, True, h, w)
    assert torch.equal(lines["out"], plain) and lines["lse"].dtype == lines["delta"].dtype == torch.float32
    tok, _ = R.window_index(h, w, ksp, True)
    assert torch.equal(lines["lse"][:, tok].reshape(-1, tok.shape[1]), torch.logsumexp(parts["scores"], dim=-1))


def _pooled_passes(x, lines, want):
    """The rule of tests/test_gpu_window_attention.py for one tensor."""
    e, el = (x.double() - want).abs(), (lines.double() - want).abs()
    floor = 2.0 ** -24 * want.abs().max().item()
    return e.max().item() <= max(1.5 * el.max().item(), floor) and e.mean().item() <= max(1.5 * el.mean().item(), floor)


def _row_rule_passes(kernel_units, yardstick_units):
    return yardstick_units <= YARDSTICK_LIMIT and kernel_units <= max(2.0 * yardstick_units, 0.5)


def test_planted_defects_pass_the_pooled_rule_and_fail_the_per_row_rule():
    """Shape "multi" of tests/test_gpu_window_attention.py with shift, q and k x 3.  Defect 1: the float32 lines' g_k times
    (1 + 1e-4) on the 10 % of key rows of the smallest scale.  Defect 2: delta off by 1e-5 relative on one query row."""
    b, m, h, w, ksp, c = 2, 3, 8, 12, 2, 128
    q, k, v, g = R.random_case(b, m, h, w, c=c, scale=3.0, seed=1029)
    want, sc = R.row_scales(q, k, v, g, ksp, True, h, w)
    lines = R.lines_rows(q, k, v, g, ksp, True, h, w)
    yard = R.worst_rows(lines, want, sc)
    assert all(_row_rule_passes(yard[n], yard[n]) for n in R.ROW_NAMES), yard                  # the lines themselves pass
    small = sc["g_k"] <= torch.quantile(sc["g_k"].reshape(-1), 0.10)
    bad = torch.where(small.unsqueeze(-1), lines["g_k"] * (1 + 1e-4), lines["g_k"])
    units = R.row_units(bad, want["g_k"], sc["g_k"]).max().item()
    print(f"planted g_k defect: {units:.2f} units, the lines alone {yard['g_k']:.2f}")
    assert _pooled_passes(bad, lines["g_k"], want["g_k"]) and not _row_rule_passes(units, yard["g_k"])
    # delta is compared with nothing in the old file; the pooled rule applied to it does not see the defect either
    err = (lines["delta"].double() - want["delta"]).abs()
    hidden = err + 1e-5 * want["delta"].abs() <= err.max()                                    # rows where the pooled maximum cannot move
    row = torch.where(hidden, want["delta"].abs() / sc["delta"], torch.zeros_like(err)).reshape(-1).argmax().item()
    bad = lines["delta"].clone().reshape(-1)
    bad[row] *= 1 + 1e-5
    bad = bad.reshape(lines["delta"].shape)
    units = R.row_units(bad, want["delta"], sc["delta"]).max().item()
    print(f"planted delta defect: {units:.2f} units, the lines alone {yard['delta']:.2f}")
    assert _pooled_passes(bad, lines["delta"], want["delta"])
    assert not _row_rule_passes(units, yard["delta"])


@pytest.mark.parametrize("name", ["c96", "m5"])
def test_a_one_hot_gradient_gives_scale_zero_where_nothing_arrives(name):
    (q, k, v, g), _, _ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = R.ROW_CASES[name]
    bi, row = b - 1, (h // 2) * w + 3
    hot = torch.zeros_like(g)
    hot[bi, row] = g[bi, row]
    want, sc = R.row_scales(q, k, v, hot, ksp, True, h, w)
    tok, _ = R.window_index(h, w, ksp, True)
    win = (tok == row).any(dim=1).nonzero().item()
    own_window = torch.zeros(h * w, dtype=torch.bool)
    own_window[tok[win]] = True
    for n in ("g_q", "delta"):                                  # every other query row
        expect = torch.zeros(b, h * w, dtype=torch.bool)
        expect[bi, row] = True
        assert torch.equal(sc[n] > 0, expect), n
    for n in ("g_k", "g_v"):                                    # every key of another window, every other batch element
        expect = torch.zeros(b, h * w, dtype=torch.bool)
        expect[bi] = own_window
        expect = expect if m == 0 else expect.unsqueeze(1).expand(b, m, h * w)
        assert torch.equal(sc[n] > 0, expect), n
        assert (want[n][~expect] == 0).all()
    assert (sc["out"] > 0).all() and (sc["lse"] >= 1).all()     # the forward does not see g_out
