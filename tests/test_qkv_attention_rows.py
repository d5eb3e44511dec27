"""The per-row measure of tests/test_gpu_qkv_attention_float64.py, pinned on the CPU so that the GPU test cannot be vacuous:
qkv_attention_reference.row_scales gives the statement's values in the per-row indexing, the float32 lines measure a few units of
2^-24 in every run the GPU test makes (the condition the GPU test asserts of its yardstick), planted defects pass the pooled
rule of tests/test_gpu_qkv_attention.py and fail the per-row rule, and a scale of exactly 0 means "nothing of this row's inputs
reaches it": another head, another batch element, another query.

Measured (float32 lines on the CPU, the 38 runs of R.ROW_RUNS; worst row, units of 2^-24): out 0.00 to 1.69, g_q 0.00 to 0.87,
g_k 0.00 to 2.38, g_v 0.00 to 2.45, lse 0.14 to 2.26, delta 0.01 to 0.72 (the zeros are `one` at scale 6: two keys, all weight on
one; the largest out, g_q and delta are `mixed`, the largest g_k and g_v `frames_unused` at scale 6).  Planted: g_k x (1 + 1e-4) on
the tenth of key rows of smallest scale 9.45 units against the lines' 1.37; one row of delta x (1 + 1e-5) 5.77 against 0.72; head 0's
out leaking into head 3's 42.15 (1e-6, one tile) and 8.33 (2e-7, everywhere) against 1.69; all pass the pooled rule.
"""
import functools

import pytest
import torch

import qkv_attention_reference as R

YARDSTICK_LIMIT = 4.0                                           # units; the GPU test's "yardstick not usable" bound


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    qkv, g = R.row_inputs(name, scale)
    want, sc = R.row_scales(qkv, g, heads, views, cross, order)
    return (qkv, g), want, sc


def test_the_default_random_case_is_unchanged_and_the_factors_land_on_their_rows():
    """The golden file and the pooled GPU test depend on random_case's default tensors: the generator's first draws, times
    scale.  head_scales multiplies the q and k rows of each head where they lie in the given order, row_gains the rows of g."""
    gen = torch.Generator().manual_seed(7)
    qkv0, g0 = torch.randn(2, 4 * 96, 5, generator=gen) * 3.0, torch.randn(2, 4 * 32, 5, generator=gen)
    qkv, g = R.random_case(2, 4, 5, scale=3.0, seed=7)
    assert torch.equal(qkv, qkv0) and torch.equal(g, g0)
    hs, gains = (6.0, 2.2, 0.8, 0.3), (1.0, 1e-2)
    for order in R.ORDERS:
        x, gg = R.random_case(2, 4, 5, scale=3.0, seed=7, head_scales=hs, row_gains=gains, order=order)
        for got, plain, f in zip(R.parts(x, 4, order), R.parts(qkv0, 4, order), (hs, hs, (1.0,) * 4)):
            assert torch.equal(got, plain * torch.tensor(f).view(1, 4, 1, 1)), order
        assert torch.equal(gg, g0 * torch.tensor(gains).view(2, 1, 1))


@pytest.mark.parametrize("name", list(R.ROW_CASES))
def test_the_layout_maps_are_each_other_s_inverses(name):
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    qkv, g = R.row_inputs(name)
    b, length = n // (views if cross else 1), (views if cross else 1) * t
    rows = R.qkv_rows(qkv, heads, views, cross, order)
    assert all(x.shape == (b, heads, length, 32) for x in rows) and R.out_rows(g, heads, views, cross).shape == (b, heads, length, 32)
    assert torch.equal(R.qkv_from_rows(*rows, views, cross, order), qkv)
    assert torch.equal(R.out_from_rows(R.out_rows(g, heads, views, cross), views, cross), g)
    vec = R.out_rows(g, heads, views, cross)[..., 5]                                # channel 5 of every head, per row
    assert torch.equal(R.vector_to_out(vec, views, cross), g.reshape(n, heads, 32, t)[:, :, 5])
    assert torch.equal(R.vector_from_out(R.vector_to_out(vec, views, cross), views, cross), vec)
    # joint token s of batch element bi is token s mod T of batch row (s // T) B + bi
    bi, hd, s = b - 1, heads - 1, length - 1
    assert torch.equal(R.out_rows(g, heads, views, cross)[bi, hd, s], g[(s // t) * b + bi, hd * 32:(hd + 1) * 32, s % t])


@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_row_scales_gives_the_statement_s_values(name, scale):
    (qkv, g), want, sc = _run(name, scale)
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    out, g_qkv = R.gradients(lambda x: R.statement(x, heads, views, cross, order), qkv, g, torch.float64)
    ref = dict(zip(R.ROW_NAMES, (R.out_rows(out, heads, views, cross), *R.qkv_rows(g_qkv, heads, views, cross, order))))
    # lse from the statement's own scaled operands; Delta_i = sum_c g_ic out_ic, the identity the kernels do NOT use
    q, k, _ = (x.double() * 32 ** -0.25 for x in R.split_heads(qkv, heads, views, cross, order))
    ref["lse"] = torch.logsumexp(torch.einsum("bhct,bhcs->bhts", q, k), dim=-1)
    ref["delta"] = (R.out_rows(g.double(), heads, views, cross) * ref["out"]).sum(-1)
    assert set(want) == set(sc) == set(R.ROW_NAMES)
    for name_, x in ref.items():
        assert want[name_].dtype == sc[name_].dtype == torch.float64 and want[name_].shape == x.shape, name_
        assert (want[name_] - x).abs().max().item() <= 1e-12 * max(1.0, x.abs().max().item()), name_
        assert sc[name_].shape == x.shape[:3] and (sc[name_] >= 0).all(), name_
        # a correctly rounded result is within half a unit: |want| <= scale, row by row
        mag = want[name_].abs().amax(-1) if want[name_].dim() == 4 else want[name_].abs()
        assert (mag <= sc[name_] * (1 + 1e-12)).all(), name_


@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_the_float32_lines_measure_a_few_units_in_every_case(name, scale):
    (qkv, g), want, sc = _run(name, scale)
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    worst = R.worst_rows(R.lines_rows(qkv, g, heads, views, cross, order), want, sc)
    print(f"[qa64-cpu] {name} scale={scale:g} " + " ".join(f"{n_}={x:.2f}" for n_, x in worst.items()))
    assert set(worst) == set(R.ROW_NAMES) and all(x <= YARDSTICK_LIMIT for x in worst.values()), worst


@pytest.mark.parametrize("name", ["straddle", "new_mixed"])
def test_the_yardstick_s_lse_and_delta_are_the_lines_own(name):
    """lines_rows' lse and delta come from reference_lines' own float32 scores and probabilities, and asking for them does not
    change what reference_lines returns."""
    (qkv, g), want, sc = _run(name, 1.0)
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    b, length = n // (views if cross else 1), (views if cross else 1) * t
    got = {}
    plain = R.reference_lines(qkv, heads, views, cross, order)
    again = R.reference_lines(qkv, heads, views, cross, order, parts=got)
    assert torch.equal(plain, again) and set(got) == {"scores", "probabilities", "values"}
    assert got["scores"].dtype == got["probabilities"].dtype == torch.float32
    assert got["scores"].shape == got["probabilities"].shape == (b * heads, length, length) and got["values"].shape == (b * heads, 32, length)
    assert torch.equal(got["probabilities"], torch.softmax(got["scores"], dim=-1))
    lines = R.lines_rows(qkv, g, heads, views, cross, order)
    assert torch.equal(lines["out"], R.out_rows(plain, heads, views, cross))
    assert lines["lse"].dtype == lines["delta"].dtype == torch.float32 and lines["lse"].shape == lines["delta"].shape == (b, heads, length)
    assert torch.equal(lines["lse"].reshape(b * heads, length), torch.logsumexp(got["scores"], dim=-1))
    dp = torch.einsum("bct,bcs->bts", R.joint(g, heads, views, cross).reshape(b * heads, 32, length), got["values"])
    assert torch.equal(lines["delta"].reshape(b * heads, length), (got["probabilities"] * dp).sum(-1))


def _pooled_passes(x, lines, want):
    """The rule of tests/test_gpu_qkv_attention.py (_check_rule) for one tensor."""
    e, el = (x.double() - want).abs(), (lines.double() - want).abs()
    floor = 2.0 ** -24 * want.abs().max().item()
    return e.max().item() <= max(1.5 * el.max().item(), floor) and e.mean().item() <= max(1.5 * el.mean().item(), floor)


def _row_rule_passes(kernel_units, yardstick_units):
    return yardstick_units <= YARDSTICK_LIMIT and kernel_units <= max(2.0 * yardstick_units, 0.5)


def _lines(name, scale):
    (qkv, g), want, sc = _run(name, scale)
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    lines = R.lines_rows(qkv, g, heads, views, cross, order)
    yard = R.worst_rows(lines, want, sc)
    assert all(_row_rule_passes(yard[n_], yard[n_]) for n_ in R.ROW_NAMES), yard      # the lines themselves pass
    return want, sc, lines, yard


def test_a_scaled_g_k_on_the_rows_of_small_scale_passes_the_pooled_rule_and_fails_per_row():
    """`straddle` at input scale 6, where the scale of g_k spans many orders of magnitude within one tensor: the float32 lines'
    g_k times (1 + 1e-4) on the 10 % of key rows of the smallest scale.  The pooled rule is applied to g_k alone and to the whole
    g_qkv in qkv's layout, as the pooled file applies it."""
    want, sc, lines, yard = _lines("straddle", 6.0)
    n, views, cross, heads, t, order = R.ROW_CASES["straddle"]
    spread = sc["g_k"].max().item() / sc["g_k"].min().item()
    small = sc["g_k"] <= torch.quantile(sc["g_k"].reshape(-1), 0.10)
    bad = torch.where(small.unsqueeze(-1), lines["g_k"] * (1 + 1e-4), lines["g_k"])
    units = R.row_units(bad, want["g_k"], sc["g_k"]).max().item()
    print(f"planted g_k defect: {units:.2f} units, the lines alone {yard['g_k']:.2f}; the scale of g_k spans a factor {spread:.1e}")
    assert spread > 1e3
    assert _pooled_passes(bad, lines["g_k"], want["g_k"])
    whole = lambda d, k: R.qkv_from_rows(d["g_q"], k, d["g_v"], views, cross, order)
    assert _pooled_passes(whole(lines, bad), whole(lines, lines["g_k"]), whole(want, want["g_k"]))
    assert not _row_rule_passes(units, yard["g_k"])


def test_one_row_of_delta_off_by_1e_5_passes_the_pooled_rule_and_fails_per_row():
    """Delta is compared with nothing in the pooled file; the pooled rule applied to it does not see the defect either.  On
    `mixed`, where the rows' g differ by factors of ten: the pooled maximum is the error of a row of gain 1, and a row of gain
    1e-1 or less hides under it.  (The scale of Delta is at least (1 + 2 A) |Delta|, so 1e-5 of Delta is at most 170 / (1 + 2 A)
    units: the plant shows in a head of small A; at A of some hundreds it is inside what the measure grants a float32 score.)"""
    want, sc, lines, yard = _lines("mixed", 1.0)
    err = (lines["delta"].double() - want["delta"]).abs()
    hidden = err + 1e-5 * want["delta"].abs() <= err.max()                          # rows where the pooled maximum cannot move
    row = torch.where(hidden, want["delta"].abs() / sc["delta"], torch.zeros_like(err)).reshape(-1).argmax().item()
    bad = lines["delta"].clone().reshape(-1)
    bad[row] *= 1 + 1e-5
    bad = bad.reshape(lines["delta"].shape)
    units = R.row_units(bad, want["delta"], sc["delta"]).max().item()
    print(f"planted delta defect: {units:.2f} units, the lines alone {yard['delta']:.2f}")
    assert _pooled_passes(bad, lines["delta"], want["delta"]) and not _row_rule_passes(units, yard["delta"])


def test_a_leak_between_heads_passes_the_pooled_rule_and_fails_per_row():
    """`mixed`: head 0's out (q, k x 6: the float32 lines err most there, 1.5e-5 at the worst element and 1.5e-7 in the mean over the
    tensor) leaks into the out of the smallest head (x 0.3): 1e-6 of it within one 32-query owner tile (the one that spans both
    views of the last batch element), and 2e-7 of it everywhere.  1e-6 of it everywhere adds 1.9e-7 to the pooled mean, which
    the pooled rule does catch: that plant does not belong here.  Then the same kind of leak in g_v, from batch element 0 (g x 1,
    1e-2) into batch element 1 (g x 1e-1, 1e-3)."""
    want, sc, lines, yard = _lines("mixed", 1.0)
    n, views, cross, heads, t, order = R.ROW_CASES["mixed"]
    for what, factor, rows in (("one tile", 1e-6, slice(32, 64)), ("everywhere", 2e-7, slice(None))):
        bad = lines["out"].clone()
        bad[-1, heads - 1, rows] += factor * lines["out"][-1, 0, rows]
        if what == "everywhere":
            bad[:-1, heads - 1] += factor * lines["out"][:-1, 0]
        units = R.row_units(bad, want["out"], sc["out"]).max().item()
        print(f"planted head leak in out, {factor:g} {what}: {units:.2f} units, the lines alone {yard['out']:.2f}")
        assert _pooled_passes(bad, lines["out"], want["out"]), what
        assert _pooled_passes(R.out_from_rows(bad, views, cross), R.out_from_rows(lines["out"], views, cross),
                              R.out_from_rows(want["out"], views, cross)), what
        assert not _row_rule_passes(units, yard["out"]), what
    bad = lines["g_v"].clone()
    bad[1] += 1e-6 * lines["g_v"][0]
    units = R.row_units(bad, want["g_v"], sc["g_v"]).max().item()
    print(f"planted batch leak in g_v: {units:.3g} units (keys of head 0 that no query attends to), the lines alone {yard['g_v']:.2f}")
    assert _pooled_passes(bad, lines["g_v"], want["g_v"]) and not _row_rule_passes(units, yard["g_v"])


@pytest.mark.parametrize("name", ["straddle", "thin4", "new_mixed"])
def test_a_one_hot_gradient_gives_scale_zero_where_nothing_arrives(name):
    """g non-zero at one token of one head of the last batch row (the last view of the last batch element)."""
    (qkv, g), _, _ = _run(name, 1.0)
    n, views, cross, heads, t, order = R.ROW_CASES[name]
    nv = views if cross else 1
    b, length = n // nv, nv * t
    hd, tok = heads - 1, t // 2
    hot = torch.zeros_like(g)
    hot[n - 1, hd * 32:(hd + 1) * 32, tok] = g[n - 1, hd * 32:(hd + 1) * 32, tok]
    want, sc = R.row_scales(qkv, hot, heads, views, cross, order)
    bi, s = b - 1, (nv - 1) * t + tok
    for n_ in ("g_q", "delta"):                                 # every other query row
        expect = torch.zeros(b, heads, length, dtype=torch.bool)
        expect[bi, hd, s] = True
        assert torch.equal(sc[n_] > 0, expect), n_
    for n_ in ("g_k", "g_v"):                                   # all L keys of its (batch element, head), across all views
        expect = torch.zeros(b, heads, length, dtype=torch.bool)
        expect[bi, hd] = True
        assert torch.equal(sc[n_] > 0, expect) and int(expect.sum()) == length, n_
    for n_ in ("g_q", "g_k", "g_v", "delta"):
        assert (want[n_][sc[n_] == 0] == 0).all(), n_
    assert (sc["out"] > 0).all() and (sc["lse"] >= 1).all()     # the forward does not see g
