"""The per-row measure of tests/test_gpu_transformer_ffn_float64.py, pinned on the CPU so that the GPU test cannot be vacuous: the
cases reach the paths of the launch geometry they are named for (read from the kernel file's constants: a later change of a
constant fails here and does not quietly turn a case into a one-workgroup case), transformer_ffn_reference.row_results is
autograd of the float64 statement with z included, the float32 lines alone meet the rule's conditions in every run, and planted
defects fail the per-row rule — the pooled rule of tests/test_gpu_transformer_ffn.py is applied to each of them too, and what it
says is asserted as it is.

Measured (torch's float32 lines on the CPU, the 19 runs of R.ROW_RUNS but `stride` and the 6 of R.NORM_RUNS; units of 2^-24 of
the row's own magnitude, worst row / the worst row over the median row).  Token rows: out 0.73 to 17.4 / 1.0 to 2.8, z 3.3 to 18.4
/ 1.0 to 2.2, g_source 0.54 to 12.8 / 1.0 to 2.7, g_m 5.3 to 26.2 / 1.0 to 3.2.  Hidden-unit rows (T >= 129): g_w1 13.6 to 23.1 /
1.9 to 3.3, g_w2 14.5 to 25.4 / 2.1 to 2.9.  Channels: norm1's gradients 0.70 to 4.6 / 3.2 to 5.7, norm2's 0.41 to 6.1 / 3.9 to 7.6
(no median condition: the mean rule carries that job).  no_ffn: out 0.96 to 3.4 / 1.6 to 2.9, g_x 3.5 to 4.3 / 2.2 to 3.0, g_weight
and g_bias 0.52 to 1.2 / 3.9 to 7.6, g_residual exact.
"""
import functools
import re
from pathlib import Path

import pytest
import torch

import transformer_ffn_reference as R
from splatter360_amd import _lib

CSRC = Path(__file__).resolve().parent.parent / "splatter360_amd" / "csrc"
CPU_RUNS = [run for run in R.ROW_RUNS if run[0] != "stride"]


@functools.lru_cache(maxsize=None)
def constants():
    """The launch geometry's constants as the kernel file states them: `constexpr int NAME = <integer expression>;` over earlier
    names and the two workgroup macros."""
    values = {}
    for header in ("s360_launch.h", "s360_device.h"):
        for name, number in re.findall(r"^#define (S360_BLOCK|S360_WAVE) (\d+)\b", (CSRC / header).read_text(), flags=re.M):
            values[name] = int(number)
    for name, expr in re.findall(r"^constexpr int (FF_\w+) = ([\w\s*/+()-]+);", (CSRC / "s360_transformer_ffn.hip").read_text(), flags=re.M):
        values[name] = eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(values))    # noqa: S307 (the project's own source)
    return values


def geometry(tokens):
    """ff_chunk_tokens, ff_chunks, ff_token_wgs, ff_row_wgs and the tile counts of the kernel file, restated from its constants."""
    k = constants()
    tm = k["FF_T"] * k["FF_WAVES"]
    tiles = -(-tokens // k["FF_T"])
    chunk_tokens = -(-tiles // k["FF_MAX_CHUNKS"]) * k["FF_T"]
    token_tiles = -(-tokens // tm)
    return dict(tm=tm, tiles=tiles, chunk_tokens=chunk_tokens, chunks=-(-tokens // chunk_tokens), token_tiles=token_tiles,
                token_wgs=min(k["FF_TOKEN_WGS"], token_tiles), row_wgs=min(k["FF_ROW_WGS"], -(-tokens // k["FF_ROWS"])))


def test_the_constants_are_read_from_the_kernel_file():
    k = constants()
    assert {"S360_BLOCK", "S360_WAVE", "FF_T", "FF_WAVES", "FF_TM", "FF_MAX_CHUNKS", "FF_TOKEN_WGS", "FF_ROW_WGS", "FF_ROWS"} <= set(k)
    assert k["FF_TM"] == k["FF_T"] * k["FF_WAVES"] and k["FF_WAVES"] == k["S360_BLOCK"] // k["S360_WAVE"]
    assert k["FF_ROWS"] == k["S360_BLOCK"] // 32 and k["FF_C"] == 128 and k["FF_H"] == 1024
    lib = _lib.lib()
    for name, tokens in R.ROW_CASES.items():                                        # the chunk count is the library's own (host only)
        assert lib.s360_ffn_tail_weight_chunks(tokens) == geometry(tokens)["chunks"], name


def test_every_case_reaches_the_path_it_is_named_for():
    k = constants()
    ft, rows = k["FF_T"], k["FF_ROWS"]
    geo = {name: geometry(tokens) for name, tokens in R.ROW_CASES.items()}
    assert set(R.ROW_CASES) == {"one", "tiny", "ragged", "wg2", "wg3", "tiles2", "tiles3", "rows", "mixed", "stride"}
    tm = geo["one"]["tm"]
    # the pooled file's small shapes: one workgroup, one tile per chunk
    assert R.ROW_CASES["one"] == 1 and R.ROW_CASES["tiny"] < ft and R.ROW_CASES["ragged"] == ft + 1
    assert all(geo[n]["token_tiles"] == 1 and geo[n]["chunk_tokens"] == ft for n in R.SMALL_CASES)
    # wg2: a second workgroup with one valid token in wave 0 and three empty waves
    t = R.ROW_CASES["wg2"]
    assert geo["wg2"]["token_tiles"] == geo["wg2"]["token_wgs"] == 2 and t - tm == 1 and t >= R.UNITS_FROM
    # wg3: three workgroups, the last one a full wave and a one-token wave
    t = R.ROW_CASES["wg3"]
    assert geo["wg3"]["token_tiles"] == geo["wg3"]["token_wgs"] == 3 and t - 2 * tm == ft + 1 and k["FF_WAVES"] >= 2
    # tiles2: 18 tiles in 9 chunks of two tiles; the last chunk is one full tile and a one-token tile
    t, g = R.ROW_CASES["tiles2"], geo["tiles2"]
    assert g["tiles"] == 18 and g["chunks"] == 9 and g["chunk_tokens"] == 2 * ft and t - 8 * g["chunk_tokens"] == ft + 1
    # tiles3: 34 tiles in 12 chunks of three tiles; the last chunk is 7 tokens
    t, g = R.ROW_CASES["tiles3"], geo["tiles3"]
    assert g["tiles"] == 34 and g["chunks"] == 12 and g["chunk_tokens"] == 3 * ft and t - 11 * g["chunk_tokens"] == 7
    # rows: the row backward's grid stride; workgroup 0 takes a second round of 8 rows, workgroup 1 one of 3, the others none
    t, g = R.ROW_CASES["rows"], geo["rows"]
    span = k["FF_ROW_WGS"] * rows
    assert g["row_wgs"] == k["FF_ROW_WGS"] and span < t < 2 * span
    second = [sum(1 for slot in range(rows) if span + wg * rows + slot < t) for wg in range(3)]
    assert second == [rows, 3, 0] and g["chunk_tokens"] > ft
    # mixed: two workgroups, every gain in each, enough tokens for the hidden-unit rows
    t = R.ROW_CASES["mixed"]
    assert geo["mixed"]["token_tiles"] == 2 and t - tm >= len(R.MIXED_GAINS) and t >= R.UNITS_FROM
    # stride: 514 token tiles on 512 workgroups; workgroups 0 and 1 walk two tiles, the second one of workgroup 1 has 5 tokens
    t, g = R.ROW_CASES["stride"], geo["stride"]
    assert g["token_wgs"] == k["FF_TOKEN_WGS"] and g["token_tiles"] == k["FF_TOKEN_WGS"] + 2 and t - (g["token_tiles"] - 1) * tm == 5
    assert (k["FF_TOKEN_WGS"] + 1) * tm < t                                          # and T - 5 would still stride: the tile of 5 is chosen
    # no other case strides over token tiles, and only `rows` and `stride` stride over rows
    for name, tokens in R.ROW_CASES.items():
        assert (geo[name]["token_tiles"] > k["FF_TOKEN_WGS"]) == (name == "stride"), name
        assert (tokens > span) == (name in ("rows", "stride")), name
    # the runs: every case but stride at both scales, stride once; the no_ffn tail on wg2, rows and mixed
    assert sorted(R.ROW_RUNS) == sorted([(n, s) for n in R.ROW_CASES if n != "stride" for s in (1.0, 6.0)] + [("stride", 1.0)])
    assert sorted(R.NORM_RUNS) == sorted((n, s) for n in ("wg2", "rows", "mixed") for s in (1.0, 6.0))
    assert all(R.row_names(R.ROW_CASES[n]) == (R.TOKEN_ROWS if n in R.SMALL_CASES else R.FFN_ROW_NAMES) for n in R.ROW_CASES)


def test_the_inputs_are_random_case_s_and_mixed_scales_the_rows_of_g():
    tensors, g = R.row_inputs("mixed", 6.0)
    seed = 5000 + 7 * sorted(R.ROW_CASES).index("mixed")
    plain, g0 = R.random_case(R.ROW_CASES["mixed"], scale=6.0, seed=R.ROW_SEEDS.get("mixed", seed))
    assert all(torch.equal(a, b) for a, b in zip(tensors, plain))
    gains = torch.tensor([R.MIXED_GAINS[i % 4] for i in range(g.shape[0])])
    assert torch.equal(g, g0 * gains[:, None]) and g.shape == (161, 128)
    tensors, g = R.row_inputs("wg3", 1.0)
    assert all(t.dtype == torch.float32 for t in (*tensors, g)) and tensors[0].shape == g.shape == (289, 128)


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    tensors, g = R.row_inputs(name, scale)
    want, sc = R.row_statement(tensors, g)
    return (tensors, g), want, sc, R.lines_rows(tensors, g)


@functools.lru_cache(maxsize=None)
def _run_norm(name, scale):
    tensors, g = R.norm_case(R.row_inputs(name, scale))
    want, sc = R.norm_row_statement(tensors, g)
    return (tensors, g), want, sc, R.norm_lines_rows(tensors, g)


@pytest.mark.parametrize("name,scale", [("tiny", 6.0), ("wg2", 1.0), ("mixed", 6.0), ("tiles2", 1.0)])
def test_row_results_is_autograd_of_the_float64_statement(name, scale):
    (tensors, g), want, sc, _ = _run(name, scale)
    out, *grads = R.gradients(lambda *t: R.statement(*t), tensors, g, torch.float64)
    ref = dict(zip(("out", *("g_" + n for n in R.TAIL_NAMES)), (out, *grads)))
    source, m, n1w, n1b, w1, w2, n2w, n2b = (t.double() for t in tensors)
    y = R.layer_norm(m, n1w, n1b, 1e-5)
    ref["z"] = R.gelu(torch.cat([source, y], dim=-1) @ w1.T) @ w2.T
    again = R.row_results(tensors, g)
    assert set(want) == set(sc) == set(again) == set(R.FFN_ROW_NAMES)
    for n in R.FFN_ROW_NAMES:
        x = ref[n].t() if n == "g_w2" else ref[n]
        assert want[n].dtype == sc[n].dtype == torch.float64 and want[n].shape == x.shape and torch.equal(want[n], again[n]), n
        assert (want[n] - x).abs().max().item() <= 1e-12 * max(1.0, x.abs().max().item()), n
        assert sc[n].shape == x.shape[:1] and (sc[n] >= 0).all(), n
        mag = want[n].abs().amax(-1) if want[n].dim() == 2 else want[n].abs()
        assert (mag <= sc[n] * (1 + 1e-12)).all(), n                                # a correctly rounded result is within half a unit
    assert want["g_w2"].shape == (1024, 128) and want["g_w1"].shape == (1024, 256) and want["z"].shape == g.shape
    assert all(torch.equal(R.row_scales(tensors, g)[n], sc[n]) for n in sc)
    # the channel scales are the sums over tokens of the summed terms' magnitudes, and the sums of the terms are the gradients
    xh2 = (ref["z"] - ref["z"].mean(-1, keepdim=True)) / torch.sqrt(ref["z"].var(-1, unbiased=False, keepdim=True) + 1e-5)
    assert (((g.double() * xh2).sum(0) - want["g_norm2_weight"]).abs() <= 1e-12 * sc["g_norm2_weight"]).all()
    assert torch.equal(sc["g_norm2_bias"], g.double().abs().sum(0))
    for n in ("g_norm1_bias", "g_norm1_weight"):
        assert (sc[n] * (1 + 1e-12) >= want[n].abs()).all(), n


def test_the_no_ffn_rows_are_autograd_of_the_float64_statement():
    (tensors, g), want, sc, lines = _run_norm("mixed", 1.0)
    ref = R.gradients(lambda *t: R.norm_statement(*t), tensors, g, torch.float64)
    assert set(want) == set(lines) == set(R.NORM_ROW_NAMES) and set(sc) == set(R.NORM_ROW_NAMES) - {"g_residual"}
    for n, x in zip(("out", "g_x", "g_weight", "g_bias", "g_residual"), ref):
        assert torch.equal(want[n], x) and lines[n].dtype == torch.float32 and lines[n].shape == x.shape, n
    assert torch.equal(want["g_residual"], g.double()) and torch.equal(lines["g_residual"], g)
    assert torch.equal(sc["g_bias"], g.double().abs().sum(0)) and (sc["g_weight"] >= want["g_weight"].abs()).all()


@pytest.mark.parametrize("name,scale", CPU_RUNS)
def test_the_float32_lines_alone_meet_the_rule_s_conditions(name, scale):
    """The yardstick against itself: its worst row is within 5 medians (token and hidden-unit rows), every figure is finite, and
    nothing but the quantities judged at this T is looked at."""
    _, want, sc, lines = _run(name, scale)
    names = R.row_names(R.ROW_CASES[name])
    for n in names:
        failures, (kworst, kmean, yworst, ymean, ymedian) = R.rule_failures(n, lines[n], lines[n], want[n], sc[n])
        print(f"[ff64-cpu] {name}/x{scale:g} {n} worst {yworst:.3f} mean {ymean:.3f} median {ymedian:.3f}")
        assert not failures and kworst == yworst and 0 < ymedian <= ymean * 2 and yworst < 64, (n, failures)


@pytest.mark.parametrize("name,scale", R.NORM_RUNS)
def test_the_no_ffn_lines_alone_meet_the_rule_s_conditions(name, scale):
    (_, g), want, sc, lines = _run_norm(name, scale)
    for n in R.NORM_ROW_NAMES[:-1]:
        failures, (_, _, yworst, ymean, ymedian) = R.rule_failures(n, lines[n], lines[n], want[n], sc[n])
        print(f"[ff64-cpu] norm {name}/x{scale:g} {n} worst {yworst:.3f} mean {ymean:.3f} median {ymedian:.3f}")
        assert not failures and yworst < 16, (n, failures)
    assert torch.equal(lines["g_residual"], g)


def test_the_rule_s_arithmetic():
    """On made-up rows: the floors, the two factors, the median condition and its exemption, the dead row, a NaN."""
    want = torch.full((8, 4), 0.375, dtype=torch.float64)                       # float32 steps of half a unit around it
    sc = torch.ones(8, dtype=torch.float64)
    off = lambda units: (want + units * R.UNIT * torch.eye(8, 4, dtype=torch.float64)[:, :1]).float()   # noqa: E731 (row 0 is off)
    exact = want.float()
    fails = lambda n, x, lines: [f[1] for f in R.rule_failures(n, x, lines, want, sc)[0]]     # noqa: E731
    assert fails("out", off(4), exact) == ["worst row"]                             # 4 units in one row: mean 0.5, the floor
    assert fails("out", off(3.5), exact) == ["worst row"] and fails("out", off(0.5), exact) == []
    every = lambda units: (want + units * R.UNIT).float()                          # noqa: E731
    assert fails("out", every(4), every(2)) == ["mean row"]                         # worst 4 <= 2 x 2, mean 4 > 1.5 x 2
    assert fails("out", every(2), every(2)) == [] and fails("out", every(3), every(2)) == []
    assert fails("out", exact, off(8)) == ["yardstick not usable"]                  # the median is 0
    assert fails("g_norm1_bias", exact, off(8)) == []                               # the channels have no such condition
    dead = sc.clone()
    dead[3] = 0.0
    zero = torch.where(dead[:, None] == 0, 0.0, want)
    x = zero.float()
    assert R.rule_failures("out", x, x, zero, dead)[0] == []
    x[3, 2] = 1e-30
    assert R.rule_failures("out", x, zero.float(), zero, dead)[0][0][1] == "a row of scale 0 is not 0"
    x = exact.clone()
    x[5, 1] = float("nan")
    assert fails("out", x, every(2)) == ["worst row", "mean row"]


# ---- planted defects: the float64 results rounded to float32, one defect each, under both rules ---------------------------------

def _pooled_passes(x, lines, want):
    """The rule of tests/test_gpu_transformer_ffn.py (_check_rule) for one tensor."""
    e, el = (x.double() - want).abs(), (lines.double() - want).abs()
    floor = 2.0 ** -24 * want.abs().max().item()
    return bool(torch.isfinite(x).all()) and e.max().item() <= max(1.5 * el.max().item(), floor) and e.mean().item() <= max(1.5 * el.mean().item(), floor)


def _both_rules(n, x, run):
    _, want, sc, lines = run
    failures, fig = R.rule_failures(n, x, lines[n], want[n], sc[n])
    return _pooled_passes(x, lines[n], want[n]), failures, fig


def _quiet_row(sc):
    """A token of `mixed` with gain 1e-3, in the second workgroup."""
    row = 128 + 3 + 4 * 3
    assert row % 4 == 3 and R.MIXED_GAINS[3] == 1e-3 and row < sc["g_m"].shape[0]
    return row


@pytest.mark.parametrize("scale", R.ROW_SCALES)
def test_the_correctly_rounded_results_pass_both_rules(scale):
    run = _run("mixed", scale)
    for n in R.FFN_ROW_NAMES:
        pooled, failures, fig = _both_rules(n, run[1][n].float(), run)
        assert pooled and not failures and fig[0] <= 1.0, (n, failures, fig)       # half a float32 step is 0.5 to 1 unit of the value


def test_a_quiet_token_row_with_its_neighbour_s_values_fails_per_row():
    """g_source and g_m of a row whose g is 1e-3 of its neighbour's, replaced by the row behind it (g x 1).  The pooled rule sees
    this one too (the neighbour's values are of the size of the largest, far above the lines' error); it is here as the plainest
    form of a token that reads another token's data."""
    run = _run("mixed", 1.0)
    _, want, sc, _ = run
    row = _quiet_row(sc)
    for n in ("g_source", "g_m"):
        x = want[n].float()
        x[row] = x[row + 1]
        pooled, failures, fig = _both_rules(n, x, run)
        print(f"planted neighbour row in {n}: {fig[0]:.3g} units against the lines' {fig[2]:.2f}; pooled rule passes: {pooled}")
        assert sc[n][row] < 0.01 * sc[n][row + 1] and not pooled and [f[1] for f in failures] == ["worst row", "mean row"], n


def test_a_quiet_row_of_g_m_off_by_64_units_passes_the_pooled_rule_and_fails_per_row():
    run = _run("mixed", 1.0)
    _, want, sc, _ = run
    row = _quiet_row(sc)
    x = want["g_m"].double().clone()
    x[row] += 64 * R.UNIT * sc["g_m"][row]
    pooled, failures, fig = _both_rules("g_m", x.float(), run)
    print(f"planted 64 units in a quiet row of g_m: {fig[0]:.2f} units against the lines' {fig[2]:.2f}")
    assert pooled and [f[1] for f in failures] == ["worst row"] and 60 < fig[0] < 68


def test_a_zeroed_hidden_unit_of_g_w1_fails_per_row():
    """One row of g_w1 zero: an error of the row's whole magnitude, 2^24 units.  Every row of g_w1 is of the same order here, so
    the pooled maximum sees it as well."""
    run = _run("mixed", 1.0)
    x = run[1]["g_w1"].float()
    x[517] = 0.0
    pooled, failures, fig = _both_rules("g_w1", x, run)
    print(f"planted zero row in g_w1: {fig[0]:.3g} units against the lines' {fig[2]:.2f}; pooled rule passes: {pooled}")
    assert not pooled and [f[1] for f in failures] == ["worst row", "mean row"] and fig[0] == pytest.approx(2.0 ** 24, rel=1e-6)


def test_a_channel_of_g_norm1_weight_off_by_64_units_fails_per_row():
    """64 units of the channel's scale, the sum of the magnitudes of its 161 terms.  The lines' worst channel is at 4 units of
    its scale and the tensor has 128 values, so the pooled maximum sees this one as well."""
    run = _run("mixed", 1.0)
    _, want, sc, _ = run
    n = "g_norm1_weight"
    x = want[n].clone()
    x[77] += 64 * R.UNIT * sc[n][77]
    pooled, failures, fig = _both_rules(n, x.float(), run)
    print(f"planted 64 units in a channel of {n}: {fig[0]:.2f} units against the lines' {fig[2]:.2f}; pooled rule passes: {pooled}")
    assert not pooled and [f[1] for f in failures] == ["worst row"] and 60 < fig[0] < 68


def test_a_row_of_z_left_at_nan_fails_per_row():
    """z is compared with nothing in the pooled file (it is not among its FFN_OUT); the per-row rule holds it like out."""
    import ast
    source = (Path(__file__).resolve().parent / "test_gpu_transformer_ffn.py").read_text()
    pooled_names = next(ast.literal_eval(node.value) for node in ast.parse(source).body
                        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "FFN_OUT")
    assert "z" not in pooled_names and set(pooled_names) == set(R.FFN_ROW_NAMES) - {"z"}
    run = _run("mixed", 1.0)
    x = run[1]["z"].float()
    x[130] = float("nan")
    _, failures, _ = _both_rules("z", x, run)
    assert [f[1] for f in failures] == ["worst row", "mean row"]
