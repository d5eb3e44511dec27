"""The per-row measure of tests/test_gpu_mono_fusion_float64.py, pinned on the CPU so that the GPU test cannot be vacuous: the cases
reach the paths of the launch geometry they are named for (read from the kernel file's constants: a later change of a constant
fails here and does not quietly turn a case into a small one), mono_fusion_reference.row_statement is autograd of the float64
statement with y included, the float32 lines alone and the three-term statement alone meet the rule's conditions in every run, and
planted defects fail the per-row rule — the pooled rule of tests/test_gpu_mono_fusion.py is applied to each of them too, and what
it says is asserted as it is.

Measured (torch's float32 lines on the CPU, the 18 runs of R.ROW_RUNS with the "highest" seeds; units of 2^-24 of the row's own
scale, worst row / the worst row over the median row, rows of scale 0 left out).  Token rows: out 6.7 to 14.6 / 1.5 to 2.6, y 9.0
to 20.9 / 1.5 to 3.3, g_erp_feat 9.4 to 17.0 / 1.5 to 3.0.  Column rows (T >= 129): g_w1 10.5 to 18.4 / 1.8 to 2.7, g_w2 6.4 to
19.0 / 1.4 to 2.8 (62 to 71 of its 128 rows are dead units in the decided cases: scale 0, exactly 0).  Channels: g_ln_weight 0.48
to 4.0 / 3.2 to 5.8, g_ln_bias 0.31 to 1.7 / 3.2 to 4.0 (no median condition: the mean rule carries that job).  The three-term
statement with the "high" seeds: token and column rows 93 to 264 / 1.2 to 2.5, channels 2.7 to 59 / 2.9 to 5.9.
"""
import ast
import functools
import re
from pathlib import Path

import pytest
import torch

import mono_fusion_high_reference as HR
import mono_fusion_reference as R
import transformer_ffn_reference as FF
import window_attention_reference as W
from splatter360_amd import _lib

TESTS = Path(__file__).resolve().parent
CSRC = TESTS.parent / "splatter360_amd" / "csrc"
KERNEL_FILE = CSRC / "s360_mono_fusion.hip"
NEW_CASES = ("wg2", "mixed", "tiles3", "tiles5")
POOLED_ROW_CASES = ("wave", "tile", "straddle", "config", "wide")
C = 128


@functools.lru_cache(maxsize=None)
def constants():
    """The launch geometry's constants as the kernel file states them: `constexpr int NAME = <integer expression>;` over earlier
    names and the two workgroup macros, and the batch of k_mf_reduce's loop over the LayerNorm partials."""
    values = {}
    for header in ("s360_launch.h", "s360_device.h"):
        for name, number in re.findall(r"^#define (S360_BLOCK|S360_WAVE) (\d+)\b", (CSRC / header).read_text(), flags=re.M):
            values[name] = int(number)
    text = KERNEL_FILE.read_text()
    for name, expr in re.findall(r"^constexpr int (MF_\w+) = ([\w\s*/+()-]+);", text, flags=re.M):
        values[name] = eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(values))    # noqa: S307 (the project's own source)
    (a, b), = re.findall(r"for \(; c \+ (\d+) <= parts; c \+= (\d+)\)", text)
    assert a == b
    values["REDUCE_BATCH"] = int(a)
    return values


def geometry(tokens):
    """mf_tiles, mf_chunks, mf_token_wgs and the chunk bounds `first = (chunk * tiles / chunks) * MF_WT` of the kernel file,
    restated from its constants: the tokens of every tile of every chunk, and the tokens of every token workgroup."""
    k = constants()
    wt, tm = k["MF_WT"], k["MF_TM"]
    tiles = -(-tokens // wt)
    chunks = min(k["MF_MAX_CHUNKS"], tiles)
    chunk_tiles = []                                            # per chunk: the token counts of its tiles
    for chunk in range(chunks):
        first, last = (chunk * tiles // chunks) * wt, min(tokens, ((chunk + 1) * tiles // chunks) * wt)
        chunk_tiles.append([min(wt, last - t0) for t0 in range(first, last, wt)])
    wgs = -(-tokens // tm)
    return dict(tiles=tiles, chunks=chunks, chunk_tiles=chunk_tiles, per_chunk=sorted({len(c) for c in chunk_tiles}), wgs=wgs,
                wg_tokens=[min(tm, tokens - w * tm) for w in range(wgs)], batches=divmod(wgs, k["REDUCE_BATCH"]))


def panoramas_per_wave(tokens, hw):
    """The set of the numbers of panoramas that the 32 tokens of a wave of the token-owned kernels belong to."""
    t = constants()["MF_T"]
    return {len({tok // hw for tok in range(w0, min(w0 + t, tokens))}) for w0 in range(0, tokens, t)}


def _literal(path, name):
    return next(ast.literal_eval(node.value) for node in ast.parse(path.read_text()).body
                if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name)


def _hw(geometry_):
    _, h, w = R.GEOMETRIES[geometry_] if isinstance(geometry_, str) else geometry_
    return h * w


def pooled_tokens():
    """name: (tokens, H W) of the cases of tests/test_gpu_mono_fusion.py (the "high" file runs the same ones); `chunks` is its
    _chunks_n(): the smallest N on g3 with three chunks and a ragged last one."""
    cases = _literal(TESTS / "test_gpu_mono_fusion.py", "CASES")
    out = {}
    for name, (n, geo, _, _) in cases.items():
        hw = _hw(geo)
        if n is None:
            n = next(i for i in range(1, 64) if geometry(i * hw)["chunks"] >= 3 and (i * hw) % 64)
        out[name] = (n * hw, hw)
    return out


def test_the_constants_are_read_from_the_kernel_file():
    k = constants()
    assert {"S360_BLOCK", "S360_WAVE", "MF_C", "MF_T", "MF_WAVES", "MF_TM", "MF_KC", "MF_WT", "MF_MAX_CHUNKS", "REDUCE_BATCH"} <= set(k)
    assert k["MF_C"] == C and k["MF_WAVES"] == k["S360_BLOCK"] // k["S360_WAVE"] and k["MF_TM"] == k["MF_T"] * k["MF_WAVES"]
    assert k["MF_WT"] == k["S360_WAVE"]                         # the weight pass stages one token per lane
    lib = _lib.lib()
    for name in R.ROW_CASES:                                    # the chunk count is the library's own (host only)
        assert lib.s360_mono_fusion_weight_chunks(R.row_tokens(name)) == geometry(R.row_tokens(name))["chunks"], name
    for name, (tokens, _) in pooled_tokens().items():
        assert lib.s360_mono_fusion_weight_chunks(tokens) == geometry(tokens)["chunks"], name


def test_every_case_reaches_the_path_it_is_named_for():
    k = constants()
    wt, tm, t, batch = k["MF_WT"], k["MF_TM"], k["MF_T"], k["REDUCE_BATCH"]
    assert tuple(R.ROW_CASES) == POOLED_ROW_CASES + NEW_CASES
    geo = {name: geometry(R.row_tokens(name)) for name in R.ROW_CASES}
    # the pooled files' cases: the same shapes and kinds, the pooled file's seeds for "highest" and the "high" file's for "high"
    pooled_cases = _literal(TESTS / "test_gpu_mono_fusion.py", "CASES")
    seeds = {"highest": _literal(TESTS / "test_gpu_mono_fusion.py", "SEEDS"), "high": _literal(TESTS / "test_gpu_mono_fusion_high.py", "SEEDS")}
    for name in POOLED_ROW_CASES:
        assert R.ROW_CASES[name] == pooled_cases[name] and R.row_tokens(name) < R.UNITS_FROM + 16, name
        for precision in ("highest", "high"):
            assert R.row_seed(name, precision) == seeds[precision][name], (name, precision)
    # no pooled case has a chunk of three tiles, several reduce batches or more than two panoramas in a wave
    pooled = pooled_tokens()
    assert max(tokens for tokens, _ in pooled.values()) == 2304
    for name, (tokens, hw) in pooled.items():
        g = geometry(tokens)
        assert max(g["per_chunk"]) <= 2 and g["batches"][0] <= 1 and max(panoramas_per_wave(tokens, hw)) <= 2, name
    # every new case is decided (the pooled files' five are random, with the margin assertions of their files: `straddle`, 144
    # tokens, is the one of them that is judged in every quantity); the widths suit sample_grid_numpy
    for name, (n, geo_, cm, kind) in R.ROW_CASES.items():
        w = (R.GEOMETRIES[geo_] if isinstance(geo_, str) else geo_)[2]
        assert (kind == "decided") == (name in NEW_CASES) and w % 4 == 0 and cm % k["MF_KC"] == 0, name
        assert name not in NEW_CASES or R.row_tokens(name) >= R.UNITS_FROM, name
        assert R.row_names(R.row_tokens(name)) == (R.ROW_NAMES if name in NEW_CASES + ("straddle",) else R.TOKEN_ROWS), name
    # wg2: 132 tokens in panoramas of 12: three or four panoramas per wave; the second workgroup has four tokens, all in wave 0;
    # the weight pass has three tiles, one per chunk, the last of 4 tokens
    g, tokens = geo["wg2"], R.row_tokens("wg2")
    assert tokens == 132 and _hw(R.ROW_CASES["wg2"][1]) == 12 and panoramas_per_wave(tokens, 12) == {1, 3, 4}
    assert {len({tok // 12 for tok in range(w0, w0 + t)}) for w0 in range(0, tm, t)} == {3, 4}      # the four full waves of workgroup 0
    assert g["wg_tokens"] == [tm, 4] and 4 < t and g["chunk_tiles"] == [[wt], [wt], [4]]
    # mixed: 576 tokens in 4.5 workgroups, every gain in every wave; two stitched column groups, both channel gains in each
    g, tokens = geo["mixed"], R.row_tokens("mixed")
    assert tokens == 576 and g["wg_tokens"] == [tm] * 4 + [tm // 2] and t % len(R.MIXED_GAINS) == 0
    assert R.ROW_CASES["mixed"][2] == 2 * k["MF_KC"] and k["MF_KC"] % len(R.MIXED_CHANNEL_GAINS) == 0
    # tiles3: 68 tiles in 32 chunks of two and three tiles (the in-loop reload of the first register buffer runs, the second's
    # does not), the last tile of 32 tokens; 34 workgroups: two reduce batches and a tail of 2; the last has three valid waves
    g, tokens = geo["tiles3"], R.row_tokens("tiles3")
    assert tokens == 4320 and g["tiles"] == 68 and g["chunks"] == k["MF_MAX_CHUNKS"] == 32 and g["per_chunk"] == [2, 3]
    assert g["chunk_tiles"][-1][-1] == 32 and all(n == wt for c in g["chunk_tiles"] for n in c[:-1])
    assert g["wgs"] == 34 and g["batches"] == (2, 2) and batch == 16 and g["wg_tokens"][-1] == 3 * t
    # tiles5: the smallest N on g3 past 128 tiles: 131 tiles in chunks of four and five (reload, reload, odd tail); 66 workgroups:
    # four reduce batches and a tail of 2
    g, tokens = geo["tiles5"], R.row_tokens("tiles5")
    hw = _hw("g3")
    assert tokens == 8352 and g["tiles"] == 131 and g["per_chunk"] == [4, 5] and g["wgs"] == 66 and g["batches"] == (4, 2)
    assert R.ROW_CASES["tiles5"][0] == next(n for n in range(1, 64) if geometry(n * hw)["tiles"] > 4 * k["MF_MAX_CHUNKS"])
    assert g["chunk_tiles"][-1][-1] == 32 and 4 * k["MF_MAX_CHUNKS"] * wt == 8192 < tokens
    # chunks of three, four and five tiles are each reached by a named case, and five by tiles5 alone
    per_chunk = {name: set(geo[name]["per_chunk"]) for name in R.ROW_CASES}
    assert 3 in per_chunk["tiles3"] and 4 not in per_chunk["tiles3"] and {4, 5} <= per_chunk["tiles5"]
    assert [name for name in R.ROW_CASES if max(per_chunk[name]) >= 5] == ["tiles5"]
    assert [name for name in R.ROW_CASES if geo[name]["batches"][0] >= 2] == ["tiles3", "tiles5"]
    assert [name for name in R.ROW_CASES if max(panoramas_per_wave(R.row_tokens(name), _hw(R.ROW_CASES[name][1]))) >= 3] == ["wg2"]
    # the runs: every case at scales 1 and 6
    assert R.ROW_RUNS == [(name, scale) for name in R.ROW_CASES for scale in (1.0, 6.0)]
    # the factors are the project's, not restated
    assert (R.WORST_FACTOR, R.MEAN_FACTOR, R.UNITS_FLOOR, R.MEDIAN_CAP) == (FF.WORST_FACTOR, FF.MEAN_FACTOR, FF.UNITS_FLOOR, FF.MEDIAN_CAP)
    assert R.row_units is W.row_units and (R.UNIT, R.SCALE_FLOOR) == (W.UNIT, W.SCALE_FLOOR)


def test_the_inputs_are_the_cases_own_and_mixed_scales_g_and_the_mono_channels():
    tensors, g = R.row_inputs("mixed", 6.0)
    plain, g0 = R.decided_case(2, "g3", 128, scale=6.0, seed=R.row_seed("mixed"))
    assert all(torch.equal(a, b) for i, (a, b) in enumerate(zip(tensors, plain)) if i != 1)
    gains = torch.tensor([R.MIXED_GAINS[i % 4] for i in range(576)]).reshape(2, 1, 12, 24)
    assert torch.equal(g, g0 * gains) and g.shape == (2, C, 12, 24)
    cgains = torch.tensor([R.MIXED_CHANNEL_GAINS[i % 2] for i in range(128)]).reshape(1, 128, 1, 1)
    assert torch.equal(tensors[1], plain[1] * cgains) and R.MIXED_GAINS[3] == 1e-3 and R.MIXED_CHANNEL_GAINS[1] == 1e-3
    for precision in ("highest", "high"):
        tensors, g = R.row_inputs("straddle", 1.0, precision)
        plain, g0 = R.random_case(3, "g2", 192, scale=1.0, seed=R.row_seed("straddle", precision))
        assert all(torch.equal(a, b) for a, b in zip((*tensors, g), (*plain, g0)))
    tensors, g = R.row_inputs("wg2", 1.0)
    assert all(x.dtype == torch.float32 for x in (*tensors, g)) and g.shape == (11, C, 3, 4) and tensors[2].shape == (3, 4, 3)


@functools.lru_cache(maxsize=None)
def _run(name, scale, precision="highest"):
    tensors, g = R.row_inputs(name, scale, precision)
    want, sc = R.row_statement(tensors, g)
    return (tensors, g), want, sc, R.lines_rows(tensors, g), HR.three_rows(tensors, g) if precision == "high" else None


@pytest.mark.parametrize("name,scale", [("wave", 6.0), ("wg2", 1.0), ("mixed", 6.0), ("tiles3", 1.0)])
def test_row_statement_is_autograd_of_the_float64_statement(name, scale):
    (tensors, g), want, sc, _, _ = _run(name, scale)
    m = R.stitch32(tensors[1], tensors[2])
    ref = dict(zip(R.RESULTS, R.gradients(lambda *t: R.statement(*t, m=m), tensors, g, torch.float64)))
    erp, _, _, w1, lnw, lnb, w2 = (t.double() for t in tensors)
    x = torch.cat([erp, m.double()], dim=1).permute(0, 2, 3, 1).reshape(-1, w1.shape[1])
    ref["y"] = x @ w1.T
    tokens, k = x.shape
    assert set(want) == set(sc) == set(R.ROW_NAMES) and tokens == R.row_tokens(name)
    shapes = {"out": (tokens, C), "y": (tokens, C), "g_erp_feat": (tokens, C), "g_w1": (k, C), "g_w2": (C, C), "g_ln_weight": (C,), "g_ln_bias": (C,)}
    for n in R.ROW_NAMES:
        r = ref[n].permute(0, 2, 3, 1).reshape(-1, C) if n in ("out", "g_erp_feat") else ref[n].t() if n in R.COLUMN_ROWS else ref[n]
        assert want[n].dtype == sc[n].dtype == torch.float64 and tuple(want[n].shape) == shapes[n] == tuple(r.shape), n
        assert (want[n] - r).abs().max().item() <= 1e-12 * max(1.0, r.abs().max().item()), n
        assert sc[n].shape == r.shape[:1] and (sc[n] >= 0).all(), n
        mag = want[n].abs().amax(-1) if want[n].dim() == 2 else want[n].abs()
        assert (mag <= sc[n] * (1 + 1e-12)).all(), n                                # a correctly rounded result is within half a unit
    # g_w1 row k is input channel k of X and g_w2 row j is unit j of a, whatever the layouts of the tensors
    assert torch.equal(want["g_w1"], ref["g_w1"].t()) and torch.equal(want["g_w2"], ref["g_w2"].t())
    # the channel scales are the sums over tokens of the summed terms' magnitudes, and the sums of the terms are the gradients
    parts = {}
    xs = [t.detach().double().requires_grad_(True) if i in R.DIFFERENTIABLE else t for i, t in enumerate(tensors)]
    out = R.statement(*xs, parts=parts, m=m)
    parts["ln"].retain_grad()
    out.backward(g.double())
    g_ln = parts["ln"].grad.reshape(-1, C)
    y = ref["y"]
    x_hat = (y - y.mean(-1, keepdim=True)) / torch.sqrt(y.var(-1, unbiased=False, keepdim=True) + 1e-5)
    assert ((sc["g_ln_weight"] - (g_ln * x_hat).abs().sum(0)).abs() <= 1e-12 * sc["g_ln_weight"]).all()
    assert torch.equal(sc["g_ln_bias"], g_ln.abs().sum(0))
    assert (((g_ln * x_hat).sum(0) - want["g_ln_weight"]).abs() <= 1e-12 * sc["g_ln_weight"]).all()
    assert ((g_ln.sum(0) - want["g_ln_bias"]).abs() <= 1e-12 * sc["g_ln_bias"]).all()
    # a unit that is off at every token: scale 0 in its row of g_w2 and its two channels, and want exactly 0
    off = (parts["a"].reshape(-1, C) == 0).all(0)
    for n in ("g_w2", "g_ln_weight", "g_ln_bias"):
        assert torch.equal(sc[n] == 0, off) and (want[n][off] == 0).all(), n
    if name != "wave":
        assert 62 <= int(off.sum()) <= 71
    assert all((sc[n] > 0).all() for n in R.TOKEN_ROWS + ("g_w1",))


@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_the_float32_lines_alone_meet_the_rule_s_conditions(name, scale):
    """The yardstick against itself: its worst row is within 5 medians (token and column rows), every figure is finite, its rows
    of scale 0 are exactly 0, and nothing but the quantities judged at this T is looked at."""
    _, want, sc, lines, _ = _run(name, scale)
    for n in R.row_names(R.row_tokens(name)):
        failures, (kworst, kmean, yworst, ymean, ymedian) = R.rule_failures(n, lines[n], lines[n], want[n], sc[n])
        print(f"[mf64-cpu] {name}/x{scale:g} {n} worst {yworst:.3f} mean {ymean:.3f} median {ymedian:.3f} dead {int((sc[n] == 0).sum())}")
        assert not failures and kworst == yworst and 0 < ymedian <= ymean * 2 and yworst < 64, (n, failures)
        assert lines[n].dtype == torch.float32 and lines[n].shape == want[n].shape


@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_the_three_term_statement_alone_meets_the_rule_s_conditions(name, scale):
    """The second yardstick of the "high" rule, with the "high" seeds: the lines and the three-term statement each within 5 medians,
    finite figures, rows of scale 0 exactly 0; the three-term statement judged as a kernel at "high" holds its own rule."""
    _, want, sc, lines, three = _run(name, scale, "high")
    for n in R.row_names(R.row_tokens(name)):
        failures, fig = R.rule_failures(n, three[n].float(), lines[n], want[n], sc[n], three[n])
        print(f"[mf64-cpu] high {name}/x{scale:g} {n} three-term worst {fig[5]:.3f} mean {fig[6]:.3f} median {fig[7]:.3f} | lines worst "
              f"{fig[2]:.3f} mean {fig[3]:.3f} median {fig[4]:.3f}")
        assert not failures and all(v == v and v < 1024 for v in fig) and fig[7] > 0, (n, failures, fig)
        assert three[n].dtype == torch.float64 and three[n].shape == want[n].shape


def test_the_rule_s_arithmetic():
    """On made-up rows: the floors, the two factors, the median condition and its exemption, the dead row and its exclusion from
    the figures, a NaN, the "high" sum bound."""
    want = torch.full((8, 4), 0.375, dtype=torch.float64)                       # float32 steps of half a unit around it
    sc = torch.ones(8, dtype=torch.float64)
    off = lambda units: (want + units * R.UNIT * torch.eye(8, 4, dtype=torch.float64)[:, :1]).float()   # noqa: E731 (row 0 is off)
    every = lambda units: (want + units * R.UNIT).float()                          # noqa: E731
    exact = want.float()
    fails = lambda n, x, lines, three=None: [f[1] for f in R.rule_failures(n, x, lines, want, sc, three)[0]]     # noqa: E731
    assert fails("out", off(4), exact) == ["worst row"]                             # 4 units in one row: mean 0.5, the floor
    assert fails("out", off(3.5), exact) == ["worst row"] and fails("out", off(0.5), exact) == []
    assert fails("out", every(4), every(2)) == ["mean row"]                         # worst 4 <= 2 x 2, mean 4 > 1.5 x 2
    assert fails("out", every(2), every(2)) == [] and fails("out", every(3), every(2)) == []
    assert fails("out", every(5), every(2)) == ["worst row", "mean row"]
    assert fails("out", exact, off(8)) == ["yardstick not usable"]                  # the median is 0
    assert fails("g_ln_bias", exact, off(8)) == []                                  # the channels have no such condition
    # the "high" bound is on the sum of the two yardsticks, and the median condition is put on each
    three = lambda units: want + units * R.UNIT                                    # noqa: E731 (float64)
    assert fails("out", every(11), every(2), three(4)) == ["mean row"]              # worst 11 <= 2 x 6, mean 11 > 1.5 x 6
    assert fails("out", every(9), every(2), three(4)) == [] and fails("out", every(9), every(2)) == ["worst row", "mean row"]
    assert fails("out", every(13), every(2), three(4)) == ["worst row", "mean row"]
    assert fails("out", every(2), every(2), want + 8 * R.UNIT * torch.eye(8, 4, dtype=torch.float64)[:, :1]) == ["three-term yardstick not usable"]
    assert fails("out", every(2), off(8), three(4)) == ["yardstick not usable"]
    assert fails("g_ln_weight", every(2), off(8), three(4)) == []
    # dead rows: exactly 0 in all three, and left out of the figures (five of eight rows dead: with them the median would be 0)
    dead = sc.clone()
    dead[3:] = 0.0
    zero = torch.where(dead[:, None] == 0, 0.0, want)
    mask = (dead != 0)[:, None]
    x, lines = torch.where(mask, every(3), 0.0), torch.where(mask, every(2), 0.0)
    failures, fig = R.rule_failures("g_w2", x, lines, zero, dead)
    assert failures == [] and fig == (3.0, 3.0, 2.0, 2.0, 2.0)
    failures, fig = R.rule_failures("g_w2", x, lines, zero, dead, torch.where(mask, three(4), 0.0))
    assert failures == [] and fig == (3.0, 3.0, 2.0, 2.0, 2.0, 4.0, 4.0, 4.0)
    bad = x.clone()
    bad[5, 2] = 1e-30
    assert [f[1] for f in R.rule_failures("g_w2", bad, lines, zero, dead)[0]] == ["a row of scale 0 is not 0"]
    assert [f[1] for f in R.rule_failures("g_w2", x, bad, zero, dead)[0]] == ["a row of scale 0 is not 0 in the lines"]
    assert [f[1] for f in R.rule_failures("g_w2", x, lines, zero, dead, bad.double())[0]] == ["a row of scale 0 is not 0 in the three-term statement"]
    bad[5, 2] = float("nan")
    assert [f[1] for f in R.rule_failures("g_w2", bad, lines, zero, dead)[0]] == ["a row of scale 0 is not 0"]
    assert [f[1] for f in R.rule_failures("g_w2", x, lines, zero, torch.zeros_like(dead))[0]][-1] == "no row has a scale"
    # a NaN in a live row
    x = exact.clone()
    x[5, 1] = float("nan")
    assert fails("out", x, every(2)) == ["worst row", "mean row"] and fails("out", x, every(2), three(4)) == ["worst row", "mean row"]
    assert R.rule_failures("out", x, every(2), want, sc)[0][0][-1] == 5              # and the rule names the row


# ---- planted defects: the float64 results rounded to float32, one defect each, under both rules ---------------------------------

def _pooled_passes(x, lines, want, three=None):
    """The rule of tests/test_gpu_mono_fusion.py (_check_rule) for one tensor; with `three` that of
    tests/test_gpu_mono_fusion_high.py (window_attention_high_reference.check_rule)."""
    e, el = (x.double() - want).abs(), (lines.double() - want).abs()
    bmax, bmean = el.max().item(), el.mean().item()
    if three is not None:
        bmax, bmean = bmax + (three - want).abs().max().item(), bmean + (three - want).abs().mean().item()
    floor = 2.0 ** -24 * want.abs().max().item()
    return bool(torch.isfinite(x).all()) and e.max().item() <= max(1.5 * bmax, floor) and e.mean().item() <= max(1.5 * bmean, floor)


def _both_rules(n, x, run):
    _, want, sc, lines, three = run
    failures, fig = R.rule_failures(n, x, lines[n], want[n], sc[n], None if three is None else three[n])
    return _pooled_passes(x, lines[n], want[n], None if three is None else three[n]), failures, fig


def _quiet_token(sc):
    """A token of `mixed` with gain 1e-3, in the second workgroup."""
    row = 128 + 3 + 4 * 3
    assert row % 4 == 3 and R.MIXED_GAINS[3] == 1e-3 and row < sc["g_erp_feat"].shape[0]
    return row


@pytest.mark.parametrize("precision", ["highest", "high"])
@pytest.mark.parametrize("scale", R.ROW_SCALES)
def test_the_correctly_rounded_results_pass_both_rules(scale, precision):
    run = _run("mixed", scale, precision)
    for n in R.ROW_NAMES:
        pooled, failures, fig = _both_rules(n, run[1][n].float(), run)
        assert pooled and not failures and fig[0] <= 1.0, (n, failures, fig)       # half a float32 step is 0.5 to 1 unit of the value


def test_a_quiet_token_s_g_erp_feat_row_off_by_64_units_passes_the_pooled_rule_and_fails_per_row():
    run = _run("mixed", 1.0)
    _, want, sc, _, _ = run
    row = _quiet_token(sc)
    assert sc["g_erp_feat"][row] < 0.01 * sc["g_erp_feat"][row + 1]
    x = want["g_erp_feat"].clone()
    x[row] += 64 * R.UNIT * sc["g_erp_feat"][row]
    pooled, failures, fig = _both_rules("g_erp_feat", x.float(), run)
    print(f"planted 64 units in a quiet row of g_erp_feat: {fig[0]:.2f} units against the lines' {fig[2]:.2f}; pooled rule passes: {pooled}")
    assert pooled and [f[1] for f in failures] == ["worst row"] and failures[0][-1] == row and 60 < fig[0] < 68


def test_a_quiet_stitched_channel_s_g_w1_row_off_by_64_units_passes_the_pooled_rule_and_fails_per_row():
    """Stitched channel 65 (gain 1e-3, the second stitched column group): the column of g_w1 that only the re-gather in the
    weight pass feeds."""
    run = _run("mixed", 1.0)
    _, want, sc, _, _ = run
    row = C + 65
    assert R.MIXED_CHANNEL_GAINS[65 % 2] == 1e-3 and sc["g_w1"][row] < 0.01 * sc["g_w1"][row - 1] and sc["g_w1"][row] < 0.01 * sc["g_w1"][:C].min()
    x = want["g_w1"].clone()
    x[row] += 64 * R.UNIT * sc["g_w1"][row]
    pooled, failures, fig = _both_rules("g_w1", x.float(), run)
    print(f"planted 64 units in a quiet row of g_w1: {fig[0]:.2f} units against the lines' {fig[2]:.2f}; pooled rule passes: {pooled}")
    assert pooled and [f[1] for f in failures] == ["worst row"] and failures[0][-1] == row and 60 < fig[0] < 68


@pytest.mark.parametrize("precision", ["highest", "high"])
def test_a_g_w1_row_of_tiles5_missing_one_tile_fails_per_row(precision):
    """Row 40 of g_w1 (an erp_feat channel) without the contribution of the fourth tile of chunk 0 — what a reload that fetched
    nothing would leave.  One tile of 131 is an error of the order of a tenth of the row's magnitude, so the pooled maximum sees
    this one as well; what each rule says is asserted as it is."""
    run = _run("tiles5", 1.0, precision)
    (tensors, g), want, sc, _, _ = run
    m = R.stitch32(tensors[1], tensors[2])
    parts = {}
    xs = [t.detach().double().requires_grad_(True) if i in R.DIFFERENTIABLE else t for i, t in enumerate(tensors)]
    out = R.statement(*xs, parts=parts, m=m)
    parts["y"].retain_grad()
    out.backward(g.double())
    g_y = parts["y"].grad
    x_in = torch.cat([xs[0].detach(), m.double()], dim=1).permute(0, 2, 3, 1).reshape(g_y.shape[0], -1)
    k, wt = 40, constants()["MF_WT"]
    assert ((x_in[:, k] @ g_y - want["g_w1"][k]).abs() <= 1e-12 * sc["g_w1"][k]).all()          # the row is the sum over the tokens
    tile = slice(3 * wt, 4 * wt)
    assert len(geometry(R.row_tokens("tiles5"))["chunk_tiles"][0]) >= 4
    x = want["g_w1"].clone()
    x[k] -= x_in[tile, k] @ g_y[tile]
    pooled, failures, fig = _both_rules("g_w1", x.float(), run)
    print(f"planted missing tile in a row of g_w1 ({precision}): {fig[0]:.3g} units against the yardsticks' {fig[2]:.2f}; pooled rule passes: {pooled}")
    assert not pooled and [f[1] for f in failures] == ["worst row", "mean row"] and failures[0][-1] == k and fig[0] > 1e5


def test_a_row_of_y_left_at_nan_fails_per_row():
    """y is compared with nothing in the pooled files: both judge R.RESULTS, and y is not among them."""
    assert "y" not in R.RESULTS and set(R.RESULTS) == set(R.ROW_NAMES) - {"y"}
    assert "zip(R.RESULTS, want, lines, got)" in (TESTS / "test_gpu_mono_fusion.py").read_text()
    assert "R.RESULTS, want, three, lines, got)" in (TESTS / "test_gpu_mono_fusion_high.py").read_text()
    run = _run("mixed", 1.0)
    x = run[1]["y"].float()
    x[130] = float("nan")
    _, failures, _ = _both_rules("y", x, run)
    assert [f[1] for f in failures] == ["worst row", "mean row"] and failures[0][-1] == 130


def test_a_dead_g_w2_row_holding_1e_30_passes_the_pooled_rule_and_fails_per_row():
    run = _run("mixed", 1.0)
    _, want, sc, _, _ = run
    dead = torch.nonzero(sc["g_w2"] == 0).reshape(-1)
    assert 62 <= dead.numel() <= 71
    x = want["g_w2"].float()
    x[dead[7], 5] = 1e-30
    pooled, failures, fig = _both_rules("g_w2", x, run)
    assert pooled and [f[1] for f in failures] == ["a row of scale 0 is not 0"] and fig[0] <= 1.0
