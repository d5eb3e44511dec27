"""The fused transformer FFN tail (csrc/s360_transformer_ffn.hip) held to float64 PER ROW, past one workgroup and one tile.
tests/test_gpu_transformer_ffn.py pools each tensor into one maximum and one mean and stops at 120 tokens: one workgroup of the
forward and the token pass, one tile per weight chunk, no grid stride anywhere.  Here every token row (out, z, g_source, g_m),
every hidden unit's row of g_w1 and column of g_w2 and every channel of the LayerNorm parameter gradients is measured in units
of 2^-24 of its own scale (transformer_ffn_reference.row_statement), at the smallest T that reaches each path of the launch
geometry (R.ROW_CASES; tests/test_transformer_ffn_rows.py asserts that they do, from the kernel file's constants).

Three evaluations of the same float32 inputs on the same GPU: the kernels (through the C ABI, into NaN-filled buffers between
sentinels, the scratch between sentinels too, so every run also shows that the kernels write all they own and nothing else),
R.row_statement in float64 and R.lines_rows, the stock float32 lines (the yardstick).

Rule (R.rule_failures), per run and quantity, all rows counted, a row's error max_c |x - want| / max(scale, 2^-100) in units:

    kernel's worst row <= max(2 x yardstick's worst row, 0.5)        kernel's mean row <= max(1.5 x yardstick's mean row, 0.5)
    token and hidden-unit rows: yardstick's worst row <= 5 x its median row, else "yardstick not usable" (a failure)
    a row of scale 0 is exactly 0;  g_residual of the no_ffn tail is g_out bit for bit

Each test prints `[ff64] case/xscale quantity kernel/yardstick (worst) kernel/yardstick (mean) median <the yardstick's>` (pytest -s).

Measured on one MI355X (the 19 runs of R.ROW_RUNS and the 6 of R.NORM_RUNS, 178 figures; units of 2^-24 of the row's own scale,
kernel / float32 lines; "largest" is the largest kernel / bound of the quantity, with its run):

    quantity         worst row: kernel    lines              mean row: kernel    lines             largest, worst row            largest, mean row
    out              0.860 to 6.290       0.728 to 35.365    0.732 to 2.613      0.728 to 10.717   0.860 / 1.456 = 0.59 one/x6    0.860 / 1.092 = 0.79 one/x6
    z                2.181 to 7.882       3.936 to 52.752    2.181 to 3.561      3.936 to 14.865   4.770 / 13.750 = 0.35 tiny/x6  3.561 / 8.416 = 0.42 tiny/x6
    g_source         0.840 to 6.919       0.914 to 30.345    0.840 to 2.341      0.914 to 8.805    0.840 / 1.828 = 0.46 one/x6    0.840 / 1.371 = 0.61 one/x6
    g_m              3.356 to 15.559      6.333 to 44.670    3.356 to 4.529      5.889 to 14.284   9.769 / 24.762 = 0.39 wg2/x6   3.705 / 8.834 = 0.42 tiny/x1
    g_w1             5.721 to 45.912      14.613 to 125.974  2.839 to 20.665     6.659 to 52.108   19.753 / 41.584 = 0.48 wg2/x6  3.491 / 10.104 = 0.35 wg2/x6
    g_w2             5.871 to 43.531      16.714 to 144.516  2.692 to 21.179     7.074 to 51.298   7.758 / 35.390 = 0.22 wg3/x1   2.925 / 10.611 = 0.28 wg2/x1
    g_norm1_weight   0.049 to 2.957       0.183 to 4.789     0.015 to 0.780      0.055 to 1.269    2.957 / 7.898 = 0.37 mixed/x6  0.780 / 1.817 = 0.43 mixed/x6
    g_norm1_bias     0.054 to 2.290       0.154 to 3.646     0.015 to 0.581      0.043 to 1.077    1.700 / 5.304 = 0.32 wg2/x6    0.403 / 0.992 = 0.41 wg2/x6
    g_norm2_weight   0.066 to 2.238       0.213 to 5.646     0.014 to 0.559      0.058 to 1.409    0.755 / 2.302 = 0.33 tiles2/x1 0.357 / 1.030 = 0.35 wg2/x1
    g_norm2_bias     0.008 to 0.383       0.046 to 1.074     0.001 to 0.053      0.011 to 0.173    0.113 / 0.500 = 0.23 wg3/x1    0.053 / 0.500 = 0.11 mixed/x1
    no_ffn out       0.957 to 1.565       0.993 to 3.256     0.562 to 0.788      0.597 to 1.271    0.997 / 1.986 = 0.50 wg2/x6    0.593 / 0.939 = 0.63 wg2/x6
    no_ffn g_x       0.879 to 0.974       2.783 to 4.006     0.551 to 0.572      1.411 to 1.471    0.960 / 5.566 = 0.17 wg2/x6    0.572 / 2.136 = 0.27 rows/x1
    no_ffn g_weight  0.079 to 0.353       0.165 to 1.322     0.010 to 0.065      0.052 to 0.308    0.331 / 1.206 = 0.27 wg2/x1    0.065 / 0.500 = 0.13 mixed/x1
    no_ffn g_bias    0.068 to 0.383       0.108 to 1.074     0.007 to 0.053      0.036 to 0.173    0.383 / 2.148 = 0.18 mixed/x1  0.053 / 0.500 = 0.11 mixed/x1

(the largest figures of g_w1 and g_w2, kernel and lines, are `stride`: sums over 65 669 tokens.)  The yardstick's worst row over its median
row: 1.00 to 3.82 for token rows (the 3.82 is z of `stride`), 2.02 to 3.17 for hidden-unit rows, 2.97 to 8.14 for channels.  Found by this
file: nothing; every run passes with the kernels as they were, every buffer is fully written with its sentinels intact (the
scratch's too; its body is handed over as NaN, so a partial that is read without having been written would show in the rule), the
Python layer gives the ABI's bits, a second call gives identical bits, and workgroups 1 and 2 keep their bits when workgroup 0's
tokens change.  `stride` takes 0.3 s (statement, lines and kernels), the whole file 5 s.

Planted on scratch builds, arithmetic only (never an address or an index), the pooled file (48 tests) and this file (34) once each:
(a) in k_ff_backward_weights both ff_fold calls start from a zero tile instead of gw1[ct] / gw2[ct], so a chunk keeps its last
    tile only: the pooled file passes all 48; here test_every_row_against_float64 fails at tiles2, tiles3, rows (both scales) and
    stride, in g_w1 and g_w2 (worst rows 1.9e7 to 2.7e7 units);
(b) in k_ff_backward_tokens `double v = s_ln[i]` becomes `0.0`, so a workgroup keeps its last tile's LayerNorm sums only: the
    pooled file passes all 48; here stride fails in the four LayerNorm parameter gradients (g_norm1_weight 2.1e4 units against
    the lines' 0.18), and nothing else does;
(c) in k_ff_norm_residual_backward `pw[i] +=` / `pb[i] +=` become `=`: the pooled file passes all 48; here
    test_every_row_of_the_no_ffn_tail_against_float64 fails at rows (both scales) in g_weight (1.9e5 units) and g_bias (8.3e4).
What the pooled file holds and this one does not: the shapes below 129 tokens for the hidden-unit rows and the channels (at
T = 5 and scale 6 a hidden unit can have gelu ~ 0 on every token, and the float32 lines miss its g_w2 row by 1e4 units of its own
magnitude), the constant row, norm2 = 0, leading dimensions, memory, the seam.  The two files are kept side by side.
"""
import ctypes as C
import functools

import pytest
import torch

import transformer_ffn_reference as R
from splatter360_amd import _lib, transformer_ffn as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH, HIDDEN = 128, 1024
EPS = 1e-5
GUARD = 64                                                      # sentinel elements on either side: 256 B of floats, 512 B of doubles
_SENTINEL = 12345.678
FFN_SHAPES = {"g_source": None, "g_m": None, "g_w1": (HIDDEN, 2 * CH), "g_w2": (CH, HIDDEN), "g_norm1_weight": (CH,),
              "g_norm1_bias": (CH,), "g_norm2_weight": (CH,), "g_norm2_bias": (CH,)}      # None: [T, C]; the ABI's order
TOKEN_TENSORS = ("out", "z", "g_source", "g_m")


# ------------------------------------------------------------------------------------------------ the kernels through the C ABI
def _guarded(n, dtype=torch.float32):
    """n NaNs between two runs of GUARD sentinels; the body starts 16-byte aligned (256 or 512 bytes into the allocation)."""
    buf = torch.full((n + 2 * GUARD,), _SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf


def _assert_owned(buf, n, what, written=True):
    """Every owned element written (not the scratch: its contents are the kernels' own), both runs of sentinels intact."""
    if written:
        unwritten = int(torch.isnan(buf[GUARD:GUARD + n]).sum())
        assert unwritten == 0, (what, "elements not written", unwritten)
    s = torch.full((GUARD,), _SENTINEL, dtype=buf.dtype, device=buf.device)
    assert torch.equal(buf[:GUARD], s) and torch.equal(buf[GUARD + n:], s), (what, "a sentinel was overwritten")


def _buffers(shapes):
    bufs, raw = {}, {}
    for k, (shape, dtype) in shapes.items():
        numel = int(torch.Size(shape).numel())
        buf = _guarded(numel, dtype)
        bufs[k] = (buf, numel)
        raw[k] = buf[GUARD:GUARD + numel].view(shape)
    return bufs, raw


def _scratch(tokens):
    """The scratch of s360_ffn_tail_scratch_bytes(T) bytes as floats between sentinels."""
    need = int(_lib.lib().s360_ffn_tail_scratch_bytes(tokens))
    assert need > 0 and need % 16 == 0
    return _guarded(need // 4), need


def _p(x):
    return C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _abi(tensors, g):
    """One forward and one backward call of s360_ffn_tail_*.  Returns (raw, bufs): raw maps out, z, stats and the eight
    gradients to views into the guarded buffers in the kernels' layouts, bufs maps them and "scratch" to (buffer, owned elements)."""
    tokens = g.shape[0]
    assert all(t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in (*tensors, g)) and g.shape == (tokens, CH)
    shapes = {"out": ((tokens, CH), torch.float32), "z": ((tokens, CH), torch.float32), "stats": ((2, tokens, 2), torch.float64)}
    shapes.update({k: (s or (tokens, CH), torch.float32) for k, s in FFN_SHAPES.items()})
    bufs, raw = _buffers(shapes)
    scratch, need = _scratch(tokens)
    bufs["scratch"] = (scratch, need // 4)
    lib, eps = _lib.lib(), C.byref(C.c_double(EPS))
    _lib.check(lib.s360_ffn_tail_forward(*map(_p, tensors), tokens, CH, HIDDEN, eps, _p(raw["out"]), _p(raw["z"]), _p(raw["stats"]), _stream()),
               "forward")
    _lib.check(lib.s360_ffn_tail_backward(*map(_p, tensors), _p(raw["z"]), _p(raw["stats"]), _p(g), tokens, CH, HIDDEN, eps,
                                          _p(scratch[GUARD:]), need, *(_p(raw[k]) for k in FFN_SHAPES), _stream()), "backward")
    torch.cuda.synchronize()
    return raw, bufs


def _abi_norm(tensors, g):
    """The same for the no_ffn tail: out, stats, g_x, g_residual, g_weight, g_bias and the scratch."""
    x, weight, bias, residual = tensors
    tokens = g.shape[0]
    assert all(t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in (*tensors, g)) and g.shape == (tokens, CH)
    bufs, raw = _buffers({"out": ((tokens, CH), torch.float32), "stats": ((tokens, 2), torch.float64), "g_x": ((tokens, CH), torch.float32),
                          "g_residual": ((tokens, CH), torch.float32), "g_weight": ((CH,), torch.float32), "g_bias": ((CH,), torch.float32)})
    scratch, need = _scratch(tokens)
    bufs["scratch"] = (scratch, need // 4)
    lib = _lib.lib()
    _lib.check(lib.s360_layer_norm_residual_forward(_p(x), _p(weight), _p(bias), _p(residual), tokens, CH, C.byref(C.c_double(EPS)),
                                                    _p(raw["out"]), _p(raw["stats"]), _stream()), "forward")
    _lib.check(lib.s360_layer_norm_residual_backward(_p(x), _p(weight), _p(raw["stats"]), _p(g), tokens, CH, _p(scratch[GUARD:]), need,
                                                     _p(raw["g_x"]), _p(raw["g_residual"]), _p(raw["g_weight"]), _p(raw["g_bias"]), _stream()),
               "backward")
    torch.cuda.synchronize()
    return raw, bufs


def _evaluate(name, scale):
    tensors, g = R.row_inputs(name, scale, device=DEV)
    want, sc = R.row_statement(tensors, g, EPS)
    lines = R.lines_rows(tensors, g, EPS)
    raw, bufs = _abi(tensors, g)
    return (tensors, g), want, sc, lines, raw, bufs


@functools.lru_cache(maxsize=None)
def _cached(name, scale):
    """Inputs, row_statement, the float32 lines and the kernels' results of one run: computed once, shared, never modified."""
    assert name != "stride"
    return _evaluate(name, scale)


@pytest.fixture(scope="module")
def stride_run():
    """`stride` (T = 65 669) is evaluated once for the tests that use it and freed behind them: its float64 statement holds a few
    [T, 1024] float64 tensors of 0.5 GB while it runs, and its results are 34 MB a tensor."""
    run = [_evaluate("stride", 1.0)]
    yield run[0]
    run.clear()
    torch.cuda.empty_cache()


def _run(name, scale, request):
    return request.getfixturevalue("stride_run") if name == "stride" else _cached(name, scale)


@functools.lru_cache(maxsize=None)
def _run_norm(name, scale):
    tensors, g = R.norm_case(R.row_inputs(name, scale, device=DEV))
    want, sc = R.norm_row_statement(tensors, g, EPS)
    return (tensors, g), want, sc, R.norm_lines_rows(tensors, g, EPS), *_abi_norm(tensors, g)


def _check_rule(tag, names, got, want, sc, lines):
    failures = []
    for n in names:
        x = got[n]
        assert x.dtype == torch.float32 and x.shape == want[n].shape, (tag, n)
        fails, (kworst, kmean, yworst, ymean, ymedian) = R.rule_failures(n, x, lines[n], want[n], sc[n])
        print(f"[ff64] {tag} {n} {kworst:.3f}/{yworst:.3f} {kmean:.3f}/{ymean:.3f} median {ymedian:.3f}")
        failures += fails
    assert not failures, (tag, failures)


def _assert_all_owned(tag, bufs):
    for k, (buf, numel) in bufs.items():
        _assert_owned(buf, numel, (tag, k), written=k != "scratch")


# ------------------------------------------------------------------------------------------------ the rule and the ownership, run by run
@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_every_row_against_float64(name, scale, request):
    """Every run: the rule for every quantity judged at its T, every owned element written, every sentinel intact (out, z, stats,
    the eight gradients, and behind the scratch's bytes)."""
    _, want, sc, lines, raw, bufs = _run(name, scale, request)
    assert set(bufs) == {"out", "z", "stats", "scratch", *FFN_SHAPES}
    _assert_all_owned(f"{name}/x{scale:g}", bufs)
    _check_rule(f"{name}/x{scale:g}", R.row_names(R.ROW_CASES[name]), R.as_rows(raw), want, sc, lines)


@pytest.mark.parametrize("name,scale", R.NORM_RUNS)
def test_every_row_of_the_no_ffn_tail_against_float64(name, scale):
    (_, g), want, sc, lines, raw, bufs = _run_norm(name, scale)
    assert set(bufs) == {"out", "stats", "g_x", "g_residual", "g_weight", "g_bias", "scratch"}
    _assert_all_owned(f"norm {name}/x{scale:g}", bufs)
    _check_rule(f"norm {name}/x{scale:g}", R.NORM_ROW_NAMES[:-1], raw, want, sc, lines)
    assert torch.equal(raw["g_residual"], g)                                        # exact


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.mark.parametrize("name", ["tiles2", "rows"])
def test_the_python_layer_gives_the_c_abi_s_bits(name):
    (tensors, g), *_, raw, _ = _cached(name, 1.0)
    out, z, stats = tf.ffn_tail_forward(*tensors)
    assert torch.equal(out, raw["out"]) and torch.equal(z, raw["z"]) and torch.equal(stats, raw["stats"])
    xs = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = tf.ffn_tail(*xs)
    out.backward(g)
    assert torch.equal(out, raw["out"])
    for n, x in zip(tf.FFN_GRADIENTS, xs):
        assert torch.equal(x.grad, raw[n]), n
    (tensors, g), *_, raw, _ = _run_norm(name, 1.0)
    xs = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = tf.layer_norm_residual(*xs)
    out.backward(g)
    assert torch.equal(out, raw["out"])
    for n, x in zip(tf.NORM_GRADIENTS, xs):
        assert torch.equal(x.grad, raw[n]), n


# ------------------------------------------------------------------------------------------------ the saved statistics
@pytest.mark.parametrize("name", ["wg3", "tiles3", "stride"])
def test_the_saved_statistics_are_float64_s(name, request):
    """norm1's (mean, rstd) against float64 on m, norm2's against float64 over the kernel's own float32 z: the mean within 1e-12 of
    the largest element, rstd within 1e-12 of itself (the statement of tests/test_gpu_transformer_ffn.py, past one workgroup)."""
    (tensors, _), *_, raw, _ = _run(name, 1.0, request)
    stats = raw["stats"]
    assert stats.shape == (2, R.ROW_CASES[name], 2)
    for k, x in enumerate((tensors[1].double(), raw["z"].double())):
        mean = x.mean(dim=1)
        rstd = 1 / torch.sqrt(((x - mean[:, None]) ** 2).mean(dim=1) + EPS)
        assert (stats[k, :, 0] - mean).abs().max().item() <= 1e-12 * x.abs().max().item(), k
        assert ((stats[k, :, 1] - rstd) / rstd).abs().max().item() <= 1e-12, k


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["tiles2", "rows", "stride"])
def test_a_second_call_gives_identical_bits(name, request):
    (tensors, g), *_, raw, _ = _run(name, 1.0, request)
    again, bufs = _abi(tensors, g)
    _assert_all_owned(name, bufs)
    for k in raw:
        assert torch.equal(again[k], raw[k]), k
    if name != "stride":
        (tensors, g), *_, raw, _ = _run_norm(name, 1.0)
        again, _ = _abi_norm(tensors, g)
        for k in raw:
            assert torch.equal(again[k], raw[k]), k


# ------------------------------------------------------------------------------------------------ independence
def test_the_workgroups_do_not_see_each_other():
    """`wg3` once more with source, m and g of the tokens of workgroup 0 replaced: out, z, g_source and g_m of the tokens of
    workgroups 1 and 2 keep their bits (and those of workgroup 0 do not)."""
    (tensors, g), *_, raw, _ = _cached("wg3", 1.0)
    tm = 128
    other, g_other = R.random_case(tm, scale=2.0, seed=77, device=DEV)
    source, m, g2 = tensors[0].clone(), tensors[1].clone(), g.clone()
    source[:tm], m[:tm], g2[:tm] = other[0], other[1], g_other
    again, bufs = _abi((source, m, *tensors[2:]), g2)
    _assert_all_owned("wg3 with workgroup 0 replaced", bufs)
    for k in TOKEN_TENSORS:
        assert torch.equal(again[k][tm:], raw[k][tm:]), k
        assert not torch.equal(again[k][:tm], raw[k][:tm]), k
    assert torch.equal(again["stats"][:, tm:], raw["stats"][:, tm:])
