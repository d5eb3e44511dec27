"""The fused mono-feature fusion (csrc/s360_mono_fusion.hip) held to float64 PER ROW, in both precisions, past the shapes of the
pooled files.  tests/test_gpu_mono_fusion.py and tests/test_gpu_mono_fusion_high.py pool each tensor into one maximum and one mean,
compare y and stats with nothing and stop at 2 304 tokens: one or two tiles per chunk of the weight pass, one reduce batch, at most
two panoramas in a wave.  Here every token row (out, y, g_erp_feat), every input channel's row of g_w1 and every unit's row of g_w2
(both held transposed) and every channel of the LayerNorm parameter gradients is measured in units of 2^-24 of its own scale
(mono_fusion_reference.row_statement), at the smallest shapes that reach each path of the launch geometry (R.ROW_CASES;
tests/test_mono_fusion_rows.py asserts that they do, from the kernel file's constants).

Evaluations of the same float32 inputs on the same GPU: the kernels (through the C ABI, into NaN-filled buffers between sentinels,
the scratches between sentinels too and handed over as NaN, so every run also shows that the kernels write all they own and nothing
else, and a partial that is read without having been written would show in the rule), R.row_statement in float64, R.lines_rows, the
stock float32 lines, and for "high" mono_fusion_high_reference.three_rows, the specification's own rows.

Rule (R.rule_failures), per run and quantity, a row's error max_c |x - want| / max(scale, 2^-100) in units; the factors are the
project's (transformer_ffn_reference):

    a row of scale 0 (a unit that is off at every token: about half of the rows of g_w2 and of the channels of a decided case) is
      exactly 0 in the kernel's result, the lines' and the three-term statement's, and is left out of the figures below
    "highest":  kernel's worst row <= max(2 x lines' worst row, 0.5)      kernel's mean row <= max(1.5 x lines' mean row, 0.5)
    "high":     kernel's worst row <= max(2 x (worst e3 + worst e32), 0.5)  kernel's mean row <= max(1.5 x (mean e3 + mean e32), 0.5)
                e3 the per-row units of three_rows, e32 those of the lines: the pooled "high" rule row by row
    token and column rows: a yardstick's worst row <= 5 x its median row (e32, and e3 at "high"), else "not usable" (a failure)

Token rows are judged in every case, column rows and channels from 129 tokens on (the pooled files keep the small shapes for them).
The five random cases keep the margin assertions of their pooled files.  Each test prints `[mf64] precision case/xscale quantity
kernel/yardstick (worst) kernel/yardstick (mean) median <the yardstick's>` (pytest -s); at "high" the yardstick is e3 + e32.

Measured on one MI355X (the 18 runs of R.ROW_RUNS in each precision, 94 figures each; units of 2^-24 of the row's own scale, rows of
scale 0 left out; "yardstick" is the float32 lines at "highest" and e3 + e32 at "high"; "largest" is the largest kernel / bound of the
quantity, with its run):

    "highest"     worst row: kernel   yardstick          mean row: kernel   yardstick         largest, worst row               largest, mean row
    out           2.777 to 5.472      6.430 to 14.121    1.529 to 3.129     3.185 to 7.959    5.165 / 18.124 = 0.28 tile/x6     2.809 / 7.830 = 0.36 wave/x6
    y             3.619 to 10.242     9.894 to 21.311    2.636 to 3.263     6.381 to 11.284   10.242 / 33.822 = 0.30 tiles3/x6  3.263 / 9.796 = 0.33 wave/x1
    g_erp_feat    4.749 to 9.264      8.203 to 18.738    3.156 to 3.373     5.746 to 6.399    5.569 / 16.406 = 0.34 wave/x1     3.354 / 8.619 = 0.39 wg2/x6
    g_w1          6.690 to 9.930      11.243 to 84.375   3.591 to 3.876     5.669 to 36.749   9.435 / 24.108 = 0.39 straddle/x6 3.752 / 8.503 = 0.44 wg2/x6
    g_w2          3.971 to 5.903      6.387 to 92.812    2.744 to 3.294     4.170 to 41.284   5.221 / 12.774 = 0.41 wg2/x6      3.039 / 6.255 = 0.49 wg2/x1
    g_ln_weight   0.136 to 1.652      0.205 to 3.402     0.044 to 0.529     0.074 to 0.972    0.326 / 0.500 = 0.65 tiles3/x6    0.389 / 0.891 = 0.44 wg2/x1
    g_ln_bias     0.090 to 0.919      0.139 to 1.635     0.029 to 0.312     0.042 to 0.409    0.762 / 2.016 = 0.38 mixed/x1     0.257 / 0.500 = 0.51 wg2/x1
    "high"
    out           111.09 to 219.98    119.06 to 221.15   76.24 to 114.96    79.70 to 121.05   168.21 / 336.11 = 0.50 wide/x1    80.33 / 125.27 = 0.64 tiles3/x1
    y             103.11 to 174.40    114.77 to 189.68   72.05 to 79.41     78.36 to 88.27    113.95 / 243.78 = 0.47 wide/x1    78.53 / 127.33 = 0.62 wg2/x6
    g_erp_feat    157.67 to 260.33    164.96 to 281.51   110.31 to 116.88   116.47 to 122.81  213.29 / 440.57 = 0.48 mixed/x6   111.72 / 175.08 = 0.64 wide/x1
    g_w1          192.78 to 253.65    216.07 to 332.21   106.12 to 117.42   113.79 to 144.00  242.77 / 475.97 = 0.51 wg2/x1     110.49 / 173.18 = 0.64 wg2/x1
    g_w2          95.36 to 192.87     100.66 to 213.01   74.64 to 108.40    78.94 to 134.33   192.87 / 390.98 = 0.49 straddle/x1 105.40 / 167.06 = 0.63 straddle/x1
    g_ln_weight   4.342 to 58.774     4.509 to 63.815    1.272 to 17.037    1.350 to 18.146   5.892 / 12.168 = 0.48 tiles5/x6   13.168 / 20.543 = 0.64 wg2/x1
    g_ln_bias     2.583 to 30.307     2.793 to 31.535    0.691 to 9.857     0.734 to 10.311   3.666 / 7.536 = 0.49 tiles3/x1    9.857 / 15.466 = 0.64 straddle/x1

(the lines' largest figures of g_w1 and g_w2 are tiles3 and tiles5: rocBLAS's float32 sums over 4 320 and 8 352 tokens, where the
kernels add their tiles in float64 and stay at 7 to 9 units.)  The lines' worst row over their median row: 1.40 to 3.29 for token
rows, 1.53 to 2.87 for column rows, 2.63 to 4.85 for channels; the three-term statement's (CPU figures of
tests/test_mono_fusion_rows.py, the same tensors): 1.2 to 2.5.  62 to 71 of the 128 rows of g_w2, g_ln_weight and g_ln_bias of a
decided case have scale 0 and are exactly 0 in the kernels' results in both precisions.

"high", the distance from its own specification (test_high_sits_on_its_specification_row_by_row; |kernel - three_rows| per row, its
worst row over the lines' worst row, the range over the 18 runs): y 0.42 to 1.66, g_ln_weight 0.40 to 0.81, g_ln_bias 0.60 to 1.04,
g_w1 0.34 to 5.66, g_w2 0.07 to 6.09, out 3.64 to 9.51, g_erp_feat 3.39 to 10.11 (mixed/x6: 123.2 units against the lines' 12.2; tiles3/x1: 136.3 against 13.5; the
mean row of out is 2.9 to 24.2 units, of g_erp_feat 9.7 to 14.7).  1.5 x 10.11 asks for a factor of 16, above 8, so NOTHING IS
ASSERTED of this distance: row by row the kernels do not "sit on the specification" to a float32-accumulation distance in every
quantity.  The quantities that do (ratios up to 1.7) are those whose operands are the call's inputs (y = X W1^T) or float64 sums;
those that do not have an operand that is PRODUCED and then split: a (out, g_w2) and g_y (g_erp_feat, g_w1).  The specification is
not continuous there: hi = bf16(x) and lo = bf16(x - hi) keep 16 bits, and a change of x by one float32 rounding can move what the
split drops by 2^-17 |x|, the size of e3 itself.  On the CPU, rounding the three-term y to float32 (half a unit per element, what
the kernel's float32 accumulator does) moves the three-term out by 34 to 84 units in its worst row (mean 0.6 to 3.2), and by 1.0 to
1.3 units through an exact product.  So the distance is a property of bf16x3 on produced operands, not a defect of these kernels;
the pooled figure "kernel / e3 is 1 to within 8 %" compares two distances from float64 and does not say otherwise.

Found by this file: nothing wrong in the kernels.  Every run passes with the kernels as they were, every buffer is fully written
with its sentinels intact (the scratches' too), dead rows are exact zeros, the saved statistics are float64's, the Python layer
gives the ABI's bits, a second call gives identical bits, and the other workgroups keep their bits when workgroup 0's tokens
change.  One run of `tiles5` (inputs, float64 statement, lines, three-term rows and the kernels) takes 0.03 s, the whole file 5 s
(70 tests; 2 s of it is the first call's start-up).

Planted on scratch builds, arithmetic only (never an address, an index or a loop bound), the two pooled files (61 tests) and this
file (70) once each:
(a) in k_mfh_backward_weights the register values xs, gs of the tile fetched by the in-loop reload of `ta` are zeroed: both pooled
    files pass all 61; here test_every_row_against_float64 fails at "high" in tiles3 and tiles5 (both scales), in g_w1 and g_w2,
    worst and mean row (worst rows 3.8e6 to 1.6e7 units against e3 + e32 of 190 to 330), and nothing else does;
(b) the same for the reload of `tb`: both pooled files pass all 61; here "high" tiles5 (both scales) fails in g_w1 and g_w2
    (8.5e6 and 2.1e7 units), and tiles3, which has no chunk of four tiles, passes;
(c) k_mf_forward stores y scaled by 1 + 2^-12 while its LayerNorm uses the unscaled value: here every "highest" run fails in y at
    4 096 units in the mean row (the plant itself), the saved statistics fail at wg2, tiles3 and tiles5, and the gradients that read y
    back fail with it (x_hat is formed from the stored y and the statistics of the unscaled one: g_erp_feat 3 100 units at wave,
    g_w1 1 000, g_w2 350 and g_ln_weight 160 at tiles5; g_ln_bias, which does not read y, stays at 0.09).  The pooled "highest" file
    sees this one too, through the gradients alone (21 of its tests fail, out passes everywhere): a defect of y of this size is
    not hidden from it, only y itself is.  "high" is untouched by (c) and passes in all three files.
What the pooled files hold and this one does not: the shapes below 129 tokens for the column rows and the channels, the zero
panorama, dead units through ln_weight = 0, the guards around the inputs, the clipped pixels, memory, the scratch refusals, side
streams, the seam.  The files are kept side by side.
"""
import ctypes as C
import functools
import time

import pytest
import torch

import mono_fusion_high_reference as HR
import mono_fusion_reference as R
from splatter360_amd import _lib, mono_fusion as mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = 128
EPS = 1e-5
GUARD = 64                                                      # sentinel elements on either side: 256 B of floats, 512 B of doubles
_SENTINEL = 12345.678
PRECISIONS = ("highest", "high")
GRADIENTS = ("g_erp_feat", "g_w1", "g_ln_weight", "g_ln_bias", "g_w2")          # the ABI's order


# ------------------------------------------------------------------------------------------------ the kernels through the C ABI
def _guarded(n, dtype=torch.float32):
    """n NaNs between two runs of GUARD sentinels; the body starts 16-byte aligned (256 or 512 bytes into the allocation)."""
    buf = torch.full((n + 2 * GUARD,), _SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf


def _assert_owned(buf, n, what, written=True):
    """Every owned element written (not the scratches: their contents are the kernels' own), both runs of sentinels intact."""
    if written:
        unwritten = int(torch.isnan(buf[GUARD:GUARD + n]).sum())
        assert unwritten == 0, (what, "elements not written", unwritten)
    s = torch.full((GUARD,), _SENTINEL, dtype=buf.dtype, device=buf.device)
    assert torch.equal(buf[:GUARD], s) and torch.equal(buf[GUARD + n:], s), (what, "a sentinel was overwritten")


def _assert_all_owned(tag, bufs):
    for k, (buf, numel) in bufs.items():
        _assert_owned(buf, numel, (tag, k), written=not k.startswith("scratch"))


def _p(x):
    return C.c_void_p(x.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _abi(tensors, g, precision):
    """One forward and one backward call of s360_mono_fusion_* ("high": s360_mono_fusion_high_*).  Returns (raw, bufs): raw maps
    out, y, stats and the five gradients to views into the guarded buffers in the kernels' layouts, bufs maps them and the
    scratches to (buffer, owned elements)."""
    n, c, h, w = tensors[0].shape
    cm, fw = tensors[1].shape[1], tensors[1].shape[2]
    tokens = n * h * w
    assert c == CH and all(t.is_contiguous() and t.dtype == torch.float32 and t.data_ptr() % 16 == 0 for t in (*tensors, g)) and g.shape == tensors[0].shape
    shapes = {"out": ((n, c, h, w), torch.float32), "y": ((tokens, c), torch.float32), "stats": ((tokens, 2), torch.float64),
              "g_erp_feat": ((n, c, h, w), torch.float32), "g_w1": ((c, c + cm), torch.float32), "g_ln_weight": ((c,), torch.float32),
              "g_ln_bias": ((c,), torch.float32), "g_w2": ((c, c), torch.float32)}
    bufs, raw = {}, {}
    for k, (shape, dtype) in shapes.items():
        numel = int(torch.Size(shape).numel())
        bufs[k] = (_guarded(numel, dtype), numel)
        raw[k] = bufs[k][0][GUARD:GUARD + numel].view(shape)
    lib, eps, high = _lib.lib(), C.byref(C.c_double(EPS)), precision == "high"
    need = int(lib.s360_mono_fusion_high_scratch_bytes(tokens, cm, 1) if high else lib.s360_mono_fusion_scratch_bytes(tokens, cm))
    assert need > 0 and need % 16 == 0 and need == mf.scratch_bytes(tokens, cm, True, precision)
    bufs["scratch"] = (_guarded(need // 4), need // 4)
    ins = [_p(t) for t in tensors]
    sizes = (n, c, cm, fw, h, w, eps)
    if high:
        fneed = int(lib.s360_mono_fusion_high_scratch_bytes(tokens, cm, 0))
        assert 0 < fneed < need and fneed % 16 == 0
        bufs["scratch_forward"] = (_guarded(fneed // 4), fneed // 4)
        _lib.check(lib.s360_mono_fusion_high_forward(*ins, *sizes, _p(raw["out"]), _p(raw["y"]), _p(raw["stats"]),
                                                     _p(bufs["scratch_forward"][0][GUARD:]), fneed, _stream()), "forward")
    else:
        _lib.check(lib.s360_mono_fusion_forward(*ins, *sizes, _p(raw["out"]), _p(raw["y"]), _p(raw["stats"]), _stream()), "forward")
    backward = lib.s360_mono_fusion_high_backward if high else lib.s360_mono_fusion_backward
    _lib.check(backward(*ins, _p(raw["y"]), _p(raw["stats"]), _p(g), *sizes, _p(bufs["scratch"][0][GUARD:]), need,
                        *(_p(raw[k]) for k in GRADIENTS), _stream()), "backward")
    torch.cuda.synchronize()
    return raw, bufs


@functools.lru_cache(maxsize=None)
def _run(precision, name, scale):
    """Inputs, row_statement, the float32 lines, the three-term rows ("high") and the kernels' results of one run: computed once,
    shared, never modified.  `tiles5` holds 4 MB a tensor: nothing here needs freeing."""
    t0 = time.perf_counter()
    assert torch.get_float32_matmul_precision() == "highest"
    tensors, g = R.row_inputs(name, scale, precision, device=DEV)
    want, sc = R.row_statement(tensors, g, EPS)
    lines = R.lines_rows(tensors, g, EPS)
    three = HR.three_rows(tensors, g, EPS) if precision == "high" else None
    raw, bufs = _abi(tensors, g, precision)
    print(f"[mf64] {precision} {name}/x{scale:g} evaluated in {time.perf_counter() - t0:.2f} s")
    return (tensors, g), want, sc, lines, three, raw, bufs


def _rows(raw):
    return R.as_rows({n: raw[n] for n in R.ROW_NAMES})


# ------------------------------------------------------------------------------------------------ the rule and the ownership, run by run
@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_row_against_float64(precision, name, scale):
    """Every run: every owned element written and every sentinel intact (out, y, stats, the five gradients, and around the
    scratches' bytes), a row of scale 0 exactly 0, the rule for every quantity judged at its T."""
    (tensors, _), want, sc, lines, three, raw, bufs = _run(precision, name, scale)
    tag = f"{precision} {name}/x{scale:g}"
    if R.ROW_CASES[name][3] != "decided":                      # the margin assertions of the pooled files, unchanged
        cpu = tuple(t.cpu() for t in tensors)
        m = R.stitch32(cpu[1], cpu[2])
        if precision == "high":
            assert HR.ln_margin_abs(cpu, m) >= 8.0 * HR.ln_deviation(cpu, m) and HR.flipped_decisions(cpu, m) == 0, tag
        else:
            assert R.ln_margin(cpu, m=m) >= 2.0 ** -17, tag
    assert set(bufs) == {"out", "y", "stats", "scratch", *GRADIENTS} | ({"scratch_forward"} if precision == "high" else set())
    _assert_all_owned(tag, bufs)
    got, failures = _rows(raw), []
    for n in R.row_names(R.row_tokens(name)):
        x = got[n]
        assert x.dtype == torch.float32 and x.shape == want[n].shape, (tag, n)
        fails, fig = R.rule_failures(n, x, lines[n], want[n], sc[n], None if three is None else three[n])
        yworst, ymean = (fig[2], fig[3]) if three is None else (fig[2] + fig[5], fig[3] + fig[6])
        median = f"{fig[4]:.3f}" if three is None else f"{fig[4]:.3f} (e32) {fig[7]:.3f} (e3)"
        print(f"[mf64] {tag} {n} {fig[0]:.3f}/{yworst:.3f} {fig[1]:.3f}/{ymean:.3f} median {median}")
        failures += fails
    assert not failures, (tag, failures)


# ------------------------------------------------------------------------------------------------ "high": the distance from its own specification
@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_high_sits_on_its_specification_row_by_row(name, scale):
    """Per row |kernel - three_rows| in the row's units, against the lines' worst row.  Printed as `[mf64-spec] case/xscale
    quantity distance (worst, mean) lines (worst, mean) ratio of the worst rows`.  NOT asserted as a bound: the largest measured
    ratio is 10.1 (the docstring of this file), the factor would be 16, and a factor above 8 is not a bound on "sitting on the
    specification".  What is asserted is that every distance is a finite number."""
    _, want, sc, lines, three, raw, _ = _run("high", name, scale)
    got = _rows(raw)
    for n in R.row_names(R.row_tokens(name)):
        live = sc[n] != 0
        d = R.row_units(got[n], three[n], sc[n])[live]
        e32 = R.row_units(lines[n], want[n], sc[n])[live]
        ratio = d.max().item() / e32.max().item()
        print(f"[mf64-spec] {name}/x{scale:g} {n} {d.max().item():.3f} {d.mean().item():.3f} lines {e32.max().item():.3f} {e32.mean().item():.3f} ratio {ratio:.3f}")
        assert bool(torch.isfinite(d).all()) and d.numel() > 0, (name, scale, n)


# ------------------------------------------------------------------------------------------------ the saved statistics
@pytest.mark.parametrize("name", ["wg2", "tiles3", "tiles5"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_saved_statistics_are_float64_s(precision, name):
    """(mean, rstd) against float64 over the kernel's own float32 y: the mean within 1e-12 of the largest element, rstd within
    1e-12 of itself (the kernels form both in float64)."""
    raw = _run(precision, name, 1.0)[5]
    stats, y = raw["stats"], raw["y"].double()
    assert stats.shape == (R.row_tokens(name), 2) and stats.dtype == torch.float64
    mean = y.mean(dim=1)
    rstd = 1 / torch.sqrt(((y - mean[:, None]) ** 2).mean(dim=1) + EPS)
    assert (stats[:, 0] - mean).abs().max().item() <= 1e-12 * y.abs().max().item()
    assert ((stats[:, 1] - rstd) / rstd).abs().max().item() <= 1e-12


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.mark.parametrize("name", ["mixed", "tiles3"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_python_layer_gives_the_c_abi_s_bits(precision, name):
    (tensors, g), *_, raw, _ = _run(precision, name, 1.0)
    out, y, stats = mf.mono_fusion_forward(*tensors, EPS, precision=precision)
    assert torch.equal(out, raw["out"]) and torch.equal(y, raw["y"]) and torch.equal(stats, raw["stats"])
    grads = mf.mono_fusion_backward(*tensors, y, stats, g, EPS, precision=precision)
    assert mf.GRADIENTS == GRADIENTS
    for n, x in zip(GRADIENTS, grads):
        assert torch.equal(x, raw[n]), n
    xs = [t.detach().clone() for t in tensors]
    for i in R.DIFFERENTIABLE:
        xs[i].requires_grad_(True)
    out = mf.mono_fusion(*xs, eps=EPS, precision=precision)
    out.backward(g)
    assert torch.equal(out, raw["out"])
    for n, i in zip(GRADIENTS, R.DIFFERENTIABLE):
        assert torch.equal(xs[i].grad, raw[n]), n


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("name", ["tiles3", "tiles5"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_second_call_gives_identical_bits(precision, name):
    (tensors, g), *_, raw, _ = _run(precision, name, 1.0)
    again, bufs = _abi(tensors, g, precision)
    _assert_all_owned((precision, name), bufs)
    for k in raw:
        assert torch.equal(again[k], raw[k]), k


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_workgroups_do_not_see_each_other(precision):
    """`mixed` once more with erp_feat and g replaced at the 128 tokens of workgroup 0: out, y, stats and g_erp_feat of every
    other token keep their bits (and those of workgroup 0 do not)."""
    (tensors, g), *_, raw, _ = _run(precision, "mixed", 1.0)
    tm = 128
    n, c, h, w = tensors[0].shape
    assert h * w > tm                                           # workgroup 0's tokens are the first 128 pixels of panorama 0
    gen = torch.Generator().manual_seed(77)
    erp, g2 = tensors[0].clone(), g.clone()
    erp.view(n, c, h * w)[0, :, :tm] = (2.0 * torch.randn(c, tm, generator=gen)).to(DEV)
    g2.view(n, c, h * w)[0, :, :tm] = torch.randn(c, tm, generator=gen).to(DEV)
    again, bufs = _abi((erp, *tensors[1:]), g2, precision)
    _assert_all_owned((precision, "mixed with workgroup 0 replaced"), bufs)
    first, second = _rows(raw), _rows(again)
    for k in R.TOKEN_ROWS:
        assert torch.equal(second[k][tm:], first[k][tm:]), k
        assert not torch.equal(second[k][:tm], first[k][:tm]), k
    assert torch.equal(again["stats"][tm:], raw["stats"][tm:]) and not torch.equal(again["stats"][:tm], raw["stats"][:tm])
