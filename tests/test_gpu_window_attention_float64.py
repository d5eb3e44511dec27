"""The fused window attention (csrc/s360_window_attention.hip) held to float64 PER ROW, at C = 32, 64 and 96 and at the edges of
its block decomposition.  tests/test_gpu_window_attention.py pools each tensor into one maximum and one mean and runs C = 32 and
128 only; here every query row and every key row is measured against its own scale, all four channel maps run, and lse and Delta
are compared too.

Three evaluations of the same float32 inputs on the same GPU: the kernels (through the C ABI, into NaN-filled buffers between
sentinels, so every case also shows what the kernels write), window_attention_reference.row_scales in float64 (the statement's
values and each row's scale) and window_attention_reference.lines_rows, the reference's lines in float32 (the yardstick).

Rule, for every case and each of out, g_q, g_k, g_v, lse, delta, with a row's error max_c |x - want| / max(scale, 2^-100) in
units of 2^-24 (no row is left out; a row of scale 0 must be exactly 0):

    kernel's worst row <= max(2 x yardstick's worst row, 0.5) units,    yardstick's worst row <= 4 units, else "not usable"

The 2 is the project's (test_gpu_adapter_float64.py, test_gpu_lazy_seam.py: another order of operations, a few-ulp expf); the
0.5 is the final rounding of a correctly rounded result, |want| <= scale.  tests/test_window_attention_rows.py pins the measure
on the CPU.  Each test prints `[wa64] case quantity kernel/yardstick` (pytest -s).

Measured on one MI355X (53 runs, two full-attention runs and the structure cases, 6 quantities each; worst row in units of 2^-24, kernel / float32 lines):

    quantity   kernel            lines             largest kernel / bound          the case of the largest ratio
    out        0.015 to 1.593    0.047 to 1.590    0.387 / 0.500 = 0.77            m11/shift=0/x1/reference
    g_q        0.019 to 0.409    0.030 to 1.070    0.269 / 0.520 = 0.52            m5/shift=1/x1/reference
    g_k        0.133 to 2.226    0.149 to 2.522    2.226 / 3.482 = 0.64            m5/shift=1/x6/reference
    g_v        0.225 to 1.122    0.269 to 2.554    0.482 / 0.668 = 0.72            c64/shift=1/x1/reference
    lse        0.000 to 0.953    0.534 to 2.979    0.644 / 1.068 = 0.60            c64/shift=1/x3/reference
    delta      0.007 to 0.322    0.017 to 0.802    0.322 / 0.538 = 0.60            m5/shift=1/x6/reference

Found by this file: at C = 32 and more than one key tile per window (cases "edge" and "m5") g_q was wrong in channels 27 and 31
of every row, by 1e4 to 4e5 units and differently from run to run; every other quantity passed.  k_wa_backward_q<1, true> read
its accumulator tile back 7 wait states after the last MFMA of the previous key tile; fixed in the kernel (its comment).

Planted on scratch builds: `NCB * l31` replaced by `4 * l31` in a wa_load_c of k_wa_backward_kv reads past the row, at the last
row past the tensor, and the first case (c64) ended in an illegal memory access: every test of this file fails from there on;
it was not run a second time and not against the pooled file (which has no C < 128 case with more than 32 channels to read
past).  The two mask rules swapped in wa_key fails 18 tests here (6 of the pooled file's); lse narrowed to
float before the subtraction in k_wa_backward_kv does NOT fail this file: an error of 2^-25 |lse| in the exponent is inside
what the scale's (1 + a + A) factor grants a float32 score (|lse| <~ a + A at every case here), while the pooled file, which
compares with the lines' actual error, fails 7 tests with it.  The two files are kept side by side for that reason.
"""
import ctypes as C
import functools

import pytest
import torch

import window_attention_reference as R
from splatter360_amd import _lib, window_attention as wa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.ROW_CASES
YARDSTICK_LIMIT = 4.0
GUARD = 64                                                      # sentinel elements on either side: 256 B of floats, 512 B of doubles
_SENTINEL = 12345.678

RUNS = [(name, shift, scale, "reference") for name in CASES for shift in (False, True) for scale in (1.0, 3.0, 6.0)]
RUNS += [("m11", True, scale, "aligned") for scale in (1.0, 3.0, 6.0)]
RUNS += [(name, True, 7.7, "reference") for name in ("c64", "c96")]                  # the finite -100 decides rows


# ------------------------------------------------------------------------------------------------ the kernels through the C ABI
def _guarded(n, dtype):
    """n NaNs between two runs of GUARD sentinels; the body starts 16-byte aligned (256 or 512 bytes into the allocation)."""
    buf = torch.full((n + 2 * GUARD,), _SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf


def _assert_owned(buf, n, what):
    b = buf.cpu()
    unwritten = int(torch.isnan(b[GUARD:GUARD + n]).sum())
    assert unwritten == 0, (what, "elements not written", unwritten)
    s = torch.full((GUARD,), _SENTINEL, dtype=buf.dtype)
    assert torch.equal(b[:GUARD], s) and torch.equal(b[GUARD + n:], s), (what, "a sentinel was overwritten")


def _abi(q, k, v, g, h, w, ksp, shift, rule="reference", needs=(True, True, True)):
    """One forward and one backward call of the C ABI.  Returns (got, bufs): got maps R.ROW_NAMES to views into the guarded
    buffers (None for a gradient that `needs` leaves out: a null pointer), bufs maps them to (buffer, owned elements)."""
    b, l, c = q.shape
    partners = k.shape[1] if k.dim() == 4 else 0
    shapes = dict(out=q.shape, g_q=q.shape, g_k=k.shape, g_v=k.shape, lse=(b, l), delta=(b, l))
    want = dict(out=True, g_q=needs[0], g_k=needs[1], g_v=needs[2], lse=True, delta=True)
    bufs, got = {}, {}
    for n in R.ROW_NAMES:
        if not want[n]:
            got[n] = None
            continue
        numel = int(torch.Size(shapes[n]).numel())
        buf = _guarded(numel, torch.float64 if n in ("lse", "delta") else torch.float32)
        bufs[n] = (buf, numel)
        got[n] = buf[GUARD:GUARD + numel].view(shapes[n])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    dims = (b, partners, h, w, c, ksp, int(shift), wa.MASK_RULES[rule])
    lib = _lib.lib()
    _lib.check(lib.s360_window_attention_forward(p(q), p(k), p(v), *dims, p(got["out"]), p(got["lse"]), stream), "forward")
    _lib.check(lib.s360_window_attention_backward(p(q), p(k), p(v), p(got["lse"]), p(g), *dims, p(got["delta"]), p(got["g_q"]),
                                                  p(got["g_k"]), p(got["g_v"]), stream), "backward")
    torch.cuda.synchronize()
    return got, bufs


def _python(q, k, v, g, h, w, ksp, shift, rule="reference", needs=(True, True, True)):
    q, k, v = (t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), needs))
    out = wa.window_attention(q, k, v, height=h, width=w, num_splits=ksp, with_shift=shift, mask_rule=rule)
    out.backward(g)
    return out.detach(), q.grad, k.grad, v.grad


def _evaluate(q, k, v, g, h, w, ksp, shift, rule="reference"):
    want, scale = R.row_scales(q, k, v, g, ksp, shift, h, w, rule)
    lines = R.lines_rows(q, k, v, g, ksp, shift, h, w, rule)
    got, bufs = _abi(q, k, v, g, h, w, ksp, shift, rule)
    return want, scale, lines, got, bufs


@functools.lru_cache(maxsize=None)
def _run(name, shift, scale, rule="reference"):
    """Inputs, row_scales, the float32 lines and the kernels' results of one case: computed once, shared, never modified."""
    b, m, h, w, ksp, c = CASES[name]
    seed = 3000 + 7 * sorted(CASES).index(name) + int(shift)
    inputs = R.random_case(b, m, h, w, c=c, scale=scale, seed=seed, device=DEV)
    return (inputs, *_evaluate(*inputs, h, w, ksp, shift, rule))


def _check_rule(tag, got, want, scale, lines, names=R.ROW_NAMES):
    failures = []
    for n in names:
        x = got[n]
        assert x.dtype == (torch.float64 if n in ("lse", "delta") else torch.float32) and x.shape == want[n].shape, (tag, n)
        kern = R.row_units(x, want[n], scale[n]).max().item()
        yard = R.row_units(lines[n], want[n], scale[n]).max().item()
        print(f"[wa64] {tag} {n} {kern:.3f}/{yard:.3f}")
        dead = scale[n] == 0                                    # nothing reaches these rows: exactly 0, not merely small
        if bool(dead.any()) and bool((x[dead] != 0).any()):
            failures.append((n, "a row of scale 0 is not 0", int((x[dead] != 0).sum())))
        if not yard <= YARDSTICK_LIMIT:
            failures.append((n, "yardstick not usable", yard))
        elif not kern <= max(2.0 * yard, 0.5):
            worst = R.row_units(x, want[n], scale[n]).reshape(-1).argmax().item()
            failures.append((n, kern, yard, "worst row", worst))
    assert not failures, (tag, failures)


# ------------------------------------------------------------------------------------------------ the rule, case by case
@pytest.mark.parametrize("name,shift,scale,rule", RUNS)
def test_every_row_against_float64(name, shift, scale, rule):
    _, want, sc, lines, got, _ = _run(name, shift, scale, rule)
    _check_rule(f"{name}/shift={int(shift)}/x{scale:g}/{rule}", got, want, sc, lines)


@pytest.mark.parametrize("name", ["c64", "c96"])
def test_the_finite_mask_decides_rows_at_scale_7_7(name):
    """q, k randn x 7.7: rows exist whose unmasked scores all lie more than 100 below a masked key's.  The case tells the finite
    -100 from -inf (the rule itself is asserted by test_every_row_against_float64 on this very run)."""
    (q, k, v, g), want, *_ = _run(name, True, 7.7)
    b, m, h, w, ksp, c = CASES[name]
    minus_inf = R.statement(q, k, v, ksp, True, h, w, mask_value=float("-inf"))
    assert (minus_inf - want["out"]).abs().max().item() > 0.5


@pytest.mark.parametrize("name", ["c64", "c96"])
def test_full_attention_at_64_and_96_channels(name):
    """K = 1, no shift, one window of all tokens: through full_attention, and its bits through the C ABI under the rule."""
    b, _, h, w, _, c = CASES[name]
    q, k, v, g = R.random_case(b, 0, h, w, c=c, scale=3.0, seed=3100 + c, device=DEV)
    want, sc, lines, got, _ = _evaluate(q, k, v, g, 1, h * w, 1, False)
    _check_rule(f"{name}/full", got, want, sc, lines)
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = wa.full_attention(q, k, v)
    out.backward(g)
    assert torch.equal(out, got["out"]) and torch.equal(q.grad, got["g_q"])
    assert torch.equal(k.grad, got["g_k"]) and torch.equal(v.grad, got["g_v"])


@pytest.mark.parametrize("name", list(CASES))
def test_the_python_layer_gives_the_c_abi_s_bits(name):
    (q, k, v, g), _, _, _, got, _ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    again = _python(q, k, v, g, h, w, ksp, True)
    assert all(torch.equal(x, got[n]) for x, n in zip(again, R.ROW_NAMES))
    out, lse = wa.attention_forward(q, k, v, height=h, width=w, num_splits=ksp, with_shift=True)
    assert torch.equal(out, got["out"]) and torch.equal(lse, got["lse"])


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, True), (False, False, True), (False, True, False)])
@pytest.mark.parametrize("name", ["c64", "c96"])
def test_partial_gradients_at_64_and_96_channels(name, needs):
    """With the full call these run all five backward instantiations of NCB = 2 and 3; each is bit-equal to the full call."""
    (q, k, v, g), _, _, _, got, _ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    part = _python(q, k, v, g, h, w, ksp, True, needs=needs)
    assert torch.equal(part[0], got["out"])
    for need, x, n in zip(needs, part[1:], R.ROW_NAMES[1:4]):
        assert (x is None) if not need else torch.equal(x, got[n]), n


# ------------------------------------------------------------------------------------------------ structure
STRUCTURE = ["c96", "m5"]


@pytest.mark.parametrize("name", STRUCTURE)
def test_a_zero_gradient_gives_exact_zeros(name):
    (q, k, v, g), *_ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    got, _ = _abi(q, k, v, torch.zeros_like(g), h, w, ksp, True)
    for n in ("g_q", "g_k", "g_v", "delta"):
        assert int(torch.count_nonzero(got[n])) == 0, n


@pytest.mark.parametrize("name", STRUCTURE)
def test_a_one_hot_gradient_reaches_its_window_only(name):
    """One query row of g_out non-zero: exact zeros wherever row_scales says 0 (every other query row of g_q and delta, every key
    of another window or batch element), the rule elsewhere."""
    (q, k, v, g), *_ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    bi, row = b - 1, (h // 2) * w + 3
    hot = torch.zeros_like(g)
    hot[bi, row] = g[bi, row]
    want, sc, lines, got, _ = _evaluate(q, k, v, hot, h, w, ksp, True)
    assert int((sc["g_q"] > 0).sum()) == 1 and int((sc["g_k"] > 0).sum()) == max(m, 1) * (h * w) // ksp ** 2
    for n in ("g_q", "g_k", "g_v", "delta"):
        assert int(torch.count_nonzero(got[n][sc[n] == 0])) == 0, n
    _check_rule(f"{name}/one-hot", got, want, sc, lines)


@pytest.mark.parametrize("name", STRUCTURE)
def test_equal_scores_give_the_mean_of_v(name):
    """q = 0 (the constant for which it holds whatever k is): every unmasked score of a row is 0 and every masked one -100, so
    lse is log(n_same + n_other e^-100) by counting and out the so-weighted mean of v: both to the rule."""
    (q, k, v, g), *_ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    q0 = torch.zeros_like(q)
    want, sc, lines, got, _ = _evaluate(q0, k, v, g, h, w, ksp, True)
    tok, region = R.window_index(h, w, ksp, True, DEV)
    lw, mm = tok.shape[1], max(m, 1)
    key_region = region[:, torch.arange(lw * mm, device=DEV) % lw]
    same = (region.unsqueeze(2) == key_region.unsqueeze(1)).sum(-1).double()             # [K^2, Lw]
    counted = torch.log(same + (lw * mm - same) * torch.exp(torch.tensor(-100.0, dtype=torch.float64, device=DEV)))
    assert (want["lse"][:, tok] - counted).abs().max().item() <= 1e-12
    _check_rule(f"{name}/q=0", got, want, sc, lines, names=("out", "lse"))
    assert int(torch.count_nonzero(got["g_k"])) == 0           # dS k = 0 / sqrt(C) q: no query, no gradient to the keys


def test_a_window_one_token_high():
    """"thin": wh = 1, so sh = 0 and the rows add nothing to the mask: it is the column rule alone, the same in both window rows,
    and all zeros in the windows of column 0 (rolled columns 0 .. 7, one region).  There the shifted call is, bit for bit, the
    unshifted call on inputs rolled by (0, -sw) along the columns."""
    b, m, h, w, ksp, c = CASES["thin"]
    wh, ww = h // ksp, w // ksp
    assert (wh, wh // 2, ww // 2) == (1, 0, 4)
    dense = R.dense_mask(h, w, ksp, DEV)
    assert torch.equal(wa.ShiftMask(h, w, wh, ww, 0, ww // 2, device=DEV).dense(), dense)
    assert torch.equal(dense[:ksp], dense[ksp:]) and int(torch.count_nonzero(dense[0])) == 0
    column = (torch.arange(ww, device=DEV) >= ww - ww // 2)
    assert torch.equal(dense[1] != 0, column.unsqueeze(0) != column.unsqueeze(1))
    (q, k, v, g), _, _, _, got, _ = _run("thin", True, 1.0)
    roll = lambda t: torch.roll(t.reshape(b, h, w, c), shifts=-(ww // 2), dims=2).reshape(b, h * w, c).contiguous()
    plain, _ = _abi(roll(q), roll(k), roll(v), roll(g), h, w, ksp, False)
    tok, _ = R.window_index(h, w, ksp, True, DEV)
    tok0, _ = R.window_index(h, w, ksp, False, DEV)
    for win in (0, ksp):                                        # the windows of column 0
        for n in R.ROW_NAMES:
            assert torch.equal(got[n][:, tok[win]], plain[n][:, tok0[win]]), (win, n)
    assert not torch.equal(got["out"][:, tok[1]], plain["out"][:, tok0[1]])              # column 1 is masked


# ------------------------------------------------------------------------------------------------ ownership
@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_write_all_they_own_and_nothing_else(name):
    """out, lse, delta, g_q, g_k, g_v of _run are views into NaN-filled buffers between sentinels (doubles for lse and delta)."""
    for shift in (False, True):
        *_, got, bufs = _run(name, shift, 1.0)
        for n, (buf, numel) in bufs.items():
            _assert_owned(buf, numel, (name, shift, n))


@pytest.mark.parametrize("needs", [(True, False, True), (True, True, False), (False, True, True)])
@pytest.mark.parametrize("name", STRUCTURE)
def test_a_null_gradient_leaves_the_others_fully_written(name, needs):
    (q, k, v, g), _, _, _, full, _ = _run(name, True, 1.0)
    b, m, h, w, ksp, c = CASES[name]
    got, bufs = _abi(q, k, v, g, h, w, ksp, True, needs=needs)
    assert set(bufs) == {n for n, need in zip(("g_q", "g_k", "g_v"), needs) if need} | {"out", "lse", "delta"}
    for n, (buf, numel) in bufs.items():
        _assert_owned(buf, numel, (name, needs, n))
        assert torch.equal(got[n], full[n]), n
