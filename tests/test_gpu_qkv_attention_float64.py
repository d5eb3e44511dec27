"""The fused multi-head QKV attention (csrc/s360_qkv_attention.hip) held to float64 PER ROW — per (batch element, head, joint
token) — with lse and Delta included.  tests/test_gpu_qkv_attention.py pools each tensor into one maximum and one mean; at input
scale 6 the scale of a key row of g_k spans sixteen orders of magnitude within one tensor, so a pooled maximum sees a handful of
rows, and it compares neither lse nor Delta.  Here every query row and every key row is measured against its own scale.

Three evaluations of the same float32 inputs on the same GPU: the kernels (through the C ABI, into NaN-filled buffers between
sentinels, so every run also shows that the kernels write all they own and nothing else), qkv_attention_reference.row_scales in
float64 (the statement's values and each row's scale: the window attention's formulas for one unmasked window of the L joint
tokens) and qkv_attention_reference.lines_rows, the stock float32 lines (the yardstick).

Rule (the project's, tests/test_gpu_window_attention_float64.py), for every run and each of out, g_q, g_k, g_v, lse, delta, with a
row's error max_c |x - want| / max(scale, 2^-100) in units of 2^-24 (no row is left out; a row of scale 0 must be exactly 0):

    kernel's worst row <= max(2 x yardstick's worst row, 0.5) units,    yardstick's worst row <= 4 units, else "not usable"

tests/test_qkv_attention_rows.py pins the measure on the CPU (and shows defects that the pooled rule passes and this one fails).
Each test prints `[qa64] case quantity kernel/yardstick` (pytest -s).  The cases (R.ROW_CASES) are the pooled file's nine and
`edge` (five tiles on four waves, two valid rows in the last), `thin4` (one tile over four views), `one` (T = 1), `mixed` and
`new_mixed` (heads x 6, 2.2, 0.8, 0.3 and batch rows of g x 1 .. 1e-3 in one tensor), at input scales 1, 3 and 6.

Measured on one MI355X (the 38 runs and the structure cases — one-hot g: 6 quantities, q = 0: out and lse, k + c: out — 246 figures;
worst row in units of 2^-24, kernel / float32 lines):

    quantity   kernel            lines             largest kernel / bound          the case of the largest ratio
    out        0.000 to 1.100    0.000 to 1.564    0.631 / 0.808 = 0.78            tile/x1
    g_q        0.000 to 0.289    0.000 to 0.858    0.206 / 0.500 = 0.41            views3/x1
    g_k        0.000 to 2.005    0.000 to 2.385    2.005 / 3.880 = 0.52            long/x6
    g_v        0.004 to 1.191    0.000 to 2.640    0.764 / 1.630 = 0.47            straddle/one-hot
    lse        0.000 to 0.768    0.089 to 2.264    0.599 / 0.892 = 0.67            one/x3
    delta      0.003 to 0.295    0.008 to 0.717    0.210 / 0.500 = 0.42            one/x1

(the zeros are `one` at scale 6: two keys, all weight on one).  Found by this file: nothing; every run passes with the kernels as
they were, every buffer is fully written with its sentinels intact, and heads 1 to 3 keep their bits when head 0 changes.

Planted on scratch builds, arithmetic only (never an index: the window file's note), the 38 runs here against the 19 accuracy and
lse tests of the pooled file: `alpha` applied to O after the tile's accumulate in k_qa_forward fails all 38 runs here and 18 of
the pooled file's 19.  lse narrowed to float before the subtraction in k_qa_backward_kv does NOT fail this file (largest
kernel / bound 0.78, in out; g_k 0.55, g_v 0.67) and fails 10 tests of the pooled file (every shape at scale 6 and `frames_unused`
at 1); Delta as the plain sum P dP without the division by sum P does NOT fail this file either (g_q and g_k as in the table,
delta 0.43) and fails the pooled file's `tiny` at scale 6.  Both are roundings of 2^-25 |lse| in an exponent or 1e-7 |Delta|, inside
what a row's scale — the (1 + a + A) factor, (1 + 2 A) |Delta| in e — grants a float32 score, while the pooled file compares with
the lines' actual error; what the pooled file cannot see (rows of small scale, lse, Delta, another head or batch element, unwritten
or overwritten memory) is tests/test_qkv_attention_rows.py's subject.  The two files are kept side by side for that reason.
"""
import ctypes as C
import functools

import pytest
import torch

import qkv_attention_reference as R
from splatter360_amd import _lib, qkv_attention as qa

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = R.ROW_CASES
CH = 32
YARDSTICK_LIMIT = 4.0
GUARD = 64                                                      # sentinel elements on either side: 256 B of floats, 512 B of doubles
_SENTINEL = 12345.678
STRUCTURE = ["straddle", "thin4"]
GRADS = ("g_q", "g_k", "g_v")


def _dims(name):
    """(N, walked views, B, heads, T, L, order) of a case."""
    n, views, cross, heads, t, order = CASES[name]
    nv = views if cross else 1
    return n, nv, n // nv, heads, t, nv * t, order


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


def _abi(name, qkv, g):
    """One forward and one backward call of the C ABI.  Returns (got, raw, bufs): raw maps out, lse, delta, g_qkv to views into
    the guarded buffers in the kernels' layouts, got maps R.ROW_NAMES to the per-row indexing of the same memory, bufs maps the
    four to (buffer, owned elements)."""
    n, nv, b, heads, t, length, order = _dims(name)
    assert qkv.is_contiguous() and g.is_contiguous() and qkv.dtype == g.dtype == torch.float32
    assert tuple(qkv.shape) == (n, heads * 3 * CH, t) and tuple(g.shape) == (n, heads * CH, t)
    shapes = dict(out=(n, heads * CH, t), lse=(b, heads, length), delta=(b, heads, length), g_qkv=(n, heads * 3 * CH, t))
    bufs, raw = {}, {}
    for k, shape in shapes.items():
        numel = int(torch.Size(shape).numel())
        buf = _guarded(numel, torch.float64 if k in ("lse", "delta") else torch.float32)
        bufs[k] = (buf, numel)
        raw[k] = buf[GUARD:GUARD + numel].view(shape)
    p = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    dims = (n, nv, heads, CH, t, qa.ORDERS[order])
    lib = _lib.lib()
    _lib.check(lib.s360_qkv_attention_forward(p(qkv), *dims, p(raw["out"]), p(raw["lse"]), stream), "forward")
    _lib.check(lib.s360_qkv_attention_backward(p(qkv), p(raw["lse"]), p(g), *dims, p(raw["delta"]), p(raw["g_qkv"]), stream), "backward")
    torch.cuda.synchronize()
    _, views, cross, *_ = CASES[name]
    got = dict(zip(R.ROW_NAMES, (R.out_rows(raw["out"], heads, views, cross), *R.qkv_rows(raw["g_qkv"], heads, views, cross, order),
                                 raw["lse"], raw["delta"])))
    return got, raw, bufs


def _evaluate(name, qkv, g):
    n, views, cross, heads, t, order = CASES[name]
    want, scale = R.row_scales(qkv, g, heads, views, cross, order)
    lines = R.lines_rows(qkv, g, heads, views, cross, order)
    got, raw, bufs = _abi(name, qkv, g)
    return want, scale, lines, got, raw, bufs


@functools.lru_cache(maxsize=None)
def _run(name, scale=1.0):
    """Inputs, row_scales, the float32 lines and the kernels' results of one run: computed once, shared, never modified."""
    inputs = R.row_inputs(name, scale, device=DEV)
    return (inputs, *_evaluate(name, *inputs))


def _check_rule(tag, got, want, scale, lines, names=R.ROW_NAMES):
    failures = []
    for n in names:
        x = got[n]
        assert x.dtype == (torch.float64 if n in ("lse", "delta") else torch.float32) and x.shape == want[n].shape, (tag, n)
        units = R.row_units(x, want[n], scale[n])
        kern = units.max().item()
        yard = R.row_units(lines[n], want[n], scale[n]).max().item()
        print(f"[qa64] {tag} {n} {kern:.3f}/{yard:.3f}")
        dead = scale[n] == 0                                    # nothing reaches these rows: exactly 0, not merely small
        if bool(dead.any()) and bool((x[dead] != 0).any()):
            failures.append((n, "a row of scale 0 is not 0", int((x[dead] != 0).sum())))
        if not yard <= YARDSTICK_LIMIT:
            failures.append((n, "yardstick not usable", yard))
        elif not kern <= max(2.0 * yard, 0.5):                  # a NaN fails here
            failures.append((n, kern, yard, "worst row of [B, heads, L]", tuple(units.shape), units.reshape(-1).argmax().item()))
    assert not failures, (tag, failures)


# ------------------------------------------------------------------------------------------------ the rule, run by run
@pytest.mark.parametrize("name,scale", R.ROW_RUNS)
def test_every_row_against_float64(name, scale):
    _, want, sc, lines, got, _, _ = _run(name, scale)
    _check_rule(f"{name}/x{scale:g}", got, want, sc, lines)


# ------------------------------------------------------------------------------------------------ ownership
@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_write_all_they_own_and_nothing_else(name):
    """out, lse, delta and g_qkv of _run are views into NaN-filled buffers between sentinels (doubles for lse and delta); then a
    backward through the Python layer into a caller's g_qkv buffer of the same kind, which gives the same bits."""
    (qkv, g), *_, raw, bufs = _run(name)
    n, views, cross, heads, t, order = CASES[name]
    assert set(bufs) == {"out", "lse", "delta", "g_qkv"}
    for k, (buf, numel) in bufs.items():
        _assert_owned(buf, numel, (name, k))
    buf = _guarded(qkv.numel(), torch.float32)
    mine = buf[GUARD:GUARD + qkv.numel()].view(qkv.shape)
    back = qa.attention_backward(qkv, raw["lse"], g, heads, n_frames=views, cross_view=cross, order=order, g_qkv=mine)
    torch.cuda.synchronize()
    assert back is mine
    _assert_owned(buf, qkv.numel(), (name, "a caller's g_qkv"))
    assert torch.equal(mine, raw["g_qkv"])


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.mark.parametrize("name", list(CASES))
def test_the_python_layer_gives_the_c_abi_s_bits(name):
    (qkv, g), *_, raw, _ = _run(name)
    n, views, cross, heads, t, order = CASES[name]
    opts = dict(n_frames=views, cross_view=cross, order=order)
    x = qkv.detach().clone().requires_grad_(True)
    out = qa.qkv_attention(x, heads, **opts)
    out.backward(g)
    assert torch.equal(out, raw["out"]) and torch.equal(x.grad, raw["g_qkv"])
    out, lse = qa.attention_forward(qkv, heads, **opts)
    assert torch.equal(out, raw["out"]) and torch.equal(lse, raw["lse"])
    # the gradient of a sum is an expanded tensor of stride 0: the layer hands the kernels what the ABI gets as a tensor of ones
    _, ones, _ = _abi(name, qkv, torch.ones_like(g))
    x = qkv.detach().clone().requires_grad_(True)
    qa.qkv_attention(x, heads, **opts).sum().backward()
    assert torch.equal(x.grad, ones["g_qkv"])


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("name", STRUCTURE)
def test_a_zero_gradient_gives_exact_zeros(name):
    (qkv, g), *_ = _run(name)
    got, raw, _ = _abi(name, qkv, torch.zeros_like(g))
    assert int(torch.count_nonzero(raw["g_qkv"])) == 0 and int(torch.count_nonzero(raw["delta"])) == 0


@pytest.mark.parametrize("name", STRUCTURE)
def test_a_one_hot_gradient_reaches_its_batch_element_and_head_only(name):
    """g non-zero at one token of one head of the last batch row: exact zeros wherever row_scales says 0 — every other head and
    batch element of g_qkv, every other query of g_q and delta — and the rule elsewhere; the keys it reaches are the L joint
    tokens of its (batch element, head), in every view."""
    (qkv, g), *_ = _run(name)
    n, nv, b, heads, t, length, order = _dims(name)
    hd, tok = heads - 1, t // 2
    hot = torch.zeros_like(g)
    hot[n - 1, hd * CH:(hd + 1) * CH, tok] = g[n - 1, hd * CH:(hd + 1) * CH, tok]
    want, sc, lines, got, raw, _ = _evaluate(name, qkv, hot)
    assert int((sc["g_q"] > 0).sum()) == int((sc["delta"] > 0).sum()) == 1 and bool(sc["g_q"][b - 1, hd, (nv - 1) * t + tok] > 0)
    assert int((sc["g_k"] > 0).sum()) == int((sc["g_v"] > 0).sum()) == length and bool((sc["g_k"][b - 1, hd] > 0).all())
    for k in (*GRADS, "delta"):
        assert int(torch.count_nonzero(got[k][sc[k] == 0])) == 0, k
    live = int(torch.count_nonzero(raw["g_qkv"].reshape(n, -1, t).abs().amax(1)))   # (batch row, token) pairs with anything in them
    assert live <= length
    _check_rule(f"{name}/one-hot", got, want, sc, lines)


@pytest.mark.parametrize("name", STRUCTURE)
def test_zero_queries_give_the_mean_of_v(name):
    """q = 0: every score is 0 whatever k is, so lse = log L and out is the mean of v over the joint sequence (to 1e-12 in the
    statement, to the rule in the kernels), and dS^T q = 0: the k rows of g_qkv are exactly zero."""
    (qkv, g), *_ = _run(name)
    n, views, cross, heads, t, order = CASES[name]
    length = _dims(name)[5]
    x = qkv.clone()
    R.parts(x, heads, order)[0].zero_()                         # a view: the q rows of every head
    want, sc, lines, got, raw, _ = _evaluate(name, x, g)
    log_l = torch.log(torch.tensor(float(length), dtype=torch.float64))
    assert (want["lse"] - log_l).abs().max().item() <= 1e-12
    mean_v = R.qkv_rows(x.double(), heads, views, cross, order)[2].mean(dim=2, keepdim=True)
    assert (want["out"] - mean_v).abs().max().item() <= 1e-12
    _check_rule(f"{name}/q=0", got, want, sc, lines, names=("out", "lse"))
    assert int(torch.count_nonzero(got["g_k"])) == 0
    assert int(torch.count_nonzero(R.parts(raw["g_qkv"], heads, order)[1])) == 0


@pytest.mark.parametrize("name", STRUCTURE)
def test_the_same_shift_on_every_key_moves_the_maximum_and_not_the_weights(name):
    """k_j + c for every key j of a head moves every score of query i by q_i . c / sqrt(ch): the running maximum and lse move
    (by more than 1 in some row, asserted), the weights do not.  out obeys the rule against the statement of the shifted input,
    which is the unshifted statement but for float64 rounding."""
    (qkv, g), want0, *_ = _run(name)
    n, views, cross, heads, t, order = CASES[name]
    c = torch.randn(heads, CH, generator=torch.Generator().manual_seed(9)).to(DEV) * 2.0
    x = qkv.clone()
    R.parts(x, heads, order)[1].add_(c.view(1, heads, CH, 1))
    want, sc, lines, got, _, _ = _evaluate(name, x, g)
    moved = (want["lse"] - want0["lse"]).abs().max().item()
    print(f"{name}: lse moves by up to {moved:.2f}")
    assert moved > 1.0
    # the weights stay but for the float32 rounding of k + c: a score moves by at most 2^-24 max|k + c| sum_c |q_ic| / sqrt(ch),
    # a weight by twice that relative to itself, out by that times max|v|
    q, k, v = R.qkv_rows(x.double(), heads, views, cross, order)
    slack = 2.0 * R.UNIT * k.abs().max().item() * q.abs().sum(-1).max().item() / CH ** 0.5 * v.abs().max().item()
    assert (want["out"] - want0["out"]).abs().max().item() <= slack
    _check_rule(f"{name}/k+c", got, want, sc, lines, names=("out",))


def test_the_heads_do_not_see_each_other():
    """`mixed` once more with head 0's q and k rows doubled: out, lse, delta and g_qkv of heads 1 to 3 keep their bits."""
    (qkv, g), *_, got, _, _ = _run("mixed")
    n, views, cross, heads, t, order = CASES["mixed"]
    x = qkv.clone()
    for rows in R.parts(x, heads, order)[:2]:
        rows[:, 0] *= 2.0
    again, _, _ = _abi("mixed", x, g)
    for k in R.ROW_NAMES:
        assert torch.equal(again[k][:, 1:], got[k][:, 1:]), k
        assert not torch.equal(again[k][:, 0], got[k][:, 0]), k
