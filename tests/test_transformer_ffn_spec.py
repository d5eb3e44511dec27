"""tests/transformer_ffn_reference.py against the reference's recorded outputs (tests/golden/transformer_ffn.npz, made by
tests/golden/make_golden_transformer_ffn.py from the reference's TransformerLayer on the CPU, d_model = 32, full attention): the
float64 layer statement is the reference's function, the float32 lines are its float32 run, and the rules the kernels implement —
the order of the concatenation, the erf GELU, the biased variance, the residual behind norm2 — are the ones a wrong rule would
miss.  Further the C ABI's declarations.  No GPU."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import transformer_ffn_reference as R
from splatter360_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "transformer_ffn.npz"
CASES = ("ffn", "no_ffn", "zero_norm")
NOT_STORED = ("q_proj.weight", "k_proj.weight", "v_proj.weight")
E24 = 2.0 ** -24
ENTRIES = ("s360_ffn_tail_scratch_bytes", "s360_ffn_tail_forward", "s360_ffn_tail_backward", "s360_layer_norm_residual_forward",
           "s360_layer_norm_residual_backward")


@functools.lru_cache(maxsize=None)
def recorded(case):
    """The case's arrays: inputs and parameters as float32 tensors, the float64 recordings, the float32 run rebuilt from its step
    distances."""
    with np.load(GOLDEN) as z:
        g = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}
        if case == "zero_norm":                                                     # the ffn case's layer but for norm2
            g.update({k[4:]: z[k] for k in z.files if k.startswith("ffn_p_") and not k.startswith("ffn_p_norm2")})

    def from_steps(want64, steps):
        i = np.ascontiguousarray(want64.astype(np.float32)).view(np.int32).astype(np.int64)
        key = np.where(i < 0, -(i & 0x7fffffff), i) + steps
        return np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32).view(np.float32).reshape(want64.shape)

    b, l, c, expansion, no_ffn = (int(x) for x in g["cfg"])
    value = lambda k: torch.from_numpy(g[k].astype(np.float32) / 64.0)             # noqa: E731
    names = [k[:-2] for k in g if k.endswith("64")]
    return {"source": value("source"), "target": value("target"), "g": value("g"),
            "params": {k[2:]: value(k) for k in g if k.startswith("p_")},
            "want64": {n: g[n + "64"] for n in names}, "run32": {n: from_steps(g[n + "64"], g[n + "32d"]) for n in names},
            "no_ffn": bool(no_ffn), "shape": (b, l, c, expansion)}


def layer_gradients(case, dtype, wrong=None):
    """{name: array} of the layer statement's output and gradients in `dtype`, named as the recording names them."""
    rec = recorded(case)
    keys = R.layer_params(rec["no_ffn"])
    tensors = [rec["source"], rec["target"], *(rec["params"][k] for k in keys)]

    def fn(source, target, *params):
        p = dict(zip(keys, params))
        if wrong is None:
            return R.layer_statement(p, source, target, rec["no_ffn"], dtype=dtype)
        q, k, v = source @ p["q_proj.weight"].T, target @ p["k_proj.weight"].T, target @ p["v_proj.weight"].T
        m = R.W.full_lines(q, k, v) @ p["merge.weight"].T
        return R.statement(source, m, p["norm1.weight"], p["norm1.bias"], p["mlp.0.weight"], p["mlp.2.weight"], p["norm2.weight"],
                           p["norm2.bias"], dtype=dtype, wrong=wrong)

    out = R.gradients(fn, tensors, rec["g"], dtype)
    return dict(zip(("out", "g_source", "g_target", *("g_" + k for k in keys)), (t.numpy() for t in out)))


def test_the_golden_file_is_small_and_holds_the_cases():
    assert GOLDEN.stat().st_size < 128 * 1024
    for case in CASES:
        rec = recorded(case)
        b, l, c, expansion = rec["shape"]
        assert c == 32 and rec["source"].shape == (b, l, c) == rec["target"].shape == rec["g"].shape
        assert set(rec["params"]) == set(R.layer_params(rec["no_ffn"]))
        assert set(rec["want64"]) == {"out", "g_source", "g_target"} | {"g_" + k for k in rec["params"] if k not in NOT_STORED}
        assert all(v.dtype == np.float64 for v in rec["want64"].values())
    assert recorded("ffn")["shape"][:2] == (2, 5) and not recorded("ffn")["no_ffn"] and recorded("no_ffn")["no_ffn"]
    zero = recorded("zero_norm")
    assert not zero["params"]["norm2.weight"].any() and not zero["params"]["norm2.bias"].any()
    assert np.array_equal(zero["want64"]["out"], zero["source"].double().numpy())   # the layer is the identity on source
    assert np.array_equal(zero["want64"]["g_source"], zero["g"].double().numpy())
    assert all(not zero["want64"]["g_" + k].any() for k in ("merge.weight", "norm1.weight", "norm1.bias", "mlp.0.weight", "mlp.2.weight"))


@pytest.mark.parametrize("case", CASES)
def test_layer_statement_and_float32_lines_reproduce_the_recorded_runs(case):
    """float64: the layer statement is the reference's function to float64 rounding (1e-12 of the largest element), inside the
    float32 run's own distance from it.  float32: the statement in float32 and the recorded run round the same operations; their
    sums may be taken in another order on another machine, which moves a sum of n float32 terms by at most n 2^-24 of the sum of
    the terms' magnitudes — n = 64, the longest sum here (the mlp's two products over 2C = 64 values)."""
    rec = recorded(case)
    want, lines = layer_gradients(case, torch.float64), layer_gradients(case, torch.float32)
    for name, rec64 in rec["want64"].items():
        rec32 = rec["run32"][name].astype(np.float64)
        top = np.abs(rec64).max()
        d64 = np.abs(want[name] - rec64).max()
        own = np.abs(rec32 - rec64).max()                                           # the float32 run's own distance
        d32 = np.abs(lines[name].astype(np.float64) - rec32).max()
        print(f"{case} {name}: statement {d64:.3e}, float32 run's own distance {own:.3e}, lines vs float32 run {d32:.3e}, largest {top:.3e}")
        assert want[name].dtype == np.float64 and lines[name].dtype == np.float32
        assert d64 <= 1e-12 * top and (d64 <= own or own == 0)                     # own == 0: sums of lattice values, exact in float32
        assert d32 <= 64 * E24 * top


@pytest.mark.parametrize("wrong", ["cat_order", "unbiased_variance", "residual_before_norm2"])
def test_a_wrong_rule_changes_the_result(wrong):
    rec = recorded("ffn")
    got = layer_gradients("ffn", torch.float64, wrong=wrong)
    moved = max(np.abs(got[n] - rec["want64"][n]).max() / np.abs(rec["want64"][n]).max() for n in ("out", "g_source", "g_mlp.0.weight"))
    print(f"{wrong}: moves the result by {moved:.3e} of the largest element")
    assert moved > 1e-2
    right = layer_gradients("ffn", torch.float64)
    assert np.abs(right["out"] - rec["want64"]["out"]).max() <= 1e-12 * np.abs(rec["want64"]["out"]).max()


def test_the_tanh_gelu_changes_the_result_where_the_hidden_units_sit_in_the_tail():
    """The tanh form is never further than 4.8e-4 from the erf form, so on hidden values of order one — the recorded ffn case — it
    moves the output and every gradient by 1.5e-4 to 1.2e-3 of the largest element (printed), not by 1e-2.  Where the form
    decides is the negative tail: at a pre-activation of -3.5 the two differ by a third of their value, and norm2 rescales a
    small z to unit size.  So the rule is shown on the statement itself (which the test above pins to the recording) with inputs
    whose pre-activations are -3.5 +- 0.5: norm1's weight 0 and bias 1 make LN1(m) the ones vector, whose columns of W1 are
    -3.5 / C; the source's columns add the spread."""
    rec = recorded("ffn")
    got = layer_gradients("ffn", torch.float64, wrong="tanh_gelu")
    on_record = max(np.abs(got[n] - rec["want64"][n]).max() / np.abs(rec["want64"][n]).max() for n in rec["want64"])
    x = torch.linspace(-8, 8, 16001, dtype=torch.float64)
    assert (R.gelu(x) - R.gelu(x, tanh=True)).abs().max().item() < 4.8e-4
    c, tokens = 32, 10
    gen = torch.Generator().manual_seed(5)
    source, m = (torch.randn(tokens, c, generator=gen, dtype=torch.float64) for _ in range(2))
    w1 = torch.cat([torch.randn(8 * c, c, generator=gen, dtype=torch.float64) * 0.5 / c ** 0.5,
                    torch.full((8 * c, c), -3.5 / c, dtype=torch.float64)], dim=1)
    w2 = torch.randn(c, 8 * c, generator=gen, dtype=torch.float64) / (8 * c) ** 0.5
    n2w, n2b = 1 + 0.2 * torch.randn(c, generator=gen, dtype=torch.float64), 0.2 * torch.randn(c, generator=gen, dtype=torch.float64)
    tensors = (source, m, torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64), w1, w2, n2w, n2b)
    right, wrong = R.statement(*tensors), R.statement(*tensors, wrong="tanh_gelu")
    moved = ((right - wrong).abs().max() / right.abs().max()).item()
    print(f"tanh_gelu: moves the recorded case by {on_record:.3e}, the tail case by {moved:.3e} of the largest element")
    assert on_record > 1e-4 and moved > 1e-2


def test_the_tail_statement_is_the_layer_s_tail_and_the_float32_lines_follow_it():
    """statement and reference_lines on the tail's own tensors (C = 128, hidden 1024, the shapes the GPU tests use): the float32
    lines stay within 1024 x 2^-24 of the float64 statement, and norm_statement is the no_ffn tail."""
    tensors, g = R.random_case(7, seed=3)
    want = R.gradients(lambda *t: R.statement(*t), tensors, g, torch.float64)
    lines = R.gradients(lambda *t: R.reference_lines(*t), tensors, g)
    for name, w64, l32 in zip(("out", *R.TAIL_NAMES), want, lines):
        assert w64.dtype == torch.float64 and l32.dtype == torch.float32
        assert (l32.double() - w64).abs().max().item() <= 1024 * E24 * w64.abs().max().item(), name
    ntensors, g = R.norm_case((tensors, g))
    want = R.gradients(lambda *t: R.norm_statement(*t), ntensors, g, torch.float64)
    lines = R.gradients(lambda *t: R.norm_lines(*t), ntensors, g)
    for name, w64, l32 in zip(("out", *R.NORM_NAMES), want, lines):
        assert (l32.double() - w64).abs().max().item() <= 128 * E24 * w64.abs().max().item(), name
    assert torch.equal(want[4], g.double())                                        # the residual's gradient is g itself


def test_the_header_declares_the_entries_and_the_library_exports_them():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\b(int|size_t)\s+{name}\s*\(", header), name
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25
    assert "s360_transformer_ffn.hip" in _lib.SOURCES and (ROOT / "splatter360_amd" / "csrc" / "s360_transformer_ffn.hip").exists()


def test_the_host_only_entries_and_the_argument_checks_need_no_gpu():
    """The scratch size is fixed beyond sixteen chunks; unsupported widths, null pointers and sizes < 1 are refused before any GPU
    work (the refusals below would otherwise fail on a machine without one).  The two backward entries likewise: an output that
    aliases an input, another output or the scratch, a pointer that is not 16-byte aligned, a null pointer, a scratch one byte
    short (S360_E_WORKSPACE) and unsupported widths, every one with nothing else wrong in the call."""
    import ctypes as C
    lib = _lib.lib()
    assert lib.s360_ffn_tail_scratch_bytes(0) == 0 and lib.s360_ffn_tail_scratch_bytes(-3) == 0
    sizes = [lib.s360_ffn_tail_scratch_bytes(t) for t in (1, 33, 65, 512, 513, 65536, 1 << 20, (1 << 24) - 1)]
    assert min(sizes) > 0 and max(sizes) == sizes[-1] == sizes[-2] == sizes[-3] == 26 * 1024 * 1024
    assert [lib.s360_ffn_tail_weight_chunks(t) for t in (1, 32, 33, 64, 65, 512, 513, 65536)] == [1, 1, 2, 2, 3, 16, 9, 16]
    eps = C.byref(C.c_double(1e-5))
    p = C.c_void_p(4096)                                                            # never dereferenced: every call below is refused
    fwd = lambda tokens, c, h, *ptrs: lib.s360_ffn_tail_forward(*ptrs, tokens, c, h, eps, C.c_void_p(8192), C.c_void_p(12288), C.c_void_p(16384), None)  # noqa: E731
    assert fwd(4, 64, 512, *[p] * 8) == -4 and fwd(4, 128, 512, *[p] * 8) == -4 and fwd(0, 128, 1024, *[p] * 8) == -1
    assert fwd(4, 128, 1024, None, *[p] * 7) == -1
    assert fwd(4, 128, 1024, C.c_void_p(8192), *[p] * 7) == -1                     # out aliases source
    assert fwd(1 << 24, 128, 1024, *[p] * 8) == -1                                  # 2^31 elements
    assert lib.s360_layer_norm_residual_forward(p, p, p, p, 4, 96, eps, C.c_void_p(8192), C.c_void_p(16384), None) == -4
    assert lib.s360_layer_norm_residual_forward(p, p, p, p, 4, 128, None, C.c_void_p(8192), C.c_void_p(16384), None) == -1
    # the backward entries: eleven inputs, the scratch and eight outputs (the no_ffn tail: four, the scratch and four), every one
    # at an address of its own, then one thing wrong per call
    tokens = 545
    need = lib.s360_ffn_tail_scratch_bytes(tokens)
    at = lambda i: 4096 * (i + 1)                                                   # noqa: E731
    ins, scratch, outs = [at(i) for i in range(11)], at(11), [at(12 + i) for i in range(8)]

    def bwd(ins=ins, scratch=scratch, outs=outs, tokens=tokens, c=128, h=1024, eps=eps, scratch_bytes=need):
        v = lambda a: None if a is None else C.c_void_p(a)                          # noqa: E731
        return lib.s360_ffn_tail_backward(*map(v, ins), tokens, c, h, eps, v(scratch), scratch_bytes, *map(v, outs), None)

    swap = lambda xs, i, a: [*xs[:i], a, *xs[i + 1:]]                                # noqa: E731
    assert bwd(scratch_bytes=need - 1) == -2 and bwd(scratch_bytes=0) == -2        # S360_E_WORKSPACE
    assert bwd(tokens=0) == -1 and bwd(tokens=1 << 24) == -1 and bwd(eps=None) == -1
    assert bwd(c=64, h=512) == -4 and bwd(h=512) == -4 and bwd(c=96) == -4          # unsupported widths
    for i in range(8):
        assert bwd(outs=swap(outs, i, None)) == -1, i                               # a null gradient pointer
        assert bwd(outs=swap(outs, i, outs[i] + 8)) == -1, i                        # 8-byte aligned only
        assert bwd(outs=swap(outs, i, scratch)) == -1, i                            # a gradient in the scratch
        for j in range(11):
            assert bwd(outs=swap(outs, i, ins[j])) == -1, (i, j)                    # an output that aliases an input
        for j in range(i + 1, 8):
            assert bwd(outs=swap(outs, i, outs[j])) == -1, (i, j)                   # two outputs that alias each other
    for j in range(11):
        assert bwd(ins=swap(ins, j, None)) == -1 and bwd(ins=swap(ins, j, ins[j] + 4)) == -1, j
        assert bwd(scratch=ins[j]) == -1, j
    assert bwd(scratch=None) == -1 and bwd(scratch=scratch + 8) == -1
    nins, nouts = ins[:4], outs[:4]

    def nbwd(ins=nins, scratch=scratch, outs=nouts, tokens=tokens, c=128, scratch_bytes=need):
        v = lambda a: None if a is None else C.c_void_p(a)                          # noqa: E731
        return lib.s360_layer_norm_residual_backward(*map(v, ins), tokens, c, v(scratch), scratch_bytes, *map(v, outs), None)

    assert nbwd(scratch_bytes=need - 1) == -2 and nbwd(tokens=0) == -1 and nbwd(tokens=1 << 24) == -1
    assert nbwd(c=96) == -4 and nbwd(c=64) == -4
    for i in range(4):
        assert nbwd(outs=swap(nouts, i, None)) == -1 and nbwd(outs=swap(nouts, i, nouts[i] + 8)) == -1, i
        assert nbwd(outs=swap(nouts, i, scratch)) == -1, i
        for j in range(4):
            assert nbwd(outs=swap(nouts, i, nins[j])) == -1, (i, j)
        for j in range(i + 1, 4):
            assert nbwd(outs=swap(nouts, i, nouts[j])) == -1, (i, j)
    for j in range(4):
        assert nbwd(ins=swap(nins, j, None)) == -1 and nbwd(ins=swap(nins, j, nins[j] + 4)) == -1 and nbwd(scratch=nins[j]) == -1, j
    assert nbwd(scratch=None) == -1 and nbwd(scratch=scratch + 8) == -1
