"""The fused transformer FFN tail on the GPU (csrc/s360_transformer_ffn.hip through splatter360_amd/transformer_ffn.py) against the
float64 statement of tests/transformer_ffn_reference.py, with the reference's float32 lines on the same GPU and inputs as the
yardstick.

Accuracy rule (the project's, tests/test_gpu_qkv_attention.py): for each of out, g_source, g_m, g_W1, g_W2 and the four LayerNorm
parameter gradients of ffn_tail, and for out, g_x, g_weight, g_bias and g_residual of layer_norm_residual — over all elements, the
kernel's max and mean absolute error against statement(float64) are <= max(1.5 x the same figure of the float32 lines,
2^-24 max|want|).

Measured on one MI355X (kernel / float32 lines; eight cases x two scales; zero_norm's exact zeros left out).  ffn_tail, maxima and
means: out 0.37 to 0.85 and 0.45 to 0.66; g_source 0.18 to 0.93 and 0.34 to 0.73; g_m 0.26 to 1.05 and 0.34 to 0.73; norm1's weight
and bias gradients 0.26 to 0.81 and 0.27 to 0.79; g_w1 0.28 to 1.13 and 0.46 to 0.66; g_w2 0.36 to 0.99 and 0.37 to 0.67; norm2's
0.10 to 0.74 and 0.13 to 0.70.  layer_norm_residual: out 0.43 to 1.00 and 0.48 to 0.90 (one rounding of the sum either way), g_x
0.23 to 0.55 and 0.28 to 0.45, the parameter gradients 0.09 to 0.68 and 0.10 to 0.50, g_residual exact.  The layer through the seam
(both no_ffn values, with and without install(window_attention=True): 44 tensors) 0.11 to 1.17 and 0.14 to 1.00.
Three arrangements missed the rule before this one held (the kernel file's comments say where): dX as one float32 chain over the
hidden width (g_source, g_m and norm1's gradients: maxima 2.1 to 3.9 x, means 1.4 to 1.6 x; now one chain per 32-unit chunk, the
chunks added), dz W2c in chains of 64 values, and X W1c^T in chains of 64 values in the weight-owned pass, where gelu' near 0 turns
the rounding of a pre-activation that is a small difference of large terms (inputs of scale 6) into an error of dH: g_w1 of `tiny`
at scale 6 stood at 1.67 x, of `constant_row` at 1.52 x; with chains of 32 values they are 0.66 x and 0.71 x.
Memory at T = 32 768: forward + backward rise 108.5 MiB (0.85 of one hidden tensor); the float32 lines 464.8 MiB (3.63).
Every accuracy case here is one workgroup of the token-owned kernels and one tile per weight chunk, pooled into one maximum and one
mean per tensor: tests/test_gpu_transformer_ffn_float64.py holds the same kernels per row at the sizes past that (a second and
third workgroup, two and three tiles per chunk, both grid strides), with sentinels around every buffer.
"""
import functools
import sys

import pytest
import torch

import transformer_ffn_reference as R
from splatter360_amd import plugin, transformer_ffn as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 128


def _chunks_tokens():
    """The smallest T whose weight-gradient pass has at least three token chunks and a ragged last one."""
    t = 1
    while not (tf.weight_chunks(t) >= 3 and t % 32 != 0):
        t += 1
    return t


# name: leading dimensions (None: filled in by _lead) and what is special about the inputs
CASES = {
    "one": (1,),                                      # T = 1
    "tiny": (5,),                                     # less than a tile
    "tile": (32,),                                    # exactly one tile
    "ragged": (33,),                                  # one token past a tile: a second wave with one token
    "lead": (2, 3, 20),                               # leading dimensions; T = 120
    "chunks": None,                                   # three token chunks in the weight-gradient pass, the last one ragged
    "constant_row": (40,),                            # one row of m constant: its variance is 0
    "zero_norm": (37,),                               # norm2's weight and bias zero
}
SCALES = (1.0, 6.0)
FFN_OUT = ("out", "g_source", "g_m", "g_norm1_weight", "g_norm1_bias", "g_w1", "g_w2", "g_norm2_weight", "g_norm2_bias")
NORM_OUT = ("out", "g_x", "g_weight", "g_bias", "g_residual")


def _lead(name):
    return CASES[name] if CASES[name] is not None else (_chunks_tokens(),)


@functools.lru_cache(maxsize=None)
def _inputs(name, scale):
    lead = _lead(name)
    tokens = 1
    for n in lead:
        tokens *= n
    seed = 3000 + 7 * sorted(CASES).index(name)
    tensors, g = R.random_case(tokens, scale=scale, seed=seed, device=DEV, lead=lead)
    source, m, n1w, n1b, w1, w2, n2w, n2b = tensors
    if name == "constant_row":
        m = m.clone()
        m.view(-1, C)[tokens // 2] = 0.75 * scale
    if name == "zero_norm":
        n2w, n2b = torch.zeros_like(n2w), torch.zeros_like(n2b)
    return (source, m, n1w, n1b, w1, w2, n2w, n2b), g


def _native(fn, tensors, g):
    xs = [t.detach().clone().requires_grad_(True) for t in tensors]
    out = fn(*xs)
    out.backward(g)
    return (out.detach(), *(x.grad for x in xs))


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    """Inputs, the float64 statement, the float32 lines and the kernels' results of one case: computed once, shared, never
    modified."""
    tensors, g = _inputs(name, scale)
    want = R.gradients(lambda *t: R.statement(*t), tensors, g, torch.float64)
    lines = R.gradients(lambda *t: R.reference_lines(*t), tensors, g)
    got = _native(tf.ffn_tail, tensors, g)
    return (tensors, g), want, lines, got


@functools.lru_cache(maxsize=None)
def _run_norm(name, scale):
    tensors, g = R.norm_case(_inputs(name, scale))
    want = R.gradients(lambda *t: R.norm_statement(*t), tensors, g, torch.float64)
    lines = R.gradients(lambda *t: R.norm_lines(*t), tensors, g)
    got = _native(tf.layer_norm_residual, tensors, g)
    return (tensors, g), want, lines, got


def _errors(x, want):
    e = (x.double() - want).abs()
    return e.max().item(), e.mean().item()


def _check_rule(tag, names, want, lines, got):
    failures = []
    for n, w64, l32, x in zip(names, want, lines, got):
        assert x.dtype == torch.float32 and x.shape == w64.shape, (tag, n)
        assert torch.isfinite(x).all(), (tag, n)
        (kmax, kmean), (lmax, lmean) = _errors(x, w64), _errors(l32, w64)
        floor = 2.0 ** -24 * w64.abs().max().item()
        print(f"{tag} {n}: kernel max {kmax:.3e} mean {kmean:.3e} | float32 lines max {lmax:.3e} mean {lmean:.3e} | floor {floor:.3e}"
              f" | ratios {kmax / lmax if lmax else 0:.2f} {kmean / lmean if lmean else 0:.2f}")
        if not (kmax <= max(1.5 * lmax, floor) and kmean <= max(1.5 * lmean, floor)):
            failures.append((n, kmax, kmean, lmax, lmean, floor))
    assert not failures, (tag, failures)


def test_the_chunks_case_has_three_chunks_and_a_ragged_last_one():
    t = _chunks_tokens()
    chunks = tf.weight_chunks(t)
    per_chunk = -(-t // chunks)
    per_chunk += -per_chunk % 32                                                   # chunks are whole tiles of 32 tokens
    assert chunks >= 3 and 0 < t - (chunks - 1) * per_chunk < per_chunk and t % 32 != 0
    assert tf.weight_chunks(65536) == tf.weight_chunks(1 << 20)                     # a fixed number beyond that


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_ffn_tail_accuracy_against_the_float64_statement(name, scale):
    _, want, lines, got = _run(name, scale)
    _check_rule(f"ffn {name} scale={scale:g}", FFN_OUT, want, lines, got)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_layer_norm_residual_accuracy_against_the_float64_statement(name, scale):
    _, want, lines, got = _run_norm(name, scale)
    _check_rule(f"norm {name} scale={scale:g}", NORM_OUT, want, lines, got)


@pytest.mark.parametrize("scale", SCALES)
def test_zero_norm_is_the_identity_bit_for_bit(scale):
    (tensors, g), _, _, got = _run("zero_norm", scale)
    named = dict(zip(FFN_OUT, got))
    assert torch.equal(named["out"], tensors[0]) and torch.equal(named["g_source"], g)
    for n in ("g_m", "g_w1", "g_w2", "g_norm1_weight", "g_norm1_bias"):
        assert not named[n].any(), n
    assert named["g_norm2_weight"].abs().max().item() > 0 and named["g_norm2_bias"].abs().max().item() > 0


def _direct(tensors, g, buffers=None):
    out, z, stats = tf.ffn_tail_forward(*tensors)
    return (out, z, stats, *tf.ffn_tail_backward(*tensors, z, stats, g, buffers=buffers))


def _direct_norm(tensors, g, buffers=None):
    x, weight, bias, residual = tensors
    out, stats = tf.layer_norm_residual_forward(x, weight, bias, residual)
    return (out, stats, *tf.layer_norm_residual_backward(x, weight, stats, g, buffers=buffers))


@pytest.mark.parametrize("name", ["lead", "chunks"])
def test_forward_and_backward_are_deterministic(name):
    for run, direct in ((_run, _direct), (_run_norm, _direct_norm)):
        (tensors, g), _, _, got = run(name, 1.0)
        first = direct(tensors, g)
        skip = 3 if direct is _direct else 2
        assert torch.equal(first[0], got[0]) and all(torch.equal(x, y) for x, y in zip(first[skip:], got[1:]))   # the autograd node runs the same calls
        again = direct(tensors, g)
        assert all(torch.equal(x, y) for x, y in zip(first, again))
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            again = direct(tensors, g)
        side.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(first, again))
    tokens = _run(name, 1.0)[0][1].numel() // C
    z, stats = _direct(*_run(name, 1.0)[0])[1:3]
    assert z.shape == (tokens, C) and z.dtype == torch.float32 and stats.shape == (2, tokens, 2) and stats.dtype == torch.float64


def test_the_saved_statistics_are_the_statement_s():
    (tensors, g), _, _, _ = _run("lead", 1.0)
    _, z, stats = tf.ffn_tail_forward(*tensors)
    for k, x in enumerate((tensors[1].double().reshape(-1, C), z.double())):
        mean = x.mean(dim=1)
        rstd = 1 / torch.sqrt(((x - mean[:, None]) ** 2).mean(dim=1) + 1e-5)
        assert (stats[k, :, 0] - mean).abs().max().item() <= 1e-12 * x.abs().max().item()
        assert ((stats[k, :, 1] - rstd) / rstd).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", ["ragged", "chunks"])
def test_every_element_of_every_gradient_is_written(name):
    """The backwards write into buffers that hold NaN everywhere: the masked tails of the last tile and chunk included, nothing is
    left."""
    (tensors, g), _, _, got = _run(name, 1.0)
    buffers = {n: torch.full_like(t, float("nan")) for n, t in zip(tf.FFN_GRADIENTS, tensors)}
    res = _direct(tensors, g, buffers=buffers)[3:]
    for n, x, ref in zip(tf.FFN_GRADIENTS, res, got[1:]):
        assert x is buffers[n] and torch.isfinite(x).all() and torch.equal(x, ref), n
    (tensors, g), _, _, got = _run_norm(name, 1.0)
    buffers = {n: torch.full_like(t, float("nan")) for n, t in zip(tf.NORM_GRADIENTS, tensors)}
    res = _direct_norm(tensors, g, buffers=buffers)[2:]
    for n, x, ref in zip(tf.NORM_GRADIENTS, res, got[1:]):
        assert x is buffers[n] and torch.isfinite(x).all() and torch.equal(x, ref), n


def test_no_host_synchronisation():
    (tensors, g), _, _, got = _run("lead", 1.0)
    (ntensors, ng), _, _, ngot = _run_norm("lead", 1.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = _native(tf.ffn_tail, tensors, g)
        nagain = _native(tf.layer_norm_residual, ntensors, ng)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(again, got)) and all(torch.equal(x, y) for x, y in zip(nagain, ngot))


def test_a_non_contiguous_input_is_copied_once():
    (tensors, g), _, _, got = _run("ragged", 1.0)
    source = torch.cat([tensors[0], tensors[0]], dim=1)[:, :C]
    w1 = tensors[4].t().contiguous().t()
    assert not source.is_contiguous() and not w1.is_contiguous()
    again = _native(tf.ffn_tail, (source, *tensors[1:4], w1, *tensors[5:]), g)
    assert all(torch.equal(x, y) for x, y in zip(again, got))


def test_memory_stays_under_one_hidden_tensor():
    """T = 32 768: one [T, 8C] hidden tensor is 128 MiB.  A forward plus backward of the native path allocates out, z, g_source and
    g_m (16 MiB each; the test's own g_out is a fifth), 1 MiB of statistics, the parameter gradients and at most 26 MiB of
    T-independent scratch; the bound is ONE hidden tensor.  The float32 lines keep the concatenation and two hidden tensors for
    the backward by construction; their rise is measured here and printed."""
    tokens = 32768
    hidden = tokens * 1024 * 4
    tensors, _ = R.random_case(tokens, seed=3, device=DEV)
    tensors = [t.requires_grad_(True) for t in tensors]
    assert hidden == 128 * 1024 * 1024

    def rise(fn):
        def step():
            out = fn(*tensors)
            out.backward(torch.ones_like(out))
        step()                                                                      # warm-up
        for t in tensors:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(DEV)
        base = torch.cuda.memory_allocated(DEV)
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(DEV) - base
        assert all(torch.isfinite(t.grad).all() and t.grad.abs().max().item() > 0 for t in tensors)
        for t in tensors:
            t.grad = None
        return peak

    native, lines = rise(tf.ffn_tail), rise(R.reference_lines)
    print(f"forward + backward peak rise: native {native / 2 ** 20:.1f} MiB ({native / hidden:.2f} hidden tensors), "
          f"float32 lines {lines / 2 ** 20:.1f} MiB ({lines / hidden:.2f} hidden tensors)")
    assert native <= hidden
    assert lines >= 2 * hidden


def test_argument_errors_come_before_any_launch(monkeypatch):
    (tensors, g), _, _, _ = _run("tiny", 1.0)
    source, m, n1w, n1b, w1, w2, n2w, n2b = tensors
    monkeypatch.setattr(tf._lib, "lib", lambda: pytest.fail("a launch was reached"))
    with pytest.raises(ValueError, match="GPU"):
        tf.ffn_tail(source.cpu(), *tensors[1:])
    with pytest.raises(ValueError, match="float32"):
        tf.ffn_tail(source, m.half(), *tensors[2:])
    with pytest.raises(ValueError, match="C = 128"):
        tf.ffn_tail(source[:, :64], m[:, :64], *tensors[2:])
    with pytest.raises(ValueError, match="hidden width"):
        tf.ffn_tail(source, m, n1w, n1b, w1[:512], w2[:, :512], n2w, n2b)
    with pytest.raises(ValueError, match="shape"):
        tf.ffn_tail(source, m[:3], *tensors[2:])
    with pytest.raises(ValueError, match="shape"):
        tf.ffn_tail(source, m, n1w[:64], *tensors[3:])
    with pytest.raises(ValueError, match="eps"):
        tf.ffn_tail(*tensors, eps=0.0)
    with pytest.raises(ValueError, match="GPU"):
        tf.layer_norm_residual(m.cpu(), n1w, n1b, source)
    with pytest.raises(ValueError, match="float32"):
        tf.layer_norm_residual(m.double(), n1w, n1b, source)
    with pytest.raises(ValueError, match="shape"):
        tf.layer_norm_residual(m, n1w, n1b, source[:2])
    with pytest.raises(ValueError, match="C = 128"):
        tf.layer_norm_residual(m[:, :96], n1w[:96], n1b[:96], source[:, :96])
    with pytest.raises(ValueError, match="g_out"):
        tf.ffn_tail_backward(*tensors, torch.zeros_like(source), torch.zeros(2, 5, 2, dtype=torch.float64, device=DEV), g[:2])
    with pytest.raises(ValueError, match="tokens"):
        tf.weight_chunks(0)


# ---- the seam on the GPU -------------------------------------------------------------------------------------------------------

MODULE = plugin.TRANSFORMER_FFN_MODULE


@pytest.fixture
def standin():
    assert MODULE not in sys.modules
    mod = R.standin_module(MODULE)
    sys.modules[MODULE] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        del sys.modules[MODULE]


def _layer64(layer, source, target, g):
    keys = R.layer_params(layer.no_ffn)
    named = dict(layer.named_parameters())
    out = R.gradients(lambda s, t, *p: R.layer_statement(dict(zip(keys, p)), s, t, layer.no_ffn), [source, target, *(named[k] for k in keys)],
                      g, torch.float64)
    return out


def _layer32(layer, source, target, g):
    layer.zero_grad(set_to_none=True)
    s, t = (x.detach().clone().requires_grad_(True) for x in (source, target))
    out = layer(s, t, height=4, width=6, attn_num_splits=1)
    out.backward(g)
    named = dict(layer.named_parameters())
    return (out.detach(), s.grad, t.grad, *(named[k].grad.clone() for k in R.layer_params(layer.no_ffn)))


@pytest.mark.parametrize("with_window_attention", [False, True])
@pytest.mark.parametrize("no_ffn", [False, True])
def test_seam_runs_the_kernels_in_the_layer_and_holds_the_rule(standin, no_ffn, with_window_attention):
    """The stand-in TransformerLayer (d_model 128, 3 x 24 tokens, full attention): output, input gradients and every parameter
    gradient against the layer in float64, with the uninstalled float32 layer on the same GPU as the yardstick."""
    layer = R.randomise(standin.TransformerLayer(d_model=128, no_ffn=no_ffn), 21).to(DEV)
    gen = torch.Generator().manual_seed(22)
    source, target, g = (torch.randn(3, 24, 128, generator=gen).to(DEV) for _ in range(3))
    names = ("out", "g_source", "g_target", *("g_" + k for k in R.layer_params(no_ffn)))
    want = _layer64(layer, source, target, g)
    lines = _layer32(layer, source, target, g)
    assert layer.calls == 1
    plugin.install(lazy=True, transformer_ffn=True, window_attention=with_window_attention)
    wrapper = standin.TransformerLayer.__dict__["forward"]
    assert wrapper.replaced is not None and wrapper.native_calls == 0
    standin.calls.clear()
    got = _layer32(layer, source, target, g)
    assert wrapper.native_calls == 1 and layer.calls == 1                          # the kernels, once; the replaced method, never
    assert standin.calls == ([] if with_window_attention else [("full", None)])    # the attention came from the module's globals
    _check_rule(f"layer no_ffn={int(no_ffn)} window_attention={int(with_window_attention)}", names, want, lines, got)
    assert tuple(layer.state_dict()) == R.layer_params(no_ffn)
    cpu = R.randomise(standin.TransformerLayer(d_model=128, no_ffn=no_ffn), 21)
    cpu(source.cpu(), target.cpu(), attn_num_splits=1)                             # CPU tensors reach the replaced method
    assert cpu.calls == 1 and wrapper.native_calls == 1
    plugin.uninstall()
    assert getattr(standin.TransformerLayer.__dict__["forward"], "replaced", None) is None
    back = _layer32(layer, source, target, g)
    assert layer.calls == 2 and torch.equal(back[0], lines[0])
