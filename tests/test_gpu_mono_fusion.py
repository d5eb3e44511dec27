"""The fused mono-feature fusion (splatter360_amd.mono_fusion, csrc/s360_mono_fusion.hip) on the GPU.

Accuracy rule (the project's, tests/test_gpu_qkv_attention.py): for each of out, g_erp_feat, g_w1, g_ln_weight, g_ln_bias, g_w2 the
kernels' max and mean absolute error against mono_fusion_reference.statement(float64) are each <= max(1.5 x the same figure of
reference_lines (float32 torch on the device), 2^-24 max|want|).  No element is left out of any comparison.

ReLU decisions are not left to rounding.  The random cases assert that the float64 statement (on the CPU) has no LayerNorm output
with |value| < 2^-17 max|value| — about ten times the float32 evaluation error of a 128 + Cm term chain after normalisation — and
their seeds (SEEDS) were chosen so that this holds; the cases beyond 144 tokens are `decided_case`s, ln_weight = +-0.05 (lattice in
[0.5, 1]) and ln_bias = +-1, where |ln_weight x_hat| <= 0.05 sqrt(127) < 1 and every unit is on or off by its bias's sign.

Measured (kernel / float32 lines, worst ratio over the six results and both scales; max, mean):
  out          0.60 (zero_panorama at scale 1), 0.68 (long at scale 1)
  g_erp_feat   0.58 (straddle at scale 1), 0.64 (chunks at scale 6)
  g_w1         1.22 (wide at scale 1), 0.78 (wave at scale 6)
  g_ln_weight  1.03 (wide at scale 6), 0.74 (wide at scale 1)
  g_ln_bias    0.98 (wide at scale 1), 0.77 (straddle at scale 1)
  g_w2         0.63 (straddle at scale 1), 0.61 (tile at scale 6)
  the seam test (against the uninstalled run with rgbd_fusion in float64): out 0.30 / 0.36, g_erp_feat 0.42 / 0.61, g_w1 0.58 / 0.59, g_ln_weight 0.51 / 0.48, g_ln_bias 1.23 / 0.64, g_w2 0.43 / 0.37
Memory at N = 1, (64, 128, 256), Cm = 384 (32 768 tokens), forward + backward rise of torch.cuda.max_memory_allocated:
  native 75.3 MiB (its declared buffers are 75.3 MiB), reference_lines 160.3 MiB.
"""
import functools
import sys

import pytest
import torch

import mono_fusion_reference as R
import splatter360_amd
from splatter360_amd import mono_fusion as mf, plugin

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALES = (1.0, 6.0)
MIB = 1 << 20


def _chunks_n():
    """The smallest N on g3 with weight_chunks >= 3 and a ragged last chunk (tokens no multiple of the 64-token tile)."""
    fw, h, w = R.GEOMETRIES["g3"]
    return next(n for n in range(1, 64) if mf.weight_chunks(n * h * w) >= 3 and (n * h * w) % 64)


# name: (N, geometry, Cm, kind)
CASES = {
    "wave": (1, "g0", 64, "random"),             # fewer tokens than a workgroup, one K chunk of mono
    "tile": (1, "g1", 64, "random"),             # exactly one workgroup
    "straddle": (3, "g2", 192, "random"),        # 144 tokens: a tile spanning two panoramas, a ragged second tile
    "config": (1, "g1", 384, "random"),          # the configuration's width
    "wide": (1, "g0", 1024, "random"),           # the widest supported K
    "edges": (2, "g3", 64, "decided"),           # clipped taps, 4.5 workgroups
    "chunks": (None, "g3", 64, "decided"),       # the ordered partial sums: N = _chunks_n()
    "long": (8, "g3", 64, "decided"),            # 2 304 tokens = 36 tiles of the weight pass in 32 chunks: chunks of one and of two tiles
    "zero_panorama": (2, "g1", 64, "zero"),      # variance-0 rows
}
SEEDS = {"wave": 100, "tile": 101, "straddle": 100, "config": 100, "wide": 100, "zero_panorama": 101, "edges": 200, "chunks": 201, "long": 202}


def _case(name, scale):
    n, geometry, cm, kind = CASES[name]
    n = _chunks_n() if n is None else n
    make = R.decided_case if kind == "decided" else R.random_case
    tensors, g = make(n, geometry, cm, scale=scale, seed=SEEDS[name])
    if kind == "zero":
        tensors[0][1].zero_()
        tensors[1][1].zero_()
    return tensors, g


def _native(tensors, g):
    xs = [t.detach().clone() for t in tensors]
    for i in R.DIFFERENTIABLE:
        xs[i].requires_grad_(True)
    out = mf.mono_fusion(*xs)
    out.backward(g)
    return (out.detach(), *(xs[i].grad for i in R.DIFFERENTIABLE))


@functools.lru_cache(maxsize=None)
def _run(name, scale):
    """Inputs, the float64 statement (CPU), the float32 lines and the kernels' results (GPU) of one case: computed once, shared,
    never modified."""
    cpu, g = _case(name, scale)
    m = R.stitch32(cpu[1], cpu[2])
    want = R.gradients(lambda *t: R.statement(*t, m=m), cpu, g, torch.float64)
    dev = tuple(t.to(DEV) for t in cpu)
    lines = R.gradients(R.reference_lines, dev, g.to(DEV))
    got = _native(dev, g.to(DEV))
    torch.cuda.synchronize()
    return (cpu, g, m), tuple(w.to(DEV) for w in want), lines, got


def _errors(x, want):
    e = (x.double() - want).abs()
    return e.max().item(), e.mean().item()


def _check_rule(tag, want, lines, got, maxima_only=False):
    failures = []
    for n, w64, l32, x in zip(R.RESULTS, want, lines, got):
        assert x.dtype == torch.float32 and x.shape == w64.shape, (tag, n)
        assert torch.isfinite(x).all(), (tag, n)
        (kmax, kmean), (lmax, lmean) = _errors(x, w64), _errors(l32, w64)
        floor = 2.0 ** -24 * w64.abs().max().item()
        print(f"{tag} {n}: kernel max {kmax:.3e} mean {kmean:.3e} | float32 lines max {lmax:.3e} mean {lmean:.3e} | floor {floor:.3e}"
              f" | ratios {kmax / lmax if lmax else 0:.2f} {kmean / lmean if lmean else 0:.2f}")
        if not (kmax <= max(1.5 * lmax, floor) and (maxima_only or kmean <= max(1.5 * lmean, floor))):
            failures.append((n, kmax, kmean, lmax, lmean, floor))
    assert not failures, (tag, failures)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_against_the_float64_statement(name, scale):
    (cpu, _, m), want, lines, got = _run(name, scale)
    n, geometry, cm, kind = CASES[name]
    if kind != "decided":
        margin = R.ln_margin(cpu, m=m)
        assert margin >= 2.0 ** -17, (name, scale, margin)                                  # the seed was chosen for this
    else:
        assert cpu[0].shape[0] * cpu[0].shape[2] * cpu[0].shape[3] > 144
    _check_rule(f"{name} scale={scale:g}", want, lines, got)


def test_chunks_case_has_three_chunks_and_a_ragged_last_one():
    fw, h, w = R.GEOMETRIES["g3"]
    tokens = _chunks_n() * h * w
    assert mf.weight_chunks(tokens) >= 3 and tokens % 64 and tokens % 128
    assert mf.weight_chunks(8 * h * w) == 32 and -(-8 * h * w // 64) == 36


@pytest.mark.parametrize("scale", SCALES)
def test_rule_holds_over_the_clipped_pixels_alone(scale):
    """g3 has 16 pixels with a coordinate clipped to exactly +-1: a weight-0 tap at index fw.  The rule, maxima only, over the
    tokens of those pixels alone, for the two results that are indexed by token."""
    pix = torch.from_numpy(R.clipped_pixels("g3")).to(DEV)
    assert pix.numel() == 16
    _, want, lines, got = _run("edges", scale)
    sub = lambda t: t.reshape(t.shape[0], t.shape[1], -1)[:, :, pix]
    for i in (0, 1):
        w64, l32, x = sub(want[i]), sub(lines[i]), sub(got[i])
        kmax, lmax = _errors(x, w64)[0], _errors(l32, w64)[0]
        print(f"clipped pixels scale={scale:g} {R.RESULTS[i]}: kernel max {kmax:.3e} | lines max {lmax:.3e}")
        assert kmax <= max(1.5 * lmax, 2.0 ** -24 * w64.abs().max().item()), (R.RESULTS[i], kmax, lmax)


def test_zero_panorama_is_finite_and_its_rows_are_the_bias():
    (cpu, _, _), want, _, got = _run("zero_panorama", 1.0)
    assert all(torch.isfinite(x).all() for x in got)
    lnb, w2 = cpu[5].double(), cpu[6].double()
    row = (torch.relu(lnb) @ w2.T).to(DEV)                                                  # LN of a constant row is its bias
    assert torch.allclose(got[0][1].double(), row[:, None, None].expand_as(got[0][1]), rtol=0, atol=2.0 ** -22 * row.abs().max().item())


def test_dead_units_give_exact_zeros():
    (erp, cube, grid, w1, _, _, w2), g = R.random_case(1, "g1", 64, seed=300, device=DEV)
    lnw, lnb = torch.zeros(128, device=DEV), -torch.ones(128, device=DEV)
    got = _native((erp, cube, grid, w1, lnw, lnb, w2), g)
    for name, x in zip(R.RESULTS, got):
        assert torch.count_nonzero(x) == 0, name


def test_forward_and_backward_are_bit_identical_again_and_on_a_side_stream():
    tensors, g = (tuple(t.to(DEV) for t in _case("straddle", 1.0)[0]), _case("straddle", 1.0)[1].to(DEV))
    first = _native(tensors, g)
    second = _native(tensors, g)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = _native(tensors, g)
    side.synchronize()
    for name, a, b, c in zip(R.RESULTS, first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c), name


def _guarded(t, guard):
    """t inside an allocation whose `guard` elements before and after hold NaN; (the view, the whole allocation)."""
    assert (guard * t.element_size()) % 16 == 0
    whole = torch.full((guard + t.numel() + guard,), float("nan"), dtype=t.dtype, device=DEV)
    view = whole[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.is_contiguous()
    return view, whole


def test_no_tap_and_no_token_reads_outside_its_tensor():
    """mono_cube and erp_feat each inside an allocation whose guard regions before and after (one strip of the six faces / one
    channel plane each) hold NaN: every output stays finite, so no value from outside the tensors entered a sum.  g3 has the
    clipped pixels whose upper taps would fall at index fw."""
    (erp, cube, grid, w1, lnw, lnb, w2), g = _case("edges", 1.0)
    fw, h, w = R.GEOMETRIES["g3"]
    erp_v, erp_all = _guarded(erp, h * w)
    cube_v, cube_all = _guarded(cube, fw * 6 * fw)
    tensors = (erp_v, cube_v, *(t.to(DEV) for t in (grid, w1, lnw, lnb, w2)))
    out, y, stats = mf.mono_fusion_forward(*tensors)
    grads = mf.mono_fusion_backward(*tensors, y, stats, g.to(DEV))
    for x in (out, y, stats, *grads):
        assert torch.isfinite(x).all()
    want = _run("edges", 1.0)[3]
    assert torch.equal(out, want[0]) and all(torch.equal(a, b) for a, b in zip(grads, want[1:]))
    for whole, guard in ((erp_all, h * w), (cube_all, fw * 6 * fw)):
        assert torch.isnan(whole[:guard]).all() and torch.isnan(whole[-guard:]).all()


def test_every_output_element_is_written_and_nothing_else():
    """Outputs between NaN-prefilled sentinels: afterwards every output element is finite and every sentinel is still NaN."""
    cpu, g = _case("straddle", 1.0)
    tensors, g = tuple(t.to(DEV) for t in cpu), g.to(DEV)
    n, c, h, w = tensors[0].shape
    tokens, cm = n * h * w, tensors[1].shape[1]
    guard = 256
    shapes = {"out": ((n, c, h, w), torch.float32), "y": ((tokens, c), torch.float32), "stats": ((tokens, 2), torch.float64),
              "g_erp_feat": ((n, c, h, w), torch.float32), "g_w1": ((c, c + cm), torch.float32), "g_ln_weight": ((c,), torch.float32),
              "g_ln_bias": ((c,), torch.float32), "g_w2": ((c, c), torch.float32)}
    whole, bufs = {}, {}
    for name, (shape, dtype) in shapes.items():
        bufs[name], whole[name] = _guarded(torch.full(shape, float("nan"), dtype=dtype), guard)
    out, y, stats = mf.mono_fusion_forward(*tensors, buffers={k: bufs[k] for k in mf.FORWARD_OUTPUTS})
    assert out.data_ptr() == bufs["out"].data_ptr() and y.data_ptr() == bufs["y"].data_ptr() and stats.data_ptr() == bufs["stats"].data_ptr()
    grads = mf.mono_fusion_backward(*tensors, y, stats, g, buffers={k: bufs[k] for k in mf.GRADIENTS})
    assert all(x.data_ptr() == bufs[k].data_ptr() for x, k in zip(grads, mf.GRADIENTS))
    torch.cuda.synchronize()
    for name in shapes:
        assert torch.isfinite(bufs[name]).all(), name
        assert torch.isnan(whole[name][:guard]).all() and torch.isnan(whole[name][-guard:]).all(), name
    want = _run("straddle", 1.0)[3]
    assert torch.equal(out, want[0]) and all(torch.equal(a, b) for a, b in zip(grads, want[1:]))


def _rise(fn, tensors, g):
    xs = [t.detach().clone() for t in tensors]
    for i in R.DIFFERENTIABLE:
        xs[i].requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(*xs)
    out.backward(g)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_memory_is_the_declared_buffers_and_below_the_reference_lines():
    """N = 1, (64, 128, 256), Cm = 384: 32 768 tokens.  The native forward + backward rise is at most the bytes of its declared
    buffers (out, y, stats, g_erp_feat, the four parameter gradients, scratch_bytes) plus 2 MiB of allocator rounding per buffer,
    and below the rise of reference_lines."""
    geometry, cm, c = (64, 128, 256), 384, 128
    tensors, g = R.random_case(1, geometry, cm, seed=400, device=DEV)
    tokens = geometry[1] * geometry[2]
    declared = [tokens * c * 4, tokens * c * 4, tokens * 2 * 8, tokens * c * 4, c * (c + cm) * 4, c * 4, c * 4, c * c * 4, mf.scratch_bytes(tokens, cm)]
    native = _rise(mf.mono_fusion, tensors, g)
    lines = _rise(R.reference_lines, tensors, g)
    print(f"memory: native {native / MIB:.1f} MiB (declared {sum(declared) / MIB:.1f} MiB), reference_lines {lines / MIB:.1f} MiB")
    assert native <= sum(declared) + 2 * MIB * len(declared), (native, sum(declared))
    assert native < lines, (native, lines)


def test_seam_runs_one_native_call_forms_no_concatenation_and_uninstall_restores(monkeypatch):
    """The stand-in encoder under install(lazy=True, mono_fusion=True) on the GPU: one native call; during its forward the peak
    stays below T (C + Cm) 4 bytes over the inputs, so no tensor of C + Cm channels was allocated; output and gradients meet the
    accuracy rule against the uninstalled run with rgbd_fusion in float64; after uninstall() the original bits return."""
    name = plugin.MONO_FUSION_MODULE
    assert name not in sys.modules
    mod = R.standin_module(name)
    sys.modules[name] = mod
    try:
        n, geometry, cm, c = 2, R.GEOMETRIES["g1"], 384, 128
        tensors, g = R.random_case(n, geometry, cm, seed=500, device=DEV)
        feats, cube = tensors[0], tensors[1]
        tokens = n * geometry[1] * geometry[2]

        def run(enc, dtype=torch.float32):
            enc.zero_grad(set_to_none=True)
            x = feats.detach().clone().to(dtype).requires_grad_(True)
            out = enc(x, cube)
            out.backward(g.to(dtype))
            return (out.detach(), x.grad, *(p.grad for p in enc.rgbd_fusion.parameters()))

        build = lambda: R.set_parameters(mod.EncoderCostVolume(geometry, c, cm), tensors).to(DEV)
        before = run(build())
        want = build()
        want.rgbd_fusion.double()
        want = run(want, torch.float64)
        splatter360_amd.install(lazy=True, mono_fusion=True)
        enc = build()
        assert isinstance(enc.rgbd_fusion, mf.FusedMonoFusion)
        calls, native = [], mf.mono_fusion_forward
        monkeypatch.setattr(mf, "mono_fusion_forward", lambda *a, **k: calls.append(1) or native(*a, **k))
        x = feats.detach().clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = enc(x, cube)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert len(calls) == 1 and enc.c2e.calls == 0                                       # one native call, no stitch
        assert out.shape == feats.shape and out.is_contiguous() and type(out) is torch.Tensor
        print(f"seam: forward peak {peak} bytes over the inputs, a [T, C + Cm] tensor is {tokens * (c + cm) * 4}")
        assert peak < tokens * (c + cm) * 4, (peak, tokens * (c + cm) * 4)
        out.backward(g)
        got = (out.detach(), x.grad, *(p.grad for p in enc.rgbd_fusion.parameters()))
        _check_rule("seam", want, before, got)
        splatter360_amd.uninstall()
        after = run(build())
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    finally:
        splatter360_amd.uninstall()
        sys.modules.pop(name, None)
