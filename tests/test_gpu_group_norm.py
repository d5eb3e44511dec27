"""The fused group norm + activation + residual kernels (splatter360_amd.group_norm, csrc/s360_group_norm.hip) on the GPU
against the float64 statement of tests/group_norm_reference.py.

The accuracy rule, per element (derived, not measured: one float32 rounding plus 2^12 float64 ulps for summation order):
    out       |got - want| <= 2^-23 |want| + 2^-40 A,  A = |xh gamma_c| + |beta_c| + |residual|
    g_x       |got - want| <= 2^-23 |want| + 2^-40 r (|gamma_c dz| + |m1| + |xh m2|)
    g_weight, g_bias      <= 2^-23 |want| + 2^-40 sum |term|
    stats     mu and r within 2^-40 relative
For every relu case the statement has no element with |z| < 2^-30 A, so the branch cannot depend on rounding (asserted first;
the seeds of RELU_SEEDS were chosen on the CPU).

How far torch's float32 lines (F.group_norm, the activation, the add, autograd; the float32 CPU build of the same torch) sit from
the statement on the 144 cases of the first test, as the largest |got - want| / bound of a case — recorded so that a later
reader sees what the rule buys, not a bound (the bound of an element near zero is 2^-40 A, which float32 arithmetic misses by
orders of magnitude):
    out       median 727, largest 34 070      g_x     median 1 940, largest 448 958
    g_weight  median 11.5, largest 584        g_bias  median 9.6, largest 756
At the conditioning case (x = 2^20 + k / 16) the float32 lines are off by 0.15 - 0.17 absolute in out (2e9 - 3e10 bounds).
"""
import ctypes as C
import functools
import itertools
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import group_norm_reference as R
from splatter360_amd import _lib, group_norm as gn, plugin
from test_group_norm_spec import BLOCK_SEEDS, recorded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH = gn.ROW_CHUNK
SHAPES = {"gn8": ((2, 32, 6, 10), 8), "odd": ((1, 36, 5, 7), 4), "inst": ((3, 16, 5, 9), 16), "m4": ((1, 8, 1, 1), 2),
          "chunk-1": ((1, 4, CH - 1), 1), "chunk": ((1, 4, CH), 1), "chunk+1": ((1, 4, CH + 1), 1), "2chunk+5": ((1, 4, 2 * CH + 5), 1),
          "3d": ((2, 32, 24), 8)}
RELU_SEEDS = {name: i for i, name in enumerate(SHAPES)}                               # seed of make_case per shape
GUARD, SENTINEL = 64, 12345.678
NAMES = ("out", "g_x", "g_weight", "g_bias")
SCALES = {"out": "A", "g_x": "gx_scale", "g_weight": "gw_scale", "g_bias": "gb_scale"}


def dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


@functools.lru_cache(maxsize=None)
def case_of(name, affine, residual):
    shape, groups = SHAPES[name]
    return R.make_case(shape, groups, affine, residual, seed=RELU_SEEDS[name])


@functools.lru_cache(maxsize=None)
def want_of(name, act, affine, residual):
    c = case_of(name, affine, residual)
    return R.statement(c["x"], c["groups"], c["weight"], c["bias"], 1e-5, act, c["residual"], c["g_out"])


def native(c, act, eps=1e-5):
    """The Python layer, forward and backward -> {out, g_x, g_weight, g_bias, g_residual} (None where there is no input)."""
    x, w, b, res = (None if c[k] is None else dev(c[k]).requires_grad_(True) for k in ("x", "weight", "bias", "residual"))
    out = gn.group_norm_act(x, c["groups"], w, b, eps, act, res)
    out.backward(dev(c["g_out"]))
    return {"out": out.detach(), "g_x": x.grad, "g_weight": None if w is None else w.grad, "g_bias": None if b is None else b.grad,
            "g_residual": None if res is None else res.grad}


def assert_rule(got, want, what, names=NAMES):
    for n in names:
        if got.get(n) is not None:
            worst = R.worst(got[n], want[n], want[SCALES[n]])
            print(what, n, f"{worst:.3f} of the bound")
            assert worst <= 1.0, (what, n, worst)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("act", R.ACTIVATIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_accuracy_rule_forward_and_all_three_gradients(name, act, affine, residual):
    c, want = case_of(name, affine, residual), want_of(name, act, affine, residual)
    if act == "relu":
        assert R.relu_is_unambiguous(want)
    got = native(c, act)
    assert got["out"].dtype == torch.float32 and tuple(got["out"].shape) == SHAPES[name][0]
    assert_rule(got, want, (name, act, affine, residual))
    if residual:
        assert torch.equal(got["g_residual"], dev(c["g_out"]))                     # a pass-through
    _, stats = gn.norm_forward(dev(c["x"]), c["groups"], dev(c["weight"]), dev(c["bias"]), 1e-5, act, dev(c["residual"]))
    assert stats.dtype == torch.float64 and R.stats_worst(stats, want["stats"]) <= 1.0


# ---- conditioning ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_a_large_mean_over_a_small_spread(act):
    rng = np.random.default_rng(7)
    shape = (1, 4, 2 * CH + 5)
    c = R.make_case(shape, 1, True, True, seed=11)
    c["x"] = (2.0 ** 20 + rng.integers(0, 16, shape) / 16.0).astype(np.float32)
    assert np.array_equal(c["x"].astype(np.float64), 2.0 ** 20 + np.round((c["x"].astype(np.float64) - 2.0 ** 20) * 16) / 16)
    want = R.statement(c["x"], 1, c["weight"], c["bias"], 1e-5, act, c["residual"], c["g_out"])
    assert act != "relu" or R.relu_is_unambiguous(want)
    assert_rule(native(c, act), want, ("conditioning", act))
    _, stats = gn.norm_forward(dev(c["x"]), 1, dev(c["weight"]), dev(c["bias"]), 1e-5, act)
    assert R.stats_worst(stats, want["stats"]) <= 1.0


@pytest.mark.parametrize("act", R.ACTIVATIONS)
@pytest.mark.parametrize("name", ["gn8", "odd", "2chunk+5"])
def test_a_constant_slab_gives_the_activation_of_the_bias_exactly(name, act):
    c = dict(case_of(name, True, False))
    shape, groups = SHAPES[name]
    n, ch = shape[:2]
    vals = np.random.default_rng(3).standard_normal((n, groups)).astype(np.float32) * 100
    c["x"] = np.broadcast_to(np.repeat(vals, ch // groups, axis=1).reshape((n, ch) + (1,) * (len(shape) - 2)), shape).copy()
    got = native(c, act)
    a, _ = R.act64(torch.from_numpy(c["bias"]).double(), act)
    want = np.broadcast_to(a.numpy().astype(np.float32).reshape((1, ch) + (1,) * (len(shape) - 2)), shape)
    assert np.array_equal(got["out"].cpu().numpy(), want)
    assert torch.isfinite(got["g_x"]).all() and torch.isfinite(got["g_weight"]).all()
    _, stats = gn.norm_forward(dev(c["x"]), groups, dev(c["weight"]), dev(c["bias"]), 1e-5, act)
    assert np.array_equal(stats[:, 0].cpu().numpy(), vals.reshape(-1).astype(np.float64))          # mu exactly
    assert R.stats_worst(stats[:, 1], np.full(n * groups, 1.0 / np.sqrt(np.float64(1e-5)))) <= 1.0


@pytest.mark.parametrize("act", R.ACTIVATIONS)
@pytest.mark.parametrize("name", ["gn8", "chunk+1"])
def test_zero_weight_and_bias_the_zero_module_state(name, act):
    c = dict(case_of(name, True, True))
    c["weight"], c["bias"] = np.zeros_like(c["weight"]), np.zeros_like(c["bias"])
    got = native(c, act)
    if act in ("none", "silu"):
        assert torch.equal(got["out"], dev(c["residual"]))
    assert torch.equal(got["g_x"], torch.zeros_like(got["g_x"]))
    want = R.statement(c["x"], c["groups"], c["weight"], c["bias"], 1e-5, act, c["residual"], c["g_out"])
    assert_rule(got, want, ("zero module", name, act), names=("out", "g_weight", "g_bias"))
    if act in ("none", "silu", "gelu"):
        assert np.abs(want["g_weight"]).max() > 0                                   # the block can still learn


# ---- structure ---------------------------------------------------------------------------------------------------------------------

def guarded(n, dtype, shift=0):
    """n NaNs between two runs of GUARD sentinels; the body starts `shift` elements past a 16-byte boundary."""
    buf = torch.full((n + 2 * GUARD + shift,), SENTINEL, dtype=dtype, device=DEV)
    buf[GUARD + shift:GUARD + shift + n] = float("nan")
    assert (buf.data_ptr() + GUARD * buf.element_size()) % 16 == 0
    return buf


def assert_owned(buf, n, shift, what):
    b = buf.cpu()
    body = b[GUARD + shift:GUARD + shift + n]
    assert int(torch.isnan(body).sum()) == 0, (what, "elements not written")
    assert bool((b[:GUARD + shift] == SENTINEL).all()) and bool((b[GUARD + shift + n:] == SENTINEL).all()), (what, "a sentinel was overwritten")


def abi(c, act, needs=(True, True, True), shift=0, eps=1e-5):
    """One forward and one backward call of the C ABI into guarded buffers.  Inputs and float32 outputs start `shift` floats past
    a 16-byte boundary (shift 1: the element-by-element path).  Returns (got, bufs)."""
    shape = c["x"].shape
    n, ch, s = shape[0], shape[1], int(np.prod(shape[2:]))
    groups, numel = c["groups"], int(np.prod(shape))

    def placed(a):
        if a is None:
            return None
        buf = torch.zeros(a.size + 4 + shift, device=DEV)
        off = (-(buf.data_ptr() // 4) % 4) + shift
        buf[off:off + a.size] = dev(a).reshape(-1)
        return buf[off:off + a.size]
    x, w, b, res, g = (placed(c[k]) for k in ("x", "weight", "bias", "residual", "g_out"))
    affine = w is not None
    nd = gn.scratch_doubles(n, ch, s)
    sizes = {"out": (numel, torch.float32, True), "stats": (2 * n * groups, torch.float64, True), "scratch_f": (nd, torch.float64, True),
             "scratch_b": (nd, torch.float64, True), "g_x": (numel, torch.float32, needs[0]),
             "g_weight": (ch, torch.float32, needs[1] and affine), "g_bias": (ch, torch.float32, needs[2] and affine)}
    bufs, got = {}, {}
    for k, (cnt, dtype, need) in sizes.items():
        sh = shift if dtype == torch.float32 else 0
        got[k] = None
        if need:
            bufs[k] = (guarded(cnt, dtype, sh), cnt, sh)
            got[k] = bufs[k][0][GUARD + sh:GUARD + sh + cnt]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())                    # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    lib, a = _lib.lib(), gn.ACTIVATIONS[act]
    _lib.check(lib.s360_group_norm_forward(p(x), p(w), p(b), p(res), n, ch, s, groups, C.byref(C.c_double(eps)), a, p(got["scratch_f"]), p(got["stats"]),
                                           p(got["out"]), stream), "forward")
    _lib.check(lib.s360_group_norm_backward(p(x), p(w), p(b), p(got["stats"]), p(g), n, ch, s, groups, C.byref(C.c_double(eps)), a, p(got["scratch_b"]),
                                            p(got["g_x"]), p(got["g_weight"]), p(got["g_bias"]), stream), "backward")
    torch.cuda.synchronize()
    got["out"], got["g_x"] = got["out"].view(shape), None if got["g_x"] is None else got["g_x"].view(shape)
    return got, bufs


STRUCTURE = [("gn8", "silu", True, True), ("odd", "gelu", True, False), ("2chunk+5", "relu", True, True), ("inst", "relu", False, False),
             ("m4", "none", True, True)]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name,act,affine,residual", STRUCTURE)
def test_the_python_layer_gives_the_c_abi_s_bits_and_the_kernels_write_all_they_own_and_nothing_else(name, act, affine, residual, shift):
    c = case_of(name, affine, residual)
    py = native(c, act)
    got, bufs = abi(c, act, shift=shift)
    for k, (buf, cnt, sh) in bufs.items():
        if not k.startswith("scratch"):                                             # scratch: sentinels only (its contents are the kernels')
            assert_owned(buf, cnt, sh, (name, k))
        else:
            b = buf.cpu()
            assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + cnt:] == SENTINEL).all()), (name, k)
    for k in NAMES:
        assert (py[k] is None and got[k] is None) or torch.equal(py[k], got[k]), k  # aligned or not: the same bits
    assert_rule(got, want_of(name, act, affine, residual), (name, act, "abi", shift))


@pytest.mark.parametrize("needs", [n for n in itertools.product([False, True], repeat=3) if any(n) and not all(n)])
@pytest.mark.parametrize("name,act,affine,residual", STRUCTURE[:3])
def test_a_null_gradient_leaves_the_others_fully_written(name, act, affine, residual, needs):
    c = case_of(name, affine, residual)
    full, _ = abi(c, act)
    got, bufs = abi(c, act, needs=needs)
    assert {k for k in bufs if k.startswith("g_")} == {k for k, need in zip(NAMES[1:], needs) if need}
    for k, (buf, cnt, sh) in bufs.items():
        if not k.startswith("scratch"):
            assert_owned(buf, cnt, sh, (name, needs, k))
            assert torch.equal(got[k].reshape(-1), full[k].reshape(-1)), k
    x, w, b, g = (dev(c[k]) for k in ("x", "weight", "bias", "g_out"))
    _, stats = gn.norm_forward(x, c["groups"], w, b, 1e-5, act, dev(c["residual"]))
    low = gn.norm_backward(x, c["groups"], w, b, stats, g, 1e-5, act, needs=needs)
    for need, t, k in zip(needs, low, NAMES[1:]):
        assert (t is None) if not need else torch.equal(t, full[k].view(t.shape)), k


@pytest.mark.parametrize("name,act,affine,residual", STRUCTURE[:3])
def test_forward_and_backward_are_deterministic_over_runs_and_streams(name, act, affine, residual):
    c = case_of(name, affine, residual)
    first = native(c, act)
    again = native(c, act)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = native(c, act)
    side.synchronize()
    for k in NAMES:
        assert torch.equal(first[k], again[k]) and torch.equal(first[k], other[k]), k


@pytest.mark.parametrize("act", R.ACTIVATIONS)
def test_a_zero_output_gradient_gives_exact_zeros(act):
    c = dict(case_of("2chunk+5", True, True))
    c["g_out"] = np.zeros_like(c["g_out"])
    got = native(c, act)
    for k in NAMES[1:]:
        assert torch.equal(got[k], torch.zeros_like(got[k])), k


def test_no_host_synchronisation():
    c = case_of("gn8", True, True)
    want = native(c, "silu")
    x, w, b, res = (dev(c[k]).requires_grad_(True) for k in ("x", "weight", "bias", "residual"))
    g = dev(c["g_out"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = gn.group_norm_act(x, c["groups"], w, b, 1e-5, "silu", res)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(out, want["out"]) and torch.equal(x.grad, want["g_x"]) and torch.equal(w.grad, want["g_weight"])


def test_needs_input_grad_is_honoured_and_errors_on_the_gpu():
    c = case_of("gn8", True, True)
    full = native(c, "gelu")
    x, w, b, res = (dev(c[k]) for k in ("x", "weight", "bias", "residual"))
    w = w.requires_grad_(True)
    calls = []
    backward = gn.norm_backward
    try:
        gn.norm_backward = lambda *a, **k: calls.append(k["needs"]) or backward(*a, **k)
        gn.group_norm_act(x, c["groups"], w, b, 1e-5, "gelu", res).backward(dev(c["g_out"]))
    finally:
        gn.norm_backward = backward
    assert calls == [(False, True, False)] and torch.equal(w.grad, full["g_weight"])
    with pytest.raises(ValueError, match="contiguous float32 GPU"):
        gn.group_norm_act(x.half(), c["groups"])
    with pytest.raises(ValueError, match="contiguous float32 GPU"):
        gn.group_norm_act(x, c["groups"], w.detach().cpu(), b.cpu())
    with pytest.raises(ValueError, match="contiguous float32 GPU"):
        gn.group_norm_act(x.transpose(2, 3), c["groups"])
    assert torch.equal(gn.instance_norm_act(x, "relu"), gn.group_norm_act(x, x.shape[1], activation="relu"))


# ---- memory ------------------------------------------------------------------------------------------------------------------------

def test_the_forward_keeps_only_its_output():
    """[2, 32, 256, 256]: out is 16.8 MB.  With x requiring grad, the bytes still allocated after the forward, out alive, exceed
    those before by at most out + 1 MB (statistics and scratch are small); torch's lines keep the norm's output too."""
    x = torch.randn(2, 32, 256, 256, device=DEV).requires_grad_(True)
    w, b = torch.randn(32, device=DEV).requires_grad_(True), torch.randn(32, device=DEV).requires_grad_(True)

    def kept(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated(DEV)
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated(DEV) - before, out

    kept(lambda: gn.group_norm_act(x, 8, w, b, 1e-5, "silu"))                       # warm-up
    ours, out = kept(lambda: gn.group_norm_act(x, 8, w, b, 1e-5, "silu"))
    nbytes = out.numel() * 4
    theirs, ref = kept(lambda: F.silu(F.group_norm(x, 8, w, b, 1e-5)))
    print(f"kept after the forward: native {ours / nbytes:.3f} out, torch {theirs / nbytes:.3f} out")
    assert ours <= nbytes + (1 << 20)
    assert theirs >= 2 * nbytes
    assert (out - ref).abs().max().item() < 1e-4


# ---- the seam on the device ----------------------------------------------------------------------------------------------------------

MODULES = (plugin.GROUP_NORM_UNET_MODULE, plugin.COST_VOLUME_MODULE, plugin.GROUP_NORM_BACKBONE_MODULE)


@pytest.fixture
def standin():
    assert not any(m in sys.modules for m in MODULES)
    mods = R.standin_modules(*MODULES)
    sys.modules.update(mods)
    try:
        yield [mods[m] for m in MODULES]
    finally:
        plugin.uninstall()
        for m in MODULES:
            del sys.modules[m]


class Conv64(nn.Module):
    """A convolution done in float64 torch on the host, rounded once to float32: the same bits on every call and both sides."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv.double().cpu()

    def forward(self, x):
        return self.conv(x.double().cpu()).float().to(x.device)


def with_float64_convolutions(module):
    for parent in list(module.modules()):
        for key, child in list(parent._modules.items()):
            if isinstance(child, (nn.Conv1d, nn.Conv2d)):
                parent._modules[key] = Conv64(child)
    return module


@pytest.mark.parametrize("case", sorted(BLOCK_SEEDS))
def test_seam_runs_the_kernel_gives_the_direct_api_s_bits_and_holds_the_rule(standin, monkeypatch, case):
    unet, _, backbone = standin
    g = recorded(case)
    module = {"resblock_same": lambda: unet.ResBlock(32, 32), "resblock_proj": lambda: unet.ResBlock(64, 32),
              "attention": lambda: unet.AttentionBlock(32, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True),
              "residual": lambda: backbone.ResidualBlock(64, 96, stride=2)}[case]()
    module = with_float64_convolutions(R.randomise(module, BLOCK_SEEDS[case]).to(DEV))
    calls = []
    kernel = gn.group_norm_act

    def recording(x, num_groups, weight=None, bias=None, eps=1e-5, activation="none", residual=None):
        out = kernel(x, num_groups, weight, bias, eps, activation, residual)
        rec = dict(x=x.detach(), groups=num_groups, weight=weight, bias=bias, eps=eps, act=activation, out=out.detach(),
                   residual=None if residual is None else residual.detach())
        if x.requires_grad:
            x.register_hook(lambda t, rec=rec: rec.__setitem__("g_x", t.detach().clone()))
            out.register_hook(lambda t, rec=rec: rec.__setitem__("g_out", t.detach().clone()))
        calls.append(rec)
        return out

    monkeypatch.setattr(gn, "group_norm_act", recording)
    plugin.install_group_norm()
    x = dev(g["x"]).requires_grad_(True)
    out = module._forward(x) if case != "residual" else module(x)
    out.backward(dev(g["g"]))
    expected = {"resblock_same": [("silu", False), ("silu", True)], "resblock_proj": [("silu", False), ("silu", True)],
                "attention": [("none", True)], "residual": [("relu", False), ("relu", False)]}[case]
    assert [(c["act"], c["residual"] is not None) for c in calls] == expected      # the kernel ran, once per norm stage
    # the direct API's bits: the same stages by hand
    monkeypatch.setattr(gn, "group_norm_act", kernel)
    with torch.no_grad():
        xd = x.detach()
        if case.startswith("resblock"):
            n1, n2 = module.in_layers[1], module.out_layers[1]
            h = gn.group_norm_act(module.in_layers[0](xd), n1.num_groups, n1.weight, n1.bias, n1.eps, "silu")
            direct = gn.group_norm_act(module.out_layers[0](h), n2.num_groups, n2.weight, n2.bias, n2.eps, "silu", module.skip_connection(xd).contiguous())
        elif case == "attention":
            flat = xd.reshape(2, 32, -1)
            h = module.proj_out(module.attention(module.qkv(flat)))
            direct = gn.group_norm_act(h, module.norm.num_groups, module.norm.weight, module.norm.bias, module.norm.eps, "none", flat).reshape(xd.shape)
        else:
            y = gn.instance_norm_act(module.conv1(xd), "relu")
            y = gn.instance_norm_act(module.conv2(y), "relu")
            direct = F.relu(module.downsample(xd) + y)
    assert torch.equal(out.detach(), direct)
    # every norm stage holds the rule against the float64 statement on the tensors it was given
    for i, c in enumerate(calls):
        want = R.statement(c["x"], c["groups"], c["weight"], c["bias"], c["eps"], c["act"], c["residual"], c["g_out"])
        assert c["act"] != "relu" or R.relu_is_unambiguous(want)
        assert_rule({"out": c["out"], "g_x": c["g_x"]}, want, (case, "stage", i), names=("out", "g_x"))
    # the block as a whole against the recorded float64 reference (float32 activations between float64 convolutions)
    tol = 64 * 2.0 ** -24
    assert np.abs(out.detach().cpu().numpy() - g["out64"]).max() <= tol * np.abs(g["out64"]).max()
    assert np.abs(x.grad.cpu().numpy() - g["gx64"]).max() <= tol * np.abs(g["gx64"]).max()


def test_fused_module_and_fuse_pairs_run_the_kernel_on_the_device(monkeypatch):
    net = nn.Sequential(nn.GroupNorm(4, 16), nn.GELU(), nn.GroupNorm(8, 16), nn.SiLU()).to(DEV)
    with torch.no_grad():
        for p in net.parameters():
            p.normal_(0.5, 0.5)
    x = torch.randn(2, 16, 7, 5, device=DEV)
    calls = []
    kernel = gn.group_norm_act
    monkeypatch.setattr(gn, "group_norm_act", lambda *a, **k: calls.append(1) or kernel(*a, **k))
    gn.fuse_pairs(net)
    got = net(x)
    h = kernel(x, 4, net[0].weight, net[0].bias, net[0].eps, "gelu")
    assert len(calls) == 2 and torch.equal(got, kernel(h, 8, net[2].weight, net[2].bias, net[2].eps, "silu"))
    assert net.double()(x.double()).dtype == torch.float64 and len(calls) == 2     # float64: F.group_norm and torch's activation
