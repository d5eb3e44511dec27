"""The float64 statement of tests/group_norm_reference.py against the reference's recorded outputs (tests/golden/group_norm.npz,
made by tests/golden/make_golden_group_norm.py), the stand-in classes against the recorded blocks, fuse_pairs, the C ABI's
argument checks and the Python layer's refusals.  No GPU.  The GPU half is tests/test_gpu_group_norm.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

import group_norm_reference as R
from splatter360_amd import _lib, group_norm as gn

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = np.load(ROOT / "tests" / "golden" / "group_norm.npz")
PAIRS = {"gn8_silu": ((2, 32, 6, 10), 8, "silu"), "gn4_silu": ((1, 36, 5, 7), 4, "silu"), "gn4_gelu": ((2, 32, 4, 6), 4, "gelu"),
         "in_relu": ((3, 16, 5, 9), 16, "relu")}
BLOCK_SEEDS = {"resblock_same": 4, "resblock_proj": 5, "attention": 6, "residual": 7}       # the maker's randomise seeds
NAMES = ("s360_group_norm_scratch_doubles", "s360_group_norm_forward", "s360_group_norm_backward")


def recorded(case):
    """x, g float32; out64, gx64; out32, gx32 rebuilt from their recorded distance in float32 steps."""
    def steps(want64, d):
        i = want64.astype(np.float32).view(np.int32).astype(np.int64)
        key = np.where(i < 0, -(i & 0x7fffffff), i) + d
        return np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32).view(np.float32)
    g = {k[len(case) + 1:]: GOLDEN[k] for k in GOLDEN.files if k.startswith(case + "_")}
    g["x"], g["g"] = (g["x"].astype(np.float32) / 64.0), (g["g"].astype(np.float32) / 64.0)
    g["out32"], g["gx32"] = steps(g["out64"], g["out32d"]), steps(g["gx64"], g["gx32d"])
    return g


def build_block(case):
    """The stand-in of a recorded block with the maker's parameters, and how to call it."""
    seed = BLOCK_SEEDS[case]
    if case == "resblock_same":
        return R.randomise(R.StandinResBlock(32, 32), seed), lambda m, t: m._forward(t)
    if case == "resblock_proj":
        return R.randomise(R.StandinResBlock(64, 32), seed), lambda m, t: m._forward(t)
    if case == "attention":
        return R.randomise(R.StandinAttentionBlock(32, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True), seed), \
            lambda m, t: m._forward(t)
    return R.randomise(R.StandinResidualBlock(64, 96, stride=2), seed), lambda m, t: m(t)


def test_the_golden_file_holds_the_cases_the_tests_need():
    assert (ROOT / "tests" / "golden" / "group_norm.npz").stat().st_size < 1 << 20
    for case, (shape, groups, _) in PAIRS.items():
        g = recorded(case)
        assert g["x"].shape == shape and g["out64"].dtype == np.float64 and g["gx64"].shape == shape and int(g["groups"]) == groups
        if case != "in_relu":                                                       # randomised, not the zero initialisation
            assert np.abs(g["p_0.weight"]).min() > 0 and np.abs(g["p_0.bias"]).max() > 0
    for case in BLOCK_SEEDS:
        g = recorded(case)
        assert g["out64"].shape == g["g"].shape and g["gx64"].shape == g["x"].shape
        assert all(np.abs(v).max() > 0 for k, v in g.items() if k.startswith("p_"))


@pytest.mark.parametrize("case", sorted(PAIRS))
def test_statement_is_the_reference_at_float64_and_within_a_few_steps_at_float32(case):
    shape, groups, act = PAIRS[case]
    g = recorded(case)
    want = R.statement(g["x"], groups, g.get("p_0.weight"), g.get("p_0.bias"), 1e-5, act, None, g["g"])
    for name, ref in (("out", g["out64"]), ("g_x", g["gx64"])):
        assert np.abs(want[name] - ref).max() <= 1e-12 * np.abs(ref).max(), (case, name)
    # torch's float32 lines round about ten times per element and sum a slab in float32: 16 float32 half-steps of the largest scale
    for name, scale, got in (("out", want["A"], g["out32"]), ("g_x", want["gx_scale"], g["gx32"])):
        assert np.abs(got.astype(np.float64) - want[name]).max() <= 16 * 2.0 ** -24 * max(scale.max(), np.abs(want[name]).max()), (case, name)
    if act == "relu":
        assert R.relu_is_unambiguous(want)


@pytest.mark.parametrize("case", sorted(BLOCK_SEEDS))
def test_stand_in_blocks_reproduce_the_recorded_blocks(case):
    g = recorded(case)
    module, call = build_block(case)
    for key, p in module.state_dict().items():
        if p.dim() == 1:
            assert np.array_equal(p.numpy(), g[f"p_{key}"]), key                    # the maker's parameters, to the bit
    x32 = torch.from_numpy(g["x"]).requires_grad_(True)
    out32 = call(module, x32)
    out32.backward(torch.from_numpy(g["g"]))
    tol = 64 * 2.0 ** -24                                                           # convolutions of up to 576 float32 terms
    assert np.abs(out32.detach().numpy() - g["out64"]).max() <= tol * np.abs(g["out64"]).max()
    assert np.abs(x32.grad.numpy() - g["gx64"]).max() <= tol * np.abs(g["gx64"]).max()
    module = module.double()
    for m in module.modules():
        if isinstance(m, R.GroupNorm8):
            m.forward = types_method(nn.GroupNorm.forward, m)                       # as the maker: no cast to float32 in the float64 run
    x64 = torch.from_numpy(g["x"]).double().requires_grad_(True)
    out64 = call(module, x64)
    out64.backward(torch.from_numpy(g["g"]).double())
    assert np.abs(out64.detach().numpy() - g["out64"]).max() <= 1e-12 * np.abs(g["out64"]).max()
    assert np.abs(x64.grad.numpy() - g["gx64"]).max() <= 1e-12 * np.abs(g["gx64"]).max()


def types_method(fn, obj):
    import types
    return types.MethodType(fn, obj)


@pytest.mark.parametrize("act", R.ACTIVATIONS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_statement_is_torch_s_float64_autograd(act, affine, residual):
    c = R.make_case((2, 12, 3, 5), 3, affine, residual, seed=3)
    want = R.statement(c["x"], 3, c["weight"], c["bias"], 1e-5, act, c["residual"], c["g_out"])
    out, gx, gw, gb = R.torch_lines(c["x"], 3, c["weight"], c["bias"], 1e-5, act, c["residual"], c["g_out"], dtype=torch.float64)
    pairs = [("out", out), ("g_x", gx)] + ([("g_weight", gw), ("g_bias", gb)] if affine else [])
    for name, ref in pairs:
        assert np.abs(want[name] - ref.numpy()).max() <= 1e-13 * max(np.abs(ref.numpy()).max(), 1.0), name
    assert (want["A"] >= 0).all() and (want["gx_scale"] >= np.abs(want["g_x"]) * (1 - 1e-12)).all()
    assert (want["gw_scale"] >= np.abs(want["g_weight"]) * (1 - 1e-12)).all()


def test_lattice_is_integer_arithmetic_and_exact():
    a = R.lattice((3, 5, 7), 2)
    assert a.dtype == np.float32 and np.array_equal(a * 64, np.round(a * 64)) and np.abs(a).max() <= 15 / 64
    assert np.array_equal(a, R.lattice((3, 5, 7), 2)) and not np.array_equal(a, R.lattice((3, 5, 7), 3))


# ---- fuse_pairs -------------------------------------------------------------------------------------------------------------------

def tree():
    """Pairs (GroupNorm8 + SiLU, GroupNorm + GELU, GroupNorm + ReLU), non-pairs (tanh-GELU, norm + conv, norm + Sigmoid) and a norm
    at the end of a Sequential."""
    torch.manual_seed(0)
    net = nn.Sequential(
        nn.Conv2d(3, 16, 3, 1, 1), nn.GroupNorm(8, 16), nn.GELU(),
        nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), R.normalization(16), nn.SiLU(), nn.Conv2d(16, 16, 1), nn.GroupNorm(4, 16), nn.ReLU()),
        nn.Sequential(nn.GroupNorm(2, 16), nn.GELU(approximate="tanh"), nn.GroupNorm(2, 16), nn.Conv2d(16, 16, 1), nn.GroupNorm(2, 16), nn.Sigmoid()),
        nn.Sequential(nn.Conv2d(16, 8, 1), nn.GroupNorm(4, 8)))
    for p in net.parameters():
        nn.init.normal_(p, 0.1, 0.5)
    return net


def test_fuse_pairs_keeps_keys_parameters_indices_and_bits():
    plain, fused = tree(), tree()
    params = dict(fused.named_parameters())
    assert gn.fuse_pairs(fused) is fused
    assert list(fused.state_dict()) == list(plain.state_dict())
    assert all(p is params[k] for k, p in fused.named_parameters()) and len(dict(fused.named_parameters())) == len(params)
    kinds = lambda net: [(k, type(m).__name__) for k, m in net.named_modules()]     # noqa: E731
    got = dict(kinds(fused))
    assert [k for k, _ in kinds(fused)] == [k for k, _ in kinds(plain)]               # indices
    assert (got["1"], got["2"], got["3.1"], got["3.2"], got["3.4"], got["3.5"]) == ("FusedGroupNormAct", "Identity") * 3
    assert (fused[1].activation, fused[3][1].activation, fused[3][4].activation) == ("gelu", "silu", "relu")
    assert {k: v for k, v in got.items() if k.startswith("4") or k.startswith("5")} == \
        {k: v for k, v in kinds(plain) if k.startswith("4") or k.startswith("5")}     # non-pairs and the trailing norm: untouched
    x = torch.randn(2, 3, 6, 5)
    assert torch.equal(fused(x), plain(x))                                            # the CPU fallback: torch's own bits
    before = kinds(fused)
    mods = list(fused.modules())
    gn.fuse_pairs(fused)                                                              # idempotent
    assert kinds(fused) == before and all(a is b for a, b in zip(fused.modules(), mods))
    fresh = tree()
    with torch.no_grad():
        for p in fresh.parameters():
            p.add_(1.0)
    fused.load_state_dict(fresh.state_dict())
    assert torch.equal(fused(x), fresh(x)) and not torch.equal(fused(x), plain(x))


def test_fused_module_falls_back_on_cpu_float64_and_strided_inputs_with_autograd():
    m = gn.FusedGroupNormAct(4, 8, activation="silu")
    with torch.no_grad():
        m.weight.normal_()
        m.bias.normal_()
    x = torch.randn(2, 8, 5, 3, requires_grad=True)
    res = torch.randn(2, 8, 5, 3)
    want = res + torch.nn.functional.silu(torch.nn.functional.group_norm(x, 4, m.weight, m.bias, m.eps))
    got = m(x, res)
    assert torch.equal(got, want)
    got.sum().backward()
    assert torch.isfinite(x.grad).all() and m.weight.grad is not None
    assert not gn.supported(x) and not gn.supported(x.double()) and "activation=silu" in repr(m)
    strided = torch.randn(2, 5, 3, 8).permute(0, 3, 1, 2)
    assert torch.equal(m(strided), torch.nn.functional.silu(torch.nn.functional.group_norm(strided, 4, m.weight, m.bias, m.eps)))
    md = gn.FusedGroupNormAct(4, 8, activation="gelu").double()
    assert md(x.detach().double()).dtype == torch.float64
    with pytest.raises(ValueError, match="activations"):
        gn.FusedGroupNormAct(4, 8, activation="tanh")


# ---- the C ABI and the Python layer ----------------------------------------------------------------------------------------------

def test_abi_has_the_group_norm_entry_points_and_they_reject_bad_arguments():
    lib = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\b(int|size_t)\s+{name}\s*\(", header)
    for i, name in enumerate(("NONE", "RELU", "SILU", "GELU")):
        assert re.search(rf"#define\s+S360_GN_ACT_{name}\s+{i}\b", header) and getattr(_lib, f"GN_ACT_{name}") == i
    assert "s360_group_norm.hip" in _lib.SOURCES and (ROOT / "splatter360_amd" / "csrc" / "s360_group_norm.hip").exists()
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25                  # additive: the version stays
    sd = lib.s360_group_norm_scratch_doubles
    assert sd(1, 1, gn.ROW_CHUNK) == 2 and sd(1, 1, gn.ROW_CHUNK + 1) == 4 and sd(2, 3, 2 * gn.ROW_CHUNK + 5) == 36   # ROW_CHUNK is the kernels'
    assert sd(0, 1, 1) == 0 and sd(1, 0, 1) == 0 and sd(1, 1, 0) == 0
    p, q = C.c_void_p(1 << 20), C.c_void_p(1 << 24)                                 # never dereferenced: every call below is refused
    fwd, bwd = lib.s360_group_norm_forward, lib.s360_group_norm_backward
    eps = lambda v: C.byref(C.c_double(v))                                          # noqa: E731  (a host pointer, see the header)
    ok = (2, 8, 35, 4, eps(1e-5), 0)

    def f(x=p, w=p, b=p, res=p, dims=ok, scratch=q, stats=q, out=q):
        return fwd(x, w, b, res, *dims, scratch, stats, out, None)

    def g(x=p, w=p, b=p, stats=q, g_out=q, dims=ok, scratch=q, g_x=q, g_w=q, g_b=q):
        return bwd(x, w, b, stats, g_out, *dims, scratch, g_x, g_w, g_b, None)

    assert f(x=None) == -1 and f(scratch=None) == -1 and f(stats=None) == -1 and f(out=None) == -1
    assert g(x=None) == -1 and g(stats=None) == -1 and g(g_out=None) == -1 and g(scratch=None) == -1
    e = eps(1e-5)
    for dims in ((0, 8, 35, 4, e, 0), (2, 0, 35, 4, e, 0), (2, 8, 0, 4, e, 0), (2, 8, 35, 0, e, 0), (2, 8, 35, -2, e, 0),
                 (2, 8, 35, 3, e, 0),                                                 # channels % groups != 0
                 (2, 8, 35, 4, e, 4), (2, 8, 35, 4, e, -1),                           # unknown activation
                 (2, 8, 35, 4, eps(0.0), 0), (2, 8, 35, 4, eps(-1e-5), 0), (2, 8, 35, 4, eps(float("nan")), 0), (2, 8, 35, 4, None, 0),   # eps <= 0
                 (1 << 15, 1 << 15, 2 * gn.ROW_CHUNK, 1, e, 0),                       # 2^31 workgroups
                 (1 << 16, 1 << 16, 1, 1, e, 0)):
        assert f(dims=dims) == -1 and g(dims=dims) == -1, dims
    assert f(w=None) == -1 and f(b=None) == -1 and g(w=None) == -1 and g(b=None) == -1   # only one of weight and bias
    assert f(out=p) == -1 and g(g_x=p) == -1                                          # out / g_x is x
    assert f(out=C.c_void_p((1 << 20) + 4 * 100)) == -1 and g(g_x=C.c_void_p((1 << 20) - 4 * 100)) == -1   # ... or overlaps it
    assert g(w=None, b=None) == -1                                                    # parameter gradients without parameters
    assert g(g_x=None, g_w=None, g_b=None) == 0                                       # nothing asked for: no GPU work


def test_python_layer_refuses_what_it_cannot_run():
    c = R.make_case((2, 8, 3, 5), 4, seed=1)
    x, w, b = (torch.from_numpy(c[k]) for k in ("x", "weight", "bias"))
    for call in (lambda: gn.group_norm_act(x, 4, w, b), lambda: gn.group_norm_act(x.double(), 4), lambda: gn.instance_norm_act(x),
                 lambda: gn.norm_forward(x, 4), lambda: gn.group_norm_act(x.permute(0, 1, 3, 2), 4)):
        with pytest.raises(ValueError, match="contiguous float32 GPU"):
            call()
    for groups in (3, 0, -1, 16, 2.0, True):
        with pytest.raises(ValueError, match="num_groups"):
            gn.group_norm_act(x, groups)
    with pytest.raises(ValueError, match="together"):
        gn.group_norm_act(x, 4, w, None)
    with pytest.raises(ValueError, match="weight and bias must be"):
        gn.group_norm_act(x, 4, w[:4], b[:4])
    with pytest.raises(ValueError, match="residual"):
        gn.group_norm_act(x, 4, residual=x[:1])
    with pytest.raises(ValueError, match="activations"):
        gn.group_norm_act(x, 4, activation="tanh")
    with pytest.raises(ValueError, match="eps"):
        gn.group_norm_act(x, 4, eps=0.0)
    with pytest.raises(ValueError):
        gn.group_norm_act(x[0, 0, 0], 1)
    assert gn.ROW_CHUNK == 4096 and gn.ACTIVATIONS == {"none": 0, "relu": 1, "silu": 2, "gelu": 3}
    assert gn.activation_of(nn.SiLU()) == "silu" and gn.activation_of(nn.GELU()) == "gelu" and gn.activation_of(nn.ReLU(inplace=True)) == "relu"
    assert gn.activation_of(nn.GELU(approximate="tanh")) is None and gn.activation_of(nn.Tanh()) is None
