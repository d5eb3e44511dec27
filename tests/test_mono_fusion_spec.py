"""The mono-feature fusion on CPU: the project's statement (tests/mono_fusion_reference.py) against the reference's recorded run
(tests/golden/mono_fusion.npz: the reference's own Cube2Equirec and an nn.Sequential of rgbd_fusion's four layers, recorded by
tests/golden/make_golden_mono_fusion.py), what the C ABI refuses before any GPU work, the scratch and chunk helpers, and what the
Python wrappers refuse.  The kernels themselves are held to the statement in tests/test_gpu_mono_fusion.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import mono_fusion_reference as R
from splatter360_amd import _lib, mono_fusion as mf

ROOT = Path(__file__).resolve().parent.parent
GOLD = np.load(ROOT / "tests" / "golden" / "mono_fusion.npz")
KEYS = ("0.weight", "1.weight", "1.bias", "3.weight")
RECORDED = ("out", "g_erp_feat", "g_0.weight", "g_1.weight", "g_1.bias", "g_3.weight")      # R.RESULTS' order


def _steps32(got32, want64):
    def key(a):
        i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return (key(got32) - key(np.asarray(want64).astype(np.float32))).astype(np.int64)


def _case():
    f = lambda k: torch.from_numpy(GOLD[k].astype(np.float32) / 64)
    p = {k: f("p_" + k) + (1.0 if k == "1.weight" else 0.0) for k in KEYS}
    return (f("erp_feat"), f("mono_cube"), torch.from_numpy(GOLD["grid"]), p["0.weight"], p["1.weight"], p["1.bias"], p["3.weight"]), f("g")


def test_fixture_is_the_configuration_the_issue_names_and_data_only():
    assert tuple(GOLD["cfg"]) == (2, 16, 24, 4, 8, 16)
    assert (ROOT / "tests" / "golden" / "mono_fusion.npz").stat().st_size < 128 * 1024
    assert all(GOLD[k].dtype.kind in "iuf" for k in GOLD.files)
    assert np.array_equal(GOLD["grid"], R.grid_of((4, 8, 16)).numpy())


def test_statement_reproduces_the_recorded_float64_run():
    tensors, g = _case()
    got = R.gradients(R.statement, tensors, g, torch.float64)
    for name, x in zip(RECORDED, got):
        want = GOLD[name + "64"]
        assert x.dtype == torch.float64 and tuple(x.shape) == want.shape, name
        err = np.abs(x.numpy() - want).max()
        assert err <= 1e-12 * max(1.0, np.abs(want).max()), (name, err)


def test_float32_statement_lies_within_the_recorded_float32_distances():
    tensors, g = _case()
    got = R.gradients(lambda *t: R.statement(*t, dtype=torch.float32), tensors, g, torch.float32)
    for name, x in zip(RECORDED, got):
        d = np.abs(_steps32(x.numpy(), GOLD[name + "64"]))
        recorded = np.abs(GOLD[name + "32d"].astype(np.int64))
        print(f"{name}: float32 statement at most {d.max()} float32 steps from the float64 run, the recorded float32 run {recorded.max()}")
        assert d.max() <= recorded.max() + 1, (name, d.max(), recorded.max())


def test_stitch32_is_the_stitch_reference_in_float32_and_close_to_its_float64():
    import stitch_reference as S
    (erp, cube, grid, *_), _ = _case()
    m = R.stitch32(cube, grid).numpy()
    n, cm, fw, _ = cube.shape
    faces = cube.numpy().reshape(n, cm, fw, 6, fw).transpose(0, 3, 1, 2, 4)                 # [N, 6, Cm, fw, fw]
    for b in range(n):
        want = S.forward64(faces[b], grid.numpy())
        assert np.abs(m[b] - want).max() <= 2.0 ** -21 * np.abs(want).max()
    assert np.array_equal(m, R.stitch_lines(cube, grid).numpy())                            # torch's float32 grid_sample, bit for bit


# ---- the ABI, without a GPU --------------------------------------------------------------------------------------------------

class _Args:
    """A valid argument set for both entry points with fake (never dereferenced) 16-byte aligned addresses."""

    def __init__(self):
        self.eps = C.c_double(1e-5)
        self.ptr = {k: 0x10000 * (i + 1) for i, k in enumerate(
            ("erp_feat", "mono_cube", "grid", "w1", "ln_weight", "ln_bias", "w2", "y", "stats", "g_out", "out", "scratch", "g_erp_feat",
             "g_w1", "g_ln_weight", "g_ln_bias", "g_w2"))}
        self.dims = dict(n=1, channels=128, mono_channels=64, face_w=4, equ_h=8, equ_w=16)
        self.scratch_bytes = None
        self.eps_ptr = C.byref(self.eps)

    def forward(self):
        p, d = self.ptr, self.dims
        return _lib.lib().s360_mono_fusion_forward(p["erp_feat"], p["mono_cube"], p["grid"], p["w1"], p["ln_weight"], p["ln_bias"], p["w2"],
                                                   *d.values(), self.eps_ptr, p["out"], p["y"], p["stats"], None)

    def backward(self):
        p, d = self.ptr, self.dims
        need = _lib.lib().s360_mono_fusion_scratch_bytes(d["n"] * d["equ_h"] * d["equ_w"], d["mono_channels"])
        return _lib.lib().s360_mono_fusion_backward(p["erp_feat"], p["mono_cube"], p["grid"], p["w1"], p["ln_weight"], p["ln_bias"], p["w2"],
                                                    p["y"], p["stats"], p["g_out"], *d.values(), self.eps_ptr, p["scratch"],
                                                    need if self.scratch_bytes is None else self.scratch_bytes, p["g_erp_feat"], p["g_w1"],
                                                    p["g_ln_weight"], p["g_ln_bias"], p["g_w2"], None)


BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
FWD_PTRS = ("erp_feat", "mono_cube", "grid", "w1", "ln_weight", "ln_bias", "w2", "out", "y", "stats")
BWD_PTRS = ("erp_feat", "mono_cube", "grid", "w1", "ln_weight", "ln_bias", "w2", "y", "stats", "g_out", "scratch", "g_erp_feat", "g_w1",
            "g_ln_weight", "g_ln_bias", "g_w2")


@pytest.mark.parametrize("which, names", [("forward", FWD_PTRS), ("backward", BWD_PTRS)])
def test_abi_refuses_null_and_misaligned_pointers(which, names):
    for name in names:
        for value in (None, 0x10000 * 40 + 8):
            a = _Args()
            a.ptr[name] = value
            assert getattr(a, which)() == BADARG, (which, name, value)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_abi_refuses_bad_sizes_eps_and_widths(which):
    for key in ("n", "channels", "mono_channels", "face_w", "equ_h", "equ_w"):
        for bad in (0, -3):
            a = _Args()
            a.dims[key] = bad
            assert getattr(a, which)() == BADARG, (key, bad)
    for eps in (0.0, -1e-5, float("nan")):
        a = _Args()
        a.eps_ptr = C.byref(C.c_double(eps))
        assert getattr(a, which)() == BADARG, eps
    a = _Args()
    a.eps_ptr = None
    assert getattr(a, which)() == BADARG
    for key, bad in (("channels", 64), ("channels", 256), ("mono_channels", 32), ("mono_channels", 96), ("mono_channels", 1088), ("mono_channels", 2048)):
        a = _Args()
        a.dims[key] = bad
        assert getattr(a, which)() == UNSUPPORTED, (key, bad)
    # 2^31 or more elements (erp_feat / out; mono_cube), and equ_h equ_w 8 beyond int32
    for dims in (dict(n=4, equ_h=2048, equ_w=2048), dict(n=64, mono_channels=1024, face_w=74), dict(equ_h=16384, equ_w=16384)):
        a = _Args()
        a.dims.update(dims)
        assert getattr(a, which)() == BADARG, dims


def test_abi_refuses_aliased_outputs_and_a_short_scratch():
    for out, other in (("out", "erp_feat"), ("out", "w2"), ("y", "mono_cube"), ("stats", "grid"), ("out", "y"), ("y", "stats"), ("out", "stats")):
        a = _Args()
        a.ptr[out] = a.ptr[other]
        assert a.forward() == BADARG, (out, other)
    outs = ("g_erp_feat", "g_w1", "g_ln_weight", "g_ln_bias", "g_w2", "scratch")
    for i, out in enumerate(outs):
        for other in ("erp_feat", "g_out", "y", "stats", "w1") + outs[i + 1:]:
            a = _Args()
            a.ptr[out] = a.ptr[other]
            assert a.backward() == BADARG, (out, other)
    a = _Args()
    a.scratch_bytes = _lib.lib().s360_mono_fusion_scratch_bytes(128, 64) - 1
    assert a.backward() == WORKSPACE
    a.scratch_bytes = 0
    assert a.backward() == WORKSPACE


def test_scratch_and_chunk_helpers_are_monotone_and_aligned():
    lib = _lib.lib()
    assert lib.s360_mono_fusion_scratch_bytes(0, 64) == 0 and lib.s360_mono_fusion_scratch_bytes(128, 96) == 0
    assert lib.s360_mono_fusion_weight_chunks(0) == 0 and lib.s360_mono_fusion_weight_chunks(-5) == 0
    tokens = sorted({1, 2, 31, 32, 63, 64, 65, 127, 128, 129, 143, 144, 288, 576, 1000, 2047, 2048, 2049, 4096, 4097, 32768, 65536, 65537, 1 << 20})
    for cm in (64, 384, 768, 1024):
        sizes = [mf.scratch_bytes(t, cm) for t in tokens]
        assert all(s > 0 and s % 16 == 0 for s in sizes), cm
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), cm
    assert [mf.scratch_bytes(4096, cm) for cm in (64, 128, 384, 1024)] == sorted(mf.scratch_bytes(4096, cm) for cm in (64, 128, 384, 1024))
    chunks = [mf.weight_chunks(t) for t in tokens]
    assert chunks == sorted(chunks) and chunks[0] == 1 and max(chunks) == 32
    assert [mf.weight_chunks(t) for t in (64, 65, 128, 129, 288, 2048, 2049)] == [1, 2, 2, 3, 5, 32, 32]
    # the declared layout: g_y, the partials, the LayerNorm partials
    for t, cm in ((144, 192), (32768, 384)):
        want = t * 128 * 4 + mf.weight_chunks(t) * 128 * (256 + cm) * 4 + -(-t // 128) * 256 * 8
        assert mf.scratch_bytes(t, cm) == want
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            mf.weight_chunks(bad)
        with pytest.raises(ValueError):
            mf.scratch_bytes(bad, 64)
    with pytest.raises(ValueError):
        mf.scratch_bytes(128, 96)


def test_supported_widths():
    assert all(mf.supported_widths(128, cm) for cm in (64, 128, 384, 768, 1024))
    assert not any(mf.supported_widths(c, cm) for c, cm in ((64, 384), (256, 384), (128, 0), (128, 32), (128, 100), (128, 1088)))


# ---- the Python wrappers ------------------------------------------------------------------------------------------------------

def test_wrappers_refuse_cpu_tensors_with_a_clear_message():
    tensors, g = R.random_case(1, "g0", 64)
    with pytest.raises(RuntimeError, match="GPU only.*no CPU path.*erp_feat"):
        mf.mono_fusion(*tensors)
    with pytest.raises(RuntimeError, match="GPU only"):
        mf.mono_fusion_forward(*tensors)
    with pytest.raises(RuntimeError, match="GPU only"):
        mf.mono_fusion_backward(*tensors, torch.zeros(32, 128), torch.zeros(32, 2, dtype=torch.float64), g)


def test_wrappers_refuse_dtype_widths_and_a_differentiable_mono_cube(monkeypatch):
    """The checks behind the device check, reached on CPU by letting every tensor pass for a GPU tensor: nothing is launched,
    because each call raises before the library is touched."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    tensors, _ = R.random_case(1, "g0", 64)
    erp, cube, grid, w1, lnw, lnb, w2 = tensors
    with pytest.raises(ValueError, match="erp_feat must be float32"):
        mf.mono_fusion(erp.double(), *tensors[1:])
    with pytest.raises(ValueError, match="w1 must be float32"):
        mf.mono_fusion(erp, cube, grid, w1.half(), lnw, lnb, w2)
    with pytest.raises(ValueError, match="unsupported widths C = 128, Cm = 96"):
        mf.mono_fusion(erp, torch.zeros(1, 96, 2, 12), grid, torch.zeros(128, 224), lnw, lnb, w2)
    with pytest.raises(ValueError, match="unsupported widths C = 64"):
        mf.mono_fusion(erp[:, :64], cube, grid, w1, lnw, lnb, w2)
    with pytest.raises(ValueError, match="six faces side by side"):
        mf.mono_fusion(erp, torch.zeros(1, 64, 2, 10), grid, w1, lnw, lnb, w2)
    with pytest.raises(ValueError, match="grid must have shape"):
        mf.mono_fusion(erp, cube, grid[:2], w1, lnw, lnb, w2)
    with pytest.raises(ValueError, match="eps must be a positive number"):
        mf.mono_fusion(*tensors, eps=0.0)
    with pytest.raises(RuntimeError, match="mono_cube requires a gradient"):
        mf.mono_fusion(erp, cube.clone().requires_grad_(True), grid, w1, lnw, lnb, w2)
