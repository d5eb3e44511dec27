"""The fused window attention's CPU-checkable parts: the two statements of tests/window_attention_reference.py against the
reference's recorded outputs and gradients (tests/golden/window_attention.npz, made by tests/golden/make_golden_window_attention.py
from the reference's own functions), the two mask rules, ShiftMask.dense(), the C ABI's two new symbols and the Python layer's
argument errors.  The GPU half is tests/test_gpu_window_attention.py."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import window_attention_reference as R
from splatter360_amd import _lib, window_attention as wa

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("s360_window_attention_forward", "s360_window_attention_backward")
GOLDEN = np.load(ROOT / "tests" / "golden" / "window_attention.npz")
CASES = sorted(k[:-5] for k in GOLDEN.files if k.endswith("_meta"))


def _case(name):
    b, m, h, w, k, shift, full = (int(x) for x in GOLDEN[f"{name}_meta"])
    q, kk, v, g = (torch.from_numpy(GOLDEN[f"{name}_{t}"]) for t in ("q", "k", "v", "g"))
    return (b, m, h, w, k, bool(shift), bool(full)), (q, kk, v, g)


def _rel(got, want):
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


def test_the_golden_file_holds_the_cases_the_tests_need():
    assert set(CASES) == {"self_s0", "self_s1", "m1_s0", "m1_s1", "m3_s0", "m3_s1", "odd_s1", "k1", "full"}
    (_, _, h, w, k, shift, _), _ = _case("odd_s1")
    assert (h // k) % 2 == 1 and (w // k) % 2 == 1 and shift                      # odd windows: shifts 1 and 2
    assert _case("m3_s1")[0][:5] == (1, 3, 6, 8, 2) and _case("k1")[0][4] == 1


@pytest.mark.parametrize("name", CASES)
def test_statement_at_float64_is_the_reference(name):
    """Outputs and the three gradients to 1e-12 of the largest entry, against the reference's float64 run."""
    (b, m, h, w, k, shift, full), (q, kk, v, g) = _case(name)
    got = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, k, shift, h, w, "reference"), q, kk, v, g, torch.float64)
    for t, key in zip(got, ("out64", "gq64", "gk64", "gv64")):
        want = torch.from_numpy(GOLDEN[f"{name}_{key}"])
        assert t.shape == want.shape and _rel(t, want) <= 1e-12, (name, key)


@pytest.mark.parametrize("name", CASES)
def test_reference_lines_are_the_statement_and_the_reference(name):
    """The restated lines: float64 equals the statement to 1e-12; float32 is the reference's float32 run to a few float32
    roundings (the same operations, in a matmul whose summation order may differ)."""
    (b, m, h, w, k, shift, full), (q, kk, v, g) = _case(name)
    mask = R.dense_mask(h, w, k) if k > 1 else None

    def lines(a, bb, cc):
        if full:
            return R.full_lines(a, bb, cc)
        return R.reference_lines(a, bb, cc, k, shift, h, w, mask)

    got64 = R.gradients(lines, q, kk, v, g, torch.float64)
    want64 = R.gradients(lambda a, bb, cc: R.statement(a, bb, cc, k, shift, h, w), q, kk, v, g, torch.float64)
    for t, want in zip(got64, want64):
        assert _rel(t, want) <= 1e-12, name
    got32 = R.gradients(lines, q, kk, v, g)
    for t, key in zip(got32, ("out32", "gq32", "gk32", "gv32")):
        want = torch.from_numpy(GOLDEN[f"{name}_{key}"])
        assert t.dtype == torch.float32 and _rel(t, want) <= 32 * 2.0 ** -24, (name, key)


@pytest.mark.parametrize("name", [c for c in CASES if f"{c}_mask" in GOLDEN.files])
def test_dense_mask_and_shift_mask_are_the_recorded_mask(name):
    (b, m, h, w, k, shift, full), _ = _case(name)
    want = torch.from_numpy(GOLDEN[f"{name}_mask"])
    assert want.dtype == torch.float32 and set(want.unique().tolist()) <= {0.0, -100.0}
    assert torch.equal(R.dense_mask(h, w, k), want)
    wh, ww = h // k, w // k
    handle = wa.ShiftMask(h, w, wh, ww, wh // 2, ww // 2)
    assert torch.equal(handle.dense(), want) and handle.dense() is handle.dense() and handle.matches(h, w, k)
    assert not handle.matches(h, w, k + 1) and handle.num_splits == k
    built = wa.ShiftMask(h, w, wh, ww, wh // 2, ww // 2, build=lambda: want + 0)
    assert torch.equal(built.dense(), want)


def test_mask_rules_agree_at_one_partner_and_differ_at_three_with_shift():
    for name, differs in (("m1_s1", False), ("self_s1", False), ("m3_s0", False), ("m3_s1", True)):
        (b, m, h, w, k, shift, full), (q, kk, v, g) = _case(name)
        ref, ali = (R.statement(q, kk, v, k, shift, h, w, rule) for rule in ("reference", "aligned"))
        if differs:
            assert (ref - ali).abs().max().item() > 0.1, name                       # O(1): the tiled mask hits other keys
            mask = R.dense_mask(h, w, k).double()
            lines = R.reference_lines(q.double(), kk.double(), v.double(), k, shift, h, w, mask, rule="aligned")
            assert _rel(lines, ali) <= 1e-12
        else:
            assert torch.equal(ref, ali), name


def test_abi_has_the_window_attention_entry_points_and_they_reject_bad_arguments():
    lib = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header)
    assert "s360_window_attention.hip" in _lib.SOURCES
    assert (ROOT / "splatter360_amd" / "csrc" / "s360_window_attention.hip").exists()
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25                  # additive: the version stays
    # distinct 16-byte aligned addresses, never dereferenced: every call below is refused
    q, k, v, o, l, g, d, gq, gk, gv = (C.c_void_p(4096 * (i + 1)) for i in range(10))
    fwd, bwd = lib.s360_window_attention_forward, lib.s360_window_attention_backward
    ok = (2, 0, 8, 16, 128, 2, 1, 0)
    assert fwd(None, k, v, *ok, o, l, None) == -1 and fwd(q, k, v, *ok, None, l, None) == -1 and fwd(q, k, v, *ok, o, None, None) == -1
    for dims in ((0, 0, 8, 16, 128, 2, 1, 0), (2, -1, 8, 16, 128, 2, 1, 0), (2, 0, 0, 16, 128, 2, 1, 0), (2, 0, 8, 16, 128, 0, 1, 0),
                 (2, 0, 8, 16, 128, 3, 1, 0), (2, 0, 8, 16, 128, 2, 1, 2)):
        assert fwd(q, k, v, *dims, o, l, None) == -1, dims
    assert fwd(C.c_void_p(4100), k, v, *ok, o, l, None) == -1                        # not 16-byte aligned
    for c in (16, 48, 160, 256):
        assert fwd(q, k, v, 2, 0, 8, 16, c, 2, 1, 0, o, l, None) == -4, c            # S360_E_UNSUPPORTED
    assert bwd(q, k, v, None, g, *ok, d, gq, gk, gv, None) == -1 and bwd(q, k, v, l, g, *ok, None, gq, gk, gv, None) == -1
    assert bwd(q, k, v, l, g, *ok, d, None, None, None, None) == 0                   # nothing asked for: no GPU work


def test_python_layer_refuses_what_it_cannot_run():
    q, k, v, g = R.random_case(2, 0, 4, 8, c=32, seed=1)
    opts = dict(height=4, width=8, num_splits=2)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.window_attention(q, k, v, **opts)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.full_attention(q, k, v)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.attention_forward(q, k, v, **opts)
    with pytest.raises(RuntimeError, match="GPU only"):
        wa.window_attention(q.double(), k.double(), v.double(), **opts)
    with pytest.raises(ValueError, match="mask rule"):
        wa.window_attention(q, k, v, mask_rule="tiled", **opts)
    with pytest.raises(ValueError, match="num_splits"):
        wa.window_attention(q, k, v, height=4, width=8, num_splits=3)
    with pytest.raises(ValueError, match="token count"):
        wa.window_attention(q, k, v, height=4, width=7, num_splits=1)
    with pytest.raises(ValueError, match="channels"):
        wa.window_attention(q[..., :16], k[..., :16], v[..., :16], **opts)
    big = torch.zeros(1, 32, 160)
    with pytest.raises(ValueError, match="channels"):
        wa.window_attention(big, big, big, **opts)
    with pytest.raises(ValueError):
        wa.window_attention(q[0], k, v, **opts)
    with pytest.raises(ValueError, match="one shape"):
        wa.window_attention(q, k, v[:, :16], **opts)
    with pytest.raises(ValueError, match="does not match"):
        wa.window_attention(q, k[:1], v[:1], **opts)
    with pytest.raises(ValueError, match="Lq == Lk"):
        wa.full_attention(q, k[:, :16], v[:, :16])
    assert wa.MASK_RULES == {"reference": 0, "aligned": 1}

