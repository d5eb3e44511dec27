"""The numpy statement of the depth-smoothness loss (tests/depth_smooth_reference.py) against the reference's own LossDepth,
recorded on CPU in tests/golden/depth_smooth.npz (tests/golden/make_golden_depth_smooth.py), and the library's side of the
contract: exports, header, ABI version, source list.

Bars: loss within 1e-5 relative, gradient within 1e-5 A per pixel (A: the statement's sum of the absolute contributions) — the
project's bar for a float32 torch path; the gradient is exactly 0 where A = 0."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import depth_smooth_reference as R
from splatter360_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
G = np.load(ROOT / "tests" / "golden" / "depth_smooth.npz")
CASES = ("s2657_vn1", "s2657_vn6", "s1133_vn1")


def _inputs(case):
    near, far = G[f"{case}_near"], G[f"{case}_far"]
    return G[f"{case}_depth"], torch.from_numpy(near).log().numpy(), torch.from_numpy(far).log().numpy(), G[f"{case}_image"]


def test_fixture_holds_the_edge_cases():
    assert {G[f"{c}_depth"].shape for c in CASES} == {(2, 6, 5, 7), (1, 1, 3, 3)}
    assert G["s2657_vn1_near"].shape == (2, 1) and G["s2657_vn6_near"].shape == (2, 6)
    for case in CASES:
        d, ln, lf, _ = _inputs(case)
        per = d.shape[1] // ln.shape[1]
        lo, hi = np.repeat(ln, per, 1)[:, :, None, None], np.repeat(lf, per, 1)[:, :, None, None]
        assert (d == hi).any() and (d == lo).any() and (d > hi).any() and (d < lo).any()
        assert (np.diff(d, axis=-1) == 0).any() and (np.diff(d, axis=-2) == 0).any()


@pytest.mark.parametrize("mode,second,sigma", R.MODES)
@pytest.mark.parametrize("case", CASES)
def test_statement_matches_the_reference(case, mode, second, sigma):
    d, ln, lf, image = _inputs(case)
    s = R.statement(d, ln, lf, image, sigma, second)
    want, want_g = float(G[f"{case}_{mode}_loss"]), G[f"{case}_{mode}_grad"].astype(np.float64)
    assert s["loss"].dtype == np.float32 and s["grad"].dtype == np.float32 and s["grad"].shape == d.shape
    assert abs(float(s["loss"]) - want) <= 1e-5 * abs(want), (float(s["loss"]), want)
    err, a = np.abs(s["grad"].astype(np.float64) - want_g), s["A"]
    print(case, mode, "loss rel", abs(float(s["loss"]) - want) / abs(want), "grad / A", (err[a > 0] / a[a > 0]).max())
    assert (err <= 1e-5 * a).all()
    assert (a == 0).any() and (s["grad"][a == 0] == 0).all() and (want_g[a == 0] == 0).all()
    # the weight is a plain multiply on the result
    assert np.float32(0.25) * G[f"{case}_{mode}_loss"] == G[f"{case}_{mode}_loss_w025"]
    assert abs(float(R.statement(d, ln, lf, image, sigma, second, g=0.25)["grad64"].sum()) - 0.25 * float(s["grad64"].sum())) <= 1e-12


def test_entry_points_are_exported_declared_and_built_from_the_new_source():
    for name in ("s360_depth_smooth_forward", "s360_depth_smooth_backward"):
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+s360_depth_smooth_forward\s*\(", header) and re.search(r"\bint\s+s360_depth_smooth_backward\s*\(", header)
    assert _lib.ABI_VERSION == 25 and "#define S360_ABI_VERSION 25" in (ROOT / "include" / "s360.h").read_text()
    assert "s360_depth_smooth.hip" in _lib.SOURCES and (ROOT / "splatter360_amd" / "csrc" / "s360_depth_smooth.hip").is_file()


def test_bad_arguments_are_rejected_before_any_gpu_work():
    import ctypes as C
    l = _lib.lib()
    n = C.c_size_t(0)
    one = C.c_void_p(16)                                          # a non-null pointer that is never dereferenced: every call below fails first

    def fwd(b=1, v=6, vn=1, c=3, h=8, w=8, flags=0, depth=None, ws=None, nbytes=n):
        return l.s360_depth_smooth_forward(depth, None, None, None, b, v, vn, c, h, w, C.c_float(2.0), flags, None, ws,
                                           C.byref(nbytes) if nbytes is not None else None, None)

    assert fwd() == 0 and n.value == 6 * 16                       # the size query: one double pair per 32 x 64 tile
    assert fwd(h=33, w=65) == 0 and n.value == 6 * 4 * 16
    assert fwd(vn=4) == -1 and fwd(vn=0) == -1                    # bound_views does not divide views
    assert fwd(h=1) == -1 and fwd(w=1) == -1 and fwd(h=2, flags=1) == -1 and fwd(w=2, flags=1) == -1 and fwd(h=2, w=2) == 0
    assert fwd(c=0, flags=2) == -1 and fwd(c=0, flags=0) == 0 and fwd(flags=4) == -1
    assert fwd(nbytes=None) == -1
    assert fwd(ws=one) == -1                                      # null depth / bounds / loss with a workspace
    assert l.s360_depth_smooth_backward(None, None, None, None, 1, 6, 1, 3, 8, 8, C.c_float(2.0), 0, None, None, None) == -1
    assert l.s360_depth_smooth_backward(one, one, one, None, 1, 6, 1, 3, 8, 8, C.c_float(2.0), 2, one, one, None) == -1   # bilateral, no image
    assert l.s360_depth_smooth_backward(one, one, one, one, 1, 6, 4, 3, 8, 8, C.c_float(2.0), 0, one, one, None) == -1


def test_python_layer_refuses_cpu_tensors_and_bad_shapes_without_a_gpu():
    from splatter360_amd import depth_smooth
    d, nf = torch.zeros(1, 2, 4, 4), torch.ones(1, 1)
    with pytest.raises(RuntimeError):
        depth_smooth.depth_smoothness_loss(d, nf, nf)
    with pytest.raises(ValueError):
        depth_smooth.depth_smoothness_loss(d, nf, nf, sigma_image=2.0)
