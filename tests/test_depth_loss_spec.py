"""The numpy statement of the context-depth loss (tests/depth_loss_reference.py) against the reference's own erode and
compute_l1_sphere_loss, recorded on CPU in tests/golden/depth_loss.npz (tests/golden/make_golden_depth_loss.py).

Bars: erode bit-exact (NaN where the reference has NaN), loss and gradients within 1e-6 relative."""
from pathlib import Path

import numpy as np
import pytest

import depth_loss_reference as R

G = np.load(Path(__file__).resolve().parent / "golden" / "depth_loss.npz")


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a), np.nan_to_num(b))


def _rel(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return float(np.abs(got[ok] - want[ok]).max() / max(np.abs(want[ok]).max(), 1e-30)) if ok.any() else 0.0


ERODE_CASES = sorted({k[len("erode_"):-2] for k in G.files if k.startswith("erode_")})
LOSS_CASES = sorted({k[len("loss_"):-len("_loss")] for k in G.files if k.startswith("loss_") and k.endswith("_loss")})


def _loss_inputs(name):
    if f"loss_{name}_inputs" in G.files:
        src = str(G[f"loss_{name}_inputs"])
        sign = np.float32(G[f"loss_{name}_mask_sign"])
        return G[f"inputs_{src}_pred"], G[f"inputs_{src}_target"], (sign * G[f"inputs_{src}_mask"]).astype(np.float32)
    return G[f"loss_{name}_pred"], G[f"loss_{name}_target"], G[f"loss_{name}_mask"]


@pytest.mark.parametrize("case", ERODE_CASES)
def test_erode_matches_the_reference_bit_for_bit(case):
    x, k, want = G[f"erode_{case}_x"], int(G[f"erode_{case}_k"]), G[f"erode_{case}_y"]
    got = R.erode(x, k)
    assert _same_bits(got, want), case
    if case.startswith("special"):
        assert np.isnan(want).any() and np.isinf(x).any()


def test_cases_cover_the_edges():
    assert {"basic", "basic_keep", "zero_element_keep", "negative_mask_keep", "odd"} <= set(LOSS_CASES)
    assert len(ERODE_CASES) >= 6


@pytest.mark.parametrize("case", LOSS_CASES)
def test_loss_and_gradients_match_the_reference(case):
    p, t, m = _loss_inputs(case)
    keep = bool(G[f"loss_{case}_keep_batch"])
    r = R.l1_sphere(p, t, m, keep_batch=keep)
    want = G[f"loss_{case}_loss"]
    assert np.size(r["loss32"]) == np.size(want)
    assert _rel(r["loss32"], want) <= 1e-6, case
    assert _rel(r["loss64"], want) <= 1e-6, case
    g = np.ones(p.shape[0] if keep else 1, np.float32)
    gp, gt = R.l1_sphere_grads(p, t, m, g, r["den32"])
    assert _rel(gp, G[f"loss_{case}_grad_pred"]) <= 1e-6, case
    assert _rel(gt, G[f"loss_{case}_grad_target"]) <= 1e-6, case
    if case == "zero_element_keep":
        assert want[1] == 0.0 and r["den32"][1] == np.float32(1e-10)
    if case == "negative_mask_keep":
        assert (r["den32"] < 0).all()


@pytest.mark.parametrize("case", ["holes", "dense"])
def test_closure_matches_the_reference(case):
    pred, depth, far = G[f"closure_{case}_pred"], G[f"closure_{case}_depth"], float(G[f"closure_{case}_far"])
    r = R.closure(pred, depth, far)
    assert bool(G[f"closure_{case}_eroded"]) == (case == "holes")
    assert _same_bits(r["mask"], G[f"closure_{case}_mask"])
    assert _rel(r["loss"], G[f"closure_{case}_loss"]) <= 1e-6
    gp, _ = R.l1_sphere_grads(pred, r["target"], r["mask"], np.float32(0.1), r["den32"])
    assert _rel(gp, G[f"closure_{case}_grad_pred"]) <= 1e-6
    if case == "holes":
        assert (depth < 1e-7).any() and (r["target"][depth < 1e-7] == np.float32(far)).all()


@pytest.mark.parametrize("case", ["holes", "dense"])
def test_unconditional_erosion_equals_the_conditional_one(case):
    pred, depth, far = G[f"closure_{case}_pred"], G[f"closure_{case}_depth"], float(G[f"closure_{case}_far"])
    a, b = R.closure(pred, depth, far), R.closure(pred, depth, far, conditional=False)
    assert _same_bits(a["mask"], b["mask"]) and _same_bits(a["loss"], b["loss"])


def test_eroding_all_ones_gives_all_ones():
    assert (R.erode(np.ones((2, 1, 9, 17), np.float32), 5) == 1.0).all()


@pytest.mark.parametrize("h", [5, 13, 32, 37, 512])
def test_row_weights_within_one_ulp(h):
    want = G[f"row_weights_{h}"]
    got = R.row_weights(h)
    ulp = np.spacing(np.abs(want).astype(np.float32))
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    import torch
    from splatter360_amd.depth_loss import row_weights
    assert np.array_equal(row_weights(h, "cpu").numpy(), want)      # the Python layer's expression is the reference's
