"""The numpy statement of the depth metrics and PSNR (tests/depth_metrics_reference.py) against numbers recorded from the
reference's own functions on CPU (tests/golden/eval_scores.npz, written by tests/golden/make_golden_eval_scores.py), the
nearest-neighbour index rule against F.interpolate, and the evaluation step's protocol against its torch expressions.

Bars (the ones tests/test_gpu_eval_scores.py holds the kernels to; here the reference's float32 arithmetic must meet them):
  a-metrics, NaN and inf patterns      exact (bit-equal)
  abs_diff, abs_rel, sq_rel, rmse      relative 2^-22 against the float32-terms / float64-sums statement
  rmse_log                             depth_metrics_reference.rmse_log_bound with u = 2^-22 against the all-float64 statement
                                       (measured on the golden's finite rows: the reference sits at most at 0.044 of that
                                       bound, the float32 statement at 0.065, so u stays)
  PSNR                                 4.35 * 2^-22 + 4 ulp32(|psnr|) dB against the float64-sum statement
"""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_metrics_reference as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "eval_scores.npz"
REL = 2.0 ** -22
DEPTH_CASES = ("holes", "clean", "masked")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def same_specials(a, b):
    """NaN and +-inf in the same places."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isinf(a), a, 0), np.where(np.isinf(b), b, 0))


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    return np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), 1e-300) if fin.any() else np.zeros(1)


def test_golden_holds_numbers_only_and_the_cases(golden):
    assert tuple(golden["depth_keys"]) == R.KEYS
    for v in golden.values():
        assert v.dtype.kind in "fbU"
    assert GOLDEN.stat().st_size < 1 << 20
    gt, pred, valid = (golden[f"depth_holes_{k}"] for k in ("gt", "pred", "valid"))
    assert gt.shape[0] <= 15 and gt.shape[1] <= 64 * 64
    assert not valid[3].any() and valid.any(axis=1).sum() == 14
    assert (pred[valid] == 0).any() and np.isnan(pred[5][valid[5]]).any() and (pred[6][valid[6]] < 0).any()
    want = golden["depth_holes_out"]
    # a row without a valid element: NaN twelve times; pred == 0 under a valid element: rmse_log = inf, everything else finite
    assert np.isnan(want[:, 3]).all() and np.isinf(np.delete(want[4], 3)).all() and np.isfinite(np.delete(want[:4], 3, axis=1)).all()
    assert np.isfinite(golden["depth_clean_out"]).all()


@pytest.mark.parametrize("case", DEPTH_CASES)
@pytest.mark.parametrize("mult_a", (False, True))
def test_statement_reproduces_the_reference(golden, case, mult_a):
    gt, pred, valid = (golden[f"depth_{case}_{k}"] for k in ("gt", "pred", "valid"))
    want = golden[f"depth_{case}_out_mult" if mult_a else f"depth_{case}_out"]
    got, count = R.depth_metrics(gt, pred, valid, mult_a)
    assert np.array_equal(count, valid.sum(axis=1))
    f64 = R.depth_metrics_f64(gt, pred, valid)
    bound = R.rmse_log_bound(gt, pred, valid)
    for i, k in enumerate(R.KEYS):
        assert got[k].dtype == np.float32 and same_specials(got[k], want[i]), k
        if k in R.A_KEYS:
            assert np.array_equal(got[k], want[i], equal_nan=True), k
        elif k != "rmse_log":
            err = rel_err(want[i], got[k]).max()
            print(f"{case} {k}: reference at {err:.2e} of the statement (bar {REL:.2e})")
            assert err <= REL, (k, err)
    # rmse_log: the reference's CPU float32 and the float32 statement against the all-float64 one, inside the computed bound
    for name, val in (("reference", want[4]), ("statement", got["rmse_log"])):
        assert same_specials(val, f64["rmse_log"])
        fin = np.isfinite(f64["rmse_log"])
        err = np.abs(val.astype(np.float64)[fin] - f64["rmse_log"][fin])
        print(f"{case} rmse_log: {name} at most {np.max(err / np.maximum(bound[fin], 1e-300), initial=0):.3f} of the bound")
        assert (err <= bound[fin]).all(), (name, err, bound[fin])
    # the float64 variant agrees with the float32-terms one far inside the same bar x 4 (terms differ by float32 roundings)
    for k in ("abs_diff", "abs_rel", "sq_rel", "rmse"):
        assert same_specials(got[k], f64[k]) and rel_err(got[k], f64[k]).max() <= 4 * REL, k


def test_threshold_comparison_is_in_float32(golden):
    """Row 7 of `holes` holds gt = 1 against pred = float32(t) (a miss: float32(1.05) < 1.05 is False in float32, True if the
    threshold stayed a double) and one ulp below (a hit), for the five thresholds."""
    gt, pred = golden["depth_holes_gt"][7:8, :11], golden["depth_holes_pred"][7:8, :11]
    for i, t in enumerate((1.05, 1.10, 1.25, 1.25 ** 2, 1.25 ** 3)):
        at, below = 1 + 2 * i, 2 + 2 * i
        assert gt[0, at] == 1 and pred[0, at] == np.float32(t) and pred[0, below] == np.nextafter(np.float32(t), np.float32(0))
        key = ("a5", "a10", "a25", "a2", "a3")[i]
        only = np.zeros((1, 11), bool)
        only[0, at] = True
        assert R.depth_metrics(gt, pred, only)[0][key][0] == 0.0
        only[0, at], only[0, below] = False, True
        assert R.depth_metrics(gt, pred, only)[0][key][0] == 1.0


def test_psnr_statement_reproduces_the_reference(golden):
    want = golden["psnr_out"]
    got = R.psnr(golden["psnr_pred"], golden["psnr_gt"])
    assert same_specials(got, want) and np.isnan(want).sum() == 1
    fin = np.isfinite(got)
    err, bar = np.abs(want.astype(np.float64) - got)[fin], R.psnr_bar(got)[fin]
    print("psnr", got, "reference error", err, "bar", bar)
    assert (err <= bar).all()
    assert got[7] == 100.0 and got[9] == 100.0 and 5 < got[0] < 20 and got[5] > 90


@pytest.mark.parametrize("src,dst", [(256, 512), (256, 320), (512, 256), (100, 37), (37, 100), (5, 5), (1, 7)])
def test_nearest_rule_equals_interpolate(src, dst):
    x = torch.arange(src, dtype=torch.float32).view(1, 1, src, 1).expand(1, 1, src, 3).contiguous()
    want = F.interpolate(x, size=(dst, 3), mode="nearest")[0, 0, :, 0].numpy().astype(np.int64)
    assert np.array_equal(R.nearest_index(dst, src), want)
    want_w = F.interpolate(x.transpose(2, 3).contiguous(), size=(3, dst), mode="nearest")[0, 0, 0].numpy().astype(np.int64)
    assert np.array_equal(R.nearest_index(dst, src), want_w)


def _step_expressions(depth_pred, depth_gt, v, num_cubes=6):
    """The evaluation step's depth block (model_wrapper_erp.py:500-541) in plain torch, without einops, around the statement's
    per-row metrics: drop face 0, flatten to rows, F.interpolate pred if the sizes differ, valid = gt > 0.1, rows without a
    valid element set to 0, the sum divided by the number of rows that have one."""
    b = depth_gt.shape[0]
    gt = depth_gt[:, :, 1:]
    gt = gt.reshape(b * v * (num_cubes - 1), 1, *gt.shape[3:5])
    pred = depth_pred.reshape(b, v, num_cubes, *depth_pred.shape[2:])[:, :, 1:]
    pred = pred.reshape(b * v * (num_cubes - 1), 1, *pred.shape[3:])
    if pred.shape != gt.shape:
        pred = F.interpolate(pred, size=(gt.shape[-2], gt.shape[-1]), mode="nearest")
    valid = gt > 0.1
    valid_rows = torch.any(valid.reshape(b * v * (num_cubes - 1), -1), dim=-1)
    rows, _ = R.depth_metrics(gt.flatten(1).float().numpy(), pred.flatten(1).float().numpy(), valid.flatten(1).numpy(), mult_a=True)
    out = {}
    for k, r in rows.items():
        r = torch.from_numpy(r.copy())
        r[~valid_rows] = 0
        out[k] = (r.sum() / valid_rows.count_nonzero()).item()
    return out


@pytest.mark.parametrize("hw,HW", [((16, 16), (16, 16)), ((16, 16), (32, 32)), ((20, 12), (9, 31))])
def test_depth_scores_protocol(hw, HW):
    g = torch.Generator().manual_seed(11)
    b, v = 2, 3
    depth_gt = torch.rand((b, v, 6, *HW, 1), generator=g) * 8 + 0.2
    depth_gt[torch.rand(depth_gt.shape, generator=g) < 0.1] = 0.0
    depth_gt[0, 1, 2] = 0.0                                   # a dropped-in face without any valid depth
    depth_gt[:, :, 0] = 0.0                                   # the top face: empty, and dropped
    depth_pred = torch.rand((b, v * 6, *hw), generator=g) * 8 + 0.2
    want = _step_expressions(depth_pred, depth_gt, v)
    scores, rows, count = R.depth_scores(depth_pred.numpy(), depth_gt.numpy())
    assert count.shape == (b * v * 5,) and (count == 0).sum() == 1
    assert rows["abs_diff"].shape == (b * v * 5,)
    # torch sums the n = 30 float32 rows in float32 ((n - 1) roundings at most) and divides (one more); the statement rounds once
    bar = (b * v * 5 + 1) * 2.0 ** -24
    for k in R.KEYS:
        assert np.isfinite(scores[k]) and abs(float(scores[k]) - want[k]) <= bar * abs(want[k]), (k, scores[k], want[k])
    # keeping face 0 changes the rows
    assert R.depth_scores(depth_pred.numpy(), depth_gt.numpy(), drop_first_face=False)[2].shape == (b * v * 6,)
