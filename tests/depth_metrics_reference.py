"""Numpy statement of the evaluation step's weight-free scores besides SSIM, as include/s360.h specifies them for
s360_depth_metrics and s360_psnr.  Written for this project from that specification; tests/test_eval_scores_spec.py pins it to
numbers recorded from the reference (tests/golden/eval_scores.npz).

depth_metrics       float32 terms, float64 sums, per-metric NaN-skipping counts, float32 thresholds, float32 a-metric division
depth_metrics_f64   the five continuous metrics with every operation (log and subtraction included) in float64
rmse_log_bound      the data-dependent bound of a float32 rmse_log against depth_metrics_f64's
psnr                float32 squared differences, float64 sum
nearest_index       F.interpolate(mode="nearest")'s source index
depth_scores        the evaluation step's protocol around depth_metrics (face drop, nearest lookup, averaging over valid faces)
"""
import numpy as np

F32 = np.float32
KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")
CONTINUOUS = KEYS[:5]
A_KEYS = KEYS[5:]
THRESHOLDS = {"a5": 1.05, "a10": 1.10, "a25": 1.25, "a0": 1.10, "a1": 1.25, "a2": 1.25 ** 2, "a3": 1.25 ** 3}


def _terms(gt, pred, dtype):
    gt, pred = gt.astype(dtype), pred.astype(dtype)
    with np.errstate(all="ignore"):
        d = gt - pred
        lg = np.log(gt) - np.log(pred)
        return {"abs_diff": np.abs(d), "abs_rel": np.abs(d) / gt, "sq_rel": (d * d) / gt, "rmse": d * d, "rmse_log": lg * lg}


def _nan_skipping_mean(term, valid):
    ok = valid & ~np.isnan(term)
    with np.errstate(all="ignore"):
        return np.where(ok, term.astype(np.float64), 0.0).sum(axis=1) / ok.sum(axis=1)


def depth_metrics(gt, pred, valid, mult_a=False):
    """gt, pred float32 [B,N], valid bool [B,N] -> ({key: float32 [B]}, valid_count int64 [B])."""
    gt, pred, valid = np.asarray(gt, F32), np.asarray(pred, F32), np.asarray(valid, bool)
    out = {}
    for k, t in _terms(gt, pred, F32).items():
        assert t.dtype == F32
        with np.errstate(all="ignore"):
            m = _nan_skipping_mean(t, valid).astype(F32)
            out[k] = np.sqrt(m) if k in ("rmse", "rmse_log") else m
    count = valid.sum(axis=1)
    with np.errstate(all="ignore"):
        q1, q2 = gt / pred, pred / gt
        for k in A_KEYS:
            t = F32(THRESHOLDS[k])
            hits = (valid & (q1 < t) & (q2 < t)).sum(axis=1)       # max with NaN propagating < t: both quotients below t
            a = hits.astype(F32) / count.astype(F32)
            out[k] = a * F32(100) if mult_a else a
    assert all(v.dtype == F32 for v in out.values())
    return out, count


def depth_metrics_f64(gt, pred, valid):
    """The five continuous metrics of float32 inputs with every operation in float64 -> {key: float64 [B]}."""
    valid = np.asarray(valid, bool)
    out = {}
    for k, t in _terms(np.asarray(gt, F32), np.asarray(pred, F32), np.float64).items():
        with np.errstate(all="ignore"):
            m = _nan_skipping_mean(t, valid)
            out[k] = np.sqrt(m) if k in ("rmse", "rmse_log") else m
    return out


def rmse_log_bound(gt, pred, valid, u=2.0 ** -22):
    """Per row, how far a float32 evaluation of rmse_log may sit from depth_metrics_f64's: every float32 log is within u
    (relative; two float32 ulps) of the exact one, the float32 subtraction and square add 3 * 2^-24 relative on d^2, so per
    element |err(d^2)| <= e = 2 |d| (u |log gt| + u |log pred|) + 3 * 2^-24 d^2; the mean moves by at most mean(e), its root by
    mean(e) / (2 rmse_log), and the rounding of mean and root adds 2^-23 rmse_log.  Rows whose rmse_log is not finite and
    positive get 0 (they are compared exactly)."""
    gt, pred = np.asarray(gt, F32).astype(np.float64), np.asarray(pred, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        lg, lp = np.log(gt), np.log(pred)
        d = lg - lp
        ok = np.asarray(valid, bool) & ~np.isnan(d * d)
        e = 2 * np.abs(d) * (u * np.abs(lg) + u * np.abs(lp)) + 3 * 2.0 ** -24 * d * d
        mean_e = np.where(ok, e, 0.0).sum(axis=1) / ok.sum(axis=1)
        r = depth_metrics_f64(gt, pred, valid)["rmse_log"]
        b = mean_e / (2 * r) + 2.0 ** -23 * r
    return np.where(np.isfinite(r) & (r > 0) & np.isfinite(b), b, 0.0)


def psnr(pred, gt):
    """pred, gt float32 [N,C,H,W] -> float64 [N]: both clipped to [0, 1] (NaN stays), float32 (gt - pred)^2, float64 mean;
    a mean that rounds to 0 in float32 becomes 1e-10; -10 log10."""
    p, g = np.asarray(pred, F32), np.asarray(gt, F32)
    with np.errstate(all="ignore"):
        p = np.where(p < 0, F32(0), np.where(p > 1, F32(1), p))
        g = np.where(g < 0, F32(0), np.where(g > 1, F32(1), g))
        d = g - p
        t = d * d
        assert t.dtype == F32
        m = t.reshape(t.shape[0], -1).astype(np.float64).mean(axis=1)
        m = np.where(m.astype(F32) == 0, 1e-10, m)
        return -10.0 * np.log10(m)


def psnr_bar(want):
    """4.35 * 2^-22 + 4 ulp32(|psnr|) dB: 10 / ln 10 x the rounding of the mean, plus log10 and the final product."""
    return 4.35 * 2.0 ** -22 + 4 * np.spacing(np.abs(want).astype(F32)).astype(np.float64)


def nearest_index(dst_size, src_size):
    """Source index per destination index: min(floor(float32(dst) * (float32(src_size) / float32(dst_size))), src_size - 1)."""
    scale = F32(src_size) / F32(dst_size)
    prod = np.arange(dst_size, dtype=F32) * scale
    assert prod.dtype == F32
    return np.minimum(np.floor(prod).astype(np.int64), src_size - 1)


def depth_score_rows(depth_pred, depth_gt, faces_per_view=6, drop_first_face=True, min_depth=0.1):
    """The rows the evaluation step scores: depth_pred [b, v*F, h, w], depth_gt [b, v, F, H, W] (a trailing 1 allowed) ->
    gt [R, H*W], pred [R, H*W] (looked up by nearest_index when the sizes differ), valid = gt > float32(min_depth)."""
    gt = np.asarray(depth_gt, F32)
    if gt.ndim == 6:
        gt = gt[..., 0]
    b, v, f, H, W = gt.shape
    pred = np.asarray(depth_pred, F32).reshape(b, v, f, *depth_pred.shape[2:])
    first = 1 if drop_first_face else 0
    gt, pred = gt[:, :, first:], pred[:, :, first:]
    h, w = pred.shape[-2:]
    if (h, w) != (H, W):
        pred = pred[..., nearest_index(H, h), :][..., nearest_index(W, w)]
    gt, pred = gt.reshape(-1, H * W), pred.reshape(-1, H * W)
    return gt, pred, gt > F32(min_depth)


def average_valid_rows(rows, count):
    """{key: [R]} -> {key: float32 scalar}: the float64 sum over the rows with a valid element, one division, rounded."""
    has = np.asarray(count) > 0
    with np.errstate(all="ignore"):
        return {k: F32(np.where(has, np.asarray(r, np.float64), 0.0).sum() / has.sum()) for k, r in rows.items()}


def depth_scores(depth_pred, depth_gt, faces_per_view=6, drop_first_face=True, min_depth=0.1):
    """-> ({key: float32 scalar}, per-row metrics, valid_count): depth_metrics (a-metrics x 100) of depth_score_rows, averaged
    over the rows that have a valid element."""
    gt, pred, valid = depth_score_rows(depth_pred, depth_gt, faces_per_view, drop_first_face, min_depth)
    rows, count = depth_metrics(gt, pred, valid, mult_a=True)
    return average_valid_rows(rows, count), rows, count
