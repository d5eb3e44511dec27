"""Scores of the evaluation step on the GPU: SSIM (s360_ssim, csrc/s360_metrics.hip), PSNR and the depth metrics
(s360_psnr, s360_depth_metrics, csrc/s360_eval_scores.hip).

The reference scores every rendered face with PSNR, SSIM and LPIPS (src/model/model_wrapper_erp.py:479-493, :635;
src/evaluation/metrics.py).  Its `compute_ssim` (metrics.py:38-54) copies each image to the host and calls skimage's
structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) one image at a time;
`ssim` computes the same score for a whole batch in two kernel launches on the current stream, with no host synchronisation.
Its `compute_psnr` (metrics.py:11-21, also called by every training step) is nine torch launches; `psnr` is two.  Its
`compute_depth_metrics_batched` (src/scripts/compute_depth_metrics.py:47-116) is about eighty launches and a dozen [B,N]
temporaries; `depth_metrics` is one pass and a per-row reduction, and `depth_scores` is the whole protocol of
model_wrapper_erp.py:500-541 on the tensors the step holds, without rearranging or copying them.
There is no CPU path: CPU tensors raise (plugin.install(metrics=True / psnr=True / depth_metrics=True) keeps the replaced
function for those).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from ._call import call, invoke, ptr

WIN_SIZE = 11


def ssim(pred: Tensor, gt: Tensor) -> Tensor:
    """Mean SSIM per image of pred[N,C,H,W] against gt[N,C,H,W] -> float32 [N] on their device (symmetric in the two).
    ValueError for shapes that differ, are not 4-D or have H or W < 11; RuntimeError for tensors not on the GPU."""
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"ssim expects pred and gt of one [N,C,H,W] shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    n, c, h, w = (int(s) for s in pred.shape)
    if h < WIN_SIZE or w < WIN_SIZE:
        raise ValueError(f"ssim needs H, W >= {WIN_SIZE} (the Gaussian window), got {h}x{w}")
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError("ssim runs on the GPU only (no CPU path)")
    if pred.device != gt.device:
        raise ValueError(f"pred and gt are on different devices ({pred.device}, {gt.device})")
    if c < 1:
        raise ValueError("ssim needs at least one channel")
    out = torch.empty(n, dtype=torch.float32, device=pred.device)
    if n == 0:
        return out
    x = pred.detach().float().contiguous()
    y = gt.detach().float().contiguous()
    ws, nbytes = _workspace(pred.device, "s360_ssim", None, None, n, c, h, w, None, None)
    call("s360_ssim", pred.device, ptr(x), ptr(y), n, c, h, w, ptr(out), ptr(ws), C.byref(nbytes))
    return out


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """The reference's compute_ssim(ground_truth, predicted) (metrics.py:38-54): SSIM per batch element, returned with
    predicted's dtype on predicted's device; no host synchronisation."""
    return ssim(predicted, ground_truth).to(dtype=predicted.dtype)


DEPTH_METRIC_KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")


def _workspace(device, name, *args) -> tuple:
    """The size query of entry point `name` (null pointers in `args`, no launch) and a workspace of that size."""
    nbytes = C.c_size_t(0)
    invoke(name, *args, C.byref(nbytes), None)
    return torch.empty(max(int(nbytes.value), 8), dtype=torch.uint8, device=device), nbytes


def _rows(t: Tensor) -> Tensor:
    """float32 [B,N] whose elements of a row are adjacent (a row stride is passed to the kernel): converted only if needed."""
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    return t


def psnr(pred: Tensor, gt: Tensor) -> Tensor:
    """PSNR per image of pred[N,C,H,W] against gt[N,C,H,W], both clipped to [0, 1] -> float32 [N] on their device; an identical
    pair gives 100 dB (the mean 0 is replaced by 1e-10), a NaN pixel NaN.
    ValueError for shapes that differ or are not 4-D; RuntimeError for tensors not on the GPU."""
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"psnr expects pred and gt of one [N,C,H,W] shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if not (pred.is_cuda and gt.is_cuda):
        raise RuntimeError("psnr runs on the GPU only (no CPU path)")
    if pred.device != gt.device:
        raise ValueError(f"pred and gt are on different devices ({pred.device}, {gt.device})")
    n, c, h, w = (int(s) for s in pred.shape)
    if n > 0 and c * h * w == 0:
        raise ValueError(f"psnr needs non-empty images, got {tuple(pred.shape)}")
    out = torch.empty(n, dtype=torch.float32, device=pred.device)
    if n == 0:
        return out
    x = pred.detach().float().contiguous()
    y = gt.detach().float().contiguous()
    ws, nbytes = _workspace(pred.device, "s360_psnr", None, None, n, c, h, w, None, None)
    call("s360_psnr", pred.device, ptr(x), ptr(y), n, c, h, w, ptr(out), ptr(ws), C.byref(nbytes))
    return out


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """The reference's compute_psnr(ground_truth, predicted) (metrics.py:11-21): PSNR per batch element with the dtype torch gives
    `ground_truth - predicted`, on their device."""
    return psnr(predicted, ground_truth).to(dtype=torch.result_type(ground_truth, predicted))


def _depth_metrics_call(gt, pred, valid, n_rows, n, strides, rows_per_group, group_strides, threshold, lookup, mult_a, scores):
    dev = gt.device
    out = torch.empty((len(DEPTH_METRIC_KEYS), n_rows), dtype=torch.float32, device=dev)
    count = torch.empty(n_rows, dtype=torch.int32, device=dev)
    red = torch.empty(len(DEPTH_METRIC_KEYS), dtype=torch.float32, device=dev) if scores else None
    dims = (n_rows, n, *strides, rows_per_group, *group_strides, float(threshold), *lookup, int(bool(mult_a)))
    ws, nbytes = _workspace(dev, "s360_depth_metrics", None, None, None, *dims, None, None, None, None)
    call("s360_depth_metrics", dev, ptr(gt), ptr(pred), ptr(valid), *dims, ptr(out), ptr(count), ptr(red), ptr(ws), C.byref(nbytes))
    return out, count, red


def depth_metrics(gt_bN: Tensor, pred_bN: Tensor, valid_bN: Tensor, mult_a: bool = False, return_valid_count: bool = False):
    """The twelve depth metrics per row of gt[B,N] against pred[B,N] over the elements where valid[B,N] is set ->
    {key: float32 [B]} in the order DEPTH_METRIC_KEYS (return_valid_count: also the int32 [B] number of valid elements).
    A continuous metric is the mean over the valid elements where its own term is not NaN; an a-metric is the share of the valid
    elements with max(gt / pred, pred / gt) < t (x 100 with mult_a; a NaN ratio is a miss); a row with no valid element gives NaN.
    Rows may be strided views (no copy); other float types and layouts are converted.
    ValueError for shapes that differ or are not 2-D; RuntimeError for tensors not on the GPU."""
    if gt_bN.dim() != 2 or gt_bN.shape != pred_bN.shape or gt_bN.shape != valid_bN.shape:
        raise ValueError(f"depth_metrics expects gt, pred and valid of one [B,N] shape, got {tuple(gt_bN.shape)}, "
                         f"{tuple(pred_bN.shape)} and {tuple(valid_bN.shape)}")
    if not (gt_bN.is_cuda and pred_bN.is_cuda and valid_bN.is_cuda):
        raise RuntimeError("depth_metrics runs on the GPU only (no CPU path)")
    if not (gt_bN.device == pred_bN.device == valid_bN.device):
        raise ValueError(f"gt, pred and valid are on different devices ({gt_bN.device}, {pred_bN.device}, {valid_bN.device})")
    b, n = (int(s) for s in gt_bN.shape)
    if b == 0 or n == 0:
        vals = torch.full((len(DEPTH_METRIC_KEYS), b), float("nan"), dtype=torch.float32, device=gt_bN.device)
        count = torch.zeros(b, dtype=torch.int32, device=gt_bN.device)
    else:
        g, p = _rows(gt_bN), _rows(pred_bN)
        v = valid_bN.detach()
        if v.dtype != torch.bool:
            v = v != 0
        if n > 1 and v.stride(1) != 1:
            v = v.contiguous()
        vals, count, _ = _depth_metrics_call(g, p, v, b, n, (g.stride(0), p.stride(0), v.stride(0)), b, (0, 0), 0.0, (0, 0, 0, 0),
                                             mult_a, False)
    out = {k: vals[i] for i, k in enumerate(DEPTH_METRIC_KEYS)}
    return (out, count) if return_valid_count else out


@torch.no_grad()
def compute_depth_metrics_batched(gt_bN: Tensor, pred_bN: Tensor, valid_masks_bN: Tensor, mult_a: bool = False) -> dict:
    """The reference's compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a) (compute_depth_metrics.py:47-116):
    the same twelve keys, float32 [B] each on the inputs' device; the inputs are not modified."""
    return depth_metrics(gt_bN, pred_bN, valid_masks_bN, mult_a)


@torch.no_grad()
def depth_scores(depth_pred: Tensor, depth_gt: Tensor, *, faces_per_view: int = 6, drop_first_face: bool = True,
                 min_depth: float = 0.1) -> dict:
    """The evaluation step's depth protocol (model_wrapper_erp.py:500-541) on the tensors the step holds: depth_pred[b, v*F, h, w]
    (the decoder's `output.depth`) against depth_gt[b, v, F, H, W, 1] (`batch["target"]["depth_cubes"]`; [b, v, F, H, W] too),
    F = faces_per_view.  Face 0 of every view (the top face) is dropped, pred is looked up with F.interpolate(mode="nearest")'s
    index rule when (h, w) != (H, W), an element is valid where gt > min_depth, the a-metrics are x 100, and each of the twelve
    metrics is averaged over the faces that have a valid element (none: NaN) -> {key: float32 scalar} on the device, with no
    host read.  Neither tensor is rearranged or copied when it is contiguous float32."""
    if depth_gt.dim() == 6 and depth_gt.shape[-1] == 1:
        depth_gt = depth_gt[..., 0]
    f = int(faces_per_view)
    if depth_gt.dim() != 5 or depth_pred.dim() != 4 or f < 1 or depth_gt.shape[2] != f:
        raise ValueError(f"depth_scores expects depth_pred [b, v*{f}, h, w] and depth_gt [b, v, {f}, H, W, 1], got "
                         f"{tuple(depth_pred.shape)} and {tuple(depth_gt.shape)}")
    b, v, _, H, W = (int(s) for s in depth_gt.shape)
    if depth_pred.shape[0] != b or depth_pred.shape[1] != v * f:
        raise ValueError(f"depth_pred {tuple(depth_pred.shape)} does not hold {b} x {v} x {f} faces")
    if not (depth_pred.is_cuda and depth_gt.is_cuda):
        raise RuntimeError("depth_scores runs on the GPU only (no CPU path)")
    if depth_pred.device != depth_gt.device:
        raise ValueError(f"depth_pred and depth_gt are on different devices ({depth_pred.device}, {depth_gt.device})")
    h, w = int(depth_pred.shape[2]), int(depth_pred.shape[3])
    first = 1 if drop_first_face else 0
    per_view = f - first
    rows = b * v * per_view
    if rows == 0 or H * W == 0 or h * w == 0:
        nan = torch.full((), float("nan"), dtype=torch.float32, device=depth_pred.device)
        return {k: nan.clone() for k in DEPTH_METRIC_KEYS}
    g = depth_gt.detach().float().contiguous()
    p = depth_pred.detach().float().contiguous()
    lookup = (H, W, h, w) if (h, w) != (H, W) else (0, 0, 0, 0)
    # row r is face first + r % per_view of view r // per_view: start at face `first`, groups of per_view rows every f planes
    _, _, red = _depth_metrics_call(g.view(-1)[first * H * W:], p.view(-1)[first * h * w:], None, rows, H * W, (H * W, h * w, 0),
                                    per_view, (f * H * W, f * h * w), min_depth, lookup, True, True)
    return {k: red[i] for i, k in enumerate(DEPTH_METRIC_KEYS)}
