"""Image metrics of the evaluation step on the GPU: SSIM (s360_ssim, csrc/s360_metrics.hip).

The reference scores every rendered face with PSNR, SSIM and LPIPS (src/model/model_wrapper_erp.py:479-493, :635;
src/evaluation/metrics.py).  Its `compute_ssim` (metrics.py:38-54) copies each image to the host and calls skimage's
structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0) one image at a time;
`ssim` computes the same score for a whole batch in two kernel launches on the current stream, with no host synchronisation.
There is no CPU path: CPU tensors raise (plugin.install(metrics=True) keeps the replaced function for those).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from . import _lib

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
    l = _lib.lib()
    nbytes = C.c_size_t(0)
    _lib.check(l.s360_ssim(None, None, n, c, h, w, None, None, C.byref(nbytes), None), "s360_ssim (workspace size)")
    ws = torch.empty(max(int(nbytes.value), 8), dtype=torch.uint8, device=pred.device)
    with torch.cuda.device(pred.device):
        st = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
        rc = l.s360_ssim(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), n, c, h, w, C.c_void_p(out.data_ptr()),
                         C.c_void_p(ws.data_ptr()), C.byref(nbytes), st)
    _lib.check(rc, "s360_ssim")
    return out


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """The reference's compute_ssim(ground_truth, predicted) (metrics.py:38-54): SSIM per batch element, returned with
    predicted's dtype on predicted's device; no host synchronisation."""
    return ssim(predicted, ground_truth).to(dtype=predicted.dtype)
