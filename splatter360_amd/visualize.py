"""The pictures of the evaluation step on the GPU: depth colour maps, colour tables, 8-bit frames and error maps
(s360_depth_colormap, s360_colorize, s360_prep_image, s360_error_map, csrc/s360_visualize.hip).

With save_image / save_video and eval_depth on, the reference's test_step (src/model/model_wrapper_erp.py:361-468) calls
depth_map (:122-133) once per rendered depth face and once per stitched depth panorama: a boolean selection, two full
torch.quantile sorts, a log and a normalisation, then apply_color_map (src/visualization/color_map.py:9-19), which copies the map
to the host, runs matplotlib's turbo and copies the float64 [h, w, 3] picture back — which prep_image (src/misc/image_io.py:38-54)
copies to the host again, after six torch launches on float data.  Every error image is |gt - pred|.mean(0) -> .cpu() -> matplotlib
viridis -> uint8 -> float -> prep_image (:369-372, :109-120).  Here `depth_map` colours any number of maps in five launches (an
exact radix selection instead of the sorts, one colouring pass) and can hand back the [h, w, 3] bytes that PIL or ffmpeg consume,
so a picture leaves the device once, at one byte per sample.
There is no CPU path and no autograd: CPU tensors raise, inputs are detached (plugin.install(visualization=True) keeps the
replaced functions for everything the kernels do not take).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from ._call import call, invoke, ptr

COLOR_MAPS = ("turbo", "viridis", "inferno")                 # S360_CMAP_*
MAX_MAP_ELEMENTS = 16_000_000


def _gpu_f32(t, what: str) -> Tensor:
    if not isinstance(t, Tensor):
        raise ValueError(f"{what} expects a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only (no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} expects float32, got {t.dtype}")
    return t.detach()


def _maps(depth: Tensor, what: str):
    """depth[..., h, w] -> (tensor whose maps are contiguous h x w blocks one uniform stride apart, n, h, w, map stride)."""
    d = _gpu_f32(depth, what)
    if d.dim() < 2:
        raise ValueError(f"{what} expects [..., h, w], got {tuple(d.shape)}")
    h, w = int(d.shape[-2]), int(d.shape[-1])
    if h * w < 1 or d.numel() < 1:
        raise ValueError(f"{what} needs non-empty maps, got {tuple(d.shape)}")
    if h * w > MAX_MAP_ELEMENTS:
        raise ValueError(f"{what} takes maps of at most {MAX_MAP_ELEMENTS} elements, got {h} x {w}")
    n = d.numel() // (h * w)
    inner = (w == 1 or d.stride(-1) == 1) and (h == 1 or d.stride(-2) == w)
    if d.dim() == 2:
        d3 = d.unsqueeze(0) if inner else d.contiguous().unsqueeze(0)
    elif inner and d.dim() == 3:
        d3 = d
    else:
        d3 = None
        if inner:
            try:
                d3 = d.view(n, h, w)                         # leading dims that collapse to one stride: still in place
            except RuntimeError:
                d3 = None
        if d3 is None:
            d3 = d.contiguous().view(n, h, w)
    stride = int(d3.stride(0)) if n > 1 else h * w
    if stride < h * w:                                       # expanded or overlapping maps
        d3, stride = d3.contiguous(), h * w
    return d3, n, h, w, stride


def _depth_call(d3, n, h, w, stride, rgb, u8, rng):
    nbytes = C.c_size_t(0)
    invoke("s360_depth_colormap", None, n, h, w, stride, None, None, None, None, C.byref(nbytes), None)
    ws = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=d3.device)
    call("s360_depth_colormap", d3.device, ptr(d3), n, h, w, stride, ptr(rgb), ptr(u8), ptr(rng), ptr(ws), C.byref(nbytes))


def depth_map(depth: Tensor, out: str = "float") -> Tensor:
    """The reference's depth_map for every map of depth[..., h, w] (float32, GPU), each normalised on its own ->
    float32 [..., 3, h, w] (out="float") or uint8 [..., h, w, 3] (out="uint8": the bytes prep_image makes of that picture).
    Leading dims are batch; a view with a uniform leading stride (x[:, 2] of [v, 6, h, w]) is read in place.
    ValueError for a bad shape, dtype or `out`; RuntimeError for a tensor not on the GPU."""
    if out not in ("float", "uint8"):
        raise ValueError(f"out is 'float' or 'uint8', got {out!r}")
    d3, n, h, w, stride = _maps(depth, "depth_map")
    lead = tuple(depth.shape[:-2])
    rgb = torch.empty((n, 3, h, w), dtype=torch.float32, device=d3.device) if out == "float" else None
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=d3.device) if out == "uint8" else None
    _depth_call(d3, n, h, w, stride, rgb, u8, None)
    return rgb.view(*lead, 3, h, w) if out == "float" else u8.view(*lead, h, w, 3)


def depth_map_whole(depth: Tensor) -> Tensor:
    """The reference's depth_map called with depth[..., h, w] as it stands: ONE normalisation over the whole argument (its
    quantiles run over every element), float32 [..., 3, h, w] on the device — a view of a channel-first picture, as the
    reference's rearrange returns one.  At most 16 000 000 elements.  Errors as depth_map."""
    d = _gpu_f32(depth, "depth_map_whole")
    if d.dim() < 2 or d.numel() < 1 or d.numel() > MAX_MAP_ELEMENTS:
        raise ValueError(f"depth_map_whole expects non-empty [..., h, w] of at most {MAX_MAP_ELEMENTS} elements, got {tuple(d.shape)}")
    d = d.contiguous()
    h, w = int(d.shape[-2]), int(d.shape[-1])
    rows = d.numel() // w
    rgb = torch.empty((1, 3, rows, w), dtype=torch.float32, device=d.device)
    _depth_call(d.view(1, rows, w), 1, rows, w, rows * w, rgb, None, None)
    return rgb.view(3, *d.shape[:-2], h, w).movedim(0, -3)


def depth_range(depth: Tensor) -> Tensor:
    """float32 [..., 4] per map of depth[..., h, w]: near_q (the 0.01 quantile of the positive elements), far_q (the 0.99
    quantile of all), log near_q, log far_q — what depth_map normalises with; a map without a positive element gives min, max,
    NaN, NaN.  Errors as depth_map."""
    d3, n, h, w, stride = _maps(depth, "depth_range")
    rng = torch.empty((n, 4), dtype=torch.float32, device=d3.device)
    _depth_call(d3, n, h, w, stride, None, None, rng)
    return rng.view(*depth.shape[:-2], 4)


def colorize(x: Tensor, color_map: str = "inferno", channels: str = "last", out: str = "float") -> Tensor:
    """The reference's apply_color_map for float32 GPU x of any shape: clip to [0, 1], matplotlib's index rule (NaN: black),
    the table of "turbo", "viridis" or "inferno" -> [..., 3] (channels="last"), or [..., 3, h, w] for x[..., h, w]
    (channels="first", apply_color_map_to_image), float32 or uint8 (out="uint8": trunc(float32 * 255)).
    ValueError for an unknown map, layout, `out` or a shape channels="first" cannot take; RuntimeError off the GPU."""
    if color_map not in COLOR_MAPS:
        raise ValueError(f"color_map is one of {COLOR_MAPS}, got {color_map!r}")
    if channels not in ("last", "first") or out not in ("float", "uint8"):
        raise ValueError(f"channels is 'last' or 'first' and out 'float' or 'uint8', got {channels!r}, {out!r}")
    v = _gpu_f32(x, "colorize")
    first = channels == "first"
    if first and v.dim() < 2:
        raise ValueError(f"channels='first' expects [..., h, w], got {tuple(v.shape)}")
    shape = (*v.shape[:-2], 3, *v.shape[-2:]) if first else (*v.shape, 3)
    res = torch.empty(shape, dtype=torch.float32 if out == "float" else torch.uint8, device=v.device)
    if v.numel() == 0:
        return res
    v = v.contiguous()
    plane = int(v.shape[-2] * v.shape[-1]) if first else 0
    call("s360_colorize", v.device, ptr(v), v.numel(), plane, COLOR_MAPS.index(color_map), int(first),
         ptr(res) if out == "float" else None, ptr(res) if out == "uint8" else None)
    return res


def prep_image(image: Tensor) -> Tensor:
    """The reference's prep_image on the device: float32 GPU [c, h, w], [h, w] or [b, c, h, w] with c in {1, 3, 4} ->
    uint8 [h, b w, 3 | 4] on the same device (batch entries side by side, one channel replicated to three,
    trunc(clip(v, 0, 1) * 255), NaN -> 0).  `.cpu().numpy()` of it is what save_image / save_video consume.
    ValueError for a bad shape or dtype; RuntimeError off the GPU."""
    v = _gpu_f32(image, "prep_image")
    if v.dim() == 2:
        v = v[None, None]
    elif v.dim() == 3:
        v = v[None]
    if v.dim() != 4 or int(v.shape[1]) not in (1, 3, 4) or v.numel() == 0:
        raise ValueError(f"prep_image expects non-empty [h, w], [c, h, w] or [b, c, h, w] with c in (1, 3, 4), got {tuple(image.shape)}")
    b, c, h, w = (int(s) for s in v.shape)
    v = v.contiguous()
    res = torch.empty((h, b * w, 4 if c == 4 else 3), dtype=torch.uint8, device=v.device)
    call("s360_prep_image", v.device, ptr(v), b, c, h, w, ptr(res))
    return res


def error_map(pred: Tensor, gt: Tensor) -> Tensor:
    """The evaluation step's error image (model_wrapper_erp.py:369-371): |gt - pred|.mean(0) of float32 GPU [3, h, w] tensors in
    viridis by get_colormap's rule -> uint8 [h, w, 3] on the device (symmetric in the two).
    ValueError for shapes that differ or are not [3, h, w]; RuntimeError off the GPU."""
    a, b = _gpu_f32(pred, "error_map"), _gpu_f32(gt, "error_map")
    if a.dim() != 3 or a.shape[0] != 3 or a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"error_map expects pred and gt of one non-empty [3, h, w] shape, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if a.device != b.device:
        raise ValueError(f"pred and gt are on different devices ({a.device}, {b.device})")
    a, b = a.contiguous(), b.contiguous()
    h, w = int(a.shape[1]), int(a.shape[2])
    res = torch.empty((h, w, 3), dtype=torch.uint8, device=a.device)
    call("s360_error_map", a.device, ptr(a), ptr(b), h, w, ptr(res))
    return res
