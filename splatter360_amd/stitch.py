"""Cube -> equirectangular stitch on the MI355X (replaces Cube2Equirec, /root/reference/
src/geometry/layers.py:41-116, and fuses change_order, src/model/model_wrapper_erp.py:135-158).

The sampling grid is host-side numpy restated from layers.py:60-106 (same float32/float64 mix so
it is bit-identical; pinned by tests/golden/cube2equirec_*.npz); the gather is one HIP kernel.  The
adjoint is a second gather over the grid's inverse (adjoint_plan, built once per grid here): no
atomics, so gradients through the stitch are bit-reproducible.

depth_to_distance and Cube2Equirec.stitch_distance_rendered are the depth channel's counterpart: z-depth -> ray distance
(depth_to_distance_map_batch, src/geometry/z_depth_to_distance.py:4-34) alone, and fused into the stitch for the evaluation
step's depth panorama (model_wrapper_erp.py:445-463).
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import torch
from torch import Tensor, nn

from ._call import call, ptr

# Cube2Equirec slot order is (F R B L U D); faces rendered in the order (top, front, left, back,
# right, bottom) are mapped by the reference's change_order(): flip faces 0 and 5 on both image
# axes, then slots <- rendered [3, 4, 1, 2, 0, 5].  Bit 3 (value 8) = flipped.
CHANGE_ORDER_FACE_MAP = (3, 4, 1, 2, 0 | 8, 5 | 8)


def face_type_map(equ_h: int, equ_w: int) -> np.ndarray:
    """[H,W] int face slot per ERP pixel (0F 1R 2B 3L 4U 5D), layers.py:60-76."""
    q = equ_w // 4
    shift = 3 * equ_w // 8
    tp = np.roll(np.repeat(np.arange(4), q)[None, :].repeat(equ_h, 0), shift, axis=1)
    lon = np.linspace(-np.pi, np.pi, q) / 4
    top_rows = equ_h // 2 - np.round(np.arctan(np.cos(lon)) * equ_h / np.pi).astype(int)  # rows above -> ceiling
    col_mask = np.arange(equ_h)[:, None] < top_rows[None, :]
    mask = np.roll(np.concatenate([col_mask] * 4, 1), shift, axis=1)
    tp = tp.copy()
    tp[mask] = 4
    tp[mask[::-1]] = 5
    return tp


@lru_cache(maxsize=8)
def sample_grid_numpy(face_w: int, equ_h: int, equ_w: int) -> np.ndarray:
    """[H,W,3] float32 (u, v, face-z) = Cube2Equirec.sample_grid[0,0]  (layers.py:78-106)."""
    tp = face_type_map(equ_h, equ_w)
    f32 = np.float32
    lon = ((np.linspace(0, equ_w - 1, num=equ_w, dtype=f32) + 0.5) / equ_w - 0.5) * 2 * np.pi
    lat = -((np.linspace(0, equ_h - 1, num=equ_h, dtype=f32) + 0.5) / equ_h - 0.5) * np.pi
    lon, lat = np.meshgrid(lon, lat)
    u = np.zeros((equ_h, equ_w), f32)
    v = np.zeros((equ_h, equ_w), f32)
    for i in range(4):  # side faces: tangent-plane coordinates
        m = tp == i
        u[m] = 0.5 * np.tan(lon[m] - np.pi * i / 2)
        v[m] = -0.5 * np.tan(lat[m]) / np.cos(lon[m] - np.pi * i / 2)
    m = tp == 4
    c = 0.5 * np.tan(np.pi / 2 - lat[m])
    u[m] = c * np.sin(lon[m])
    v[m] = c * np.cos(lon[m])
    m = tp == 5
    c = 0.5 * np.tan(np.pi / 2 - np.abs(lat[m]))
    u[m] = c * np.sin(lon[m])
    v[m] = -c * np.cos(lon[m])
    u = np.clip(u, -0.5, 0.5) * 2
    v = np.clip(v, -0.5, 0.5) * 2
    z = tp.astype(f32) / 2.5 - 1
    return np.ascontiguousarray(np.stack([u, v, z], -1).astype(f32))


def _unnorm_clip(g: np.ndarray, size: int) -> np.ndarray:
    """The kernel's float32 unnormalise + border clip (align_corners=True)."""
    f32 = np.float32
    i = ((g.astype(f32) + f32(1)) / f32(2)) * f32(size - 1)
    return np.minimum(f32(size - 1), np.maximum(i, f32(0)))


def adjoint_plan(grid: np.ndarray, face_w: int):
    """The inverse of a sampling grid [H,W,3] (float32) over the [6,fw,fw] slot-space volume, for s360_cube2erp_backward:
    (offsets int32 [6*fw*fw + 1], entries int32) — texel t = s*fw*fw + y*fw + x is read by the taps
    entries[offsets[t]:offsets[t+1]] = pixel*8 + (4*dz + 2*dy + dx), sorted by pixel.  Every in-range tap is listed once, weight 0
    included (grid_sample adds those too); taps outside the volume are not.  It does not depend on the face map."""
    g = np.ascontiguousarray(grid, dtype=np.float32).reshape(-1, 3)
    n = g.shape[0]
    if n * 8 > np.iinfo(np.int32).max:
        raise ValueError("stitch adjoint plan: equ_h * equ_w * 8 must fit in int32")
    x0 = np.floor(_unnorm_clip(g[:, 0], face_w)).astype(np.int64)
    y0 = np.floor(_unnorm_clip(g[:, 1], face_w)).astype(np.int64)
    z0 = np.floor(_unnorm_clip(g[:, 2], 6)).astype(np.int64)
    k = np.arange(8)
    x, y, z = x0[:, None] + (k & 1), y0[:, None] + ((k >> 1) & 1), z0[:, None] + (k >> 2)   # [n, 8] in tap order
    ok = (x < face_w) & (y < face_w) & (z <= 5)                                              # the lower corners are >= 0
    tex = ((z * face_w + y) * face_w + x)[ok]
    tap = np.arange(n * 8, dtype=np.int64).reshape(n, 8)[ok]                                 # pixel*8 + tap, ascending
    order = np.argsort(tex, kind="stable")                                                   # keeps pixel order per texel
    texels = 6 * face_w * face_w
    offsets = np.zeros(texels + 1, np.int64)
    np.cumsum(np.bincount(tex, minlength=texels), out=offsets[1:])
    return offsets.astype(np.int32), tap[order].astype(np.int32)


@lru_cache(maxsize=4)
def adjoint_plan_numpy(face_w: int, equ_h: int, equ_w: int):
    """adjoint_plan of sample_grid_numpy(face_w, equ_h, equ_w), cached like the grid (<= 8 int32 entries per ERP pixel)."""
    return adjoint_plan(sample_grid_numpy(face_w, equ_h, equ_w), face_w)


def _face_map_arr(face_map):
    return None if face_map is None else (C.c_int32 * 6)(*face_map)


# z-depth -> distance conventions (include/s360.h S360_D2D_*)
DISTANCE_CONVENTIONS = {"reference": 0, "pixel": 1}


def _convention_code(convention: str) -> int:
    if convention not in DISTANCE_CONVENTIONS:
        raise ValueError(f"convention must be one of {sorted(DISTANCE_CONVENTIONS)}, not {convention!r}")
    return DISTANCE_CONVENTIONS[convention]


def _check_gpu_f32(what: str, **tensors) -> None:
    """RuntimeError for CPU tensors (GPU only, no CPU path), ValueError for another dtype or mismatched devices."""
    first = None
    for name, t in tensors.items():
        if not isinstance(t, Tensor):
            raise ValueError(f"{what}: {name} must be a tensor")
        if not t.is_cuda:
            raise RuntimeError(f"{what} runs on the GPU only (no CPU path): {name} is on {t.device}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, not {t.dtype}")
        first = t if first is None else first
        if t.device != first.device:
            raise ValueError(f"{what}: {name} is on {t.device}, not {first.device}")


def fxfycxcy_from_intrinsics(intrinsics: Tensor, h: int, w: int) -> Tensor:
    """K[..., 3, 3] normalised intrinsics -> [..., 4] (fx, fy, cx, cy) in pixels of an h x w image, with the reference's own
    multiplications in K's dtype (model_wrapper_erp.py:450-454: fx = K[0,0] * width, fy = K[1,1] * height, cx = K[0,2] * width,
    cy = K[1,2] * height)."""
    if intrinsics.dim() < 2 or tuple(intrinsics.shape[-2:]) != (3, 3):
        raise ValueError(f"intrinsics must be [..., 3, 3], not {tuple(intrinsics.shape)}")
    return torch.stack([intrinsics[..., 0, 0] * w, intrinsics[..., 1, 1] * h, intrinsics[..., 0, 2] * w, intrinsics[..., 1, 2] * h], dim=-1)


class _DepthToDistance(torch.autograd.Function):
    """depth [N,H,W], k4 [N,4] (contiguous float32 on one GPU) -> distance [N,H,W]."""

    @staticmethod
    def forward(ctx, depth, k4, conv):
        n, h, w = depth.shape
        dist = torch.empty_like(depth)
        call("s360_depth_to_distance_forward", depth.device, ptr(depth), ptr(k4), ptr(dist), n, h, w, conv)
        ctx.save_for_backward(depth, k4)
        ctx.conv = conv
        return dist

    @staticmethod
    def backward(ctx, d_dist):
        depth, k4 = ctx.saved_tensors
        n, h, w = depth.shape
        g = d_dist.detach().float().contiguous()
        d_depth = torch.empty_like(depth)
        call("s360_depth_to_distance_backward", depth.device, ptr(g), ptr(depth), ptr(k4), ptr(d_depth), n, h, w, ctx.conv)
        return d_depth, None, None


def depth_to_distance(depth: Tensor, fxfycxcy: Tensor, convention: str = "reference") -> Tensor:
    """z-depth maps depth[..., H, W] -> ray distance |d| s, s = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1), the same shape:
    depth_to_distance_map_batch (z_depth_to_distance.py:4-34) in one kernel, float64 arithmetic rounded once.  fxfycxcy[N, 4] holds
    (fx, fy, cx, cy) in pixels, one row per map (N = the product of depth's leading dimensions); it takes no gradient.  The input
    is not modified.
    convention="reference": u is the ROW index and v the column index — what the reference's "ij" meshgrid pairs with cx / fx and
      cy / fy; H == W is required, as it is for the reference to broadcast.
    convention="pixel": u is the column (x with fx, cx) and v the row (y with fy, cy); any H, W.
    d = 0 gives 0 and a negative d gives |d| s.  The gradient is sign(d) s, and 0 at d = 0: finite, where torch's autograd of the
    reference's sqrt gives NaN."""
    what = "depth_to_distance"
    conv = _convention_code(convention)
    _check_gpu_f32(what, depth=depth, fxfycxcy=fxfycxcy)
    if depth.dim() < 2 or fxfycxcy.dim() != 2 or fxfycxcy.shape[1] != 4:
        raise ValueError(f"{what}: depth must be [..., H, W] and fxfycxcy [N, 4], not {tuple(depth.shape)} and {tuple(fxfycxcy.shape)}")
    h, w = int(depth.shape[-2]), int(depth.shape[-1])
    n = int(fxfycxcy.shape[0])
    lead = 1
    for s in depth.shape[:-2]:
        lead *= int(s)
    if lead != n:
        raise ValueError(f"{what}: depth {tuple(depth.shape)} holds {lead} maps, fxfycxcy {n} rows")
    if conv == DISTANCE_CONVENTIONS["reference"] and h != w:
        raise ValueError(f"{what}: convention='reference' needs square maps (the reference only broadcasts for H == W), not {h} x {w}")
    if depth.numel() == 0:
        return torch.empty_like(depth)
    out = _DepthToDistance.apply(depth.contiguous().view(n, h, w), fxfycxcy.detach().contiguous(), conv)
    return out.view(depth.shape)


class _StitchDistance(torch.autograd.Function):
    """depth faces [N,6,fw,fw], k4 [N,6,4] (contiguous float32 on one GPU) -> ERP distance [N,eh,ew] through `grid` / its plan."""

    @staticmethod
    def forward(ctx, depth, k4, grid, plan_offsets, plan_entries, face_map, conv):
        n, fw = int(depth.shape[0]), int(depth.shape[-1])
        eh, ew = int(grid.shape[0]), int(grid.shape[1])
        erp = torch.empty((n, eh, ew), dtype=torch.float32, device=depth.device)
        call("s360_cube2erp_distance_forward", depth.device, ptr(depth), ptr(k4), ptr(grid), ptr(erp), n, fw, eh, ew, conv,
             _face_map_arr(face_map), None)
        ctx.save_for_backward(depth, k4, grid, plan_offsets, plan_entries)
        ctx.meta = (face_map, conv)
        return erp

    @staticmethod
    def backward(ctx, d_erp):
        depth, k4, grid, offs, ents = ctx.saved_tensors
        face_map, conv = ctx.meta
        n, fw = int(depth.shape[0]), int(depth.shape[-1])
        eh, ew = int(grid.shape[0]), int(grid.shape[1])
        if (offs.dtype, ents.dtype) != (torch.int32, torch.int32) or offs.numel() != 6 * fw * fw + 1 \
                or not (offs.is_cuda and ents.is_cuda and offs.is_contiguous() and ents.is_contiguous()):
            raise RuntimeError("cube->ERP distance stitch backward: the adjoint plan does not belong to this grid / device")
        g = d_erp.detach().float().contiguous()
        d_depth = torch.empty_like(depth)
        call("s360_cube2erp_distance_backward", depth.device, ptr(g), ptr(depth), ptr(k4), ptr(grid), ptr(offs), ptr(ents),
             ptr(d_depth), n, fw, eh, ew, conv, _face_map_arr(face_map), None)
        return d_depth, None, None, None, None, None, None


class _Stitch(torch.autograd.Function):
    """faces -> ERP through `grid` [eh,ew,3]; `plan` = (offsets, entries) = adjoint_plan(grid) on the same device."""

    @staticmethod
    def forward(ctx, faces, grid, plan_offsets, plan_entries, face_map, strides, channels, face_w):
        if not faces.is_cuda:
            raise RuntimeError("cube->ERP stitch runs on the GPU only (no CPU path)")
        eh, ew = int(grid.shape[0]), int(grid.shape[1])
        x = faces.detach().float()
        if strides is None:
            x = x.contiguous()
        erp = torch.empty((channels, eh, ew), dtype=torch.float32, device=faces.device)
        sarr = None if strides is None else (C.c_int64 * 3)(*strides)
        call("s360_cube2erp_forward", faces.device, ptr(x), ptr(grid), ptr(erp), channels, face_w, eh, ew, _face_map_arr(face_map), sarr)
        ctx.save_for_backward(grid, plan_offsets, plan_entries)
        ctx.meta = (face_map, strides, channels, face_w, tuple(faces.shape))
        return erp

    @staticmethod
    def backward(ctx, d_erp):
        grid, offs, ents = ctx.saved_tensors
        face_map, strides, channels, face_w, shape = ctx.meta
        eh, ew = int(grid.shape[0]), int(grid.shape[1])
        if (offs.dtype, ents.dtype) != (torch.int32, torch.int32) or offs.numel() != 6 * face_w * face_w + 1 \
                or not (offs.is_cuda and ents.is_cuda and offs.is_contiguous() and ents.is_contiguous()):
            raise RuntimeError("cube->ERP stitch backward: the adjoint plan does not belong to this grid / device")
        g = d_erp.detach().float().contiguous()
        d_faces = torch.empty((6, channels, face_w, face_w), dtype=torch.float32, device=g.device)
        call("s360_cube2erp_backward", g.device, ptr(g), ptr(grid), ptr(offs), ptr(ents), ptr(d_faces), channels, face_w, eh, ew,
             _face_map_arr(face_map), None)
        if strides is not None:  # input was [C, fw, 6*fw]
            d_faces = d_faces.permute(1, 2, 0, 3).reshape(shape)
        return d_faces, None, None, None, None, None, None, None


class Cube2Equirec(nn.Module):
    """Same constructor and forward contract as the reference module (layers.py:41-116):
    forward(cube_feat[B,C,fw,6*fw]) -> [B,C,equ_h,equ_w]; faces side by side in slot order F R B L U D."""

    def __init__(self, face_w: int, equ_h: int, equ_w: int):
        super().__init__()
        self.face_w, self.equ_h, self.equ_w = face_w, equ_h, equ_w
        grid = torch.from_numpy(sample_grid_numpy(face_w, equ_h, equ_w)).view(1, 1, equ_h, equ_w, 3)
        self.sample_grid = nn.Parameter(grid, requires_grad=False)
        # the grid's inverse for the backward (not in the state dict: the reference module has only sample_grid)
        offsets, entries = adjoint_plan_numpy(face_w, equ_h, equ_w)
        self.register_buffer("plan_offsets", torch.from_numpy(offsets), persistent=False)
        self.register_buffer("plan_entries", torch.from_numpy(entries), persistent=False)

    def forward(self, cube_feat: Tensor) -> Tensor:
        bs, ch, h, w = cube_feat.shape
        assert h == self.face_w and w // 6 == self.face_w
        grid = self.sample_grid[0, 0]
        x = cube_feat.float().contiguous()
        fw = self.face_w
        strides = (fw, fw * 6 * fw, 6 * fw)
        return torch.stack([_Stitch.apply(x[b], grid, self.plan_offsets, self.plan_entries, None, strides, ch, fw) for b in range(bs)])

    def stitch_rendered(self, faces: Tensor) -> Tensor:
        """faces[6,C,fw,fw] in the reference's RENDERED order (top, front, left, back, right,
        bottom) -> ERP [C,equ_h,equ_w] = Cube2Equirec(change_order(faces)) without the flip /
        permute / concat copies (model_wrapper_erp.py:393-400)."""
        return _Stitch.apply(faces, self.sample_grid[0, 0], self.plan_offsets, self.plan_entries, CHANGE_ORDER_FACE_MAP, None,
                             int(faces.shape[1]), self.face_w)

    def stitch_distance_rendered(self, depth_faces: Tensor, fxfycxcy: Tensor, convention: str = "reference") -> Tensor:
        """z-depth faces[N,6,fw,fw] in the reference's RENDERED order (top, front, left, back, right, bottom) with per-face
        intrinsics fxfycxcy[N,6,4] (fx, fy, cx, cy in pixels, rendered order) -> ERP ray-distance panoramas [N,equ_h,equ_w]:
        Cube2Equirec(depth_to_distance_map_batch(change_order_batch(depth))) of model_wrapper_erp.py:445-463 in ONE kernel for all N
        panoramas, without the distance faces, the reordered copy or the intrinsics broadcast, and without writing to the input
        (change_order_batch flips faces 0 and 5 of its argument in place).  faces[6,fw,fw] with fxfycxcy[6,4] or [1,6,4] gives
        [equ_h,equ_w].  Bit-identical to depth_to_distance followed by the stitch; the backward has no atomics.
        convention="reference": the reference's lines as they are — the conversion happens AFTER the reorder with the intrinsics
          still in rendered order, so slot s uses fxfycxcy[:, s] and the slot-space texel position with u = the ROW index; the two
          flipped faces (0 and 5) therefore see (fw - 1 - u) - cx where their own image has u - cx.
        convention="pixel": each face is converted in its own image with its own intrinsics row before the reorder, x (column)
          with fx, cx and y (row) with fy, cy.
        The gradient with respect to a depth texel is the stitch's adjoint times sign(d) s, and 0 at d = 0 (finite, where torch's
        autograd of the reference's sqrt gives NaN).  fxfycxcy takes no gradient."""
        what = "stitch_distance_rendered"
        conv = _convention_code(convention)
        _check_gpu_f32(what, depth_faces=depth_faces, fxfycxcy=fxfycxcy)
        fw = self.face_w
        single = depth_faces.dim() == 3
        d = depth_faces[None] if single else depth_faces
        k = fxfycxcy[None] if single and fxfycxcy.dim() == 2 else fxfycxcy
        if d.dim() != 4 or tuple(d.shape[1:]) != (6, fw, fw):
            raise ValueError(f"{what}: depth_faces must be [N, 6, {fw}, {fw}] or [6, {fw}, {fw}], not {tuple(depth_faces.shape)}")
        if tuple(k.shape) != (d.shape[0], 6, 4):
            raise ValueError(f"{what}: fxfycxcy must be [{d.shape[0]}, 6, 4], not {tuple(fxfycxcy.shape)}")
        grid = self.sample_grid[0, 0]
        if grid.device != d.device:
            raise ValueError(f"{what}: depth_faces is on {d.device}, the module on {grid.device}")
        if d.shape[0] == 0:
            return torch.empty((0, self.equ_h, self.equ_w), dtype=torch.float32, device=d.device)
        erp = _StitchDistance.apply(d.contiguous(), k.detach().contiguous(), grid, self.plan_offsets, self.plan_entries,
                                    CHANGE_ORDER_FACE_MAP, conv)
        return erp[0] if single else erp
