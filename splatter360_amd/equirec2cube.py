"""Equirectangular -> cube resampling on the MI355X: the opposite direction of stitch.Cube2Equirec (replaces Equirec2Cube,
src/geometry/util.py:7-101, which the hm3d loader runs per frame on the host with numpy + scipy, and folds in the
reorder + flip that makes image_cubes_supervise, src/dataset/dataset_hm3d.py:204-213).

The coordinate plane is host-side numpy restated from util.py:26-69 (same float32 arithmetic, so it is bit-identical; pinned by
tests/golden/equirec2cube.npz); the gather is one HIP kernel for the whole batch, float64 inside, and applies the reference's pole
padding and scipy's mode='wrap' (period n - 1) itself.  The adjoint is a second gather over the plane's inverse (adjoint_plan, built
once per plane, boundary rule and mode here): no atomics, so gradients are bit-reproducible.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import torch
from torch import Tensor, nn

from ._call import call, ptr

# Output face j shows slot (F R B L U D) code & 7, flipped on both image axes when bit 3 is set (the encoding of
# stitch.CHANGE_ORDER_FACE_MAP, of which this is the inverse): rendered order U B L F R D, faces 0 and 5 flipped.
RENDERED_FACE_MAP = (4 | 8, 2, 3, 0, 1, 5 | 8)
MODES = {"bilinear": 0, "nearest": 1}
BOUNDARIES = {"reference": 0, "periodic": 1}


def _face_grid(face_w: int) -> np.ndarray:
    rng = np.linspace(-0.5, 0.5, num=face_w, dtype=np.float32)
    return np.stack(np.meshgrid(rng, -rng), -1)


@lru_cache(maxsize=8)
def coordinates_numpy(equ_h: int, equ_w: int, face_w: int) -> np.ndarray:
    """[fw, 6*fw, 2] float32 (coor_y, coor_x) = Equirec2Cube.coor_y / coor_x (util.py:26-69), faces side by side in slot order."""
    fw = face_w
    grid = _face_grid(fw)
    xyz = np.zeros((fw, fw * 6, 3), np.float32)
    xyz[:, 0 * fw:1 * fw, [0, 1]] = grid                 # front, z = 0.5
    xyz[:, 0 * fw:1 * fw, 2] = 0.5
    xyz[:, 1 * fw:2 * fw, [2, 1]] = grid[:, ::-1]        # right, x = 0.5
    xyz[:, 1 * fw:2 * fw, 0] = 0.5
    xyz[:, 2 * fw:3 * fw, [0, 1]] = grid[:, ::-1]        # back, z = -0.5
    xyz[:, 2 * fw:3 * fw, 2] = -0.5
    xyz[:, 3 * fw:4 * fw, [2, 1]] = grid                 # left, x = -0.5
    xyz[:, 3 * fw:4 * fw, 0] = -0.5
    xyz[:, 4 * fw:5 * fw, [0, 2]] = grid[::-1, :]        # up, y = 0.5
    xyz[:, 4 * fw:5 * fw, 1] = 0.5
    xyz[:, 5 * fw:6 * fw, [0, 2]] = grid                 # down, y = -0.5
    xyz[:, 5 * fw:6 * fw, 1] = -0.5
    x, y, z = np.split(xyz, 3, axis=-1)
    lon = np.arctan2(x, z)
    lat = np.arctan2(y, np.sqrt(x ** 2 + z ** 2))
    coor_x = (lon / (2 * np.pi) + 0.5) * equ_w - 0.5
    coor_y = (-lat / np.pi + 0.5) * equ_h - 0.5
    out = np.ascontiguousarray(np.concatenate([coor_y, coor_x], -1), dtype=np.float32)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=8)
def cosmap_numpy(face_w: int) -> np.ndarray:
    """[fw, 6*fw] float32 = Equirec2Cube.cosmaps[..., 0] (util.py:22-24): z-depth = distance * cosmap."""
    grid = _face_grid(face_w)
    cosmap = 1 / np.sqrt((2 * grid[..., 0]) ** 2 + (2 * grid[..., 1]) ** 2 + 1)
    out = np.ascontiguousarray(np.concatenate(6 * [cosmap], axis=1), dtype=np.float32)
    out.setflags(write=False)
    return out


def _wrap_taps(c: np.ndarray, n: int, nearest: bool) -> np.ndarray:
    """scipy's mode='wrap' on an axis of n samples: tap indices [N, K] (K = 1 nearest, 2 bilinear), as the kernel computes them."""
    c = c.astype(np.float64)
    s = float(n - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.where(c < 0, c + s * (np.trunc(-c / s) + 1), np.where(c > s, c - s * np.trunc(c / s), c))
        if nearest:
            idx = np.floor(c + 0.5)[:, None]
        else:
            i0 = np.floor(c)
            i1 = i0 + 1
            i1 = np.where(i1 > s, i1 - s * np.floor(i1 / s), i1)
            idx = np.stack([i0, i1], 1)
        return np.clip(np.nan_to_num(idx, nan=0.0), 0, n - 1).astype(np.int64)


def tap_texels(coor: np.ndarray, equ_h: int, equ_w: int, boundary: str = "reference", mode: str = "bilinear") -> np.ndarray:
    """[fw*6*fw, K*K] int64: the ERP texel row * W + col behind tap 2*ky + kx of every cube texel, pole-row taps folded onto
    their real texel — the kernel's index rule (csrc/s360_equirec2cube.hip e2c_taps), clamping included."""
    H, W = equ_h, equ_w
    c = np.ascontiguousarray(coor, dtype=np.float32).reshape(-1, 2)
    y, x = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
    nearest = MODES[mode] == 1
    if BOUNDARIES[boundary] == 0:
        py, px = _wrap_taps(y, H + 2, nearest), _wrap_taps(x, W, nearest)
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            cy = np.clip(np.nan_to_num(y, nan=-1.0), -1.0, float(H))
            cx = x - W * np.floor(x / W)
            y0 = np.floor(cy + 0.5) if nearest else np.floor(cy)
            x0 = np.floor(cx + 0.5) if nearest else np.floor(cx)
            r0 = y0.astype(np.int64)
            q0 = np.clip(np.nan_to_num(x0, nan=0.0), 0, W).astype(np.int64) % W
        r = r0[:, None] if nearest else np.stack([r0, np.minimum(r0 + 1, H)], 1)
        px = q0[:, None] if nearest else np.stack([q0, (q0 + 1) % W], 1)
        py = np.where(r < 0, H + 1, r)
    pole = py >= H
    row = np.where(py < H, py, np.where(py == H, H - 1, 0))
    col = np.where(pole[:, :, None], (px[:, None, :] - W // 2) % W, px[:, None, :])
    return (row[:, :, None] * W + col).reshape(c.shape[0], -1)


def adjoint_plan(coor: np.ndarray, equ_h: int, equ_w: int, boundary: str = "reference", mode: str = "bilinear"):
    """The inverse of a coordinate plane [fw, 6*fw, 2] (float32) over the [H, W] ERP plane, for s360_erp2cube_backward:
    (offsets int32 [H*W + 1], entries int32) — ERP texel e = row*W + col is read by entries[offsets[e]:offsets[e+1]] =
    cube_texel*4 + tap (tap = 2*ky + kx; 0 for nearest), sorted.  Every tap is listed once, weight 0 included, pole-row taps under
    the real texel they resolve to.  It does not depend on the face map."""
    tex = tap_texels(coor, equ_h, equ_w, boundary, mode)
    n, k = tex.shape
    if n * 4 > np.iinfo(np.int32).max or equ_h * equ_w + 1 > np.iinfo(np.int32).max:
        raise ValueError("equirec2cube adjoint plan: 24 * face_w**2 and equ_h * equ_w + 1 must fit in int32")
    ent = (np.arange(n, dtype=np.int64)[:, None] * 4 + (np.arange(4) if k == 4 else np.zeros(1, np.int64))[None, :]).reshape(-1)
    order = np.argsort(tex.reshape(-1), kind="stable")        # entries ascend already: stable keeps them sorted per texel
    offsets = np.zeros(equ_h * equ_w + 1, np.int64)
    np.cumsum(np.bincount(tex.reshape(-1), minlength=equ_h * equ_w), out=offsets[1:])
    return offsets.astype(np.int32), ent[order].astype(np.int32)


@lru_cache(maxsize=8)
def adjoint_plan_numpy(equ_h: int, equ_w: int, face_w: int, boundary: str = "reference", mode: str = "bilinear"):
    """adjoint_plan of coordinates_numpy(equ_h, equ_w, face_w), cached like the plane (4 int32 entries per cube texel)."""
    return adjoint_plan(coordinates_numpy(equ_h, equ_w, face_w), equ_h, equ_w, boundary, mode)


def _i32x6(face_map):
    return None if face_map is None else (C.c_int32 * 6)(*face_map)


def _launch_forward(x: Tensor, coor: Tensor, scale, out: Tensor, fw: int, mode: int, boundary: int, face_map, strides):
    b, c, h, w = x.shape
    call("s360_erp2cube_forward", x.device, ptr(x), ptr(coor), ptr(scale), ptr(out),
         b, c, h, w, fw, mode, boundary, int(x.dtype == torch.uint8), _i32x6(face_map),
         None if strides is None else (C.c_int64 * 4)(*strides))


class _Resample(torch.autograd.Function):
    """erp [B,C,H,W] float32 -> cube through `coor`; (plan_offsets, plan_entries) = adjoint_plan(coor, ...) on the same device.
    as_faces: write [B,6,C,fw,fw] (strided store) instead of [B,C,fw,6*fw]."""

    @staticmethod
    def forward(ctx, erp, coor, scale, plan_offsets, plan_entries, mode, boundary, face_map, as_faces):
        x = erp.detach().contiguous()
        b, c = int(x.shape[0]), int(x.shape[1])
        fw = int(coor.shape[0])
        strides = (6 * c * fw * fw, c * fw * fw, fw * fw, fw) if as_faces else None
        out = torch.empty((b, 6, c, fw, fw) if as_faces else (b, c, fw, 6 * fw), dtype=torch.float32, device=x.device)
        _launch_forward(x, coor, scale, out, fw, mode, boundary, face_map, strides)
        ctx.save_for_backward(coor, plan_offsets, plan_entries, *(() if scale is None else (scale,)))
        ctx.meta = (mode, boundary, face_map, strides, tuple(x.shape))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_cube):
        coor, offs, ents, *rest = ctx.saved_tensors
        mode, boundary, face_map, strides, (b, c, h, w) = ctx.meta
        if (offs.dtype, ents.dtype) != (torch.int32, torch.int32) or offs.numel() != h * w + 1 \
                or not (offs.is_cuda and ents.is_cuda and offs.is_contiguous() and ents.is_contiguous()):
            raise RuntimeError("equirec2cube backward: the adjoint plan does not belong to this plane / device")
        g = d_cube.detach().float().contiguous()
        d_erp = torch.empty((b, c, h, w), dtype=torch.float32, device=g.device)
        call("s360_erp2cube_backward", g.device, ptr(g), ptr(coor), ptr(rest[0]) if rest else None, ptr(offs),
             ptr(ents), ptr(d_erp), b, c, h, w,
             int(coor.shape[0]), mode, boundary, _i32x6(face_map),
             None if strides is None else (C.c_int64 * 4)(*strides))
        return d_erp, None, None, None, None, None, None, None, None


class Equirec2Cube(nn.Module):
    """The reference's Equirec2Cube (util.py:7-101) with its constructor order, on GPU tensors.  The input size is the module's:
    there is no cv2.resize branch (util.py:84-88) — resize before the call.  boundary="reference" reproduces the pole padding and
    scipy's mode='wrap' (period n - 1) bit for bit; "periodic" wraps x modulo equ_w and rolls the rows beyond the poles, which is
    what the padding was meant to do.  The two differ only at the centre row / column of a face of odd face_w."""

    def __init__(self, equ_h: int, equ_w: int, face_w: int, boundary: str = "reference"):
        super().__init__()
        if boundary not in BOUNDARIES:
            raise ValueError(f"boundary must be one of {sorted(BOUNDARIES)}")
        self.equ_h, self.equ_w, self.face_w, self.boundary = equ_h, equ_w, face_w, boundary
        self.register_buffer("coor", torch.from_numpy(coordinates_numpy(equ_h, equ_w, face_w).copy()), persistent=False)
        self.register_buffer("cosmaps", torch.from_numpy(cosmap_numpy(face_w).copy()), persistent=False)
        for mode in MODES:
            offsets, entries = adjoint_plan_numpy(equ_h, equ_w, face_w, boundary, mode)
            self.register_buffer(f"plan_offsets_{mode}", torch.from_numpy(offsets), persistent=False)
            self.register_buffer(f"plan_entries_{mode}", torch.from_numpy(entries), persistent=False)

    def _resample(self, erp: Tensor, mode: str, order, scale=None) -> Tensor:
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        if order not in (None, "slots", "rendered"):
            raise ValueError('order must be "slots" or "rendered"')
        if not erp.is_cuda:
            raise RuntimeError("ERP->cube resampling runs on the GPU only (no CPU path)")
        if erp.dim() != 4 or tuple(erp.shape[2:]) != (self.equ_h, self.equ_w):
            raise ValueError(f"expected erp[B,C,{self.equ_h},{self.equ_w}], got {tuple(erp.shape)}")
        face_map = RENDERED_FACE_MAP if order == "rendered" else None
        as_faces = order is not None
        m, bnd, fw = MODES[mode], BOUNDARIES[self.boundary], self.face_w
        if erp.dtype == torch.uint8:                    # the reference's uint8 image contract: uint8 out, no gradient
            if scale is not None:
                raise ValueError("a uint8 plane has no z-depth: pass a float distance map")
            x = erp.contiguous()
            b, c = int(x.shape[0]), int(x.shape[1])
            out = torch.empty((b, 6, c, fw, fw) if as_faces else (b, c, fw, 6 * fw), dtype=torch.uint8, device=x.device)
            strides = (6 * c * fw * fw, c * fw * fw, fw * fw, fw) if as_faces else None
            _launch_forward(x, self.coor, None, out, fw, m, bnd, face_map, strides)
            return out
        return _Resample.apply(erp.float(), self.coor, scale, getattr(self, f"plan_offsets_{mode}"),
                               getattr(self, f"plan_entries_{mode}"), m, bnd, face_map, as_faces)

    def forward(self, erp: Tensor, mode: str = "bilinear") -> Tensor:
        """erp[B,C,equ_h,equ_w] (float, or uint8 -> uint8) -> [B,C,fw,6*fw], faces side by side in slot order F R B L U D: what
        the reference's run() returns per image, channel-first.  Once differentiable in erp."""
        return self._resample(erp, mode, None)

    def faces(self, erp: Tensor, order: str = "slots", mode: str = "bilinear") -> Tensor:
        """-> [B,6,C,fw,fw], written directly.  order="slots": F R B L U D (image_cubes_input); "rendered": U B L F R D with faces
        0 and 5 flipped on both axes, the layout of image_cubes_supervise (dataset_hm3d.py:204-213) that the decoder renders and
        Cube2Equirec.stitch_rendered consumes."""
        return self._resample(erp, mode, order)

    def depth_faces(self, distance: Tensor, order: str = "slots") -> Tensor:
        """distance[B,1,equ_h,equ_w] (panoramic ray length) -> per-face z-depth [B,6,1,fw,fw]: nearest sampling times cosmaps
        (util.py:22-24,93-96)."""
        return self._resample(distance, "nearest", order, scale=self.cosmaps)

    def run(self, equ_img: Tensor, equ_dep: Tensor = None):
        """The reference's run() on GPU tensors, channel-last: equ_img[H,W,C] -> cube_img[fw,6*fw,C] (bilinear; uint8 stays uint8),
        and with equ_dep[H,W,D] also cube_dep[fw,6*fw,D] (nearest times cosmaps)."""
        cube_img = self.forward(equ_img.permute(2, 0, 1)[None])[0].permute(1, 2, 0)
        if equ_dep is None:
            return cube_img
        d = equ_dep.permute(2, 0, 1)[None]
        return cube_img, self._resample(d, "nearest", None, scale=self.cosmaps)[0].permute(1, 2, 0)
