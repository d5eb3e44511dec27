"""A float64 statement of the z-depth -> ray distance map and of the fused depth-faces -> ERP distance stitch, in plain numpy.

distance = |d| s,  s = sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1),  gradient = g sign(d) s (0 at d = 0), all in float64 from
the float32 inputs.  d = 0 gives 0, a negative d gives |d| s, inf and NaN propagate.

- convention "reference": u is the ROW index and v the column index (what the reference's "ij" meshgrid pairs with cx / fx and
  cy / fy); square maps only.  In the fused stitch the conversion happens in SLOT space, after the reorder: slot s uses row s of
  the [6, 4] intrinsics and the slot-space texel position.
- convention "pixel": u is the column and v the row; any map shape.  In the fused stitch each face is converted in its own image with
  its own row, before the reorder.

The stitch itself is tests/stitch_reference.py's forward64 / adjoint64 with the face map of splatter360_amd.stitch.
"""
from __future__ import annotations

import numpy as np

import stitch_reference as SR

CONVENTIONS = ("reference", "pixel")
CHANGE_ORDER_FACE_MAP = (3, 4, 1, 2, 0 | 8, 5 | 8)     # splatter360_amd.stitch.CHANGE_ORDER_FACE_MAP


def scale64(k4, h, w, convention="reference"):
    """k4 [N, 4] (fx, fy, cx, cy) -> s [N, h, w] float64."""
    if convention not in CONVENTIONS:
        raise ValueError(convention)
    if convention == "reference" and h != w:
        raise ValueError("the reference convention needs square maps")
    k4 = np.asarray(k4, np.float64).reshape(-1, 4)
    row, col = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = (row, col) if convention == "reference" else (col, row)
    fx, fy, cx, cy = (k4[:, i, None, None] for i in range(4))
    a, b = (u[None] - cx) / fx, (v[None] - cy) / fy
    return np.sqrt(a * a + b * b + 1.0)


def distance64(depth, k4, convention="reference"):
    """depth [N, h, w] -> distance [N, h, w] float64."""
    d = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.abs(d) * scale64(k4, d.shape[-2], d.shape[-1], convention)


def distance_grad64(g, depth, k4, convention="reference"):
    """d(distance)/d(depth) applied to g: g sign(d) s, 0 at d = 0."""
    d = np.asarray(depth, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(g, np.float64) * (np.sign(d) * scale64(k4, d.shape[-2], d.shape[-1], convention))


def reorder(faces, face_map=CHANGE_ORDER_FACE_MAP):
    """faces [N, 6, h, w] in rendered order -> slot order with the flips applied (change_order_batch without the in-place write)."""
    return np.stack([SR.slot_volume(f[:, None], face_map)[:, 0] for f in np.asarray(faces)])


def unreorder(slots, face_map=CHANGE_ORDER_FACE_MAP):
    """The inverse of reorder for a permutation face map: slot-space [N, 6, h, w] -> rendered order."""
    slots = np.asarray(slots)
    out = np.zeros_like(slots)
    for s, code in enumerate(face_map):
        out[:, code & 7] = slots[:, s, ::-1, ::-1] if code & 8 else slots[:, s]
    return out


def slot_distance64(depth_faces, k4, convention="reference", face_map=CHANGE_ORDER_FACE_MAP):
    """depth_faces [N, 6, fw, fw] (rendered order), k4 [N, 6, 4] (rendered order) -> the slot-space distance volume [N, 6, fw, fw]
    float64 that the stitch samples."""
    d = np.asarray(depth_faces)
    n, fw = d.shape[0], d.shape[-1]
    k4 = np.asarray(k4).reshape(n * 6, 4)
    if convention == "reference":       # reorder first, then convert slot s with row s at the slot-space position
        return distance64(reorder(d, face_map).reshape(n * 6, fw, fw), k4, "reference").reshape(n, 6, fw, fw)
    return reorder(distance64(d.reshape(n * 6, fw, fw), k4, "pixel").reshape(n, 6, fw, fw), face_map)


def slot_scale64(k4, n, fw, convention="reference", face_map=CHANGE_ORDER_FACE_MAP):
    """sign-free d(slot distance)/d|d| in RENDERED face order [N, 6, fw, fw]: the s each rendered texel is multiplied by."""
    k4 = np.asarray(k4).reshape(n * 6, 4)
    s = scale64(k4, fw, fw, convention).reshape(n, 6, fw, fw)
    return unreorder(s, face_map) if convention == "reference" else s


def stitch_distance64(depth_faces, k4, grid, convention="reference", face_map=CHANGE_ORDER_FACE_MAP, tp=None):
    """-> ERP distance [N, eh, ew] float64 (products and sums in float64 over the float64 slot distances)."""
    vol = slot_distance64(depth_faces, k4, convention, face_map)
    return np.stack([SR.forward64(v[:, None], grid, None, tp=tp)[0] for v in vol])


def stitch_distance_grad64(d_erp, depth_faces, k4, grid, convention="reference", face_map=CHANGE_ORDER_FACE_MAP, tp=None):
    """-> d_depth_faces [N, 6, fw, fw] float64 in rendered order."""
    d = np.asarray(depth_faces, np.float64)
    n, fw = d.shape[0], d.shape[-1]
    d_slots = np.stack([SR.adjoint64(g[None], grid, None, fw, tp=tp)[:, 0] for g in np.asarray(d_erp, np.float64)])
    with np.errstate(invalid="ignore", over="ignore"):
        return unreorder(d_slots, face_map) * (np.sign(d) * slot_scale64(k4, n, fw, convention, face_map))


def ulp32(x):
    """The float32 spacing at the float64 value x (finite x)."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, np.finfo(np.float32).tiny)))
    return np.maximum(2.0 ** (e - 23), 2.0 ** -149)
