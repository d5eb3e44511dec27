"""A float64 statement of the equirectangular -> cube resampling, in plain numpy: the reference's Equirec2Cube
(src/geometry/util.py:7-101) restated rule by rule, and the truly periodic boundary rule beside it, each with its adjoint.

1. Coordinates: coor_y, coor_x [fw, 6 fw] float32 from the unit cube's xyz (float32) through arctan2 (float32) and the float64
   scalars of 2 pi / pi: the reference's own mix.  Six faces side by side in slot order F R B L U D.
2. Pole padding: the ERP plane [H, W] gets row H = row H-1 rolled by W // 2 and row H+1 = row 0 rolled by W // 2
   (pad[x] = row[(x - W // 2) mod W]).
3. scipy's mode='wrap' on both axes, n = H + 2 rows and n = W columns, period n - 1:
       s = n - 1;  c < 0: c += s (trunc(-c / s) + 1);  c > n - 1: c -= s trunc(c / s)
   bilinear: i0 = floor(c), upper weight c - i0, i1 = i0 + 1 and, if i1 > n - 1, i1 -= s (i1 // s);  nearest: floor(c + 0.5).
4. float64: t = 0; t += (v * wy) * wx over (ky, kx) = (0,0) (0,1) (1,0) (1,1), wy = (1 - fy, fy).  uint8 in, uint8 out:
   floor(t + 0.5) clipped to 0..255.
5. Depth: nearest sampling times cosmaps (float32, 1 / sqrt((2 gx)^2 + (2 gy)^2 + 1) of the face grid, tiled six times).

The periodic rule ("periodic"): x modulo W with taps floor(x) mod W and (floor(x) + 1) mod W; y held in [-1, H], row -1 = row 0
rolled by W // 2, row H = row H-1 rolled by W // 2.
"""
from __future__ import annotations

import numpy as np

RENDERED = (4 | 8, 2, 3, 0, 1, 5 | 8)    # output face j shows slot code & 7, flipped on both axes if bit 3: U B L F R D


def coordinates(equ_h, equ_w, face_w):
    """(coor_y, coor_x) [fw, 6 fw] float32 (util.py:26-69)."""
    f32 = np.float32
    xyz = np.zeros((face_w, face_w * 6, 3), f32)
    rng = np.linspace(-0.5, 0.5, num=face_w, dtype=f32)
    grid = np.stack(np.meshgrid(rng, -rng), -1)
    fw = face_w
    xyz[:, 0 * fw:1 * fw, [0, 1]] = grid
    xyz[:, 0 * fw:1 * fw, 2] = 0.5
    xyz[:, 1 * fw:2 * fw, [2, 1]] = grid[:, ::-1]
    xyz[:, 1 * fw:2 * fw, 0] = 0.5
    xyz[:, 2 * fw:3 * fw, [0, 1]] = grid[:, ::-1]
    xyz[:, 2 * fw:3 * fw, 2] = -0.5
    xyz[:, 3 * fw:4 * fw, [2, 1]] = grid
    xyz[:, 3 * fw:4 * fw, 0] = -0.5
    xyz[:, 4 * fw:5 * fw, [0, 2]] = grid[::-1, :]
    xyz[:, 4 * fw:5 * fw, 1] = 0.5
    xyz[:, 5 * fw:6 * fw, [0, 2]] = grid
    xyz[:, 5 * fw:6 * fw, 1] = -0.5
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    lon = np.arctan2(x, z)
    lat = np.arctan2(y, np.sqrt(x ** 2 + z ** 2))
    coor_x = (lon / (2 * np.pi) + 0.5) * equ_w - 0.5
    coor_y = (-lat / np.pi + 0.5) * equ_h - 0.5
    return coor_y, coor_x


def cosmap(face_w):
    """cosmaps [fw, 6 fw] float32 (util.py:22-24)."""
    rng = np.linspace(-0.5, 0.5, num=face_w, dtype=np.float32)
    grid = np.stack(np.meshgrid(rng, -rng), -1)
    c = 1 / np.sqrt((2 * grid[..., 0]) ** 2 + (2 * grid[..., 1]) ** 2 + 1)
    return np.concatenate(6 * [c], axis=1)


def _wrap_axis(c, n, nearest):
    """scipy's 'wrap' on n samples -> (i [N, K] int64, upper weight f [N] float64); K = 1 for nearest."""
    c = np.asarray(c, np.float64).copy()
    s = float(n - 1)
    lo, hi = c < 0, c > n - 1
    c[lo] += s * (np.trunc(-c[lo] / s) + 1)
    c[hi] -= s * np.trunc(c[hi] / s)
    if nearest:
        return np.floor(c + 0.5).astype(np.int64)[:, None], np.zeros_like(c)
    i0 = np.floor(c)
    f = c - i0
    i0 = i0.astype(np.int64)
    i1 = i0 + 1
    over = i1 > n - 1
    i1[over] -= (n - 1) * (i1[over] // (n - 1))
    return np.stack([i0, i1], 1), f


def taps(coor_y, coor_x, equ_h, equ_w, mode="bilinear", boundary="reference"):
    """Per cube texel (row-major over [fw, 6 fw]) its taps, pole rows folded onto the real plane:
    (texel [N, K*K] int64 = row * W + col, wy [N, K*K], wx [N, K*K] float64, pole [N, K*K] bool), tap k = 2 ky + kx; K = 2 for
    bilinear, 1 for nearest."""
    H, W = equ_h, equ_w
    y = np.asarray(coor_y, np.float32).reshape(-1).astype(np.float64)
    x = np.asarray(coor_x, np.float32).reshape(-1).astype(np.float64)
    nearest = mode == "nearest"
    assert mode in ("bilinear", "nearest") and boundary in ("reference", "periodic")
    if boundary == "reference":
        py, fy = _wrap_axis(y, H + 2, nearest)          # padded rows: H = row H-1 rolled, H+1 = row 0 rolled
        px, fx = _wrap_axis(x, W, nearest)
    else:
        cy = np.clip(y, -1.0, float(H))
        cx = x - W * np.floor(x / W)
        if nearest:
            r, q = np.floor(cy + 0.5).astype(np.int64)[:, None], np.floor(cx + 0.5).astype(np.int64)[:, None] % W
            fy, fx = np.zeros_like(cy), np.zeros_like(cx)
        else:
            y0, x0 = np.floor(cy), np.floor(cx)
            fy, fx = cy - y0, cx - x0
            r = np.stack([y0.astype(np.int64), np.minimum(y0.astype(np.int64) + 1, H)], 1)
            q = np.stack([x0.astype(np.int64) % W, (x0.astype(np.int64) + 1) % W], 1)
        py, px = np.where(r < 0, H + 1, r), q           # row -1 is the padded plane's row H+1
    K = 1 if nearest else 2
    n = y.shape[0]
    tex = np.zeros((n, K * K), np.int64)
    wy = np.zeros((n, K * K))
    wx = np.zeros((n, K * K))
    pole = np.zeros((n, K * K), bool)
    wys, wxs = (np.ones_like(fy),) if nearest else (1.0 - fy, fy), (np.ones_like(fx),) if nearest else (1.0 - fx, fx)
    for ky in range(K):
        p = py[:, ky] >= H
        row = np.where(py[:, ky] < H, py[:, ky], np.where(py[:, ky] == H, H - 1, 0))
        for kx in range(K):
            col = np.where(p, (px[:, kx] - W // 2) % W, px[:, kx])
            k = K * ky + kx
            tex[:, k], wy[:, k], wx[:, k], pole[:, k] = row * W + col, wys[ky], wxs[kx], p
    return tex, wy, wx, pole


def forward64(erp, coor_y, coor_x, mode="bilinear", boundary="reference", scale=None, tp=None):
    """erp [..., H, W] -> cube [..., fw, 6 fw] float64, summed in scipy's order; scale [fw, 6 fw] multiplies the result."""
    erp = np.asarray(erp)
    H, W = erp.shape[-2:]
    tex, wy, wx, _ = taps(coor_y, coor_x, H, W, mode, boundary) if tp is None else tp
    flat = erp.reshape(-1, H * W).astype(np.float64)
    out = np.zeros((flat.shape[0], tex.shape[0]))
    for k in range(tex.shape[1]):
        out += flat[:, tex[:, k]] if mode == "nearest" else (flat[:, tex[:, k]] * wy[None, :, k]) * wx[None, :, k]
    if scale is not None:
        out = out * np.asarray(scale, np.float32).reshape(-1).astype(np.float64)[None]
    return out.reshape(erp.shape[:-2] + np.shape(coor_y)[-2:])


def to_uint8(t):
    """scipy's uint8 output: floor(t + 0.5) clipped to 0..255 (rule 4)."""
    return np.clip(np.floor(np.asarray(t, np.float64) + 0.5), 0, 255).astype(np.uint8)


def adjoint64(d_cube, coor_y, coor_x, equ_h, equ_w, mode="bilinear", boundary="reference", scale=None, tp=None, absolute=False):
    """The explicit transpose of forward64: d_cube [..., fw, 6 fw] -> d_erp [..., H, W] float64.  absolute=True sums |term| instead:
    the scale of the sum's rounding error."""
    d_cube = np.asarray(d_cube, np.float64)
    tex, wy, wx, _ = taps(coor_y, coor_x, equ_h, equ_w, mode, boundary) if tp is None else tp
    g = d_cube.reshape(-1, tex.shape[0])
    if scale is not None:
        g = g * np.asarray(scale, np.float32).reshape(-1).astype(np.float64)[None]
    out = np.zeros((g.shape[0], equ_h * equ_w))
    for p in range(g.shape[0]):
        for k in range(tex.shape[1]):
            term = g[p] if mode == "nearest" else (g[p] * wy[:, k]) * wx[:, k]
            np.add.at(out[p], tex[:, k], np.abs(term) if absolute else term)
    return out.reshape(d_cube.shape[:-2] + (equ_h, equ_w))


def read_counts(coor_y, coor_x, equ_h, equ_w, mode="bilinear", boundary="reference"):
    """[H, W] int: how many taps read each ERP texel."""
    tex = taps(coor_y, coor_x, equ_h, equ_w, mode, boundary)[0]
    return np.bincount(tex.reshape(-1), minlength=equ_h * equ_w).reshape(equ_h, equ_w)


def split_faces(cube, order="slots"):
    """cube [..., C, fw, 6 fw] -> faces [..., 6, C, fw, fw]; "rendered": the reorder + flip of dataset_hm3d.py:204-213."""
    cube = np.asarray(cube)
    fw = cube.shape[-2]
    f = np.stack([cube[..., s * fw:(s + 1) * fw] for s in range(6)], -4)
    if order == "slots":
        return f
    assert order == "rendered"
    return np.stack([f[..., c & 7, :, ::-1, ::-1] if c & 8 else f[..., c & 7, :, :, :] for c in RENDERED], -4)


def join_faces(faces, order="slots"):
    """The inverse (and, being a permutation, the transpose) of split_faces."""
    faces = np.asarray(faces)
    slots = [None] * 6
    for j, c in enumerate(RENDERED if order == "rendered" else range(6)):
        slots[c & 7] = faces[..., j, :, ::-1, ::-1] if c & 8 else faces[..., j, :, :, :]
    return np.concatenate(slots, -1)


def invert_taps(coor_y, coor_x, equ_h, equ_w, mode="bilinear", boundary="reference"):
    """Brute-force inverse of taps(): per ERP texel the sorted list of cube_texel * 4 + tap that read it (tap = 2 ky + kx)."""
    tex = taps(coor_y, coor_x, equ_h, equ_w, mode, boundary)[0]
    out = [[] for _ in range(equ_h * equ_w)]
    for t in range(tex.shape[0]):
        for k in range(tex.shape[1]):
            out[tex[t, k]].append(t * 4 + k)
    return [sorted(v) for v in out]
