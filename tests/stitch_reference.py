"""A float64 statement of the cube -> ERP stitch, in plain numpy: torch's 5-D grid_sample as the reference calls it
(trilinear, padding_mode="border", align_corners=True) over the [C, 6, fw, fw] slot-space volume, with the face map of
splatter360_amd.stitch folded in (slot s reads source face code & 7, flipped on both image axes when bit 3 is set).

- Each coordinate is unnormalised and clipped in float32, as the kernel and torch (float32 input) do: i = ((g + 1) / 2) * (size - 1),
  clipped to [0, size - 1].  `coord=np.float64` does the same in float64, which is what torch does for float64 input.
- The eight corner taps come in the kernel's order k = 4*dz + 2*dy + dx; weight (wx * wy) * wz with wx = (1 - fx, fx) in the
  coordinate's precision.
- A tap outside the volume is skipped; an in-range tap is always added, weight 0 included (inf * 0 = NaN, as in torch).
- Products and sums are float64.
"""
from __future__ import annotations

import numpy as np


def _unnorm_clip(g, size, dt):
    i = ((g.astype(dt) + dt(1)) / dt(2)) * dt(size - 1)
    return np.minimum(dt(size - 1), np.maximum(i, dt(0)))


def taps(grid, fw, coord=np.float32):
    """grid [..., 3] -> (texel [N, 8] int64 slot-space index z*fw*fw + y*fw + x, or -1 outside the volume; weight [N, 8] in `coord`
    precision, 0 outside; valid [N, 8] bool).  N = the grid's pixels in row-major order, taps in the kernel's order."""
    g = np.asarray(grid).reshape(-1, 3)
    dt = np.dtype(coord).type
    ix, iy, iz = _unnorm_clip(g[:, 0], fw, dt), _unnorm_clip(g[:, 1], fw, dt), _unnorm_clip(g[:, 2], 6, dt)
    x0f, y0f, z0f = np.floor(ix), np.floor(iy), np.floor(iz)
    fx, fy, fz = ix - x0f, iy - y0f, iz - z0f
    wx = np.stack([dt(1) - fx, fx], 1)
    wy = np.stack([dt(1) - fy, fy], 1)
    wz = np.stack([dt(1) - fz, fz], 1)
    x0, y0, z0 = x0f.astype(np.int64), y0f.astype(np.int64), z0f.astype(np.int64)
    n = g.shape[0]
    tex = np.full((n, 8), -1, np.int64)
    w = np.zeros((n, 8), dt)
    valid = np.zeros((n, 8), bool)
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                k = 4 * dz + 2 * dy + dx
                x, y, z = x0 + dx, y0 + dy, z0 + dz
                ok = (x >= 0) & (x < fw) & (y >= 0) & (y < fw) & (z >= 0) & (z <= 5)
                valid[:, k] = ok
                tex[ok, k] = (z[ok] * fw + y[ok]) * fw + x[ok]
                w[ok, k] = (wx[ok, dx] * wy[ok, dy]) * wz[ok, dz]
    return tex, w, valid


def _codes(face_map):
    return [(s, False) for s in range(6)] if face_map is None else [(c & 7, bool(c & 8)) for c in face_map]


def slot_volume(faces, face_map=None):
    """faces [6, C, fw, fw] in source order -> the [6, C, fw, fw] volume grid_sample sees (slot order, flips applied)."""
    faces = np.asarray(faces)
    return np.stack([faces[src][..., ::-1, ::-1] if fl else faces[src] for src, fl in _codes(face_map)])


def forward64(faces, grid, face_map=None, coord=np.float32, tp=None):
    """faces [6, C, fw, fw] (source order), grid [eh, ew, 3] -> ERP [C, eh, ew] float64.  tp: taps(grid, fw, coord) if at hand."""
    faces = np.asarray(faces, np.float64)
    c, fw = faces.shape[1], faces.shape[2]
    eh, ew = grid.shape[0], grid.shape[1]
    tex, w, valid = taps(grid, fw, coord) if tp is None else tp
    vol = np.ascontiguousarray(slot_volume(faces, face_map).transpose(0, 2, 3, 1).reshape(-1, c))   # [6*fw*fw, C]
    out = np.zeros((tex.shape[0], c), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(8):                                                      # the kernel's (and torch's) tap order
            ok = valid[:, k]
            out[ok] += vol[tex[ok, k]] * w[ok, k, None].astype(np.float64)
    return np.ascontiguousarray(out.T).reshape(c, eh, ew)


def adjoint64(d_erp, grid, face_map=None, fw=None, coord=np.float32, tp=None):
    """The explicit transpose of forward64: d_erp [C, eh, ew] -> d_faces [6, C, fw, fw] float64 in source order."""
    d_erp = np.asarray(d_erp, np.float64)
    c = d_erp.shape[0]
    tex, w, valid = taps(grid, fw, coord) if tp is None else tp
    g = d_erp.reshape(c, -1)
    pix = np.broadcast_to(np.arange(tex.shape[0])[:, None], tex.shape)[valid]
    t, wt = tex[valid], w[valid].astype(np.float64)
    d_vol = np.zeros((c, 6 * fw * fw), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for ch in range(c):
            np.add.at(d_vol[ch], t, g[ch, pix] * wt)
    d_vol = d_vol.reshape(c, 6, fw, fw).transpose(1, 0, 2, 3)                  # slot order
    d_faces = np.zeros_like(d_vol)
    for s, (src, fl) in enumerate(_codes(face_map)):
        d_faces[src] += d_vol[s][..., ::-1, ::-1] if fl else d_vol[s]
    return d_faces


def abs_forward64(faces, grid, face_map=None, tp=None):
    """sum_k |v_k * w_k| per ERP pixel: the scale of the forward's rounding error."""
    return forward64(np.abs(np.asarray(faces, np.float64)), grid, face_map, tp=tp)


def abs_adjoint64(d_erp, grid, face_map=None, fw=None, tp=None):
    """sum |g * w| per texel: the scale of the adjoint's rounding error."""
    return adjoint64(np.abs(np.asarray(d_erp, np.float64)), grid, face_map, fw, tp=tp)


def texel_coord(fw, slot, y, x):
    """The grid value (u, v, face-z) that lands exactly on texel (y, x) of slot `slot` (float32)."""
    c = lambda i: 2 * i / max(fw - 1, 1) - 1
    return np.float32([c(x), c(y), slot / 2.5 - 1])


def synthetic_grid(rng, eh, ew, fw):
    """A grid [eh, ew, 3] with coordinates in and beyond [-1, 1] (clipped), exactly +-1 and +-1.5, exact texel centres, and
    face coordinates that are the stitch grid's own face values (an exact integer face, or within rounding of one) or one ulp
    either side of them."""
    g = rng.uniform(-1.3, 1.3, (eh, ew, 3)).astype(np.float32)
    n = eh * ew
    flat = g.reshape(-1, 3)
    pick = rng.choice(n, n // 2, replace=False)
    q = len(pick) // 5
    flat[pick[:q], rng.integers(0, 3, q)] = rng.choice(np.float32([-1, 1, -1.5, 1.5]), q)
    flat[pick[q:2 * q], :2] = (2 * rng.integers(0, fw, (q, 2)) / max(fw - 1, 1) - 1).astype(np.float32)
    zf = (np.arange(6, dtype=np.float32) / np.float32(2.5) - 1).astype(np.float32)     # the stitch grid's face-z values
    flat[pick[2 * q:3 * q], 2] = rng.choice(zf, q)
    flat[pick[3 * q:4 * q], 2] = np.nextafter(rng.choice(zf, q), np.float32(2))
    flat[pick[4 * q:], 2] = np.nextafter(rng.choice(zf, len(pick) - 4 * q), np.float32(-2))
    return g


def invert_taps(grid, fw):
    """Brute-force inverse of taps(): for each slot-space texel the list of pixel*8 + tap that read it, in pixel order."""
    tex, _, valid = taps(grid, fw)
    out = [[] for _ in range(6 * fw * fw)]
    for p in range(tex.shape[0]):
        for k in range(8):
            if valid[p, k]:
                out[tex[p, k]].append(p * 8 + k)
    return out
