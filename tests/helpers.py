"""Shared scene builders for the tests (CPU-only; uses the product's camera helpers)."""
from __future__ import annotations

import numpy as np
import torch

from splatter360_amd import cameras, synthetic


def face_settings(face: int, h: int, w: int, near=0.1, far=10.0, position=(0.0, 0.0, 0.0), bg=(0.0, 0.0, 0.0)):
    """GaussianRasterizationSettings fields (numpy) of one cube face, built the way the reference
    builds them (cuda_splatting.py:64-112) for a panorama at `position` with identity rotation."""
    pano = torch.from_numpy(synthetic.target_pano_pose(position))[None]
    ext = cameras.cube_face_extrinsics(pano)[0, face][None]
    k = cameras.cube_face_intrinsics(1)[0, face][None]
    vs = cameras.view_setup(ext, k, torch.tensor([near]), torch.tensor([far]))
    return dict(image_height=h, image_width=w, tanfovx=float(vs["tan_fov_x"][0]),
                tanfovy=float(vs["tan_fov_y"][0]), bg=np.asarray(bg, np.float32),
                viewmatrix=vs["view_matrix"][0].numpy(), projmatrix=vs["full_projection"][0].numpy(),
                sh_degree=4, campos=vs["campos"][0].numpy(), scale=float(vs["scale"][0]))


def settings_from_views(views, i: int, h: int, w: int, sh_degree: int = 4):
    """The same GaussianRasterizationSettings fields, read back from row i of a packed S360View tensor [V,44] — so
    that the oracle sees bit-identical camera records to the HIP path whichever glue (torch ops or the one-kernel
    s360_pack_views) produced them."""
    r = views[i].detach().cpu().numpy().astype(np.float32)
    return dict(image_height=h, image_width=w, tanfovx=float(r[35]), tanfovy=float(r[36]), bg=r[37:40].copy(),
                viewmatrix=r[0:16].reshape(4, 4).copy(), projmatrix=r[16:32].reshape(4, 4).copy(), sh_degree=sh_degree,
                campos=r[32:35].copy(), scale=float(r[40]))


def boundary_tensors(cloud: dict, scale: float):
    """means3D, cov6, shs[G,n,3], opacities[G,1] exactly as render_cuda hands them over
    (cuda_splatting.py:68-75,115-123)."""
    means = cloud["means"] * np.float32(scale)
    cov = cloud["covariances"] * np.float32(scale) ** 2
    r, c = np.triu_indices(3)
    cov6 = np.ascontiguousarray(cov[:, r, c])
    shs = np.ascontiguousarray(cloud["harmonics"].transpose(0, 2, 1))
    return means.astype(np.float32), cov6.astype(np.float32), shs.astype(np.float32), cloud["opacities"][:, None].astype(np.float32)


def small_front_scene(n=40, seed=0, h=64, w=64, d_sh=25, spread=0.6, zrange=(2.0, 6.0), srange=(0.03, 0.25)):
    """A handful of well-conditioned Gaussians in front of an identity camera (tanfov 1), as
    already-scaled boundary tensors.  Used for finite-difference and known-answer tests."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(*zrange, n)
    xy = rng.uniform(-spread, spread, (n, 2)) * z[:, None]
    means = np.concatenate([xy, z[:, None]], 1)
    s = np.exp(rng.uniform(np.log(srange[0]), np.log(srange[1]), (n, 3)))
    r = synthetic._random_rotations(rng, n)
    cov = np.einsum("nij,nj,nkj->nik", r, s * s, r)
    rr, cc = np.triu_indices(3)
    cov6 = cov[:, rr, cc]
    shs = rng.standard_normal((n, d_sh, 3)) * synthetic.sh_band_mask(d_sh)[None, :, None] * 3
    shs[:, 0, :] = rng.uniform(0.2, 1.5, (n, 3))
    opac = rng.uniform(0.2, 0.95, (n, 1))
    near, far = 1.0, 100.0
    proj = cameras.get_projection_matrix(torch.tensor([near]), torch.tensor([far]), torch.tensor([np.pi / 2]), torch.tensor([np.pi / 2]))[0].numpy().astype(np.float64)
    view = np.eye(4)
    settings = dict(image_height=h, image_width=w, tanfovx=1.0, tanfovy=1.0, bg=np.array([0.1, 0.2, 0.3]),
                    viewmatrix=view.T.copy(), projmatrix=(view.T @ proj.T).copy(), sh_degree=int(round(np.sqrt(d_sh))) - 1,
                    campos=np.zeros(3))
    return settings, means, cov6, shs, opac


def check_instance_slots(slot_base, slot_pair, tiles_touched, L):
    """Training state that replaces upstream's point_offsets scan: every visible pair owns `touched` consecutive
    instance slots starting at slot_base[pair]; the ranges tile [0, L) exactly and slot_pair is their owner table.
    (Which range a pair gets is run-dependent: k_emit reserves block-wise with one atomic per block.)"""
    import numpy as np
    base = np.asarray(slot_base).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    tt = np.asarray(tiles_touched).reshape(-1).astype(np.int64)
    vis = np.nonzero(tt > 0)[0]
    assert tt.sum() == L
    if L == 0:
        return
    order = np.argsort(base[vis], kind="stable")
    b, n = base[vis][order], tt[vis][order]
    assert b[0] == 0 and (b[1:] == (b + n)[:-1]).all() and (b + n)[-1] == L
    owner = np.repeat(vis[order], n)
    sp = np.asarray(slot_pair).reshape(-1)[:L].astype(np.int64) & 0xFFFFFFFF
    np.testing.assert_array_equal(sp & 0x7FFFFFFF, owner)
    np.testing.assert_array_equal(sp >> 31, (tt[owner] > 32).astype(np.int64))      # bit 31: a slot of a pair that owns more than 32


# ------------------------------------------------------------------------------ split lists: host model + designed scenes
# Mirrors of the constants of S360_FLAG_SPLIT_LISTS (splatter360_amd/csrc/s360_device.h, s360_forward.hip); tests/test_split_model.py
# pins them to the sources, so that a retune cannot silently desynchronise the model below.
SORT_SHORT, SORT_CHUNK = 2048, 4096
SEG_HEAD, SEG_LEN, SEG_MIN_REST = 1024, 512, 512
SEG_PER_CHUNK, SEG_K0 = SORT_CHUNK // SEG_LEN, SEG_HEAD // SEG_LEN
SEG_T_FAR = 1.0 / 16.0
SUB_W = 8                      # four 8x8 quadrants per 16x16 tile: quadrant w has its origin at (8 (w & 1), 8 (w >> 1))
SPLIT_MARGIN = 0.02            # |T / SEG_T_FAR - 1| below this: the decision may fall either way in float32 (one 1/255 accept flip is 0.4 %)


def seg_slots(cap: int) -> int:
    """s360_device.h seg_slots: the segment slots of a call without S360Params.max_segments."""
    return SEG_PER_CHUNK * (cap // 2048 + 1)


def chunk_table(ranges):
    """k_tile_scan's chunk_start[]: sort chunks of the lists longer than SORT_SHORT in front of every tile (tile index order)."""
    import numpy as np
    n = np.diff(np.asarray(ranges, np.int64), axis=1)[:, 0]
    nch = np.where(n > SORT_SHORT, (n + SORT_CHUNK - 1) // SORT_CHUNK, 0)
    return np.concatenate([[0], np.cumsum(nch)]).astype(np.int64)


def split_model(ranges, values, xy, conic_opacity, h: int, w: int, n_slots: int):
    """Host model of k_render's hand-over decision (s360_forward.hip, the `split_at` / SEG_T_FAR test) for one call of V images.

    ranges / values / xy / conic_opacity: tile ranges over the call's global tile index t = v T + tile (T tiles per image, image-major,
    as k_tile_scan numbers them — chunk_start runs across the images), the sorted list of record indices, and per record its pixel
    centre and conic + opacity (one image: the oracle's forward outputs; V images: the per-image records stacked, v P + g).
    A (tile, quadrant) hands the rest of its list over iff the list has more than SORT_SHORT and at least SEG_HEAD + SEG_MIN_REST
    entries, some pixel of the quadrant inside the image has not stopped and has T >= SEG_T_FAR after the first SEG_HEAD entries
    (the oracle's alpha / stop rule, float64), and the tile's segments fit: SEG_PER_CHUNK chunk_start[t] + ceil(n / SEG_LEN) <= n_slots.
    Returns dict(split=[tiles, 4] bool, clear=[tiles, 4] bool — False where T lands within SPLIT_MARGIN of SEG_T_FAR —, t_far=[tiles, 4]
    the largest live transmittance after the head (0 where none), n_split (header[5]), n_items (header[6]), chunk_start)."""
    import numpy as np
    ranges = np.asarray(ranges, np.int64)
    nt = ranges.shape[0]
    gx = (w + 15) // 16
    T_img = gx * ((h + 15) // 16)
    assert nt % T_img == 0
    cs = chunk_table(ranges)
    split = np.zeros((nt, 4), bool)
    clear = np.ones((nt, 4), bool)
    t_far = np.zeros((nt, 4))
    n_items = 0
    xy = np.asarray(xy, np.float64)
    co = np.asarray(conic_opacity, np.float64)
    for t in range(nt):
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        n = e - s
        if not (n > SORT_SHORT and n >= SEG_HEAD + SEG_MIN_REST):
            continue
        ids = np.asarray(values[s:s + SEG_HEAD], np.int64)
        ty, tx = divmod(t % T_img, gx)
        fits = SEG_PER_CHUNK * int(cs[t]) + (n + SEG_LEN - 1) // SEG_LEN <= n_slots
        for q in range(4):
            lx, ly = np.meshgrid(np.arange(SUB_W), np.arange(64 // SUB_W))
            px = (tx * 16 + 8 * (q & 1) + lx).reshape(-1)
            py = (ty * 16 + 8 * (q >> 1) + ly).reshape(-1)
            inside = (px < w) & (py < h)
            if not inside.any():
                continue
            px, py = px[inside].astype(np.float64), py[inside].astype(np.float64)
            dx = xy[ids, 0][:, None] - px[None]
            dy = xy[ids, 1][:, None] - py[None]
            c = co[ids]
            power = -0.5 * (c[:, 0:1] * dx * dx + c[:, 2:3] * dy * dy) - c[:, 1:2] * dx * dy
            alpha = np.minimum(0.99, c[:, 3:4] * np.exp(power))
            alpha = np.where((power > 0) | (alpha < 1.0 / 255.0), 0.0, alpha)
            T = np.prod(1.0 - alpha, axis=0)           # monotone: a pixel stopped in the head iff its full product fell below 1e-4
            live = T >= 1e-4
            tf = float(T[live].max()) if live.any() else 0.0
            t_far[t, q] = tf
            clear[t, q] = abs(tf / SEG_T_FAR - 1.0) > SPLIT_MARGIN
            if tf >= SEG_T_FAR and fits:
                split[t, q] = True
                n_items += (n + SEG_LEN - 1) // SEG_LEN - SEG_K0
    return dict(split=split, clear=clear, t_far=t_far, n_split=int(split.sum()), n_items=int(n_items), chunk_start=cs)


def pixel_splats(px, py, sigma_px, z, h: int, w: int):
    """means3D / cov6 of splats centred on pixel coordinates (px, py) with an isotropic screen footprint of sigma_px pixels (before
    the rasteriser's 0.3 low-pass), at view depth z, for the camera of small_front_scene (identity view, tanfov 1, h x w)."""
    import numpy as np
    px, py, z = (np.asarray(a, np.float64) for a in (px, py, z))
    sig = np.broadcast_to(np.asarray(sigma_px, np.float64), px.shape)
    fx, fy = w / 2.0, h / 2.0
    means = np.stack([((2 * px + 1) / w - 1) * z, ((2 * py + 1) / h - 1) * z, z], 1)
    sx, sy = sig * z / fx, sig * z / fy
    cov6 = np.zeros((px.shape[0], 6))
    cov6[:, 0], cov6[:, 3], cov6[:, 5] = sx * sx, sy * sy, (1e-3 * sx) ** 2
    return means, cov6


def tile_box(tx: int, ty: int, r: int = 4):
    """Centres whose 3-sigma rectangle (radius r pixels) touches tile (tx, ty) only (getRect's rounding): [x0, x1) x [y0, y1)."""
    return 16 * tx + r, 16 * tx + 17 - r, 16 * ty + r, 16 * ty + 17 - r
