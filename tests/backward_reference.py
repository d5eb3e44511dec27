"""Float64 statements of the rasteriser's backward at its seam, shared by tests/test_oracle_backward_parts.py (CPU) and
tests/test_gpu_backward_float64.py (GPU).  CPU only: numpy, the CPU oracle and the product's camera helpers.

The backward has two stages.  The COMPOSITE leaves one 48-byte raster-gradient record per (view, Gaussian) pair; the CHAIN turns
the records into the gradients of the inputs.  oracle/s360_oracle.c has the same seam (g_xy / g_conic / g_op / g_rgb between the
two loops of orc_backward), uses the kernels' formulas (upstream's 1 / (det^2 + 1e-7) included) and is therefore the float64
statement of both stages.

THE RECORD (include/s360.h s360_backward_pair_records), word by word, in the oracle's convention — the mapping is the identity:
    0, 1   dL/dx, dL/dy of the centre, in PIXELS            == raster_xy_pix
    2..4   dL/dA, dL/dB, dL/dC of the conic (A, B, C)       == raster_conic   (B: the TRUE d/dB, power = -A dx^2 / 2 - B dx dy - C dy^2 / 2:
                                                               no half factor, exactly as the oracle's g_conic[1])
    5      dL/dopacity                                       == raster_opacity
    6..8   dL/dr, dL/dg, dL/db BEFORE the clamp mask         == raster_rgb
    9      dL/d(depth value) = sum_pixels alpha T dL/ddepth  == raster_depth_value
    10, 11 unused
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from helpers import boundary_tensors, face_settings, pixel_splats, settings_from_views, small_front_scene
from oracle import oracle

EPS = 2.0 ** -24               # half an ulp of 1: the unit of every ratio below
# A float32 centre has an ulp of about 4e-6 px (64 .. 128 px images); times a dx <= 6 (a dx: conic x distance, bounded by the
# 3-sigma reach) it moves `power` by up to ~2.4e-5.  Four times that: a pixel whose nearest decision is farther away than this in
# float64 takes the same decisions in float32.
MARGIN = 1e-4
GROUPS = (("xy", slice(0, 2)), ("conic", slice(2, 5)), ("opacity", slice(5, 6)), ("rgb", slice(6, 9)))
DEPTH_WORD = 9
TAN_BAND = 1e-5                # |t_x / t_z| this close to 1.3 tan(fov): the clamp's derivative switch may fall either way in float32


def oracle_records(bw: dict, with_depth: bool = False):
    """backward()'s raster_* (and *_abs) as one [NP, 10] array each, in the record's word order."""
    cols = ("raster_xy_pix", "raster_conic", "raster_opacity", "raster_rgb") + (("raster_depth_value",) if with_depth else ())
    val = np.concatenate([np.asarray(bw[c], np.float64).reshape(bw[c].shape[0], -1) for c in cols], 1)
    mag = np.concatenate([np.asarray(bw[c + "_abs"], np.float64).reshape(bw[c].shape[0], -1) for c in cols], 1)
    return val, mag


def pair_ratios(rec, rec64, abs64, visible, words=slice(0, 9)):
    """|rec - rec64| / (2^-24 abs64) per visible pair and record word -> [n_visible, n_words].  A word whose abs64 is 0 (no term at
    all) must hold exactly 0: inf otherwise."""
    r = np.asarray(rec, np.float64)[visible][:, words]
    w = np.asarray(rec64, np.float64)[visible][:, words]
    a = np.asarray(abs64, np.float64)[visible][:, words]
    err = np.abs(r - w)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = err / (EPS * a)
    return np.where(a > 0, q, np.where(err == 0, 0.0, np.inf))


def group_stats(ratios):
    """{group: (worst, mean)} over the pairs, a pair's figure being the max over the group's words."""
    out = {}
    for name, sl in GROUPS:
        per = ratios[:, sl].max(1) if ratios.shape[0] else np.zeros(0)
        out[name] = (float(per.max(initial=0.0)), float(per.mean()) if per.size else 0.0)
    return out


def depth_value_grad(z, near, far, mode):
    """d(depth value) / dz of the fused depth channel (csrc/s360_bwd_em.h depth_value_grad), float64.  Mode 3 ("log") keeps the
    reference's swapped clamp: non-zero only where z < near and z > far, i.e. nowhere when near < far."""
    z = np.asarray(z, np.float64)
    if mode == 1:
        return -1.0 / (z * z)
    if mode == 2:
        eps = 1e-10
        disp_near, disp_far, disp = 1.0 / (near + eps), 1.0 / (far + eps), 1.0 / (z + eps)
        return (disp * disp) / (disp_near - disp_far + eps)
    if mode == 3:
        return np.where((z < near) & (z > far), 1.0 / z, 0.0)
    return np.ones_like(z)


def depth_value(z, near, far, mode):
    """A pair's value in the fused depth image (csrc/s360_device.h depth_value) from its unscaled camera depth, in z's precision."""
    z = np.asarray(z)
    dt = z.dtype.type
    if mode == 1:
        with np.errstate(divide="ignore"):                                  # culled pairs carry depth 0 and are never composited
            return dt(1) / z
    if mode == 2:
        eps = dt(1e-10)
        disp_near, disp_far, disp = dt(1) / (dt(near) + eps), dt(1) / (dt(far) + eps), dt(1) / (z + eps)
        return dt(1) - (disp - disp_far) / (disp_near - disp_far + eps)
    if mode == 3:
        return np.log(np.maximum(np.minimum(z, dt(near)), dt(far)))
    return z


# ------------------------------------------------------------------------------------------------------------------- scenes (test A)
def _wide_scene():
    """128 x 96 (8 x 6 = 48 tiles): a sparse background + 10 planted splats of sigma 16 .. 24 px, whose 3-sigma rectangles cover more
    than 32 tiles each: the wave-parallel slot sum of k_gather_slots."""
    h, w = 96, 128
    S, means, cov6, shs, opac = small_front_scene(n=40, seed=5, h=h, w=w, srange=(0.03, 0.12))
    rng = np.random.default_rng(11)
    n = 10
    z = rng.uniform(3.0, 5.0, n)
    m2, c2 = pixel_splats(rng.uniform(40, 88, n), rng.uniform(30, 66, n), rng.uniform(16, 24, n), z, h, w)
    sh2 = rng.standard_normal((n, 25, 3)) * 0.05
    sh2[:, 0, :] = rng.uniform(0.2, 1.5, (n, 3))
    return S, np.concatenate([means, m2]), np.concatenate([cov6, c2]), np.concatenate([shs, sh2]), \
        np.concatenate([opac, rng.uniform(0.15, 0.4, (n, 1))]), None, dict(planted=np.arange(40, 50))


def _split_scene():
    """tests/test_gpu_split_parity.py's designed one-tile scene at its smallest length that is handed over: more than SORT_SHORT
    (2048) entries."""
    from test_gpu_split_parity import _scene
    S, means, cov6, op, colors, info = _scene(2049, "sq", seed=3)
    return S, means, cov6, None, op, colors, info


def _dense_scene():
    """The config-0 cloud of tests/test_gpu_parity.py::test_config0_faces_vs_oracle on one 64 x 64 face.  Face 2: on each of the other
    five, one or two of the ~2800 visible pairs put the float32 ORACLE itself beyond the 2^10 usability bar of the yardstick
    (1800 .. 4500 units: T / (1 - alpha) behind entries at the 0.99 clamp), which tests/test_oracle_backward_parts.py asserts; face 2
    stays at 770 and has the smallest flagged share (7.4 %)."""
    from splatter360_amd import synthetic
    cloud = synthetic.uniform_cloud(10_000, seed=3, extent=3.0, scale_range=(0.02, 0.3))
    S = face_settings(2, 64, 64)
    means, cov6, shs, opac = boundary_tensors(cloud, S["scale"])
    return S, means, cov6, shs, opac, None, {}


def _small_scene():
    S, means, cov6, shs, opac = small_front_scene(n=60, h=64, w=80)
    return S, means, cov6, shs, opac, None, {}


SCENES = {"small": _small_scene, "dense": _dense_scene, "wide": _wide_scene, "split": _split_scene}


def view_record(S) -> torch.Tensor:
    """[1,44] S360View of a settings dict (CPU tensor; near / far only feed a depth channel these scenes do not have)."""
    from splatter360_amd import rasterizer
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    return rasterizer.pack_views(t(S["viewmatrix"]), t(S["projmatrix"]), t(S["campos"]), float(S["tanfovx"]), float(S["tanfovy"]),
                                 t(S["bg"]), near=1.0, far=100.0)


@functools.lru_cache(maxsize=None)
def scene(name: str) -> dict:
    """One scene of test A, float32 inputs as both the kernels and the oracles read them, the float64 oracle's forward (decision
    margins, flagged pixels), the masked seed, and both oracles' records on it.  Cached: shared by every mode and by the CPU tests;
    nobody writes into it."""
    S, means, cov6, shs, opac, colors, info = SCENES[name]()
    f32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.float32))
    means, cov6, shs, opac, colors = f32(means), f32(cov6), f32(shs), f32(opac), f32(colors)
    h, w = int(S["image_height"]), int(S["image_width"])
    views = view_record(S)
    So = settings_from_views(views, 0, h, w, int(S["sh_degree"]))
    out = dict(S=S, So=So, views=views, means=means, cov6=cov6, shs=shs, opac=opac, colors=colors, h=h, w=w, info=info)
    orc = {}
    for dt in (np.float64, np.float32):
        o = oracle.rasterize(So, means3D=means, cov3D_precomp=cov6, opacities=opac, shs=shs, colors_precomp=colors, dtype=dt)
        orc[dt] = (o, o.forward())
    f64 = orc[np.float64][1]
    flagged = f64["decision_margin"] < MARGIN
    seed = np.random.default_rng(1234).standard_normal((3, h, w)).astype(np.float32)
    seed_raw = seed.copy()
    seed[:, flagged] = 0.0
    out.update(flagged=flagged, seed=seed, seed_raw=seed_raw, f64=f64, f32=orc[np.float32][1], orc64=orc[np.float64][0], orc32=orc[np.float32][0])
    out["b64"] = orc[np.float64][0].backward(seed)
    out["b32"] = orc[np.float32][0].backward(seed)
    return out


def last_contributor(n_contrib, ranges, values, h, w):
    """Gaussian index of each pixel's last contributor (-1: none) from n_contrib (a list position) and the tile lists: the statement
    of n_contrib that does not depend on which entries a list mode keeps."""
    gx = (w + 15) // 16
    py, px = np.mgrid[0:h, 0:w]
    tile = (py // 16) * gx + px // 16
    n = np.asarray(n_contrib, np.int64)
    pos = np.asarray(ranges, np.int64)[tile, 0] + n - 1
    vals = np.asarray(values, np.int64)
    return np.where(n > 0, vals[np.clip(pos, 0, max(len(vals) - 1, 0))] if len(vals) else -1, -1)


# ------------------------------------------------------------------------------------------------------------ role cloud (test B)
N_ROLES = 10
FACE = 32


def role_cloud(p: int, m: int = 25, seed: int = 0):
    """The cloud of tests/test_gpu_gaussians_bwd_fused.py (role by index mod 10: 0 inside every near plane | 1 cube edge | 2 cube
    corner | 3, 4, 5 one / two / three clamped channels | 6, 7 plain) with two more roles: 8 a large splat centred at 1.5 x the
    1.3 tan(fov) limit of a neighbouring face (tangent-clamped there in x or in y, still visible) | 9 far and small (depth 8,
    sigma 0.1 .. 0.3 px: radius 3 px, the smallest there is — the 0.3 dilation and the max(0.1, .) under the eigenvalue's root
    give lambda >= 0.3 + sqrt(0.1), and 3 sqrt(0.616) rounds up to 3; a radius of 1 or 2 px does not exist).
    No covariance here lets det^2 overflow float32: the d2inv == 0 branch (1 / inf) cannot be stated in float64, where det^2 does
    not overflow, so it stays outside this test."""
    from splatter360_amd import synthetic
    c = synthetic.uniform_cloud(p, d_sh=m, seed=seed, extent=2.0, scale_range=(0.05, 0.4))
    rng = np.random.default_rng(seed + 1000)
    role = np.arange(p) % N_ROLES
    means, sh, cov = c["means"], c["harmonics"], c["covariances"]
    d = rng.standard_normal((p, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    means[role == 0] = 0.01 * d[role == 0]
    sgn = np.where(rng.random((p, 3)) < 0.5, -1.0, 1.0).astype(np.float32)
    r = rng.uniform(0.8, 1.5, (p, 1)).astype(np.float32)
    roll = lambda a: np.stack([np.roll(a[i], i % 3) for i in range(p)])
    edge = roll(sgn * r * np.array([1.0, 1.0, 0.05], np.float32))
    means[role == 1] = edge[role == 1]
    means[role == 2] = (sgn * r)[role == 2]
    for n_ch, ro in ((1, 3), (2, 4), (3, 5)):
        sh[role == ro, :n_ch, 0] = -4.0
        sh[role == ro, :n_ch, 1:] *= 0.1
    tang = roll(sgn * r * np.array([1.95, 0.3, 1.0], np.float32))          # t_x / t_z = 1.95 = 1.5 x 1.3 in the face of the last axis
    means[role == 8] = tang[role == 8]
    s8 = (0.45 * r[:, 0]) ** 2
    far = roll(sgn * np.concatenate([rng.uniform(0.0, 3.0, (p, 2)), np.full((p, 1), 8.0)], 1).astype(np.float32))
    means[role == 9] = far[role == 9]
    s9 = rng.uniform(0.05, 0.15, p) ** 2
    eye = np.eye(3, dtype=np.float32)
    for ro, s in ((8, s8), (9, s9)):
        cov[role == ro] = s[role == ro, None, None].astype(np.float32) * eye * np.array([1.0, 0.8, 1.2], np.float32)
    return c, role


def cube_views(n_views: int = 6, positions=((0.0, 0.0, 0.0),), near: float = 0.1, far: float = 10.0) -> torch.Tensor:
    """[n_views,44] CPU view records: the first n_views face cameras of a panorama at positions[0], or (several positions) face
    i of the panorama at positions[i].  near = 0.1: the scale-invariant rescale gives every view the scale 10."""
    from splatter360_amd import decoder, synthetic
    rows = []
    for i, pos in enumerate(positions):
        ext, k, nr, fr = decoder.cube_cameras(torch.from_numpy(synthetic.target_pano_pose(pos)), near, far)
        sl = slice(0, n_views) if len(positions) == 1 else slice(i, i + 1)
        rows.append(decoder.pack_camera_views(ext[sl], k[sl], nr[sl], fr[sl], torch.zeros(3), glue="torch"))
    return torch.cat(rows).contiguous()


def cloud_arrays(cloud: dict):
    """float32 means[P,3], cov6[P,6], shs[P,M,3], opacities[P,1] of a cloud dict (unscaled)."""
    r, c = np.triu_indices(3)
    return (np.ascontiguousarray(cloud["means"], np.float32), np.ascontiguousarray(cloud["covariances"][:, r, c], np.float32),
            np.ascontiguousarray(cloud["harmonics"].transpose(0, 2, 1), np.float32), np.ascontiguousarray(cloud["opacities"][:, None], np.float32))


class ViewOracles:
    """Per view of one call: the oracle (of one precision) on the view's scaled float32 cloud, exactly the numbers the kernels form
    (mean * scale, cov * (scale * scale), both float32 products), and its forward."""

    def __init__(self, views, cloud, h, w, deg, dtype, colors=None):
        self.views = np.asarray(views.detach().cpu().numpy(), np.float32)
        self.V, self.h, self.w, self.deg, self.dt = self.views.shape[0], h, w, deg, np.dtype(dtype)
        means, cov6, shs, opac = cloud_arrays(cloud)
        self.P, self.M = means.shape[0], shs.shape[1]
        self.use_sh = colors is None
        self.S, self.orc, self.fwd, self.scaled_means = [], [], [], []
        for v in range(self.V):
            S = settings_from_views(views, v, h, w, deg)
            sc = np.float32(S["scale"])
            mv, cv = means * sc, cov6 * (sc * sc)
            o = oracle.rasterize(S, means3D=mv, cov3D_precomp=cv, opacities=opac, shs=shs if self.use_sh else None,
                                 colors_precomp=None if self.use_sh else np.asarray(colors, np.float32), dtype=dtype)
            self.S.append(S)
            self.orc.append(o)
            self.fwd.append(o.forward())
            self.scaled_means.append(mv)
        self.visible = np.stack([f["radii"] > 0 for f in self.fwd])                      # [V,P]
        self.clamped = np.stack([f["clamped"].astype(bool) for f in self.fwd])           # [V,P,3]

    def tangent(self):
        """|t_x / t_z| - 1.3 tan(fov_x) and the same in y, per pair, float64 from the float32 inputs: > 0 means clamped.  [V,2,P]"""
        out = []
        for v in range(self.V):
            Vm = self.S[v]["viewmatrix"].astype(np.float64).reshape(16)
            m = self.scaled_means[v].astype(np.float64)
            t = [Vm[i] * m[:, 0] + Vm[4 + i] * m[:, 1] + Vm[8 + i] * m[:, 2] + Vm[12 + i] for i in range(3)]
            with np.errstate(divide="ignore", invalid="ignore"):
                out.append((np.abs(t[0] / t[2]) - 1.3 * self.S[v]["tanfovx"], np.abs(t[1] / t[2]) - 1.3 * self.S[v]["tanfovy"]))
        return np.asarray(out)

    def chain(self, R, depth_mode=None, want_abs=False):
        """The per-Gaussian chain on records R[V,P,12]: per view the oracle's backward_gaussians on R[v], folded back to the
        unscaled cloud with scale (means) and scale^2 (covariance) in view order, + the depth-value chain in numpy.  All in this
        object's precision.  want_abs: also D = sum_v sum_k |J_k| |R_k| per output element (nine unit-record runs per view give the
        Jacobian columns; the depth column is closed form): the condition of each output."""
        dt, P = self.dt.type, self.P
        R = np.asarray(R)
        out = dict(means=np.zeros((P, 3), dt), cov=np.zeros((P, 6), dt), opac=np.zeros(P, dt), means2D=np.zeros((self.V, P, 3), dt))
        out["sh" if self.use_sh else "colors"] = np.zeros((P, self.M, 3) if self.use_sh else (P, 3), dt)
        D = {k: np.zeros(v.shape, np.float64) for k, v in out.items()} if want_abs else None
        key = dict(means="means3D", cov="cov3D", sh="shs", colors="colors_precomp")
        for v in range(self.V):
            sc = np.float32(self.S[v]["scale"])
            fold = dict(means=dt(sc), cov=dt(sc * sc), sh=dt(1), colors=dt(1))
            r = R[v].astype(dt)
            g = self.orc[v].backward_gaussians(r[:, 0:2], r[:, 2:5], r[:, 5], r[:, 6:9])
            for k in key:
                if k in out:
                    out[k] = out[k] + fold[k] * g[key[k]]
            out["opac"] = out["opac"] + g["opacities"][:, 0]
            out["means2D"][v] = g["means2D"]
            if want_abs:
                for word in range(9):
                    unit = np.zeros((P, 12), dt)
                    unit[:, word] = 1
                    j = self.orc[v].backward_gaussians(unit[:, 0:2], unit[:, 2:5], unit[:, 5], unit[:, 6:9])
                    mag = np.abs(r[:, word].astype(np.float64))
                    for k in key:
                        if k in out:
                            D[k] += float(fold[k]) * np.abs(j[key[k]]) * mag.reshape((P,) + (1,) * (out[k].ndim - 1))
                    D["opac"] += np.abs(j["opacities"][:, 0]) * mag
                    D["means2D"][v] += np.abs(j["means2D"]) * mag[:, None]
            if depth_mode is not None:
                Vm = self.S[v]["viewmatrix"].astype(dt).reshape(16)
                m = self.scaled_means[v].astype(dt)
                tzs = Vm[2] * m[:, 0] + Vm[6] * m[:, 1] + Vm[10] * m[:, 2] + Vm[14]
                dvg = depth_value_grad(tzs * (dt(1) / dt(sc)), float(self.views[v, 41]), float(self.views[v, 42]), depth_mode).astype(dt)
                dzu = np.where(self.visible[v], r[:, DEPTH_WORD] * dvg, dt(0))
                row = np.stack([Vm[2] * dzu, Vm[6] * dzu, Vm[10] * dzu], 1)
                out["means"] = out["means"] + row
                if want_abs:
                    D["means"] += np.abs(row.astype(np.float64))
        return (out, D) if want_abs else out


def element_ratios(got, want64, D):
    """|got - want64| / (2^-24 D) per element; D == 0 demands exactly 0 (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = err / (EPS * D)
    return np.where(D > 0, q, np.where(np.asarray(got, np.float64) == 0, 0.0, np.inf))


def gaussian_stats(got, want64, D, keep):
    """(worst, mean) over the Gaussians in `keep` of each Gaussian's largest element ratio; the mean runs over the Gaussians that have
    a non-zero condition (the others must be, and are checked to be, exactly 0)."""
    P = D.shape[0]
    q = element_ratios(got, want64, D).reshape(P, -1).max(1)
    live = keep & (D.reshape(P, -1).max(1) > 0)
    return float(q[keep].max(initial=0.0)), float(q[live].mean()) if live.any() else 0.0


def excluded(vo64: ViewOracles, vis_hip, clamped_hip):
    """Gaussians left out of the chain's bound: HIP's visibility bit or clamp bits differ from the float64 oracle's in some view, or
    |t / t_z| of a visible pair lies within TAN_BAND of the 1.3 tan(fov) limit.  vis_hip[V,P] bool, clamped_hip[V,P,3] bool."""
    vis = vo64.visible
    bad = (vis != vis_hip).any(0)
    if vo64.use_sh:
        bad |= (vis[:, :, None] & (vo64.clamped != clamped_hip)).any((0, 2))
    tg = vo64.tangent()
    bad |= (vis[:, None, :] & (np.abs(tg) < TAN_BAND)).any((0, 1))
    return bad


# ------------------------------------------------------------------------------------------------------------- chain cases (test B)
CHAIN_P = (64 * 3 + 17, 256 + 14)        # a ragged last block for the 64-wide and for the 256-wide kernels


@functools.lru_cache(maxsize=None)
def chain_setup(p: int, m: int = 25, deg: int = 4, kind: str = "cube6", colors: bool = False) -> dict:
    """Cloud, views and both precisions' per-view oracles of one chain case.  kind "cube6": the six faces of one panorama (one
    camera centre); "two_centres": face 0 and face 1 of two panoramas at different positions.  Cached; nobody writes into it."""
    cloud, role = role_cloud(p, m, seed=p)
    views = cube_views(6) if kind == "cube6" else cube_views(positions=((0.3, -0.2, 0.1), (-0.25, 0.15, 0.2)))
    col = np.random.default_rng(p).uniform(0.0, 1.0, (p, 3)).astype(np.float32) if colors else None
    vo = {dt: ViewOracles(views, cloud, FACE, FACE, deg, dt, col) for dt in (np.float64, np.float32)}
    return dict(cloud=cloud, role=role, views=views, colors=col, vo64=vo[np.float64], vo32=vo[np.float32], deg=deg, m=m)


def roles_reached(setup: dict) -> dict:
    """How many Gaussians (or pairs) of a cube6 case play each role the cloud is built for, by the float64 oracle."""
    vo, role = setup["vo64"], setup["role"]
    vis = vo.visible
    n_faces = vis.sum(0)
    n_cl = (vo.clamped & vis[:, :, None]).any(0).sum(1) if vo.use_sh else np.zeros(vo.P, int)
    tg = vo.tangent()
    radii = np.stack([f["radii"] for f in vo.fwd])
    return dict(invisible=int((n_faces == 0).sum()), one_face=int((n_faces == 1).sum()), two_faces=int((n_faces == 2).sum()),
                three_faces=int((n_faces >= 3).sum()), clamped_1=int((n_cl == 1).sum()), clamped_2=int((n_cl == 2).sum()),
                clamped_3=int((n_cl == 3).sum()), tangent_x=int((vis & (tg[:, 0] > 0) & (role == 8)[None]).sum()),
                tangent_y=int((vis & (tg[:, 1] > 0) & (role == 8)[None]).sum()),
                far_small=int(((radii > 0) & (radii <= 3) & (role == 9)[None]).sum()))


CUBE_DEPTH_MODE = 1


@functools.lru_cache(maxsize=None)
def cube_scene() -> dict:
    """The V = 6 case of test A: the role cloud on six 32 x 32 faces with a depth channel ("disparity": value = 1 / unscaled camera
    depth).  Per view the float64 oracle's flagged pixels, the masked seeds (image and depth), and both oracles' records ([V,P,10]:
    word 9 is the depth record) with the float64 term magnitudes.  The depth image is a fourth colour channel of the composite: its
    seed reaches dL/dalpha, so every word of the record depends on it."""
    s = chain_setup(CHAIN_P[0])
    vo64, vo32 = s["vo64"], s["vo32"]
    rng = np.random.default_rng(77)
    seed = rng.standard_normal((6, 3, FACE, FACE)).astype(np.float32)
    dseed = rng.standard_normal((6, FACE, FACE)).astype(np.float32)
    flagged = np.stack([f["decision_margin"] < MARGIN for f in vo64.fwd])
    seed[np.broadcast_to(flagged[:, None], seed.shape)] = 0.0
    dseed[flagged] = 0.0
    rec = {}
    for name, vo in (("64", vo64), ("32", vo32)):
        dt = vo.dt.type
        zval = [depth_value(vo.fwd[v]["depth"] * (dt(1) / dt(np.float32(vo.S[v]["scale"]))), vo.views[v, 41], vo.views[v, 42], CUBE_DEPTH_MODE)
                for v in range(6)]
        pairs = [oracle_records(vo.orc[v].backward(seed[v], dL_ddepth=dseed[v], depth_values=zval[v]), with_depth=True) for v in range(6)]
        rec["r" + name] = np.stack([p[0] for p in pairs])
        rec["a" + name] = np.stack([p[1] for p in pairs])
    return dict(setup=s, seed=seed, dseed=dseed, flagged=flagged, **rec)


# =========================================================================================== spherical mode (S360_FLAG_SPHERICAL)
# One panorama is the oracle's NP = 2P pairs (rows 0 .. P-1: the main pair of each Gaussian, rows P .. 2P-1: its seam ghost), which
# are the kernels' views 2i (main) and 2i + 1 (ghost) of panorama i.  tests/test_oracle_spherical_parts.py pins everything below on
# the CPU; tests/test_gpu_spherical_float64.py holds the kernels to it.
POLE_CLAMP = 0.05              # geo_sph: rho < 0.05 r clamps rho inside the Jacobian and switches a derivative branch
POLE_RATIOS = (0.003, 0.01, 0.03, 0.049, 0.051, 0.2)       # planted rho / r: both sides of the clamp, nothing below 0.003 (see below)
POLE_BAND = 1e-5               # |rho / r - 0.05| this small: the switch may fall either way in float32 (the analogue of TAN_BAND)
SEAM_BAND = 0.03               # planted seam Gaussians: azimuth within this many radians of +-pi
SPH_GROUPS = ("plain", "ghost", "pole")
# The centre's column is atan2(t0, t2): a rounding of t0 / t2 (relative 2^-24 of r) moves it by (r / rho) 2^-24 W / 2 pi pixels, which
# the *_abs sums of the pixel loop do not see.  At rho / r = 0.003 the float32 oracle's pair ratio reaches ~2^11 units, at 0.001
# 15 000 .. 28 000, and on the axis float32 and float64 disagree on hundreds of unflagged pixels: the planted ratios start at 0.003,
# the pole group has its own usability bar, and the axis itself gets a finiteness check only.
# A ghost's centre is u +- W, outside the image: only its tail reaches pixels, and its float32 rounding (half an ulp of up to 2 W,
# against a main pair's mean W / 2) enters every term through conic x dx x rounding, which the *_abs sums do not see either.  A
# small splat (radius 3 .. 4 px) just beyond the seam reaches 1034 units at W = 64 and 1505 at W = 160 on the float32 oracle
# (344 and 663 on the other two scenes): the ghost group gets four times the plain bar.  The pole group's worst (2728 .. 4469, and
# 5227 with a view matrix one ulp away) gets eight times: tests/test_oracle_spherical_parts.py.
SPH_BARS = dict(plain=2.0 ** 10, ghost=2.0 ** 12, pole=2.0 ** 13)


def sph_pose(pos=(0.1, -0.2, 0.05), seed=4):
    """tests/test_gpu_spherical.py's _pose(): a random rotation and a small offset (seed 4 is that test's)."""
    from splatter360_amd import synthetic
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = synthetic._random_rotations(np.random.default_rng(seed), 1)[0]
    m[:3, 3] = pos
    return m


def _camera_to_world(t, pose):
    """R t + c in float64 with explicit products and sums (no BLAS: the same bits on every host), rounded to float32."""
    t, R, c = np.asarray(t, np.float64), pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    return np.stack([R[k, 0] * t[..., 0] + R[k, 1] * t[..., 1] + R[k, 2] * t[..., 2] + c[k] for k in range(3)], -1).astype(np.float32)


def plant_sphere(cloud: dict, first: int, pose, rng, n_pole: int, n_seam: int, sigma=(0.04, 0.12), radius=(1.5, 3.0)):
    """Overwrite cloud rows first .. first + 12 n_pole + n_seam - 1 with Gaussians placed in the camera frame of `pose` (+z: panorama
    centre, +y: top row) and mapped to the world with it: n_pole at every POLE_RATIOS x {north, south} with a random azimuth, n_seam
    with the azimuth within SEAM_BAND of +-pi at latitudes across -1.3 .. 1.3 rad.  Near-isotropic covariances.
    -> dict(pole_ratio[P] (nan: not planted there), pole_sign[P], seam[P] bool)."""
    p = cloud["means"].shape[0]
    info = dict(pole_ratio=np.full(p, np.nan), pole_sign=np.zeros(p, int), seam=np.zeros(p, bool))
    g = first
    eye = np.eye(3, dtype=np.float32)

    def put(t):
        nonlocal g
        cloud["means"][g] = _camera_to_world(t, pose)
        s = rng.uniform(*sigma)
        cloud["covariances"][g] = (s * s * eye * rng.uniform(0.8, 1.25, 3)).astype(np.float32)
        cloud["opacities"][g] = rng.uniform(0.3, 0.9)
        g += 1
        return g - 1

    for sign in (1, -1):
        for ratio in POLE_RATIOS:
            for _ in range(n_pole):
                az, r = rng.uniform(-np.pi, np.pi), rng.uniform(*radius)
                i = put(r * np.array([ratio * np.sin(az), sign * np.sqrt(1 - ratio * ratio), ratio * np.cos(az)]))
                info["pole_ratio"][i], info["pole_sign"][i] = ratio, sign
    for k in range(n_seam):
        th = np.pi + rng.uniform(-SEAM_BAND, SEAM_BAND)
        ph = -1.3 + 2.6 * (k + rng.uniform(0.1, 0.9)) / n_seam
        r = rng.uniform(*radius)
        info["seam"][put(r * np.array([np.cos(ph) * np.sin(th), np.sin(ph), np.cos(ph) * np.cos(th)]))] = True
    assert g <= p
    return info


def sph_views(poses, near: float = 0.1, bg=(0.1, 0.2, 0.3)) -> torch.Tensor:
    """[2n,44] CPU view records of n panoramas (camera, seam ghost), laid out as rasterizer.pack_views_spherical lays them out; near
    = 0.1 gives the scale 10.  The world-to-camera matrix is the rigid inverse (R^T, -R^T c) formed in float64 with explicit
    products and sums instead of that function's LAPACK inverse: at the pole one ulp of the view matrix is amplified by r / rho
    (it moved the float32 oracle's worst pole pair of the 48 x 96 scene between 3693 and 5227 units from one host to another), so
    the records must be the same bits wherever the tests run.  tests/test_gpu_spherical.py covers pack_views_spherical itself."""
    from splatter360_amd import rasterizer
    sc = np.float32(1.0 / near)
    vms, cps = [], []
    for pose in poses:
        R = pose[:3, :3].astype(np.float64)
        c = (pose[:3, 3].astype(np.float32) * sc).astype(np.float64)                      # the scaled centre, a float32 product
        w2c = np.eye(4)
        w2c[:3, :3] = R.T
        w2c[:3, 3] = [-(R[0, k] * c[0] + R[1, k] * c[1] + R[2, k] * c[2]) for k in range(3)]
        vms.append(w2c.T.astype(np.float32))                                             # stored transposed, as the kernels read it
        cps.append(c.astype(np.float32))
    n = len(poses)
    one = torch.ones(n)
    v = rasterizer.pack_views(torch.from_numpy(np.stack(vms)), torch.eye(4).expand(n, 4, 4), torch.from_numpy(np.stack(cps)), one, one,
                              torch.tensor(bg, dtype=torch.float32), scale=torch.full((n,), float(sc)), near=near, far=0.0)
    return v.repeat_interleave(2, dim=0).contiguous()


def pair_rows(x, i: int):
    """Rows of panorama i in the oracle's order (main pairs, then ghosts) from a per-view array x[V, P, ...]."""
    return np.concatenate([x[2 * i], x[2 * i + 1]])


class SphereOracles:
    """Per panorama of one spherical call: the oracle (of one precision) on the panorama's scaled float32 cloud and its forward.
    visible / clamped are laid out per VIEW like the kernels' ([V,P] / [V,P,3]; V = 2 n: view 2i main, 2i + 1 ghost)."""

    def __init__(self, views, cloud, h, w, deg, dtype, colors=None):
        self.views = np.asarray(views.detach().cpu().numpy(), np.float32)
        self.V, self.h, self.w, self.deg, self.dt = self.views.shape[0], h, w, deg, np.dtype(dtype)
        self.n = self.V // 2
        means, cov6, shs, opac = cloud_arrays(cloud)
        self.P, self.M = means.shape[0], shs.shape[1]
        self.use_sh = colors is None
        self.S, self.orc, self.fwd, self.scaled_means = [], [], [], []
        for i in range(self.n):
            assert np.array_equal(self.views[2 * i], self.views[2 * i + 1])
            S = settings_from_views(views, 2 * i, h, w, deg)
            sc = np.float32(S["scale"])
            mv, cv = means * sc, cov6 * (sc * sc)
            o = oracle.rasterize(S, means3D=mv, cov3D_precomp=cv, opacities=opac, shs=shs if self.use_sh else None,
                                 colors_precomp=None if self.use_sh else np.asarray(colors, np.float32), dtype=dtype, spherical=True)
            self.S.append(S)
            self.orc.append(o)
            self.fwd.append(o.forward())
            self.scaled_means.append(mv)
        P = self.P
        self.visible = np.concatenate([(f["radii"] > 0).reshape(2, P) for f in self.fwd])                     # [V,P]
        self.clamped = np.concatenate([f["clamped"].astype(bool).reshape(2, P, 3) for f in self.fwd])         # [V,P,3]

    def rho_over_r(self):
        """rho / r of every Gaussian in every panorama, float64 from the float32 inputs.  [n,P]"""
        out = []
        for i in range(self.n):
            Vm = self.S[i]["viewmatrix"].astype(np.float64).reshape(16)
            m = self.scaled_means[i].astype(np.float64)
            t = [Vm[k] * m[:, 0] + Vm[4 + k] * m[:, 1] + Vm[8 + k] * m[:, 2] + Vm[12 + k] for k in range(3)]
            rho2 = t[0] * t[0] + t[2] * t[2]
            out.append(np.sqrt(rho2) / np.sqrt(rho2 + t[1] * t[1]))
        return np.asarray(out)

    def groups(self):
        """[V,P] index into SPH_GROUPS: pole (float64 rho < 0.05 r; both pairs of the Gaussian) | ghost (views 2i + 1) | plain."""
        pole = self.rho_over_r() < POLE_CLAMP
        g = np.zeros((self.V, self.P), int)
        g[1::2] = SPH_GROUPS.index("ghost")
        g[np.repeat(pole, 2, axis=0)] = SPH_GROUPS.index("pole")
        return g

    def chain(self, R, want_abs=False):
        """The per-Gaussian chain on records R[V,P,12]: per panorama the oracle's backward_gaussians (backward_one_sph: the main and
        the ghost record add, then geo_sph's chain) on its 2P rows, folded back to the unscaled cloud with scale / scale^2.
        want_abs: D = sum over BOTH pairs and the nine words of |J_k| |R_k| per output element; the Jacobian columns come from unit
        records set in one pair at a time (set in both, the two columns would add inside |.| and could cancel).  The depth-record
        word is not produced in this mode (no fused depth channel)."""
        dt, P = self.dt.type, self.P
        R = np.asarray(R)
        out = dict(means=np.zeros((P, 3), dt), cov=np.zeros((P, 6), dt), opac=np.zeros(P, dt))
        out["sh" if self.use_sh else "colors"] = np.zeros((P, self.M, 3) if self.use_sh else (P, 3), dt)
        D = {k: np.zeros(v.shape, np.float64) for k, v in out.items()} if want_abs else None
        key = dict(means="means3D", cov="cov3D", sh="shs", colors="colors_precomp")
        run = lambda o, r: o.backward_gaussians(r[:, 0:2], r[:, 2:5], r[:, 5], r[:, 6:9])
        for i in range(self.n):
            sc = np.float32(self.S[i]["scale"])
            fold = dict(means=dt(sc), cov=dt(sc * sc), sh=dt(1), colors=dt(1))
            r = pair_rows(R, i).astype(dt)
            g = run(self.orc[i], r)
            for k in key:
                if k in out:
                    out[k] = out[k] + fold[k] * g[key[k]]
            out["opac"] = out["opac"] + g["opacities"][:, 0]
            if want_abs:
                for half in range(2):
                    rows = slice(half * P, (half + 1) * P)
                    for word in range(9):
                        unit = np.zeros((2 * P, 12), dt)
                        unit[rows, word] = 1
                        j = run(self.orc[i], unit)
                        mag = np.abs(r[rows, word].astype(np.float64))
                        for k in key:
                            if k in out:
                                D[k] += float(fold[k]) * np.abs(j[key[k]]) * mag.reshape((P,) + (1,) * (out[k].ndim - 1))
                        D["opac"] += np.abs(j["opacities"][:, 0]) * mag
        return (out, D) if want_abs else out


def excluded_sph(so64: SphereOracles, vis_hip, clamped_hip):
    """Gaussians left out of the spherical chain's bound: the kernels' visibility bit differs from the float64 oracle's on either
    pair of some panorama, a colour clamp bit of a visible pair differs, or a visible pair has |rho / r - 0.05| < POLE_BAND."""
    vis = so64.visible
    bad = (vis != vis_hip).any(0)
    if so64.use_sh:
        bad |= (vis[:, :, None] & (so64.clamped != clamped_hip)).any((0, 2))
    near = np.abs(so64.rho_over_r() - POLE_CLAMP) < POLE_BAND                              # [n,P]
    bad |= (np.repeat(near, 2, axis=0) & vis).any(0)
    return bad


# -------------------------------------------------------------------------------------------------- spherical pair scenes (test A)
def _sph_cloud(n_uniform, n_pole, n_seam, poses, seed=3, extra=0):
    """synthetic.uniform_cloud(n_uniform, seed, extent 3, scales 0.05 .. 0.3) exactly, with the planted rows appended."""
    from splatter360_amd import synthetic
    cloud = synthetic.uniform_cloud(n_uniform, seed=seed, extent=3.0, scale_range=(0.05, 0.3))
    n_add = (12 * n_pole + n_seam) * len(poses) + extra
    more = synthetic.uniform_cloud(n_add, seed=seed + 50, extent=3.0, scale_range=(0.05, 0.3))          # harmonics of the planted rows
    cloud = {k: np.concatenate([cloud[k], more[k]]) for k in cloud}
    rng = np.random.default_rng(seed + 100)
    infos, first = [], n_uniform
    for pose in poses:
        infos.append(plant_sphere(cloud, first, pose, rng, n_pole, n_seam))
        first += 12 * n_pole + n_seam
    return cloud, infos, first


def _sph_p32():
    poses = [sph_pose()]
    cloud, infos, _ = _sph_cloud(900, 4, 32, poses)
    return cloud, poses, infos, 32, 64


def _sph_p48():
    poses = [sph_pose()]
    cloud, infos, _ = _sph_cloud(1500, 4, 32, poses)
    return cloud, poses, infos, 48, 96


def _sph_two():
    """TWO panoramas at different poses in one call (V = 4 views, no shared camera centre): image_of_view / view_of_image and
    nt = V / 2 x T.  Each pose has its own planted poles and seam."""
    poses = [sph_pose(), sph_pose((-0.3, 0.25, -0.15), seed=9)]
    cloud, infos, _ = _sph_cloud(900, 2, 16, poses)
    return cloud, poses, infos, 32, 64


def _sph_wide():
    """80 x 160 (5 x 10 = 50 tiles; the two sizes above have 8 and 18 tiles, so no pair of theirs can own more than 32): a sparse
    cloud and two large Gaussians (sigma 0.6 and 0.9 at distance 2 and 2.4, rho / r = 0.2 and 0.3) whose main pairs own more than 32 tiles:
    the wave-parallel slot sum of k_gather_slots."""
    poses = [sph_pose()]
    cloud, infos, first = _sph_cloud(400, 1, 8, poses, extra=2)
    rng = np.random.default_rng(17)
    for k, (ratio, sign) in enumerate(((0.2, 1), (0.3, -1))):
        g = first + k
        cloud["means"][g] = _camera_to_world((2.0 + 0.4 * k) * np.array([ratio * np.sin(0.7 + k), sign * np.sqrt(1 - ratio * ratio), ratio * np.cos(0.7 + k)]), poses[0])
        cloud["covariances"][g] = ((0.6 + 0.3 * k) ** 2 * np.eye(3) * rng.uniform(0.8, 1.25, 3)).astype(np.float32)
        cloud["opacities"][g] = 0.3
    infos[0]["large"] = np.arange(first, first + 2)
    return cloud, poses, infos, 80, 160


SPH_SCENES = {"p32": _sph_p32, "p48": _sph_p48, "two": _sph_two, "wide": _sph_wide}


@functools.lru_cache(maxsize=None)
def sph_scene(name: str) -> dict:
    """One spherical scene of test A: the cloud, the view records, both precisions' per-panorama oracles, the float64 flagged pixels,
    the masked seed [n,3,h,w], both oracles' records on it as [n,2P,9] (+ the float64 term magnitudes) and every pair's group.
    Cached; nobody writes into it."""
    cloud, poses, infos, h, w = SPH_SCENES[name]()
    views = sph_views(poses)
    so = {dt: SphereOracles(views, cloud, h, w, 4, dt) for dt in (np.float64, np.float32)}
    so64, so32 = so[np.float64], so[np.float32]
    n = so64.n
    flagged = np.stack([f["decision_margin"] < MARGIN for f in so64.fwd])
    seed = np.random.default_rng(4321).standard_normal((n, 3, h, w)).astype(np.float32)
    seed[np.broadcast_to(flagged[:, None], seed.shape)] = 0.0
    rec = {}
    for tag, s in (("64", so64), ("32", so32)):
        pairs = [oracle_records(s.orc[i].backward(seed[i])) for i in range(n)]
        rec["r" + tag] = np.stack([p[0] for p in pairs])
        rec["a" + tag] = np.stack([p[1] for p in pairs])
    groups = so64.groups()
    return dict(cloud=cloud, poses=poses, infos=infos, h=h, w=w, n=n, P=so64.P, views=views, so64=so64, so32=so32, flagged=flagged, seed=seed,
                group=np.stack([pair_rows(groups, i) for i in range(n)]), **rec)


def sph_group_stats(ratios, group):
    """{(pair group, record group): (worst, mean)} of pair_ratios' rows, whose pair groups are `group` (indices into SPH_GROUPS)."""
    out = {}
    for gi, gname in enumerate(SPH_GROUPS):
        for k, v in group_stats(ratios[group == gi]).items():
            out[gname, k] = v
    return out


def sph_reached(name: str) -> dict:
    """The mechanisms a spherical scene is built for, counted on the float64 oracle: visible pole-clamped pairs per planted ratio
    and pole, Gaussians with both pairs visible, pairs over 32 tiles."""
    sc = sph_scene(name)
    so = sc["so64"]
    P, vis = sc["P"], so.visible
    out = dict(both_pairs=0, over_32_tiles=0)
    clamped_pole = so.rho_over_r() < POLE_CLAMP
    for i, info in enumerate(sc["infos"]):
        v = vis[2 * i] | vis[2 * i + 1]
        out["both_pairs"] += int((vis[2 * i] & vis[2 * i + 1]).sum())
        out["over_32_tiles"] += int((so.fwd[i]["tiles_touched"] > 32).sum())
        for ratio in POLE_RATIOS:
            for sign in (1, -1):
                mine = (info["pole_ratio"] == ratio) & (info["pole_sign"] == sign) & v
                assert (clamped_pole[i][mine] == (ratio < POLE_CLAMP)).all()
                key = f"{'north' if sign > 0 else 'south'}_{ratio}"
                out[key] = out.get(key, 0) + int(mine.sum())
        out["seam_both"] = out.get("seam_both", 0) + int((info["seam"] & vis[2 * i] & vis[2 * i + 1]).sum())
    return out


# ------------------------------------------------------------------------------------------------- spherical chain cases (test B)
def sph_role_cloud(p: int, poses, m: int = 25, seed: int = 0):
    """uniform cloud of p Gaussians; role by index mod 8: 0 inside the radial cull of panorama 0 (r <= 0.2 scaled units: invisible
    there) | 1, 2, 3 one / two / three clamped colour channels | 4 .. 7 plain; the last 12 + 6 rows per pose are planted poles (one
    per ratio and pole) and seam Gaussians."""
    from splatter360_amd import synthetic
    c = synthetic.uniform_cloud(p, d_sh=m, seed=seed, extent=2.0, scale_range=(0.05, 0.4))
    rng = np.random.default_rng(seed + 1000)
    role = np.arange(p) % 8
    d = rng.standard_normal((p, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c["means"][role == 0] = (poses[0][:3, 3] + 0.01 * d)[role == 0]
    for n_ch, ro in ((1, 1), (2, 2), (3, 3)):
        c["harmonics"][role == ro, :n_ch, 0] = -4.0
        c["harmonics"][role == ro, :n_ch, 1:] *= 0.1
    first = p - 18 * len(poses)
    infos = []
    for pose in poses:
        infos.append(plant_sphere(c, first, pose, rng, 1, 6))
        first += 18
    return c, role, infos


@functools.lru_cache(maxsize=None)
def sph_chain_setup(p: int, m: int = 25, deg: int = 4, kind: str = "one", colors: bool = False) -> dict:
    """Cloud, views and both precisions' oracles of one spherical chain case on 32 x 64.  kind "one": one panorama (a shared camera
    centre); "two": two panoramas at different poses in one call."""
    poses = [sph_pose()] if kind == "one" else [sph_pose(), sph_pose((-0.3, 0.25, -0.15), seed=9)]
    cloud, role, infos = sph_role_cloud(p, poses, m, seed=p)
    views = sph_views(poses)
    col = np.random.default_rng(p).uniform(0.0, 1.0, (p, 3)).astype(np.float32) if colors else None
    so = {dt: SphereOracles(views, cloud, 32, 64, deg, dt, col) for dt in (np.float64, np.float32)}
    return dict(cloud=cloud, role=role, infos=infos, views=views, colors=col, so64=so[np.float64], so32=so[np.float32], deg=deg, m=m, h=32, w=64)


# ================================================================================ the raw-input backward's tail (s360_backward_raw*)
def sh_block_slices(d_sh: int = 25):
    return [(l * l, (l + 1) ** 2) for l in range(int(round(np.sqrt(d_sh))))]


def raw_rank1_harmonics(tt, means32, group_views, d_rgb_sum):
    """g_harm[P,3,25] = sum over the camera groups of Y_k(dir_group) dRGB_group[c] in the torch dtype tt: what k_raw_bwd forms in
    place of a dL/dSH buffer.  dir = normalise(mean x scale - campos) with the kernels' float32 forward means and the group's
    camera record (views[w], w = the int32 bits of d_rgb_sum[..., 3]); a group whose w is -1 contributes 0."""
    from oracle import torch_ref
    means = torch.as_tensor(means32, dtype=torch.float32).to(tt)
    views = torch.as_tensor(np.asarray(group_views, np.float32))
    rgb = torch.as_tensor(np.asarray(d_rgb_sum, np.float32)).reshape(-1, means.shape[0], 4)
    g = torch.zeros((means.shape[0], 3, 25), dtype=tt)
    for j in range(rgb.shape[0]):
        w = rgb[j, :, 3].contiguous().view(torch.int32).long()
        ok = w >= 0
        vw = views[w.clamp_min(0)].to(tt)
        d = means * vw[:, 40:41] - vw[:, 32:35]
        d = d * (1 / (d * d).sum(-1, keepdim=True).sqrt())
        y = torch_ref.sh_basis(4, d)                                                           # [P,25]
        g = g + torch.where(ok[:, None, None], y[:, None, :] * rgb[j, :, :3].to(tt)[:, :, None], torch.zeros((), dtype=tt))
    return g


def raw_tail_reference(tt, ext, dep, raw, rot, means32, group_views, d_cov6, d_rgb_sum, d_means, hw, per_ray=1, name="hm3d",
                       smin=0.5, smax=15.0, eps=1e-8):
    """The adapter tail's forward and backward in the torch dtype tt on the CPU (oracle/adapter_ref.adapter_tail_torch + autograd) from
    the cotangents the rasteriser hands k_raw_bwd: d_cov6[P,6] (an off-diagonal entry stands for both symmetric ones),
    d_rgb_sum[n_groups,P,4] through raw_rank1_harmonics, d_means[P,3] or None (the reference's detached means).
    ext[V,4,4], dep[V,Gv], raw[V,Gv,82], rot[V,25,25] or None: float32 tensors.  -> a namespace in the fields of
    tests/test_gpu_adapter_float64.py's _errors (means, cov, scales, rot, harm, d_dep, d_raw) + g_harm, all float64 CPU."""
    from types import SimpleNamespace
    from oracle import adapter_ref
    v, gv = dep.shape
    d = dep.detach().to(tt).requires_grad_(True)
    r = raw.detach().to(tt).requires_grad_(True)
    out = adapter_ref.adapter_tail_torch(ext.to(tt), d, torch.zeros((v, gv), dtype=tt), r, hw, smin, smax, sh_rotation=None if rot is None else rot.to(tt),
                                         eps=eps, per_ray=per_ray, differentiable_means=d_means is not None, dataset_name=name)
    g_harm = raw_rank1_harmonics(tt, means32, group_views, d_rgb_sum).reshape(v, gv, 3, 25)
    r_, c_ = torch.triu_indices(3, 3)
    loss = (out.covariances[:, :, r_, c_] * torch.as_tensor(np.asarray(d_cov6, np.float32)).to(tt).reshape(v, gv, 6)).sum() + (out.harmonics * g_harm).sum()
    if d_means is not None:
        loss = loss + (out.means * torch.as_tensor(np.asarray(d_means, np.float32)).to(tt).reshape(v, gv, 3)).sum()
    loss.backward()
    f = lambda x: x.detach().double()
    return SimpleNamespace(means=f(out.means), cov=f(out.covariances), scales=f(out.scales), rot=f(out.rotations), harm=f(out.harmonics),
                           d_dep=f(d.grad), d_raw=f(r.grad), g_harm=f(g_harm))


def raw_colours(tt, harm, means32, view):
    """(colour before the clamp [P,3], its condition 0.5 + sum_k |Y_k h_k|) of k_raw_eval in the torch dtype tt: 0.5 + sum_k Y_k h_k
    with h = D (mask . raw) (harm[P,3,25], any dtype) and dir from the kernels' float32 means and the call's first camera record."""
    from oracle import torch_ref
    vw = torch.as_tensor(np.asarray(view, np.float32)).to(tt)
    d = torch.as_tensor(means32, dtype=torch.float32).to(tt) * vw[40] - vw[32:35]
    d = d * (1 / (d * d).sum(-1, keepdim=True).sqrt())
    terms = torch_ref.sh_basis(4, d)[:, None, :] * harm.to(tt).reshape(-1, 3, 25)
    return (terms.sum(-1) + 0.5).double(), (terms.double().abs().sum(-1) + 0.5)
