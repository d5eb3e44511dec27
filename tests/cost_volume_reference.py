"""A plain torch statement of the encoder's spherical cost volume (the 'hm3d' / 'replica' convention), in the reference's operation
order, for any dtype and device: float32 gives the reference's own numbers up to rounding order, float64 is the yardstick of the
GPU tests.  The depth axis can be walked in chunks, so the [n, C, D, h, w] warped tensor of the full workload never has to exist
at once.  Not a test module."""
import math
import types

import torch
import torch.nn.functional as F


def warp(pose, depths, h, w, dtype=torch.float64):
    """pose [n, 4, 4], depths [n, D] -> (grid [n, D, h w, 2] normalised for an align_corners=True sampler, as the reference feeds
    it; points [n, D, h w, 3]: the warped points).  Everything in `dtype` on pose's device."""
    dev = pose.device
    pose, depths = pose.to(dtype), depths.to(dtype)
    n, d = depths.shape
    x = torch.linspace(0, w - 1, w, dtype=dtype, device=dev).view(1, w).expand(h, w)
    y = torch.linspace(0, h - 1, h, dtype=dtype, device=dev).view(h, 1).expand(h, w)
    theta = (0.5 - (x + 0.5) / w) * 2 * math.pi
    phi = -((y + 0.5) / h - 0.5) * math.pi
    rad = depths.view(n, d, 1, 1)
    py = torch.sin(phi) * rad
    px = torch.cos(phi) * torch.sin(theta) * rad
    pz = torch.cos(phi) * torch.cos(theta) * rad
    pts = torch.stack((px, py, pz), dim=2).reshape(n, d, 3, h * w)
    pts = pose[:, None, :3, :3] @ pts + pose[:, None, :3, -1:]
    pts = pts.transpose(2, 3)                                   # [n, D, h w, 3]
    qx, qy, qz = pts[..., 0], pts[..., 1], pts[..., 2]
    theta2 = torch.atan2(qx, qz)
    phi2 = torch.atan2(qy, torch.sqrt(qx ** 2 + qz ** 2))
    xl = (-theta2 / (2 * math.pi) + 0.5) * w - 0.5
    yl = (-phi2 / math.pi + 0.5) * h - 0.5
    u = (xl + 0.5) / w
    v = (yl + 0.5) / h
    u = u * 2.0 - 1.0
    v = v * 2.0 - 1.0
    return torch.stack([u, v], dim=-1), pts


def warped_features(f_partner, pose, depths, dtype=torch.float64):
    """[n, C, h, w] -> the materialised [n, C, D, h, w] tensor of warp_with_pose_depth_candidates."""
    n, c, h, w = f_partner.shape
    d = depths.shape[1]
    grid, _ = warp(pose, depths, h, w, dtype)
    out = F.grid_sample(f_partner.to(dtype).contiguous(), grid.view(n, d * h, w, 2).contiguous(), mode="bilinear", padding_mode="zeros",
                        align_corners=True)
    return out.view(n, c, d, h, w)


def pair_sum(f_own, f_partner, pose, depths, dtype=torch.float64, chunk=None):
    """sum_c f_own * warped(f_partner) -> [n, D, h, w] (not divided by sqrt C), `chunk` depths at a time."""
    d = depths.shape[1]
    chunk = chunk or d
    own = f_own.to(dtype).unsqueeze(2)
    return torch.cat([(own * warped_features(f_partner, pose, depths[:, s:s + chunk], dtype)).sum(1) for s in range(0, d, chunk)], dim=1)


def partner_order(v, idx):
    order = list(range(v))
    return order[idx:] + order[:idx]


def cost_volume(features, poses, depths, dtype=torch.float64, chunk=None):
    """features [b, v, C, h, w], poses [v - 1, v b, 4, 4], depths [v b, D] -> [v b, D, h, w]: per rolled pairing the sum over
    channels / sqrt(C), then the mean over the pairings (stack + mean), as the reference writes it."""
    b, v, c, h, w = features.shape
    feat01 = features.transpose(0, 1).reshape(v * b, c, h, w)
    vols = []
    for idx in range(1, v):
        feat10 = features[:, partner_order(v, idx)].transpose(0, 1).reshape(v * b, c, h, w)
        vols.append(pair_sum(feat01, feat10, poses[idx - 1], depths, dtype, chunk) / (c ** 0.5))
    return torch.mean(torch.stack(vols, dim=0), dim=0, keepdim=False)


def feature_gradient(features, poses, depths, g, dtype=torch.float64, chunk=None):
    """autograd's gradient of sum(cost_volume * g) with respect to features, `chunk` depths at a time."""
    f = features.detach().to(dtype).requires_grad_(True)
    d = depths.shape[1]
    chunk = chunk or d
    for s in range(0, d, chunk):
        vol = cost_volume(f, poses, depths[:, s:s + chunk], dtype)
        (vol * g[:, s:s + chunk].to(dtype)).sum().backward()
    return f.grad


def well_conditioned(poses, depths, h, w, chunk=None):
    """bool [v - 1, v b, D, h w]: the samples whose float64 warped point p is away from the poles (rho / |p| >= 1e-2,
    rho = sqrt(x^2 + z^2)), from the partner's centre (|p| >= 1e-2 depth) and from the ERP seam (pi - |theta| >= 1e-3)."""
    d = depths.shape[1]
    chunk = chunk or d
    out = []
    for k in range(poses.shape[0]):
        parts = []
        for s in range(0, d, chunk):
            dep = depths[:, s:s + chunk].to(torch.float64)
            _, p = warp(poses[k], dep, h, w, torch.float64)
            rho = torch.sqrt(p[..., 0] ** 2 + p[..., 2] ** 2)
            r = torch.linalg.norm(p, dim=-1)
            theta = torch.atan2(p[..., 0], p[..., 2])
            parts.append((rho >= 1e-2 * r) & (r >= 1e-2 * dep[:, :, None]) & (math.pi - theta.abs() >= 1e-3))
        out.append(torch.cat(parts, dim=1))
    return torch.stack(out, dim=0)


def random_inputs(b, v, c, h, w, seed, device="cpu", rotation=0.3, translation=0.5, near=0.5, far=20.0):
    """White-noise features and camera-to-world poses with rotations of about `rotation` rad and translations of about
    `translation`."""
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(b, v, c, h, w, generator=gen)
    ext = torch.eye(4).repeat(b, v, 1, 1)
    rv = torch.randn(b, v, 3, generator=gen)
    rv = rv / rv.norm(dim=-1, keepdim=True) * rotation * (0.5 + torch.rand(b, v, 1, generator=gen))
    k = torch.zeros(b, v, 3, 3)
    k[..., 0, 1], k[..., 0, 2], k[..., 1, 2] = -rv[..., 2], rv[..., 1], -rv[..., 0]
    k = k - k.transpose(-1, -2)
    ext[..., :3, :3] = torch.linalg.matrix_exp(k)
    ext[..., :3, 3] = torch.randn(b, v, 3, generator=gen) * translation / math.sqrt(3.0)
    nr = torch.full((b, v), float(near)) * (1.0 + 0.1 * torch.rand(b, v, generator=gen))
    fr = torch.full((b, v), float(far)) * (1.0 + 0.1 * torch.rand(b, v, generator=gen))
    return tuple(t.to(device) for t in (feats, ext, nr, fr))


# ---- the per-element float64 statement with the magnitude of its terms (tests/test_cost_volume_terms.py, tests/test_gpu_cost_volume_terms.py)
#
# Everything below is float64 torch on the CPU, whatever device the arguments live on, and is written at the level of the C entry
# points: f_own [n, C, h, w], f_partner [m, C, h, w], slots [pairs, n] (or None: slot i), poses [pairs, n, 4, 4], depths [n, D],
# one `scale`.  A slot outside [0, m) contributes nothing, as include/s360.h documents.


def taps(pose, depths, h, w):
    """The four bilinear taps of every sample of one pairing, from warp()'s grid: ix = (u + 1) / 2 (w - 1), iy likewise, x0, y0 =
    floor, wx, wy the fractions.  A sample is valid when its position is finite and inside (-1, w) x (-1, h); a tap is inside
    when its sample is valid and the texel exists.  -> namespace of x0, y0 int64 [n, D, h w], valid bool [n, D, h w], lin int64
    [n, D, h w, 4] (y w + x of tap t = 2 dy + dx; 0 where not inside), wt float64 [n, D, h w, 4] (the bilinear weights; 0 where
    not inside) and inside bool [n, D, h w, 4]."""
    grid, _ = warp(pose.detach().cpu(), depths.detach().cpu(), h, w, torch.float64)
    ix = (grid[..., 0] + 1.0) / 2.0 * (w - 1)
    iy = (grid[..., 1] + 1.0) / 2.0 * (h - 1)
    valid = torch.isfinite(ix) & torch.isfinite(iy) & (ix > -1.0) & (ix < w) & (iy > -1.0) & (iy < h)
    ix, iy = torch.where(valid, ix, torch.zeros_like(ix)), torch.where(valid, iy, torch.zeros_like(iy))
    fx, fy = torch.floor(ix), torch.floor(iy)
    wx, wy = ix - fx, iy - fy
    x0, y0 = fx.long(), fy.long()
    xs = torch.stack((x0, x0 + 1, x0, x0 + 1), dim=-1)
    ys = torch.stack((y0, y0, y0 + 1, y0 + 1), dim=-1)
    wt = torch.stack(((1 - wx) * (1 - wy), wx * (1 - wy), (1 - wx) * wy, wx * wy), dim=-1)
    inside = valid[..., None] & (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    lin = torch.where(inside, ys * w + xs, torch.zeros_like(xs))
    wt = torch.where(inside, wt, torch.zeros_like(wt))
    return types.SimpleNamespace(x0=x0, y0=y0, valid=valid, lin=lin, wt=wt, inside=inside)


def rolled_slots(b, v):
    """int64 [v - 1, v b]: the (v b) slot that pairing idx samples for slot k b + i (cost_volume.partner_slots, restated)."""
    return torch.tensor([[partner_order(v, idx)[k] * b + i for k in range(v) for i in range(b)] for idx in range(1, v)])


def _cpu64(t):
    return t.detach().cpu().to(torch.float64)


def _pairings(slots, poses, depths, n, m, h, w):
    """Yields (the taps of pairing k, i, slot) for every (k, i) whose slot lies in [0, m)."""
    for k in range(poses.shape[0]):
        t = taps(poses[k], depths, h, w)
        for i in range(n):
            s = i if slots is None else int(slots[k][i])
            if 0 <= s < m:
                yield t, i, s


def _gather(plane, t, i):
    """plane [C, h w] -> the taps of slot-row i [C, D, h w, 4], zero where a tap is not inside."""
    return plane[:, t.lin[i]] * t.inside[i]


def correlation_terms(f_own, f_partner, slots, poses, depths, scale):
    """Per (n, d, pixel): V = scale sum_pairing sum_c o_c sum_t w_t tap_{t,c} and its magnitude A = |scale| sum_pairing sum_c
    |o_c| sum_t |tap_{t,c}| (unit weights: the kernel's weight error is absolute, not relative to the weight) -> two
    [n, D, h, w]."""
    n, c, h, w = f_own.shape
    m, d = f_partner.shape[0], depths.shape[1]
    fo, fp = _cpu64(f_own).reshape(n, c, h * w), _cpu64(f_partner).reshape(m, c, h * w)
    val, mag = torch.zeros(n, d, h * w, dtype=torch.float64), torch.zeros(n, d, h * w, dtype=torch.float64)
    for t, i, s in _pairings(slots, poses, depths, n, m, h, w):
        tap = _gather(fp[s], t, i)
        val[i] += (fo[i][:, None, :] * (tap * t.wt[i]).sum(-1)).sum(0)
        mag[i] += (fo[i].abs()[:, None, :] * tap.abs().sum(-1)).sum(0)
    return (val * scale).view(n, d, h, w), (mag * abs(scale)).view(n, d, h, w)


def volume_terms(features, poses, depths):
    """correlation_terms for spherical_cost_volume's arguments: features [b, v, C, h, w], every rolled pairing, scale =
    1 / ((v - 1) sqrt C) rounded to float32 as the C entry point receives it."""
    b, v, c, h, w = features.shape
    f = features.transpose(0, 1).reshape(v * b, c, h, w)
    return correlation_terms(f, f, rolled_slots(b, v), poses, depths, volume_scale(v, c))


def volume_scale(v, c):
    return torch.tensor(1.0 / ((v - 1) * c ** 0.5), dtype=torch.float32).item()


def own_gradient_terms(g, f_partner, slots, poses, depths, scale):
    """Per (n, c, pixel): scale sum_pairing sum_d g_d sum_t w_t tap_{t,c} and its magnitude |scale| sum_pairing sum_d |g_d|
    sum_t |tap_{t,c}| -> two [n, C, h, w]."""
    n, d, h, w = g.shape
    m, c = f_partner.shape[:2]
    g64, fp = _cpu64(g).reshape(n, 1, d, h * w), _cpu64(f_partner).reshape(m, c, h * w)
    val, mag = torch.zeros(n, c, h * w, dtype=torch.float64), torch.zeros(n, c, h * w, dtype=torch.float64)
    for t, i, s in _pairings(slots, poses, depths, n, m, h, w):
        tap = _gather(fp[s], t, i)
        val[i] += (g64[i] * (tap * t.wt[i]).sum(-1)).sum(1)
        mag[i] += (g64[i].abs() * tap.abs().sum(-1)).sum(1)
    return (val * scale).view(n, c, h, w), (mag * abs(scale)).view(n, c, h, w)


def partner_gradient_terms(g, f_own, m, slots, poses, depths, scale):
    """Per (slot, c, texel): the scatter of scale g w_t o_c over every (pairing, n with that slot, d, pixel, tap) that hits the
    texel, its magnitude (the scatter of |scale g o_c|, unit weights) and the number of terms N (the scatter of ones; the same
    for every channel) -> value, magnitude [m, C, h, w], N [m, h, w]."""
    n, d, h, w = g.shape
    c = f_own.shape[1]
    g64, fo = _cpu64(g).reshape(n, 1, d, h * w, 1), _cpu64(f_own).reshape(n, c, 1, h * w, 1)
    val, mag = torch.zeros(m, c, h * w, dtype=torch.float64), torch.zeros(m, c, h * w, dtype=torch.float64)
    count = torch.zeros(m, h * w, dtype=torch.float64)
    for t, i, s in _pairings(slots, poses, depths, n, m, h, w):
        idx = t.lin[i].reshape(-1)
        val[s].index_add_(1, idx, (scale * g64[i] * t.wt[i] * fo[i]).reshape(c, -1))
        mag[s].index_add_(1, idx, (abs(scale) * g64[i].abs() * t.inside[i] * fo[i].abs()).reshape(c, -1))
        count[s].index_add_(0, idx, t.inside[i].reshape(-1).to(torch.float64))
    return val.view(m, c, h, w), mag.view(m, c, h, w), count.view(m, h, w)


def warp_terms(f_partner, pose, depths):
    """The warped tensor of the _warp entry point, one pairing, slot i: sum_t w_t tap and sum_t |tap| -> two [n, C, D, h, w]."""
    n, c, h, w = f_partner.shape
    fp = _cpu64(f_partner).reshape(n, c, h * w)
    t = taps(pose, depths, h, w)
    tap = torch.stack([_gather(fp[i], t, i) for i in range(n)])
    shape = (n, c, depths.shape[1], h, w)
    return (tap * t.wt[:, None]).sum(-1).view(shape), tap.abs().sum(-1).view(shape)


def near_singular(pose, depths, h, w, tol=1e-9):
    """bool [n, D, h w]: the samples at which the float64 position itself jumps, so that two correct float64 evaluations may
    differ: on the ERP seam (q_z < 0 and |q_x| <= tol rho), at a pole (rho <= tol r) or at the partner's centre (r <= tol
    depth); q the warped point, rho = sqrt(q_x^2 + q_z^2), r = |q|.  The inputs of the per-element tests must have none."""
    dep = _cpu64(depths)
    _, q = warp(pose.detach().cpu(), dep, h, w, torch.float64)
    rho = torch.sqrt(q[..., 0] ** 2 + q[..., 2] ** 2)
    r = torch.linalg.norm(q, dim=-1)
    return ((q[..., 2] < 0) & (q[..., 0].abs() <= tol * rho)) | (rho <= tol * r) | (r <= tol * dep[:, :, None])


def unit_ray(y, x, h, w):
    """The float64 unit ray of pixel (y, x), as warp() forms it."""
    theta = (0.5 - (x + 0.5) / w) * 2 * math.pi
    phi = -((y + 0.5) / h - 0.5) * math.pi
    return torch.tensor([math.cos(phi) * math.sin(theta), math.sin(phi), math.cos(phi) * math.cos(theta)], dtype=torch.float64)


def pose_set(depths, h, w):
    """The hand-made poses of the per-element tests, float32 [1, 4, 4] each (partner from own): identity; 180 degrees about y
    with a translation (the seam comes to the image's middle); 90 degrees about x (the poles come to the equator); identity
    with a tiny translation (every depth of a pixel stays in one tap cell); and a general rotation whose translation puts the
    partner's centre 1e-4 depths[3] beyond the point of pixel (4, 13) at depths[3]."""
    def pose(rot, t):
        p = torch.eye(4, dtype=torch.float64)
        p[:3, :3], p[:3, 3] = torch.as_tensor(rot, dtype=torch.float64), torch.as_tensor(t, dtype=torch.float64)
        return p.to(torch.float32).unsqueeze(0)

    eye = torch.eye(3, dtype=torch.float64)
    k = torch.tensor([[0.0, -0.5, -0.7], [0.5, 0.0, -0.4], [0.7, 0.4, 0.0]], dtype=torch.float64)      # rotation vector (0.4, -0.7, 0.5)
    general = torch.linalg.matrix_exp(k)
    centre = -(general @ unit_ray(4, 13, h, w)) * float(depths.reshape(-1)[3]) * (1.0 + 1e-4)
    return {
        "identity": pose(eye, [0.0, 0.0, 0.0]),
        "half_turn_y": pose([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]], [0.1, 0.0, -0.2]),
        "quarter_turn_x": pose([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]], [0.0, 0.0, 0.0]),
        "tiny_t": pose(eye, [1e-3, -2e-3, 1e-3]),
        "centre": pose(general, centre),
    }


def pose_set_inputs(device="cpu"):
    """The pose set's tensors: f_own, f_partner [1, 5, 12, 20] white noise, depths [1, 7] log-spaced 0.5 ... 20, grad_out
    [1, 7, 12, 20], and the poses by name."""
    gen = torch.Generator().manual_seed(360)
    f_own, f_partner = torch.randn(1, 5, 12, 20, generator=gen), torch.randn(1, 5, 12, 20, generator=gen)
    g = torch.randn(1, 7, 12, 20, generator=gen)
    depths = torch.logspace(math.log10(0.5), math.log10(20.0), 7, dtype=torch.float64).to(torch.float32).view(1, 7)
    poses = {k: p.to(device) for k, p in pose_set(depths, 12, 20).items()}
    return f_own.to(device), f_partner.to(device), depths.to(device), g.to(device), poses


def terms_cases():
    """name -> (b, v, C, D, h, w, sampling) of the per-element tests: tests/test_gpu_cost_volume.py's three small shapes with its
    inputs (random_inputs with seed = sum of the name's character codes), and D = 33 (one depth alone in the second depth
    block)."""
    return {
        "small_v2": (1, 2, 8, 16, 32, 64, "inverse_depth"),
        "odd_v3": (2, 3, 5, 7, 12, 20, "log_depth"),
        "wide_c": (1, 2, 132, 40, 16, 32, "linear_depth"),
        "d33": (1, 2, 4, 33, 8, 16, "inverse_depth"),
    }
