"""A plain torch statement of the encoder's spherical cost volume (the 'hm3d' / 'replica' convention), in the reference's operation
order, for any dtype and device: float32 gives the reference's own numbers up to rounding order, float64 is the yardstick of the
GPU tests.  The depth axis can be walked in chunks, so the [n, C, D, h, w] warped tensor of the full workload never has to exist
at once.  Not a test module."""
import math

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
