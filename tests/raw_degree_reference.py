"""Degree-general forms of tests/backward_reference.py's raw-path references (raw_rank1_harmonics, raw_tail_reference, raw_colours are
fixed there at 25 coefficients and sh_basis(4, .)): the raw-input path at d_sh = (degree + 1)^2 in {1, 4, 9, 16, 25}.  Built on
oracle/adapter_ref.adapter_tail_torch and oracle/torch_ref.sh_basis(degree, .); sh_block_slices is general already and is imported."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from backward_reference import sh_block_slices  # noqa: F401  (general: re-exported for the tests)
from oracle import adapter_ref, torch_ref


def degree_of(d_sh: int) -> int:
    deg = math.isqrt(int(d_sh)) - 1
    assert (deg + 1) ** 2 == d_sh and 0 <= deg <= 4, d_sh
    return deg


def _directions(tt, means32, vw):
    """normalise(mean x scale - campos) in the dtype tt from the kernels' float32 means and per-Gaussian camera records vw[P,44]."""
    d = torch.as_tensor(means32, dtype=torch.float32).to(tt) * vw[:, 40:41] - vw[:, 32:35]
    return d * (1 / (d * d).sum(-1, keepdim=True).sqrt())


def raw_rank1_harmonics(tt, means32, group_views, d_rgb_sum, d_sh):
    """g_harm[P,3,d_sh] = sum over the camera groups of Y_k(dir_group) dRGB_group[c] in the torch dtype tt: what k_raw_bwd forms in
    place of a dL/dSH buffer.  The group's camera record is views[w], w = the int32 bits of d_rgb_sum[..., 3]; w = -1 contributes 0."""
    deg = degree_of(d_sh)
    p = int(torch.as_tensor(means32).shape[0])
    views = torch.as_tensor(np.asarray(group_views, np.float32))
    rgb = torch.as_tensor(np.asarray(d_rgb_sum, np.float32)).reshape(-1, p, 4)
    g = torch.zeros((p, 3, d_sh), dtype=tt)
    for j in range(rgb.shape[0]):
        w = rgb[j, :, 3].contiguous().view(torch.int32).long()
        y = torch_ref.sh_basis(deg, _directions(tt, means32, views[w.clamp_min(0)].to(tt)))[:, :d_sh]          # [P,d_sh]
        g = g + torch.where((w >= 0)[:, None, None], y[:, None, :] * rgb[j, :, :3].to(tt)[:, :, None], torch.zeros((), dtype=tt))
    return g


def raw_tail_reference(tt, ext, dep, raw, rot, means32, group_views, d_cov6, d_rgb_sum, d_means, hw, per_ray=1, name="hm3d",
                       smin=0.5, smax=15.0, eps=1e-8):
    """backward_reference.raw_tail_reference at the degree of `raw` ([V,Gv,7 + 3 d_sh]; rot [V,d_sh,d_sh] or None): the adapter tail's
    forward and backward in the torch dtype tt on the CPU from the cotangents the rasteriser hands k_raw_bwd.  -> the namespace of
    tests/test_gpu_adapter_float64.py's _errors (means, cov, scales, rot, harm, d_dep, d_raw) + g_harm, all float64 CPU."""
    v, gv = dep.shape
    d_sh = (int(raw.shape[-1]) - 7) // 3
    d = dep.detach().to(tt).requires_grad_(True)
    r = raw.detach().to(tt).requires_grad_(True)
    out = adapter_ref.adapter_tail_torch(ext.to(tt), d, torch.zeros((v, gv), dtype=tt), r, hw, smin, smax, sh_rotation=None if rot is None else rot.to(tt),
                                         eps=eps, per_ray=per_ray, differentiable_means=d_means is not None, dataset_name=name)
    g_harm = raw_rank1_harmonics(tt, means32, group_views, d_rgb_sum, d_sh).reshape(v, gv, 3, d_sh)
    r_, c_ = torch.triu_indices(3, 3)
    loss = (out.covariances[:, :, r_, c_] * torch.as_tensor(np.asarray(d_cov6, np.float32)).to(tt).reshape(v, gv, 6)).sum() + (out.harmonics * g_harm).sum()
    if d_means is not None:
        loss = loss + (out.means * torch.as_tensor(np.asarray(d_means, np.float32)).to(tt).reshape(v, gv, 3)).sum()
    loss.backward()
    f = lambda x: x.detach().double()
    return SimpleNamespace(means=f(out.means), cov=f(out.covariances), scales=f(out.scales), rot=f(out.rotations), harm=f(out.harmonics),
                           d_dep=f(d.grad), d_raw=f(r.grad), g_harm=f(g_harm))


def raw_colours(tt, harm, means32, view):
    """(colour before the clamp [P,3], its condition 0.5 + sum_k |Y_k h_k|) of k_raw_eval in the torch dtype tt, harm[..., 3, d_sh]."""
    d_sh = int(harm.shape[-1])
    vw = torch.as_tensor(np.asarray(view, np.float32)).to(tt).reshape(1, -1)
    y = torch_ref.sh_basis(degree_of(d_sh), _directions(tt, means32, vw))[:, :d_sh]
    terms = y[:, None, :] * harm.to(tt).reshape(-1, 3, d_sh)
    return (terms.sum(-1) + 0.5).double(), (terms.double().abs().sum(-1) + 0.5)
