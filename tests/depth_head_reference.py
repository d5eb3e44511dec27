"""The encoder's softmax depth head stated in plain torch, for any dtype and device: what splatter360_amd/depth_head.py is tested
against.  The project's own few lines; the statement the reference's predictor makes after its refinement U-Net
(src/model/encoder/costvolume/depth_predictor_multiview_360.py:643-651)."""
import types

import torch


def head(logits, cand, dtype=torch.float64):
    """logits [n, D, h, w], cand [n, D] or [n, D, 1, 1] -> (depth, pmax), both [n, 1, h, w], in `dtype`."""
    z = logits.to(dtype)
    c = cand.to(dtype).reshape(z.shape[0], z.shape[1], 1, 1)
    pdf = torch.softmax(z, dim=1)
    depth = (c * pdf).sum(dim=1, keepdim=True)
    pmax = torch.max(pdf, dim=1, keepdim=True)[0]
    return depth, pmax


def logits_gradient(logits, cand, g_depth, g_pmax, dtype=torch.float64):
    """d (sum g_depth depth + sum g_pmax pmax) / d logits by autograd, in `dtype`; either gradient may be None."""
    z = logits.detach().to(dtype).requires_grad_(True)
    outs = [o for o, g in zip(head(z, cand, dtype), (g_depth, g_pmax)) if g is not None]
    grads = [g.to(dtype) for g in (g_depth, g_pmax) if g is not None]
    return torch.autograd.grad(outs, z, grads)[0]


def formula_gradient(logits, cand, g_depth, g_pmax, dtype=torch.float64):
    """The closed form the backward kernel evaluates: g_z[d] = p_d (g_depth (c_d - depth) - g_pmax pmax) + [d == a] g_pmax pmax."""
    z = logits.to(dtype)
    c = cand.to(dtype).reshape(z.shape[0], z.shape[1], 1, 1)
    pdf = torch.softmax(z, dim=1)
    depth, (pmax, a) = (c * pdf).sum(dim=1, keepdim=True), torch.max(pdf, dim=1, keepdim=True)
    gd = torch.zeros_like(depth) if g_depth is None else g_depth.to(dtype)
    gp = torch.zeros_like(depth) if g_pmax is None else g_pmax.to(dtype)
    return pdf * (gd * (c - depth) - gp * pmax) + torch.zeros_like(z).scatter_(1, a, gp * pmax)


def random_case(shape, scale, sampling, seed, device="cpu"):
    """(logits, candidates [n, D], g_depth, g_pmax): logits randn * scale, candidates of cost_volume.depth_candidates for near in
    [0.1, 0.5] and far in [5, 10], gradients randn."""
    from splatter360_amd import cost_volume as cv
    n, d, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    logits = (torch.randn(n, d, h, w, generator=gen) * scale).to(device)
    near = (0.1 + 0.4 * torch.rand(1, n, generator=gen)).to(device)
    far = (5.0 + 5.0 * torch.rand(1, n, generator=gen)).to(device)
    cand = cv.depth_candidates(near, far, d, sampling).to(torch.float32).contiguous()
    g_depth, g_pmax = (torch.randn(n, 1, h, w, generator=gen).to(device) for _ in range(2))
    return logits, cand, g_depth, g_pmax


STANDIN_SOURCE = """
import torch
import torch.nn.functional as F


def depth_head(logits, depth_candi_curr, keepdim=True):
    pdf = F.softmax(logits, dim=1)
    coarse_depths = (depth_candi_curr * pdf).sum(dim=1, keepdim=keepdim)
    pdf_max = torch.max(pdf, dim=1, keepdim=keepdim)[0]
    return coarse_depths, pdf_max


def upsample(x, factor):
    return F.interpolate(x, scale_factor=factor)
"""


def standin_module(name):
    """A stand-in for the predictor's module: it binds torch.nn.functional as `F` and makes the three calls through that name."""
    mod = types.ModuleType(name)
    exec(compile(STANDIN_SOURCE, name, "exec"), mod.__dict__)
    return mod
