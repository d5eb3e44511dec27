"""The encoder's fine-depth and opacity tail stated in plain torch, for any dtype and device: what splatter360_amd/depth_tail.py is
tested against, at float64 as the yardstick and at float32 as "what torch does".  The project's own few lines; the statements the
reference makes in src/model/encoder/costvolume/depth_predictor_multiview_360.py:650-658 and :694-719 and in
src/model/encoder/encoder_costvolume.py:228-241, :420, written out, not imported."""
import types

import torch
import torch.nn.functional as F
from einops import rearrange, repeat


def upsample(x, s, mode, reciprocal=False, dtype=torch.float64):
    """F.interpolate itself on x [n, 1, h, w] (of 1 / x with reciprocal), in `dtype`."""
    x = x.to(dtype)
    if reciprocal:
        x = 1 / x
    if mode == "nearest":
        return F.interpolate(x, scale_factor=s)
    return F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=True)


def fullres_maps(coarse_depths, pdf_max, s, dtype=torch.float64):
    """:650-658 -> (fullres_disps, pdf_max)."""
    coarse_disps = 1 / coarse_depths.to(dtype)
    pdf_max = F.interpolate(pdf_max.to(dtype), scale_factor=s)
    fullres_disps = F.interpolate(coarse_disps, scale_factor=s, mode="bilinear", align_corners=True)
    return fullres_disps, pdf_max


def bounds(near, far):
    """(lo, hi) [(v b), 1, 1, 1] in float32, as the reference forms them from its float32 near / far [b, v]."""
    return 1.0 / far.t().reshape(-1, 1, 1, 1), 1.0 / near.t().reshape(-1, 1, 1, 1)


def map_pdf_to_opacity(pdf, exponent):
    return 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent))


def tail_planes(fullres_disps, delta_disps_density, near, far, gpp, exponent, dtype=torch.float64):
    """:694-712 and the encoder's opacity before any relayout: (depths, opacities, densities, sum, lo, hi), the first three
    [(v b), gpp, H, W] in `dtype`; `sum` is fullres + delta as `dtype` adds it, lo / hi the float32 bounds cast to `dtype`."""
    lo, hi = (t.to(dtype) for t in bounds(near, far))
    delta_disps, raw_densities = delta_disps_density.to(dtype).split(gpp, dim=1)
    densities = torch.sigmoid(raw_densities)
    total = fullres_disps.to(dtype) + delta_disps
    fine_disps = total.clamp(lo, hi)
    depths = 1.0 / fine_disps
    opacities = map_pdf_to_opacity(densities, exponent) / gpp
    return depths, opacities, densities, total, lo, hi


def relayout(x, b, v):
    """The reference's einops pattern (:700-719)."""
    return repeat(x, "(v b) dpt h w -> b v (h w) srf dpt", b=b, v=v, srf=1)


def planes(x, h, w):
    """The other way: [b, v, h w, 1, gpp] -> [(v b), gpp, h, w]."""
    return rearrange(x, "b v (h w) srf dpt -> (v b) (srf dpt) h w", h=h, w=w)


def tail(fullres_disps, delta_disps_density, near, far, gpp, exponent, dtype=torch.float64):
    """(depths, opacities, densities), each [b, v, H W, 1, gpp] in `dtype`."""
    b, v = near.shape
    return tuple(relayout(x, b, v) for x in tail_planes(fullres_disps, delta_disps_density, near, far, gpp, exponent, dtype)[:3])


def tail_gradient(fullres_disps, delta_disps_density, near, far, gpp, exponent, grads, dtype=torch.float64):
    """(g_fullres_disps, g_delta_disps_density) of sum_i <grads[i], out_i> by autograd, in `dtype`; a gradient may be None."""
    f = fullres_disps.detach().to(dtype).requires_grad_(True)
    d = delta_disps_density.detach().to(dtype).requires_grad_(True)
    pairs = [(o, g.to(dtype)) for o, g in zip(tail(f, d, near, far, gpp, exponent, dtype), grads) if g is not None]
    return torch.autograd.grad([o for o, _ in pairs], (f, d), [g for _, g in pairs])


def opacity_logit_slope(x, exponent, gpp=1):
    """The closed form the tail's backward evaluates: d opacity / d x = (e (1 - p)^e p + (1 / e) p^(1 / e) (1 - p)) / (2 gpp), with
    1 - p taken as sigmoid(-x), which keeps its digits where 1 - sigmoid(x) cancels."""
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    return 0.5 * (exponent * q ** exponent * p + (1 / exponent) * p ** (1 / exponent) * q) / gpp


def clamp_pass(total, lo, hi):
    """Where torch's clamp backward passes the gradient: bounds included."""
    return (total >= lo) & (total <= hi)


def random_case(b, v, h, w, gpp, seed, device="cpu"):
    """(fullres_disps, delta_disps_density, near, far, g_depths, g_opacities, g_densities): near = (0.1, 0.5, ...), far =
    (100, 20, ...) over the b v views, fullres = lo - 0.1 (hi - lo) + 1.2 (hi - lo) U[0, 1) so that both sides of the clamp are
    exercised, delta ~ 0.3 N(0, 1), density logits ~ 3 N(0, 1), gradients N(0, 1)."""
    gen = torch.Generator().manual_seed(seed)
    n = b * v
    near = torch.tensor([(0.1, 0.5)[i % 2] for i in range(n)], dtype=torch.float32).reshape(b, v)
    far = torch.tensor([(100.0, 20.0)[i % 2] for i in range(n)], dtype=torch.float32).reshape(b, v)
    lo, hi = bounds(near, far)
    fullres = lo - 0.1 * (hi - lo) + 1.2 * (hi - lo) * torch.rand(n, 1, h, w, generator=gen)
    delta = 0.3 * torch.randn(n, gpp, h, w, generator=gen)
    logits = 3.0 * torch.randn(n, gpp, h, w, generator=gen)
    grads = [torch.randn(b, v, h * w, 1, gpp, generator=gen) for _ in range(3)]
    return tuple(t.to(device) for t in (fullres, torch.cat((delta, logits), dim=1), near, far, *grads))


def random_maps(n, h, w, s, seed, device="cpu"):
    """(coarse_depths in [0.5, 10), pdf_max in (0, 1], g_fullres_disps, g_pdf_max) for the two interpolations."""
    gen = torch.Generator().manual_seed(seed)
    depth = 0.5 + 9.5 * torch.rand(n, 1, h, w, generator=gen)
    pmax = 1.0 - torch.rand(n, 1, h, w, generator=gen)
    grads = [torch.randn(n, 1, h * s, w * s, generator=gen) for _ in range(2)]
    return tuple(t.to(device) for t in (depth, pmax, *grads))


PREDICTOR_SOURCE = """
import torch
import torch.nn.functional as F


def depth_head(logits, depth_candi_curr, keepdim=True):
    pdf = F.softmax(logits, dim=1)
    coarse_depths = (depth_candi_curr * pdf).sum(dim=1, keepdim=keepdim)
    pdf_max = torch.max(pdf, dim=1, keepdim=keepdim)[0]
    return coarse_depths, pdf_max


def fullres(coarse_depths, pdf_max, upscale_factor):
    coarse_disps = 1 / coarse_depths
    pdf_max = F.interpolate(pdf_max, scale_factor=upscale_factor)
    fullres_disps = F.interpolate(
        coarse_disps,
        scale_factor=upscale_factor,
        mode="bilinear",
        align_corners=True,
    )
    return fullres_disps, pdf_max


def half_pixel(x, factor):
    return F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False)
"""

ENCODER_SOURCE = """
import types


class EncoderCostVolume:
    def __init__(self, initial=0.0, final=0.0, warm_up=1):
        self.cfg = types.SimpleNamespace(opacity_mapping=types.SimpleNamespace(initial=initial, final=final, warm_up=warm_up))

    def map_pdf_to_opacity(self, pdf, global_step):
        cfg = self.cfg.opacity_mapping
        x = cfg.initial + min(global_step / cfg.warm_up, 1) * (cfg.final - cfg.initial)
        exponent = 2**x
        return 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent))
"""


def standin_module(name, source):
    """A stand-in for one of the reference's two modules: the predictor's binds torch.nn.functional as `F` and makes its calls
    through that name; the encoder's defines EncoderCostVolume.map_pdf_to_opacity."""
    mod = types.ModuleType(name)
    exec(compile(source, name, "exec"), mod.__dict__)
    return mod
