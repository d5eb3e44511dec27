"""The encoder's fine-depth and opacity tail stated in plain torch, for any dtype and device: what splatter360_amd/depth_tail.py is
tested against, at float64 as the yardstick and at float32 as "what torch does".  The project's own few lines; the statements the
reference makes in src/model/encoder/costvolume/depth_predictor_multiview_360.py:650-658 and :694-719 and in
src/model/encoder/encoder_costvolume.py:228-241, :420, written out, not imported."""
import types

import torch
import torch.nn.functional as F
from einops import rearrange, repeat

from depth_head_reference import COND, TINY, UNIT, bound, worst  # noqa: F401  (the measure, shared)


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


# ------------------------------------------------------------------------------------------------ the per-element measure
# bound = 2^-24 |want| + 2^-40 A + 2^-149, as in tests/depth_head_reference.py: one float32 rounding, 2^13 float64 ulps of the
# element's condition A (the sum of the magnitudes of its terms), half the smallest float32 subnormal.
PLANTED_LOGITS = (17.5, -17.5, 20.0, -20.0, 40.0, -40.0, 88.0, -88.0, 100.0, -100.0)


def sigmoid_parts(x):
    """(log p, log(1 - p), p, 1 - p) of p = sigmoid(x) in float64, each to a few ulps of ITSELF for every finite x, from
    t = exp(-|x|) alone: no difference of near-equal numbers is formed.  (torch's 1 - sigmoid(x) keeps no digit from x = 37 on.)"""
    x = x.double()
    t = (-x.abs()).exp()
    lt = torch.log1p(t)
    big, small = 1.0 / (1.0 + t), t / (1.0 + t)
    pos = x >= 0
    return torch.where(pos, -lt, x - lt), torch.where(pos, -x - lt, -lt), torch.where(pos, big, small), torch.where(pos, small, big)


def opacity_elements(x, exponent, gpp=1):
    """The float64 `want` of the tail's opacity, its slope in the logit x, p and p (1 - p), in a form without cancellation:
    1 - (1 - p)^e = -expm1(e log(1 - p)), and every other factor is a product of positive numbers.  Pinned against 200-bit
    arithmetic by tests/test_depth_tail_elements.py.  Returns a dict of opacity, slope, p, pq."""
    lp, lq, p, q = sigmoid_parts(x)
    e = float(exponent)
    root = (lp / e).exp()
    return dict(opacity=(root - torch.special.expm1(e * lq)) * (0.5 / gpp), slope=(e * (e * lq).exp() * p + root * q / e) * (0.5 / gpp), p=p, pq=p * q)


def _taps(n_in, s, mode):
    """The [n_in s, n_in] float64 matrix of one axis of the upsampling, from exact integer taps: nearest takes Y // s; bilinear
    with align_corners=True has the source coordinate Y (h - 1) / (H - 1), so the upper tap's weight is the rational
    (Y (h - 1) mod (H - 1)) / (H - 1)."""
    import numpy as np
    n_out = n_in * s
    m = np.zeros((n_out, n_in))
    for Y in range(n_out):
        if mode == "nearest":
            m[Y, Y // s] = 1.0
        elif n_out == 1:
            m[Y, 0] = 1.0
        else:
            y0, r = divmod(Y * (n_in - 1), n_out - 1)
            m[Y, y0] += (n_out - 1 - r) / (n_out - 1)
            m[Y, min(y0 + 1, n_in - 1)] += r / (n_out - 1)
    return m


def upsample_elements(x, s, mode, reciprocal=False):
    """The project's own numpy statement of the upsampling of x [n, 1, h, w]: (want, A), float64 [n, 1, h s, w s], with
    A = sum_i |w_i v_i| over the taps (v = 1 / x with reciprocal)."""
    import numpy as np
    v = x.detach().cpu().double().numpy()[:, 0]
    if reciprocal:
        v = 1.0 / v
    wy, wx = _taps(v.shape[1], s, mode), _taps(v.shape[2], s, mode)
    want = np.einsum("Yy,nyx,Xx->nYX", wy, v, wx)
    cond = np.einsum("Yy,nyx,Xx->nYX", wy, np.abs(v), wx)
    return torch.from_numpy(want)[:, None], torch.from_numpy(cond)[:, None]


def upsample_backward_elements(g, x, s, mode, reciprocal=False):
    """The adjoint: (want, A) [n, 1, h, w] for g [n, 1, h s, w s]; A = sum |w g|, and both times 1 / x^2 (want: -1 / x^2) with
    reciprocal."""
    import numpy as np
    gg = g.detach().cpu().double().numpy()[:, 0]
    v = x.detach().cpu().double().numpy()[:, 0]
    wy, wx = _taps(v.shape[1], s, mode), _taps(v.shape[2], s, mode)
    want = np.einsum("Yy,nYX,Xx->nyx", wy, gg, wx)
    cond = np.einsum("Yy,nYX,Xx->nyx", wy, np.abs(gg), wx)
    if reciprocal:
        want, cond = -want / (v * v), cond / (v * v)
    return torch.from_numpy(want)[:, None], torch.from_numpy(cond)[:, None]


def clamp_pattern(fullres, delta, lo, hi):
    """Where the tail's backward passes the disparity gradient — its stated contract: lo <= float32(f) + float32(d) <= hi on the
    FLOAT32 sum, bounds included — computed in numpy.  fullres [n, 1, H, W], delta [n, gpp, H, W], lo / hi [n] -> bool tensor."""
    import numpy as np
    f, d = (t.detach().cpu().numpy().astype(np.float32) for t in (fullres, delta))
    l, u = (t.detach().cpu().numpy().astype(np.float32).reshape(-1, 1, 1, 1) for t in (lo, hi))
    total = f + d
    assert total.dtype == np.float32
    return torch.from_numpy((total >= l) & (total <= u))


def tail_elements(fullres, delta_density, lo, hi, gpp, exponent, grads):
    """The float64 `want` and the condition A of everything the tail computes, in plane layout ([(v b), gpp, H, W]; g_fullres
    [(v b), 1, H, W]) — depths, opacities, densities, g_fullres, g_delta (disparity half), g_logit (density half).  lo / hi are the
    float32 bounds [(v b)]; grads are (g_depths, g_opacities, g_densities) in [b, v, H W, 1, gpp], any may be None."""
    n, _, h, w = fullres.shape
    f, dd = fullres.detach().cpu().double(), delta_density.detach().cpu().double()
    l, u = (t.detach().cpu().double().reshape(-1, 1, 1, 1) for t in (lo, hi))
    total = f + dd[:, :gpp]
    fine = torch.minimum(torch.maximum(total, l), u)
    o = opacity_elements(dd[:, gpp:], exponent, gpp)
    zero = torch.zeros(n, gpp, h, w, dtype=torch.float64)
    g_dep, g_opa, g_den = (zero if g is None else planes(g.detach().cpu().double(), h, w) for g in grads)
    inside = clamp_pattern(fullres, delta_density[:, :gpp], lo, hi)
    g_delta = torch.where(inside, -g_dep / (fine * fine), zero)
    t_o, t_s = g_opa * o["slope"], g_den * o["pq"]
    want = dict(depths=1.0 / fine, opacities=o["opacity"], densities=o["p"], g_fullres=g_delta.sum(dim=1, keepdim=True), g_delta=g_delta,
                g_logit=t_o + t_s)
    cond = {k: want[k].abs() for k in ("depths", "opacities", "densities", "g_delta")}
    cond.update(g_fullres=g_delta.abs().sum(dim=1, keepdim=True), g_logit=t_o.abs() + t_s.abs())
    return want, cond


TAIL_QUANTITIES = ("depths", "opacities", "densities", "g_fullres", "g_delta", "g_logit")


def tail_model(fullres, delta_density, lo, hi, gpp, exponent, grads, opacity="stable", slope_q="stable", float64_clamp=False):
    """A float64 model of the tail kernels' formulas (log p = -softplus(-x), log(1 - p) = -softplus(x), expm1), each output rounded
    once to float32; plane layout as tail_elements.  Planted defects: opacity="pow" forms 1 - (1 - p)^e from p = sigmoid(x) in
    float64; slope_q="one_minus_p" takes q = 1 - p; float64_clamp decides the clamp on the float64 sum."""
    n, _, h, w = fullres.shape
    f, dd = fullres.detach().cpu().double(), delta_density.detach().cpu().double()
    l, u = (t.detach().cpu().double().reshape(-1, 1, 1, 1) for t in (lo, hi))
    total = f + dd[:, :gpp]
    fine = torch.minimum(torch.maximum(total, l), u)
    x, e = dd[:, gpp:], float(exponent)
    softplus = lambda t: torch.where(t > 0, t + torch.log1p((-t).exp()), torch.log1p(t.exp()))
    lp, lq = -softplus(-x), -softplus(x)
    p, q = lp.exp(), lq.exp()
    root = (lp / e).exp()
    op = (root - torch.special.expm1(e * lq)) * (0.5 / gpp)
    if opacity == "pow":
        op = (1.0 - (1.0 - torch.sigmoid(x)) ** e + torch.sigmoid(x) ** (1.0 / e)) * (0.5 / gpp)
    if slope_q == "one_minus_p":
        q = 1.0 - p
    slope = (e * (e * lq).exp() * p + root * q / e) * (0.5 / gpp)
    zero = torch.zeros(n, gpp, h, w, dtype=torch.float64)
    g_dep, g_opa, g_den = (zero if g is None else planes(g.detach().cpu().double(), h, w) for g in grads)
    inside = ((total >= l) & (total <= u)) if float64_clamp else clamp_pattern(fullres, delta_density[:, :gpp], lo, hi)
    g_delta = torch.where(inside, -g_dep / (fine * fine), zero)
    return dict(depths=(1.0 / fine).float(), opacities=op.float(), densities=p.float(), g_fullres=g_delta.sum(dim=1, keepdim=True).float(),
                g_delta=g_delta.float(), g_logit=(g_opa * slope + g_den * (p * q)).float())


def opacity_map_elements(pdf, exponent, g=None):
    """map_pdf_to_opacity on probabilities, as the reference states it (with pow, which the kernel deliberately uses too):
    (want, A) of the value, A = 0.5 (1 + (1 - p)^e + p^(1 / e)); with g, of the gradient in p, g 0.5 (e (1 - p)^(e - 1) +
    p^(1 / e - 1) / e), whose two terms have one sign: A = |want| (infinite where the statement is)."""
    p, e = pdf.detach().cpu().double(), float(exponent)
    if g is None:
        a, b = (1.0 - p) ** e, p ** (1.0 / e)
        return 0.5 * (1.0 - a + b), 0.5 * (1.0 + a + b)
    want = g.detach().cpu().double() * (0.5 * (e * (1.0 - p) ** (e - 1.0) + p ** (1.0 / e - 1.0) / e))
    return want, want.abs()


def plant(fullres, delta_density, lo, hi, gpp):
    """Copies of a random case's fullres and delta / logits with the edges planted: the first density logits of every image become
    PLANTED_LOGITS (as many as fit), and the first pixels of every image get fullres + delta exactly on lo, on hi, one float32 ulp
    on either side of each, and lo and hi with a delta of a quarter ulp either way — the float64 sum is off the bound, the float32
    sum is on it.  Image ni starts the list at entry ni, so that an image of one pixel still meets another entry."""
    fullres, dd = fullres.clone(), delta_density.clone()
    n, _, h, w = fullres.shape
    inf = torch.tensor(float("inf"), device=fullres.device)
    f_flat, d_flat, x_flat = fullres.view(n, h * w), dd[:, :gpp].reshape(n, gpp, h * w).clone(), dd[:, gpp:].reshape(n, gpp * h * w).clone()
    values = torch.tensor(PLANTED_LOGITS, device=fullres.device)
    for ni in range(n):
        l, u = lo[ni], hi[ni]
        sums = [(l, 0.0), (u, 0.0), (torch.nextafter(l, -inf), 0.0), (torch.nextafter(l, inf), 0.0), (torch.nextafter(u, -inf), 0.0),
                (torch.nextafter(u, inf), 0.0), (l, l * 2.0 ** -26), (l, -l * 2.0 ** -26), (u, u * 2.0 ** -26), (u, -u * 2.0 ** -26)]
        for i in range(min(len(sums), h * w)):
            base, delta = sums[(i + ni) % len(sums)]
            f_flat[ni, i] = base
            d_flat[ni, :, i] = delta
        k = min(len(values), x_flat.shape[1])
        x_flat[ni, :k] = values.roll(-ni)[:k]
    dd[:, :gpp] = d_flat.view(n, gpp, h, w)
    dd[:, gpp:] = x_flat.view(n, gpp, h, w)
    return fullres, dd


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
