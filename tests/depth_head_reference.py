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


# ------------------------------------------------------------------------------------------------ the per-element measure
# bound = 2^-24 |want| + 2^-40 A + 2^-149: one float32 rounding of the result, 2^13 float64 ulps of the element's condition A (the
# sum of the magnitudes of the terms that make it up: sums of at most 256 terms and library functions of a few ulps) and half the
# smallest float32 subnormal (a tiny `want` underflows).  Derived, not measured.
UNIT, COND, TINY = 2.0 ** -24, 2.0 ** -40, 2.0 ** -149
ELEMENT_SHAPES = {"plain": (2, 16, 8, 32), "odd": (3, 7, 5, 13), "ragged": (2, 130, 3, 21), "ref_d": (1, 128, 32, 64)}
ELEMENT_SCALES = (1.0, 6.0, 30.0, 1e4)
QUANTITIES = ("depth", "pmax", "lse", "g_logits")


def bound(want, cond):
    return UNIT * want.abs() + COND * cond + TINY


def worst(got, want, cond):
    """max |got - want| / bound over every element.  An infinite `want` must be met exactly, sign included; an element with
    want == 0 and condition 0 must be exactly 0; a NaN anywhere gives NaN, which fails `<= 1`."""
    got, want, cond = got.double(), want.double(), cond.double().expand_as(want)
    same = got == want
    err = torch.where(same, torch.zeros_like(want), (got - want).abs())
    b = bound(want, cond)
    ratio = err / torch.where(torch.isfinite(b), b, torch.ones_like(b))
    ratio = torch.where(~same & (torch.isinf(want) | ((want == 0) & (cond == 0))), torch.full_like(ratio, float("inf")), ratio)
    return ratio.max().item() if ratio.numel() else 0.0


def first_maximum(z):
    """(m, a): the maximum over dim 1 and the FIRST depth that attains it, both keepdim."""
    m = z.max(dim=1, keepdim=True)[0]
    idx = torch.arange(z.shape[1], device=z.device).view(1, -1, 1, 1).expand_as(z)
    a = torch.where(z == m, idx, torch.full_like(idx, z.shape[1])).min(dim=1, keepdim=True)[0]
    return m, a


def head_elements(logits, cand, g_depth, g_pmax):
    """The float64 `want` of depth, pmax, lse, argmax and g_logits, and the condition A of each (argmax: exact).  a is the first
    maximum; the gradient is float64 autograd of the statement with pmax = pdf[a].  Returns (want, cond), two dicts."""
    z = logits.detach().double().requires_grad_(True)
    n, D = z.shape[:2]
    c = cand.double().reshape(n, D, 1, 1)
    gd = torch.zeros_like(z[:, :1]) if g_depth is None else g_depth.double()
    gp = torch.zeros_like(z[:, :1]) if g_pmax is None else g_pmax.double()
    with torch.no_grad():
        m, a = first_maximum(z)
        log_s = (z - m).exp().sum(dim=1, keepdim=True).log()
    pdf = torch.softmax(z, dim=1)
    depth = (c * pdf).sum(dim=1, keepdim=True)
    pmax = pdf.gather(1, a)
    (g,) = torch.autograd.grad([depth, pmax], z, [gd, gp])
    with torch.no_grad():
        pdf, depth, pmax = pdf.detach(), depth.detach(), pmax.detach()
        spread = (c.abs() * pdf).sum(dim=1, keepdim=True)
        hot = torch.zeros_like(pdf).scatter_(1, a, gp.abs() * pmax)
        cond = dict(depth=spread, pmax=pmax, lse=m.abs() + log_s,
                    g_logits=pdf * (gd.abs() * (c.abs() + spread) + gp.abs() * pmax) + hot)
        want = dict(depth=depth, pmax=pmax, lse=m + log_s, argmax=a, g_logits=g)
    return want, cond


def kernel_model(logits, cand, g_depth, g_pmax, corrected=True, last_maximum=False):
    """A float64 model of the kernels' formulas, each output rounded once to float32: the forward's depth = t / s, pmax = 1 / s,
    lse = m + log s and the first maximum; the backward from the SAVED float32 lse and depth, with the pass that measures what
    they are off by (q, r).  corrected=False drops that pass (q = 1, r = 0, pmax = e_a); last_maximum=True takes the last
    maximum on a tie.  Returns the dict of depth, pmax, lse, argmax, g_logits."""
    z = logits.double()
    n, D = z.shape[:2]
    c = cand.double().reshape(n, D, 1, 1)
    gd = torch.zeros_like(z[:, :1]) if g_depth is None else g_depth.double()
    gp = torch.zeros_like(z[:, :1]) if g_pmax is None else g_pmax.double()
    m, a = first_maximum(z)
    if last_maximum:
        a = (D - 1) - first_maximum(z.flip(1))[1]
    e = (z - m).exp()
    s = e.sum(dim=1, keepdim=True)
    depth = ((c * e).sum(dim=1, keepdim=True) / s).float()
    pmax = (1.0 / s).float()
    lse = (m + s.log()).float()
    e = (z - lse.double()).exp()
    centred = c - depth.double()
    if corrected:
        q = e.sum(dim=1, keepdim=True)
        r = (centred * e).sum(dim=1, keepdim=True) / q
    else:
        q, r = torch.ones_like(s), torch.zeros_like(s)
    top = gp * (e.gather(1, a) / q)
    g = (e / q) * (gd * (centred - r) - top) + torch.zeros_like(z).scatter_(1, a, top)
    return dict(depth=depth, pmax=pmax, lse=lse, argmax=a, g_logits=g.float())


def float32_statement(logits, cand, g_depth, g_pmax):
    """torch's float32 statement on the inputs' device: depth, pmax, lse (logsumexp) and the autograd gradient."""
    depth, pmax = head(logits, cand, torch.float32)
    return dict(depth=depth, pmax=pmax, lse=torch.logsumexp(logits.float(), dim=1, keepdim=True),
                g_logits=logits_gradient(logits, cand, g_depth, g_pmax, torch.float32))


def pooled_passes(got, want, t32):
    """The pooled rule of tests/test_gpu_depth_head.py on one tensor."""
    e_k, e_t = (got.double() - want).abs(), (t32.double() - want).abs()
    floor = UNIT * want.abs().max().item()
    return bool(torch.isfinite(got).all()) and e_k.max().item() <= max(1.5 * e_t.max().item(), floor) \
        and e_k.mean().item() <= max(1.5 * e_t.mean().item(), floor)


def element_seed(shape, scale, sampling):
    return sum(shape) + int(scale) + len(sampling)


def mixed_case(sampling="inverse_depth", device="cpu"):
    """One tensor whose pixel rows are scaled by 1e-3, 1, 30 and 1e3, with g_depth rows scaled by 1 down to 1e-6.  P = 104."""
    logits, cand, g_depth, g_pmax = random_case((2, 40, 8, 13), 1.0, sampling, seed=77, device=device)
    rows = torch.arange(8, device=device)
    logits = logits * torch.tensor([1e-3, 1.0, 30.0, 1e3], device=device)[rows % 4].view(1, 1, 8, 1)
    g_depth = g_depth * (10.0 ** -(rows % 7).float()).view(1, 1, 8, 1)
    return logits.contiguous(), cand, g_depth.contiguous(), g_pmax


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
