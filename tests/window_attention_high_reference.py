"""The yardstick of the window attention's "high" precision mode (splatter360_amd/window_attention.py, precision="high"): the
function of tests/window_attention_reference.py with each of its six products as a bf16x3 product of split operands, every sum
in float64.  What the kernels and this file share is the specification:

  split(x)   hi = bf16(x), round to nearest even; lo = bf16(x - float32(hi)); the difference is exact in float32
  product    A B = Ah Bh + Ah Bl + Al Bh (terms=3); Al Bl is dropped.  terms=1 keeps Ah Bh alone: a single-bf16 product, the
             arithmetic a kernel that lost its lo planes would compute — tests/test_window_attention_high_spec.py shows that
             the accuracy bound of the GPU test tells the two apart.

Both operands of every product are split from their float32 values: q, k, v, g_out, and P, dS as the float64 softmax and its
backward leave them.
"""
import torch

import window_attention_reference as R


def split(x):
    """(hi, lo) of a float32 tensor, both bfloat16."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def _product(a, b, terms):
    """a [..., n, k] times b [..., k, m], float64 in and out: the operands rounded to float32, split, the terms summed in float64."""
    (ah, al), (bh, bl) = (tuple(t.double() for t in split(x.to(torch.float32))) for x in (a, b))
    out = ah @ bh
    if terms == 3:
        out = out + ah @ bl + al @ bh
    return out


class HighProduct(torch.autograd.Function):
    """a @ b as a high product, and both backward products (g b^T, a^T g) as high products of their own split operands."""

    @staticmethod
    def forward(ctx, a, b, terms):
        assert terms in (1, 3)
        ctx.save_for_backward(a, b)
        ctx.terms = terms
        return _product(a, b, terms)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        return _product(g, b.transpose(-1, -2), ctx.terms), _product(a.transpose(-1, -2), g, ctx.terms), None


def split_statement(q, k, v, num_splits, shift, h, w, rule="reference", terms=3):
    """R.statement with high products: q [B, L, C], k / v [B, L, C] or [B, m, L, C] float32 -> out [B, L, C] float64;
    differentiable (g_q = dS K, g_k = dS^T Q, g_v = P^T G and dP = G V^T are high products too)."""
    assert rule in ("reference", "aligned")
    q, k, v = (t.double() for t in (q, k, v))
    if k.dim() == 3:
        k, v = k.unsqueeze(1), v.unsqueeze(1)
    b, l, c = q.shape
    m = k.shape[1]
    assert l == h * w and h % num_splits == 0 and w % num_splits == 0
    tok, region = R.window_index(h, w, num_splits, shift, q.device)
    nw, lw = tok.shape
    qw = q[:, tok]                                              # [B, K^2, Lw, C]
    kw, vw = (t[:, :, tok].permute(0, 2, 3, 1, 4).reshape(b, nw, lw * m, c) for t in (k, v))      # key j = p m + u
    scores = HighProduct.apply(qw, kw.transpose(-1, -2), terms) / (c ** 0.5)
    if shift:
        j = torch.arange(lw * m, device=q.device)
        key_region = region[:, j % lw] if rule == "reference" else region[:, j // m]
        differ = region.unsqueeze(2) != key_region.unsqueeze(1)
        scores = scores + torch.where(differ, R.MASK_VALUE, 0.0).to(scores.dtype)
    ow = HighProduct.apply(torch.softmax(scores, dim=-1), vw, terms)                              # [B, K^2, Lw, C]
    back = torch.empty(l, dtype=torch.long, device=q.device)
    back[tok.reshape(-1)] = torch.arange(l, device=q.device)
    return ow.reshape(b, l, c)[:, back]


def errors(x, want):
    """(max, mean) absolute error of x against the float64 `want`."""
    e = (x.double() - want).abs()
    return e.max().item(), e.mean().item()


def bound(w64, t3, l32):
    """The accuracy rule's (max, mean) bounds for one tensor: max(1.5 x (e3 + e32), 2^-24 max|want|), e3 the error of the terms=3
    statement `t3` and e32 that of the float32 lines `l32` against the float64 `w64`."""
    (smax, smean), (lmax, lmean) = errors(t3, w64), errors(l32, w64)
    floor = 2.0 ** -24 * w64.abs().max().item()
    return max(1.5 * (smax + lmax), floor), max(1.5 * (smean + lmean), floor)


def check_rule(tag, names, want, three, lines, got):
    """The accuracy rule of the four "high" modes, for the tensors `names` of one case: each of `got` is float32, has the shape
    of its float64 `want`, is finite, and its max and mean absolute error against `want` are within `bound` of `three` (the
    terms=3 statement) and `lines` (the float32 lines).  One line of figures per tensor is printed; the failures are collected
    and asserted once."""
    ratio = lambda a, b: a / b if b else 0.0
    failures = []
    for n, w64, t3, l32, x in zip(names, want, three, lines, got):
        assert x.dtype == torch.float32 and x.shape == w64.shape, (tag, n)
        assert torch.isfinite(x).all(), (tag, n)
        (kmax, kmean), (e3max, e3mean), (lmax, lmean) = errors(x, w64), errors(t3, w64), errors(l32, w64)
        floor = 2.0 ** -24 * w64.abs().max().item()
        bmax, bmean = bound(w64, t3, l32)
        print(f"{tag} {n}: kernel max {kmax:.3e} mean {kmean:.3e} | e3 max {e3max:.3e} mean {e3mean:.3e} | e32 max {lmax:.3e} mean "
              f"{lmean:.3e} | floor {floor:.3e} | kernel / bound {ratio(kmax, bmax):.3f} {ratio(kmean, bmean):.3f}"
              f" | kernel / e3 {ratio(kmax, e3max):.2f} {ratio(kmean, e3mean):.2f}")
        if not (kmax <= bmax and kmean <= bmean):
            failures.append((n, kmax, kmean, bmax, bmean))
    assert not failures, (tag, failures)
