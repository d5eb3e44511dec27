"""The multi-view transformer's single-head (shifted-)window attention stated in plain torch, for any dtype and device: what
splatter360_amd/window_attention.py is tested against.  The project's own lines, two statements of one function (the reference's
single_head_split_window_attention, src/model/encoder/backbone/multiview_transformer.py:60-210):

  statement        index level: every window's tokens and regions as index tensors, one gather, one softmax, one scatter
  reference_lines  the reference's order of operations (roll, split, matmul, dense mask, softmax, matmul, merge, roll back):
                   the float32 yardstick of the GPU tests and the body of the stand-in module

and the per-row measure of tests/test_gpu_window_attention_float64.py: `row_scales` (the exact per-row quantities in float64 and
the scale each is summed from), `lines_rows` (the float32 lines' six quantities) and `row_units` (a result's error per row in
units of 2^-24 of its scale).
"""
import types

import torch

MASK_VALUE = -100.0                                             # finite: a masked key keeps weight exp(-100 + ...)


def _axis_region(i, n, win, s):
    return (i >= n - win).long() + (i >= n - s).long()


def window_index(h, w, num_splits, shift, device="cpu"):
    """(tok, region), both [K^2, Lw] int64: the ORIGINAL token of window token p of every window, and the region of its rolled
    position."""
    k = num_splits
    wh, ww = h // k, w // k
    sh, sw = (wh // 2, ww // 2) if shift else (0, 0)
    ry = torch.arange(h, device=device).view(k, 1, wh, 1).expand(k, k, wh, ww)
    rx = torch.arange(w, device=device).view(1, k, 1, ww).expand(k, k, wh, ww)
    tok = ((ry + sh) % h) * w + (rx + sw) % w
    region = 3 * _axis_region(ry, h, wh, sh) + _axis_region(rx, w, ww, sw)
    return tok.reshape(k * k, wh * ww), region.reshape(k * k, wh * ww)


def dense_mask(h, w, num_splits, device="cpu"):
    """The reference's generate_shift_window_attn_mask(...) for shift = window // 2: [K^2, Lw, Lw] float32, 0 / -100."""
    _, region = window_index(h, w, num_splits, True, device)
    differ = region.unsqueeze(1) != region.unsqueeze(2)
    return torch.where(differ, torch.tensor(MASK_VALUE, device=device), torch.tensor(0.0, device=device))


def statement(q, k, v, num_splits, shift, h, w, rule="reference", dtype=torch.float64, mask_value=MASK_VALUE):
    """q [B, L, C], k / v [B, L, C] or [B, m, L, C] -> out [B, L, C] in `dtype`; differentiable.  mask_value: what a test that
    shows the mask to be FINITE compares against (float("-inf") is the other convention)."""
    assert rule in ("reference", "aligned")
    q, k, v = (t.to(dtype) for t in (q, k, v))
    if k.dim() == 3:
        k, v = k.unsqueeze(1), v.unsqueeze(1)
    b, l, c = q.shape
    m = k.shape[1]
    assert l == h * w and h % num_splits == 0 and w % num_splits == 0
    tok, region = window_index(h, w, num_splits, shift, q.device)
    nw, lw = tok.shape
    qw = q[:, tok]                                              # [B, K^2, Lw, C]
    kw, vw = (t[:, :, tok].permute(0, 2, 3, 1, 4).reshape(b, nw, lw * m, c) for t in (k, v))      # key j = p m + u
    scores = qw @ kw.transpose(-1, -2) / (c ** 0.5)
    if shift:
        j = torch.arange(lw * m, device=q.device)
        key_region = region[:, j % lw] if rule == "reference" else region[:, j // m]
        differ = region.unsqueeze(2) != key_region.unsqueeze(1)
        scores = scores + torch.where(differ, mask_value, 0.0).to(dtype)
    ow = torch.softmax(scores, dim=-1) @ vw                     # [B, K^2, Lw, C]
    back = torch.empty(l, dtype=torch.long, device=q.device)
    back[tok.reshape(-1)] = torch.arange(l, device=q.device)
    return ow.reshape(b, l, c)[:, back]


def _split(x, n):
    """[B, H, W, C] -> [B n n, H / n, W / n, C], windows in (row, column) order."""
    b, h, w, c = x.shape
    return x.reshape(b, n, h // n, n, w // n, c).transpose(2, 3).reshape(b * n * n, h // n, w // n, c)


def _merge(x, n):
    bn, wh, ww, c = x.shape
    return x.reshape(bn // (n * n), n, n, wh, ww, c).transpose(2, 3).reshape(bn // (n * n), n * wh, n * ww, c)


def reference_lines(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None, rule="reference", parts=None):
    """The reference's order of operations in the inputs' dtype, with its signature: roll by minus half a window, split, one dense
    [B K^2, Lw, Lk] score tensor, the dense mask (tiled m times along the keys, as the reference tiles it; rule="aligned"
    repeats each column m times instead), softmax, the second product, merge, roll back.  A dict given as `parts` receives
    the intermediates, detached: "scores" (masked) and "probabilities" [B K^2, Lw, Lk], "values" [B K^2, Lk, C], and
    "to_windows", which takes a [B, L, C] tensor the way q goes (roll, split)."""
    b, l, c = q.shape
    n = num_splits
    assert l == h * w
    if k.dim() == 3:
        k, v = k.unsqueeze(1), v.unsqueeze(1)
    m = k.shape[1]
    q = q.reshape(b, h, w, c)
    k, v = (t.reshape(b, m, h, w, c).permute(0, 2, 3, 1, 4).reshape(b, h, w, m * c) for t in (k, v))
    if with_shift:
        assert attn_mask is not None
        sh, sw = (h // n) // 2, (w // n) // 2
        q, k, v = (torch.roll(t, shifts=(-sh, -sw), dims=(1, 2)) for t in (q, k, v))
    q = _split(q, n).reshape(b * n * n, -1, c)
    k, v = (_split(t, n).reshape(b * n * n, -1, c) for t in (k, v))             # [B K^2, Lw m, C]: key j = p m + u
    scores = torch.matmul(q, k.transpose(1, 2)) / (c ** 0.5)
    if with_shift:
        mask = attn_mask.repeat(b, 1, m) if rule == "reference" else attn_mask.repeat_interleave(m, dim=2).repeat(b, 1, 1)
        scores = scores + mask.to(scores.dtype)
    prob = torch.softmax(scores, dim=-1)
    if parts is not None:
        def to_windows(x):
            x = x.reshape(b, h, w, -1)
            x = torch.roll(x, shifts=(-sh, -sw), dims=(1, 2)) if with_shift else x
            return _split(x, n).reshape(b * n * n, -1, x.shape[-1])
        parts.update(scores=scores.detach(), probabilities=prob.detach(), values=v.detach(), to_windows=to_windows)
    out = torch.matmul(prob, v)
    out = _merge(out.reshape(b * n * n, h // n, w // n, c), n)
    if with_shift:
        out = torch.roll(out, shifts=(sh, sw), dims=(1, 2))
    return out.reshape(b, l, c)


def full_lines(q, k, v):
    """single_head_full_attention (:8-16) in the inputs' dtype."""
    scores = torch.matmul(q, k.transpose(1, 2)) / (q.shape[2] ** 0.5)
    return torch.matmul(torch.softmax(scores, dim=2), v)


def random_case(b, m, h, w, c=128, scale=1.0, seed=0, device="cpu"):
    """(q, k, v, g_out) float32: q, k randn * scale, v and g_out randn; k, v [B, L, C] for m = 0, else [B, m, L, C]."""
    gen = torch.Generator().manual_seed(seed)
    l = h * w
    kshape = (b, l, c) if m == 0 else (b, m, l, c)
    q = torch.randn(b, l, c, generator=gen) * scale
    k = torch.randn(*kshape, generator=gen) * scale
    v = torch.randn(*kshape, generator=gen)
    g = torch.randn(b, l, c, generator=gen)
    return tuple(t.to(device) for t in (q, k, v, g))


def gradients(fn, q, k, v, g_out, dtype=None):
    """(out, g_q, g_k, g_v) of fn(q, k, v) by autograd, inputs cast to `dtype` first (None: as they are)."""
    q, k, v = (t.detach().to(dtype or t.dtype).requires_grad_(True) for t in (q, k, v))
    out = fn(q, k, v)
    return (out.detach(), *torch.autograd.grad(out, (q, k, v), g_out.to(out.dtype)))


# ------------------------------------------------------------------------------------------------ the per-row measure
ROW_NAMES = ("out", "g_q", "g_k", "g_v", "lse", "delta")
UNIT = 2.0 ** -24
SCALE_FLOOR = 2.0 ** -100                                       # keeps a key that nobody attends to in the measure

# name: (B, m, h, w, K, C): the smallest shapes that reach each path of the kernels' block decomposition and channel maps
ROW_CASES = {
    "c64": (1, 2, 6, 10, 2, 64),          # NCB = 2; Lw = 15, Lk = 30 < one tile; odd window 3 x 5
    "c96": (1, 0, 10, 14, 2, 96),         # NCB = 3; Lw = 35
    "edge": (1, 0, 20, 26, 2, 32),        # Lw = 130: a second owner workgroup with 2 valid rows
    "m5": (3, 5, 12, 10, 2, 32),          # Lw = 30, Lk = 150: two owner blocks in the key-owned pass only; B = 3 with partners
    "m11": (1, 11, 4, 6, 2, 64),          # the cube's partner count; Lw = 6, Lk = 66; both mask rules
    "k3": (1, 1, 9, 15, 3, 64),           # K = 3, sh = 1, sw = 2
    "thin": (2, 0, 2, 16, 2, 32),         # wh = 1: with shift sh = 0
    "tiny": (2, 2, 4, 6, 2, 32),          # Lw = 6, Lk = 12: three of four waves own nothing
}


def row_scales(q, k, v, g_out, num_splits, shift, h, w, rule="reference", mask_value=MASK_VALUE):
    """(want, scale): two dicts over ROW_NAMES, float64 on the inputs' device, in the ORIGINAL row order.  want: out, g_q
    [B, L, C], g_k, g_v in k's shape, lse and delta (Delta_i = sum_j P_ij dP_ij) [B, L].  scale: one number per row ([B, L]; k's
    shape without C for g_k, g_v), the sum of the magnitudes the row's quantity is summed from, each weighted by what a
    rounding of the score in front of exp does to it.  Per window, with s the scores, P the probabilities, dP = g V^T:

        a_ij = sum_c |q_ic k_jc| / sqrt(C)    b_ij = sum_c |g_ic v_jc|    A_i = sum_j P_ij a_ij    B_i = sum_j P_ij b_ij
        pw_ij = P_ij (1 + a_ij + A_i)         e_ij = pw_ij (|dP_ij| + |Delta_i|) + P_ij (b_ij + B_i)

        out_i : max_c sum_j pw_ij |v_jc|           g_v_j : max_c sum_i pw_ij |g_ic|
        g_q_i : max_c sum_j e_ij |k_jc| / sqrt(C)  g_k_j : max_c sum_i e_ij |q_ic| / sqrt(C)
        lse_i : 1 + A_i + |lse_i|                  Delta_i : sum_j e_ij

    A score rounded by eps a_ij moves P_ij by eps P_ij (a_ij + A_i): the (1 + a + A) factor; e is the same for dS = P (dP -
    Delta)."""
    assert rule in ("reference", "aligned")
    three = k.dim() == 3
    q, k, v, g = (t.detach().double() for t in (q, k, v, g_out))
    if three:
        k, v = k.unsqueeze(1), v.unsqueeze(1)
    b, l, c = q.shape
    m = k.shape[1]
    tok, region = window_index(h, w, num_splits, shift, q.device)
    nw, lw = tok.shape
    qw, gw = q[:, tok], g[:, tok]                               # [B, K^2, Lw, C]
    kw, vw = (t[:, :, tok].permute(0, 2, 3, 1, 4).reshape(b, nw, lw * m, c) for t in (k, v))      # key j = p m + u
    root = c ** 0.5
    s = qw @ kw.transpose(-1, -2) / root
    if shift:
        j = torch.arange(lw * m, device=q.device)
        key_region = region[:, j % lw] if rule == "reference" else region[:, j // m]
        s = s + torch.where(region.unsqueeze(2) != key_region.unsqueeze(1), mask_value, 0.0).to(s.dtype)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    dp = gw @ vw.transpose(-1, -2)
    delta = (p * dp).sum(-1)
    ds = p * (dp - delta.unsqueeze(-1))
    a = qw.abs() @ kw.abs().transpose(-1, -2) / root
    bb = gw.abs() @ vw.abs().transpose(-1, -2)
    big_a, big_b = (p * a).sum(-1), (p * bb).sum(-1)
    pw = p * (1.0 + a + big_a.unsqueeze(-1))
    e = pw * (dp.abs() + delta.abs().unsqueeze(-1)) + p * (bb + big_b.unsqueeze(-1))
    back = torch.empty(l, dtype=torch.long, device=q.device)
    back[tok.reshape(-1)] = torch.arange(l, device=q.device)

    def query_rows(x):                                          # [B, K^2, Lw, ...] -> [B, L, ...]
        return x.reshape(b, l, *x.shape[3:])[:, back]

    def key_rows(x):                                            # [B, K^2, Lw m, ...] -> k's shape
        x = x.reshape(b, nw, lw, m, *x.shape[3:]).movedim(3, 1).reshape(b, m, l, *x.shape[3:])[:, :, back]
        return x[:, 0] if three else x

    pt, dst, pwt, et = (t.transpose(-1, -2) for t in (p, ds, pw, e))
    want = dict(out=query_rows(p @ vw), g_q=query_rows(ds @ kw / root), g_k=key_rows(dst @ qw / root), g_v=key_rows(pt @ gw),
                lse=query_rows(lse), delta=query_rows(delta))
    scale = dict(out=query_rows((pw @ vw.abs()).amax(-1)), g_q=query_rows((e @ kw.abs()).amax(-1) / root),
                 g_k=key_rows((et @ qw.abs()).amax(-1) / root), g_v=key_rows((pwt @ gw.abs()).amax(-1)),
                 lse=query_rows(1.0 + big_a + lse.abs()), delta=query_rows(e.sum(-1)))
    return want, scale


def lines_rows(q, k, v, g_out, num_splits, shift, h, w, rule="reference"):
    """The float32 yardstick of all six quantities, a dict over ROW_NAMES in the inputs' dtype: out and the gradients of
    reference_lines by autograd, lse = torch.logsumexp of its scores and delta = (P * dP).sum(-1) of its probabilities, with
    dP = g V^T formed from the same tensors."""
    mask = dense_mask(h, w, num_splits, q.device) if shift else None
    parts = {}
    got = gradients(lambda a, b, c: reference_lines(a, b, c, num_splits, shift, h, w, mask, rule=rule, parts=parts), q, k, v, g_out)
    scores, prob, vw = parts["scores"], parts["probabilities"], parts["values"]
    dp = torch.matmul(parts["to_windows"](g_out.to(prob.dtype)), vw.transpose(1, 2))
    wh, ww = h // num_splits, w // num_splits

    def rows(x):                                                # [B K^2, Lw] -> [B, L], as the output goes (merge, roll back)
        x = _merge(x.reshape(-1, wh, ww, 1), num_splits)
        x = torch.roll(x, shifts=(wh // 2, ww // 2), dims=(1, 2)) if shift else x
        return x.reshape(q.shape[0], h * w)

    return dict(zip(ROW_NAMES, (*got, rows(torch.logsumexp(scores, dim=-1)), rows((prob * dp).sum(-1)))))


def row_units(x, want, scale):
    """The error of `x` per row in units of 2^-24 of the row's scale: max_c |x - want| / max(scale, 2^-100) (lse and delta have
    no channel axis).  No row is left out: a row of scale 0 that is not exactly 0 in `x` measures 2^76 units or more."""
    err = (x.double() - want).abs()
    if err.dim() > scale.dim():
        err = err.amax(-1)
    assert err.shape == scale.shape, (err.shape, scale.shape)
    return err / scale.clamp_min(SCALE_FLOOR) / UNIT


def worst_rows(got, want, scale):
    """{name: the worst row's units} of a dict of results over ROW_NAMES (any subset)."""
    return {n: row_units(got[n], want[n], scale[n]).max().item() for n in ROW_NAMES if n in got and got[n] is not None}


def standin_module(name):
    """A stand-in for the reference's backbone module: the three names install(window_attention=True) rebinds, a multi-head
    function that takes the mask, and a layer function that looks the names up as module globals at call time, as
    TransformerLayer.forward does."""
    mod = types.ModuleType(name)
    mod.calls = []

    def single_head_full_attention(q, k, v):
        mod.calls.append(("full", None))
        return full_lines(q, k, v)

    def generate_shift_window_attn_mask(input_resolution, window_size_h, window_size_w, shift_size_h, shift_size_w,
                                        device=torch.device("cpu")):
        h, w = input_resolution
        assert (shift_size_h, shift_size_w) == (window_size_h // 2, window_size_w // 2)
        return dense_mask(h, w, w // window_size_w, device)

    def single_head_split_window_attention(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None):
        mod.calls.append(("single", attn_mask))
        return reference_lines(q, k, v, num_splits, with_shift, h, w, attn_mask)

    def multi_head_split_window_attention(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None, num_head=1):
        mod.calls.append(("multi", attn_mask))
        assert num_head == 1
        return reference_lines(q, k, v, num_splits, with_shift, h, w, attn_mask)

    def layer(q, k, v, h, w, num_splits, with_shift, multi_head=False):
        g = mod.__dict__
        if num_splits == 1:
            return g["single_head_full_attention"](q, k, v)
        mask = g["generate_shift_window_attn_mask"]((h, w), h // num_splits, w // num_splits, h // num_splits // 2,
                                                    w // num_splits // 2, device=q.device)
        fn = g["multi_head_split_window_attention" if multi_head else "single_head_split_window_attention"]
        return fn(q, k, v, num_splits=num_splits, with_shift=with_shift, h=h, w=w, attn_mask=mask)

    for f in (single_head_full_attention, generate_shift_window_attn_mask, single_head_split_window_attention,
              multi_head_split_window_attention, layer):
        setattr(mod, f.__name__, f)
    return mod
