"""The yardstick of the fused transformer FFN tail (splatter360_amd.transformer_ffn): the project's own statement of what the
reference's TransformerLayer.forward (src/model/encoder/backbone/multiview_transformer.py:334-414) computes behind its attention,

    X = cat([source, LN1(m)], -1);  h = gelu(X W1^T);  z = h W2^T;  out = source + LN2(z)        (no_ffn: out = source + LN1(m))
    LN(x) = (x - mean) / sqrt(var + eps) weight + bias over the last axis, var the BIASED variance; gelu the erf form

generic in C, in any dtype (`statement`, `norm_statement`; float64 is what the kernels are held to), the whole layer with full
attention (`layer_statement`), the same lines in float32 as stock torch runs them (`reference_lines`, `norm_lines`: the yardstick
of the accuracy rule), deterministic inputs, gradients, and a stand-in for the reference's backbone module with a TransformerLayer
written for this project that the installed seam rebinds.  The statement is held to the reference's recorded outputs
(tests/golden/transformer_ffn.npz) by tests/test_transformer_ffn_spec.py.  Further the per-row measure of
tests/test_gpu_transformer_ffn_float64.py: `row_statement` (the float64 results per token, hidden unit and channel, and each row's
scale), `lines_rows` (the float32 lines in the same indexing), the rule (`rule_failures`) and the cases.  Nothing here needs a GPU.
"""
import math
import sys

import torch
import torch.nn.functional as F
from torch import nn

import window_attention_reference as W

TAIL_NAMES = ("source", "m", "norm1_weight", "norm1_bias", "w1", "w2", "norm2_weight", "norm2_bias")
NORM_NAMES = ("x", "weight", "bias", "residual")
LAYER_PARAMS = ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "norm1.weight", "norm1.bias", "mlp.0.weight",
                "mlp.2.weight", "norm2.weight", "norm2.bias")


def layer_norm(x, weight, bias, eps, unbiased=False):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).sum(dim=-1, keepdim=True) / (x.shape[-1] - (1 if unbiased else 0))
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def statement(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps=1e-5, dtype=torch.float64, wrong=None,
              parts=None):
    """The tail in `dtype`, pure torch, differentiable, generic in C.  wrong: one of the rules the spec test shows to matter —
    "cat_order", "tanh_gelu", "unbiased_variance", "residual_before_norm2".  parts: a dict that receives "y" = LN1(m) and "z",
    the second Linear's output, as they stand in the graph."""
    source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias = (
        t.to(dtype) for t in (source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias))
    unbiased = wrong == "unbiased_variance"
    y = layer_norm(m, norm1_weight, norm1_bias, eps, unbiased)
    x = torch.cat([y, source] if wrong == "cat_order" else [source, y], dim=-1)
    z = gelu(x @ w1.transpose(0, 1), tanh=wrong == "tanh_gelu") @ w2.transpose(0, 1)
    if parts is not None:
        parts["y"], parts["z"] = y, z
    if wrong == "residual_before_norm2":
        return layer_norm(source + z, norm2_weight, norm2_bias, eps, unbiased)
    return source + layer_norm(z, norm2_weight, norm2_bias, eps, unbiased)


def norm_statement(x, weight, bias, residual, eps=1e-5, dtype=torch.float64):
    x, weight, bias, residual = (t.to(dtype) for t in (x, weight, bias, residual))
    return residual + layer_norm(x, weight, bias, eps)


def reference_lines(source, m, norm1_weight, norm1_bias, w1, w2, norm2_weight, norm2_bias, eps=1e-5, parts=None):
    """The reference's lines in float32 on the tensors' device: F.layer_norm, the concatenation, two F.linear around F.gelu,
    F.layer_norm, the add.  Forms the [T, 2C] and both [T, 8C] tensors.  parts: a dict that receives "z", the second Linear's
    output."""
    c = source.shape[-1]
    message = F.layer_norm(m, (c,), norm1_weight, norm1_bias, eps)
    message = F.linear(F.gelu(F.linear(torch.cat([source, message], dim=-1), w1)), w2)
    if parts is not None:
        parts["z"] = message
    return source + F.layer_norm(message, (c,), norm2_weight, norm2_bias, eps)


def norm_lines(x, weight, bias, residual, eps=1e-5):
    return residual + F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


def gradients(fn, tensors, g, dtype=None):
    """(out, gradient of every tensor) of fn(*tensors) with the output gradient g, all detached; in `dtype` if given."""
    xs = [t.detach().clone().to(dtype or t.dtype).requires_grad_(True) for t in tensors]
    out = fn(*xs)
    out.backward(g.to(out.dtype))
    return (out.detach(), *(x.grad for x in xs))


def random_case(tokens, scale=1.0, seed=0, device="cpu", c=128, lead=None):
    """(the eight tensors of TAIL_NAMES, g), float32, deterministic: source and m standard normal times `scale` (m with an offset
    of its own per token, so that norm1 has a mean to take out), the Linear weights normal with nn.Linear's 1 / sqrt(fan-in)
    deviation, norm weights around 1, g standard normal.  lead: the leading dimensions (their product is `tokens`)."""
    gen = torch.Generator().manual_seed(seed)
    shape = (*(lead or (tokens,)), c)
    assert math.prod(shape[:-1]) == tokens
    source = torch.randn(shape, generator=gen) * scale
    m = (torch.randn(shape, generator=gen) + 0.5 * torch.randn(*shape[:-1], 1, generator=gen)) * scale
    n1w, n2w = (1 + 0.2 * torch.randn(c, generator=gen) for _ in range(2))
    n1b, n2b = (0.2 * torch.randn(c, generator=gen) for _ in range(2))
    w1 = torch.randn(8 * c, 2 * c, generator=gen) / math.sqrt(2 * c)
    w2 = torch.randn(c, 8 * c, generator=gen) / math.sqrt(8 * c)
    g = torch.randn(shape, generator=gen)
    return tuple(t.to(device) for t in (source, m, n1w, n1b, w1, w2, n2w, n2b)), g.to(device)


def norm_case(case):
    """The no_ffn tail's tensors (NORM_NAMES) from a case of random_case: x = m, residual = source."""
    (source, m, n1w, n1b, *_), g = case
    return (m, n1w, n1b, source), g


def layer_statement(params, source, target, no_ffn=False, eps=1e-5, dtype=torch.float64):
    """The whole single-head TransformerLayer with full attention in `dtype` from a {state_dict key: tensor} dict of its
    parameters: projections, softmax(q k^T / sqrt(C)) v, merge, then the tail."""
    p = {k: v.to(dtype) for k, v in params.items()}
    source, target = source.to(dtype), target.to(dtype)
    q, k, v = source @ p["q_proj.weight"].T, target @ p["k_proj.weight"].T, target @ p["v_proj.weight"].T
    m = W.full_lines(q, k, v) @ p["merge.weight"].T
    if no_ffn:
        return norm_statement(m, p["norm1.weight"], p["norm1.bias"], source, eps, dtype)
    return statement(source, m, p["norm1.weight"], p["norm1.bias"], p["mlp.0.weight"], p["mlp.2.weight"], p["norm2.weight"],
                     p["norm2.bias"], eps, dtype)


def layer_params(no_ffn):
    return tuple(k for k in LAYER_PARAMS if not (no_ffn and (k.startswith("mlp") or k.startswith("norm2"))))


# ---- the per-row measure (tests/test_transformer_ffn_rows.py, tests/test_gpu_transformer_ffn_float64.py) ------------------------
# Every quantity is indexed by what owns it in the kernels, one number per row, in units of 2^-24 of the ROW'S OWN magnitude
# (row_units: the window attention's definition).  Token rows [T, C]: out, z, g_source, g_m (no_ffn: out, g_x), scale max_c |want|.
# Hidden-unit rows [8C, .]: g_w1's row j and g_w2's COLUMN j (g_w2 is held transposed, [8C, C], in this indexing), scale
# max |want| over the row.  Channels [C]: the LayerNorm parameter gradients, each a sum over tokens; scale the sum over tokens
# of the summed terms' magnitudes.  (A scale propagated through the chain as a sum of magnitudes, the attentions' kind, overstates
# the float32 lines' error here by three orders of magnitude: DESIGN.md.)
TOKEN_ROWS = ("out", "z", "g_source", "g_m")
UNIT_ROWS = ("g_w1", "g_w2")
CHANNEL_ROWS = ("g_norm1_weight", "g_norm1_bias", "g_norm2_weight", "g_norm2_bias")
FFN_ROW_NAMES = TOKEN_ROWS + UNIT_ROWS + CHANNEL_ROWS
NORM_TOKEN_ROWS = ("out", "g_x")
NORM_CHANNEL_ROWS = ("g_weight", "g_bias")
NORM_ROW_NAMES = NORM_TOKEN_ROWS + NORM_CHANNEL_ROWS + ("g_residual",)
UNIT, SCALE_FLOOR = W.UNIT, W.SCALE_FLOOR
row_units = W.row_units

# name: T.  Each is the smallest T that reaches its path of the launch geometry (tests/test_transformer_ffn_rows.py asserts the
# structure from the kernel file's constants); `one`, `tiny` and `ragged` are the pooled file's small shapes.
ROW_CASES = {
    "one": 1,
    "tiny": 5,
    "ragged": 33,
    "wg2": 129,        # a second workgroup of the forward and the token pass: one valid token in wave 0, three empty waves
    "wg3": 289,        # three workgroups; the last has one full wave and a one-token wave
    "tiles2": 545,     # 18 tiles: 9 weight chunks of 64 tokens, two tiles a chunk; the last chunk is a full tile and a one-token tile
    "tiles3": 1063,    # 34 tiles: 12 chunks of 96 tokens, three tiles a chunk; the last chunk is 7 tokens
    "rows": 2059,      # the row backward past 256 x 8 rows: workgroup 0 a second round of 8, workgroup 1 a second round of 3
    "mixed": 161,      # rows of g times 1, 1e-1, 1e-2, 1e-3 cyclically
    "stride": 65669,   # 514 token tiles on 512 workgroups: workgroups 0 and 1 walk two tiles, the last one of 5 tokens
}
MIXED_GAINS = (1.0, 1e-1, 1e-2, 1e-3)
SMALL_CASES = ("one", "tiny", "ragged")                        # token rows only (UNITS_FROM)
UNITS_FROM = 129                                                # hidden-unit rows and channels are judged from this T on: below,
#                                                                 a hidden unit can have gelu ~ 0 on every token, and the float32
#                                                                 lines miss its g_w2 row by 1e4 units of its own magnitude
ROW_SCALES = (1.0, 6.0)
ROW_RUNS = [(name, scale) for name in ROW_CASES if name != "stride" for scale in ROW_SCALES] + [("stride", 1.0)]
NORM_RUNS = [(name, scale) for name in ("wg2", "rows", "mixed") for scale in ROW_SCALES]
ROW_SEEDS = {}                                                  # name: a seed other than the default (the yardstick's condition)


def row_inputs(name, scale=1.0, device="cpu"):
    """(the eight tensors, g) of a run of ROW_RUNS, [T, C]: the one set of inputs the CPU and the GPU tests of the per-row rule
    share.  NORM_RUNS take norm_case of it."""
    seed = ROW_SEEDS.get(name, 5000 + 7 * sorted(ROW_CASES).index(name))
    tensors, g = random_case(ROW_CASES[name], scale=scale, seed=seed, device=device)
    if name == "mixed":
        g = g * torch.tensor(MIXED_GAINS, device=g.device).repeat(-(-g.shape[0] // 4))[:g.shape[0], None]
    return tensors, g


def row_names(tokens):
    """The quantities of the FFN tail that are judged at `tokens` tokens."""
    return FFN_ROW_NAMES if tokens >= UNITS_FROM else TOKEN_ROWS


def as_rows(named):
    """A {name: tensor} dict of the FFN tail's results in the tensors' own layouts -> the per-row indexing: token tensors
    [T, C], g_w2 transposed to [8C, C].  Views, no copies."""
    return {n: (x.t() if n == "g_w2" else x.reshape(-1, x.shape[-1]) if n in TOKEN_ROWS else x) for n, x in named.items()}


def _x_hat(x, eps):
    mean = x.mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)


def row_statement(tensors, g, eps=1e-5):
    """(want, scale): two dicts over FFN_ROW_NAMES, float64 on the inputs' device, in the per-row indexing.  want: `statement`
    by autograd, z (the second Linear's output) taken from inside it.  scale: one number per row."""
    parts = {}
    xs = [t.detach().double().requires_grad_(True) for t in tensors]
    out = statement(*xs, eps=eps, parts=parts)
    parts["y"].retain_grad()
    out.backward(g.double())
    g64, z, d_y = g.double().reshape(-1, g.shape[-1]), parts["z"].detach(), parts["y"].grad
    want = as_rows(dict(zip(FFN_ROW_NAMES, (out.detach(), z, xs[0].grad, xs[1].grad, xs[4].grad, xs[5].grad, xs[2].grad, xs[3].grad,
                                            xs[6].grad, xs[7].grad))))
    scale = {n: want[n].abs().amax(-1) for n in TOKEN_ROWS + UNIT_ROWS}
    d_y = d_y.reshape(g64.shape)
    scale["g_norm1_weight"] = (d_y * _x_hat(xs[1].detach().reshape(g64.shape), eps)).abs().sum(0)
    scale["g_norm1_bias"] = d_y.abs().sum(0)
    scale["g_norm2_weight"] = (g64 * _x_hat(z.reshape(g64.shape), eps)).abs().sum(0)
    scale["g_norm2_bias"] = g64.abs().sum(0)
    return want, scale


def row_results(tensors, g, eps=1e-5):
    """The float64 results of `statement` by autograd over FFN_ROW_NAMES, z included, in the per-row indexing."""
    return row_statement(tensors, g, eps)[0]


def row_scales(tensors, g, eps=1e-5):
    """The scale of every row of row_results: a dict over FFN_ROW_NAMES."""
    return row_statement(tensors, g, eps)[1]


def lines_rows(tensors, g, eps=1e-5):
    """The float32 yardstick in the same indexing: reference_lines and its gradients by autograd, z taken from inside."""
    parts = {}
    out, *grads = gradients(lambda *t: reference_lines(*t, eps=eps, parts=parts), tensors, g)
    named = dict(zip(("out", *("g_" + n for n in TAIL_NAMES)), (out, *grads)))
    named["z"] = parts["z"].detach()
    return as_rows({n: named[n] for n in FFN_ROW_NAMES})


def norm_row_statement(tensors, g, eps=1e-5):
    """(want, scale) of the no_ffn tail over NORM_ROW_NAMES: norm_statement by autograd.  g_residual is g_out itself: it has no
    scale, it is compared bit for bit."""
    out, g_x, g_weight, g_bias, g_residual = gradients(lambda *t: norm_statement(*t, eps=eps), tensors, g, torch.float64)
    g64 = g.double().reshape(-1, g.shape[-1])
    flat = lambda x: x.reshape(g64.shape)                                           # noqa: E731
    want = dict(zip(NORM_ROW_NAMES, (flat(out), flat(g_x), g_weight, g_bias, flat(g_residual))))
    scale = {n: want[n].abs().amax(-1) for n in NORM_TOKEN_ROWS}
    scale["g_weight"] = (g64 * _x_hat(flat(tensors[0].detach().double()), eps)).abs().sum(0)
    scale["g_bias"] = g64.abs().sum(0)
    return want, scale


def norm_lines_rows(tensors, g, eps=1e-5):
    out, g_x, g_weight, g_bias, g_residual = gradients(lambda *t: norm_lines(*t, eps=eps), tensors, g)
    flat = lambda x: x.reshape(-1, x.shape[-1])                                     # noqa: E731
    return dict(zip(NORM_ROW_NAMES, (flat(out), flat(g_x), g_weight, g_bias, flat(g_residual))))


# The rule, per run and quantity, all rows counted (units of 2^-24 of the row's scale):
#   worst row:  kernel <= max(2 x yardstick's worst row, 0.5)       2: the project's per-row factor; 0.5: one correct rounding
#   mean row:   kernel <= max(1.5 x yardstick's mean row, 0.5)      1.5: the pooled file's factor
#   token and hidden-unit rows: the yardstick's worst row <= 5 x its own median row, else "yardstick not usable" (a failure):
#     one bad yardstick row must not set every row's bound.  The channel gradients (128 values with a long tail, worst / median
#     4 to 6 with torch's float32 lines on the CPU) have no such condition; the mean rule carries that job.
#   a row of scale 0 is exactly 0.
WORST_FACTOR, MEAN_FACTOR, UNITS_FLOOR, MEDIAN_CAP = 2.0, 1.5, 0.5, 5.0
NO_MEDIAN = CHANNEL_ROWS + NORM_CHANNEL_ROWS


def row_figures(x, lines, want, scale):
    """(kernel worst, kernel mean, yardstick worst, yardstick mean, yardstick median) of one quantity, in units."""
    k, y = row_units(x, want, scale).reshape(-1), row_units(lines, want, scale).reshape(-1)
    return k.max().item(), k.mean().item(), y.max().item(), y.mean().item(), y.median().item()


def rule_failures(name, x, lines, want, scale):
    """The rule for one quantity: a list of what it misses (empty: it holds), and the figures."""
    fig = row_figures(x, lines, want, scale)
    kworst, kmean, yworst, ymean, ymedian = fig
    failures = []
    dead = scale == 0
    if bool(dead.any()) and bool((x[dead] != 0).any()):
        failures.append((name, "a row of scale 0 is not 0", int((x[dead] != 0).sum())))
    if name not in NO_MEDIAN and not yworst <= MEDIAN_CAP * ymedian:
        failures.append((name, "yardstick not usable", yworst, ymedian))
    if not kworst <= max(WORST_FACTOR * yworst, UNITS_FLOOR):                      # a NaN fails here
        failures.append((name, "worst row", kworst, yworst, int(row_units(x, want, scale).reshape(-1).nan_to_num(nan=float("inf")).argmax())))
    if not kmean <= max(MEAN_FACTOR * ymean, UNITS_FLOOR):
        failures.append((name, "mean row", kmean, ymean))
    return failures, fig


# ---- a stand-in for the reference's backbone module (written for this project; attribute names are those the wrapper reads) -----

class StandinTransformerLayer(nn.Module):
    """The reference's TransformerLayer as the seam sees it: the same attributes and submodule names (so the same state_dict
    keys), a forward with its signature that looks the attention functions up in its module's globals at call time, and a
    counter of its calls."""

    def __init__(self, d_model=128, nhead=1, attention_type="swin", no_ffn=False, ffn_dim_expansion=4, with_shift=False,
                 add_per_view_attn=False, **kwargs):
        super().__init__()
        self.dim, self.nhead, self.attention_type, self.no_ffn = d_model, nhead, attention_type, no_ffn
        self.add_per_view_attn, self.with_shift = add_per_view_attn, with_shift
        self.q_proj, self.k_proj, self.v_proj, self.merge = (nn.Linear(d_model, d_model, bias=False) for _ in range(4))
        self.norm1 = nn.LayerNorm(d_model)
        if not no_ffn:
            self.mlp = nn.Sequential(nn.Linear(2 * d_model, 2 * d_model * ffn_dim_expansion, bias=False), nn.GELU(),
                                     nn.Linear(2 * d_model * ffn_dim_expansion, d_model, bias=False))
            self.norm2 = nn.LayerNorm(d_model)
        self.calls = 0

    def forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, attn_num_splits=None, **kwargs):
        self.calls += 1
        g = sys.modules[type(self).__module__].__dict__
        attn_type = kwargs.get("attn_type", self.attention_type)
        query, key, value = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        if attn_type == "swin" and attn_num_splits > 1:
            opts = dict(num_splits=attn_num_splits, with_shift=self.with_shift, h=height, w=width, attn_mask=shifted_window_attn_mask)
            if self.nhead > 1:
                message = g["multi_head_split_window_attention"](query, key, value, num_head=self.nhead, **opts)
            elif self.add_per_view_attn:
                b, l, c = query.shape
                views = key.shape[1]
                message = g["single_head_split_window_attention"](query.unsqueeze(1).expand(b, views, l, c).reshape(-1, l, c),
                                                                  key.reshape(-1, l, c), value.reshape(-1, l, c), **opts)
                message = message.view(b, views, l, c).sum(1)
            else:
                message = g["single_head_split_window_attention"](query, key, value, **opts)
        else:
            message = g["single_head_full_attention"](query, key, value)
        message = self.norm1(self.merge(message))
        if not self.no_ffn:
            message = self.norm2(self.mlp(torch.cat([source, message], dim=-1)))
        return source + message


def standin_module(name):
    """window_attention_reference.standin_module (the attention functions install(window_attention=True) rebinds) plus a
    TransformerLayer class of the module's own: a fresh class per module, so patches do not leak."""
    mod = W.standin_module(name)
    mod.TransformerLayer = type("TransformerLayer", (StandinTransformerLayer,), {"__module__": name})
    return mod


def randomise(layer, seed, scale=1.0):
    """Every parameter of a layer from a seeded generator: Linear weights with deviation scale / sqrt(fan-in), norm weights
    around 1, norm biases around 0."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for key, p in layer.named_parameters():
            if p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=gen) * scale / math.sqrt(p.shape[1]))
            elif key.endswith("weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(0.2 * torch.randn(p.shape, generator=gen))
    return layer
