"""The yardstick of the fused mono-feature fusion (splatter360_amd.mono_fusion): the project's own statement of what the
reference's EncoderCostVolume.forward computes with add_mono_feat (src/model/encoder/encoder_costvolume.py:297, :351-354, with the
rgbd_fusion of :119-125),

    m = Cube2Equirec(mono_cube)                     under no_grad: a constant
    X = cat([erp_feat, m], 1) as channel-last tokens;  yv = X W1^T;  a = relu(LN(yv));  out = a W2^T, back as [N, C, H, W]
    LN(x) = (x - mean) / sqrt(var + eps) weight + bias over the channels, var the BIASED variance

generic in C and Cm (`statement`: m is the FLOAT32 stitch value — the eight taps of tests/stitch_reference.py, float32 weights
(wx wy) wz, float32 products added in tap order — and everything after it runs in the dtype asked for; float64 is what the kernels
are held to), the same five lines in float32 as stock torch runs them on the tensors' device (`reference_lines`: F.grid_sample as
the reference's Cube2Equirec.forward calls it, torch.cat, the permute, F.linear, F.layer_norm, F.relu, F.linear — the yardstick of
the accuracy rule), gradients, deterministic inputs (`random_case`; `decided_case`, whose ReLU decisions no rounding can move) and a
stand-in for the reference's encoder module, written for this project, that the installed seam rebinds.  The statement is held to
the reference's recorded outputs (tests/golden/mono_fusion.npz) by tests/test_mono_fusion_spec.py.  Further the per-row measure of
tests/test_gpu_mono_fusion_float64.py: `row_statement` (the float64 results per token, per column of the two weight gradients and
per channel, and each row's scale), `lines_rows` (the float32 lines in the same indexing), the rule (`rule_failures`) and the cases.
Nothing here needs a GPU.
"""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import stitch_reference as S
import transformer_ffn_reference as FF
import window_attention_reference as W
from group_norm_reference import lattice
from splatter360_amd import stitch as _stitch

NAMES = ("erp_feat", "mono_cube", "grid", "w1", "ln_weight", "ln_bias", "w2")
DIFFERENTIABLE = (0, 3, 4, 5, 6)                 # erp_feat and the four parameters; mono_cube and the grid are constants
RESULTS = ("out", "g_erp_feat", "g_w1", "g_ln_weight", "g_ln_bias", "g_w2")
# (face_w, equ_h, equ_w): each builds with the reference's Cube2Equirec and gives the project's grid bit for bit
GEOMETRIES = {"g0": (2, 4, 8), "g1": (4, 8, 16), "g2": (3, 6, 8), "g3": (8, 12, 24)}


def grid_of(geometry) -> torch.Tensor:
    """[H, W, 3] float32: Cube2Equirec.sample_grid[0, 0] as splatter360_amd.stitch builds it."""
    fw, h, w = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    return torch.from_numpy(_stitch.sample_grid_numpy(fw, h, w).copy())


def stitch32(mono_cube, grid) -> torch.Tensor:
    """The float32 stitch [N, Cm, H, W] of mono_cube [N, Cm, fw, 6 fw] (faces side by side, slot order): per pixel the eight taps
    of stitch_reference.taps in float32, a tap outside the volume skipped, float32 products added in tap order from zero."""
    cube = np.asarray(mono_cube.detach().cpu().numpy(), np.float32)
    g = np.asarray(grid.detach().cpu().numpy(), np.float32)
    n, cm, fw, _ = cube.shape
    h, w = g.shape[:2]
    tex, wgt, valid = S.taps(g, fw, np.float32)
    vol = cube.reshape(n, cm, fw, 6, fw).transpose(0, 1, 3, 2, 4).reshape(n, cm, 6 * fw * fw)     # slot-space z, y, x
    out = np.zeros((n, cm, h * w), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(8):
            ok = valid[:, k]
            out[:, :, ok] = out[:, :, ok] + vol[:, :, tex[ok, k]] * wgt[ok, k]
    return torch.from_numpy(out.reshape(n, cm, h, w))


def layer_norm(x, weight, bias, eps):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def statement(erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps=1e-5, dtype=torch.float64, parts=None, m=None):
    """The fusion in `dtype`, pure torch, differentiable in erp_feat and the parameters, generic in C and Cm.  m: stitch32 of the
    case if at hand.  parts: a dict that receives "y" = X W1^T [T, C], "ln", LayerNorm's output [N, H, W, C], and "a", its ReLU,
    as they stand in the graph."""
    if m is None:
        m = stitch32(mono_cube, grid)
    m = m.to(device=erp_feat.device, dtype=dtype)
    erp_feat, w1, ln_weight, ln_bias, w2 = (t.to(dtype) for t in (erp_feat, w1, ln_weight, ln_bias, w2))
    x = torch.cat([erp_feat, m], dim=1).permute(0, 2, 3, 1)
    y = x @ w1.transpose(0, 1)
    rows = y.reshape(-1, y.shape[-1])                              # [T, C], in the graph: LayerNorm reads it
    ln = layer_norm(rows.reshape(y.shape), ln_weight, ln_bias, eps)
    a = torch.relu(ln)
    if parts is not None:
        parts["y"], parts["ln"], parts["a"] = rows, ln, a
    return (a @ w2.transpose(0, 1)).permute(0, 3, 1, 2)


def stitch_lines(mono_cube, grid):
    """Cube2Equirec.forward's lines (the reference's src/geometry/layers.py:108-116) on the grid [H, W, 3]."""
    bs, ch, h, w = mono_cube.shape
    cube = mono_cube.view(bs, ch, 1, h, w)
    cube = torch.cat(torch.split(cube, h, dim=-1), dim=2).view(bs, ch, 6, h, h)
    sample_grid = torch.cat(bs * [grid.view(1, 1, *grid.shape)], dim=0)
    return F.grid_sample(cube, sample_grid, padding_mode="border", align_corners=True).squeeze(2)


def reference_lines(erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps=1e-5, parts=None):
    """The reference's five lines in float32 on the tensors' device.  Forms the stitched map, the concatenation, its channel-last
    copy and the three [T, C] activations.  parts: a dict that receives "y", the first Linear's float32 output [T, C]."""
    with torch.no_grad():
        features_mono = stitch_lines(mono_cube, grid)
    t = torch.cat([erp_feat, features_mono], dim=1)
    t = t.permute(0, 2, 3, 1)
    t = F.linear(t, w1)
    if parts is not None:
        parts["y"] = t.reshape(-1, t.shape[-1])
    t = F.linear(F.relu(F.layer_norm(t, (w1.shape[0],), ln_weight, ln_bias, eps)), w2)
    return t.permute(0, 3, 1, 2)


def gradients(fn, tensors, g, dtype=None):
    """(out, gradients of erp_feat, w1, ln_weight, ln_bias, w2) of fn(*tensors) with the output gradient g, all detached, in
    RESULTS' order; the differentiable tensors in `dtype` if given (mono_cube and the grid are passed as they are)."""
    xs = [t.detach().clone() for t in tensors]
    for i in DIFFERENTIABLE:
        xs[i] = xs[i].to(dtype or xs[i].dtype).requires_grad_(True)
    out = fn(*xs)
    out.backward(g.to(out.dtype))
    return (out.detach(), *(xs[i].grad for i in DIFFERENTIABLE))


def random_case(n, geometry, cm, scale=1.0, seed=0, device="cpu", c=128):
    """(the seven tensors of NAMES, g), float32, deterministic: erp_feat and mono_cube standard normal times `scale`, the Linear
    weights normal with nn.Linear's 1 / sqrt(fan-in) deviation, the norm's weight around 1 and bias around 0, g standard normal."""
    fw, h, w = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    gen = torch.Generator().manual_seed(seed)
    erp = torch.randn(n, c, h, w, generator=gen) * scale
    cube = torch.randn(n, cm, fw, 6 * fw, generator=gen) * scale
    w1 = torch.randn(c, c + cm, generator=gen) / math.sqrt(c + cm)
    lnw = 1 + 0.2 * torch.randn(c, generator=gen)
    lnb = 0.2 * torch.randn(c, generator=gen)
    w2 = torch.randn(c, c, generator=gen) / math.sqrt(c)
    g = torch.randn(n, c, h, w, generator=gen)
    return tuple(t.to(device) for t in (erp, cube, grid_of((fw, h, w)), w1, lnw, lnb, w2)), g.to(device)


def decided_case(n, geometry, cm, scale=1.0, seed=0, device="cpu", c=128):
    """random_case with ln_weight = +-0.05 (lattice in [0.5, 1]) and ln_bias = +-1: |ln_weight x_hat| <= 0.05 sqrt(C - 1) < 1
    for C = 128, so every unit is on or off by its bias's sign whatever the rounding of the products before it."""
    (erp, cube, grid, w1, _, _, w2), g = random_case(n, geometry, cm, scale, seed, "cpu", c)
    k = lattice((c,), 7000 + seed, scale=1.0, span=33).astype(np.float64)            # integers in [-16, 16]
    sign = np.where(lattice((c,), 7100 + seed, scale=1.0, span=2) < 0, -1.0, 1.0)
    lnw = torch.from_numpy((sign * 0.05 * (0.75 + k / 64.0)).astype(np.float32))
    lnb = torch.from_numpy(np.where(lattice((c,), 7200 + seed, scale=1.0, span=2) < 0, -1.0, 1.0).astype(np.float32))
    assert 0.05 * math.sqrt(c - 1) < 1 and lnw.abs().min() >= 0.025 and lnw.abs().max() <= 0.05
    return tuple(t.to(device) for t in (erp, cube, grid, w1, lnw, lnb, w2)), g.to(device)


def ln_margin(tensors, m=None) -> float:
    """min |v| / max |v| over LayerNorm's outputs of the float64 statement, on the CPU: how far the nearest ReLU decision is
    from 0 in units of the largest value."""
    parts = {}
    statement(*(t.detach().cpu() for t in tensors), parts=parts, m=m)
    v = parts["ln"].abs()
    return (v.min() / v.max()).item()


def clipped_pixels(geometry) -> np.ndarray:
    """Flat indices of the grid's pixels that have a coordinate clipped to exactly +-1 in u or v: their upper tap along that axis
    has weight 0 at index fw."""
    g = grid_of(geometry).numpy().reshape(-1, 3)
    return np.flatnonzero((np.abs(g[:, 0]) == 1) | (np.abs(g[:, 1]) == 1))


# ---- the per-row measure (tests/test_mono_fusion_rows.py, tests/test_gpu_mono_fusion_float64.py) --------------------------------
# Every quantity is indexed by what owns it in the kernels, one number per row, in units of 2^-24 of the ROW'S OWN scale
# (row_units: the window attention's definition).  Token rows [T, C]: out, y (the first Linear's output, which the forward saves)
# and g_erp_feat, scale max_c |want|.  Column rows, both held TRANSPOSED: g_w1 as [C + Cm, C], one row per input channel k of X
# (rows [0, C) are erp_feat's channels, row C + j is stitched channel j: each on its own scale; 64 consecutive rows are one
# workgroup column group of the weight pass), g_w2 as [C, C], one row per unit j of a; scale max |want| over the row.  Channels
# [C]: the LayerNorm parameter gradients, each a sum over tokens; scale the sum over tokens of the summed terms' magnitudes.
TOKEN_ROWS = ("out", "y", "g_erp_feat")
COLUMN_ROWS = ("g_w1", "g_w2")
CHANNEL_ROWS = ("g_ln_weight", "g_ln_bias")
ROW_NAMES = TOKEN_ROWS + COLUMN_ROWS + CHANNEL_ROWS
UNIT, SCALE_FLOOR = W.UNIT, W.SCALE_FLOOR
row_units = W.row_units
WORST_FACTOR, MEAN_FACTOR, UNITS_FLOOR, MEDIAN_CAP = FF.WORST_FACTOR, FF.MEAN_FACTOR, FF.UNITS_FLOOR, FF.MEDIAN_CAP

# name: (N, geometry, Cm, kind).  The first five are the shapes of tests/test_gpu_mono_fusion.py with its seeds ("high": those of
# tests/test_gpu_mono_fusion_high.py); the others are the smallest shapes that reach each path of the launch geometry
# (tests/test_mono_fusion_rows.py asserts the structure from the kernel file's constants).  Each of the others is a decided_case:
# no ReLU decision hangs on rounding; the five random ones keep the margin assertions of their files.
ROW_CASES = {
    "wave": (1, "g0", 64, "random"),
    "tile": (1, "g1", 64, "random"),
    "straddle": (3, "g2", 192, "random"),
    "config": (1, "g1", 384, "random"),
    "wide": (1, "g0", 1024, "random"),
    "wg2": (11, (2, 3, 4), 64, "decided"),     # 132 tokens in panoramas of 12: three or four panoramas per wave; a second workgroup of
    #                                            four tokens in wave 0 and three empty waves; 3 tiles of the weight pass, the last of 4 tokens
    "mixed": (2, "g3", 128, "decided"),        # 576 tokens: g times MIXED_GAINS cyclically over the tokens, mono_cube's channels times
    #                                            MIXED_CHANNEL_GAINS alternately: quiet token rows and quiet g_w1 rows next to loud ones
    "tiles3": (15, "g3", 64, "decided"),       # 4 320 tokens: 68 tiles in 32 chunks of two and three, the last tile of 32 tokens; 34 token
    #                                            workgroups (two reduce batches and a tail of 2), the last with three valid waves
    "tiles5": (29, "g3", 64, "decided"),       # 8 352 tokens: 131 tiles in chunks of four and five; 66 workgroups (four batches and 2)
}
POOLED_SEEDS = {"highest": {"wave": 100, "tile": 101, "straddle": 100, "config": 100, "wide": 100},
                "high": {"wave": 101, "tile": 111, "straddle": 108, "config": 100, "wide": 101}}
NEW_SEEDS = {"wg2": 210, "mixed": 211, "tiles3": 212, "tiles5": 213}
ROW_SEEDS = {}                                                  # (name, precision): a seed other than the default (the yardstick's condition)
MIXED_GAINS = (1.0, 1e-1, 1e-2, 1e-3)
MIXED_CHANNEL_GAINS = (1.0, 1e-3)
UNITS_FROM = 129                                                # column rows and channels are judged from this T on; the pooled files
#                                                                 keep the small shapes for them, as with the FFN tail
ROW_SCALES = (1.0, 6.0)
ROW_RUNS = [(name, scale) for name in ROW_CASES for scale in ROW_SCALES]


def row_tokens(name) -> int:
    n, geometry, _, _ = ROW_CASES[name]
    _, h, w = GEOMETRIES[geometry] if isinstance(geometry, str) else geometry
    return n * h * w


def row_seed(name, precision="highest") -> int:
    return ROW_SEEDS.get((name, precision), POOLED_SEEDS[precision][name] if name in POOLED_SEEDS[precision] else NEW_SEEDS[name])


def row_inputs(name, scale=1.0, precision="highest", device="cpu"):
    """(the seven tensors, g) of a run of ROW_RUNS: the one set of inputs the CPU and the GPU tests of the per-row rule share."""
    n, geometry, cm, kind = ROW_CASES[name]
    make = decided_case if kind == "decided" else random_case
    tensors, g = make(n, geometry, cm, scale=scale, seed=row_seed(name, precision))
    if name == "mixed":
        tokens = g.shape[0] * g.shape[2] * g.shape[3]
        gains = torch.tensor(MIXED_GAINS)[torch.arange(tokens) % len(MIXED_GAINS)]
        g = g * gains.reshape(g.shape[0], 1, g.shape[2], g.shape[3])
        cube = tensors[1] * torch.tensor(MIXED_CHANNEL_GAINS)[torch.arange(cm) % len(MIXED_CHANNEL_GAINS)].reshape(1, cm, 1, 1)
        tensors = (tensors[0], cube, *tensors[2:])
    return tuple(t.to(device) for t in tensors), g.to(device)


def row_names(tokens):
    """The quantities that are judged at `tokens` tokens."""
    return ROW_NAMES if tokens >= UNITS_FROM else TOKEN_ROWS


def as_rows(named):
    """A {name: tensor} dict of the fusion's results in the tensors' own layouts -> the per-row indexing: out and g_erp_feat
    [N, C, H, W] as [T, C] (a copy), y [T, C], g_w1 and g_w2 transposed (views)."""
    def rows(n, x):
        if n in ("out", "g_erp_feat"):
            return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        return x.t() if n in COLUMN_ROWS else x
    return {n: rows(n, x) for n, x in named.items()}


def _x_hat(y, eps):
    mean = y.mean(dim=-1, keepdim=True)
    return (y - mean) / torch.sqrt(((y - mean) ** 2).mean(dim=-1, keepdim=True) + eps)


def _rows_of(fn, tensors, g, dtype=None):
    """ROW_NAMES' results of fn(*tensors, parts=) by autograd in the per-row indexing, and LayerNorm's output with its gradient
    if fn records it."""
    parts = {}
    xs = [t.detach().clone() for t in tensors]
    for i in DIFFERENTIABLE:
        xs[i] = xs[i].to(dtype or xs[i].dtype).requires_grad_(True)
    out = fn(*xs, parts=parts)
    if "ln" in parts:
        parts["ln"].retain_grad()
    out.backward(g.to(out.dtype))
    named = {"out": out.detach(), "y": parts["y"].detach(), "g_erp_feat": xs[0].grad, "g_w1": xs[3].grad, "g_ln_weight": xs[4].grad,
             "g_ln_bias": xs[5].grad, "g_w2": xs[6].grad}
    return as_rows({n: named[n] for n in ROW_NAMES}), parts


def row_statement(tensors, g, eps=1e-5):
    """(want, scale): two dicts over ROW_NAMES, float64 on the inputs' device, in the per-row indexing.  want: `statement` by
    autograd (m = stitch32 of the case), y taken from inside it.  scale: one number per row; a unit that is off at every token
    has scale 0 in its row of g_w2 and in its two channels."""
    m = stitch32(tensors[1], tensors[2])
    want, parts = _rows_of(lambda *t, parts: statement(*t, eps=eps, parts=parts, m=m), tensors, g, torch.float64)
    c = want["y"].shape[-1]
    g_ln = parts["ln"].grad.reshape(-1, c)
    scale = {n: want[n].abs().amax(-1) for n in TOKEN_ROWS + COLUMN_ROWS}
    scale["g_ln_weight"] = (g_ln * _x_hat(want["y"], eps)).abs().sum(0)
    scale["g_ln_bias"] = g_ln.abs().sum(0)
    return want, scale


def lines_rows(tensors, g, eps=1e-5):
    """The float32 yardstick in the same indexing: reference_lines and its gradients by autograd, y taken from inside."""
    return _rows_of(lambda *t, parts: reference_lines(*t, eps=eps, parts=parts), tensors, g)[0]


# The rule, per run and quantity (units of 2^-24 of the row's scale), the factors being transformer_ffn_reference's:
#   a row of scale 0 (a dead unit) is exactly 0 in the kernel's result, in the lines' and in the three-term statement's, and is
#   left out of every figure below: a decided_case switches about half the units off, so with them the median of g_w2 would be 0
#   "highest":  worst row: kernel <= max(2 x lines' worst row, 0.5)        mean row: kernel <= max(1.5 x lines' mean row, 0.5)
#   "high" (three given): the pooled "high" rule row by row, e3 the three-term statement's units and e32 the lines':
#               worst row: kernel <= max(2 x (worst e3 + worst e32), 0.5)   mean row: kernel <= max(1.5 x (mean e3 + mean e32), 0.5)
#   token and column rows: a yardstick's worst row <= 5 x its own median row (e32, and e3 where it is given), else "yardstick
#   not usable" (a failure).  The channel gradients have no such condition, as in the FFN tail.
NO_MEDIAN = CHANNEL_ROWS


def _figures(units, live):
    u = units.reshape(-1)[live.reshape(-1)]
    return u.max().item(), u.mean().item(), u.median().item()


def rule_failures(name, x, lines, want, scale, three=None):
    """The rule for one quantity: a list of what it misses (empty: it holds), and the figures (kernel worst, kernel mean, lines'
    worst, mean, median; with `three` also the three-term statement's worst, mean, median), all over the rows of scale > 0."""
    failures = []
    dead = scale == 0
    live = ~dead
    for what, t in (("a row of scale 0 is not 0", x), ("a row of scale 0 is not 0 in the lines", lines),
                    ("a row of scale 0 is not 0 in the three-term statement", three)):
        if t is not None and bool(dead.any()) and bool((t[dead] != 0).any()):
            failures.append((name, what, int((t[dead] != 0).sum())))
    if not bool(live.any()):
        return failures + [(name, "no row has a scale")], (float("nan"),) * (5 if three is None else 8)
    ku = row_units(x, want, scale)
    kworst, kmean, _ = _figures(ku, live)
    yworst, ymean, ymedian = _figures(row_units(lines, want, scale), live)
    fig = (kworst, kmean, yworst, ymean, ymedian)
    bworst, bmean = yworst, ymean
    if name not in NO_MEDIAN and not yworst <= MEDIAN_CAP * ymedian:
        failures.append((name, "yardstick not usable", yworst, ymedian))
    if three is not None:
        tworst, tmean, tmedian = _figures(row_units(three, want, scale), live)
        fig += (tworst, tmean, tmedian)
        bworst, bmean = tworst + yworst, tmean + ymean
        if name not in NO_MEDIAN and not tworst <= MEDIAN_CAP * tmedian:
            failures.append((name, "three-term yardstick not usable", tworst, tmedian))
    if not kworst <= max(WORST_FACTOR * bworst, UNITS_FLOOR):                      # a NaN fails here
        at = int(torch.where(live.reshape(-1), ku.reshape(-1).nan_to_num(nan=float("inf")), -1.0).argmax())
        failures.append((name, "worst row", kworst, bworst, at))
    if not kmean <= max(MEAN_FACTOR * bmean, UNITS_FLOOR):
        failures.append((name, "mean row", kmean, bmean))
    return failures, fig


# ---- a stand-in for the reference's encoder module (written for this project; attribute names are those the seam reads) ---------

class StandinCube2Equirec(nn.Module):
    """Cube2Equirec as the seam sees it: face_w, equ_h, equ_w, the sample_grid parameter [1, 1, H, W, 3] and a forward that is
    grid_sample over the six faces (stitch_lines)."""

    def __init__(self, face_w, equ_h, equ_w):
        super().__init__()
        self.face_w, self.equ_h, self.equ_w = face_w, equ_h, equ_w
        self.sample_grid = nn.Parameter(grid_of((face_w, equ_h, equ_w)).view(1, 1, equ_h, equ_w, 3), requires_grad=False)
        self.calls = 0

    def forward(self, cube_feat):
        self.calls += 1
        return stitch_lines(cube_feat, self.sample_grid[0, 0])


class StandinEncoderCostVolume(nn.Module):
    """EncoderCostVolume as the seam sees it: a c2e, an rgbd_fusion (only with add_mono_feat) with the reference's four layers,
    map_pdf_to_opacity (what install(depth_tail=True) rebinds on the same class), and a forward that runs the five statements with
    einops."""

    def __init__(self, geometry=(4, 8, 16), d=128, mono_channels=64, add_mono_feat=True):
        super().__init__()
        self.c2e = StandinCube2Equirec(*geometry)
        if add_mono_feat:
            self.rgbd_fusion = nn.Sequential(nn.Linear(mono_channels + d, d, bias=False), nn.LayerNorm(d), nn.ReLU(),
                                             nn.Linear(d, d, bias=False))

    def map_pdf_to_opacity(self, pdf, global_step):
        return pdf

    def forward(self, trans_features, features_mono):
        from einops import rearrange
        with torch.no_grad():
            features_mono = self.c2e(features_mono)
        trans_features = torch.cat([trans_features, features_mono], dim=1)
        trans_features = self.rgbd_fusion(rearrange(trans_features, "bv c h w -> bv h w c"))
        trans_features = rearrange(trans_features, "bv h w c -> bv c h w")
        return trans_features


def standin_module(name):
    """A module of the given name with an EncoderCostVolume class of its own (a fresh class per module, so patches do not leak)."""
    mod = types.ModuleType(name)
    mod.Cube2Equirec = StandinCube2Equirec
    mod.EncoderCostVolume = type("EncoderCostVolume", (StandinEncoderCostVolume,), {
        "__module__": name,
        "__init__": lambda self, *a, **k: StandinEncoderCostVolume.__init__(self, *a, **k),
        "map_pdf_to_opacity": lambda self, pdf, global_step: pdf})
    return mod


def set_parameters(encoder, tensors):
    """Copy w1, ln_weight, ln_bias, w2 of a case into an encoder's rgbd_fusion."""
    _, _, _, w1, lnw, lnb, w2 = tensors
    with torch.no_grad():
        encoder.rgbd_fusion[0].weight.copy_(w1)
        encoder.rgbd_fusion[1].weight.copy_(lnw)
        encoder.rgbd_fusion[1].bias.copy_(lnb)
        encoder.rgbd_fusion[3].weight.copy_(w2)
    return encoder
