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
the reference's recorded outputs (tests/golden/mono_fusion.npz) by tests/test_mono_fusion_spec.py.  Nothing here needs a GPU.
"""
import math
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

import stitch_reference as S
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
    case if at hand.  parts: a dict that receives "ln", LayerNorm's output [N, H, W, C] as it stands in the graph."""
    if m is None:
        m = stitch32(mono_cube, grid)
    m = m.to(device=erp_feat.device, dtype=dtype)
    erp_feat, w1, ln_weight, ln_bias, w2 = (t.to(dtype) for t in (erp_feat, w1, ln_weight, ln_bias, w2))
    x = torch.cat([erp_feat, m], dim=1).permute(0, 2, 3, 1)
    ln = layer_norm(x @ w1.transpose(0, 1), ln_weight, ln_bias, eps)
    if parts is not None:
        parts["ln"] = ln
    return (torch.relu(ln) @ w2.transpose(0, 1)).permute(0, 3, 1, 2)


def stitch_lines(mono_cube, grid):
    """Cube2Equirec.forward's lines (the reference's src/geometry/layers.py:108-116) on the grid [H, W, 3]."""
    bs, ch, h, w = mono_cube.shape
    cube = mono_cube.view(bs, ch, 1, h, w)
    cube = torch.cat(torch.split(cube, h, dim=-1), dim=2).view(bs, ch, 6, h, h)
    sample_grid = torch.cat(bs * [grid.view(1, 1, *grid.shape)], dim=0)
    return F.grid_sample(cube, sample_grid, padding_mode="border", align_corners=True).squeeze(2)


def reference_lines(erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps=1e-5):
    """The reference's five lines in float32 on the tensors' device.  Forms the stitched map, the concatenation, its channel-last
    copy and the three [T, C] activations."""
    with torch.no_grad():
        features_mono = stitch_lines(mono_cube, grid)
    t = torch.cat([erp_feat, features_mono], dim=1)
    t = t.permute(0, 2, 3, 1)
    t = F.linear(F.relu(F.layer_norm(F.linear(t, w1), (w1.shape[0],), ln_weight, ln_bias, eps)), w2)
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
