"""The yardstick of the fused group norm + activation + residual (splatter360_amd.group_norm): a float64 statement of

    mu, var = mean and biased variance of the slab (n, g): channels g cpg .. (g + 1) cpg - 1, all trailing dims
    r = 1 / sqrt(var + eps),  xh = (x - mu) r,  z = xh gamma_c + beta_c,  out = residual + a(z)
    dz = g_out a'(z),  m1 = sum_c gamma_c sum_s dz / M,  m2 = sum_c gamma_c sum_s dz xh / M
    g_x = r (gamma_c dz - m1 - xh m2),  g_weight[c] = sum_{n,s} dz xh,  g_bias[c] = sum_{n,s} dz,  g_residual = g_out

with a in {none, relu, silu, gelu (erf form)}, the per-element scales of the accuracy rule, the rule itself, deterministic
cases, and stand-ins for the reference's classes the installed seam rebinds.  The statement is held to the reference's recorded
outputs (tests/golden/group_norm.npz) by tests/test_group_norm_spec.py.  Everything here runs on the CPU.
"""
import math
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ACTIVATIONS = ("none", "relu", "silu", "gelu")
E23, E40, E30 = 2.0 ** -23, 2.0 ** -40, 2.0 ** -30


def _t64(a):
    if a is None:
        return None
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(torch.float64)


def act64(z, activation):
    """(a(z), a'(z)) in float64, closed forms."""
    if activation == "none":
        return z, torch.ones_like(z)
    if activation == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z)), (z > 0).to(z.dtype)
    if activation == "silu":
        s = torch.sigmoid(z)
        return z * s, s * (1 + z * (1 - s))
    if activation == "gelu":
        phi = 0.5 * torch.special.erfc(-z / math.sqrt(2.0))
        return z * phi, phi + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    raise ValueError(activation)


def statement(x, groups, weight=None, bias=None, eps=1e-5, activation="none", residual=None, g_out=None):
    """The float64 statement on float32 (or float64) inputs -> dict of float64 numpy arrays: out, A (the scale of out's rule), z,
    stats [N G, 2] = (mu, r); with g_out also g_x, gx_scale, g_weight, gw_scale, g_bias, gb_scale."""
    x, weight, bias, residual, g_out = (_t64(t) for t in (x, weight, bias, residual, g_out))
    shape = tuple(x.shape)
    n, c = shape[:2]
    cpg = c // groups
    xs = x.reshape(n, groups, cpg, -1)
    m = xs.shape[2] * xs.shape[3]
    mu = xs.mean(dim=(2, 3), keepdim=True)
    var = ((xs - mu) ** 2).mean(dim=(2, 3), keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (xs - mu) * r
    gam = (torch.ones(c, dtype=torch.float64) if weight is None else weight).reshape(1, groups, cpg, 1)
    bet = (torch.zeros(c, dtype=torch.float64) if bias is None else bias).reshape(1, groups, cpg, 1)
    z = xh * gam + bet
    a, da = act64(z, activation)
    res = torch.zeros_like(xs) if residual is None else residual.reshape(xs.shape)
    out = res + a
    want = {"out": out.reshape(shape), "A": ((xh * gam).abs() + bet.abs() + res.abs()).reshape(shape), "z": z.reshape(shape),
            "stats": torch.stack([mu.reshape(-1), r.reshape(-1)], dim=1)}
    if g_out is not None:
        dz = g_out.reshape(xs.shape) * da
        m1 = (gam * dz).sum(dim=(2, 3), keepdim=True) / m
        m2 = (gam * dz * xh).sum(dim=(2, 3), keepdim=True) / m
        want["g_x"] = (r * (gam * dz - m1 - xh * m2)).reshape(shape)
        want["gx_scale"] = (r * ((gam * dz).abs() + m1.abs() + (xh * m2).abs())).reshape(shape)
        want["g_weight"] = (dz * xh).sum(dim=(0, 3)).reshape(c)
        want["gw_scale"] = (dz * xh).abs().sum(dim=(0, 3)).reshape(c)
        want["g_bias"] = dz.sum(dim=(0, 3)).reshape(c)
        want["gb_scale"] = dz.abs().sum(dim=(0, 3)).reshape(c)
    return {k: v.numpy() for k, v in want.items()}


def torch_lines(x, groups, weight=None, bias=None, eps=1e-5, activation="none", residual=None, g_out=None, dtype=torch.float32,
                device="cpu"):
    """What stock torch computes: F.group_norm, the activation, the add, autograd — in `dtype` on `device`.  Returns
    (out, g_x, g_weight, g_bias) (gradients None without g_out / parameters)."""
    def leaf(a):
        return None if a is None else torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype).requires_grad_(True)
    x, weight, bias = leaf(x), leaf(weight), leaf(bias)
    y = F.group_norm(x, groups, weight, bias, eps)
    y = {"none": lambda t: t, "relu": F.relu, "silu": F.silu, "gelu": F.gelu}[activation](y)
    if residual is not None:
        y = torch.as_tensor(np.asarray(residual)).to(device=device, dtype=dtype) + y
    if g_out is None:
        return y.detach(), None, None, None
    y.backward(torch.as_tensor(np.asarray(g_out)).to(device=device, dtype=dtype))
    return y.detach(), x.grad, None if weight is None else weight.grad, None if bias is None else bias.grad


# ---- the accuracy rule ---------------------------------------------------------------------------------------------------------

def worst(got, want, scale):
    """max over elements of |got - want| / (2^-23 |want| + 2^-40 scale) (0 / 0 counts as 0): the rule holds iff <= 1."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    err, bound = np.abs(got - want), E23 * np.abs(want) + E40 * scale
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max())


def stats_worst(got, want):
    """max relative distance of (mu, r) from the statement's, in units of 2^-40."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
    return float(rel.max() / E40)


def relu_is_unambiguous(want) -> bool:
    """No element of the statement has |z| < 2^-30 A: the branch of relu cannot depend on rounding."""
    return bool((np.abs(want["z"]) >= E30 * want["A"]).all())


# ---- cases ---------------------------------------------------------------------------------------------------------------------

def make_case(shape, groups, affine=True, residual=True, seed=0, offset=0.5, spread=1.5):
    """Deterministic float32 numpy inputs: x, weight, bias (None without affine), residual (or None), g_out."""
    rng = np.random.default_rng(1000 + seed)
    c = shape[1]
    per_channel = rng.standard_normal((1, c) + (1,) * (len(shape) - 2))
    case = {"x": (offset + spread * rng.standard_normal(shape) + 0.7 * per_channel).astype(np.float32),
            "weight": (1.0 + 0.5 * rng.standard_normal(c)).astype(np.float32) if affine else None,
            "bias": (0.3 * rng.standard_normal(c)).astype(np.float32) if affine else None,
            "residual": rng.standard_normal(shape).astype(np.float32) if residual else None,
            "g_out": rng.standard_normal(shape).astype(np.float32), "groups": groups}
    return case


def lattice(shape, seed, scale=1.0 / 64.0, span=31):
    """A deterministic float32 array from integer arithmetic alone (the same bits on every machine, exact in float32): the
    golden's convolution weights, which are too large to store.  Values k scale, k in [-span // 2, span // 2]."""
    count = int(np.prod(shape))
    h = (np.arange(count, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(40503 * (seed + 1))) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    k = (h % np.uint64(span)).astype(np.int64) - span // 2
    return (k.astype(np.float64) * scale).astype(np.float32).reshape(shape)


# ---- stand-ins for the reference's classes (written for this project; attribute names are those the wrappers read) --------------

class GroupNorm8(nn.GroupNorm):
    """The reference's norm class: computes in float32 whatever comes in."""

    def forward(self, x):
        return super().forward(x.float()).type(x.dtype)


def normalization(channels):
    return GroupNorm8(8 if channels % 8 == 0 else 4, channels)


def _zeroed(module):
    for p in module.parameters():
        p.detach().zero_()
    return module


class StandinResBlock(nn.Module):
    def __init__(self, channels, out_channels=None, postnorm=True, up=False, down=False):
        super().__init__()
        out_channels = out_channels or channels
        self.channels, self.out_channels = channels, out_channels
        if postnorm:
            self.in_layers = nn.Sequential(nn.Conv2d(channels, out_channels, 3, padding=1), normalization(out_channels), nn.SiLU())
            self.out_layers = nn.Sequential(nn.Conv2d(out_channels, out_channels, 3, padding=1), _zeroed(normalization(out_channels)), nn.SiLU())
        else:
            self.in_layers = nn.Sequential(normalization(channels), nn.SiLU(), nn.Conv2d(channels, out_channels, 3, padding=1))
            self.out_layers = nn.Sequential(normalization(out_channels), nn.SiLU(), nn.Dropout(p=0.0),
                                            _zeroed(nn.Conv2d(out_channels, out_channels, 3, padding=1)))
        self.updown = up or down
        self.h_upd = self.x_upd = nn.Upsample(scale_factor=2, mode="nearest") if up else nn.AvgPool2d(2) if down else nn.Identity()
        self.skip_connection = nn.Identity() if out_channels == channels else nn.Conv2d(channels, out_channels, 1)

    def forward(self, x, emb=None):
        return self._forward(x, emb)                              # the method is looked up on the instance per call

    def _forward(self, x, emb=None):
        if self.updown:
            h = self.in_layers[-1](self.h_upd(self.in_layers[:-1](x)))
            x = self.x_upd(x)
        else:
            h = self.in_layers(x)
        return self.skip_connection(x) + self.out_layers(h)


class StandinAttention(nn.Module):
    """softmax((q c^-1/4)^T (k c^-1/4)) v per head on [N, heads * 3 * c, T], heads split before q, k, v; with cross_view the
    views of the (v b) batch are laid side by side along T."""

    def __init__(self, n_heads, n_frames=2, use_cross_view_self_attn=False):
        super().__init__()
        self.n_heads, self.n_frames, self.use_cross_view_self_attn = n_heads, n_frames, use_cross_view_self_attn

    def forward(self, qkv):
        v = self.n_frames
        if self.use_cross_view_self_attn:
            vb, n, t = qkv.shape
            qkv = qkv.reshape(v, vb // v, n, t).permute(1, 2, 0, 3).reshape(vb // v, n, v * t)
        bs, width, length = qkv.shape
        ch = width // (3 * self.n_heads)
        q, k, val = qkv.reshape(bs * self.n_heads, ch * 3, length).split(ch, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        w = torch.einsum("bct,bcs->bts", q * scale, k * scale)
        w = torch.softmax(w.float(), dim=-1).type(w.dtype)        # in float32 whatever comes in, as the reference's
        a = torch.einsum("bts,bcs->bct", w, val).reshape(bs, -1, length)
        if self.use_cross_view_self_attn:
            b, n, vt = a.shape
            a = a.reshape(b, n, v, vt // v).permute(2, 0, 1, 3).reshape(v * b, n, vt // v)
        return a


class StandinAttentionBlock(nn.Module):
    def __init__(self, channels, num_head_channels=32, postnorm=True, num_frames=2, use_cross_view_self_attn=True):
        super().__init__()
        self.channels, self.num_heads, self.postnorm = channels, channels // num_head_channels, postnorm
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.attention = StandinAttention(self.num_heads, num_frames, use_cross_view_self_attn)
        if postnorm:
            self.proj_out = nn.Conv1d(channels, channels, 1)
            self.norm = _zeroed(normalization(channels))
        else:
            self.norm = normalization(channels)
            self.proj_out = _zeroed(nn.Conv1d(channels, channels, 1))

    def forward(self, x):
        return self._forward(x)

    def _forward(self, x):
        b, c, *spatial = x.shape
        x = x.reshape(b, c, -1)
        if self.postnorm:
            h = self.norm(self.proj_out(self.attention(self.qkv(x))))
        else:
            h = self.proj_out(self.attention(self.qkv(self.norm(x))))
        return (x + h).reshape(b, c, *spatial)


class StandinResidualBlock(nn.Module):
    def __init__(self, in_planes, planes, norm_layer=nn.InstanceNorm2d, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, 3, padding=1, stride=stride, bias=False)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2 = norm_layer(planes), norm_layer(planes)
        self.downsample = None
        if stride != 1 or in_planes != planes:
            self.norm3 = norm_layer(planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, 1, stride=stride), self.norm3)

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)


class StandinPredictor(nn.Module):
    """Two heads of the predictor's shape: Conv2d -> nn.GroupNorm -> GELU -> blocks (-> Conv2d); `bare` builds the ablation's
    single Conv2d in place of refine_unet."""

    def __init__(self, channels=16, bare=False):
        super().__init__()
        self.corr_refine_net = nn.Sequential(nn.Conv2d(5, channels, 3, 1, 1), nn.GroupNorm(8, channels), nn.GELU(),
                                             nn.Sequential(StandinResBlock(channels)), nn.Conv2d(channels, 4, 3, 1, 1))
        self.refine_unet = nn.Conv2d(5, channels, 3, 1, 1) if bare else nn.Sequential(
            nn.Conv2d(5, channels, 3, 1, 1), nn.GroupNorm(4, channels), nn.GELU(), nn.Sequential(StandinResBlock(channels)))


def standin_modules(unet_name, predictor_name, backbone_name):
    """{module name: stand-in module} for the three modules install(group_norm=True) patches."""
    unet, predictor, backbone = (types.ModuleType(n) for n in (unet_name, predictor_name, backbone_name))
    for mod, classes in ((unet, {"ResBlock": StandinResBlock, "AttentionBlock": StandinAttentionBlock}),
                         (predictor, {"DepthPredictorMultiView360": StandinPredictor}), (backbone, {"ResidualBlock": StandinResidualBlock})):
        for name, base in classes.items():
            setattr(mod, name, type(name, (base,), {"__module__": mod.__name__}))   # a fresh class per module: patches do not leak
    return {unet_name: unet, predictor_name: predictor, backbone_name: backbone}


def randomise(module, seed):
    """Every parameter of `module` from the integer lattice, keyed by its state_dict name (no zero initialisation left; buffers stay); norm
    weights around 1."""
    with torch.no_grad():
        for key, p in module.named_parameters():
            val = torch.from_numpy(lattice(tuple(p.shape), 100 * seed + zlib.crc32(key.encode()) % 97, scale=1.0 / 128.0 if p.dim() > 1 else 1.0 / 32.0))
            if p.dim() == 1 and key.endswith("weight"):
                val = val + 1.0
            p.copy_(val.to(p.dtype))
    return module
