"""The encoder's normalise-then-activate pair on the GPU, forward and backward (csrc/s360_group_norm.hip).

The reference's two U-Nets (src/model/encoder/costvolume/ldm_unet/unet.py: postnorm ResBlock :217-222, :249-256, :307, postnorm
AttentionBlock :370-380), the two heads in front of them (depth_predictor_multiview_360.py:425-427, :480-482) and the CNN
backbones' ResidualBlock (backbone/unimatch/backbone.py:28-36) run conv -> GroupNorm / InstanceNorm2d -> SiLU / GELU / ReLU
(-> + skip) as a statistics pass, an apply pass, an activation pass and an add, and autograd keeps the norm's input AND the
activation's input.  `group_norm_act` is the same function as two launches forward and at most three backward; its autograd node
saves x, weight, bias and one float64 (mean, 1 / std) pair per slab — not out, not the activation's input, not the residual.
`FusedGroupNormAct` is an nn.GroupNorm that carries its activation, `fuse_pairs` puts it in place of the (norm, activation)
pairs of every nn.Sequential below a module without touching state_dict keys, and plugin.install(group_norm=True) wires the four
sites.  Contiguous float32 GPU tensors; there is no CPU path for the direct functions (the module and the installed seam keep
torch's own code for everything else).  Forward and backward are bit-identical from run to run: fixed order, no atomics.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._call import _check_cuda_f32, call, ptr

ROW_CHUNK = 4096                                              # GN_ROW_CHUNK of the kernels: floats of one (n, c) row per workgroup
ACTIVATIONS = {"none": _lib.GN_ACT_NONE, "relu": _lib.GN_ACT_RELU, "silu": _lib.GN_ACT_SILU, "gelu": _lib.GN_ACT_GELU}


def _act(activation: str) -> int:
    if activation not in ACTIVATIONS:
        raise ValueError(f"group_norm_act knows the activations {sorted(ACTIVATIONS)}, got activation={activation!r}")
    return ACTIVATIONS[activation]


def supported(x, weight=None, bias=None, residual=None) -> bool:
    """True if the kernels take the call: x a contiguous float32 GPU tensor [N, C, *] with elements, weight / bias / residual
    (where given) the same on the same device.  Reads devices, dtypes, shapes and strides only."""
    ts = [t for t in (x, weight, bias, residual) if t is not None]
    if not all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device for t in ts):
        return False
    return x.dim() >= 2 and x.numel() > 0


def _checked(what: str, x: Tensor, num_groups: int, weight, bias, eps: float, residual=None) -> tuple:
    """Checks of a call; returns (N, C, S)."""
    for name, t in (("x", x), ("weight", weight), ("bias", bias), ("residual", residual)):
        if t is not None and not isinstance(t, Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if x is None or x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"{what} expects x [N, C, *] with elements")
    n, c = int(x.shape[0]), int(x.shape[1])
    if not isinstance(num_groups, int) or isinstance(num_groups, bool) or num_groups < 1 or c % num_groups:
        raise ValueError(f"{what}: num_groups = {num_groups!r} must be a positive divisor of the {c} channels")
    if (weight is None) != (bias is None):
        raise ValueError(f"{what} takes weight and bias together or neither")
    if weight is not None and (tuple(weight.shape) != (c,) or tuple(bias.shape) != (c,)):
        raise ValueError(f"{what}: weight and bias must be [{c}], got {tuple(weight.shape)} and {tuple(bias.shape)}")
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError(f"{what}: residual {tuple(residual.shape)} must have x's shape {tuple(x.shape)}")
    if not float(eps) > 0.0:
        raise ValueError(f"{what}: eps must be positive, got {eps!r}")
    if not supported(x, weight, bias, residual):
        raise ValueError(f"{what} takes contiguous float32 GPU tensors on one device (no CPU path); got x {x.dtype} on {x.device}, "
                         f"contiguous={x.is_contiguous()}")
    _check_cuda_f32(what, *[t for t in (x, weight, bias, residual) if t is not None])
    return n, c, x.numel() // (n * c)


def scratch_doubles(n: int, c: int, s: int) -> int:
    """s360_group_norm_scratch_doubles: the float64 scratch of one forward or backward call."""
    return int(_lib.lib().s360_group_norm_scratch_doubles(int(n), int(c), int(s)))


def norm_forward(x: Tensor, num_groups: int, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, eps: float = 1e-5,
                 activation: str = "none", residual: Optional[Tensor] = None) -> tuple:
    """s360_group_norm_forward -> (out in x's shape float32, stats [N * G, 2] float64 = (mean, 1 / sqrt(var + eps)) per slab)."""
    act = _act(activation)
    n, c, s = _checked("norm_forward", x, num_groups, weight, bias, eps, residual)
    x, weight, bias, residual = (None if t is None else t.detach() for t in (x, weight, bias, residual))
    out = torch.empty_like(x)
    stats = torch.empty(n * num_groups, 2, dtype=torch.float64, device=x.device)
    scratch = torch.empty(scratch_doubles(n, c, s), dtype=torch.float64, device=x.device)
    call("s360_group_norm_forward", x.device, ptr(x), ptr(weight), ptr(bias), ptr(residual), n, c, s, num_groups, C.byref(C.c_double(float(eps))), act,
         ptr(scratch), ptr(stats), ptr(out))
    return out, stats


def norm_backward(x: Tensor, num_groups: int, weight: Optional[Tensor], bias: Optional[Tensor], stats: Tensor, g_out: Tensor,
                  eps: float = 1e-5, activation: str = "none", needs=(True, True, True)) -> tuple:
    """s360_group_norm_backward -> (g_x, g_weight, g_bias), None where `needs` is False (or there is no weight)."""
    act = _act(activation)
    n, c, s = _checked("norm_backward", x, num_groups, weight, bias, eps)
    if not supported(x, g_out) or tuple(g_out.shape) != tuple(x.shape):
        raise ValueError(f"norm_backward: g_out must be a contiguous float32 GPU tensor of x's shape {tuple(x.shape)}")
    if (not isinstance(stats, Tensor) or stats.dtype != torch.float64 or tuple(stats.shape) != (n * num_groups, 2) or stats.device != x.device
            or not stats.is_contiguous()):
        raise ValueError("norm_backward: stats must be the forward's float64 [N * G, 2] tensor")
    x, weight, bias, stats, g_out = (None if t is None else t.detach() for t in (x, weight, bias, stats, g_out))
    want_x, want_w, want_b = (bool(v) for v in needs)
    g_x = torch.empty_like(x) if want_x else None
    g_w = torch.empty_like(weight) if want_w and weight is not None else None
    g_b = torch.empty_like(bias) if want_b and bias is not None else None
    if g_x is None and g_w is None and g_b is None:
        return None, None, None
    scratch = torch.empty(scratch_doubles(n, c, s), dtype=torch.float64, device=x.device)
    call("s360_group_norm_backward", x.device, ptr(x), ptr(weight), ptr(bias), ptr(stats), ptr(g_out), n, c, s, num_groups,
         C.byref(C.c_double(float(eps))), act, ptr(scratch), ptr(g_x), ptr(g_w), ptr(g_b))
    return g_x, g_w, g_b


class _GroupNormAct(torch.autograd.Function):
    """out of (x, weight, bias, residual); saves x, weight, bias and the per-slab stats — nothing else of x's size."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, num_groups, eps, activation):
        out, stats = norm_forward(x, num_groups, weight, bias, eps, activation, residual)
        ctx.save_for_backward(x.detach(), None if weight is None else weight.detach(), None if bias is None else bias.detach(), stats)
        ctx.opts = (num_groups, eps, activation)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        x, weight, bias, stats = ctx.saved_tensors
        num_groups, eps, activation = ctx.opts
        g_out = g_out.to(torch.float32).contiguous()
        need = ctx.needs_input_grad
        g_x, g_w, g_b = norm_backward(x, num_groups, weight, bias, stats, g_out, eps, activation, needs=tuple(need[:3]))
        return g_x, g_w, g_b, (g_out if need[3] else None), None, None, None


def group_norm_act(x: Tensor, num_groups: int, weight: Optional[Tensor] = None, bias: Optional[Tensor] = None, eps: float = 1e-5,
                   activation: str = "none", residual: Optional[Tensor] = None) -> Tensor:
    """residual + a(group_norm(x, num_groups, weight, bias, eps)) as one fused operator.

    x [N, C, *]; the statistics of a group are its mean and biased variance over C / num_groups channels and all trailing
    dims, as F.group_norm's; weight and bias [C] come together or not at all; activation is "none", "relu", "silu" or "gelu"
    (the erf form); residual has x's shape.  Differentiable (once) in x, weight, bias and residual; the node keeps x and one
    float64 pair per group.  Contiguous float32 GPU tensors, else ValueError: there is no CPU path."""
    _act(activation)
    _checked("group_norm_act", x, num_groups, weight, bias, eps, residual)
    return _GroupNormAct.apply(x, weight, bias, residual, int(num_groups), float(eps), activation)


def instance_norm_act(x: Tensor, activation: str = "relu", eps: float = 1e-5) -> Tensor:
    """a(instance_norm(x)) without affine and without running statistics (nn.InstanceNorm2d's defaults): a group norm with one
    channel per group."""
    if not isinstance(x, Tensor) or x.dim() < 2:
        raise ValueError("instance_norm_act expects x [N, C, *]")
    return group_norm_act(x, int(x.shape[1]), None, None, eps, activation)


_TORCH_ACT = {"none": lambda t: t, "relu": F.relu, "silu": F.silu, "gelu": F.gelu}


def activation_of(module) -> Optional[str]:
    """The activation name of a module the kernels can fuse behind a norm: nn.SiLU, nn.ReLU, nn.GELU in the erf form; else None."""
    if isinstance(module, nn.SiLU):
        return "silu"
    if isinstance(module, nn.ReLU):
        return "relu"
    if isinstance(module, nn.GELU) and getattr(module, "approximate", "none") == "none":
        return "gelu"
    return None


class FusedGroupNormAct(nn.GroupNorm):
    """An nn.GroupNorm that applies `activation` to its result: the fused kernels for a contiguous float32 GPU input (and
    parameters), F.group_norm and the torch activation otherwise (CPU, float64, non-contiguous inputs, double backward).
    Parameters, buffers and state_dict keys are nn.GroupNorm's."""

    def __init__(self, num_groups: int, num_channels: int, eps: float = 1e-5, affine: bool = True, activation: str = "none", **kw):
        super().__init__(num_groups, num_channels, eps=eps, affine=affine, **kw)
        _act(activation)
        self.activation = activation

    @classmethod
    def from_norm(cls, norm: nn.GroupNorm, activation: str) -> "FusedGroupNormAct":
        """A module of `norm`'s configuration that SHARES its weight and bias Parameter objects."""
        new = cls(norm.num_groups, norm.num_channels, eps=norm.eps, affine=False, activation=activation)
        new.affine = norm.affine
        new.weight, new.bias = norm.weight, norm.bias
        new.train(norm.training)
        return new

    def forward(self, x: Tensor, residual: Optional[Tensor] = None) -> Tensor:
        if supported(x, self.weight, self.bias, residual) and x.shape[1] == self.num_channels:
            return group_norm_act(x, self.num_groups, self.weight, self.bias, self.eps, self.activation, residual)
        y = _TORCH_ACT[self.activation](F.group_norm(x, self.num_groups, self.weight, self.bias, self.eps))
        return y if residual is None else residual + y

    def extra_repr(self) -> str:
        return super().extra_repr() + f", activation={self.activation}"


def norm_act(norm: nn.Module, x: Tensor, activation: str, residual: Optional[Tensor] = None) -> Tensor:
    """residual + a(norm(x)) for a module `norm` that is an nn.GroupNorm (or subclass) or an nn.InstanceNorm2d without affine and
    running statistics: the fused kernels when `supported`, else the module's own forward, the torch activation and the add.
    What the installed seams call (plugin.install(group_norm=True))."""
    _act(activation)
    if isinstance(norm, FusedGroupNormAct) and norm.activation != "none":
        if norm.activation != activation:
            raise ValueError(f"norm_act: the module already applies {norm.activation!r}, asked for {activation!r}")
        return norm(x, residual)
    if isinstance(norm, nn.GroupNorm):
        groups, weight, bias = norm.num_groups, norm.weight, norm.bias
    elif isinstance(norm, nn.modules.instancenorm._InstanceNorm) and not norm.affine and not norm.track_running_stats:
        groups, weight, bias = (int(x.shape[1]) if x.dim() >= 2 else 0), None, None
    else:
        raise ValueError(f"norm_act takes an nn.GroupNorm or a plain nn.InstanceNorm, got {type(norm).__name__}")
    if supported(x, weight, bias, residual) and groups >= 1 and x.shape[1] % groups == 0:
        return group_norm_act(x, groups, weight, bias, norm.eps, activation, residual)
    if isinstance(norm, FusedGroupNormAct):
        y = _TORCH_ACT[activation](F.group_norm(x, groups, weight, bias, norm.eps))
    else:
        y = _TORCH_ACT[activation](norm(x))
    return y if residual is None else residual + y


def fuse_pairs(module: nn.Module) -> nn.Module:
    """In every nn.Sequential at or below `module`, replace an nn.GroupNorm (or subclass) that is directly followed by nn.SiLU,
    nn.GELU (erf) or nn.ReLU AT ITS OWN INDEX by a FusedGroupNormAct sharing the same Parameter objects, and the activation by
    nn.Identity(): state_dict keys, parameter identities and module indices do not change, so checkpoints load unchanged.  In
    place and idempotent; returns `module`."""
    for seq in [m for m in module.modules() if isinstance(m, nn.Sequential)]:
        keys = list(seq._modules.keys())
        for here, after in zip(keys, keys[1:]):
            norm, act = seq._modules[here], activation_of(seq._modules[after])
            if not isinstance(norm, nn.GroupNorm) or act is None:
                continue
            if isinstance(norm, FusedGroupNormAct):
                if norm.activation != "none":
                    continue                                   # a fused pair followed by a further activation: leave it alone
                norm.activation = act
            else:
                seq._modules[here] = FusedGroupNormAct.from_norm(norm, act)
            seq._modules[after] = nn.Identity()
    return module
