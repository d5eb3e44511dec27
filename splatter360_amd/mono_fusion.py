"""The mono-feature fusion of the cost-volume encoder on the GPU, forward and backward (csrc/s360_mono_fusion.hip).

With add_mono_feat the reference's EncoderCostVolume.forward (src/model/encoder/encoder_costvolume.py) runs

    features_mono = self.c2e(features_mono)                                   # :297, under torch.no_grad(): [(b v), Cm, h, w]
    trans_features = torch.cat([trans_features, features_mono], dim=1)        # :351                         [(b v), C + Cm, h, w]
    trans_features = self.rgbd_fusion(rearrange(trans_features, "bv c h w -> bv h w c"))     # :353
    trans_features = rearrange(trans_features, "bv h w c -> bv c h w")        # :354

with rgbd_fusion = Sequential(Linear(C + Cm, C, bias=False), LayerNorm(C), ReLU(), Linear(C, C, bias=False)) (:119-125).  Torch
writes the stitched map, the concatenation (kept by autograd for the first Linear's weight gradient), its channel-last copy and three
[T, C] activations.  `mono_fusion` computes the same function from the cube faces themselves: the 8-tap float32 stitch is taken
inside the kernel, once per token for all Cm channels, so neither the stitched map nor the concatenation exists, forward or backward.
The autograd node saves the inputs, the first Linear's output y [T, C] and one float64 (mean, rstd) pair per token.  The 384 (768,
1024) mono channels are a constant: they take no gradient, and asking for one is an error.  The firm gain is memory; speed against
torch is what profiles/mono_fusion_timing.json says it is.  Float32 GPU tensors, C = 128 and Cm a multiple of 64 in 64 .. 1024 (the
three vit_types give 384, 768, 1024); there is no CPU path.  Forward and backward are bit-identical from run to run: fixed order, no
atomics.

precision="highest" (the default) forms every product from exact float32 products; precision="high" is what
torch.set_float32_matmul_precision('high') asks for: each float32 number as the sum of two bfloat16 numbers and each of the two
products of the forward and the four of the backward as Ah Bh + Ah Bl + Al Bh on the bf16 MFMA, float32 accumulation (the stitch
stays the float32 8-tap stitch, the LayerNorm rows float64).  The two weights are split once per call into bf16 planes in a scratch
buffer (under 1 MiB, whatever the token count); the token side is split inside the kernels, so the "high" mode saves what
"highest" saves.  A forward run in one precision takes its backward in the same one.  `precision.resolve("torch")` reads torch's
setting at call time.

`install(mono_fusion=True)` (plugin.py) reaches these kernels from the unchanged reference: `MonoStitchHandle` is what the wrapped
`c2e` returns for the no-grad mono stitch — a torch.Tensor wrapper subclass built like lazy.LazyField, metadata and no data — and
`FusedMonoFusion` is the rgbd_fusion that recognises it.
"""
from __future__ import annotations

import ctypes as C
import types
from typing import Optional

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import precision as _prec
from ._args import buffers as _buffers, eps as _eps, flat as _flat, high_scratch as _high_scratch, no_scratch as _no_scratch, \
    positive_int as _positive, tensor_rule
from ._call import call, ptr
from .precision import PRECISIONS  # noqa: F401  (the name callers of this module use)

CHANNELS = 128
MONO_STEP, MONO_MAX = 64, 1024
FORWARD_OUTPUTS = ("out", "y", "stats")
GRADIENTS = ("g_erp_feat", "g_w1", "g_ln_weight", "g_ln_bias", "g_w2")
_tensor = tensor_rule(RuntimeError, "{what} runs on the GPU only (there is no CPU path): {name} is on {device}")


def supported_widths(channels: int, mono_channels: int) -> bool:
    """channels == 128 and mono_channels a multiple of 64 in 64 .. 1024."""
    return int(channels) == CHANNELS and MONO_STEP <= int(mono_channels) <= MONO_MAX and int(mono_channels) % MONO_STEP == 0


def scratch_bytes(tokens: int, mono_channels: int, backward: bool = True, precision: str = "highest") -> int:
    """The bytes of scratch a backward (forward, with backward=False) call allocates for `tokens` tokens and `mono_channels` mono
    channels: "highest" s360_mono_fusion_scratch_bytes for the backward and none for the forward; "high"
    s360_mono_fusion_high_scratch_bytes, the same plus the weights' bf16 planes, whose size does not depend on tokens."""
    _prec.check("mono_fusion", precision)
    _positive("scratch_bytes", "tokens", tokens)
    if not supported_widths(CHANNELS, mono_channels):
        raise ValueError(f"scratch_bytes: mono_channels must be a multiple of {MONO_STEP} in {MONO_STEP} .. {MONO_MAX}, got {mono_channels!r}")
    if precision == "high":
        return int(_lib.lib().s360_mono_fusion_high_scratch_bytes(tokens, int(mono_channels), int(bool(backward))))
    return int(_lib.lib().s360_mono_fusion_scratch_bytes(tokens, int(mono_channels))) if backward else 0


def weight_chunks(tokens: int) -> int:
    """How many token chunks the weight-gradient pass of the backward uses for `tokens` tokens: min(32, ceil(tokens / 64))."""
    return int(_lib.lib().s360_mono_fusion_weight_chunks(_positive("weight_chunks", "tokens", tokens)))


def _checked(what: str, erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps) -> tuple:
    """(n, mono_channels, face_w, equ_h, equ_w) of a call the kernels take; raises otherwise."""
    _tensor(what, "erp_feat", erp_feat)
    dev = erp_feat.device
    _tensor(what, "mono_cube", mono_cube, device=dev)
    if erp_feat.dim() != 4 or mono_cube.dim() != 4:
        raise ValueError(f"{what} takes erp_feat [N, C, H, W] and mono_cube [N, Cm, fw, 6 fw], got {tuple(erp_feat.shape)} and {tuple(mono_cube.shape)}")
    n, c, h, w = (int(x) for x in erp_feat.shape)
    nm, cm, fw, fw6 = (int(x) for x in mono_cube.shape)
    if not supported_widths(c, cm):
        raise ValueError(f"{what}: unsupported widths C = {c}, Cm = {cm}: the kernels take C = {CHANNELS} and Cm a multiple of {MONO_STEP} in "
                         f"{MONO_STEP} .. {MONO_MAX}")
    if min(n, h, w, fw) < 1 or nm != n or fw6 != 6 * fw:
        raise ValueError(f"{what}: mono_cube must be [{n}, Cm, fw, 6 fw] (six faces side by side), got {tuple(mono_cube.shape)}")
    _tensor(what, "grid", grid, (h, w, 3), device=dev)
    _tensor(what, "w1", w1, (c, c + cm), device=dev)
    _tensor(what, "w2", w2, (c, c), device=dev)
    _tensor(what, "ln_weight", ln_weight, (c,), device=dev)
    _tensor(what, "ln_bias", ln_bias, (c,), device=dev)
    _eps(what, eps)
    return n, cm, fw, h, w


def mono_fusion_forward(erp_feat: Tensor, mono_cube: Tensor, grid: Tensor, w1: Tensor, ln_weight: Tensor, ln_bias: Tensor, w2: Tensor,
                        eps: float = 1e-5, *, buffers: Optional[dict] = None, precision: str = "highest",
                        scratch: Optional[Tensor] = None) -> tuple:
    """s360_mono_fusion_forward (precision "high": s360_mono_fusion_high_forward) -> (out [N, C, H, W], y [T, C] float32, stats
    [T, 2] float64), T = N H W.  `buffers`: {name: buffer} for any of FORWARD_OUTPUTS to write into; the others are allocated.
    `scratch`: a uint8 buffer of scratch_bytes(T, Cm, False, "high") bytes for the "high" call to use in place of one it
    allocates; refused (ValueError) with any other precision, whose forward has no scratch."""
    _prec.check("mono_fusion", precision)
    _no_scratch("mono_fusion_forward", precision, scratch)
    n, cm, fw, h, w = _checked("mono_fusion_forward", erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps)
    args = [_flat(t) for t in (erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2)]
    dev, tokens = erp_feat.device, n * h * w
    out, y, stats = _buffers("mono_fusion_forward", FORWARD_OUTPUTS, ((n, CHANNELS, h, w), (tokens, CHANNELS), (tokens, 2)),
                             (torch.float32, torch.float32, torch.float64), dev, buffers, _tensor)
    common = (*(ptr(t) for t in args), n, CHANNELS, cm, fw, h, w, C.byref(C.c_double(float(eps))), ptr(out), ptr(y), ptr(stats))
    if precision == "high":
        scratch = _high_scratch("mono_fusion_forward", scratch_bytes(tokens, cm, False, "high"), dev, scratch, _tensor)
        call("s360_mono_fusion_high_forward", dev, *common, ptr(scratch), scratch.numel())
    else:
        call("s360_mono_fusion_forward", dev, *common)
    return out, y, stats


def mono_fusion_backward(erp_feat: Tensor, mono_cube: Tensor, grid: Tensor, w1: Tensor, ln_weight: Tensor, ln_bias: Tensor, w2: Tensor,
                         y: Tensor, stats: Tensor, g_out: Tensor, eps: float = 1e-5, *, buffers: Optional[dict] = None,
                         precision: str = "highest", scratch: Optional[Tensor] = None) -> tuple:
    """s360_mono_fusion_backward (precision "high": s360_mono_fusion_high_backward, with y and stats of a "high" forward) -> the
    gradients in GRADIENTS' order (g_erp_feat, g_w1, g_ln_weight, g_ln_bias, g_w2).  `buffers`: {name: contiguous float32 buffer of
    the right shape} for any of them to write into (every element is written); the others and the scratch (scratch_bytes) are
    allocated.  `scratch`: as in mono_fusion_forward, scratch_bytes(T, Cm, True, "high") bytes, refused with any other precision
    (the "highest" backward allocates its own)."""
    what = "mono_fusion_backward"
    _prec.check("mono_fusion", precision)
    _no_scratch(what, precision, scratch)
    n, cm, fw, h, w = _checked(what, erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps)
    dev, tokens = erp_feat.device, n * h * w
    _tensor(what, "g_out", g_out, erp_feat.shape, device=dev)
    _tensor(what, "y", y, (tokens, CHANNELS), device=dev)
    _tensor(what, "stats", stats, (tokens, 2), dtype=torch.float64, device=dev)
    ins = [_flat(t) for t in (erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, y, stats, g_out)]
    outs = _buffers(what, GRADIENTS, [t.shape for t in (erp_feat, w1, ln_weight, ln_bias, w2)], [torch.float32] * 5, dev, buffers, _tensor)
    nbytes = scratch_bytes(tokens, cm, True, precision)
    scratch = _high_scratch(what, nbytes, dev, scratch, _tensor) if precision == "high" else _prec.scratch(nbytes, dev)
    call("s360_mono_fusion_high_backward" if precision == "high" else "s360_mono_fusion_backward", dev, *(ptr(t) for t in ins), n, CHANNELS, cm, fw, h, w, C.byref(C.c_double(float(eps))), ptr(scratch),
         scratch.numel(), *(ptr(t) for t in outs))
    return tuple(outs)


class _MonoFusion(torch.autograd.Function):
    """Saves the inputs, y [T, C] and the statistics: nothing of Cm or C + Cm channels per token and, in the "high" mode, none of
    the bf16 planes (the backward splits the weights again)."""

    @staticmethod
    def forward(ctx, erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps, precision):
        args = [_flat(t) for t in (erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2)]
        out, y, stats = mono_fusion_forward(*args, eps, precision=precision)
        ctx.save_for_backward(*args, y, stats)
        ctx.eps, ctx.precision = eps, precision
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        *args, y, stats = ctx.saved_tensors
        g_erp, g_w1, g_lnw, g_lnb, g_w2 = mono_fusion_backward(*args, y, stats, g_out.to(torch.float32), ctx.eps, precision=ctx.precision)
        return g_erp, None, None, g_w1, g_lnw, g_lnb, g_w2, None, None


def mono_fusion(erp_feat: Tensor, mono_cube: Tensor, grid: Tensor, w1: Tensor, ln_weight: Tensor, ln_bias: Tensor, w2: Tensor,
                eps: float = 1e-5, precision: str = "highest") -> Tensor:
    """relu(LN(cat([erp_feat, Cube2Equirec(mono_cube)], 1) w1^T)) w2^T over the channels -> out [N, C, H, W] (dense NCHW): the
    reference's encoder_costvolume.py:297 and :351-354.

    erp_feat [N, C, H, W]; mono_cube [N, Cm, fw, 6 fw], the six faces side by side in slot order F R B L U D (what
    Cube2Equirec.forward receives); grid [H, W, 3] = Cube2Equirec.sample_grid[0, 0] (stitch.sample_grid_numpy); w1 [C, C + Cm] and
    w2 [C, C] in nn.Linear's layout, no biases; ln_weight, ln_bias [C] (nn.LayerNorm's affine parameters, biased variance, eps).
    Differentiable (once) in erp_feat and the four parameters.  mono_cube is a constant: a mono_cube that requires a gradient is a
    RuntimeError (the reference stitches it under torch.no_grad()).  Float32 GPU tensors, C = 128, Cm a multiple of 64 in
    64 .. 1024; no CPU path; a non-contiguous input is copied once.  precision "highest": exact float32 products; "high": bf16x3
    products on the bf16 MFMA, forward and backward (the module's docstring)."""
    _prec.check("mono_fusion", precision)
    _checked("mono_fusion", erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, eps)
    if mono_cube.requires_grad:
        raise RuntimeError("mono_fusion: mono_cube requires a gradient, but the mono features are a constant of the fused kernels (the "
                           "reference stitches them under torch.no_grad()): detach it, or use the modules' own forward")
    return _MonoFusion.apply(erp_feat, mono_cube, grid, w1, ln_weight, ln_bias, w2, float(eps), precision)


# ------------------------------------------------------------------------------------------------ the seam's two halves
_METADATA = {"size", "dim", "numel", "nelement", "ndimension", "is_floating_point", "is_complex", "element_size", "get_device", "__len__",
             "__repr__", "__str__", "__format__", "__hash__", "is_shared", "is_pinned", "is_leaf", "_is_view", "type", "is_inference",
             "is_same_size"}
_CHANNELS_LAST = (0, 2, 3, 1)


class MonoStitchHandle(torch.Tensor):
    """The no-grad mono stitch that has not been computed: metadata, the stitch module and its input, no data.

    Three states, each with the shape, dtype and device of the tensor it stands for: the stitch c2e(cube) [N, Cm, H, W]; after
    torch.cat([tensor, handle], dim=1) the concatenation [N, C + Cm, H, W] (it keeps `tensor`); after permute(0, 2, 3, 1) of that
    its channel-last view [N, H, W, C + Cm] — the three statements the reference runs between c2e and rgbd_fusion.  Same-shape
    reshapes and metadata queries keep it as it is.  Any other operation first materialises it — the stitch by the module's own
    forward under no_grad, then torch's cat and permute — and runs on the real tensor."""

    @staticmethod
    def __new__(cls, c2e, cube: Tensor, erp: Optional[Tensor] = None, last: bool = False, stitch=None):
        n, cm = int(cube.shape[0]), int(cube.shape[1])
        h, w = int(c2e.equ_h), int(c2e.equ_w)
        ch = cm + (0 if erp is None else int(erp.shape[1]))
        shape = (n, h, w, ch) if last else (n, ch, h, w)
        t = torch.Tensor._make_wrapper_subclass(cls, shape, dtype=cube.dtype, device=cube.device, requires_grad=False)
        t._s360_c2e, t._s360_cube, t._s360_erp, t._s360_last = c2e, cube, erp, bool(last)
        t._s360_stitch = stitch if stitch is not None else c2e.forward
        return t

    @property
    def fusable(self) -> bool:
        """The state rgbd_fusion receives: the channel-last concatenation."""
        return self._s360_erp is not None and self._s360_last

    def materialise(self) -> Tensor:
        """The real tensor this handle stands for, with the reference's values."""
        with torch.no_grad():
            x = self._s360_stitch(self._s360_cube)
        if self._s360_erp is not None:
            x = torch.cat([self._s360_erp, x], dim=1)
        return x.permute(*_CHANNELS_LAST) if self._s360_last else x

    def __repr__(self):   # never materialise for a debugger's sake
        return f"MonoStitchHandle(shape={tuple(self.shape)}, device={self.device}, fusable={self.fusable})"

    def _cat(self, tensors, dim) -> Optional["MonoStitchHandle"]:
        """The handle of torch.cat([tensor, handle], dim=1), or None when the call is anything else."""
        if not isinstance(tensors, (list, tuple)) or len(tensors) != 2 or tensors[1] is not self or isinstance(tensors[0], MonoStitchHandle):
            return None
        e = tensors[0]
        if self._s360_erp is not None or self._s360_last or not isinstance(e, Tensor) or e.dim() != 4 or not isinstance(dim, int) or dim % 4 != 1:
            return None
        if e.dtype != self.dtype or e.device != self.device or (e.shape[0], e.shape[2], e.shape[3]) != (self.shape[0], self.shape[2], self.shape[3]):
            return None
        return MonoStitchHandle(self._s360_c2e, self._s360_cube, e, False, self._s360_stitch)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        me = args[0] if args and isinstance(args[0], MonoStitchHandle) else None
        if name == "__get__" or name in _METADATA:
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)
        if name == "cat" and args:
            dim = args[1] if len(args) > 1 else kwargs.get("dim", 0)
            hs = [t for t in args[0] if isinstance(t, MonoStitchHandle)] if isinstance(args[0], (list, tuple)) else []
            out = hs[0]._cat(args[0], dim) if len(hs) == 1 else None
            if out is not None:
                return out
        if me is not None and name == "permute":
            dims = args[1] if len(args) == 2 and isinstance(args[1], (list, tuple)) else args[1:]
            try:
                dims = tuple(int(d) % 4 for d in dims)
            except Exception:
                dims = None
            if dims == (0, 1, 2, 3):
                return me
            if dims == _CHANNELS_LAST and me._s360_erp is not None and not me._s360_last:
                return MonoStitchHandle(me._s360_c2e, me._s360_cube, me._s360_erp, True, me._s360_stitch)
        if me is not None and name in ("reshape", "view") and not any(isinstance(a, MonoStitchHandle) for a in args[1:]):
            shape = args[1] if len(args) == 2 and isinstance(args[1], (list, tuple, torch.Size)) else args[1:]
            try:
                if tuple(int(s) for s in shape) == tuple(me.shape):
                    return me
            except Exception:
                pass
        # anything else: compute on the real tensors
        real = lambda a: a.materialise() if isinstance(a, MonoStitchHandle) else a
        deep = lambda a: type(a)(deep(x) for x in a) if isinstance(a, (list, tuple)) else real(a)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*deep(tuple(args)), **{k: deep(v) for k, v in kwargs.items()})

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        """Whatever reaches the dispatcher without passing __torch_function__ (C++ callers): compute on the real tensors."""
        from torch.utils._pytree import tree_map
        real = lambda a: a.materialise() if isinstance(a, MonoStitchHandle) else a
        return func(*tree_map(real, tuple(args)), **tree_map(real, dict(kwargs or {})))


def _plain_layers(seq) -> bool:
    """Is `seq` the reference's rgbd_fusion: Linear (no bias), affine LayerNorm over the Linear's width, ReLU, Linear (no bias)?"""
    if not isinstance(seq, nn.Sequential) or len(seq) != 4:
        return False
    l1, ln, act, l2 = seq[0], seq[1], seq[2], seq[3]
    if not (isinstance(l1, nn.Linear) and isinstance(ln, nn.LayerNorm) and isinstance(act, nn.ReLU) and isinstance(l2, nn.Linear)):
        return False
    c = l1.out_features
    return (l1.bias is None and l2.bias is None and ln.elementwise_affine and ln.bias is not None and tuple(ln.normalized_shape) == (c,)
            and (l2.in_features, l2.out_features) == (c, c) and l1.in_features > c)


class FusedMonoFusion(nn.Sequential):
    """The reference's rgbd_fusion with its four children (state-dict keys 0.weight, 1.weight, 1.bias, 3.weight).  Handed the
    channel-last MonoStitchHandle of the installed seam it runs `mono_fusion` on what the handle holds and returns
    out.permute(0, 2, 3, 1), so that the reference's rearrange back to "bv c h w" yields a dense NCHW tensor; any other input runs
    nn.Sequential.forward on the real tensor.  `precision`: "highest" (the default), "high" or "torch", the precision of
    mono_fusion's products, resolved by precision.resolve at every call ("torch": torch.get_float32_matmul_precision() then); the
    installed seam stamps it with its mono_fusion_precision option."""

    precision = "highest"

    @classmethod
    def from_sequential(cls, seq: nn.Sequential) -> "FusedMonoFusion":
        """The same child modules (the same Parameter objects) in a FusedMonoFusion."""
        return cls(*list(seq.children()))

    def forward(self, x):
        if isinstance(x, MonoStitchHandle):
            grid = getattr(x._s360_c2e, "sample_grid", None)
            if (x.fusable and x.is_cuda and x.dtype == torch.float32 and _plain_layers(self) and isinstance(grid, Tensor) and grid.dim() == 5
                    and supported_widths(self[0].out_features, self[0].in_features - self[0].out_features)
                    and int(x._s360_erp.shape[1]) == self[0].out_features and grid.device == x.device):
                out = mono_fusion(x._s360_erp, x._s360_cube, grid.detach()[0, 0], self[0].weight, self[1].weight, self[1].bias, self[3].weight,
                                  float(self[1].eps), precision=_prec.resolve(self.precision))
                return out.permute(*_CHANNELS_LAST)
            x = x.materialise()
        return super().forward(x)


def wrap_stitch(c2e: nn.Module, fusion: nn.Sequential) -> None:
    """Rebind `c2e.forward` on the instance (its parameters and state-dict keys stay): a call with grad disabled on a 4-D float32
    GPU tensor of in_features - out_features channels of `fusion`'s first Linear, at widths the kernels take, returns a
    MonoStitchHandle; every other call runs the module's own forward and returns its bits.  Idempotent."""
    if getattr(c2e.forward, "replaced", None) is not None:
        return
    own = c2e.forward

    def forward(self, cube_feat):
        l1 = fusion[0] if isinstance(fusion, nn.Sequential) and len(fusion) else None
        if (isinstance(l1, nn.Linear) and not torch.is_grad_enabled() and isinstance(cube_feat, Tensor) and not isinstance(cube_feat, MonoStitchHandle)
                and cube_feat.dim() == 4 and cube_feat.is_cuda and cube_feat.dtype == torch.float32
                and int(cube_feat.shape[1]) == l1.in_features - l1.out_features and supported_widths(l1.out_features, int(cube_feat.shape[1]))
                and int(cube_feat.shape[2]) == int(self.face_w) and int(cube_feat.shape[3]) == 6 * int(self.face_w) and _plain_layers(fusion)):
            return MonoStitchHandle(self, cube_feat, stitch=own)
        return own(cube_feat)

    forward.replaced = own
    c2e.forward = types.MethodType(forward, c2e)
