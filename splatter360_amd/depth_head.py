"""The encoder's softmax depth head on the GPU, forward and backward (csrc/s360_depth_head.hip).

After the refinement U-Net the reference's predictor (src/model/encoder/costvolume/depth_predictor_multiview_360.py:643-651) turns
its [v b, D, h, w] logits into the two maps every later stage consumes,

    pdf = softmax(logits, dim=1);  coarse_depths = (depth_candi_curr * pdf).sum(1, keepdim=True);  pdf_max = max(pdf, dim=1, keepdim=True)[0]

`softmax_depth_head` computes both in one fused reduction over D that never stores the softmax, and its gradient in one
elementwise kernel from three saved per-pixel scalars; `coarse_depth_head` adds the reference's 1 / depth and two interpolations
(:650-658).  `LazyPdf` is what plugin.install(depth_head=True) puts in place of the softmax, so that the predictor's own three
statements run the fused kernels.  Float32 GPU tensors only; there is no CPU path (the installed seam keeps the replaced softmax
for everything else).  Forward and backward are bit-identical from run to run: fixed order, no atomics.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.autograd.function import once_differentiable

from ._call import _check_cuda_f32, call, ptr


def head_forward(logits: Tensor, candidates: Tensor) -> tuple:
    """s360_depth_head_forward on contiguous float32 GPU tensors: logits [n, D, h, w], candidates [n, D] ->
    (depth, pmax, lse [n, 1, h, w] float32, argmax [n, 1, h, w] int32)."""
    n, d, h, w = (int(s) for s in logits.shape)
    depth, pmax, lse = (torch.empty(n, 1, h, w, dtype=torch.float32, device=logits.device) for _ in range(3))
    argmax = torch.empty(n, 1, h, w, dtype=torch.int32, device=logits.device)
    call("s360_depth_head_forward", logits.device, ptr(logits), ptr(candidates), n, d, h, w, ptr(depth), ptr(pmax), ptr(lse), ptr(argmax))
    return depth, pmax, lse, argmax


def head_backward(logits: Tensor, candidates: Tensor, lse: Tensor, depth: Tensor, argmax: Tensor, g_depth, g_pmax) -> Tensor:
    """s360_depth_head_backward: g_logits [n, D, h, w] for g_depth, g_pmax [n, 1, h, w] (either may be None: zero)."""
    n, d, h, w = (int(s) for s in logits.shape)
    g_depth, g_pmax = (None if g is None else g.to(torch.float32).contiguous() for g in (g_depth, g_pmax))
    g_logits = torch.empty_like(logits)
    call("s360_depth_head_backward", logits.device, ptr(logits), ptr(candidates), ptr(lse), ptr(depth), ptr(argmax), ptr(g_depth),
         ptr(g_pmax), n, d, h, w, ptr(g_logits))
    return g_logits


class _DepthHead(torch.autograd.Function):
    """(coarse_depths, pdf_max) of the logits; gradient to the logits only.  Saves the logits, the candidates and three
    [n, 1, h, w] scalars (lse, depth, argmax), never the softmax.  `aux`, a list, receives the argmax."""

    @staticmethod
    def forward(ctx, logits, candidates, aux):
        logits = logits.detach().contiguous()
        depth, pmax, lse, argmax = head_forward(logits, candidates)
        ctx.save_for_backward(logits, candidates, lse, depth, argmax)
        ctx.set_materialize_grads(False)                        # an unused output hands None, which the kernel takes as zero
        if aux is not None:
            aux.append(argmax)
        return depth, pmax

    @staticmethod
    @once_differentiable
    def backward(ctx, g_depth, g_pmax):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        logits, candidates, lse, depth, argmax = ctx.saved_tensors
        return head_backward(logits, candidates, lse, depth, argmax, g_depth, g_pmax), None, None


def _checked(logits: Tensor, candidates: Tensor) -> Tensor:
    """The [n, D] contiguous candidates of a checked call."""
    if logits.dim() != 4:
        raise ValueError(f"softmax_depth_head expects [n, D, h, w] logits, got shape {tuple(logits.shape)}")
    _check_cuda_f32("softmax_depth_head", logits, candidates)
    n, d = int(logits.shape[0]), int(logits.shape[1])
    if tuple(candidates.shape) not in ((n, d), (n, d, 1, 1)):
        raise ValueError(f"softmax_depth_head expects candidates [n, D] or [n, D, 1, 1] for logits {tuple(logits.shape)}, got "
                         f"{tuple(candidates.shape)}")
    if logits.numel() == 0:
        raise ValueError("softmax_depth_head: empty tensors")
    return candidates.detach().reshape(n, d).contiguous()


def softmax_depth_head(logits: Tensor, candidates: Tensor) -> tuple:
    """The reference's depth head (depth_predictor_multiview_360.py:643-651): logits [n, D, h, w], candidates [n, D] or
    [n, D, 1, 1] -> (coarse_depths, pdf_max), both [n, 1, h, w],

        coarse_depths = sum_d candidates[:, d] softmax(logits, 1)[:, d],    pdf_max = max_d softmax(logits, 1)[:, d]

    in one pass over the logits; the softmax is not stored, forward or backward.  Differentiable in `logits` only (once): the
    reference builds the candidates from detached near / far.  exp, sums and quotients run in float64 and are rounded once.
    Finite logits of any size give finite results.  Float32 GPU tensors; no CPU path; non-contiguous logits are copied."""
    return _DepthHead.apply(logits, _checked(logits, candidates), None)


def coarse_depth_head(logits: Tensor, candidates: Tensor, upscale_factor) -> tuple:
    """The reference's :643-658 as one call: the native head, then 1 / depth and the two interpolations exactly as the reference
    makes them (nearest for pdf_max, bilinear with align_corners=True for the disparity; [n, 1, ., .] maps, in torch) ->
    (fullres_disps [n, 1, h s, w s], pdf_max [n, 1, h s, w s], coarse_depths [n, 1, h, w]) for s = upscale_factor."""
    coarse_depths, pdf_max = softmax_depth_head(logits, candidates)
    coarse_disps = 1 / coarse_depths
    pdf_max = F.interpolate(pdf_max, scale_factor=upscale_factor)
    fullres_disps = F.interpolate(coarse_disps, scale_factor=upscale_factor, mode="bilinear", align_corners=True)
    return fullres_disps, pdf_max, coarse_depths


def _is_dim1(dim) -> bool:
    return isinstance(dim, int) and not isinstance(dim, bool) and dim in (1, -3)


class LazyPdf:
    """What the installed `F.softmax(logits, dim=1)` returns: the logits, not their [n, D, h, w] softmax.
    `candidates * handle` (either order, candidates float32 [n, D, 1, 1] on the logits' device) gives a LazyDepthProduct whose
    `.sum(dim=1, keepdim=True)` is coarse_depths, and `torch.max(handle, dim=1, keepdim=True)` then gives (pdf_max, indices): both
    from ONE run of the fused kernel and one autograd node, cached on the handle.  Any other use, another order (max before the
    product: the candidates are not known yet) or keepdim=False goes through `dense()`: the replaced softmax, with torch's own
    autograd from there on."""

    def __init__(self, logits: Tensor, replaced):
        self.logits, self.replaced = logits, replaced
        self._dense = self._candidates = self._head = None

    @property
    def shape(self):
        return self.logits.shape

    def dense(self) -> Tensor:
        if self._dense is None:
            self._dense = self.replaced(self.logits, dim=1)
        return self._dense

    def _fusable(self, other) -> bool:
        z = self.logits
        return (self._dense is None and isinstance(other, Tensor) and other.is_cuda and other.dtype == torch.float32
                and other.device == z.device and tuple(other.shape) == (z.shape[0], z.shape[1], 1, 1)
                and (self._candidates is None or self._candidates is other))

    def _product(self, other):
        self._candidates = other
        return LazyDepthProduct(other, self)

    def head(self) -> tuple:
        """(coarse_depths, pdf_max, argmax) of the one kernel run; needs the candidates of a product formed before."""
        if self._head is None:
            aux = []
            depth, pmax = _DepthHead.apply(self.logits, _checked(self.logits, self._candidates), aux)
            self._head = (depth, pmax, aux[0])
        return self._head

    def max(self, *args, **kwargs):
        dim = args[0] if args else kwargs.get("dim")
        keepdim = args[1] if len(args) > 1 else kwargs.get("keepdim", False)
        if (self._candidates is not None and self._dense is None and _is_dim1(dim) and keepdim is True and len(args) <= 2
                and set(kwargs) <= {"dim", "keepdim"}):
            _, pmax, argmax = self.head()
            return torch.return_types.max((pmax, argmax.long()))
        return self.dense().max(*args, **kwargs)

    def __rmul__(self, other):
        return self._product(other) if self._fusable(other) else other * self.dense()

    def __mul__(self, other):
        return self._product(other) if self._fusable(other) else self.dense() * other

    def __getitem__(self, index):
        return self.dense()[index]

    def __getattr__(self, name):                                # anything else a tensor can do: the dense softmax does it
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.dense(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return _lazy_torch_function(func, args, kwargs)


class LazyDepthProduct:
    """candidates * LazyPdf: `.sum(dim=1, keepdim=True)` runs the fused kernel; anything else forms the dense product."""

    def __init__(self, candidates: Tensor, pdf: LazyPdf):
        self.candidates, self.pdf = candidates, pdf

    @property
    def shape(self):
        return self.pdf.shape

    def dense(self) -> Tensor:
        return self.candidates * self.pdf.dense()

    def sum(self, *args, **kwargs):
        dim = args[0] if args else kwargs.get("dim")
        keepdim = args[1] if len(args) > 1 else kwargs.get("keepdim", False)
        if (self.pdf._dense is None and self.pdf._candidates is self.candidates and _is_dim1(dim) and keepdim is True and len(args) <= 2
                and set(kwargs) <= {"dim", "keepdim"}):
            return self.pdf.head()[0]
        return self.dense().sum(*args, **kwargs)

    def __getitem__(self, index):
        return self.dense()[index]

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.dense(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return _lazy_torch_function(func, args, kwargs)


_MUL_FUNCS = (torch.mul, torch.Tensor.mul, torch.Tensor.__mul__, torch.Tensor.__rmul__)
_SUM_FUNCS = (torch.sum, torch.Tensor.sum)
_MAX_FUNCS = (torch.max, torch.Tensor.max)


def _lazy_torch_function(func, args, kwargs):
    """torch's dispatch for the two lazy classes: candidates * LazyPdf, sum(LazyDepthProduct, 1, True) and max(LazyPdf, 1, True)
    stay lazy / fused, everything else sees dense tensors."""
    kwargs = kwargs or {}
    if func in _MUL_FUNCS and len(args) == 2 and not kwargs:
        a, b = args
        if isinstance(b, LazyPdf) and b._fusable(a):
            return b._product(a)
        if isinstance(a, LazyPdf) and a._fusable(b):
            return a._product(b)
    if func in _SUM_FUNCS and args and isinstance(args[0], LazyDepthProduct):
        return args[0].sum(*args[1:], **kwargs)
    if func in _MAX_FUNCS and args and isinstance(args[0], LazyPdf):
        return args[0].max(*args[1:], **kwargs)

    def dense(x):
        return x.dense() if isinstance(x, (LazyPdf, LazyDepthProduct)) else x

    args = tuple([dense(y) for y in x] if isinstance(x, (list, tuple)) else dense(x) for x in args)
    return func(*args, **{k: dense(x) for k, x in kwargs.items()})


class FunctionalProxy:
    """Stands in for the name `F` (torch.nn.functional) of the predictor's module: every attribute is the replaced module's own,
    except that `softmax(x, dim=1)` of a 4-D float32 GPU tensor returns a LazyPdf.  `.replaced` is the module itself."""

    def __init__(self, replaced):
        self.replaced = replaced

    def __getattr__(self, name):
        if name == "replaced":                                  # not set yet (copying, unpickling): no recursion
            raise AttributeError(name)
        return getattr(self.replaced, name)

    def softmax(self, input, dim=None, *args, **kwargs):
        if (not args and not kwargs and _is_dim1(dim) and isinstance(input, Tensor) and input.is_cuda and input.dtype == torch.float32
                and input.dim() == 4 and input.numel() > 0):
            return LazyPdf(input, self.replaced.softmax)
        return self.replaced.softmax(input, dim, *args, **kwargs)
