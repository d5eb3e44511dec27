"""Lazy Gaussians — the seam that lets the UNCHANGED reference reach the fused raw path (s360_forward_raw / s360_backward_raw).

In the reference the encoder ends with `self.gaussian_adapter_erp.forward(...)` (/root/reference/src/model/encoder/encoder_costvolume.py:414-427,
the module of src/model/encoder/common/gaussian_adapter_erp.py:33-119, constructed at encoder_costvolume.py:185), flattens the result
with four `rearrange` calls into the `Gaussians` container (:490-507, src/model/types.py:7-12) and the model wrapper hands that to the
decoder (src/model/model_wrapper_erp.py:217-229).  A drop-in adapter therefore has to materialise 352 B per Gaussian (means,
[.,3,3] covariances, [.,3,25] harmonics) only for the rasteriser to read them back — the round trip the raw entry points remove.

`install(adapter=True)` (plugin.py) replaces the adapter CLASS with `make_adapter_class(...)`'s: same constructor (`cfg` with
gaussian_scale_min / gaussian_scale_max / sh_degree), same forward arguments, same result container — but `means`, `covariances`,
`harmonics`, `scales`, `rotations` are `LazyField`s: torch.Tensor wrapper subclasses that carry shape / dtype / device and a
reference to the adapter's INPUTS (a `RawBundle`), no data.  A pure reshape of a LazyField (what the encoder's `rearrange`s are)
stays lazy; ANY other operation first materialises the field with the stand-alone adapter kernels (adapter.adapter_tail: one launch,
cached in the bundle, autograd-connected to the encoder's outputs) and then runs on the real tensor — every other consumer of the
Gaussians (ply export, visualisation, a different decoder) sees ordinary tensors with the reference's values.  The fused decoder
(decoder.DecoderSplattingFused, registered by install()) recognises untouched LazyFields (`bundle_of`) and calls
rasterizer.rasterize_raw on the bundle's raw tensors instead: neither harmonics nor covariances ever exist.  This holds at every
SH degree of RAW_SEAM_DEGREES (d_sh = (sh_degree + 1)^2 coefficients per channel, raw records of 7 + 3 d_sh floats; the reference's
configuration is degree 4: [.,3,25] harmonics, 82-float records).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import adapter as _adapter

# The seam table: the SH degrees at which the adapter class hands out lazy fields, so that the fused decoder renders from the raw
# records (rasterizer.rasterize_raw).  A degree is listed when the raw path is not slower than the two-step path (adapter kernels,
# then render) beyond the run-to-run spread of scripts/raw_degrees_timing.py (profiles/raw_degrees_timing.json); at any other degree
# the class keeps the eager adapter, and rasterize_raw stays available to a caller who asks for it directly.
RAW_SEAM_DEGREES = (0, 1, 2, 3, 4)
# ... and the degrees at which the fused decoder reads the raw words where the encoder's last convolution left them (raw_planes_of
# below, rasterize_raw(raw_layout="planes")) instead of transposing them into records first.  The same rule: a degree is listed where
# the plane route is not slower than the record route from the same convolution output beyond the run-to-run spread of
# scripts/raw_planes_timing.py (profiles/raw_planes_timing.json, legs B against A).  rasterize_raw takes planes at every degree.
RAW_PLANE_SEAM_DEGREES = (0, 1, 2, 3, 4)

_FIELDS = {"means": (3,), "covariances": (3, 3), "scales": (3,), "rotations": (4,), "harmonics": None}


class RawBundle:
    """The adapter's inputs, kept instead of its outputs.  depths / opacities [b, v, r, srf, spp]; raw [b, v, r, srf, spp or 1, 7 + 3 d_sh];
    extrinsics [b, v, 4, 4] (context panoramas, camera-to-world)."""

    def __init__(self, module, dataset_name, extrinsics, depths, opacities, raw, image_shape, eps):
        self.module, self.dataset_name, self.eps = module, dataset_name, float(eps)
        self.extrinsics, self.depths, self.opacities, self.raw = extrinsics, depths, opacities, raw
        self.image_shape = (int(image_shape[0]), int(image_shape[1]))
        self.shape5 = tuple(int(x) for x in depths.shape)
        self._materialised = None
        self._rot = None

    @property
    def device(self):
        return self.depths.device

    @property
    def per_ray(self) -> int:
        return self.shape5[3] * self.shape5[4]

    @property
    def d_sh(self) -> int:
        """Coefficients per colour channel of the raw records (7 + 3 * d_sh floats each): 1, 4, 9, 16 or 25."""
        return (int(self.raw.shape[-1]) - 7) // 3

    def sh_rotation(self) -> Optional[Tensor]:
        """[b * v, d_sh, d_sh] matrices of rotate_sh for the context views (None: identity), built once per bundle."""
        if self._rot is None:
            b, v = self.shape5[:2]
            self._rot = (self.module.rotation_blocks(self.extrinsics.reshape(b * v, 4, 4)),)
        return self._rot[0]

    def materialised(self):
        """The adapter's real outputs (stand-alone kernels), computed at most once."""
        if self._materialised is None:
            b, v = self.shape5[:2]
            self._materialised = self.module.forward_eager(self.dataset_name, self.extrinsics.reshape(b, v, 1, 1, 1, 4, 4), self.depths,
                                                           self.opacities, self.raw, self.image_shape, self.eps, sh_rot=self.sh_rotation())
        return self._materialised

    def field(self, name: str, shape) -> Tensor:
        return getattr(self.materialised(), name).reshape(shape)


_PURE_RESHAPES = {"reshape", "view", "_unsafe_view", "reshape_as", "view_as", "flatten", "unflatten", "unsqueeze", "squeeze", "contiguous",
                  "detach_", "requires_grad_"}
_METADATA = {"size", "dim", "numel", "nelement", "ndimension", "is_floating_point", "is_complex", "element_size", "is_contiguous", "get_device",
             "__len__", "__repr__", "__str__", "__format__", "__hash__", "is_shared", "is_pinned", "is_leaf", "_is_view", "type", "is_inference",
             "is_same_size", "stride", "storage_offset", "data_ptr"}


class LazyField(torch.Tensor):
    """A field of the adapter's result that has not been computed: metadata + (bundle, field name).  See the module docstring."""

    @staticmethod
    def __new__(cls, bundle: RawBundle, field: str, shape):
        t = torch.Tensor._make_wrapper_subclass(cls, tuple(int(x) for x in shape), dtype=torch.float32, device=bundle.device,
                                                requires_grad=False)
        t._s360_bundle, t._s360_field = bundle, field
        return t

    def materialise(self) -> Tensor:
        """The real tensor (reference values, autograd-connected to the encoder's outputs) in this field's current shape."""
        return self._s360_bundle.field(self._s360_field, tuple(self.shape))

    def __repr__(self):   # never materialise for a debugger's sake
        return f"LazyField({self._s360_field}, shape={tuple(self.shape)}, device={self.device})"

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        me = next((a for a in args if isinstance(a, LazyField)), None)
        if name == "__get__" or name in _METADATA:      # .shape / .dtype / .device / .ndim / size() ...: the wrapper's own metadata
            if name in ("stride", "storage_offset", "data_ptr", "is_contiguous") and me is not None:
                return func(me.materialise(), *args[1:], **kwargs)
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **kwargs)
        if me is not None and me is args[0] and name in _PURE_RESHAPES and not any(isinstance(a, LazyField) for a in args[1:]):
            if name in ("contiguous", "detach_", "requires_grad_"):
                return me
            # the new shape from a storage-less meta tensor: any pure reshape keeps the element order, hence stays lazy
            meta = torch.empty(tuple(me.shape), dtype=torch.float32, device="meta")
            margs = tuple(torch.empty(tuple(a.shape), device="meta") if isinstance(a, Tensor) else a for a in args[1:])
            new_shape = tuple(func(meta, *margs, **kwargs).shape)
            return LazyField(me._s360_bundle, me._s360_field, new_shape)
        if me is not None and name in ("permute", "transpose") and _identity_permutation(name, args, kwargs, me.dim()):
            return me
        # anything else: compute on the real tensors
        real = lambda a: a.materialise() if isinstance(a, LazyField) else a
        deep = lambda a: type(a)(deep(x) for x in a) if isinstance(a, (list, tuple)) else real(a)
        with torch._C.DisableTorchFunctionSubclass():
            return func(*deep(tuple(args)), **{k: deep(v) for k, v in kwargs.items()})


    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        """Whatever reaches the dispatcher without passing __torch_function__ (C++ callers): compute on the real tensors."""
        from torch.utils._pytree import tree_map
        real = lambda a: a.materialise() if isinstance(a, LazyField) else a
        return func(*tree_map(real, tuple(args)), **tree_map(real, dict(kwargs or {})))


def _identity_permutation(name, args, kwargs, nd) -> bool:
    try:
        if name == "permute":
            dims = args[1] if len(args) == 2 and isinstance(args[1], (list, tuple)) else args[1:]
            return [int(d) % nd for d in dims] == list(range(nd))
        return len(args) == 3 and int(args[1]) % nd == int(args[2]) % nd
    except Exception:
        return False


class RawPlanes(NamedTuple):
    """What raw_planes_of found: the adapter's raw_gaussians is a view of `base` [(v b), C, h, w] (contiguous float32); per surface
    `surface_channels` = C / srf channels, of which the first `channel_offset` precede the record; context view j of batch element i is
    base[j * b + i], `view_stride` = b C h w floats after view j - 1."""
    base: Tensor
    channel_offset: int
    surface_channels: int
    view_stride: int

    def element(self, i: int, b: int) -> Tensor:
        """[v, C, h, w]: the planes of batch element i of b, in place (view stride b C h w)."""
        base = self.base
        if b == 1:
            return base
        return base.view(base.shape[0] // b, b, *base.shape[1:])[:, i]


def raw_planes_of(raw) -> Optional[RawPlanes]:
    """Is the adapter's raw_gaussians [b, v, r, srf, 1, 7 + 3 d_sh] what the reference's encoder hands over — the last convolution's
    output [(v b), C, h, w] under "(v b) c h w -> b v (h w) c", "... (srf c) -> ... srf c" and the [..., k:] slice that drops the
    offset_xy channels, three views and not one byte moved?  Decided from shape, strides, storage offset and `_base` alone (no device
    work, no data read); None for anything else — a copy, channels-last memory, another dtype, a base that is itself strided, an
    expanded samples-per-pixel dimension, a slice that does not run to the surface's last channel — and the caller keeps the record
    route.  Strides of size-1 dimensions carry no information and are ignored."""
    if not isinstance(raw, Tensor) or isinstance(raw, LazyField) or raw.dim() != 6 or raw.dtype != torch.float32:
        return None
    base = getattr(raw, "_base", None)
    if base is None or base.dim() != 4 or base.dtype != torch.float32 or not base.is_contiguous():
        return None
    b, v, r, srf, spp, width = (int(x) for x in raw.shape)
    n, c_total, h, w = (int(x) for x in base.shape)
    hw = h * w
    if spp != 1 or n != v * b or r != hw or srf < 1 or c_total % srf or min(b, v, r, width) < 1:
        return None
    cs = c_total // srf
    off = int(raw.storage_offset()) - int(base.storage_offset())
    if off < 0 or off % hw or off // hw + width != cs:
        return None
    want = (c_total * hw, b * c_total * hw, 1, cs * hw, 0, hw)       # "(v b)": the batch index is the fast one
    if any(size > 1 and int(st) != exp for size, st, exp in zip(raw.shape, raw.stride(), want)):
        return None
    return RawPlanes(base, off // hw, cs, b * c_total * hw)


def bundle_of(gaussians, d_sh: Optional[int] = None) -> Optional[RawBundle]:
    """The RawBundle behind a Gaussians container whose means / covariances / harmonics are UNTOUCHED LazyFields of one adapter call
    in the reference's flat layout ([b, G, 3], [b, G, 3, 3], [b, G, 3, d_sh]: src/model/types.py:7-12), else None.  d_sh is read from
    the bundle's own raw records (7 + 3 * d_sh floats each) unless the caller names one."""
    try:
        m, c, h = gaussians.means, gaussians.covariances, gaussians.harmonics
    except AttributeError:
        return None
    if not (isinstance(m, LazyField) and isinstance(c, LazyField) and isinstance(h, LazyField)):
        return None
    bd = m._s360_bundle
    if c._s360_bundle is not bd or h._s360_bundle is not bd or (m._s360_field, c._s360_field, h._s360_field) != ("means", "covariances", "harmonics"):
        return None
    b = bd.shape5[0]
    g = math.prod(bd.shape5[1:])
    if d_sh is None:
        d_sh = bd.d_sh
    if tuple(m.shape) != (b, g, 3) or tuple(c.shape) != (b, g, 3, 3) or tuple(h.shape) != (b, g, 3, d_sh):
        return None
    op = gaussians.opacities
    if isinstance(op, LazyField) or tuple(op.shape) != (b, g):
        return None
    return bd


def make_adapter_class(base_cls=None, container_cls=None, *, sh_rotation="native", differentiable_means: bool = False, lazy: bool = True,
                       name: str = "GaussianAdapterERPFusedMI355X"):
    """A class with the reference adapter's constructor and forward contract (gaussian_adapter_erp.py:33-119) whose forward returns
    lazy fields (module docstring).  base_cls: the reference's own GaussianAdapterERP (install(adapter=True): isinstance checks and
    its `d_sh` / `d_in` properties keep working) or None; container_cls: the reference's adapter-side `Gaussians` dataclass (six
    fields, gaussian_adapter.py) or None = adapter.AdapterGaussians."""
    container = container_cls or _adapter.AdapterGaussians
    bases = (base_cls,) if base_cls is not None else (torch.nn.Module,)

    class _Adapter(*bases):
        def __init__(self, cfg) -> None:
            if base_cls is not None:
                super().__init__(cfg)                     # registers the reference's own sh_mask buffer, keeps self.cfg
            else:
                torch.nn.Module.__init__(self)
                self.cfg = cfg
                self.register_buffer("sh_mask", _adapter.sh_mask((int(cfg.sh_degree) + 1) ** 2), persistent=False)
            self._s360 = _adapter.GaussianAdapterERP(float(cfg.gaussian_scale_min), float(cfg.gaussian_scale_max), int(cfg.sh_degree),
                                                     sh_rotation=sh_rotation, differentiable_means=differentiable_means)
            self.s360_lazy = bool(lazy)

        if base_cls is None:
            @property
            def d_sh(self) -> int:
                return (int(self.cfg.sh_degree) + 1) ** 2

            @property
            def d_in(self) -> int:
                return 7 + 3 * self.d_sh

        # ---- what RawBundle calls back
        def rotation_blocks(self, ext):
            return self._s360.rotation_blocks(ext)

        def forward_eager(self, dataset_name, extrinsics, depths, opacities, raw_gaussians, image_shape, eps, sh_rot="build"):
            g = self._s360.forward(dataset_name, extrinsics, depths, opacities, raw_gaussians, image_shape, eps, sh_rot=sh_rot)
            return g

        def forward(self, dataset_name, extrinsics, depths, opacities, raw_gaussians, image_shape, eps: float = 1e-8):
            if not depths.is_cuda:
                raise RuntimeError("GaussianAdapterERP (splatter360_amd) runs on the GPU only: depths is a CPU tensor (no CPU path in the product)")
            if dataset_name not in _adapter.ERP_CONVENTIONS:
                raise Exception(f"no ERP convention for dataset {dataset_name!r} (src/geometry/utils360.py raises for it too)")
            d_sh = (int(self.cfg.sh_degree) + 1) ** 2
            if not self.s360_lazy or int(self.cfg.sh_degree) not in RAW_SEAM_DEGREES or depths.dim() != 5:
                g = self.forward_eager(dataset_name, extrinsics, depths, opacities, raw_gaussians, image_shape, eps)
                return container(means=g.means, covariances=g.covariances, scales=g.scales, rotations=g.rotations, harmonics=g.harmonics,
                                 opacities=g.opacities)
            b, v, r, srf, spp = (int(x) for x in depths.shape)
            bundle = RawBundle(self, dataset_name, extrinsics.reshape(b, v, 4, 4), depths, opacities, raw_gaussians, image_shape, eps)
            sh5 = (b, v, r, srf, spp)
            f = lambda nm, tail: LazyField(bundle, nm, sh5 + tail)
            return container(means=f("means", (3,)), covariances=f("covariances", (3, 3)), scales=f("scales", (3,)),
                             rotations=f("rotations", (4,)), harmonics=f("harmonics", (3, d_sh)), opacities=opacities)

    _Adapter.__name__ = _Adapter.__qualname__ = name
    return _Adapter
