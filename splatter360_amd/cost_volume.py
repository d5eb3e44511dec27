"""The encoder's spherical plane-sweep cost volume on the GPU, forward and backward (csrc/s360_cost_volume.hip).

The reference builds `raw_correlation_in` (src/model/encoder/costvolume/depth_predictor_multiview_360.py:588-630) by warping every
other context view's features to each depth candidate (warp_with_pose_depth_candidates, :159-214), materialising grid_sample's
[v b, C, D, h, w] result, multiplying it with the own view's features and summing over C.  `spherical_cost_volume` computes the
same volume in one fused kernel that never forms a tensor with C * D elements; `depth_candidates` and `relative_poses` are the
reference's own torch expressions (prepare_feat_proj_data_lists_360, :299-373), so their values are the reference's to the bit.
Float32 GPU tensors only; there is no CPU path (plugin.install(cost_volume=True) keeps the replaced function for everything else).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from ._call import _check_cuda_f32, call, invoke, ptr

CONVENTIONS = {"hm3d": 0, "replica": 0}        # S360_CV_HM3D serves both (src/geometry/utils360.py:93, :148, :193, :250)
SAMPLINGS = ("inverse_depth", "log_depth", "linear_depth")


def _convention(dataset_name: str) -> int:
    if dataset_name not in CONVENTIONS:
        raise ValueError(f"the spherical cost volume knows the conventions {sorted(CONVENTIONS)}, got dataset_name={dataset_name!r}")
    return CONVENTIONS[dataset_name]


def _vb(t: Tensor) -> Tensor:
    """[b, v] -> [(v b), 1]: the reference's rearrange(t, "b v -> (v b) 1")."""
    return t.transpose(0, 1).reshape(-1, 1)


def depth_candidates(near: Tensor, far: Tensor, num_samples: int, depth_sampling_type: str = "inverse_depth") -> Tensor:
    """The depth candidates of prepare_feat_proj_data_lists_360 (:339-373) for near, far [b, v] -> [v b, D], with the reference's
    own torch expressions on the inputs' device (linspace is built on the host and moved, as there), so the values are the
    reference's to the bit.  inverse_depth: 1 / (1/far + t (1/near - 1/far)); log_depth: exp(log near + t (log far - log near));
    linear_depth: near + t (far - near).  Another name raises NotImplementedError, as the reference does."""
    near, far = near.detach(), far.detach()
    t = torch.linspace(0.0, 1.0, num_samples).unsqueeze(0)
    if depth_sampling_type == "inverse_depth":
        min_depth = _vb(1.0 / far.clone())
        max_depth = _vb(1.0 / near.clone())
        cand = min_depth + t.to(min_depth.device) * (max_depth - min_depth)
        return 1 / cand
    if depth_sampling_type == "log_depth":
        log_d_min = torch.log(_vb(near.clone()))
        log_d_max = torch.log(_vb(far.clone()))
        return torch.exp(log_d_min + t.to(log_d_min.device) * (log_d_max - log_d_min))
    if depth_sampling_type == "linear_depth":
        min_depth = _vb(near.clone())
        max_depth = _vb(far.clone())
        return min_depth + t.to(min_depth.device) * (max_depth - min_depth)
    raise NotImplementedError(depth_sampling_type)


def relative_poses(extrinsics_sphere: Tensor) -> Tensor:
    """The partner-from-own poses of prepare_feat_proj_data_lists_360 (:299-329) for extrinsics [b, v, 4, 4] -> [v - 1, v b, 4, 4]:
    pairing idx pairs view k with view (k + idx) mod v, in (v b) order.  v == 2 keeps the reference's special case
    (pose = E1.inverse() @ E0, then pose and pose.inverse()); v > 2 is E_partner.inverse() @ E_own per pair.  No gradient."""
    e = extrinsics_sphere.detach()
    b, v = int(e.shape[0]), int(e.shape[1])
    if v < 2:
        raise ValueError(f"the cost volume needs at least two views, got v={v}")
    if v == 2:
        pose = e[:, 1].clone().inverse() @ e[:, 0].clone()
        return torch.cat((pose, pose.inverse()), dim=0).unsqueeze(0)
    order = list(range(v))
    out = []
    for idx in range(1, v):
        cur = order[idx:] + order[:idx]
        out.append(torch.cat([e[:, v1].clone().inverse() @ e[:, v0].clone() for v0, v1 in zip(order, cur)], dim=0))
    return torch.stack(out, dim=0)


def partner_slots(b: int, v: int, device) -> Tensor:
    """int32 [v - 1, v b]: the (v b) slot that pairing idx samples for slot k b + i, i.e. ((k + idx) mod v) b + i."""
    k = torch.arange(v).repeat_interleave(b)
    i = torch.arange(b).repeat(v)
    rows = [((k + idx) % v) * b + i for idx in range(1, v)]
    return torch.stack(rows, dim=0).to(torch.int32).to(device)


def _workspace(name, args, device) -> tuple:
    nbytes = C.c_size_t(0)
    invoke(name, *args, None, C.byref(nbytes), None)
    return torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=device), nbytes


def correlation_forward(f_own: Tensor, f_partner: Tensor, slots, poses: Tensor, depths: Tensor, scale: float, convention: int) -> Tensor:
    """s360_cost_volume_forward on contiguous float32 GPU tensors: f_own [n, C, h, w], f_partner [m, C, h, w], slots int32
    [pairs, n] or None, poses [pairs, n, 4, 4], depths [n, D] -> [n, D, h, w]."""
    n, c, h, w = (int(s) for s in f_own.shape)
    m, pairs, d = int(f_partner.shape[0]), int(poses.shape[0]), int(depths.shape[1])
    out = torch.empty(n, d, h, w, dtype=torch.float32, device=f_own.device)
    dims = (n, m, pairs, c, h, w, d, convention, C.c_float(scale))
    ws, nbytes = _workspace("s360_cost_volume_forward", (None, None, None, None, None, *dims, None), f_own.device)
    call("s360_cost_volume_forward", f_own.device, ptr(f_own), ptr(f_partner), ptr(slots), ptr(poses), ptr(depths), *dims, ptr(out),
         ptr(ws), C.byref(nbytes))
    return out


def correlation_backward(g: Tensor, f_own: Tensor, f_partner: Tensor, slots, poses: Tensor, depths: Tensor, scale: float,
                         convention: int) -> tuple:
    """s360_cost_volume_backward: (grad_own [n, C, h, w], grad_partner [m, C, h, w]) for grad_out g [n, D, h, w]."""
    n, c, h, w = (int(s) for s in f_own.shape)
    m, pairs, d = int(f_partner.shape[0]), int(poses.shape[0]), int(depths.shape[1])
    g = g.to(torch.float32).contiguous()
    g_own, g_partner = torch.empty_like(f_own), torch.empty_like(f_partner)
    dims = (n, m, pairs, c, h, w, d, convention, C.c_float(scale))
    ws, nbytes = _workspace("s360_cost_volume_backward", (None, None, None, None, None, *dims, None, None, None), f_own.device)
    call("s360_cost_volume_backward", f_own.device, ptr(f_own), ptr(f_partner), ptr(slots), ptr(poses), ptr(depths), *dims, ptr(g),
         ptr(g_own), ptr(g_partner), ptr(ws), C.byref(nbytes))
    return g_own, g_partner


class _CostVolume(torch.autograd.Function):
    """All rolled pairings of one [v b, C, h, w] tensor in one call; gradient to the features only."""

    @staticmethod
    def forward(ctx, feats, slots, poses, depths, scale, convention):
        feats = feats.detach().contiguous()
        out = correlation_forward(feats, feats, slots, poses, depths, scale, convention)
        ctx.save_for_backward(feats, slots, poses, depths)
        ctx.opts = (scale, convention)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        feats, slots, poses, depths = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        g_own, g_partner = correlation_backward(g, feats, feats, slots, poses, depths, *ctx.opts)
        return g_own.add_(g_partner), None, None, None, None, None


class _PairCorrelation(torch.autograd.Function):
    """One pairing with the reference's own two tensors (the install seam's lazy handle): sum_c own * warp(partner), unscaled."""

    @staticmethod
    def forward(ctx, f_own, f_partner, poses, depths, convention):
        f_own, f_partner = f_own.detach().contiguous(), f_partner.detach().contiguous()
        out = correlation_forward(f_own, f_partner, None, poses, depths, 1.0, convention)
        ctx.save_for_backward(f_own, f_partner, poses, depths)
        ctx.convention = convention
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f_own, f_partner, poses, depths = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 5
        g_own, g_partner = correlation_backward(g, f_own, f_partner, None, poses, depths, 1.0, ctx.convention)
        return (g_own if ctx.needs_input_grad[0] else None), (g_partner if ctx.needs_input_grad[1] else None), None, None, None


def pair_correlation(f_own: Tensor, f_partner: Tensor, pose: Tensor, depths: Tensor, dataset_name: str = "hm3d") -> Tensor:
    """sum_c f_own[n, c] * warp(f_partner[n, c]) for one pairing -> [n, D, h, w], NOT divided by sqrt(C): f_own, f_partner
    [n, C, h, w], pose [n, 4, 4] partner from own, depths [n, D].  Differentiable in both feature tensors (once)."""
    _check_cuda_f32("pair_correlation", f_own, f_partner, pose, depths)
    if f_own.dim() != 4 or f_partner.shape != f_own.shape:
        raise ValueError(f"pair_correlation expects two [n, C, h, w] tensors, got {tuple(f_own.shape)} and {tuple(f_partner.shape)}")
    n = int(f_own.shape[0])
    if tuple(pose.shape) != (n, 4, 4) or depths.dim() != 2 or int(depths.shape[0]) != n:
        raise ValueError(f"pair_correlation expects pose [n, 4, 4] and depths [n, D], got {tuple(pose.shape)} and {tuple(depths.shape)}")
    return _PairCorrelation.apply(f_own, f_partner, pose.detach().reshape(1, n, 4, 4).contiguous(), depths.detach().contiguous(),
                                  _convention(dataset_name))


def spherical_cost_volume(features: Tensor, extrinsics_sphere: Tensor, near: Tensor, far: Tensor, num_depth_candidates: int,
                          depth_sampling_type: str = "inverse_depth", dataset_name: str = "hm3d") -> Tensor:
    """The reference's raw correlation volume (depth_predictor_multiview_360.py:588-630, before the concatenation with feat01):
    features [b, v, C, h, w], extrinsics_sphere [b, v, 4, 4], near, far [b, v] -> [v b, D, h, w] in the reference's (v b) order,

        out[n, d] = mean over the v - 1 rolled partner views of  sum_c f_own[c] * grid_sample(f_partner[c], warp(d)) / sqrt(C)

    in one fused kernel: no tensor with C * D elements exists forward or backward.  Differentiable in `features` only (once);
    poses, near / far and the candidates take no gradient, as the reference computes the grid under no_grad.  The forward and
    the own-side (gather) half of the gradient are bit-identical from run to run; the partner-side (scatter) half uses float32
    atomic adds, as grid_sample's own backward does, so the gradient's last bits depend on arrival order.
    The reference's `assert (u, v in [-1, 1]).all()` on the grid is a host synchronisation and is dropped: for this convention
    u = -theta' / pi and v = -2 phi' / pi with theta' in [-pi, pi], phi' in [-pi/2, pi/2] hold by construction.  The warp is
    evaluated in float64 from the float32 poses and candidates.  Float32 GPU tensors; no CPU path; dataset_name 'hm3d' or
    'replica' (one convention), anything else raises ValueError; v >= 2."""
    convention = _convention(dataset_name)
    if features.dim() != 5:
        raise ValueError(f"spherical_cost_volume expects [b, v, C, h, w] features, got shape {tuple(features.shape)}")
    _check_cuda_f32("spherical_cost_volume", features, extrinsics_sphere, near, far)
    b, v, c, h, w = (int(s) for s in features.shape)
    if v < 2:
        raise ValueError(f"the cost volume needs at least two views, got v={v}")
    if tuple(extrinsics_sphere.shape) != (b, v, 4, 4) or tuple(near.shape) != (b, v) or tuple(far.shape) != (b, v):
        raise ValueError("spherical_cost_volume expects extrinsics [b, v, 4, 4] and near, far [b, v], got "
                         f"{tuple(extrinsics_sphere.shape)}, {tuple(near.shape)}, {tuple(far.shape)}")
    if features.numel() == 0 or int(num_depth_candidates) < 1:
        raise ValueError("spherical_cost_volume: empty tensors")
    depths = depth_candidates(near, far, int(num_depth_candidates), depth_sampling_type).to(torch.float32).contiguous()
    poses = relative_poses(extrinsics_sphere).contiguous()
    slots = partner_slots(b, v, features.device)
    feats = features.transpose(0, 1).reshape(v * b, c, h, w)          # "b v ... -> (v b) ..."
    return _CostVolume.apply(feats, slots, poses, depths, 1.0 / ((v - 1) * c ** 0.5), convention)


def warp_with_pose_depth_candidates(utils360, feature1: Tensor, pose: Tensor, depth: Tensor, clamp_min_depth=1e-3,
                                    warp_padding_mode="zeros", debug=False, gt_rgb1=None, gt_depth0=None, gt_rgb0=None) -> Tensor:
    """The reference's warp_with_pose_depth_candidates (:73-214) with its signature: feature1 [B, C, H, W], pose [B, 4, 4],
    depth [B, D, H, W] constant over H, W (the candidates, as its one caller passes them) -> the materialised [B, C, D, H, W]
    warped tensor, by one native kernel.  It exists for callers that use the function alone; the cost volume itself never forms
    this tensor.  The reference's host-side assert on the grid is dropped (see spherical_cost_volume).  utils360.dataset names
    the convention.  No autograd: feature1 must not require grad (the install seam keeps the replaced function for that)."""
    _check_cuda_f32("warp_with_pose_depth_candidates", feature1, pose, depth)
    convention = _convention(getattr(utils360, "dataset", None))
    if warp_padding_mode != "zeros" or debug:
        raise ValueError("warp_with_pose_depth_candidates: only warp_padding_mode='zeros' without debug")
    if feature1.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("warp_with_pose_depth_candidates materialises without autograd; use spherical_cost_volume / pair_correlation")
    if feature1.dim() != 4 or depth.dim() != 4 or tuple(pose.shape) != (int(feature1.shape[0]), 4, 4):
        raise ValueError("warp_with_pose_depth_candidates expects feature1 [B, C, H, W], pose [B, 4, 4], depth [B, D, H, W]")
    n, c, h, w = (int(s) for s in feature1.shape)
    d = int(depth.shape[1])
    if int(depth.shape[0]) != n or tuple(depth.shape[2:]) != (h, w):
        raise ValueError(f"warp_with_pose_depth_candidates: depth {tuple(depth.shape)} does not match feature1 {tuple(feature1.shape)}")
    f = feature1.detach().contiguous()
    out = torch.empty(n, c, d, h, w, dtype=torch.float32, device=f.device)
    call("s360_cost_volume_warp", f.device, ptr(f), None, ptr(pose.detach().contiguous()), ptr(depth.detach()[:, :, 0, 0].contiguous()),
         n, n, c, h, w, d, convention, ptr(out))
    return out


class LazyWarp:
    """What the installed warp_with_pose_depth_candidates returns: the arguments of one pairing's warp, not its [B, C, D, H, W]
    result.  `feat01.unsqueeze(2) * handle` gives a LazyProduct whose `.sum(1)` is pair_correlation (the fused kernel: the sum
    over channels, not yet divided by sqrt(C)), so the reference's own `/ c ** 0.5`, stack and mean then run unchanged on
    [v b, D, h, w] tensors.  Any other use goes through `materialise()`: the native warp kernel, or — when a gradient to
    feature1 is needed — the replaced function."""

    def __init__(self, utils360, feature1, pose, depth, replaced, kwargs):
        self.utils360, self.feature1, self.pose, self.depth, self.replaced, self.kwargs = utils360, feature1, pose, depth, replaced, kwargs
        self._dense = None

    @property
    def shape(self):
        return torch.Size((self.feature1.shape[0], self.feature1.shape[1], self.depth.shape[1], *self.feature1.shape[2:]))

    def materialise(self) -> Tensor:
        if self._dense is None:
            native = all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 for t in (self.feature1, self.pose, self.depth))
            if not native or (self.feature1.requires_grad and torch.is_grad_enabled()):
                self._dense = self.replaced(self.utils360, self.feature1, self.pose, self.depth, **self.kwargs)
            else:
                self._dense = warp_with_pose_depth_candidates(self.utils360, self.feature1, self.pose, self.depth, **self.kwargs)
        return self._dense

    def _fusable(self, other) -> bool:
        f = self.feature1
        return (isinstance(other, Tensor) and other.is_cuda and other.dtype == torch.float32 and other.dim() == 5 and other.shape[2] == 1
                and other.device == f.device and tuple(other.shape[:2]) + tuple(other.shape[3:]) == tuple(f.shape))

    def __rmul__(self, other):
        return LazyProduct(other, self) if self._fusable(other) else other * self.materialise()

    def __mul__(self, other):
        return LazyProduct(other, self) if self._fusable(other) else self.materialise() * other

    def __getattr__(self, name):                                # anything else a tensor can do: the dense tensor does it
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.materialise(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return _lazy_torch_function(func, args, kwargs)


class LazyProduct:
    """own.unsqueeze(2) * LazyWarp: `.sum(1)` (or sum(dim=1)) runs the fused kernel; anything else forms the dense product."""

    def __init__(self, own5, warp: LazyWarp):
        self.own5, self.warp = own5, warp

    def dense(self) -> Tensor:
        return self.own5 * self.warp.materialise()

    def sum(self, *args, **kwargs):
        dim = args[0] if args else kwargs.get("dim")
        if dim == 1 and len(args) <= 1 and set(kwargs) <= {"dim"}:
            w = self.warp
            return pair_correlation(self.own5[:, :, 0], w.feature1, w.pose, w.depth[:, :, 0, 0], w.utils360.dataset)
        return self.dense().sum(*args, **kwargs)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self.dense(), name)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        return _lazy_torch_function(func, args, kwargs)


_MUL_FUNCS = (torch.mul, torch.Tensor.mul, torch.Tensor.__mul__, torch.Tensor.__rmul__)
_SUM_FUNCS = (torch.sum, torch.Tensor.sum)


def _lazy_torch_function(func, args, kwargs):
    """torch's dispatch for the two lazy classes: tensor * LazyWarp and sum(LazyProduct, 1) stay lazy / fused, everything else
    sees dense tensors."""
    kwargs = kwargs or {}
    if func in _MUL_FUNCS and len(args) == 2 and not kwargs:
        a, b = args
        if isinstance(b, LazyWarp) and b._fusable(a):
            return LazyProduct(a, b)
        if isinstance(a, LazyWarp) and a._fusable(b):
            return LazyProduct(b, a)
    if func in _SUM_FUNCS and args and isinstance(args[0], LazyProduct):
        return args[0].sum(*args[1:], **kwargs)

    def dense(x):
        return x.materialise() if isinstance(x, LazyWarp) else x.dense() if isinstance(x, LazyProduct) else x

    args = tuple([dense(y) for y in x] if isinstance(x, (list, tuple)) else dense(x) for x in args)
    return func(*args, **{k: dense(x) for k, x in kwargs.items()})
