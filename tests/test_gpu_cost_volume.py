"""The native spherical cost volume (splatter360_amd/cost_volume.py, csrc/s360_cost_volume.hip) on the GPU against the float64
statement of tests/cost_volume_reference.py.

Accuracy rule (the project's "as close to float64 as the float32 statement is", tests/test_gpu_headline_parity.py): on the
well-conditioned samples (cost_volume_reference.well_conditioned: away from the poles, the partner's centre and the ERP seam; the
excluded share must stay <= 1e-3) the kernel's max and mean absolute error against float64 are <= 1.5 x the same two figures of
the torch float32 statement on the same GPU and inputs; the gradient of the features likewise, over all elements.  An output
element is kept when every pairing's sample of it is well conditioned.

Measured on an MI355X at the hm3d shape (2 x 128 x 128 x 256, D = 128), forward, kept samples (profiles/cost_volume_timing.json,
"accuracy"): kernel max 7.05e-07 / mean 5.13e-08; torch float32 statement max 1.91e-03 / mean
6.03e-06; excluded share 3.3e-04.  Gradient of the features at that shape, all elements: kernel max 1.4e-05 / mean
1.8e-07; torch float32 max 3.0e-03 / mean 1.0e-05."""
import ctypes as C
import math
import sys
import types

import pytest
import torch

import cost_volume_reference as R
from splatter360_amd import _lib, cost_volume as cv, plugin

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (b, v, C, D, h, w, sampling, chunk of the reference's depth walk)
CASES = {
    "small_v2": (1, 2, 8, 16, 32, 64, "inverse_depth", None),
    "odd_v3": (2, 3, 5, 7, 12, 20, "log_depth", None),
    "wide_c": (1, 2, 132, 40, 16, 32, "linear_depth", None),
    "hm3d": (1, 2, 128, 128, 128, 256, "inverse_depth", 8),
}


def _inputs(name):
    b, v, c, d, h, w, smp, chunk = CASES[name]
    feats, ext, near, far = R.random_inputs(b, v, c, h, w, seed=sum(map(ord, name)), device=DEV)
    depths = cv.depth_candidates(near, far, d, smp).float().contiguous()
    poses = cv.relative_poses(ext).contiguous()
    return feats, ext, near, far, depths, poses, d, smp, chunk


def _kept(poses, depths, h, w, chunk):
    ok = R.well_conditioned(poses, depths, h, w, chunk)                 # [pairs, n, D, h w]
    return ok.all(dim=0).view(ok.shape[1], ok.shape[2], h, w), 1.0 - ok.float().mean().item()


@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64_as_closely_as_torch_float32(name):
    feats, ext, near, far, depths, poses, d, smp, chunk = _inputs(name)
    h, w = feats.shape[-2:]
    got = cv.spherical_cost_volume(feats, ext, near, far, d, smp, "hm3d")
    with torch.no_grad():
        want = R.cost_volume(feats, poses, depths, torch.float64, chunk)
        t32 = R.cost_volume(feats, poses, depths, torch.float32, chunk)
    kept, excluded = _kept(poses, depths, h, w, chunk)
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.isfinite(got).all()
    e_k, e_t = (got.double() - want).abs()[kept], (t32.double() - want).abs()[kept]
    figures = (e_k.max().item(), e_k.mean().item(), e_t.max().item(), e_t.mean().item())
    print(f"{name}: excluded {excluded:.3g}; kernel max/mean {figures[0]:.4g} {figures[1]:.4g}; torch f32 max/mean {figures[2]:.4g} {figures[3]:.4g}")
    assert excluded <= 1e-3
    assert figures[0] <= 1.5 * figures[2] and figures[1] <= 1.5 * figures[3], figures


@pytest.mark.parametrize("name", list(CASES))
def test_feature_gradient_matches_float64_as_closely_as_torch_float32(name):
    feats, ext, near, far, depths, poses, d, smp, chunk = _inputs(name)
    g = torch.randn(depths.shape[0], d, *feats.shape[-2:], device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    f = feats.clone().requires_grad_(True)
    cv.spherical_cost_volume(f, ext, near, far, d, smp, "hm3d").backward(g)
    want = R.feature_gradient(feats, poses, depths, g, torch.float64, chunk)
    t32 = R.feature_gradient(feats, poses, depths, g, torch.float32, chunk)
    e_k, e_t = (f.grad.double() - want).abs(), (t32.double() - want).abs()
    figures = (e_k.max().item(), e_k.mean().item(), e_t.max().item(), e_t.mean().item())
    print(f"{name}: gradient kernel max/mean {figures[0]:.4g} {figures[1]:.4g}; torch f32 max/mean {figures[2]:.4g} {figures[3]:.4g}")
    assert torch.isfinite(f.grad).all()
    assert figures[0] <= 1.5 * figures[2] and figures[1] <= 1.5 * figures[3], figures


def test_reference_gradient_agrees_with_central_differences():
    """Pins the reference itself: float64 autograd of the statement against central differences at one tiny shape (CPU)."""
    feats, ext, near, far = R.random_inputs(1, 2, 2, 4, 6, seed=3)
    depths, poses = cv.depth_candidates(near, far, 3).double(), cv.relative_poses(ext).double()
    g = torch.randn(2, 3, 4, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    grad = R.feature_gradient(feats, poses, depths, g)
    f64, eps = feats.double(), 1e-6
    for idx in [(0, 0, 0, 0, 0), (0, 1, 1, 3, 5), (0, 0, 1, 2, 2), (0, 1, 0, 1, 4)]:
        hi, lo = f64.clone(), f64.clone()
        hi[idx] += eps
        lo[idx] -= eps
        num = ((R.cost_volume(hi, poses, depths) - R.cost_volume(lo, poses, depths)) * g).sum() / (2 * eps)
        assert abs(num.item() - grad[idx].item()) <= 1e-7 * max(1.0, abs(num.item()))


def _own_side(feats, poses, depths, g):
    b, v, c, h, w = feats.shape
    f = feats.transpose(0, 1).reshape(v * b, c, h, w).contiguous()
    return cv.correlation_backward(g, f, f, cv.partner_slots(b, v, DEV), poses, depths, 1.0 / ((v - 1) * c ** 0.5), 0)[0]


def test_forward_and_own_side_gradient_are_bit_identical_across_runs_and_streams():
    feats, ext, near, far, depths, poses, d, smp, _ = _inputs("small_v2")
    g = torch.randn(depths.shape[0], d, *feats.shape[-2:], device=DEV)
    outs, owns = [], []
    for i in range(3):
        outs.append(cv.spherical_cost_volume(feats, ext, near, far, d, smp))
        owns.append(_own_side(feats, poses, depths, g))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        outs.append(cv.spherical_cost_volume(feats, ext, near, far, d, smp))
        owns.append(_own_side(feats, poses, depths, g))
    side.synchronize()
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs[1:]) and all(torch.equal(owns[0], o) for o in owns[1:])


def test_no_host_synchronisation_in_forward_and_backward():
    """Around the kernels' forward + backward (the autograd function with prepared poses, candidates and slot table): the
    reference's own pose expression, torch's `.inverse()`, checks its result on the host and is outside the guarded region."""
    feats, ext, near, far, depths, poses, d, smp, _ = _inputs("small_v2")
    f = feats.clone().requires_grad_(True)
    g = torch.randn(depths.shape[0], d, *feats.shape[-2:], device=DEV)
    cv.spherical_cost_volume(f, ext, near, far, d, smp).backward(g)           # warm-up: library load, allocator
    slots = cv.partner_slots(*feats.shape[:2], DEV)
    fl = feats.transpose(0, 1).reshape(-1, *feats.shape[2:]).contiguous()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = cv._CostVolume.apply(fl.requires_grad_(True), slots, poses, depths, 0.5, 0)
        out.backward(g)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_batch_elements_are_independent():
    feats, ext, near, far, depths, poses, d, smp, _ = _inputs("odd_v3")
    full = cv.spherical_cost_volume(feats, ext, near, far, d, smp)
    b, v = feats.shape[:2]
    for i in range(b):
        one = cv.spherical_cost_volume(feats[i:i + 1].contiguous(), ext[i:i + 1], near[i:i + 1], far[i:i + 1], d, smp)
        assert torch.equal(one, full.view(v, b, *full.shape[1:])[:, i])


def test_three_views_equal_the_mean_of_their_two_pairings():
    feats, ext, near, far, depths, poses, d, smp, _ = _inputs("odd_v3")
    b, v, c = feats.shape[:3]
    full = cv.spherical_cost_volume(feats, ext, near, far, d, smp)
    f01 = feats.transpose(0, 1).reshape(v * b, *feats.shape[2:]).contiguous()
    pairs = []
    for idx in (1, 2):
        f10 = feats[:, R.partner_order(v, idx)].transpose(0, 1).reshape(v * b, *feats.shape[2:]).contiguous()
        pairs.append(cv.pair_correlation(f01, f10, poses[idx - 1], depths) / c ** 0.5)
    mean = torch.stack(pairs).mean(0)
    assert (full - mean).abs().max().item() <= 4 * torch.finfo(torch.float32).eps * max(1.0, mean.abs().max().item())


def test_warp_entry_point_resamples_and_pads_with_zero():
    """Through the C entry point.  By construction of this convention ix lies in [0, w - 1] and iy in [0, h - 1], so a tap
    leaves the map only as x0 + 1 = w or y0 + 1 = h with weight zero, or when the warped position is not finite: an identity
    pose must give the reference's off-by-half resample (not the input), and a NaN / infinite candidate must give exact zeros."""
    n, c, h, w, d = 1, 3, 8, 16, 3
    f = torch.randn(n, c, h, w, device=DEV)
    pose = torch.eye(4, device=DEV).repeat(n, 1, 1)
    depths = torch.tensor([[1.0, float("nan"), float("inf")]], device=DEV)
    out = torch.full((n, c, d, h, w), 7.0, device=DEV)
    rc = _lib.lib().s360_cost_volume_warp(C.c_void_p(f.data_ptr()), None, C.c_void_p(pose.data_ptr()), C.c_void_p(depths.data_ptr()), n, n, c, h,
                                          w, d, 0, C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    # per element within 8 roundings of the sum of |taps| (tests/test_gpu_cost_volume_terms.py derives the count)
    want, mag = R.warp_terms(f, pose, depths[:, :1])
    assert ((out[:, :, :1].double().cpu() - want).abs() <= 8 * 2.0 ** -24 * mag).all()
    assert not torch.allclose(out[:, :, 0], f)                         # the off-by-half is reproduced, not fixed
    assert (out[:, :, 1] == 0).all() and (out[:, :, 2:] == 0).all()
    got = cv.warp_with_pose_depth_candidates(types.SimpleNamespace(dataset="replica"), f, pose, depths[:, :1, None, None].repeat(1, 1, h, w))
    assert torch.equal(got, out[:, :, :1])


def test_errors():
    feats, ext, near, far = R.random_inputs(1, 2, 4, 8, 16, seed=1, device=DEV)
    with pytest.raises(RuntimeError):
        cv.spherical_cost_volume(feats.cpu(), ext.cpu(), near.cpu(), far.cpu(), 4)
    with pytest.raises(ValueError):
        cv.spherical_cost_volume(feats.double(), ext.double(), near.double(), far.double(), 4)
    with pytest.raises(ValueError):
        cv.spherical_cost_volume(feats, ext, near, far, 4, dataset_name="m3d")
    with pytest.raises(ValueError):
        cv.spherical_cost_volume(feats[:, :1], ext[:, :1], near[:, :1], far[:, :1], 4)
    with pytest.raises(NotImplementedError):
        cv.spherical_cost_volume(feats, ext, near, far, 4, depth_sampling_type="sqrt_depth")


def test_memory_of_forward_and_backward_has_no_c_times_d_tensor():
    """Derived bound (no tensor with C * D elements): at the hm3d shape the peak of forward + backward stays within
    8 x (bytes of features + bytes of the output) = 536 MB; the warped tensor alone would be 4.29 GB."""
    feats, ext, near, far, depths, poses, d, smp, _ = _inputs("hm3d")
    g = torch.randn(depths.shape[0], d, *feats.shape[-2:], device=DEV)
    f = feats.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    out = cv.spherical_cost_volume(f, ext, near, far, d, smp)
    out.backward(g)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated(DEV) - base
    bound = 8 * (feats.numel() + out.numel()) * 4
    print(f"peak delta {delta / 1e6:.1f} MB, bound {bound / 1e6:.1f} MB")
    assert delta <= bound


class _FakePredictor(torch.nn.Module):
    """The calling pattern of the reference's predictor around the seam, on a fake module: warp through the module-level name,
    product with feat01.unsqueeze(2), sum over channels, / sqrt(c), stack, mean."""

    def __init__(self, mod, wo_cost_volume=False):
        super().__init__()
        self.mod, self.wo_cost_volume = mod, wo_cost_volume

    def forward(self, utils360, feat01, feat10s, poses, cand):
        if self.wo_cost_volume:
            return feat01
        c = feat01.shape[1]
        vols = []
        for feat10, pose in zip(feat10s, poses):
            warped = self.mod.warp_with_pose_depth_candidates(utils360, feat10, pose, cand.repeat([1, 1, *feat10.shape[-2:]]), warp_padding_mode="zeros")
            vols.append((feat01.unsqueeze(2) * warped).sum(1) / (c ** 0.5))
        return torch.mean(torch.stack(vols, dim=0), dim=0, keepdim=False)


def test_installed_seam_runs_the_kernels_and_falls_back():
    calls = []

    def reference_warp(utils360, feature1, pose, depth, clamp_min_depth=1e-3, warp_padding_mode="zeros", debug=False, **kw):
        calls.append(feature1.device.type)
        return R.warped_features(feature1, pose, depth[:, :, 0, 0], feature1.dtype)

    mod = types.ModuleType(plugin.COST_VOLUME_MODULE)
    mod.warp_with_pose_depth_candidates = reference_warp
    sys.modules[plugin.COST_VOLUME_MODULE] = mod
    try:
        fn = plugin.install_cost_volume()
        assert fn is mod.warp_with_pose_depth_candidates and fn.replaced is reference_warp
        feats, ext, near, far, depths, poses, d, smp, _ = _inputs("odd_v3")
        b, v = feats.shape[:2]
        f = feats.clone().requires_grad_(True)
        f01 = f.transpose(0, 1).reshape(v * b, *f.shape[2:])
        f10s = [f[:, R.partner_order(v, i)].transpose(0, 1).reshape(v * b, *f.shape[2:]) for i in range(1, v)]
        utils = types.SimpleNamespace(dataset="hm3d")
        out = _FakePredictor(mod)(utils, f01, f10s, list(poses), depths[:, :, None, None])
        assert calls == []                                              # the kernels ran, not the replaced function
        direct = cv.spherical_cost_volume(feats, ext, near, far, d, smp)
        assert (out - direct).abs().max().item() <= 4 * torch.finfo(torch.float32).eps * max(1.0, direct.abs().max().item())
        g = torch.randn_like(out)
        out.backward(g)
        f2 = feats.clone().requires_grad_(True)
        cv.spherical_cost_volume(f2, ext, near, far, d, smp).backward(g)
        assert (f.grad - f2.grad).abs().max().item() <= 1e-4 * max(1.0, f2.grad.abs().max().item())
        # fallbacks: CPU tensors go to the replaced function; wo_cost_volume never reaches the seam; another convention too
        cpu = _FakePredictor(mod)(utils, f01.detach().cpu(), [t.detach().cpu() for t in f10s], [p.cpu() for p in poses], depths[:, :, None, None].cpu())
        assert calls == ["cpu"] * (v - 1) and (cpu - direct.cpu()).abs().max().item() <= 1e-3
        del calls[:]
        assert _FakePredictor(mod, wo_cost_volume=True)(utils, f01, f10s, list(poses), depths[:, :, None, None]) is f01 and calls == []
        _FakePredictor(mod)(types.SimpleNamespace(dataset="m3d"), f01.detach(), [t.detach() for t in f10s], list(poses), depths[:, :, None, None])
        assert calls == ["cuda"] * (v - 1)
    finally:
        plugin.uninstall()
        assert sys.modules[plugin.COST_VOLUME_MODULE].warp_with_pose_depth_candidates is reference_warp
        del sys.modules[plugin.COST_VOLUME_MODULE]
