"""The depth-smoothness kernels (csrc/s360_depth_smooth.hip) through splatter360_amd.depth_smooth, against the float64 statement
of tests/depth_smooth_reference.py (its fidelity to the reference's LossDepth is pinned in tests/test_depth_smooth_spec.py) and
against torch's float32 chain of the reference's lines on the same GPU.

Bars: loss within 1 float32 ulp of the statement (one rounding is 0.5 ulp; the float64 summation order is worth N 2^-53) and
within 1e-5 relative of torch's float32 chain; gradient within 2^-23 A per pixel (one rounding is 2^-24 |g| <= 2^-24 A) and
exactly 0 where A = 0."""
import functools
import types

import numpy as np
import pytest
import torch

import depth_smooth_reference as R

pytestmark = pytest.mark.gpu

# the smallest shapes that cross a lane, a wave (64 columns), a row-tile (32 rows) and a block boundary; (1, 12, 5, 7) runs once
# with one bound per panorama of six faces (Vn = V / 6 = 2)
SHAPES = [(1, 1, 2, 2), (1, 1, 3, 3), (2, 6, 5, 7), (1, 2, 33, 260), (1, 3, 17, 130), (1, 6, 64, 64)]
CASES = [(s, vn, m) for s in SHAPES for vn in sorted({1, s[1]}) for m in R.MODES if not (m[1] and min(s[2:]) < 3)]
CASES += [((1, 12, 5, 7), 2, m) for m in R.MODES[3:]]
DEV = "cuda:0"
G_IN = 0.75                                                       # the incoming gradient of the main test


def _id(case):
    shape, vn, mode = case
    return "x".join(map(str, shape)) + f"-vn{vn}-{mode[0]}"


@functools.lru_cache(maxsize=None)
def _case(shape, vn):
    return R.make_case(shape, vn, seed=sum(shape) + 31 * vn, device=DEV)      # the ties sit at the DEVICE's float32 logs


@functools.lru_cache(maxsize=None)
def _want(shape, vn, mode, g=G_IN):
    c = _case(shape, vn)
    return R.statement(c["depth"], R.torch_log(c["near"], DEV), R.torch_log(c["far"], DEV), c["image"], mode[2], mode[1], g=g)


def _tensors(shape, vn, dev):
    c = _case(shape, vn)
    return tuple(torch.from_numpy(c[k]).to(dev) for k in ("depth", "near", "far", "image"))


def _check(loss, grad, want, what):
    """The two bars against the statement; prints each figure first."""
    got, w64 = float(loss), float(want["loss64"])
    ulp = float(np.spacing(np.float32(abs(w64))))
    a = want["A"]
    err = np.abs(grad.double().cpu().numpy() - want["grad64"])
    worst = float((err[a > 0] / a[a > 0]).max()) if (a > 0).any() else 0.0
    print(what, "loss", got, "statement", w64, "ulps", abs(got - w64) / ulp, "grad err / A", worst, "(bar", 2.0 ** -23, ")")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert abs(got - w64) <= ulp, (got, w64)
    assert (err <= 2.0 ** -23 * a).all(), worst
    assert (grad.cpu().numpy()[a == 0] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_forward_and_backward(gpu, case):
    from splatter360_amd import depth_smooth
    shape, vn, (name, second, sigma) = case
    depth, near, far, image = _tensors(shape, vn, gpu)
    depth_in, image_in = depth.clone(), image.clone()
    d = depth.clone().requires_grad_(True)
    loss = depth_smooth.depth_smoothness_loss(d, near, far, image if sigma is not None else None, sigma_image=sigma,
                                              use_second_derivative=second)
    loss.backward(torch.tensor(G_IN, device=gpu))
    want = _want(shape, vn, (name, second, sigma))
    _check(loss.detach(), d.grad, want, _id(case))
    assert torch.equal(depth, depth_in) and torch.equal(d.detach(), depth_in) and torch.equal(image, image_in)     # inputs untouched
    # torch's float32 chain of the reference's lines on the same device
    ref = R.torch_statement(depth, near, far, image, sigma, second)
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()), (loss.item(), ref.item())
    # the constant plane and the plane wholly beyond far: no loss and no gradient from their own terms
    b, v = shape[0], shape[1]
    for plane in [v - 1] * (v >= 2) + [v - 2] * (v >= 3):
        sel = (slice(b - 1, b), slice(plane, plane + 1))
        assert (want["tx"][sel] == 0).all() and (want["ty"][sel] == 0).all() and (d.grad[sel] == 0).all()
        nf = [x[b - 1:, (plane // (v // vn)):(plane // (v // vn)) + 1] for x in (near, far)]
        one = depth[sel].clone().requires_grad_(True)
        alone = depth_smooth.depth_smoothness_loss(one, *nf, image[sel] if sigma is not None else None, sigma_image=sigma,
                                                   use_second_derivative=second)
        alone.backward()
        assert alone.item() == 0.0 and (one.grad == 0).all()


def test_the_cases_hold_their_edge_inputs(gpu):
    for shape, vn in {(c[0], c[1]) for c in CASES if min(c[0][2:]) >= 3}:
        c = _case(shape, vn)
        per = shape[1] // vn
        lo, hi = (np.repeat(R.torch_log(c[k], DEV), per, 1)[:, :, None, None] for k in ("near", "far"))
        d = c["depth"]
        assert (d == hi).any() and (d == lo).any() and (d > hi).any() and (d < lo).any()
        assert (np.diff(d[0, 0], axis=-1) == 0).any() and (np.diff(d[0, 0], axis=-2) == 0).any()


@pytest.mark.parametrize("mode", R.MODES, ids=[m[0] for m in R.MODES])
def test_deterministic_and_stream_independent(gpu, mode):
    from splatter360_amd import depth_smooth
    _, second, sigma = mode
    depth, near, far, image = _tensors((1, 6, 64, 64), 6, gpu)
    runs = []
    for s in (None, torch.cuda.Stream(gpu), None):
        d = depth.clone().requires_grad_(True)
        if s is not None:
            s.wait_stream(torch.cuda.current_stream(gpu))
        ctx = torch.cuda.stream(s) if s is not None else torch.cuda.stream(torch.cuda.current_stream(gpu))
        with ctx:
            loss = depth_smooth.depth_smoothness_loss(d, near, far, image, sigma_image=sigma, use_second_derivative=second)
            loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), d.grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


def test_no_host_synchronisation(gpu):
    from splatter360_amd import depth_smooth
    depth, near, far, image = _tensors((1, 3, 17, 130), 3, gpu)
    d = depth.clone().requires_grad_(True)
    for _, second, sigma in R.MODES:                              # warm-up: the library, the allocator's blocks
        depth_smooth.depth_smoothness_loss(d, near, far, image, sigma_image=sigma, use_second_derivative=second, weight=0.5).backward()
    torch.cuda.synchronize()
    d.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _, second, sigma in R.MODES:
            depth_smooth.depth_smoothness_loss(d, near, far, image, sigma_image=sigma, use_second_derivative=second, weight=0.5).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(d.grad).all()


@pytest.mark.parametrize("mode", [R.MODES[0], R.MODES[3]], ids=lambda m: m[0])
def test_weight_is_a_plain_multiply(gpu, mode):
    from splatter360_amd import depth_smooth
    shape, vn = (2, 6, 5, 7), 6
    _, second, sigma = mode
    depth, near, far, image = _tensors(shape, vn, gpu)
    d1, d2 = depth.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    one = depth_smooth.depth_smoothness_loss(d1, near, far, image, sigma_image=sigma, use_second_derivative=second)
    quarter = depth_smooth.depth_smoothness_loss(d2, near, far, image, sigma_image=sigma, use_second_derivative=second, weight=0.25)
    assert torch.equal(quarter, 0.25 * one)
    one.backward()
    quarter.backward()
    assert torch.equal(d2.grad, 0.25 * d1.grad)                   # a power of two: the float64 chain scales exactly
    _check(quarter.detach() * 4, d2.grad, _want(shape, vn, mode, g=0.25), "weight 0.25")


@pytest.mark.parametrize("mode", R.MODES, ids=[m[0] for m in R.MODES])
def test_a_nan_pixel(gpu, mode):
    """One NaN pixel: the loss is NaN exactly when torch's is, and the gradient bar holds at every pixel whose stencil holds
    no NaN (the plus of radius 1 or 2 around the pixel)."""
    from splatter360_amd import depth_smooth
    shape, vn = (1, 3, 17, 130), 1
    _, second, sigma = mode
    depth, near, far, image = _tensors(shape, vn, gpu)
    depth = depth.clone()
    depth[0, 1, 8, 64] = float("nan")                             # at a wave boundary
    d = depth.clone().requires_grad_(True)
    loss = depth_smooth.depth_smoothness_loss(d, near, far, image, sigma_image=sigma, use_second_derivative=second)
    loss.backward()
    ref = R.torch_statement(depth, near, far, image, sigma, second)
    assert torch.isnan(loss).item() == torch.isnan(ref).item() and torch.isnan(loss).item()
    want = R.statement(depth.cpu().numpy(), near.log().cpu().numpy(), far.log().cpu().numpy(), image.cpu().numpy(), sigma, second)   # the device's logs
    r = 2 if second else 1
    clean = np.ones(shape, bool)
    clean[0, 1, 8 - r:8 + r + 1, 64] = False
    clean[0, 1, 8, 64 - r:64 + r + 1] = False
    err = np.abs(d.grad.double().cpu().numpy() - want["grad64"])
    assert np.isfinite(want["grad64"][clean]).all() and (err[clean] <= 2.0 ** -23 * want["A"][clean]).all()


def test_errors(gpu):
    from splatter360_amd import depth_smooth
    f = depth_smooth.depth_smoothness_loss
    depth, near, far, image = _tensors((2, 6, 5, 7), 1, gpu)
    with pytest.raises(RuntimeError):
        f(depth.cpu(), near.cpu(), far.cpu())
    with pytest.raises(RuntimeError):
        f(depth, near.cpu(), far)
    for bad in (lambda: f(depth[0], near, far),                                   # rank
                lambda: f(depth, near[0], far[0]),
                lambda: f(depth, near.expand(2, 4), far.expand(2, 4)),           # Vn = 4 does not divide V = 6
                lambda: f(depth, near, far.expand(2, 6)),                         # near and far differ
                lambda: f(depth, near[:1], far[:1]),                              # another batch size
                lambda: f(depth[..., :1], near, far),                             # W too small
                lambda: f(depth[..., :2, :], near, far, use_second_derivative=True),   # H too small for the mode
                lambda: f(depth, near, far, image.clone().requires_grad_(True), sigma_image=2.0),
                lambda: f(depth, near, far, sigma_image=2.0),                     # sigma without an image
                lambda: f(depth, near, far, image[..., :6], sigma_image=2.0),     # a mismatched image
                lambda: f(depth, near, far, image[:, :, 0], sigma_image=2.0),
                lambda: f(depth.double(), near, far),
                lambda: f(depth, near.double(), far.double()),
                lambda: f(depth, near, far, image.double(), sigma_image=2.0)):
        with pytest.raises(ValueError):
            bad()
    assert f(depth, near, far, image).item() == f(depth, near, far).item()       # an image without sigma_image is not read


def test_installed_wrapper_runs_the_kernels(gpu):
    from splatter360_amd import depth_smooth, plugin
    calls = []

    class LossDepth(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.cfg = cfg

        def forward(self, prediction, batch, gaussians, global_step):
            calls.append(global_step)
            return R.torch_statement(prediction.depth, batch["target"]["near"], batch["target"]["far"], batch["target"]["image"],
                                     self.cfg.sigma_image, self.cfg.use_second_derivative, self.cfg.weight)

    original = LossDepth.forward
    mod = types.ModuleType("loss_depth")
    mod.LossDepth = LossDepth
    fn = plugin.DEPTH_SMOOTH_SEAM.patch(mod)["forward"]
    assert LossDepth.__dict__["forward"] is fn and fn.replaced is original
    for vn in (1, 6):
        depth, near, far, image = _tensors((2, 6, 5, 7), vn, gpu)
        batch = {"target": {"near": near, "far": far, "image": image}}
        for _, second, sigma in R.MODES:
            loss_fn = LossDepth(types.SimpleNamespace(weight=0.05, sigma_image=sigma, use_second_derivative=second))
            d1, d2 = depth.clone().requires_grad_(True), depth.clone().requires_grad_(True)
            got = loss_fn(types.SimpleNamespace(depth=d1), batch, None, 7)
            direct = depth_smooth.depth_smoothness_loss(d2, near, far, image, sigma_image=sigma, use_second_derivative=second, weight=0.05)
            got.backward()
            direct.backward()
            assert torch.equal(got, direct) and torch.equal(d1.grad, d2.grad)
    assert not calls
    loss_fn = LossDepth(types.SimpleNamespace(weight=0.05, sigma_image=2.0, use_second_derivative=False))
    loss_fn(types.SimpleNamespace(depth=depth), {"target": {"near": near, "far": far, "image": image.clone().requires_grad_(True)}}, None, 1)
    loss_fn(types.SimpleNamespace(depth=depth.double()), {"target": {"near": near.double(), "far": far.double(), "image": image.double()}}, None, 2)
    loss_fn(types.SimpleNamespace(depth=depth.cpu()), {"target": {"near": near.cpu(), "far": far.cpu(), "image": image.cpu()}}, None, 3)
    assert calls == [1, 2, 3]
    LossDepth.forward = original


def test_through_the_rasteriser(gpu):
    """The wiring: a rendered "log" depth map, the loss with one bound per panorama, back to the Gaussians' means; against
    torch's chain of the same lines on the same rendered depth.  The two depth gradients agree to about 2e-6 A and the
    rasteriser's backward is linear in them; 1e-4 of the largest entry leaves room for cancellation in the per-Gaussian sums."""
    from splatter360_amd import cameras, decoder, depth_smooth, synthetic
    cloud = synthetic.uniform_cloud(500, seed=5, extent=3.0, scale_range=(0.03, 0.3))
    fw = 32
    ext = cameras.cube_face_extrinsics(torch.tensor(synthetic.target_pano_pose((0.1, -0.1, 0.2)))[None]).to(gpu)
    k = cameras.cube_face_intrinsics(1).to(gpu)
    near, far = torch.full((1, 6), 0.1, device=gpu), torch.full((1, 6), 10.0, device=gpu)
    pano_near, pano_far = near[:, :1].contiguous(), far[:, :1].contiguous()
    dec = decoder.DecoderSplattingFused().to(gpu)
    grads, depths = [], []
    for native in (True, False):
        gs = types.SimpleNamespace(**{key: torch.tensor(v, device=gpu)[None].requires_grad_(True) for key, v in cloud.items()})
        out = dec(gs, ext, k, near, far, (fw, fw), depth_mode="log")
        assert out.depth.shape == (1, 6, fw, fw)
        if native:
            loss = depth_smooth.depth_smoothness_loss(out.depth, pano_near, pano_far, use_second_derivative=True)
        else:
            loss = R.torch_statement(out.depth, pano_near, pano_far, second=True)
        loss.backward()
        grads.append(gs.means.grad)
        depths.append(out.depth.detach())
    assert torch.equal(depths[0], depths[1])
    a, b = grads
    assert torch.isfinite(a).all() and a.abs().max().item() > 0
    scale = b.abs().max().item()
    print("means.grad: largest", scale, "difference", (a - b).abs().max().item() / scale)
    assert (a - b).abs().max().item() <= 1e-4 * scale
