"""The context-depth loss kernels (csrc/s360_depth_loss.hip) through splatter360_amd.depth_loss, against torch's own expressions
of the reference's erode / compute_l1_sphere_loss (src/model/model_wrapper_helper.py) on the same GPU and against the float64
statement (float32 terms, float64 sums, as tests/depth_loss_reference.py states it; its fidelity to the reference is pinned in
tests/test_depth_loss_spec.py).

Bars: erode bit-identical; loss within 2 ulp of the float64 quotient and 1e-5 relative of torch's float32 path; gradients
bit-identical to torch's autograd chain evaluated with the kernel's clamped denominator; the fused closure bit-identical to
erode + compute_l1_sphere_loss."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(14, 2, 512, 1024), (2, 2, 256, 512), (1, 3, 37, 129), (3, 1, 5, 7), (2, 2, 33, 260)]


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def torch_erode(x, k=5):
    """The reference's erode, restated with the same torch calls."""
    pad = (k - 1) // 2
    return 1 - F.max_pool2d(F.pad(1 - x, pad=[pad, pad, pad, pad], mode="reflect"), kernel_size=k, stride=1, padding=0)


def torch_weights(h, dev):
    w = torch.arange(0, h, dtype=torch.float32, device=dev)
    return torch.sin((w + 0.5) * torch.pi / h)


def torch_clamp(den):
    z = torch.tensor(0.0, device=den.device)
    return torch.where(torch.ge(den, z), torch.max(den, z + 1e-10), torch.min(den, z - 1e-10))


def torch_loss(p, t, m, keep_batch=False, den_override=None):
    """The reference's compute_l1_sphere_loss in torch (float32 sums); den_override: divide by this clamped den instead."""
    b, v, h, w = p.shape
    sp = torch_weights(h, p.device).view(1, 1, h, 1).expand(b, v, h, w) * m
    axes = (1, 2, 3) if keep_batch else (0, 1, 2, 3)
    num = torch.sum(torch.abs(t - p) * sp, dim=axes)
    den = torch_clamp(torch.sum(sp, dim=axes)) if den_override is None else den_override.reshape(num.shape)
    return num / den


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _case(shape, dev, seed=0, hole_frac=0.05):
    g = _gen(seed)
    depth = torch.rand(shape, generator=g) * 20.0 + 0.2
    holes = torch.rand(shape, generator=g)
    depth[holes < hole_frac] = 0.0
    depth[(holes >= hole_frac) & (holes < 1.5 * hole_frac)] = 0.05
    pred = torch.rand(shape, generator=g) * 20.0
    return pred.to(dev), depth.to(dev)


def _inputs(shape, dev, seed=0):
    pred, depth = _case(shape, dev, seed)
    far = torch.tensor([[100.0]], device=dev)
    mask = (depth > 0.1).float()
    b, v, h, w = shape
    mask = torch_erode(mask.view(b * v, 1, h, w)).view(shape) if min(h, w) > 2 else mask
    target = torch.where(depth < 1e-7, far[0, 0], depth)
    return pred, target, mask, depth, far


ERODE_SHAPES = [(1, 1, 3, 3), (2, 3, 5, 7), (2, 1, 37, 129), (1, 1, 64, 1030), (4, 1, 17, 300)]


# pad < H and W (torch's reflect pad refuses the rest too); ksize 19 takes the direct-window kernel
@pytest.mark.parametrize("shape,k", [(s, k) for s in ERODE_SHAPES for k in (1, 3, 5, 7, 19) if (k - 1) // 2 < min(s[2:])])
def test_erode_bit_identical_to_torch(gpu, shape, k):
    from splatter360_amd import depth_loss
    g = _gen(k * 100 + shape[-1])
    x = (torch.rand(shape, generator=g) > 0.2).float()
    y = torch.randn(shape, generator=g) * 3.0
    flat = y.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=g)
    flat[idx[: max(1, n // 50)]] = float("nan")
    flat[idx[n // 50: n // 50 + max(1, n // 50)]] = float("inf")
    flat[idx[2 * (n // 50): 2 * (n // 50) + max(1, n // 50)]] = float("-inf")
    for inp in (x, y):
        inp = inp.to(gpu)
        got = depth_loss.erode(inp, k)
        assert _bits_equal(got, torch_erode(inp, k)), (shape, k)
        assert _bits_equal(depth_loss.erode(inp[0], k), torch_erode(inp[0], k))      # [C,H,W]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("keep_batch", [False, True])
def test_forward_and_backward(gpu, shape, keep_batch):
    from splatter360_amd import depth_loss
    pred, target, mask, _, _ = _inputs(shape, gpu, seed=sum(shape))
    p = pred.clone().requires_grad_(True)
    t = target.clone().requires_grad_(True)
    loss = depth_loss.compute_l1_sphere_loss(p, t, mask, keep_batch=keep_batch)
    assert loss.dtype == torch.float32 and loss.shape == ((shape[0],) if keep_batch else ())
    # the float64 statement: float32 terms, float64 sums
    b, v, h, w = shape
    sp = torch_weights(h, gpu).view(1, 1, h, 1).expand(*shape) * mask
    axes = (1, 2, 3) if keep_batch else (0, 1, 2, 3)
    num64 = (torch.abs(target - pred) * sp).double().sum(dim=axes)
    den64 = sp.double().sum(dim=axes).clamp_min(1e-10)
    want64 = (num64 / den64).cpu().numpy()
    got = loss.detach().cpu().numpy()
    ulp = np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want64) <= 2 * ulp).all(), (got, want64)
    ref32 = torch_loss(pred, target, mask, keep_batch).cpu().numpy()
    assert (np.abs(got - ref32) <= 1e-5 * np.abs(ref32)).all(), (got, ref32)
    # gradients: torch's own chain, with the kernel's den'
    gin = torch.rand(loss.shape, generator=_gen(7)).to(gpu) + 0.5
    loss.backward(gin)
    den = depth_loss._forward(pred, target, mask, keep_batch, None, 0.0, 0.0, 1)[1]
    p2, t2 = pred.clone().requires_grad_(True), target.clone().requires_grad_(True)
    torch_loss(p2, t2, mask, keep_batch, den_override=den).backward(gin)
    assert _bits_equal(p.grad, p2.grad) and _bits_equal(t.grad, t2.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_closure_bit_identical_to_the_two_step_path(gpu, shape):
    from splatter360_amd import depth_loss
    pred, target, mask, depth, far = _inputs(shape, gpu, seed=3 + shape[-1])
    depth_in = depth.clone()
    p1 = pred.clone().requires_grad_(True)
    fused = depth_loss.context_depth_loss(p1, depth, far[0, 0])
    assert torch.equal(depth, depth_in)                                   # not modified in place
    b, v, h, w = shape
    m2 = depth_loss.erode((depth > 0.1).float().view(b * v, 1, h, w)).view(shape)
    assert torch.equal(m2, mask)
    p2 = pred.clone().requires_grad_(True)
    two = 0.1 * depth_loss.compute_l1_sphere_loss(p2, target, m2)
    assert _bits_equal(fused, two), (fused, two)
    fused.backward()
    two.backward()
    assert _bits_equal(p1.grad, p2.grad)
    # and the reference's conditional erosion on a depth without holes
    dense = depth.clamp_min(0.2)
    a = depth_loss.context_depth_loss(pred, dense, far[0, 0])
    b_ = 0.1 * depth_loss.compute_l1_sphere_loss(pred, dense, torch.ones_like(dense))
    assert _bits_equal(a, b_)


def test_deterministic_and_stream_independent(gpu):
    from splatter360_amd import depth_loss
    pred, target, mask, depth, far = _inputs((2, 2, 256, 512), gpu, seed=11)
    runs = []
    for s in (None, torch.cuda.Stream(gpu), None):
        p = pred.clone().requires_grad_(True)
        if s is not None:
            s.wait_stream(torch.cuda.current_stream(gpu))
        ctx = torch.cuda.stream(s) if s is not None else torch.cuda.stream(torch.cuda.current_stream(gpu))
        with ctx:
            l1 = depth_loss.compute_l1_sphere_loss(p, target, mask, keep_batch=True)
            l1.sum().backward()
            l2 = depth_loss.context_depth_loss(pred, depth, far)
        torch.cuda.synchronize()
        runs.append((l1.detach().clone(), p.grad.clone(), l2.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))


def test_keep_batch_elements_are_independent(gpu):
    from splatter360_amd import depth_loss
    pred, target, mask, _, _ = _inputs((4, 2, 64, 128), gpu, seed=21)
    full = depth_loss.compute_l1_sphere_loss(pred, target, mask, keep_batch=True)
    for i in range(4):
        one = depth_loss.compute_l1_sphere_loss(pred[i:i + 1], target[i:i + 1], mask[i:i + 1], keep_batch=True)
        assert torch.equal(one[0], full[i])
    other = pred.clone()
    other[1:] = 0.0
    assert torch.equal(depth_loss.compute_l1_sphere_loss(other, target, mask, keep_batch=True)[0], full[0])


def test_edge_denominators(gpu):
    from splatter360_amd import depth_loss
    pred, target, mask, _, _ = _inputs((3, 2, 16, 48), gpu, seed=5)
    m = mask.clone()
    m[1] = 0.0                                                            # an all-zero mask: den' = 1e-10, loss 0
    m[2] = -m[2]                                                          # a negative mask: den' <= -1e-10
    got = depth_loss.compute_l1_sphere_loss(pred, target, m, keep_batch=True)
    want = torch_loss(pred, target, m, keep_batch=True)
    den = depth_loss._forward(pred, target, m, True, None, 0.0, 0.0, 1)[1]
    assert got[1].item() == 0.0 and den[1].item() == np.float32(1e-10) and den[2].item() < 0 and den[0].item() > 0
    assert torch.allclose(got, want, rtol=1e-5, atol=0)


def test_non_finite_inputs_follow_the_reference(gpu):
    from splatter360_amd import depth_loss
    shape = (3, 1, 16, 64)
    pred, target, mask, _, _ = _inputs(shape, gpu, seed=9)
    pred, mask = pred.clone(), mask.clone()
    pred[0, 0, 3, 5] = float("nan")                                       # element 0: NaN, even where the mask is 0
    mask[0, 0, 3, 5] = 0.0
    pred[1, 0, 4, 6] = float("inf")                                       # element 1: inf with weight > 0
    mask[1, 0, 4, 6] = 1.0
    target[2, 0, 7, 8] = float("inf")                                     # element 2: inf with weight 0 -> inf * 0 = NaN
    mask[2, 0, 7, 8] = 0.0
    p = pred.clone().requires_grad_(True)
    got = depth_loss.compute_l1_sphere_loss(p, target, mask, keep_batch=True)
    want = torch_loss(pred, target, mask, keep_batch=True)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want)), (got, want)
    assert torch.isnan(got[0]) and torch.isinf(got[1]) and torch.isnan(got[2])
    got.sum().backward()
    den = depth_loss._forward(pred, target, mask, True, None, 0.0, 0.0, 1)[1]
    p2 = pred.clone().requires_grad_(True)
    torch_loss(p2, target, mask, True, den_override=den).sum().backward()
    assert _bits_equal(p.grad, p2.grad)


def test_no_host_synchronisation(gpu):
    from splatter360_amd import depth_loss
    pred, target, mask, depth, far = _inputs((2, 2, 64, 128), gpu, seed=2)
    p = pred.clone().requires_grad_(True)
    depth_loss.context_depth_loss(p, depth, far[0, 0]).backward()          # warm-up: caches, workspace sizes
    torch.cuda.synchronize()
    p.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        depth_loss.context_depth_loss(p, depth, far[0, 0]).backward()
        l = depth_loss.compute_l1_sphere_loss(p, target, mask, keep_batch=True)
        l.sum().backward()
        depth_loss.erode(mask)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def test_errors(gpu):
    from splatter360_amd import depth_loss
    pred, target, mask, depth, far = _inputs((1, 1, 8, 8), gpu)
    with pytest.raises(NotImplementedError):
        depth_loss.compute_l1_sphere_loss(pred, target)
    with pytest.raises(RuntimeError):
        depth_loss.compute_l1_sphere_loss(pred.cpu(), target.cpu(), mask.cpu())
    with pytest.raises(ValueError):
        depth_loss.compute_l1_sphere_loss(pred, target, mask[..., :4])
    with pytest.raises(ValueError):
        depth_loss.compute_l1_sphere_loss(pred.double(), target.double(), mask.double())
    with pytest.raises(ValueError):
        depth_loss.erode(mask, 4)
    with pytest.raises(ValueError):
        depth_loss.erode(mask, 17)
    with pytest.raises(ValueError):
        depth_loss.context_depth_loss(pred, depth, far, ksize=19)


def test_installed_wrappers_run_the_kernels(gpu):
    import types
    from splatter360_amd import depth_loss, plugin
    mod = types.ModuleType("helper")
    calls = []

    def erode(bin_img, ksize=5):
        calls.append("erode")
        return torch_erode(bin_img, ksize)

    def compute_l1_sphere_loss(y_pred, y_true, mask=None, keep_batch=False):
        calls.append("loss")
        return torch_loss(y_pred, y_true, mask, keep_batch)

    mod.erode, mod.compute_l1_sphere_loss = erode, compute_l1_sphere_loss
    fns = plugin.DEPTH_LOSS_SEAM.patch(mod)
    pred, target, mask, depth, _ = _inputs((2, 2, 32, 64), gpu, seed=4)
    m = (depth > 0.1).float().view(4, 1, 32, 64)
    assert _bits_equal(mod.erode(m), depth_loss.erode(m))
    assert torch.equal(mod.compute_l1_sphere_loss(pred, target, mask=mask), depth_loss.compute_l1_sphere_loss(pred, target, mask))
    assert not calls and fns["erode"].replaced is erode
    mod.erode(m, 4)                                                       # an even ksize: the replaced function
    mod.compute_l1_sphere_loss(pred, target, mask=mask[:1])               # a broadcastable mask: the replaced function
    mod.compute_l1_sphere_loss(pred, target, mask=mask.clone().requires_grad_(True))
    assert calls == ["erode", "loss", "loss"]
