"""s360_ssim (csrc/s360_metrics.hip) through splatter360_amd.metrics, against the float64 numpy statement of skimage's
structural_similarity (tests/ssim_reference.py; its fidelity to skimage is pinned in tests/test_ssim_spec.py).

Bar: |kernel - float64 statement| <= 1e-5 per image.  Every parity case also puts the float32 statement (skimage's own
arithmetic) inside the same bar, so the bar is one skimage itself meets."""
import numpy as np
import pytest
import torch

import ssim_reference as R

pytestmark = pytest.mark.gpu

BAR = 1e-5


def _check(x: torch.Tensor, y: torch.Tensor, got: torch.Tensor = None) -> float:
    from splatter360_amd import metrics
    if got is None:
        got = metrics.ssim(x, y)
    assert got.dtype == torch.float32 and got.shape == (x.shape[0],) and got.device == x.device
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    want = R.ssim(xn, yn)
    err32 = np.abs(R.ssim(xn, yn, np.float32) - want).max()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    assert err32 <= BAR, f"the float32 statement misses the bar: {err32}"
    assert err <= BAR, (err, err32)
    print(f"shape {tuple(x.shape)}: kernel {err:.2e} float32 statement {err32:.2e} from float64")
    return err


def _rendered_faces(dev, w=256):
    """The evaluation shape: six 256 x 256 cube faces of three target panoramas, rendered by the fused path -> [18,3,w,w]."""
    from splatter360_amd import decoder, synthetic
    cloud = synthetic.encoder_like_cloud(128, 256, seed=5)
    ps = [torch.tensor(cloud[k], device=dev) for k in ("means", "covariances", "harmonics", "opacities")]
    faces = []
    with torch.no_grad():
        for pos in ((0.0, 0.0, 0.0), (0.3, -0.1, 0.2), (-0.2, 0.15, -0.3)):
            pano = torch.from_numpy(synthetic.target_pano_pose(pos)).to(dev)
            ext, K, near, far = decoder.cube_cameras(pano, 0.1, 10.0)
            faces.append(decoder.render_views_fused(ext, K, near, far, (w, w), torch.zeros(3, device=dev), *ps, shared_campos=True))
    return torch.cat(faces).contiguous()


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def test_evaluation_shape_rendered_faces(gpu):
    pred = _rendered_faces(gpu)
    assert pred.shape == (18, 3, 256, 256) and torch.isfinite(pred).all()
    noise = torch.randn(pred.shape, generator=_gen(1)).to(gpu)
    gt = (torch.roll(pred, shifts=(1, -2), dims=(2, 3)) + 0.02 * noise).contiguous()     # a perturbed copy: shifted, noisy
    _check(pred, gt)


def test_evaluation_shape_uniform_noise(gpu):
    x = torch.rand((18, 3, 256, 256), generator=_gen(2)).to(gpu)
    y = torch.rand((18, 3, 256, 256), generator=_gen(3)).to(gpu)
    _check(x, y)


def test_evaluation_shape_near_flat(gpu):
    """0.9 + 1e-3 U: <x^2> - mx^2 cancels in float32 against C2 = 9e-4 — the hardest case for precision."""
    x = 0.9 + 1e-3 * torch.rand((18, 3, 256, 256), generator=_gen(4))
    y = 0.9 + 1e-3 * torch.rand((18, 3, 256, 256), generator=_gen(5))
    _check(x.to(gpu), y.to(gpu))
    _check(x.to(gpu), (x + 2e-4 * torch.randn(x.shape, generator=_gen(6))).to(gpu))


@pytest.mark.parametrize("shape", [(1, 1, 11, 11), (18, 3, 11, 11), (18, 3, 12, 13), (55, 1, 64, 64), (55, 3, 64, 64),
                                   (1, 3, 37, 301), (18, 1, 37, 301), (1, 1, 512, 512), (6, 3, 512, 512)])
def test_shapes(gpu, shape):
    """One interior pixel (11 x 11), sizes that are no tile multiple, configs[0]'s 64 x 64 and configs[4]'s 512 x 512 faces;
    values outside [0, 1] (rendered colours are not clipped)."""
    x = 1.4 * torch.rand(shape, generator=_gen(7)) - 0.2
    y = (x + 0.15 * torch.randn(shape, generator=_gen(8))) * 1.05
    _check(x.to(gpu), y.to(gpu))


def test_identities_and_errors(gpu):
    from splatter360_amd import metrics
    x = torch.rand((5, 3, 40, 33), generator=_gen(9)).to(gpu)
    assert (metrics.ssim(x, x) - 1.0).abs().max().item() <= 1e-6
    const = torch.full((2, 1, 16, 16), 0.4, device=gpu)
    assert (metrics.ssim(const, const) - 1.0).abs().max().item() <= 1e-6
    y = torch.rand((5, 3, 40, 33), generator=_gen(10)).to(gpu)
    assert torch.equal(metrics.ssim(x, y), metrics.ssim(y, x))
    for shape in ((5, 3, 10, 33), (5, 3, 40, 10)):
        a = torch.rand(shape, device=gpu)
        with pytest.raises(ValueError):
            metrics.ssim(a, a)
    with pytest.raises(ValueError):
        metrics.ssim(x, y[:4])
    with pytest.raises(ValueError):
        metrics.ssim(x[0], y[0])
    with pytest.raises(RuntimeError):
        metrics.ssim(x.cpu(), y.cpu())
    # non-contiguous and half inputs are converted (.float().contiguous())
    xt = x.transpose(2, 3)
    assert torch.equal(metrics.ssim(xt, y.transpose(2, 3)), metrics.ssim(xt.contiguous(), y.transpose(2, 3).contiguous()))
    h = metrics.ssim(x.half(), y.half())
    assert h.dtype == torch.float32 and torch.equal(h, metrics.ssim(x.half().float(), y.half().float()))


def test_determinism_and_batch_independence(gpu):
    from splatter360_amd import metrics
    x = torch.rand((18, 3, 256, 256), generator=_gen(11)).to(gpu)
    y = (x + 0.1 * torch.randn(x.shape, generator=_gen(12)).to(gpu)).contiguous()
    a = metrics.ssim(x, y)
    b = metrics.ssim(x, y)
    assert torch.equal(a, b)
    for i in range(x.shape[0]):
        assert torch.equal(metrics.ssim(x[i:i + 1], y[i:i + 1])[0], a[i]), i


def test_non_default_stream(gpu):
    from splatter360_amd import metrics
    x = torch.rand((18, 3, 256, 256), generator=_gen(13)).to(gpu)
    y = torch.rand((18, 3, 256, 256), generator=_gen(14)).to(gpu)
    want = metrics.ssim(x, y)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        xs, ys = x * 1.0, y * 1.0                       # produced on s: the call must run after them, on s
        got = metrics.ssim(xs, ys)
    torch.cuda.current_stream(gpu).wait_stream(s)
    assert torch.equal(got, want)
    _check(x, y, got)


def test_reference_contract(gpu):
    """compute_ssim(ground_truth, predicted) -> [b] with predicted's dtype and device (metrics.py:38-54)."""
    from splatter360_amd import metrics
    gt = torch.rand((4, 3, 32, 32), generator=_gen(15)).to(gpu)
    pred = torch.rand((4, 3, 32, 32), generator=_gen(16)).to(gpu)
    got = metrics.compute_ssim(gt, pred)
    assert got.shape == (4,) and got.dtype == pred.dtype and got.device == pred.device
    assert torch.equal(got, metrics.ssim(pred, gt))
    got16 = metrics.compute_ssim(gt, pred.half())
    assert got16.dtype == torch.float16 and got16.device == pred.device
    _check(pred, gt, got)


def test_patched_compute_ssim_through_the_seam(gpu, monkeypatch):
    """install(metrics=True)'s replacement: the native score for GPU tensors, the replaced function for CPU tensors."""
    import sys
    import types

    from splatter360_amd import metrics, plugin
    calls = []

    def replaced(ground_truth, predicted):
        calls.append(ground_truth.device)
        return torch.full((ground_truth.shape[0],), -1.0, dtype=predicted.dtype, device=predicted.device)

    mod = types.ModuleType(plugin.METRICS_MODULE)
    mod.compute_ssim = replaced
    monkeypatch.setitem(sys.modules, plugin.METRICS_MODULE, mod)
    fn = plugin.install_metrics()
    assert mod.compute_ssim is fn and fn.replaced is replaced
    gt = torch.rand((6, 3, 64, 64), generator=_gen(17)).to(gpu)
    pred = torch.rand((6, 3, 64, 64), generator=_gen(18)).to(gpu)
    got = mod.compute_ssim(gt, pred)
    assert not calls and torch.equal(got, metrics.compute_ssim(gt, pred))
    _check(pred, gt, got)
    assert mod.compute_ssim(gt.cpu(), pred.cpu()).tolist() == [-1.0] * 6 and len(calls) == 1
