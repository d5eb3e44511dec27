"""The numpy SSIM statement (tests/ssim_reference.py) that tests/test_gpu_ssim.py holds the kernel to, pinned on CPU: its
window is scipy's, the score of the interior does not depend on the padding (what lets the kernel skip the border), the
identities of the index hold, and — where skimage is installed — it is skimage's structural_similarity as the reference calls it."""
import numpy as np
import pytest

import ssim_reference as R


def _pair(shape, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32)
    y = np.clip(x + 0.1 * rng.standard_normal(shape).astype(np.float32), -0.2, 1.3).astype(np.float32)
    return x, y


def test_window_is_scipys_gaussian_filter1d():
    ndimage = pytest.importorskip("scipy.ndimage")
    impulse = np.zeros(21)
    impulse[10] = 1.0
    resp = ndimage.gaussian_filter1d(impulse, sigma=R.SIGMA, truncate=R.TRUNCATE, mode="constant")
    w = R.gaussian_weights()
    assert len(w) == 11 and R.RADIUS == 5
    np.testing.assert_allclose(resp[5:16], w[::-1], rtol=0, atol=1e-15)
    assert np.all(resp[:5] == 0) and np.all(resp[16:] == 0)


def test_filter_equals_scipys_gaussian_filter_with_reflect():
    ndimage = pytest.importorskip("scipy.ndimage")
    x, _ = _pair((1, 1, 23, 31))
    want = ndimage.gaussian_filter(x[0, 0].astype(np.float64), sigma=R.SIGMA, truncate=R.TRUNCATE, mode="reflect")
    np.testing.assert_allclose(R._filter(x.astype(np.float64), np.float64, "symmetric")[0, 0], want, rtol=0, atol=1e-14)
    want32 = ndimage.gaussian_filter(x[0, 0], sigma=R.SIGMA, truncate=R.TRUNCATE, mode="reflect")
    np.testing.assert_allclose(R._filter(x, np.float32, "symmetric")[0, 0], want32, rtol=0, atol=2e-7)


@pytest.mark.parametrize("shape", [(2, 3, 11, 11), (1, 3, 12, 13), (2, 1, 37, 41)])
def test_padding_never_reaches_the_cropped_mean(shape):
    """Every interior pixel's 11 x 11 window lies inside the image: reflect and zero padding give the same score."""
    x, y = _pair(shape, seed=1)
    for dt in (np.float32, np.float64):
        a = R.ssim(x, y, dt, pad_mode="symmetric")
        b = R.ssim(x, y, dt, pad_mode="constant")
        assert np.array_equal(a, b), (a, b)
    # ... while the border itself does depend on it (the crop is what removes it)
    assert not np.array_equal(R.ssim_map(x, y, pad_mode="symmetric"), R.ssim_map(x, y, pad_mode="constant"))


def test_identities():
    x, y = _pair((3, 3, 20, 24), seed=2)
    for dt in (np.float32, np.float64):
        np.testing.assert_allclose(R.ssim(x, x, dt), 1.0, rtol=0, atol=1e-6)
        const = np.full_like(x, 0.37)
        np.testing.assert_allclose(R.ssim(const, const, dt), 1.0, rtol=0, atol=1e-7)
        assert np.array_equal(R.ssim(x, y, dt), R.ssim(y, x, dt))
    s = R.ssim(x, y)
    assert np.all(s < 1.0) and np.all(s > 0.0)
    with pytest.raises(ValueError):
        R.ssim(x[..., :10, :], y[..., :10, :])
    with pytest.raises(ValueError):
        R.ssim(x, y[:2])


def test_float32_statement_is_close_to_float64():
    x, y = _pair((2, 3, 64, 64), seed=3)
    assert np.abs(R.ssim(x, y, np.float32) - R.ssim(x, y)).max() <= 1e-6


def test_equals_skimage_structural_similarity():
    metrics = pytest.importorskip("skimage.metrics")
    x, y = _pair((3, 3, 40, 52), seed=4)
    ours = R.ssim(x, y, np.float32)
    for i in range(x.shape[0]):
        want = metrics.structural_similarity(x[i], y[i], win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
        assert abs(ours[i] - want) <= 1e-6, (i, ours[i], want)
