"""The bucket path of the tile sort (block_bucket_sort in k_sort_stage1) under controlled depth distributions, driven and checked
the way tests/test_gpu_sort_one_launch.py drives the sort: every splat sits well inside ONE 16x16 tile of an identity camera, so
a tile's key multiset is (float bits of the pair's depth) << 32 | pair for the Gaussians placed on it, and `keys`, `list`,
`tile_start` must be exactly the host's sort of it, with the sort's error word 0.  What is new here is the depth of every splat:
log-uniform lists (the bucket path), lists at ONE depth (every key in one bucket: ties broken by the pair index, through the
merge-sort branch when the list is longer than S360_SORT_BMAX and through the bucket path when it is not), a tight cluster plus one
far splat (the range stretched by an outlier: nearly everything in bucket 0), and all of them next to chunked lists in one launch."""
import numpy as np
import pytest
import torch

from test_gpu_sort_one_launch import _check, _render, _views

pytestmark = pytest.mark.gpu


def _cloud(hw, depths, seed):
    """depths[t]: the view depths of the splats on tile t (identity camera: depth == z, exactly, in float32).  Otherwise the cloud
    of tests/test_gpu_sort_one_launch.py: centres within 2 px of the tile's centre, 3-sigma radius 2 px, tiles interleaved."""
    rng = np.random.default_rng(seed)
    gx = hw // 16
    tile = np.repeat(np.arange(len(depths)), [len(d) for d in depths])
    z = np.concatenate([np.asarray(d, np.float32) for d in depths]).astype(np.float64)
    n = tile.size
    px = (tile % gx) * 16 + 8 + rng.uniform(-2.0, 2.0, n)
    py = (tile // gx) * 16 + 8 + rng.uniform(-2.0, 2.0, n)
    means = np.stack([((2 * px + 1) / hw - 1) * z, ((2 * py + 1) / hw - 1) * z, z], 1)
    s = 0.25 / hw
    cov6 = np.tile(np.array([[s * s, 0, 0, s * s, 0, s * s]]), (n, 1)) * (z[:, None] ** 2)
    perm = rng.permutation(n)
    return tile[perm], means[perm], cov6[perm], rng.uniform(0, 1, (n, 3)), rng.uniform(0.01, 0.02, (n, 1))


def _log_uniform(n, seed):
    return np.exp(np.random.default_rng(seed).uniform(np.log(2.0), np.log(30.0), n))


def _cluster_and_outlier(n, seed):
    z = 5.0 + np.random.default_rng(seed).uniform(-1e-3, 1e-3, n)
    z[n // 3] = 29.0
    return z


def _depth_words(got, cloud, t):
    """the distinct depth words the device computed for the splats of tile t (view 0)"""
    return np.unique(got["depths"].cpu().numpy().view(np.uint32).reshape(-1)[: cloud[0].size][cloud[0] == t])


def _run(gpu, hw, depths, seed):
    cloud = _cloud(hw, depths, seed)
    st, got = _render(hw, cloud, _views(hw, gpu), gpu)
    assert np.diff(got["tile_start"].cpu().numpy())[: len(depths)].tolist() == [len(d) for d in depths]
    _check(hw, cloud, 1, st, got)
    return cloud, got


@pytest.mark.parametrize("n", [1, 2, 64, 65, 2047, 2048])
def test_log_uniform_list(gpu, n):
    _run(gpu, 32, [_log_uniform(n, n)], seed=n)


@pytest.mark.parametrize("n", [20, 1500])
def test_list_at_one_depth(gpu, n):
    """Every key of the list has the same high word: the order is the pair index's."""
    cloud, got = _run(gpu, 32, [np.full(n, 3.25)], seed=n)
    assert _depth_words(got, cloud, 0).size == 1


def test_two_depths(gpu):
    cloud, got = _run(gpu, 32, [np.where(np.arange(1456) % 3 == 0, 2.0, 7.5)], seed=3)
    assert _depth_words(got, cloud, 0).size == 2


def test_cluster_and_one_far_splat(gpu):
    cloud, got = _run(gpu, 32, [_cluster_and_outlier(1456, 4)], seed=4)
    w = _depth_words(got, cloud, 0).astype(np.int64)
    assert w[-1] - w[-2] > 2048 * (w[-2] - w[0])      # the outlier stretches the range: the cluster shares the lowest bucket


MIXED = [_log_uniform(1456, 11), _cluster_and_outlier(1456, 12), _log_uniform(2049, 13), _log_uniform(5000, 14)]


def test_every_role_in_one_launch(gpu):
    """A bucket-path list, a list that takes the merge-sort branch, a one-chunk list and a two-chunk list (chunk blocks + a merge
    unit) side by side."""
    _run(gpu, 32, MIXED, seed=5)


def test_two_calls_are_bit_identical(gpu):
    cloud = _cloud(32, MIXED, seed=5)
    views = _views(32, gpu)
    _, a = _render(32, cloud, views, gpu)
    _, b = _render(32, cloud, views, gpu)
    for k in ("keys", "list", "tile_start"):
        assert torch.equal(a[k], b[k]), k
