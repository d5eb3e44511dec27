"""The one-launch tile sort (k_sort_stage1: chunk blocks, merge blocks, short-list blocks, the global-memory fallback as the merge
blocks' last role) against the host's sort of the emitted keys.  Every splat of these scenes sits well inside ONE 16x16 tile, so the
key multiset of a tile is known without an oracle: (float bits of the pair's depth) << 32 | pair, for the Gaussians placed on that
tile.  `keys`, `list` and `tile_start` of the call must be exactly np.sort of that multiset per tile, and the sort's error word
(RasterState.sort_errors, part of split_errors) must be zero.  List lengths sit on the edges of every class: one chunk, 2 .. 16
chunks with ragged last runs (1 .. 4 merge passes, both ping-pong parities), and beyond the pass budget."""
import numpy as np
import pytest
import torch

from helpers import small_front_scene
from splatter360_amd import rasterizer

pytestmark = pytest.mark.gpu


def _cloud(hw, counts, seed):
    """counts[t] splats on tile t of a hw x hw image: centres within 2 px of the tile's centre, 3-sigma radius 2 px."""
    rng = np.random.default_rng(seed)
    gx = hw // 16
    tile = np.repeat(np.arange(len(counts)), counts)
    n = tile.size
    px = (tile % gx) * 16 + 8 + rng.uniform(-2.0, 2.0, n)
    py = (tile // gx) * 16 + 8 + rng.uniform(-2.0, 2.0, n)
    z = rng.uniform(2.0, 30.0, n)
    means = np.stack([((2 * px + 1) / hw - 1) * z, ((2 * py + 1) / hw - 1) * z, z], 1)
    s = 0.25 / hw                                                     # sigma = 0.125 px (+ the 0.3 px^2 dilation): radius 2
    cov6 = np.tile(np.array([[s * s, 0, 0, s * s, 0, s * s]]), (n, 1)) * (z[:, None] ** 2)
    perm = rng.permutation(n)                                         # tiles interleaved in Gaussian order
    return tile[perm], means[perm], cov6[perm], rng.uniform(0, 1, (n, 3)), rng.uniform(0.01, 0.02, (n, 1))


def _views(hw, dev, rolled=False):
    S, _, _, _, _ = small_front_scene(n=2, seed=0, h=hw, w=hw)
    vm, pm = [np.asarray(S["viewmatrix"], np.float32)], [np.asarray(S["projmatrix"], np.float32)]
    if rolled:   # a second camera rolled by 180 degrees about its axis: pixel (x, y) -> (hw - 1 - x, hw - 1 - y), depths unchanged
        R = np.diag([-1.0, -1.0, 1.0, 1.0]).astype(np.float32)
        vm.append(R @ vm[0])
        pm.append(R @ pm[0])
    t = lambda a: torch.tensor(np.stack(a), device=dev)
    return rasterizer.pack_views(t(vm), t(pm), torch.zeros(3, device=dev), 1.0, 1.0, torch.tensor([0.1, 0.2, 0.3], device=dev))


def _render(hw, cloud, views, dev):
    _, means, cov6, colors, opac = cloud
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    rasterizer.rasterize_views(t(means), t(cov6), t(opac), None, t(colors), views=views, image_height=hw, image_width=hw, sh_degree=0,
                               shared_campos=True)
    st = rasterizer.last_state()
    L = st.num_rendered()
    ts = st.tensors()
    return st, dict(keys=ts["keys"][:L].clone(), list=ts["list"][:L].clone(), tile_start=ts["tile_start"].clone(), depths=ts["depths"].clone())


def _check(hw, cloud, nviews, st, got):
    tile = cloud[0]
    P, T, gx = tile.size, (hw // 16) ** 2, hw // 16
    depths = got["depths"].cpu().numpy().view(np.uint32).reshape(nviews, P).astype(np.uint64)
    keys = got["keys"].cpu().numpy().view(np.uint64)
    lst = got["list"].cpu().numpy().view(np.uint32)
    start = got["tile_start"].cpu().numpy().astype(np.int64)
    want_keys, want_start = [], [0]
    for v in range(nviews):
        # view 1 is the rolled camera: tile (tx, ty) -> (gx - 1 - tx, gx - 1 - ty) == T - 1 - t
        tv = tile if v == 0 else T - 1 - tile
        emitted = (depths[v] << np.uint64(32)) | (np.uint64(v * P) + np.arange(P, dtype=np.uint64))
        for t in range(T):
            k = np.sort(emitted[tv == t])
            want_keys.append(k)
            want_start.append(want_start[-1] + k.size)
    want_keys = np.concatenate(want_keys)
    assert gx * gx == T and start.size == nviews * T + 1
    np.testing.assert_array_equal(start, np.asarray(want_start))
    assert np.unique(want_keys).size == want_keys.size               # unique keys: ONE ascending order per tile
    np.testing.assert_array_equal(keys, want_keys)
    np.testing.assert_array_equal(lst, (want_keys & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert st.sort_errors() == 0 and st.split_errors() == 0


# 2 049 / 4 096: one chunk, no pass; 4 097 .. 8 192: one pass; .. 16 384: two; 16 385, 20 001: three; 32 769: four (nine chunks);
# 66 000: beyond SORT_CHUNK << MAX_PASSES, the global-memory fallback
@pytest.mark.parametrize("n", [2049, 4096, 4097, 8192, 8193, 12289, 16384, 16385, 20001, 32769, 66000])
def test_single_list(gpu, n):
    cloud = _cloud(32, [n], seed=n)
    st, got = _render(32, cloud, _views(32, gpu), gpu)
    assert int(got["tile_start"][1]) == n
    _check(32, cloud, 1, st, got)


MIXED = [0, 100, 2048, 2049, 4097, 9000, 3000, 16385]


@pytest.fixture(scope="module")
def mixed():
    return _cloud(64, MIXED, seed=7)


def test_mixed_lists_in_one_call(gpu, mixed):
    """Every list class side by side: a merge unit of one tile must not pick up another tile's counter or ping-pong parity."""
    st, got = _render(64, mixed, _views(64, gpu), gpu)
    assert np.diff(got["tile_start"].cpu().numpy())[:8].tolist() == MIXED
    _check(64, mixed, 1, st, got)


def test_mixed_lists_on_two_views(gpu, mixed):
    """The same cloud through two cameras in one call (the second rolled by 180 degrees: its lists land on the mirrored tiles):
    long lists on views 0 and 1, tile indices beyond the first image's."""
    st, got = _render(64, mixed, _views(64, gpu, rolled=True), gpu)
    n = np.diff(got["tile_start"].cpu().numpy())
    assert n[:8].tolist() == MIXED and n[16:][::-1][:8].tolist() == MIXED
    _check(64, mixed, 2, st, got)


def test_two_calls_are_bit_identical(gpu, mixed):
    views = _views(64, gpu, rolled=True)
    _, a = _render(64, mixed, views, gpu)
    _, b = _render(64, mixed, views, gpu)
    for k in ("keys", "list", "tile_start"):
        assert torch.equal(a[k], b[k]), k
