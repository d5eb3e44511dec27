"""A numpy model of the integer arithmetic of block_bucket_sort (csrc/s360_forward.hip): block min / max of the high words, the
float-scaled bucket function, the rank a returning atomic hands out (ANY arrival order), the exclusive scan, the scatter and the
in-bucket count of smaller keys — against np.sort of the 64-bit keys.  The model states what the kernel computes step by step in
the kernel's own number formats (uint32 -> float32 round-to-nearest, one float32 product, truncation, clamp), so a property that
fails here fails on the device as well: the bucket function must be monotone non-decreasing in the high word (else step 6 of the
kernel would rank a key among the wrong neighbours), buckets must stay below NB, and the packed per-key word (start | rank << 13 |
count << 20) must round-trip wherever the kernel does not take the merge sort."""
import numpy as np
import pytest

NB_SHORT, NB_CHUNK = 2048, 4096      # buckets of the short-list role and of a 4 096-key chunk
BMAX_FIELD = 0x7F                    # S360_SORT_BMAX is held below 0x80 by a static_assert: the rank field has 7 bits


def bucket_of(hi, lo, top, nb):
    """bucket = min(nb - 1, (uint)(float(hi - lo) * (float(nb) / (float(top - lo) + 1))))   — all in float32, as the kernel."""
    hi = np.asarray(hi, np.uint32)
    scale = np.float32(nb) / (np.uint32(np.uint32(top) - np.uint32(lo)).astype(np.float32) + np.float32(1.0))
    assert scale.dtype == np.float32
    prod = (hi - np.uint32(lo)).astype(np.uint32).astype(np.float32) * scale
    assert prod.dtype == np.float32 and float(prod.max(initial=0.0)) < 2.0 ** 31   # the conversion is in range
    return np.minimum(prod.astype(np.int64), nb - 1).astype(np.uint32)


def model_sort(keys, nb, rng):
    """(sorted keys, largest bucket) by the kernel's steps; the atomics arrive in a random order."""
    keys = np.asarray(keys, np.uint64)
    n = keys.size
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    lo, top = hi.min(), hi.max()
    b = bucket_of(hi, lo, top, nb)
    assert b.max() <= nb - 1
    rank = np.empty(n, np.uint32)
    cnt = np.zeros(nb, np.uint32)
    for i in rng.permutation(n):                       # a returning atomic increment per key
        rank[i] = cnt[b[i]]
        cnt[b[i]] += 1
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)
    if cnt.max() <= BMAX_FIELD:                        # the packed word of the kernel's bucket path
        pk = start[b] | (rank << np.uint32(13)) | (cnt[b] << np.uint32(20))
        assert np.array_equal(pk & np.uint32(0x1FFF), start[b]) and np.array_equal((pk >> np.uint32(13)) & np.uint32(0x7F), rank)
        assert np.array_equal(pk >> np.uint32(20), cnt[b])
    buf = np.zeros(n, np.uint64)
    buf[start[b] + rank] = keys                        # ordered by bucket, unordered inside one
    out = np.zeros(n, np.uint64)
    for i in range(n):
        s, c = int(start[b[i]]), int(cnt[b[i]])
        out[s + int(np.count_nonzero(buf[s:s + c] < keys[i]))] = keys[i]
    return out, int(cnt.max())


def make_keys(hi, rng):
    """depth word << 32 | pair, the pairs unique and in no order."""
    hi = np.asarray(hi, np.uint32).astype(np.uint64)
    pair = rng.permutation(1 << 20)[:hi.size].astype(np.uint64)
    return (hi << np.uint64(32)) | pair


def bits(depth):
    return np.asarray(depth, np.float32).view(np.uint32)


def _log_uniform(n, rng):
    return bits(np.exp(rng.uniform(np.log(0.2), np.log(50.0), n)))


def _all_equal(n, rng):
    return np.full(n, bits(3.25), np.uint32)


def _two_words(n, rng):
    return np.where(rng.integers(0, 2, n) == 0, bits(2.0), bits(7.5)).astype(np.uint32)


def _last_bit(n, rng):                                  # a range of 1: far below the bucket count
    return (bits(4.0) + rng.integers(0, 2, n).astype(np.uint32)).astype(np.uint32)


def _full_span(n, rng):
    h = bits(np.exp(rng.uniform(np.log(0.2), np.log(3e38), n)))
    h[0], h[-1] = bits(0.2), bits(3e38)
    return h


def _one_outlier(n, rng):
    h = bits(5.0 + rng.uniform(-1e-3, 1e-3, n))
    h[n // 2] = bits(900.0)
    return h


DISTRIBUTIONS = dict(log_uniform=_log_uniform, all_equal=_all_equal, two_words=_two_words, last_bit=_last_bit, full_span=_full_span,
                     one_outlier=_one_outlier)
SIZES = [1, 2, 63, 64, 65, 2047, 2048, 4096]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dist", sorted(DISTRIBUTIONS))
def test_model_sorts_like_np_sort(dist, n):
    rng = np.random.default_rng(1000 * n + len(dist))
    keys = make_keys(DISTRIBUTIONS[dist](n, rng), rng)
    assert np.unique(keys).size == n
    nb = NB_SHORT if n <= 2048 else NB_CHUNK
    got, largest = model_sort(keys, nb, rng)
    np.testing.assert_array_equal(got, np.sort(keys))
    if dist == "all_equal":
        assert largest == n                            # one bucket: beyond S360_SORT_BMAX keys the kernel takes the merge sort
    if dist == "log_uniform" and n >= 2047:
        assert largest <= 16                           # the path the headline's lists take (simulated mean ~2, largest ~5)


def test_arrival_order_does_not_matter():
    rng = np.random.default_rng(5)
    keys = make_keys(_one_outlier(1456, rng), rng)
    a, _ = model_sort(keys, NB_SHORT, np.random.default_rng(1))
    b, _ = model_sort(keys, NB_SHORT, np.random.default_rng(2))
    np.testing.assert_array_equal(a, b)


RANGES = [(bits(4.0), bits(4.0)), (bits(4.0), bits(4.0) + 1), (bits(4.0), bits(4.0) + 2047), (bits(4.0), bits(4.0) + 2048),
          (bits(4.0), bits(4.0) + 2049), (bits(2.0), bits(30.0)), (bits(0.2), bits(3e38)), (np.uint32(0), np.uint32(0xFFFFFFFF)),
          (np.uint32(1), np.uint32(0x01000001)), (np.uint32(0x7F000000), np.uint32(0xFFFFFFFF))]


@pytest.mark.parametrize("nb", [NB_SHORT, NB_CHUNK])
@pytest.mark.parametrize("lo,top", RANGES)
def test_bucket_is_monotone_on_adjacent_bit_patterns(lo, top, nb):
    lo, top = int(lo), int(top)
    rng = np.random.default_rng(lo % 9973 + nb)
    span = top - lo
    runs = [np.arange(lo, min(top, lo + 5000) + 1), np.arange(max(lo, top - 5000), top + 1)]
    if span > 10000:   # runs of adjacent patterns all over the range, among them where float(hi - lo) changes its exponent
        starts = np.concatenate([rng.integers(lo, top - 64, 2000), lo + (1 << np.arange(1, int(np.log2(span)) + 1)) - 32])
        runs += [np.clip(s + np.arange(64), lo, top) for s in starts]
    hi = np.unique(np.concatenate(runs)).astype(np.uint32)          # ascending
    b = bucket_of(hi, lo, top, nb).astype(np.int64)
    assert b[0] == 0 and b.max() <= nb - 1
    assert (np.diff(b) >= 0).all()
    if span >= nb:
        assert b[-1] >= nb // 2                        # the range is spread over the buckets, not squeezed into a few
