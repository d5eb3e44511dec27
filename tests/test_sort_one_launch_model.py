"""Host-side MODEL of the one-launch tile sort (splatter360_amd/csrc/s360_forward.hip: k_sort_stage1's chunk blocks and merge
blocks, chunk_unit, merge_unit, merge_path_global_wave): the same unit enumeration and index formulas, executed in Python on
random unique 64-bit keys.  Every multi-chunk list — 2 .. 16 chunks — takes ceil(log2 chunks) passes of (pass, chunk) units that
are handed out in pass-major order from one ticket counter.  Checked here: the ping-pong parity (the last pass lands in `keys`
and writes `list`), ragged last runs, that a unit's dependencies all have strictly lower tickets (what makes the waits of the
kernel deadlock-free), and that the result does not depend on the order in which independent units finish.  The kernels
themselves are put against a host sort in tests/test_gpu_sort_one_launch.py."""
import numpy as np
import pytest

SORT_SHORT, SORT_CHUNK, MAX_PASSES, E, THREADS = 2048, 4096, 4, 8, 512
INF = np.uint64(0xFFFFFFFFFFFFFFFF)


def ceil_log2(x):
    return 0 if x <= 1 else int(x - 1).bit_length()


def merge_passes_of(nch):
    return ceil_log2(nch)


def merge_path_wave(A, la, B, lb, d):
    """64-ary search of merge_path_global_wave: number of A elements among the first d merged outputs."""
    lo, hi = max(d - lb, 0), min(d, la)
    while lo < hi:
        step = (hi - lo + 63) // 64
        a = lo + np.arange(64) * step
        ok = a < hi
        cnt = int(np.count_nonzero(A[a[ok]] <= B[d - 1 - a[ok]]))   # the predicate holds for a prefix of the probes
        if cnt == 0:
            hi = lo
        else:
            nhi = lo + cnt * step
            lo = lo + (cnt - 1) * step + 1
            hi = min(nhi, hi)
    return lo


class Call:
    """One call's tile table: lengths -> tile_start, the chunk table of k_tile_scan, header[3], and the two key buffers."""

    def __init__(self, lengths, rng):
        self.n = np.asarray(lengths, np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.n)])
        self.nch = np.where(self.n > SORT_SHORT, (self.n + SORT_CHUNK - 1) // SORT_CHUNK, 0)
        self.chunk_start = np.concatenate([[0], np.cumsum(self.nch)])
        self.nchunks = int(self.chunk_start[-1])
        self.npass = min(merge_passes_of(int(self.nch.max(initial=0))), MAX_PASSES)   # header[3], clamped to the pass budget
        total = int(self.start[-1])
        depth = rng.integers(0, 1 << 20, total).astype(np.uint64)      # many equal depths: ties are broken by the low word
        self.bufs = [(depth << np.uint64(32)) | rng.permutation(total).astype(np.uint64), np.zeros(total, np.uint64)]   # keys, alt
        self.emitted = self.bufs[0].copy()
        self.lst = np.zeros(total, np.uint32)
        self.chunks_sorted = np.zeros(len(self.n), np.int64)
        self.merge_done = np.zeros((len(self.n), MAX_PASSES), np.int64)

    def chunk_unit(self, b):
        """chunk_unit: last tile t with chunk_start[t] <= b."""
        t = int(np.searchsorted(self.chunk_start, b, side="right") - 1)
        return dict(t=t, s=int(self.start[t]), n=int(self.n[t]), k=b - int(self.chunk_start[t]), passes=merge_passes_of(int(self.nch[t])))

    def sort_chunk(self, b):
        """a chunk block: one 4 096-key run, into `alt` when the tile's pass count is odd."""
        u = self.chunk_unit(b)
        if u["passes"] > MAX_PASSES:
            return
        c0 = u["s"] + u["k"] * SORT_CHUNK
        ln = min(SORT_CHUNK, u["n"] - u["k"] * SORT_CHUNK)
        self.bufs[u["passes"] & 1][c0:c0 + ln] = np.sort(self.bufs[0][c0:c0 + ln])
        if u["passes"] == 0:
            self.lst[c0:c0 + ln] = (self.bufs[0][c0:c0 + ln] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        else:
            self.chunks_sorted[u["t"]] += 1

    def unit_of_ticket(self, tk):
        """the merge blocks' ticket -> (pass, unit); None for the void tickets (single-chunk lists, passes the tile does not have)."""
        p, blk = divmod(tk, self.nchunks)
        u = self.chunk_unit(blk)
        if u["passes"] > MAX_PASSES or p >= u["passes"]:
            return None
        return p, blk, u

    def dependencies(self, tk):
        """tickets whose units advance the counter this unit waits for (pass 0 waits for chunk blocks: no tickets)."""
        p, blk, u = self.unit_of_ticket(tk)
        if p == 0:
            return []
        c0 = int(self.chunk_start[u["t"]])
        return [(p - 1) * self.nchunks + c0 + j for j in range(int(self.nch[u["t"]]))]

    def ready(self, tk):
        p, blk, u = self.unit_of_ticket(tk)
        nch = int(self.nch[u["t"]])
        return (self.merge_done[u["t"]][p - 1] if p else self.chunks_sorted[u["t"]]) == nch

    def merge_unit(self, tk):
        p, blk, u = self.unit_of_ticket(tk)
        n, P = u["n"], u["passes"]
        R = SORT_CHUNK << p
        src, dst = self.bufs[(P - p) & 1][u["s"]:u["s"] + n], self.bufs[(P - p - 1) & 1][u["s"]:u["s"] + n]
        o_tile = u["k"] * SORT_CHUNK
        ln = min(SORT_CHUNK, n - o_tile)
        pair0 = o_tile // (2 * R) * (2 * R)
        la = min(R, n - pair0)
        lb = min(R, n - pair0 - la)
        A, B = src[pair0:pair0 + la], src[pair0 + la:pair0 + la + lb]
        o = o_tile - pair0
        a0, a1 = merge_path_wave(A, la, B, lb, o), merge_path_wave(A, la, B, lb, o + ln)
        b0, b1 = o - a0, o + ln - a1
        na, nb = a1 - a0, b1 - b0
        assert na + nb == ln and 0 <= na <= la and 0 <= nb <= lb
        lds = np.concatenate([A[a0:a1], B[b0:b1]])
        res = np.zeros(ln, np.uint64)
        for t in range(THREADS):                                        # per-thread merge path + 8-step serial merge
            out0 = t * E
            if out0 >= ln:
                break
            lo_a, hi_a = max(out0 - nb, 0), min(out0, na)
            while lo_a < hi_a:
                mid = (lo_a + hi_a) >> 1
                if lds[mid] <= lds[na + out0 - 1 - mid]:
                    lo_a = mid + 1
                else:
                    hi_a = mid
            a, b = lo_a, out0 - lo_a
            for q in range(E):
                ka = lds[a] if a < na else INF
                kb = lds[na + b] if b < nb else INF
                take_a = ka <= kb
                if out0 + q < ln:
                    res[out0 + q] = ka if take_a else kb
                a, b = (a + 1, b) if take_a else (a, b + 1)
        dst[o_tile:o_tile + ln] = res
        if p + 1 == P:
            assert ((P - p - 1) & 1) == 0                               # the last pass lands in `keys`
            self.lst[u["s"] + o_tile:u["s"] + o_tile + ln] = (res & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        else:
            self.merge_done[u["t"]][p] += 1

    def run(self, order=None):
        """chunk blocks, then every merge unit: in ticket order, or in `order` (a permutation of the tickets), each unit run as soon
        as its counter allows — as workgroups that took their tickets in order but finish in any order would."""
        for b in range(self.nchunks):
            self.sort_chunk(b)
        tickets = [tk for tk in range(self.npass * self.nchunks) if self.unit_of_ticket(tk) is not None]
        for tk in tickets:
            assert all(d < tk for d in self.dependencies(tk)), tk      # a unit only ever waits for lower tickets
        pending = list(tickets if order is None else order)
        while pending:
            runnable = [tk for tk in pending if self.ready(tk)]
            assert runnable, "a unit waits for something that never comes"
            if order is None:
                assert runnable[0] == pending[0]                        # in ticket order nothing ever has to wait
            self.merge_unit(runnable[0])
            pending.remove(runnable[0])

    def check(self):
        for t in range(len(self.n)):
            s, e = int(self.start[t]), int(self.start[t + 1])
            if e - s <= SORT_SHORT:
                continue                                                # the short-list blocks: not modelled
            want = np.sort(self.emitted[s:e])
            assert np.array_equal(self.bufs[0][s:e], want), t
            assert np.array_equal(self.lst[s:e], (want & np.uint64(0xFFFFFFFF)).astype(np.uint32)), t


@pytest.mark.parametrize("n", [2049, 4096, 4097, 8192, 8193, 12289, 16384, 16385, 20001, 32769, 65536])
def test_single_list_units_parity_and_ragged_runs(n):
    c = Call([n], np.random.default_rng(n))
    nch = (n + SORT_CHUNK - 1) // SORT_CHUNK
    assert c.npass == ceil_log2(nch) <= MAX_PASSES
    c.run()
    c.check()
    if nch > 1:
        assert c.chunks_sorted[0] == nch and all(c.merge_done[0][p] == nch for p in range(c.npass - 1))


def test_mixed_tiles_share_one_ticket_counter():
    """Lists of every class in one call: void tickets (short and single-chunk lists, passes a shorter list does not have) are
    skipped, no unit touches another tile's counter or parity, and finishing order does not matter."""
    lengths = [0, 100, 2048, 2049, 4097, 9000, 3000, 16385]
    a = Call(lengths, np.random.default_rng(1))
    assert a.nchunks == 1 + 2 + 3 + 1 + 5 and a.npass == 3
    a.run()
    a.check()
    b = Call(lengths, np.random.default_rng(1))
    tickets = [tk for tk in range(b.npass * b.nchunks) if b.unit_of_ticket(tk) is not None]
    assert len(tickets) == 2 * 1 + 3 * 2 + 5 * 3                      # units = chunks x passes of each multi-chunk list
    b.run(order=[tickets[i] for i in np.random.default_rng(2).permutation(len(tickets))])
    b.check()
    assert np.array_equal(a.bufs[0], b.bufs[0]) and np.array_equal(a.lst, b.lst)


def test_lists_beyond_the_pass_budget_get_no_units():
    """A list of more than SORT_CHUNK << MAX_PASSES keys is left to the global-memory fallback: no chunk sort, no merge unit, and
    the other lists of the call are merged as usual (header[3] is clamped to the budget)."""
    c = Call([65537, 8193], np.random.default_rng(3))
    assert c.npass == MAX_PASSES
    before = c.bufs[0][:65537].copy()
    c.run()
    assert np.array_equal(c.bufs[0][:65537], before) and c.chunks_sorted[0] == 0
    s = int(c.start[1])
    assert np.array_equal(c.bufs[0][s:], np.sort(c.emitted[s:]))
