"""CPU: the host model of the split-list hand-over (helpers.split_model, used by tests/test_gpu_split_parity.py) — its constants pinned
to the kernel sources, and its rule on hand-made lists (length thresholds, ragged images, far / near transmittance, slot limits)."""
import re
from pathlib import Path

import numpy as np

import helpers as H

CSRC = Path(__file__).resolve().parent.parent / "splatter360_amd" / "csrc"


def _define(text, name):
    m = re.search(r"#define\s+" + name + r"\s+(\S+)", text)
    assert m, name
    return m.group(1)


def test_constants_match_the_sources():
    dev = (CSRC / "s360_device.h").read_text()
    fwd = (CSRC / "s360_forward.hip").read_text()
    assert int(_define(dev, "S360_SEG_LEN")) == H.SEG_LEN
    assert int(_define(dev, "S360_SEG_HEAD")) == H.SEG_HEAD
    assert int(_define(dev, "S360_SEG_MIN_REST")) == H.SEG_MIN_REST
    assert int(_define(dev, "S360_SUB_W")) == H.SUB_W
    assert re.search(r"SEG_PER_CHUNK = 4096 / SEG_LEN", dev) and H.SEG_PER_CHUNK == H.SORT_CHUNK // H.SEG_LEN
    assert re.search(r"SEG_K0 = SEG_HEAD / SEG_LEN", dev) and H.SEG_K0 == H.SEG_HEAD // H.SEG_LEN
    m = re.search(r"SEG_T_FAR = 1\.0f / (\d+)\.0f", dev)
    assert m and 1.0 / int(m.group(1)) == H.SEG_T_FAR
    assert re.search(r"return \(size_t\)SEG_PER_CHUNK \* \(cap / 2048 \+ 1\);", dev)          # seg_slots
    assert re.search(r"sub_ox\(int w\) \{ return SUB_W == 16 \? 0 : 8 \* \(w & 1\); \}", dev)
    assert re.search(r"sub_oy\(int w\) \{ return SUB_W == 16 \? 4 \* w : 8 \* \(w >> 1\); \}", dev)
    assert int(re.search(r"constexpr uint32_t SORT_SHORT = (\d+);", fwd).group(1)) == H.SORT_SHORT
    e, th = re.search(r"constexpr uint32_t SORT_CHUNK = (\d+) \* SORT_THREADS;", fwd).group(1), _define(fwd, "S360_SORT_THREADS")
    assert int(e) * int(th) == H.SORT_CHUNK
    # the hand-over rule itself (k_render): the length test, the far test, the slot test
    assert "end - start >= SEG_HEAD + SEG_MIN_REST && end - start > SORT_SHORT) ? start + SEG_HEAD" in fwd
    assert "const bool far_px = !done && T >= SEG_T_FAR;" in fwd
    assert "(SEG_PER_CHUNK * chunk_start[t] + (end - start + SEG_LEN - 1) / SEG_LEN) <= sgp->n_slots" in fwd
    assert "nch0 = nc0 > SORT_SHORT ? (nc0 + SORT_CHUNK - 1) / SORT_CHUNK : 0u" in fwd        # the chunk table


def _lists(lengths, opacity=0.0, h=32, w=32):
    """Tile lists of the given lengths (tile index order); every entry one splat centred on pixel (4, 4) of its tile, sigma ~1 px."""
    n_tot = sum(lengths)
    gx = (w + 15) // 16
    ranges = np.zeros((len(lengths), 2), np.int64)
    xy = np.zeros((n_tot, 2))
    s = 0
    for t, n in enumerate(lengths):
        ranges[t] = (s, s + n)
        ty, tx = divmod(t, gx)
        xy[s:s + n] = (16 * tx + 4, 16 * ty + 4)
        s += n
    co = np.tile([[0.5, 0.0, 0.5, opacity]], (n_tot, 1))
    return ranges, np.arange(n_tot), xy, co


def test_length_thresholds_and_items():
    for n, want in ((2048, False), (2049, True), (4097, True)):
        ranges, vals, xy, co = _lists([n, 0, 0, 0])
        m = H.split_model(ranges, vals, xy, co, 32, 32, H.seg_slots(1 << 20))
        assert m["split"][0].tolist() == [want] * 4 and m["clear"].all()
        k = (n + H.SEG_LEN - 1) // H.SEG_LEN - H.SEG_K0
        assert m["n_split"] == 4 * want and m["n_items"] == 4 * k * want


def test_ragged_quadrants_outside_the_image_never_split():
    ranges, vals, xy, co = _lists([0, 3000, 0, 0], h=20, w=20)
    m = H.split_model(ranges, vals, xy, co, 20, 20, H.seg_slots(1 << 20))
    assert m["split"][1].tolist() == [True, False, True, False]      # px 16..19 inside; quadrants 1 / 3 start at px 24


def test_near_and_far_transmittance():
    # opacity 0.9 at pixel (4, 4): the pixels around it stop within the head; quadrant 3 is out of the splat's reach (T = 1)
    ranges, vals, xy, co = _lists([3000, 0, 0, 0], opacity=0.9)
    m = H.split_model(ranges, vals, xy, co, 32, 32, H.seg_slots(1 << 20))
    assert m["split"][0, 3] and m["t_far"][0, 3] == 1.0
    # 512 flat entries (the same alpha at every pixel of the tile) in front, with T = 1/32 behind them: refused everywhere
    ranges, vals, xy, co = _lists([3000, 0, 0, 0])
    co[:, 0] = co[:, 2] = 0.0
    co[:512, 3] = 1.0 - (1.0 / 32.0) ** (1.0 / 512)
    m = H.split_model(ranges, vals, xy, co, 32, 32, H.seg_slots(1 << 20))
    assert not m["split"].any() and m["clear"].all() and abs(m["t_far"][0, 0] - 1 / 32) < 1e-9
    co[:512, 3] = 1.0 - (1.0 / 16.0) ** (1.0 / 512)                 # exactly SEG_T_FAR: not a clear decision
    m = H.split_model(ranges, vals, xy, co, 32, 32, H.seg_slots(1 << 20))
    assert not m["clear"][0].any()


def test_slot_limit_follows_chunk_order():
    lengths = [4097, 2561, 0, 3000]                  # 2 + 1 + 0 + 1 sort chunks
    ranges, vals, xy, co = _lists(lengths)
    cs = H.chunk_table(ranges)
    assert cs.tolist() == [0, 2, 3, 3, 4]
    exact = H.SEG_PER_CHUNK * 3 + (3000 + H.SEG_LEN - 1) // H.SEG_LEN
    m = H.split_model(ranges, vals, xy, co, 32, 32, exact)
    assert m["split"].any(1).tolist() == [True, True, False, True]
    m = H.split_model(ranges, vals, xy, co, 32, 32, exact - 1)
    assert m["split"].any(1).tolist() == [True, True, False, False]


def test_views_share_one_chunk_table():
    """Two images of 2 x 2 tiles in one call: tile index t = v T + tile, chunk_start runs across the images (k_tile_scan), so the slot
    limit of image 1's long list counts image 0's chunks; the quadrant geometry restarts per image."""
    lengths = [4097, 0, 0, 0, 0, 0, 0, 2561]           # image 0 tile 0 (2 chunks), image 1 tile 3 (1 chunk)
    ranges, vals, xy, co = _lists(lengths)
    xy[4097:] = (16 + 4, 16 + 4)                       # image 1's splats on ITS tile (1, 1)
    cs = H.chunk_table(ranges)
    assert cs[7] == 2
    exact = H.SEG_PER_CHUNK * 2 + (2561 + H.SEG_LEN - 1) // H.SEG_LEN
    m = H.split_model(ranges, vals, xy, co, 32, 32, exact)
    assert m["split"].any(1).tolist() == [True] + [False] * 6 + [True]
    assert m["n_items"] == 4 * (9 - 2) + 4 * (6 - 2)
    m = H.split_model(ranges, vals, xy, co, 32, 32, exact - 1)
    assert m["split"].any(1).tolist() == [True] + [False] * 7
