"""The segment-parallel composite of long tile lists (S360_FLAG_SPLIT_LISTS) against the oracle, at the list-length edges of the
hand-over (SORT_SHORT, SEG_HEAD, SEG_LEN, a last segment of one entry, a second sort chunk, the global-sort fallback beyond 65 536
keys), with pixels that stop in the head / at a segment's first entry / inside the last segment, quadrants whose hand-over is refused
(all pixels below SEG_T_FAR, or outside a ragged image), segment slots running out, and the fused depth / MSE / inference epilogues.

Designed scenes: small splats (sigma 0.4 - 1 px, 3-sigma rectangles inside ONE tile) so that a tile list has exactly the length asked
for on both list modes, faint enough (opacity 0.01 - 0.06) that no pixel comes near the 1e-4 stop threshold by accident; list
positions are set through the depths.  Every call pins lean= / split_lists= itself (only test_history_sized_slots_run_out goes through
the adaptive history, on purpose) and every case asserts
that it reached its regime: the list length (oracle ranges), the seg_flag pattern the host model (helpers.split_model) predicts, and
header[5] / header[6].

test_schedule_variant_is_bit_identical builds the same sources with no phase-2 workers and one-workgroup phase-1 / tail / backward
segment grids into a temporary directory: the combine adds the segments in list order whichever wave computed them, so every image,
transmittance, contributor count, loss and gradient must be the same bits — and the variant's mop-up kernel must have taken every item."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import (SEG_HEAD, SEG_LEN, SEG_PER_CHUNK, chunk_table, pixel_splats, seg_slots, small_front_scene,
                     split_model)
from oracle import oracle
from splatter360_amd import _lib, rasterizer
from test_gpu_headline_parity import _grad_err, _report
from test_gpu_parity import _settings_to_torch, check_forward

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# (h, w, long tile, box of the live centres, box of the "ghost" centres).  32 x 32: tile 0 (clamped left / top: centres anywhere in
# [0, 13)); lists of up to N_LIVE entries, all of them live.  40 x 20: tile (1, 2) of a ragged image — only px 16..19, py 32..39 (part
# of quadrant 0) inside, quadrants 1 - 3 wholly outside; entries beyond N_LIVE are ghosts: opaque splats centred inside the tile's
# 16 x 16 box but outside the image, at least 3 px below its last row (alpha < 1e-4 at every image pixel).  They lengthen the list
# without darkening it — no pixel saturates by accident, so no stop decision lands near 1e-4 — and, since they reach alpha >= 1/255
# inside the tile's box (the lean binning's test, which does not clip to the image), the lean lists hold them too: both list modes
# have exactly the designed length.
SHAPES = {
    "sq": (32, 32, 0, (0.0, 13.0, 0.0, 13.0), None),
    "rag": (40, 20, 5, (20.05, 23.0, 36.05, 40.0), (26.0, 31.0, 42.0, 47.0)),
}
# pixels of the designed stops, spaced so that their opaque pairs do not darken one another (3-sigma rectangles inside the tile)
STOP_PIXELS = {"sq": [(3, 3), (10, 2), (2, 10), (6, 6), (12, 5)], "rag": [(19, 35), (19, 37), (19, 39)]}
N_LIVE = 2600


def _scene(n, shape, seed, stops=True, refuse_q0=False):
    """One long list of exactly n entries on the shape's tile (+ nothing else).  stops: opaque (0.995) pairs centred on chosen pixels
    at chosen list positions r - 1, r, so that the pixel's stop test fires AT position r: in the head, at the first entry of the first
    segment handed over and of the next, at the last segment's first entry and in its middle.  refuse_q0: 600 opacity-0.1 splats over
    quadrant 0 in front of everything else, so that all of its pixels are far below SEG_T_FAR after SEG_HEAD entries (hand-over
    refused) without any of them stopping."""
    h, w, tile, lb, gb = SHAPES[shape]
    rng = np.random.default_rng(seed)
    K = (n + SEG_LEN - 1) // SEG_LEN
    ranks = []
    if stops:     # by priority: first entry of the first segment handed over, of the last segment, middle of the last, head, next
        want = [SEG_HEAD, (K - 1) * SEG_LEN, (K - 1) * SEG_LEN + (n - (K - 1) * SEG_LEN) // 2, 500, SEG_HEAD + SEG_LEN]
        for r in want:
            if len(ranks) < len(STOP_PIXELS[shape]) and SEG_HEAD + SEG_LEN <= n and 1 <= r < n and all(abs(r - q) >= 2 for q in ranks):
                ranks.append(r)
    n_fixed = 2 * len(ranks)
    n_front = 600 if refuse_q0 else 0
    n_live = n - n_fixed - n_front if gb is None else min(N_LIVE, n - n_fixed - n_front)
    n_ghost = n - n_fixed - n_front - n_live
    gb = gb or lb
    px = np.concatenate([rng.uniform(lb[0], lb[1], n_live), rng.uniform(gb[0], gb[1], n_ghost)])
    py = np.concatenate([rng.uniform(lb[2], lb[3], n_live), rng.uniform(gb[2], gb[3], n_ghost)])
    sig = np.concatenate([rng.uniform(0.4, 1.0, n_live), np.full(n_ghost, 0.4)])
    op = np.concatenate([rng.uniform(0.01, 0.06, n_live), np.full(n_ghost, 0.9)])
    zs = np.linspace(2.0, 40.0, n)                          # list position i <-> depth zs[i]
    fixed_pos = [p for r in ranks for p in (r - 1, r)] + list(range(n_front))
    rest = np.setdiff1d(np.arange(n), np.asarray(fixed_pos, np.int64))
    z = np.concatenate([zs[rng.permutation(rest)], zs[np.asarray(fixed_pos, np.int64)]]) if fixed_pos else zs[rng.permutation(rest)]
    for i, r in enumerate(ranks):
        x, y = STOP_PIXELS[shape][i]
        px, py = np.append(px, [x + 0.02, x + 0.02]), np.append(py, [y + 0.02, y + 0.02])   # (off the rectangle's rounding edge)
        sig, op = np.append(sig, [0.4, 0.4]), np.append(op, [0.995, 0.995])
    if n_front:
        px, py = np.append(px, rng.uniform(-1.0, 9.0, n_front)), np.append(py, rng.uniform(-1.0, 9.0, n_front))
        sig, op = np.append(sig, np.full(n_front, 1.0)), np.append(op, np.full(n_front, 0.1))
    means, cov6 = pixel_splats(px, py, sig, z, h, w)
    S, *_ = small_front_scene(n=2, seed=0, h=h, w=w)
    colors = rng.uniform(0.0, 1.0, (n, 3))
    return S, means, cov6, op[:, None], colors, dict(h=h, w=w, tile=tile, ranks=ranks)


def _oracle(S, means, cov6, op, colors, gimg=None, dtype=np.float32):
    o = oracle.rasterize(S, means3D=means, cov3D_precomp=cov6, opacities=op, colors_precomp=colors, dtype=dtype)
    f = o.forward()
    return f, (o.backward(gimg) if gimg is not None else None)


class _Segs:
    """rasterizer.default_segments pinned for the duration of a block: 0 = the library's worst case (never the history)."""

    def __init__(self, n_slots=0):
        self.n = n_slots

    def __enter__(self):
        self.old = rasterizer.default_segments
        rasterizer.default_segments = lambda key: self.n

    def __exit__(self, *a):
        rasterizer.default_segments = self.old


def _run(S, means, cov6, op, colors, dev, *, lean, split, grad=None, depth_mode=None, mse_target=None, mse_defer=False, n_slots=0,
         keep_slots=False):
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=grad is not None)
    m, c, o, col = t(means), t(cov6), t(op), t(colors)
    st = _settings_to_torch(S, dev)
    views = rasterizer.pack_views(st.viewmatrix, st.projmatrix, st.campos, st.tanfovx, st.tanfovy, st.bg, near=1.0, far=100.0)
    with _Segs(n_slots):
        res = rasterizer.rasterize_views(m, c, o, None, col, views=views, image_height=S["image_height"], image_width=S["image_width"],
                                         sh_degree=0, shared_campos=True, lean=lean, split_lists=split, depth_mode=depth_mode,
                                         mse_target=mse_target, mse_defer=mse_defer, keep_slots=keep_slots)
    state = rasterizer.last_state()
    hdr = state.header().cpu().numpy()
    out = dict(image=res[0], radii=res[1], state=state, hdr=hdr, seg_flag=state.tensors()["seg_flag"].cpu().numpy().reshape(-1, 4),
               split_errors=state.split_errors(), mopup=state.mopup_items() if split else 0, prm=state.prm)
    if depth_mode is not None:
        out["depth"] = res[2]
    if mse_target is not None:
        out["mse"] = res[-1]
    if grad is not None:
        if mse_target is not None:
            res[-1].loss.backward()
        else:
            res[0].backward(torch.tensor(np.asarray(grad, np.float32), device=dev)[None])
        out["grads"] = dict(means3D=m.grad.cpu().numpy(), cov3D=c.grad.cpu().numpy(), opacities=o.grad.cpu().numpy(),
                            colors_precomp=col.grad.cpu().numpy())
        if mse_target is not None:
            out["loss"] = float(res[-1].loss.detach())
    return out


def _gpu_lists(r):
    """(ranges [tiles, 2], list) of the call's own tile lists (the lean lists may be shorter than the oracle's rectangles)."""
    t = r["state"].tensors()
    ts = t["tile_start"].cpu().numpy().astype(np.int64)
    return np.stack([ts[:-1], ts[1:]], 1), (t["list"][: ts[-1]].cpu().numpy().astype(np.int64) & 0xFFFFFFFF)


def _check_split_state(r, f, h, w, n_slots, tag):
    """seg_flag against the host model (on the call's own lists, the oracle's 2D records) wherever its margin is clear, header[5] / [6]
    consistent with seg_flag, error word 0."""
    ranges, values = _gpu_lists(r)
    m = split_model(ranges, values, f["xy"], f["conic_opacity"], h, w, n_slots)
    got = r["seg_flag"] == 1
    assert got.shape == m["split"].shape
    assert np.array_equal(got[m["clear"]], m["split"][m["clear"]]), (tag, np.argwhere(got != m["split"]).tolist(), m["t_far"].tolist())
    assert int(r["hdr"][5]) == int(got.sum()), tag
    L = np.diff(ranges, axis=1)[:, 0]
    items = sum(int((L[t] + SEG_LEN - 1) // SEG_LEN - SEG_HEAD // SEG_LEN) for t, q in np.argwhere(got))
    assert int(r["hdr"][6]) == items, (tag, int(r["hdr"][6]), items)
    if m["clear"].all():
        assert int(r["hdr"][6]) == m["n_items"], tag
    assert r["split_errors"] == 0, tag
    return m


def _hip_for_check(r, f):
    """test_gpu_parity.check_forward's input from one rasterize_views result."""
    st = {k: v.cpu().numpy() for k, v in r["state"].tensors().items()}
    return dict(image=r["image"][0].detach().cpu().numpy(), radii=r["radii"][0].cpu().numpy(), state=st,
                num_rendered=r["state"].num_rendered())


LENGTHS = [2048, 2049, 2560, 2561, 4096, 4097, 8193]
CASES = [(n, "sq") for n in LENGTHS if n <= N_LIVE] + [(n, "rag") for n in LENGTHS]


def _case_forward(dev, n, shape, seed, **scene_kw):
    S, means, cov6, op, colors, d = _scene(n, shape, seed, **scene_kw)
    h, w, tile = d["h"], d["w"], d["tile"]
    f, _ = _oracle(S, means, cov6, op, colors)
    L = np.diff(f["ranges"].astype(np.int64), axis=1)[:, 0]
    assert L[tile] == n and L.sum() == n, (n, L.tolist())          # the regime: exactly one list, of exactly n entries
    tag = f"split_{shape}_{n}"
    res = {}
    for lean in (False, True):
        # (upstream lists: a training forward — check_forward compares the instance-slot tables too; lean: an inference call)
        r = _run(S, means, cov6, op, colors, dev, lean=lean, split=True, keep_slots=not lean)
        r0 = _run(S, means, cov6, op, colors, dev, lean=lean, split=False, keep_slots=not lean)
        n_gpu = int(np.diff(_gpu_lists(r)[0], axis=1)[tile, 0])
        assert n_gpu == n, (tag, lean, n_gpu)                        # the edge length, on both list modes
        n_slots = seg_slots(r["prm"].max_instances)
        m = _check_split_state(r, f, h, w, n_slots, tag)
        img, img0 = r["image"][0].detach().cpu().numpy(), r0["image"][0].detach().cpu().numpy()
        if lean:
            assert np.abs(img.astype(np.float64) - f["image"]).max() <= 1e-5, (tag, float(np.abs(img - f["image"]).max()))
        else:
            check_forward(_hip_for_check(r, f), f, means.shape[0], h, w)
        # split on against split off, the same lists: the kernel's stated bound, and the same contributor counts
        t1, t0 = r["state"].tensors(), r0["state"].tensors()
        assert np.abs(img.astype(np.float64) - img0).max() <= 1e-6, (tag, lean, float(np.abs(img - img0).max()))
        assert torch.equal(t1["n_contrib"], t0["n_contrib"]), (tag, lean)
        res[lean] = dict(r=r, m=m)
    # the designed stops happened where designed (positions r - 1 / r: n_contrib = r, the last contributor's 1-based position)
    nc = res[False]["r"]["state"].tensors()["n_contrib"][0].cpu().numpy()
    for i, rk in enumerate(d["ranks"]):
        x, y = STOP_PIXELS[shape][i]
        assert nc[y, x] == rk and f["n_contrib"][y, x] == rk, (tag, (x, y), rk, int(nc[y, x]))
    return S, means, cov6, op, colors, d, f, res


@pytest.mark.parametrize("n,shape", CASES)
def test_list_length_edges_forward(gpu, n, shape):
    _, _, _, _, _, d, f, res = _case_forward(gpu, n, shape, seed=n)
    got = res[True]["r"]["seg_flag"][d["tile"]]
    if n <= 2048:
        assert not got.any()                   # a list of SORT_SHORT entries never splits
    elif shape == "sq":
        assert got.tolist() == [1, 1, 1, 1], got  # quadrant 0: a pixel done in the head beside far ones; still hands over
    else:
        assert got.tolist() == [1, 0, 0, 0], got  # quadrants 1 - 3 lie outside the image: never far
    _report(f"split_{shape}_{n}_forward", seg_flag=got.tolist(), items=int(res[True]["r"]["hdr"][6]),
            mopup_items=int(res[True]["r"]["mopup"]))


def test_list_beyond_65536_keys(gpu):
    n = 80_000
    _, _, _, _, _, d, f, res = _case_forward(gpu, n, "rag", seed=7)
    assert res[True]["r"]["seg_flag"][d["tile"]].tolist() == [1, 0, 0, 0]
    for lean in (False, True):
        assert int(res[lean]["r"]["hdr"][6]) == (n + SEG_LEN - 1) // SEG_LEN - 2, lean


def test_refused_hand_over(gpu):
    """Quadrant 0 is below SEG_T_FAR everywhere after SEG_HEAD entries (no pixel stopped): refused; the others hand over."""
    n = 2561
    _, _, _, _, _, d, f, res = _case_forward(gpu, n, "sq", seed=21, stops=False, refuse_q0=True)
    m = res[True]["m"]
    assert 1e-3 < m["t_far"][0, 0] < 0.8 * (1 / 16) and m["clear"][0, 0]
    assert res[True]["r"]["seg_flag"][0].tolist() == [0, 1, 1, 1]


@pytest.mark.parametrize("n,shape", [(2049, "sq"), (2561, "sq"), (4097, "rag"), (8193, "rag")])
def test_backward_against_f64_oracle(gpu, n, shape):
    S, means, cov6, op, colors, d = _scene(n, shape, seed=100 + n)
    gimg = np.random.default_rng(n).standard_normal((3, d["h"], d["w"])).astype(np.float32)
    f32, g32 = _oracle(S, means, cov6, op, colors, gimg)
    _, g64 = _oracle(S, means, cov6, op, colors, gimg, dtype=np.float64)
    assert np.diff(f32["ranges"].astype(np.int64), axis=1)[d["tile"], 0] == n
    rep = {}
    for lean in (False, True):
        for split in (True, False):
            r = _run(S, means, cov6, op, colors, gpu, lean=lean, split=split, grad=gimg)
            if split:
                assert r["seg_flag"][d["tile"]].any() and r["split_errors"] == 0
            for k, got in r["grads"].items():
                e, e32 = _grad_err(got, g64[k], g32[k])
                rep[f"{k}_lean{int(lean)}_split{int(split)}"], rep[k + "_oracle_f32"] = e, e32
                assert e <= max(1e-4, 1.1 * e32), (k, lean, split, e, e32)
    _report(f"split_{shape}_{n}_bwd_rel_err_vs_f64_oracle", **rep)


def test_segment_slots_run_out(gpu):
    """Two long lists (tiles 0 and 3 of a 32 x 32 image, chunk order 0 then 3); max_segments such that tile 3's segments fit EXACTLY,
    then one slot fewer: tile 0 still splits, tile 3 is composited sequentially — both against the oracle."""
    h = w = 32
    rng = np.random.default_rng(5)
    n0, n3 = 4097, 2561
    boxes = [(0.0, 13.0, 0.0, 13.0, n0), (20.0, 32.0, 20.0, 32.0, n3)]
    px = np.concatenate([rng.uniform(b[0], b[1], b[4]) for b in boxes])
    py = np.concatenate([rng.uniform(b[2], b[3], b[4]) for b in boxes])
    N = n0 + n3
    sig, op = rng.uniform(0.4, 1.0, N), rng.uniform(0.006, 0.03, N)
    z = rng.permutation(np.linspace(2.0, 40.0, N))
    means, cov6 = pixel_splats(px, py, sig, z, h, w)
    S, *_ = small_front_scene(n=2, seed=0, h=h, w=w)
    colors = rng.uniform(0, 1, (N, 3))
    gimg = rng.standard_normal((3, h, w)).astype(np.float32)
    f, g32 = _oracle(S, means, cov6, op[:, None], colors, gimg)
    _, g64 = _oracle(S, means, cov6, op[:, None], colors, gimg, dtype=np.float64)
    L = np.diff(f["ranges"].astype(np.int64), axis=1)[:, 0]
    assert L.tolist() == [n0, 0, 0, n3]
    for lean in (False, True):
        ranges, _ = _gpu_lists(_run(S, means, cov6, op[:, None], colors, gpu, lean=lean, split=False))    # the call's own lists
        cs = chunk_table(ranges)
        exact = SEG_PER_CHUNK * int(cs[3]) + (int(ranges[3, 1] - ranges[3, 0]) + SEG_LEN - 1) // SEG_LEN
        for n_slots, want3 in ((exact, True), (exact - 1, False)):
            r = _run(S, means, cov6, op[:, None], colors, gpu, lean=lean, split=True, grad=gimg, n_slots=n_slots)
            assert r["prm"].max_segments == n_slots
            m = _check_split_state(r, f, h, w, n_slots, f"slots{n_slots}")
            assert r["seg_flag"][0].any() and bool(r["seg_flag"][3].any()) == want3, r["seg_flag"].tolist()
            assert m["split"][3].any() == want3
            img = r["image"][0].detach().cpu().numpy()
            assert np.abs(img.astype(np.float64) - f["image"]).max() <= 1e-5
            for k, got in r["grads"].items():
                e, e32 = _grad_err(got, g64[k], g32[k])
                assert e <= max(1e-4, 1.1 * e32), (k, n_slots, lean, e, e32)


def test_history_sized_slots_run_out(gpu):
    """split_lists="auto": calls of one shape (P, V, H, W, list mode) with a single long list (one sort chunk) size default_segments from
    the history; the next call of the same shape holds 38 lists of two chunks each — far more than those slots allow.  It splits the
    tiles whose segments fit (chunk order) and composites the rest sequentially; images and gradients against the oracle."""
    h, w, n_tiles, n_per = 16, 16 * 40, 38, 6000
    P = n_tiles * n_per
    rng = np.random.default_rng(9)
    S, *_ = small_front_scene(n=2, seed=0, h=h, w=w)
    tiles = list(range(1, 1 + n_tiles))
    px = np.concatenate([rng.uniform(16 * t + 4, 16 * t + 13, n_per) for t in tiles])
    py = rng.uniform(0.0, 16.0, P)
    z = rng.permutation(np.linspace(2.0, 40.0, P))
    means, cov6 = pixel_splats(px, py, rng.uniform(0.4, 1.0, P), z, h, w)
    op, colors = rng.uniform(0.006, 0.02, (P, 1)), rng.uniform(0, 1, (P, 3))
    first = means.copy()
    first[2600:, 2] = -5.0                 # behind the camera: the first calls hold ONE long list (tile 1, 2 600 entries)
    f1, _ = _oracle(S, first, cov6, op, colors)
    assert np.diff(f1["ranges"].astype(np.int64), axis=1)[:, 0].max() == 2600
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float32), device=gpu, requires_grad=g)
    st = _settings_to_torch(S, gpu)
    views = rasterizer.pack_views(st.viewmatrix, st.projmatrix, st.campos, st.tanfovx, st.tanfovy, st.bg)
    old = (rasterizer.SPLIT_LONG_LISTS, rasterizer.DETERMINISTIC)
    try:
        rasterizer.SPLIT_LONG_LISTS, rasterizer.DETERMINISTIC = "auto", False
        for _ in range(2):      # the first call reports "worth splitting" and its chunk count; the second splits with that history
            rasterizer.rasterize_views(t(first), t(cov6), t(op), None, t(colors), views=views, image_height=h, image_width=w,
                                       shared_campos=True, lean=True, split_lists="auto")
            torch.cuda.synchronize()
        assert rasterizer.last_state().prm.flags & _lib.FLAG_SPLIT_LISTS and rasterizer.last_state().tensors()["seg_flag"].any()
        # the slots the history allows this shape now (rasterizer.default_segments: from the largest chunk count seen, one chunk)
        want_slots = rasterizer.default_segments(rasterizer._hint_key(gpu, P, 1, h, w, True))
        gimg = rng.standard_normal((3, h, w)).astype(np.float32)
        m_ = t(means, True)
        imgs, _ = rasterizer.rasterize_views(m_, t(cov6), t(op), None, t(colors), views=views, image_height=h, image_width=w,
                                             shared_campos=True, lean=True, split_lists="auto")
    finally:
        rasterizer.SPLIT_LONG_LISTS, rasterizer.DETERMINISTIC = old
    state = rasterizer.last_state()
    flag = state.tensors()["seg_flag"].cpu().numpy().reshape(-1, 4)
    n_slots = int(state.prm.max_segments)
    assert state.prm.flags & _lib.FLAG_SPLIT_LISTS, "the call must split: the history says this shape has lists worth splitting"
    assert n_slots == want_slots > 0, ("max_segments is not the history-sized default_segments", n_slots, want_slots)
    f, g32 = _oracle(S, means, cov6, op, colors, gimg)
    L = np.diff(f["ranges"].astype(np.int64), axis=1)[:, 0]
    assert (L[tiles] == n_per).all() and L.sum() == P
    ranges = np.stack([state.tensors()["tile_start"].cpu().numpy().astype(np.int64)[:-1],
                       state.tensors()["tile_start"].cpu().numpy().astype(np.int64)[1:]], 1)
    values = state.tensors()["list"][: int(ranges[-1, 1])].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    m = split_model(ranges, values, f["xy"], f["conic_opacity"], h, w, n_slots)
    split_tiles = np.nonzero(flag.any(1))[0]
    Lg, cs = np.diff(ranges, axis=1)[:, 0], chunk_table(ranges)
    assert (Lg[tiles] > 4096).all()                 # two sort chunks each, on the lean lists as well
    fits = [t_ for t_ in tiles if SEG_PER_CHUNK * int(cs[t_]) + (int(Lg[t_]) + SEG_LEN - 1) // SEG_LEN <= n_slots]
    assert split_tiles.tolist() == fits and 0 < len(fits) < n_tiles, (split_tiles.tolist(), n_slots)
    assert np.array_equal((flag == 1)[m["clear"]], m["split"][m["clear"]])
    assert state.split_errors() == 0
    img = imgs[0].detach().cpu().numpy()
    assert np.abs(img.astype(np.float64) - f["image"]).max() <= 1e-5
    imgs.backward(torch.tensor(gimg, device=gpu)[None])
    _, g64 = _oracle(S, means, cov6, op, colors, gimg, dtype=np.float64)
    e, e32 = _grad_err(m_.grad.cpu().numpy(), g64["means3D"], g32["means3D"])
    assert e <= max(1e-4, 1.1 * e32), (e, e32)
    _report("split_history_slots", n_slots=n_slots, split_tiles=len(split_tiles), long_tiles=n_tiles, means3D_rel_err=e, oracle_f32=e32)


@pytest.mark.parametrize("lean", [False, True])
def test_epilogues_depth_mse_and_inference(gpu, lean):
    """Fused depth (WITH_DEPTH in phase 1, phase 2 and the tail), the fused MSE with and without mse_defer (loss = torch's mean over the
    returned image, and = the split-off call's), and an inference call whose image is bit-identical to the training call's — on both
    list modes, each call checked for its regime (list length, seg_flag against the model, header[5] / [6], error word)."""
    n = 2561
    S, means, cov6, op, colors, d = _scene(n, "sq", seed=33)
    f, _ = _oracle(S, means, cov6, op, colors)
    h, w, tile = d["h"], d["w"], d["tile"]
    assert np.diff(f["ranges"].astype(np.int64), axis=1)[tile, 0] == n

    def regime(r, split=True):
        assert int(np.diff(_gpu_lists(r)[0], axis=1)[tile, 0]) == n
        if split:
            m = _check_split_state(r, f, h, w, seg_slots(r["prm"].max_instances), f"epilogue_lean{int(lean)}")
            assert m["split"][tile].all() and r["seg_flag"][tile].all()
        else:
            assert not r["seg_flag"].any() and r["split_errors"] == 0

    gimg = np.random.default_rng(3).standard_normal((3, h, w)).astype(np.float32)
    r_inf = _run(S, means, cov6, op, colors, gpu, lean=lean, split=True)
    r_trn = _run(S, means, cov6, op, colors, gpu, lean=lean, split=True, grad=gimg)
    regime(r_inf)
    regime(r_trn)
    assert torch.equal(r_inf["image"], r_trn["image"])
    assert np.abs(r_inf["image"][0].detach().cpu().numpy().astype(np.float64) - f["image"]).max() <= 1e-5
    # depth
    rd = _run(S, means, cov6, op, colors, gpu, lean=lean, split=True, depth_mode="depth")
    rd0 = _run(S, means, cov6, op, colors, gpu, lean=lean, split=False, depth_mode="depth")
    regime(rd)
    regime(rd0, split=False)
    assert torch.equal(rd["image"], r_inf["image"])
    dd = (rd["depth"] - rd0["depth"]).abs().max().item()
    assert dd <= 1e-6 * max(1.0, rd0["depth"].abs().max().item()), dd
    # reference depth: sum of alpha T z over the oracle's contributions is not exposed; z as a colour channel gives it
    zc = np.repeat(means[:, 2:3], 3, axis=1)
    fz, _ = _oracle(S, means, cov6, op, zc)
    bgT = np.asarray(S["bg"], np.float64)[0] * fz["final_T"]
    want_depth = fz["image"][0] - bgT
    assert np.abs(rd["depth"][0].cpu().numpy() - want_depth).max() <= 1e-5 * max(1.0, np.abs(want_depth).max())
    # fused MSE
    target = torch.tensor(np.random.default_rng(4).uniform(0, 1, (1, 3, h, w)).astype(np.float32), device=gpu)
    losses = {}
    for split in (True, False):
        for defer in (False, True):
            r = _run(S, means, cov6, op, colors, gpu, lean=lean, split=split, grad=gimg, mse_target=target, mse_defer=defer)
            regime(r, split)
            want = float(((r["image"].detach().double() - target.double()) ** 2).mean())
            assert abs(r["loss"] - want) <= 2e-6 * want, (split, defer, r["loss"], want)
            losses[(split, defer)] = r["loss"]
    for defer in (False, True):
        assert abs(losses[(True, defer)] - losses[(False, defer)]) <= 2e-6 * losses[(False, defer)]


def _check_view_forward(fs, img, f, n_tiles):
    """test_gpu_parity.check_forward's assertions for one view of a multi-view call (its slice renumbered by _face_state): tile counts,
    sorted list, keys and ranges bit-exact; pixels <= 1e-5 where n_contrib agrees, mean <= 1e-6, n_contrib flips at most one per
    20 000 pixels (none on these sizes), final_T within 1e-5."""
    np.testing.assert_array_equal(fs["tiles_touched"], f["tiles_touched"])
    assert fs["list"].shape[0] == f["num_rendered"]
    np.testing.assert_array_equal(fs["list"], f["values"])
    tile_of = np.repeat(np.arange(n_tiles, dtype=np.uint64), np.diff(fs["tile_start"]))
    np.testing.assert_array_equal((tile_of << np.uint64(32)) | fs["depth_bits"], f["keys"])
    nonempty = f["ranges"][:, 1] > f["ranges"][:, 0]
    np.testing.assert_array_equal(fs["tile_start"][:-1][nonempty], f["ranges"][nonempty, 0])
    np.testing.assert_array_equal(fs["tile_start"][1:][nonempty], f["ranges"][nonempty, 1])
    per_px = np.abs(img.astype(np.float64) - f["image"]).mean(0)
    same = fs["n_contrib"] == f["n_contrib"]
    assert per_px.mean() <= 1e-6 and per_px[same].max(initial=0.0) <= 1e-5, (per_px.mean(), per_px[same].max())
    assert (~same).sum() <= same.size // 20000, int((~same).sum())
    np.testing.assert_allclose(fs["final_T"][same], f["final_T"][same], rtol=0, atol=1e-5)


MV_OFFSET = 100.0     # camera v sits at x = 100 v: a splat in front of one camera lies far outside the other cameras' frusta


@pytest.mark.parametrize("lean", [False, True])
def test_multi_view_chunk_table_across_views(gpu, lean):
    """V = 3 views in ONE call (different camera centres).  View 0 holds a 2 561-entry list, view 1 only short lists, view 2 a 4 097-entry
    list: tile index t = v T + tile and chunk_start runs across the views (view 2's list starts at chunk 1), which the hand-over's slot
    test, the segment slots, the phase-1 workers' tile decode (v = t / T) and the backward all index with.  Each view against its own
    oracle run (settings_from_views: the very camera records the kernels saw); seg_flag against the model over the whole call; and
    the segment slots once with view 2's segments fitting EXACTLY, once one slot short (view 0 still splits, view 2 does not)."""
    from helpers import settings_from_views
    from test_gpu_headline_parity import _face_state
    h = w = 32
    T = 4
    parts = [_scene(2561, "sq", seed=41), _scene(300, "sq", seed=42, stops=False), _scene(4097, "sq", seed=43, stops=False)]
    means = np.concatenate([p[1] + np.array([MV_OFFSET * v, 0.0, 0.0]) for v, p in enumerate(parts)])
    cov6, op, colors = (np.concatenate([p[k] for p in parts]) for k in (2, 3, 4))
    P = means.shape[0]
    S0 = parts[0][0]
    vms, pms, cps = [], [], []
    for v in range(3):
        view = np.eye(4)
        view[0, 3] = -MV_OFFSET * v                                   # world -> camera: x - 100 v
        proj = np.asarray(S0["projmatrix"], np.float64)             # (view = identity there: projmatrix = proj^T)
        vms.append(view.T)
        pms.append(view.T @ proj)
        cps.append([MV_OFFSET * v, 0.0, 0.0])
    tt = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)
    views = rasterizer.pack_views(tt(vms), tt(pms), tt(cps), 1.0, 1.0, tt(S0["bg"]))
    gimg = np.random.default_rng(44).standard_normal((3, 3, h, w)).astype(np.float32)
    fs, g32s, g64s = [], [], []
    for v in range(3):
        S = settings_from_views(views, v, h, w, sh_degree=0)
        f, g32 = _oracle(S, means, cov6, op, colors, gimg[v])
        _, g64 = _oracle(S, means, cov6, op, colors, gimg[v], dtype=np.float64)
        fs.append(f), g32s.append(g32), g64s.append(g64)
    L = np.concatenate([np.diff(f["ranges"].astype(np.int64), axis=1)[:, 0] for f in fs])
    assert L.tolist() == [2561, 0, 0, 0, 300, 0, 0, 0, 4097, 0, 0, 0], L.tolist()     # the regime: long lists on views 0 and 2 only
    xy = np.concatenate([f["xy"] for f in fs])
    co = np.concatenate([f["conic_opacity"] for f in fs])

    def run(split, n_slots=0, grad=True):
        t = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu, requires_grad=grad)
        m, c, o, col = t(means), t(cov6), t(op), t(colors)
        with _Segs(n_slots):
            imgs, _ = rasterizer.rasterize_views(m, c, o, None, col, views=views, image_height=h, image_width=w, sh_degree=0,
                                                 shared_campos=False, lean=lean, split_lists=split, keep_slots=True)
        st = rasterizer.last_state()
        tsr = st.tensors()
        out = dict(img=imgs.detach().cpu().numpy(), st=st, t=tsr, flag=tsr["seg_flag"].cpu().numpy().reshape(-1, 4),
                   hdr=st.header().cpu().numpy(), errs=st.split_errors())
        imgs.backward(torch.tensor(gimg, device=gpu))
        out["grads"] = dict(means3D=m.grad.cpu().numpy(), cov3D=c.grad.cpu().numpy(), opacities=o.grad.cpu().numpy(),
                            colors_precomp=col.grad.cpu().numpy())
        return out

    def lists(r):
        ts = r["t"]["tile_start"].cpu().numpy().astype(np.int64)
        return np.stack([ts[:-1], ts[1:]], 1), r["t"]["list"][: ts[-1]].cpu().numpy().astype(np.int64) & 0xFFFFFFFF

    r0 = run(False)
    ranges, values = lists(r0)
    assert np.diff(ranges, axis=1)[:, 0].tolist() == L.tolist()
    cs = chunk_table(ranges)
    assert cs[8] == 1                                              # view 2's list: chunk 1 of the call
    exact = SEG_PER_CHUNK * int(cs[8]) + (4097 + SEG_LEN - 1) // SEG_LEN
    rep = {}
    for n_slots, want2 in ((0, True), (exact, True), (exact - 1, False)):
        r = run(True, n_slots)
        slots = n_slots or seg_slots(r["st"].prm.max_instances)
        assert int(r["st"].prm.max_segments) == n_slots
        ranges_r, values_r = lists(r)
        m = split_model(ranges_r, values_r, xy, co, h, w, slots)
        got = r["flag"] == 1
        assert np.array_equal(got[m["clear"]], m["split"][m["clear"]]), (n_slots, got.tolist(), m["split"].tolist())
        assert got[0].all() and not got[4:8].any() and got[8].all() == want2 and got[8].any() == want2, (n_slots, got.tolist())
        assert int(r["hdr"][5]) == int(got.sum()) and r["errs"] == 0
        assert int(r["hdr"][6]) == 4 * (6 - 2) + (4 * (9 - 2) if want2 else 0), int(r["hdr"][6])
        for v in range(3):
            img, img0 = r["img"][v], r0["img"][v]
            if lean:
                assert np.abs(img.astype(np.float64) - fs[v]["image"]).max() <= 1e-5, v
            else:
                _check_view_forward(_face_state(r["t"], v, P, T), img, fs[v], T)
            assert np.abs(img.astype(np.float64) - img0).max() <= 1e-6, (v, n_slots)
            assert torch.equal(r["t"]["n_contrib"][v], r0["t"]["n_contrib"][v]), (v, n_slots)
        for k, got_g in r["grads"].items():
            want64 = sum(np.asarray(g[k], np.float64) for g in g64s)
            want32 = sum(np.asarray(g[k], np.float64) for g in g32s)
            e, e32 = _grad_err(got_g, want64, want32)
            e0, _ = _grad_err(r0["grads"][k], want64)
            rep[f"{k}_slots{n_slots}"], rep[k + "_split_off"], rep[k + "_oracle_f32"] = e, e0, e32
            assert e <= max(1e-4, 1.1 * e32) and e0 <= max(1e-4, 1.1 * e32), (k, n_slots, e, e0, e32)
    _report(f"split_multiview_lean{int(lean)}_bwd_rel_err_vs_f64_oracle", **rep)


# ------------------------------------------------------------------------------ schedule variant
VARIANT_FLAGS = ("-DS360_P2_GRID=0", "-DS360_P1_GRID=1", "-DS360_TAIL_GRID=1", "-DS360_SEG_BWD_BLOCKS=1")
_CHILD = r'''
import sys, json, numpy as np, torch
sys.path[:0] = [{root!r}, {root!r} + "/tests"]
from splatter360_amd import _lib
if {lib!r}:
    _lib.LIB_PATH = __import__("pathlib").Path({lib!r})
import test_gpu_split_parity as T
from splatter360_amd import decoder, rasterizer, synthetic
dev = torch.device("cuda:0")
out, mop = {{}}, {{}}
for n, shape in ((2049, "sq"), (2561, "sq"), (4097, "rag"), (8193, "rag")):
    S, means, cov6, op, colors, d = T._scene(n, shape, seed=100 + n)
    gimg = np.random.default_rng(n).standard_normal((3, d["h"], d["w"])).astype(np.float32)
    for lean in (False, True):
        r = T._run(S, means, cov6, op, colors, dev, lean=lean, split=True, grad=gimg)
        tt = r["state"].tensors()
        key = f"{{shape}}{{n}}_{{int(lean)}}"
        out[key] = [r["image"].detach().cpu(), tt["final_T"].cpu().clone(), tt["n_contrib"].cpu().clone()] + [torch.tensor(g) for g in r["grads"].values()]
        mop[key] = [r["mopup"], int(r["hdr"][6]), r["split_errors"]]
cloud = synthetic.surface_like_cloud(512, 1024, seed=0)
ps = [torch.tensor(cloud[k], device=dev, requires_grad=True) for k in ("means", "covariances", "harmonics", "opacities")]
ext, K, near, far = decoder.cube_cameras(torch.eye(4, device=dev), 0.1, 10.0)
rasterizer.SPLIT_LONG_LISTS = True
faces = decoder.render_views_fused(ext, K, near, far, (256, 256), torch.zeros(3, device=dev), *ps, shared_campos=True)
st = rasterizer.last_state()
tt = st.tensors()
mop["surface_like"] = [st.mopup_items(), int(st.header()[6].item()), st.split_errors()]
loss = ((faces - 0.5) ** 2).mean()
loss.backward()
out["surface_like"] = [faces.detach().cpu(), tt["final_T"].cpu().clone(), tt["n_contrib"].cpu().clone(), loss.detach().cpu()] + [p.grad.cpu() for p in ps]
torch.save(out, {dst!r})
print("MOPUP", json.dumps(mop))
'''


def _child(lib, dst):
    code = _CHILD.format(root=str(ROOT), lib=str(lib) if lib else "", dst=str(dst))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("MOPUP ")][-1]
    return torch.load(dst), json.loads(line[6:])


def test_schedule_variant_is_bit_identical(gpu, tmp_path):
    import time
    from splatter360_amd import _lib
    t0 = time.time()
    var = _lib.build(out=tmp_path / "variant" / "libs360.so", extra=VARIANT_FLAGS)
    t_build = time.time() - t0
    base, mop0 = _child(None, tmp_path / "base.pt")
    got, mop1 = _child(var, tmp_path / "variant.pt")
    assert base.keys() == got.keys()
    for k in base:
        for i, (a, b) in enumerate(zip(base[k], got[k])):
            assert torch.equal(a, b), (k, i, float((a.double() - b.double()).abs().max()))
    for k, (mopup, items, errs) in mop1.items():
        assert items > 0 and mopup == items and errs == 0, (k, mopup, items, errs)   # the variant's k_render_tail took every item
    assert all(v[2] == 0 for v in mop0.values())
    _report("split_schedule_variant", build_seconds=t_build, default_mopup=mop0, variant_mopup=mop1)
