"""The cube -> ERP stitch (csrc/s360_stitch.hip) against its float64 statement (tests/stitch_reference.py): exact tap sets and
weights, forward and backward within a rounding bar at odd and large sizes on both entry paths, synthetic grids on the volume's
borders, non-finite inputs against torch's own grid_sample, and a bit-reproducible backward.

Bars: |got - ref| <= K * 2^-24 * sum|v * w| per ERP pixel (forward) and <= K * 2^-24 * sum|g * w| per texel (backward).  The
measured worst ratios are printed (pytest -s) and, when S360_STITCH_PARITY_JSON names a file, written there."""
import json
import os
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import stitch_reference as sr
from splatter360_amd import stitch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
K_FWD = 8.0           # forward: eight float32 products summed in float32 (the a-priori bound gamma_8); measured <= 4.2 on an MI355X
K_BWD = 16.0          # backward: up to ~2 900 products per texel summed in pixel order; measured <= 6.6
SIZES = [(32, 64, 128), (24, 48, 96), (33, 66, 132), (48, 100, 200), (64, 96, 256), (256, 512, 1024), (512, 1024, 2048)]
RANDOM_MAP = (2 | 8, 0, 5, 1 | 8, 3, 4 | 8)   # a permutation with flips other than change_order's
_MEASURED = {}


def _record(key, val):
    _MEASURED[key] = max(val, _MEASURED.get(key, 0.0))
    out = os.environ.get("S360_STITCH_PARITY_JSON")
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(json.dumps(_MEASURED, indent=1, sort_keys=True))
    print(f"{key}: {val:.3f}")


@lru_cache(maxsize=4)
def _taps(fw, eh, ew):
    return sr.taps(stitch.sample_grid_numpy(fw, eh, ew), fw)


def _ratio(got, want, scale):
    """max |got - want| / (2^-24 * scale) over the elements, and whether every element with scale 0 is exactly 0."""
    err = np.abs(got.astype(np.float64) - want)
    zero = scale == 0
    r = err[~zero] / (U * scale[~zero])
    return (float(r.max()) if r.size else 0.0), bool(np.all(got[zero] == 0))


def _plan(grid, fw, dev):
    off, ent = stitch.adjoint_plan(grid, fw)
    return torch.from_numpy(off).to(dev), torch.from_numpy(ent).to(dev)


def _stitch_call(faces, grid_np, face_map, d_erp=None):
    """faces [6,C,fw,fw] (source order) through _Stitch on an arbitrary grid -> (erp, d_faces or None)."""
    fw, ch = int(faces.shape[-1]), int(faces.shape[1])
    dev = faces.device
    grid = torch.from_numpy(np.ascontiguousarray(grid_np)).to(dev)
    off, ent = _plan(grid_np, fw, dev)
    x = faces.detach().clone().requires_grad_(d_erp is not None)
    erp = stitch._Stitch.apply(x, grid, off, ent, face_map, None, ch, fw)
    if d_erp is None:
        return erp, None
    (g,) = torch.autograd.grad(erp, x, d_erp)
    return erp, g


def _source_to_slot(face_map, fw, f, y, x):
    """Slot-space texel index that source texel (f, y, x) occupies (the first slot reading face f)."""
    codes = face_map or tuple(range(6))
    for s, c in enumerate(codes):
        if c & 7 == f:
            return (s * fw + (fw - 1 - y if c & 8 else y)) * fw + (fw - 1 - x if c & 8 else x)
    raise ValueError(f)


# ---------------------------------------------------------------------------- 1. exact tap sets and weights

def _chosen_texels(fw, rng):
    """64 source texels: corners and edge midpoints (seams), rows / columns 0 and fw-1, face centres (the poles on U and D)."""
    m, e = fw // 2, fw - 1
    pts = []
    for f in range(6):
        pts += [(f, 0, 0), (f, e, e), (f, 0, m), (f, m, e), (f, e, m), (f, m, 0), (f, m, m)]
    pts += [(f, 0, e) for f in range(6)] + [(f, e, 0) for f in range(6)]
    while len(pts) < 64:
        pts.append((int(rng.integers(6)), int(rng.integers(fw)), int(rng.integers(fw))))
    return pts[:64]


def _chosen_pixels(tp, fw, rng):
    """64 ERP pixels: taps on rows / columns 0 and fw-1, weight-0 taps, z0 == 5, a blend of two faces, then random."""
    tex, w, valid = tp
    yx = np.where(valid, tex % (fw * fw), -1)
    y, x = yx // fw, yx % fw
    cats = [((y == 0) | (y == fw - 1)).any(1) & valid.all(1), ((x == 0) | (x == fw - 1)).any(1), (valid & (w == 0)).any(1),
            (tex[:, 0] // (fw * fw) == 5) & ~valid[:, 4], ((w[:, 4:] > 0) & (w[:, :4] > 0)).any(1), ~valid[:, 1]]
    pix = []
    for c in cats:
        idx = np.flatnonzero(c)
        if idx.size:
            pix += list(rng.choice(idx, min(8, idx.size), replace=False))
    pix += list(rng.choice(tex.shape[0], 64 - len(pix), replace=False))
    return [int(p) for p in pix[:64]]


@pytest.mark.parametrize("face_map", [None, stitch.CHANGE_ORDER_FACE_MAP, RANDOM_MAP], ids=["identity", "change_order", "random"])
@pytest.mark.parametrize("size", [(32, 64, 128), (33, 66, 132)])
def test_exact_tap_set_and_weights(gpu, size, face_map):
    fw, eh, ew = size
    rng = np.random.default_rng(fw)
    tex, w, valid = tp = _taps(fw, eh, ew)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    # forward: channel c is one-hot at source texel pts[c]; its ERP image is the float32 weight of that texel's taps, bit for bit
    pts = _chosen_texels(fw, rng)
    faces = torch.zeros(6, 64, fw, fw)
    for c, (f, y, x) in enumerate(pts):
        faces[f, c, y, x] = 1.0
    erp, _ = _stitch_call(faces.to(gpu), grid, face_map)
    want = np.zeros((64, eh * ew), np.float32)
    for c, (f, y, x) in enumerate(pts):
        hit = valid & (tex == _source_to_slot(face_map, fw, f, y, x))
        p, k = np.nonzero(hit)
        want[c, p] = w[p, k]
    np.testing.assert_array_equal(erp.cpu().numpy().reshape(64, -1), want)
    # backward: d_erp one-hot per channel at pixel pix[c] puts exactly that pixel's tap weights on exactly its texels
    pix = _chosen_pixels(tp, fw, rng)
    d = torch.zeros(64, eh * ew)
    d[torch.arange(64), torch.tensor(pix)] = 1.0
    _, g = _stitch_call(faces.to(gpu), grid, face_map, d.view(64, eh, ew).to(gpu))
    want = np.zeros((6, 64, fw, fw), np.float32)
    codes = face_map or tuple(range(6))
    for c, p in enumerate(pix):
        for k in np.flatnonzero(valid[p]):
            s, r = divmod(int(tex[p, k]), fw * fw)
            yy, xx = divmod(r, fw)
            if codes[s] & 8:
                yy, xx = fw - 1 - yy, fw - 1 - xx
            want[codes[s] & 7, c, yy, xx] += w[p, k]
    np.testing.assert_array_equal(g.cpu().numpy(), want)


# ---------------------------------------------------------------------------- 2./3. forward and backward against float64

def _channels(size):
    return (1, 3, 64) if size[0] <= 256 else (1, 3)          # 64 channels at 2048 x 1024 would be a 2 GB float64 reference


@pytest.mark.parametrize("size", SIZES, ids=[f"{a}_{b}_{c}" for a, b, c in SIZES])
def test_stitch_rendered_against_float64(gpu, size):
    fw, eh, ew = size
    tp = _taps(fw, eh, ew)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    mod = stitch.Cube2Equirec(fw, eh, ew).to(gpu)
    plan_n = np.diff(stitch.adjoint_plan_numpy(fw, eh, ew)[0])
    for ch in _channels(size):
        rng = np.random.default_rng(1000 * fw + ch)
        faces = rng.standard_normal((6, ch, fw, fw)).astype(np.float32)
        d = rng.standard_normal((ch, eh, ew)).astype(np.float32)
        x = torch.tensor(faces, device=gpu, requires_grad=True)
        erp = mod.stitch_rendered(x)
        (g,) = torch.autograd.grad(erp, x, torch.tensor(d, device=gpu))
        fm = stitch.CHANGE_ORDER_FACE_MAP
        rf, _ = _ratio(erp.detach().cpu().numpy(), sr.forward64(faces, grid, fm, tp=tp), sr.abs_forward64(faces, grid, fm, tp=tp))
        gn = g.cpu().numpy()
        rb, zeros_ok = _ratio(gn, sr.adjoint64(d, grid, fm, fw, tp=tp), sr.abs_adjoint64(d, grid, fm, fw, tp=tp))
        _record(f"rendered fwd {fw}_{eh}_{ew} C{ch}", rf)
        _record(f"rendered bwd {fw}_{eh}_{ew} C{ch}", rb)
        # texels no tap reaches are exactly 0 (slot-space counts mapped to source faces through change_order)
        untouched = np.zeros((6, fw, fw), bool)
        for s, c in enumerate(fm):
            u = (plan_n[s * fw * fw:(s + 1) * fw * fw] == 0).reshape(fw, fw)
            untouched[c & 7] = u[::-1, ::-1] if c & 8 else u
        assert untouched.any() and np.all(gn[np.broadcast_to(untouched[:, None], gn.shape)] == 0)
        assert zeros_ok
        assert rf <= K_FWD, (size, ch, rf)
        assert rb <= K_BWD, (size, ch, rb)


@pytest.mark.parametrize("size", SIZES, ids=[f"{a}_{b}_{c}" for a, b, c in SIZES])
def test_module_path_against_float64(gpu, size):
    """Cube2Equirec.forward on the reference's [B, C, fw, 6*fw] input (B = 2, strided face reads) and its gradient in that layout."""
    fw, eh, ew = size
    tp = _taps(fw, eh, ew)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    mod = stitch.Cube2Equirec(fw, eh, ew).to(gpu)
    for ch in _channels(size):
        rng = np.random.default_rng(2000 * fw + ch)
        cube = rng.standard_normal((2, ch, fw, 6 * fw)).astype(np.float32)
        d = rng.standard_normal((2, ch, eh, ew)).astype(np.float32)
        x = torch.tensor(cube, device=gpu, requires_grad=True)
        erp = mod(x)
        (g,) = torch.autograd.grad(erp, x, torch.tensor(d, device=gpu))
        erp, g = erp.detach().cpu().numpy(), g.cpu().numpy()
        for b in range(2):
            faces = cube[b].reshape(ch, fw, 6, fw).transpose(2, 0, 1, 3)            # [6, C, fw, fw] slot order
            rf, _ = _ratio(erp[b], sr.forward64(faces, grid, tp=tp), sr.abs_forward64(faces, grid, tp=tp))
            want = sr.adjoint64(d[b], grid, None, fw, tp=tp).transpose(1, 2, 0, 3).reshape(ch, fw, 6 * fw)
            scale = sr.abs_adjoint64(d[b], grid, None, fw, tp=tp).transpose(1, 2, 0, 3).reshape(ch, fw, 6 * fw)
            rb, zeros_ok = _ratio(g[b], want, scale)
            _record(f"module fwd {fw}_{eh}_{ew} C{ch}", rf)
            _record(f"module bwd {fw}_{eh}_{ew} C{ch}", rb)
            assert zeros_ok
            assert rf <= K_FWD, (size, ch, b, rf)
            assert rb <= K_BWD, (size, ch, b, rb)


# ---------------------------------------------------------------------------- 4. synthetic grids on the borders

@pytest.mark.parametrize("face_map", [None, stitch.CHANGE_ORDER_FACE_MAP], ids=["identity", "change_order"])
@pytest.mark.parametrize("fw", [1, 2, 5, 16])
def test_synthetic_grids_through_the_entry(gpu, fw, face_map):
    rng = np.random.default_rng(50 + fw)
    grid = sr.synthetic_grid(rng, 40, 64, fw)
    tp = sr.taps(grid, fw)
    faces = rng.standard_normal((6, 3, fw, fw)).astype(np.float32)
    d = rng.standard_normal((3, 40, 64)).astype(np.float32)
    erp, g = _stitch_call(torch.tensor(faces, device=gpu), grid, face_map, torch.tensor(d, device=gpu))
    rf, _ = _ratio(erp.detach().cpu().numpy(), sr.forward64(faces, grid, face_map, tp=tp), sr.abs_forward64(faces, grid, face_map, tp=tp))
    rb, zeros_ok = _ratio(g.cpu().numpy(), sr.adjoint64(d, grid, face_map, fw, tp=tp), sr.abs_adjoint64(d, grid, face_map, fw, tp=tp))
    _record(f"synthetic fwd fw{fw}", rf)
    _record(f"synthetic bwd fw{fw}", rb)
    assert zeros_ok and rf <= K_FWD and rb <= K_BWD, (rf, rb)


def test_a_face_no_slot_reads_gets_zeros(gpu):
    """A face map that reads source face 2 twice and face 4 never: face 4's gradient is all zeros, face 2 gets both slots' sum."""
    fw, eh, ew = 16, 32, 64
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    fm = (0, 1, 2, 3, 2 | 8, 5)
    rng = np.random.default_rng(9)
    d = rng.standard_normal((2, eh, ew)).astype(np.float32)
    faces = torch.tensor(rng.standard_normal((6, 2, fw, fw)).astype(np.float32), device=gpu)
    erp, g = _stitch_call(faces, grid, fm, torch.tensor(d, device=gpu))
    g = g.cpu().numpy()
    assert np.all(g[4] == 0)
    rb, _ = _ratio(g, sr.adjoint64(d, grid, fm, fw), sr.abs_adjoint64(d, grid, fm, fw))
    rf, _ = _ratio(erp.detach().cpu().numpy(), sr.forward64(faces.cpu().numpy(), grid, fm), sr.abs_forward64(faces.cpu().numpy(), grid, fm))
    assert rf <= K_FWD and rb <= K_BWD, (rf, rb)


# ---------------------------------------------------------------------------- 5. non-finite inputs

def _nonfinite_texels(tp, fw):
    """Slot-space texels read by the taps that used to clamp: slot 5 under z0 == 5 pixels, the last row / column under y0 / x0 ==
    fw-1 pixels; plus one ordinary texel for the NaN."""
    tex, w, valid = tp
    slot5 = tex[np.flatnonzero((tex[:, 0] // (fw * fw) == 5) & ~valid[:, 4])[0], 0]
    last_row = tex[np.flatnonzero(valid[:, 0] & ~valid[:, 2])[0], 0]
    last_col = tex[np.flatnonzero(valid[:, 0] & ~valid[:, 1])[0], 0]
    inner = np.flatnonzero(valid.all(1))
    nan = tex[inner[inner.size // 3], 0]
    return (slot5, np.inf), (last_row, np.inf), (last_col, -np.inf), (nan, np.nan)


@pytest.mark.parametrize("size", [(32, 64, 128), (256, 512, 1024)])
def test_non_finite_faces_match_torch_grid_sample(gpu, size):
    fw, eh, ew = size
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    tp = _taps(fw, eh, ew)
    fm = stitch.CHANGE_ORDER_FACE_MAP
    rng = np.random.default_rng(77)
    vol = rng.standard_normal((6, 2, fw, fw)).astype(np.float32)          # slot space
    for t, val in _nonfinite_texels(tp, fw):
        s, r = divmod(int(t), fw * fw)
        vol[s, :, r // fw, r % fw] = val
    # the same volume in rendered (source) order for stitch_rendered: undo change_order
    faces = np.empty_like(vol)
    for s, c in enumerate(fm):
        faces[c & 7] = vol[s][..., ::-1, ::-1] if c & 8 else vol[s]
    got = stitch.Cube2Equirec(fw, eh, ew).to(gpu).stitch_rendered(torch.tensor(faces, device=gpu)).cpu().numpy()
    want = torch.nn.functional.grid_sample(torch.tensor(vol.transpose(1, 0, 2, 3))[None], torch.tensor(grid)[None, None],
                                           padding_mode="border", align_corners=True)[0, :, 0].numpy()
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    ref = sr.forward64(faces, grid, fm, tp=tp)
    scale = sr.abs_forward64(np.where(np.isfinite(faces), faces, 0), grid, fm, tp=tp)
    r, _ = _ratio(got[fin], ref[fin], scale[fin])
    assert r <= K_FWD, r


@pytest.mark.parametrize("face_map", [None, stitch.CHANGE_ORDER_FACE_MAP], ids=["identity", "change_order"])
def test_backward_with_inf_gradient_matches_adjoint64(gpu, face_map):
    fw, eh, ew = 32, 64, 128
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    tex, w, valid = tp = _taps(fw, eh, ew)
    rng = np.random.default_rng(12)
    d = rng.standard_normal((2, eh, ew)).astype(np.float32)
    flat = d.reshape(2, -1)
    flat[0, np.flatnonzero((valid & (w == 0)).any(1))[0]] = np.inf      # reaches a texel with weight 0: NaN there
    flat[1, np.flatnonzero(valid.all(1) & (w > 0).all(1))[5]] = -np.inf
    faces = torch.zeros(6, 2, fw, fw, device=gpu)
    _, g = _stitch_call(faces, grid, face_map, torch.tensor(d, device=gpu))
    g = g.cpu().numpy()
    want = sr.adjoint64(d, grid, face_map, fw, tp=tp)
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(np.isnan(g), np.isnan(want))
    inf = np.isinf(want)
    np.testing.assert_array_equal(g[inf], want[inf])
    fin = np.isfinite(want)
    scale = sr.abs_adjoint64(np.where(np.isfinite(d), d, 0), grid, face_map, fw, tp=tp)
    r, _ = _ratio(g[fin], want[fin], scale[fin])
    assert r <= K_BWD, r


# ---------------------------------------------------------------------------- 6. determinism

def _grad(mod, faces, d):
    x = faces.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(mod.stitch_rendered(x), x, d)
    return g


def test_backward_is_bit_reproducible(gpu):
    fw, eh, ew = 256, 512, 1024
    mod = stitch.Cube2Equirec(fw, eh, ew).to(gpu)
    gen = torch.Generator(device=gpu).manual_seed(3)
    fa, fb = (torch.randn(6, 3, fw, fw, device=gpu, generator=gen) for _ in range(2))
    da, db = (torch.randn(3, eh, ew, device=gpu, generator=gen) for _ in range(2))
    a1 = _grad(mod, fa, da)
    b = _grad(mod, fb, db)
    a2 = _grad(mod, fa, da)
    assert torch.equal(a1, a2) and not torch.equal(a1, b)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        a3 = _grad(mod, fa, da)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    assert torch.equal(a1, a3)
