"""CPU tests of the stitch's float64 statement (tests/stitch_reference.py), of the adjoint plan the HIP backward walks
(splatter360_amd.stitch.adjoint_plan) and of the sampling grid at non-power-of-two sizes."""
from pathlib import Path

import numpy as np
import pytest
import torch

import stitch_reference as sr
from splatter360_amd import stitch

G = Path(__file__).resolve().parent / "golden"


def _torch_sample(vol, grid, dtype):
    """The reference's op: grid_sample over [1, C, 6, fw, fw] (vol is [6, C, fw, fw] in slot order)."""
    v = torch.tensor(np.ascontiguousarray(vol.transpose(1, 0, 2, 3)), dtype=dtype)[None]
    g = torch.tensor(np.asarray(grid), dtype=dtype)[None, None]
    return torch.nn.functional.grid_sample(v, g, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].numpy()


def _volume(rng, c, fw, nonfinite=False):
    v = rng.standard_normal((6, c, fw, fw))
    if nonfinite:
        v[5, :, 3, 4] = np.inf                 # slot 5: the clamped target of the dz = 1 taps
        v[1, :, fw - 1, 2] = np.inf            # last row
        v[2, :, 5, fw - 1] = -np.inf           # last column
        v[3, :, fw - 1, fw - 1] = np.inf
        v[0, :, 7, 9] = np.nan
    return v


@pytest.mark.parametrize("nonfinite", [False, True])
@pytest.mark.parametrize("fw", [1, 2, 9, 16])
def test_forward64_equals_torch_grid_sample_float64(fw, nonfinite):
    rng = np.random.default_rng(fw + 100 * nonfinite)
    grid = sr.synthetic_grid(rng, 24, 40, fw)
    vol = _volume(rng, 3, fw, nonfinite and fw >= 16)
    if nonfinite and fw >= 16:                 # pixels aimed at the non-finite texels, on and next to their integer coordinates
        for j, (s, y, x) in enumerate(((5, 3, 4), (1, fw - 1, 2), (2, 5, fw - 1), (3, fw - 1, fw - 1), (0, 7, 9))):
            grid[j, :8] = sr.texel_coord(fw, s, y, x)
            grid[j, 1, 2] = np.nextafter(grid[j, 1, 2], np.float32(2))
            grid[j, 2, 0] = np.nextafter(grid[j, 2, 0], np.float32(-2))
    want = _torch_sample(vol, grid, torch.float64)
    if nonfinite and fw >= 16:
        assert np.isnan(want).any() and np.isinf(want).any()
    got = sr.forward64(vol, grid, coord=np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-13)           # equal_nan; inf must equal inf


@pytest.mark.parametrize("fw", [2, 16])
def test_forward64_float32_coordinates_equal_torch_float32(fw):
    """float32 coordinates are what the kernel and the reference (float32 tensors) use: same taps, same weights; torch then
    sums in float32, so the values agree to float32 rounding and the NaN / inf pattern exactly."""
    rng = np.random.default_rng(7 + fw)
    grid = sr.synthetic_grid(rng, 24, 40, fw)
    vol = _volume(rng, 3, fw, fw >= 16).astype(np.float32)
    want = _torch_sample(vol, grid, torch.float32).astype(np.float64)
    got = sr.forward64(vol, grid)
    scale = sr.abs_forward64(np.where(np.isfinite(vol), vol, 0), grid)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    assert np.all(err[fin] <= 4 * 2.0 ** -24 * scale[fin] + 1e-30)


@pytest.mark.parametrize("size", [(16, 32, 64), (24, 48, 96), (33, 66, 132)])
def test_forward64_on_the_stitch_grids(size):
    fw, eh, ew = size
    rng = np.random.default_rng(fw)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    vol = rng.standard_normal((6, 2, fw, fw))
    np.testing.assert_allclose(sr.forward64(vol, grid, coord=np.float64), _torch_sample(vol, grid, torch.float64), rtol=0, atol=1e-13)
    want32 = _torch_sample(vol.astype(np.float32), grid, torch.float32)
    assert np.abs(sr.forward64(vol.astype(np.float32), grid) - want32).max() <= 1e-6


@pytest.mark.parametrize("face_map", [None, stitch.CHANGE_ORDER_FACE_MAP, (2 | 8, 0, 5, 1 | 8, 3, 4 | 8)])
def test_face_map_is_the_reference_change_order(face_map):
    rng = np.random.default_rng(3)
    faces = rng.standard_normal((6, 2, 8, 8))
    vol = sr.slot_volume(faces, face_map)
    for s, code in enumerate(face_map or range(6)):
        src = faces[code & 7]
        np.testing.assert_array_equal(vol[s], src[..., ::-1, ::-1] if code & 8 else src)
    grid = stitch.sample_grid_numpy(8, 16, 32)
    np.testing.assert_array_equal(sr.forward64(faces, grid, face_map), sr.forward64(vol, grid))


@pytest.mark.parametrize("face_map", [None, stitch.CHANGE_ORDER_FACE_MAP])
@pytest.mark.parametrize("fw", [2, 9])
def test_adjoint64_equals_torch_autograd(fw, face_map):
    rng = np.random.default_rng(fw)
    grid = sr.synthetic_grid(rng, 20, 30, fw)
    faces = torch.tensor(rng.standard_normal((6, 3, fw, fw)), requires_grad=True)
    codes = face_map or tuple(range(6))
    vol = torch.stack([faces[c & 7].flip(-1, -2) if c & 8 else faces[c & 7] for c in codes], 1)[None]
    out = torch.nn.functional.grid_sample(vol, torch.tensor(grid, dtype=torch.float64)[None, None], padding_mode="border",
                                          align_corners=True)
    d = rng.standard_normal((3, 20, 30))
    out.backward(torch.tensor(d)[None, :, None])
    np.testing.assert_allclose(sr.adjoint64(d, grid, face_map, fw, coord=np.float64), faces.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_adjoint64_is_the_transpose_and_keeps_weight_zero_taps():
    fw, eh, ew = 24, 48, 96
    rng = np.random.default_rng(5)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    u, w = rng.standard_normal((6, 2, fw, fw)), rng.standard_normal((2, eh, ew))
    for fm in (None, stitch.CHANGE_ORDER_FACE_MAP):
        lhs = (sr.forward64(u, grid, fm) * w).sum()
        rhs = (u * sr.adjoint64(w, grid, fm, fw)).sum()
        assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    # an inf in d_erp reaches every in-range texel of its pixel, weight 0 included: inf * 0 = NaN, as in torch's adjoint
    tex, wt, valid = sr.taps(grid, fw)
    p = int(np.flatnonzero((valid & (wt == 0)).any(1))[0])
    d = np.zeros((1, eh, ew))
    d.reshape(-1)[p] = np.inf
    a = sr.adjoint64(d, grid, None, fw).reshape(-1)
    for k in np.flatnonzero(valid[p]):
        assert np.isnan(a[tex[p, k]]) if wt[p, k] == 0 else a[tex[p, k]] == np.inf


def test_taps_follow_the_issue_fan_in_counts():
    """The fan-in the atomics used to serialise: max taps on one texel and untouched texels at the two smaller sizes."""
    for (fw, eh, ew), (most, none) in (((32, 64, 128), (182, 88)), ((256, 512, 1024), (1452, 1112))):
        tex, wt, valid = sr.taps(stitch.sample_grid_numpy(fw, eh, ew), fw)
        cnt = np.bincount(tex[valid & (wt != 0)], minlength=6 * fw * fw)
        assert (cnt.max(), int((cnt == 0).sum())) == (most, none)


# ---------------------------------------------------------------------------- the adjoint plan

def _check_plan(grid, fw):
    offsets, entries = stitch.adjoint_plan(grid, fw)
    texels = 6 * fw * fw
    assert offsets.dtype == np.int32 and entries.dtype == np.int32 and offsets.shape == (texels + 1,)
    assert offsets[0] == 0 and offsets[-1] == entries.size and np.all(np.diff(offsets) >= 0)
    tex, _, valid = sr.taps(grid, fw)
    # every in-range tap exactly once, nothing else
    np.testing.assert_array_equal(np.sort(entries), np.flatnonzero(valid.reshape(-1)))
    # each texel's list is the brute-force inversion, in pixel order
    inv = sr.invert_taps(grid, fw)
    for t in range(texels):
        assert entries[offsets[t]:offsets[t + 1]].tolist() == inv[t], t
    return offsets, entries


@pytest.mark.parametrize("size", [(1, 4, 8), (2, 6, 12), (9, 18, 36), (24, 48, 96)])
def test_adjoint_plan_is_the_brute_force_inverse_of_taps(size):
    fw, eh, ew = size
    _check_plan(stitch.sample_grid_numpy(fw, eh, ew), fw)


@pytest.mark.parametrize("fw", [1, 2, 7])
def test_adjoint_plan_on_synthetic_grids(fw):
    _check_plan(sr.synthetic_grid(np.random.default_rng(fw), 12, 20, fw), fw)


def test_adjoint_plan_size_bound_and_cache():
    offsets, entries = stitch.adjoint_plan_numpy(256, 512, 1024)
    assert entries.size <= 8 * 512 * 1024 and entries.nbytes + offsets.nbytes <= 17 * 2 ** 20
    assert stitch.adjoint_plan_numpy(256, 512, 1024)[1] is entries
    np.testing.assert_array_equal(entries, stitch.adjoint_plan(stitch.sample_grid_numpy(256, 512, 1024), 256)[1])


def test_module_keeps_the_plan_out_of_its_state_dict():
    mod = stitch.Cube2Equirec(8, 16, 32)
    assert set(mod.state_dict()) == {"sample_grid"}
    off, ent = stitch.adjoint_plan_numpy(8, 16, 32)
    assert mod.plan_offsets.dtype == torch.int32 and np.array_equal(mod.plan_offsets.numpy(), off)
    assert np.array_equal(mod.plan_entries.numpy(), ent)


# ---------------------------------------------------------------------------- the grid at non-power-of-two sizes

@pytest.mark.parametrize("size", [(24, 48, 96), (48, 100, 200)])
def test_sample_grid_matches_the_reference_at_odd_sizes(size):
    fw, eh, ew = size
    g = np.load(G / f"cube2equirec_{fw}_{eh}_{ew}_grid.npz")["grid"]
    got = stitch.sample_grid_numpy(fw, eh, ew)
    assert got.dtype == g.dtype == np.float32
    np.testing.assert_array_equal(got, g)
