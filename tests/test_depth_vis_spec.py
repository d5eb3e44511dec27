"""The numpy statement of the evaluation step's pictures (tests/depth_vis_reference.py) against the reference's own functions as
recorded in tests/golden/depth_vis.npz (tests/golden/make_golden_depth_vis.py), on CPU, and the C ABI of the four entries.

The statement evaluates the normalisation in float64 with one rounding where the reference chains float32 operations, so on the
256 x 256 map a value may cross a bin edge: there no index may differ by more than 1 and at most 1e-3 of the pixels may differ
(a condition set before measuring: 1 pixel of 65 536 differs).  Every smaller map must agree at every pixel.
tests/test_gpu_depth_vis.py holds the kernels to the statement byte for byte; the midpoint test below is what entitles it to."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import depth_vis_reference as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "depth_vis.npz"
BIG = "256x256"


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def names(golden):
    return [str(n) for n in golden["names"]]


def test_fixture_holds_the_cases(golden, names):
    assert names == ["1x1", "1x2", "16x16", "ties", "const", "nopos", "nan", "special", "37x53", BIG]
    m = {n: golden[f"map_{n}"] for n in names}
    assert all(v.dtype == np.float32 for v in m.values())
    assert m["ties"].size > 2 * np.unique(m["ties"]).size                       # heavy ties
    assert np.unique(m["const"]).size == 1 and not (m["nopos"] > 0).any() and (m["nopos"] == 0).sum() == 1
    assert np.isnan(m["nan"]).sum() == 1
    assert np.isinf(m["special"]).sum() == 1 and (m["special"] == 0).sum() == 1 and (m["special"] < 0).sum() == 1
    assert 0.25 < (m["37x53"] == 0).mean() < 0.35 and 0.01 < (m[BIG] == 0).mean() < 0.03
    assert not any(np.isnan(golden[f"prep_{k}_in"]).any() for k in golden["prep_names"])


def test_quantiles_are_bit_equal_to_torch(golden, names):
    for n in names:
        d = golden[f"map_{n}"]
        rng = R.depth_range(d)
        if not (d > 0).any():
            assert rng[0] == d.min() and rng[1] == d.max() and np.isnan(rng[2:]).all()
            continue
        t = torch.from_numpy(d)
        want = np.array([t[t > 0].quantile(0.01).item(), t.view(-1).quantile(0.99).item()], np.float32)
        assert want.tobytes() == golden[f"q_{n}"].tobytes(), n
        assert rng[:2].tobytes() == want.tobytes(), (n, rng, want)


def test_index_maps_equal_the_reference_on_every_small_map(golden, names):
    f32 = R.tables("turbo")[0]
    for n in names:
        if n == BIG:
            continue
        idx = R.depth_index(golden[f"map_{n}"])
        assert np.array_equal(idx, golden[f"idx_{n}"]), n
        assert np.array_equal(R.depth_map(golden[f"map_{n}"]), golden[f"rgb_{n}"]), n
        assert np.array_equal(np.moveaxis(f32[golden[f"idx_{n}"]], -1, 0), golden[f"rgb_{n}"]), n
    for n in ("nan", "const", "1x1"):
        assert (R.depth_index(golden[f"map_{n}"]) == R.BAD).all(), n
    sp, idx = golden["map_special"], R.depth_index(golden["map_special"])
    assert (idx[sp == 0] == 255).all() and (idx[sp < 0] == R.BAD).all() and (idx[np.isinf(sp)] == 0).all()


def test_index_map_of_the_large_map_is_within_one_bin_at_a_thousandth_of_the_pixels(golden):
    idx, ref = R.depth_index(golden[f"map_{BIG}"]).astype(np.int64), golden[f"idx_{BIG}"].astype(np.int64)
    diff = np.abs(idx - ref)
    print("pixels that differ:", int((diff > 0).sum()), "of", diff.size, "largest index difference:", int(diff.max()))
    assert diff.max() <= 1
    assert (diff > 0).mean() <= 1e-3


def test_prep_image_and_colorize_bytes_equal_the_reference(golden):
    for k in golden["prep_names"]:
        assert np.array_equal(R.prep_image(golden[f"prep_{k}_in"]), golden[f"prep_{k}_out"]), k
    assert golden["prep_bchw_out"].shape == (9, 28, 3) and golden["prep_4hw_out"].shape == (11, 13, 4)
    x = golden["cmap_x"]
    for name in R.MAPS:
        assert np.array_equal(R.colorize(x, name), golden[f"cmap_{name}"]), name
        assert np.array_equal(R.colorize(x, name, channels="first"), np.moveaxis(golden[f"cmap_{name}"], -1, 0))
        prep = np.trunc(np.clip(golden[f"cmap_{name}"], 0, 1) * np.float32(255)).astype(np.uint8)
        assert np.array_equal(R.colorize(x, name, out="uint8"), prep), name
    assert (R.colorize(x, "turbo")[0, 0] == 0).all()                            # NaN: black


def test_error_map_is_within_one_bin_at_a_thousandth_of_the_pixels(golden):
    got = R.error_map(golden["err_a"], golden["err_b"])
    ref = np.trunc(np.moveaxis(golden["err_out"], 0, -1) * np.float32(255)).astype(np.uint8)     # the bytes save_image writes
    idx = R.color_index(R.error_value(golden["err_a"], golden["err_b"])).astype(np.int64)
    differs = (got != ref).any(-1)
    print("error-map pixels that differ:", int(differs.sum()), "of", differs.size)
    assert np.abs(idx - golden["err_idx"].astype(np.int64))[differs].max(initial=0) <= 1
    assert differs.mean() <= 1e-3
    assert idx[0, 0] == 0 and idx[0, 1] == 255                                  # zero error; beyond the norm: the last colour


def test_get_colormap_bytes_survive_the_float_round_trip():
    codes = np.arange(256, dtype=np.uint8)
    back = np.trunc(np.clip(codes.astype(np.float32) / np.float32(255), 0, 1) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(back, codes)


def test_no_fixture_logarithm_lies_at_a_float32_rounding_midpoint(golden, names):
    """float32(log(float64 d)) is the one place where the device's float64 log and numpy's could disagree in a byte: only if the
    float64 logarithm lies within their last-bit difference of the midpoint of two float32 values.  No fixture value comes
    within 1e-12 (relative) of one, four orders of magnitude more than a float64 ulp."""
    nearest = np.inf
    for n in names:
        d = golden[f"map_{n}"].astype(np.float64).reshape(-1)
        vals = [d[np.isfinite(d) & (d > 0)]]
        rng = R.depth_range(golden[f"map_{n}"]).astype(np.float64)
        vals.append(rng[:2][np.isfinite(rng[:2]) & (rng[:2] > 0)])
        L = np.log(np.concatenate(vals))
        L = L[L != 0]
        f = L.astype(np.float32)
        other = np.nextafter(f, np.where(L > f.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2
        rel = np.abs(L - mid) / np.abs(L)
        nearest = min(nearest, rel.min(initial=np.inf))
    print("nearest relative distance to a midpoint:", nearest)
    assert nearest > 1e-12


def test_tables_in_the_header_are_the_generators(tmp_path):
    """csrc/s360_colormap_tables.h is what scripts/make_colormap_tables.py writes from the installed matplotlib."""
    import re
    text = (Path(__file__).resolve().parent.parent / "splatter360_amd" / "csrc" / "s360_colormap_tables.h").read_text()
    blocks = re.findall(r"(kCmapF32|kCmapPrep|kCmapByte)\[3\]\[257\]\[3\] = \{(.*?)\};", text, re.S)
    assert [b[0] for b in blocks] == ["kCmapF32", "kCmapPrep", "kCmapByte"]
    parsed = [np.array([float(v.rstrip("f")) for v in re.findall(r"[-+0-9.e]+f?", b[1].replace("{", " ").replace("}", " "))]).reshape(3, 257, 3)
              for b in blocks]
    for i, name in enumerate(R.MAPS):
        f32, prep, byte = R.tables(name)
        assert np.array_equal(parsed[0][i].astype(np.float32), f32), name
        assert np.array_equal(parsed[1][i], prep) and np.array_equal(parsed[2][i], byte), name


def test_abi_size_query_and_bad_arguments():
    from splatter360_amd import _lib
    lib = _lib.lib()
    assert lib.s360_abi_version() == 25
    OK, BADARG, UNSUPPORTED = 0, -1, -4
    n = C.c_size_t(0)
    assert lib.s360_depth_colormap(None, 18, 256, 256, 65536, None, None, None, None, C.byref(n), None) == OK and n.value > 0
    small = n.value
    assert lib.s360_depth_colormap(None, 3, 512, 1024, 512 * 1024, None, None, None, None, C.byref(n), None) == OK and n.value > small
    assert lib.s360_depth_colormap(None, 1, 1, 1, 1, None, None, None, None, C.byref(n), None) == OK and 0 < n.value < small
    assert lib.s360_depth_colormap(None, 1, 4000, 4001, 4000 * 4001, None, None, None, None, C.byref(n), None) == UNSUPPORTED
    assert lib.s360_depth_colormap(None, 1, 4000, 4000, 4000 * 4000, None, None, None, None, C.byref(n), None) == OK
    for bad in ((0, 8, 8, 64), (1, 0, 8, 64), (1, 8, 0, 64), (2, 8, 8, 63)):
        assert lib.s360_depth_colormap(None, *bad, None, None, None, None, C.byref(n), None) == BADARG, bad
    assert lib.s360_depth_colormap(None, 1, 8, 8, 64, None, None, None, None, None, None) == BADARG
    # with a workspace pointer every data pointer is checked before any GPU work
    assert lib.s360_depth_colormap(None, 1, 8, 8, 64, None, None, None, C.c_void_p(256), C.byref(n), None) == BADARG
    assert lib.s360_colorize(None, 16, 0, 0, 0, None, None, None) == BADARG
    assert lib.s360_colorize(C.c_void_p(256), 16, 0, 3, 0, C.c_void_p(256), None, None) == BADARG       # unknown map
    assert lib.s360_colorize(C.c_void_p(256), 16, 5, 0, 1, C.c_void_p(256), None, None) == BADARG       # 16 is no multiple of 5
    assert lib.s360_colorize(C.c_void_p(256), 16, 0, 0, 0, None, None, None) == BADARG                  # no output
    assert lib.s360_prep_image(C.c_void_p(256), 1, 2, 8, 8, C.c_void_p(256), None) == BADARG            # two channels
    assert lib.s360_prep_image(None, 1, 3, 8, 8, C.c_void_p(256), None) == BADARG
    assert lib.s360_prep_image(C.c_void_p(256), 0, 3, 8, 8, C.c_void_p(256), None) == BADARG
    assert lib.s360_error_map(None, C.c_void_p(256), 8, 8, C.c_void_p(256), None) == BADARG
    assert lib.s360_error_map(C.c_void_p(256), C.c_void_p(256), 0, 8, C.c_void_p(256), None) == BADARG
    assert lib.s360_error_string(UNSUPPORTED)
    for name in ("s360_depth_colormap", "s360_colorize", "s360_prep_image", "s360_error_map"):
        assert name in _lib.EXPORTS
