"""The ERP -> cube resampler's CPU-checkable parts: the numpy statement of tests/equirec2cube_reference.py against the arrays the
reference produced (tests/golden/equirec2cube.npz, recorded by tests/golden/make_golden_equirec2cube.py) and against scipy itself,
the package's coordinate plane, cosmap and adjoint plan, the two boundary rules, the rendered face order, and the C ABI's two new
symbols.  The GPU half is tests/test_gpu_equirec2cube.py."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import equirec2cube_reference as R
from splatter360_amd import _lib, equirec2cube as E, stitch

G = Path(__file__).resolve().parent / "golden"
SHAPES = ((8, 16, 4), (12, 24, 5), (10, 28, 7), (16, 32, 8), (32, 64, 16))
ODD = ((12, 24, 5), (10, 28, 7))
IDS = ["x".join(map(str, s)) for s in SHAPES]


@pytest.fixture(scope="module")
def golden():
    g = np.load(G / "equirec2cube.npz")
    assert [tuple(s) for s in g["shapes"].tolist()] == list(SHAPES)
    return {s: {k[len(f"e2c_{s[0]}_{s[1]}_{s[2]}_"):]: g[k] for k in g.files if k.startswith(f"e2c_{s[0]}_{s[1]}_{s[2]}_")} for s in SHAPES}


def test_golden_file_holds_arrays_only_and_is_small():
    assert (G / "equirec2cube.npz").stat().st_size < 200 * 1024
    g = np.load(G / "equirec2cube.npz", allow_pickle=False)
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_statement_reproduces_every_golden_array_exactly(golden, shape):
    h, w, fw = shape
    g = golden[shape]
    cy, cx = R.coordinates(h, w, fw)
    for got, key in ((cy, "coor_y"), (cx, "coor_x"), (R.cosmap(fw), "cosmaps")):
        assert got.dtype == np.float32 and np.array_equal(got, g[key]), key
    out64 = R.forward64(g["img"].transpose(2, 0, 1), cy, cx).transpose(1, 2, 0)
    assert np.array_equal(out64, g["img_out64"])
    assert np.array_equal(out64.astype(np.float32), g["img_out"])
    assert np.array_equal(R.to_uint8(R.forward64(g["u8"].transpose(2, 0, 1), cy, cx)).transpose(1, 2, 0), g["u8_out"])
    dep = R.forward64(g["dist"].transpose(2, 0, 1), cy, cx, mode="nearest", scale=R.cosmap(fw)).transpose(1, 2, 0)
    assert np.array_equal(dep.astype(np.float32), g["dep_out"])


def test_statement_reproduces_map_coordinates_at_the_hm3d_shape():
    ndimage = pytest.importorskip("scipy.ndimage")
    h, w, fw = 512, 1024, 256
    cy, cx = R.coordinates(h, w, fw)
    erp = np.random.default_rng(1).standard_normal((h, w)).astype(np.float32).astype(np.float64)
    pad = np.concatenate([erp, np.roll(erp[[-1]], w // 2, 1), np.roll(erp[[0]], w // 2, 1)], 0)       # util.py:72-74
    for order, mode in ((1, "bilinear"), (0, "nearest")):
        want = ndimage.map_coordinates(pad, [cy, cx], order=order, mode="wrap")
        assert np.array_equal(R.forward64(erp, cy, cx, mode=mode), want), mode
    assert 0.0 < cy.min() and cy.max() < h - 1 and 0.0 < cx.min() and cx.max() < w - 1     # even face_w: no wrap, no pole row


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_package_coordinates_and_cosmap_equal_the_golden_bit_for_bit(golden, shape):
    h, w, fw = shape
    coor = E.coordinates_numpy(h, w, fw)
    assert coor.dtype == np.float32 and coor.shape == (fw, 6 * fw, 2)
    assert np.array_equal(coor[..., 0], golden[shape]["coor_y"]) and np.array_equal(coor[..., 1], golden[shape]["coor_x"])
    cos = E.cosmap_numpy(fw)
    assert cos.dtype == np.float32 and np.array_equal(cos, golden[shape]["cosmaps"])
    assert E.coordinates_numpy(h, w, fw) is coor and E.cosmap_numpy(fw) is cos               # cached


def test_odd_face_widths_reach_the_wrap_and_the_pole_rows(golden):
    """(12, 24, 5): x up to 23.5 > W - 1 and y from -0.5 to 11.5 > H - 1, so scipy's period-(n - 1) wrap and both pole rows run."""
    g = golden[(12, 24, 5)]
    assert g["coor_x"].max() == 23.5 and g["coor_y"].min() == -0.5 and g["coor_y"].max() == 11.5
    pole = R.taps(g["coor_y"], g["coor_x"], 12, 24)[3]
    assert pole.any()
    # the quirk: coor_x = W - 0.5 blends columns 0 and 1, not W - 1 and 0
    i = int(np.argmax(g["coor_x"].reshape(-1)))
    tex = R.taps(g["coor_y"], g["coor_x"], 12, 24)[0][i]
    assert sorted(set((tex % 24).tolist())) == [0, 1]
    texp = R.taps(g["coor_y"], g["coor_x"], 12, 24, boundary="periodic")[0][i]
    assert sorted(set((texp % 24).tolist())) == [0, 23]


@pytest.mark.parametrize("boundary", ["reference", "periodic"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", ODD, ids=["12x24x5", "10x28x7"])
def test_adjoint_statement_agrees_with_central_differences(shape, mode, boundary):
    h, w, fw = shape
    cy, cx = R.coordinates(h, w, fw)
    rng = np.random.default_rng(3)
    erp, g = rng.standard_normal((2, h, w)), rng.standard_normal((2, fw, 6 * fw))
    scale = R.cosmap(fw) if mode == "nearest" else None
    tp = R.taps(cy, cx, h, w, mode, boundary)
    got = R.adjoint64(g, cy, cx, h, w, mode, boundary, scale, tp=tp)
    eps = 0.5
    want = np.zeros_like(erp)
    for p in range(2):
        for i in range(h * w):
            d = np.zeros_like(erp)
            d[p].reshape(-1)[i] = eps
            hi = (g * R.forward64(erp + d, cy, cx, mode, boundary, scale, tp=tp)).sum()
            lo = (g * R.forward64(erp - d, cy, cx, mode, boundary, scale, tp=tp)).sum()
            want[p].reshape(-1)[i] = (hi - lo) / (2 * eps)
    scale_ = R.adjoint64(g, cy, cx, h, w, mode, boundary, scale, tp=tp, absolute=True)
    assert np.all(np.abs(got - want) <= 1e-11 * (scale_ + np.abs(g).sum()))          # linear map: only rounding separates them
    unread = R.read_counts(cy, cx, h, w, mode, boundary) == 0
    assert unread.any() and np.all(got[:, unread] == 0)                              # a texel nobody reads gets 0


@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_boundary_rules_agree_except_on_a_face_centre_row_or_column(golden, shape, mode):
    h, w, fw = shape
    g = golden[shape]
    img = g["img"].transpose(2, 0, 1)
    a = R.forward64(img, g["coor_y"], g["coor_x"], mode, "reference")
    b = R.forward64(img, g["coor_y"], g["coor_x"], mode, "periodic")
    differ = (a != b).any(0)
    if fw % 2 == 0:
        assert not differ.any()
        return
    rows, cols = np.nonzero(differ)
    assert len(rows) > 0 and np.all((rows == fw // 2) | (cols % fw == fw // 2))


@pytest.mark.parametrize("boundary", ["reference", "periodic"])
@pytest.mark.parametrize("mode", ["bilinear", "nearest"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan_lists_every_tap_once_under_its_real_texel(golden, shape, mode, boundary):
    h, w, fw = shape
    g = golden[shape]
    coor = E.coordinates_numpy(h, w, fw)
    offs, ents = E.adjoint_plan_numpy(h, w, fw, boundary, mode)
    assert offs.dtype == np.int32 and ents.dtype == np.int32 and offs.shape == (h * w + 1,) and offs[0] == 0 and offs[-1] == len(ents)
    k = 4 if mode == "bilinear" else 1
    n = 6 * fw * fw
    want = np.sort((np.arange(n)[:, None] * 4 + np.arange(k)[None]).reshape(-1))
    assert np.array_equal(np.sort(ents), want)                                    # every (cube texel, tap) exactly once
    inv = R.invert_taps(g["coor_y"], g["coor_x"], h, w, mode, boundary)           # the statement's taps, inverted by brute force
    assert [ents[offs[e]:offs[e + 1]].tolist() for e in range(h * w)] == inv
    assert E.adjoint_plan(coor, h, w, boundary, mode)[1].tolist() == ents.tolist()
    # pole-row taps sit under a texel of row 0 or H - 1, at the column rolled by W // 2
    tex, _, _, pole = R.taps(g["coor_y"], g["coor_x"], h, w, mode, boundary)
    where = np.repeat(np.arange(h * w), np.diff(offs))
    owner = dict(zip(ents.tolist(), where.tolist()))
    for t, kk in zip(*np.nonzero(pole)):
        e = owner[int(t) * 4 + int(kk)]
        assert e == tex[t, kk] and e // w in (0, h - 1)
    assert pole.any() == (fw % 2 == 1)


def test_rendered_order_followed_by_change_order_is_slot_order():
    g = np.load(G / "change_order.npz")
    inp, out = g["inp"], g["out"]                                     # out = change_order(inp), recorded from the reference
    assert len(np.unique(inp)) == inp.size                            # index-valued: the recorded pair defines the permutation
    pos = {v: i for i, v in enumerate(inp.reshape(-1).tolist())}
    perm = np.array([pos[v] for v in out.reshape(-1).tolist()])

    def change_order(x):
        return x.reshape(-1)[perm].reshape(x.shape)

    rng = np.random.default_rng(0)
    slots = rng.standard_normal(inp.shape).astype(np.float32)          # [6, C, fw, fw] in slot order
    cube = R.join_faces(slots)
    rendered = R.split_faces(cube, "rendered")
    assert np.array_equal(change_order(rendered), slots)
    assert np.array_equal(R.join_faces(rendered, "rendered"), cube)
    # and the package's map is the inverse of the stitch's
    assert E.RENDERED_FACE_MAP == R.RENDERED
    for j, code in enumerate(E.RENDERED_FACE_MAP):
        assert stitch.CHANGE_ORDER_FACE_MAP[code & 7] == (j | (code & 8))


def test_uint8_near_ties_of_the_reference_stay_within_the_caps(golden):
    """The GPU test lets an element differ by one level only where the float64 value's fraction is within 1e-6 of 0.5; this is how
    often that happens (at most 0.1 % at the even shapes, 10 % at (12, 24, 5))."""
    for shape in SHAPES:
        g = golden[shape]
        t = R.forward64(g["u8"].transpose(2, 0, 1), g["coor_y"], g["coor_x"])
        near = np.abs(t - np.floor(t) - 0.5) <= 1e-6
        print(shape, int(near.sum()), "of", near.size)
        if shape[2] % 2 == 0:
            assert near.mean() <= 0.001
        elif shape == (12, 24, 5):
            assert near.mean() <= 0.10


def test_module_buffers_are_not_persistent_and_cpu_tensors_raise():
    import torch
    m = E.Equirec2Cube(12, 24, 5)
    assert (m.equ_h, m.equ_w, m.face_w, m.boundary) == (12, 24, 5, "reference")
    assert len(m.state_dict()) == 0 and {"coor", "cosmaps", "plan_offsets_bilinear", "plan_entries_nearest"} <= dict(m.named_buffers()).keys()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 12, 24))
    with pytest.raises(RuntimeError):
        m.faces(torch.zeros(1, 3, 12, 24), order="rendered")
    with pytest.raises(ValueError):
        E.Equirec2Cube(12, 24, 5, boundary="clamp")
    import splatter360_amd
    assert splatter360_amd.Equirec2Cube is E.Equirec2Cube


def test_abi_entries_reject_null_pointers_and_bad_sizes():
    lib = _lib.lib()
    assert {"s360_erp2cube_forward", "s360_erp2cube_backward"} <= set(_lib.EXPORTS) and _lib.ABI_VERSION == 25
    bad = -1                                                           # S360_E_BADARG
    assert lib.s360_erp2cube_forward(None, None, None, None, 1, 3, 12, 24, 5, 0, 0, 0, None, None, None) == bad
    assert lib.s360_erp2cube_backward(None, None, None, None, None, None, 1, 3, 12, 24, 5, 0, 0, None, None, None) == bad
    p = C.c_void_p(64)                                                 # never dereferenced: every call below fails its checks first
    for args in ((0, 3, 12, 24, 5, 0, 0, 0), (1, 0, 12, 24, 5, 0, 0, 0), (1, 3, 0, 24, 5, 0, 0, 0), (1, 3, 12, 1, 5, 0, 0, 0),
                 (1, 3, 12, 24, 0, 0, 0, 0), (1, 3, 12, 24, 5, 2, 0, 0), (1, 3, 12, 24, 5, 0, 2, 0), (1, 3, 12, 24, 5, 0, 0, 2)):
        assert lib.s360_erp2cube_forward(p, p, None, p, *args, None, None, None) == bad, args
    assert lib.s360_erp2cube_forward(p, p, None, p, 1, 3, 12, 24, 5, 0, 0, 0, (C.c_int32 * 6)(0, 1, 2, 3, 4, 6), None, None) == bad
    assert lib.s360_erp2cube_forward(p, p, p, p, 1, 3, 12, 24, 5, 1, 0, 1, None, None, None) == -4      # scaled uint8: unsupported
    for args in ((0, 3, 12, 24, 5, 0, 0), (1, 3, 12, 24, 5, 3, 0), (1, 3, 12, 24, 5, 0, -1), (65535, 5, 12, 24, 5, 0, 0)):
        assert lib.s360_erp2cube_backward(p, p, None, p, p, p, *args, None, None, None) == bad, args
    assert lib.s360_erp2cube_backward(p, p, None, None, p, p, 1, 3, 12, 24, 5, 0, 0, None, None, None) == bad
