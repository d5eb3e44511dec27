"""The ERP -> cube resampler (csrc/s360_equirec2cube.hip) against its float64 statement (tests/equirec2cube_reference.py) and the
arrays recorded from the reference (tests/golden/equirec2cube.npz).

Bars (derived, not measured).  The kernels form every product and sum in float64 and round once, so
  forward (bilinear, nearest, depth):  |out - ref64| <= 2^-23 |ref64|        (four float64 products err by ~2^-50; one rounding is left)
  backward:                            |d_erp - ref64| <= 2^-23 |ref64| + 1e-12 sum|terms|   (the float64 sum's error, by term count)
  uint8: equal to the reference's output wherever the float64 value's fraction is further than 1e-6 from 0.5.
The measured worst ratios are printed (pytest -s)."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

import equirec2cube_reference as R
import stitch_reference as sr
from splatter360_amd import _lib, equirec2cube as E, stitch

pytestmark = pytest.mark.gpu

G = Path(__file__).resolve().parent / "golden"
SHAPES = ((8, 16, 4), (12, 24, 5), (10, 28, 7), (16, 32, 8), (32, 64, 16))
ODD = ((12, 24, 5), (10, 28, 7))
CASES = [(s, 1, 3) for s in SHAPES] + [((12, 24, 5), 3, 5)]            # (shape, B, C): the last runs the batch loop, C % 4 != 0
CASE_IDS = ["x".join(map(str, s)) + f"-b{b}c{c}" for s, b, c in CASES]
FWD_BAR = 2.0 ** -23
SENTINEL = 1234.5


@lru_cache(maxsize=None)
def _golden():
    return np.load(G / "equirec2cube.npz")


def _g(shape, key):
    return _golden()[f"e2c_{shape[0]}_{shape[1]}_{shape[2]}_{key}"]


@lru_cache(maxsize=None)
def _taps(shape, mode, boundary):
    h, w, fw = shape
    cy, cx = R.coordinates(h, w, fw)
    return cy, cx, R.taps(cy, cx, h, w, mode, boundary)


@lru_cache(maxsize=None)
def _erp(shape, b, c, seed=0):
    """float32 values; some planes carry mixed signs, one is all positive (a distance map needs that)."""
    h, w, _ = shape
    x = np.random.default_rng(seed).standard_normal((b, c, h, w)).astype(np.float32)
    x[:, 0] = np.abs(x[:, 0]) + 0.25
    x.setflags(write=False)
    return x


def _fwd_ratio(got, want):
    """max |got - want| / (2^-23 |want|); elements whose reference is 0 must be 0."""
    got = got.astype(np.float64)
    zero = want == 0
    assert np.all(got[zero] == 0)
    return float((np.abs(got - want)[~zero] / (FWD_BAR * np.abs(want[~zero]))).max()) if (~zero).any() else 0.0


def _kinds(shape):
    out = [("bilinear", "reference"), ("nearest", "reference"), ("depth", "reference")]
    return out + [(k, "periodic") for k, _ in out] if shape in ODD else out


def _module(shape, boundary, dev):
    return E.Equirec2Cube(*shape, boundary=boundary).to(dev)


def _run(m, x, kind, order=None):
    if kind == "depth":
        return m._resample(x, "nearest", order, scale=m.cosmaps)
    return m._resample(x, kind, order)


def _ref_forward(shape, x, kind, boundary):
    mode = "nearest" if kind == "depth" else kind
    cy, cx, tp = _taps(shape, mode, boundary)
    return R.forward64(x, cy, cx, mode, boundary, R.cosmap(shape[2]) if kind == "depth" else None, tp=tp)


# ---------------------------------------------------------------------------- forward

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_forward_float32_is_the_float64_statement_rounded_once(gpu, case):
    shape, b, c = case
    x = _erp(shape, b, c)
    xt = torch.from_numpy(x.copy()).to(gpu)
    for kind, boundary in _kinds(shape):
        m = _module(shape, boundary, gpu)
        got = _run(m, xt, kind).cpu().numpy()
        want = _ref_forward(shape, x, kind, boundary)
        assert got.shape == want.shape == (b, c, shape[2], 6 * shape[2]) and got.dtype == np.float32
        r = _fwd_ratio(got, want)
        print(f"forward {shape} b{b} c{c} {kind} {boundary}: worst |err| / (2^-23 |ref|) = {r:.3f}")
        assert r <= 1.0
        if kind == "nearest":
            assert np.array_equal(got.astype(np.float64), want)                     # a copy is exact


def test_forward_at_the_hm3d_shape_against_the_statement(gpu):
    shape = (512, 1024, 256)
    x = _erp(shape, 1, 2, seed=4)
    m = _module(shape, "reference", gpu)
    xt = torch.from_numpy(x.copy()).to(gpu)
    for kind in ("bilinear", "depth"):
        got = _run(m, xt[:, :1], kind).cpu().numpy()
        r = _fwd_ratio(got, _ref_forward(shape, x[:, :1], kind, "reference"))
        print(f"forward {shape} {kind}: worst |err| / (2^-23 |ref|) = {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_uint8_equals_the_reference_except_at_near_ties(gpu, shape):
    h, w, fw = shape
    m = _module(shape, "reference", gpu)
    u8 = torch.from_numpy(_g(shape, "u8").transpose(2, 0, 1)[None].copy()).to(gpu)
    got = m(u8)
    assert got.dtype == torch.uint8 and got.shape == (1, 3, fw, 6 * fw)
    got = got[0].cpu().numpy().transpose(1, 2, 0)
    want = _g(shape, "u8_out")
    t = R.forward64(_g(shape, "u8").transpose(2, 0, 1), _g(shape, "coor_y"), _g(shape, "coor_x")).transpose(1, 2, 0)
    near = np.abs(t - np.floor(t) - 0.5) <= 1e-6
    print(f"uint8 {shape}: {int(near.sum())} near ties of {near.size}, {int((got != want).sum())} elements differ")
    assert np.array_equal(got[~near], want[~near])
    assert np.all(np.abs(got[near].astype(int) - want[near].astype(int)) <= 1)
    if fw % 2 == 0:
        assert near.mean() <= 0.001
    elif shape == (12, 24, 5):
        assert near.mean() <= 0.10
    # nearest: a copy of the texel; faces(): the same through the strided store
    assert np.array_equal(m(u8, mode="nearest")[0].cpu().numpy(),
                          R.forward64(_g(shape, "u8").transpose(2, 0, 1), _g(shape, "coor_y"), _g(shape, "coor_x"), "nearest").astype(np.uint8))
    assert np.array_equal(m.faces(u8, order="rendered").cpu().numpy(), R.split_faces(m(u8).cpu().numpy(), "rendered"))


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_run_matches_the_golden_run_outputs(gpu, shape):
    h, w, fw = shape
    m = _module(shape, "reference", gpu)
    img, dist = torch.from_numpy(_g(shape, "img")).to(gpu), torch.from_numpy(_g(shape, "dist")).to(gpu)
    cube_img, cube_dep = m.run(img, dist)
    for got, key in ((cube_img, "img_out"), (cube_dep, "dep_out"), (m.run(img), "img_out"), (m.run(torch.from_numpy(_g(shape, "u8")).to(gpu)), "u8_out")):
        want = _g(shape, key)
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype, key
        if key == "u8_out":
            t = R.forward64(_g(shape, "u8").transpose(2, 0, 1), _g(shape, "coor_y"), _g(shape, "coor_x")).transpose(1, 2, 0)
            keep = np.abs(t - np.floor(t) - 0.5) > 1e-6
            assert np.array_equal(got[keep], want[keep])
        else:
            want64 = _g(shape, "img_out64") if key == "img_out" else want.astype(np.float64)
            assert _fwd_ratio(got, want64) <= 1.0, key


# ---------------------------------------------------------------------------- backward

@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_backward_is_the_float64_adjoint_rounded_once_and_reproducible(gpu, case):
    shape, b, c = case
    h, w, fw = shape
    x = torch.from_numpy(_erp(shape, b, c).copy()).to(gpu)
    g = np.random.default_rng(7).standard_normal((b, c, fw, 6 * fw)).astype(np.float32)
    gt = torch.from_numpy(g).to(gpu)
    for kind, boundary in _kinds(shape):
        mode = "nearest" if kind == "depth" else kind
        m = _module(shape, boundary, gpu)
        runs = []
        for _ in range(2):
            leaf = x.clone().requires_grad_(True)
            (d,) = torch.autograd.grad(_run(m, leaf, kind), leaf, gt)
            runs.append(d)
        assert torch.equal(runs[0], runs[1])
        got = runs[0].cpu().numpy().astype(np.float64)
        cy, cx, tp = _taps(shape, mode, boundary)
        scale = R.cosmap(fw) if kind == "depth" else None
        want = R.adjoint64(g, cy, cx, h, w, mode, boundary, scale, tp=tp)
        terms = R.adjoint64(g, cy, cx, h, w, mode, boundary, scale, tp=tp, absolute=True)
        bar = FWD_BAR * np.abs(want) + 1e-12 * terms
        err = np.abs(got - want)
        unread = R.read_counts(cy, cx, h, w, mode, boundary) == 0
        assert unread.any() and np.all(got[:, :, unread] == 0)                      # texels no tap reads are exactly 0
        r = float((err[bar > 0] / bar[bar > 0]).max())
        print(f"backward {shape} b{b} c{c} {kind} {boundary}: worst |err| / bar = {r:.3f}")
        assert np.all(err <= bar)


# ---------------------------------------------------------------------------- face map, strided output, round trip

def _to_faces(cube, order):
    """torch: [B,C,fw,6fw] -> [B,6,C,fw,fw], the reorder + flip of the loader for "rendered"."""
    fw = cube.shape[-2]
    f = torch.stack(cube.split(fw, dim=-1), 1)
    if order == "slots":
        return f
    return torch.stack([f[:, c & 7].flip(-1, -2) if c & 8 else f[:, c & 7] for c in E.RENDERED_FACE_MAP], 1)


@pytest.mark.parametrize("order", ["slots", "rendered"])
@pytest.mark.parametrize("kind", ["bilinear", "nearest", "depth"])
def test_faces_equal_the_slot_plane_permuted_and_flipped_with_its_gradient(gpu, kind, order):
    shape, b, c = (12, 24, 5), 3, 5
    fw = shape[2]
    m = _module(shape, "reference", gpu)
    x = torch.from_numpy(_erp(shape, b, c).copy()).to(gpu)
    g = torch.from_numpy(np.random.default_rng(9).standard_normal((b, 6, c, fw, fw)).astype(np.float32)).to(gpu)
    a, p = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    direct = _run(m, a, kind, order)
    composed = _to_faces(_run(m, p, kind), order)
    assert direct.shape == (b, 6, c, fw, fw) and direct.is_contiguous() and torch.equal(direct, composed)
    assert np.array_equal(direct.detach().cpu().numpy(), R.split_faces(_run(m, x, kind).cpu().numpy(), order))
    (ga,), (gp,) = torch.autograd.grad(direct, a, g), torch.autograd.grad(composed, p, g)
    assert torch.equal(ga, gp)
    if kind == "depth":
        assert torch.equal(m.depth_faces(x[:, :1], order), direct.detach()[:, :, :1])
    elif order == "rendered":
        assert torch.equal(m.faces(x, order="rendered", mode=kind), direct.detach())


@pytest.mark.parametrize("shape", [(12, 24, 5), (16, 32, 8)], ids=["12x24x5", "16x32x8"])
def test_round_trip_through_the_stitch_against_the_two_statements(gpu, shape):
    h, w, fw = shape
    x = _erp(shape, 1, 3)
    xt = torch.from_numpy(x.copy()).to(gpu)
    e2c, c2e = _module(shape, "reference", gpu), stitch.Cube2Equirec(fw, h, w).to(gpu)
    got = c2e(e2c(xt))
    rendered = c2e.stitch_rendered(e2c.faces(xt, order="rendered")[0])
    assert got.shape == (1, 3, h, w) and torch.equal(rendered, got[0])             # the fused orders cancel
    cube64 = _ref_forward(shape, x, "bilinear", "reference")[0]                      # [3, fw, 6 fw]
    faces64 = R.split_faces(cube64).astype(np.float64)                               # [6, 3, fw, fw] slot order
    grid = stitch.sample_grid_numpy(fw, h, w)
    tp = sr.taps(grid, fw)
    want = sr.forward64(faces64, grid, tp=tp)
    # the stitch's own bar (8 * 2^-24 * sum|v w|, tests/test_gpu_stitch_parity.py) on an input within 2^-23 of cube64, plus that
    # input error carried through the stitch's non-negative weights
    absf = sr.abs_forward64(faces64, grid, tp=tp)
    bar = (8.0 * 2.0 ** -24 * (1 + FWD_BAR) + FWD_BAR) * absf
    err = np.abs(got[0].cpu().numpy().astype(np.float64) - want)
    print(f"round trip {shape}: worst |err| / bar = {float((err[bar > 0] / bar[bar > 0]).max()):.3f}")
    assert np.all(err <= bar)


# ---------------------------------------------------------------------------- the C ABI: every element written, nothing outside

def _guarded(n, dev, fill=float("nan")):
    """A float32 buffer of n elements between two sentinel guards of 256: (whole, view of the middle)."""
    whole = torch.full((n + 512,), SENTINEL, dtype=torch.float32, device=dev)
    whole[256:256 + n] = fill
    return whole, whole[256:256 + n]


def _guards_intact(whole, n):
    return bool((whole[:256] == SENTINEL).all() and (whole[256 + n:] == SENTINEL).all())


def _abi_forward(x, coor, scale, out, fw, mode, boundary, face_map=None, strides=None):
    b, c, h, w = x.shape
    st = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    return _lib.lib().s360_erp2cube_forward(C.c_void_p(x.data_ptr()), C.c_void_p(coor.data_ptr()),
                                            None if scale is None else C.c_void_p(scale.data_ptr()), C.c_void_p(out.data_ptr()),
                                            b, c, h, w, fw, mode, boundary, 0, None if face_map is None else (C.c_int32 * 6)(*face_map),
                                            None if strides is None else (C.c_int64 * 4)(*strides), st)


def _abi_backward(g, coor, scale, offs, ents, out, b, c, h, w, fw, mode, boundary, face_map=None, strides=None):
    st = C.c_void_p(torch.cuda.current_stream(g.device).cuda_stream)
    return _lib.lib().s360_erp2cube_backward(C.c_void_p(g.data_ptr()), C.c_void_p(coor.data_ptr()),
                                             None if scale is None else C.c_void_p(scale.data_ptr()), C.c_void_p(offs.data_ptr()),
                                             C.c_void_p(ents.data_ptr()), C.c_void_p(out.data_ptr()), b, c, h, w, fw, mode, boundary,
                                             None if face_map is None else (C.c_int32 * 6)(*face_map),
                                             None if strides is None else (C.c_int64 * 4)(*strides), st)


def _wild_plane(fw, h, w):
    """A coordinate plane [fw, 6 fw, 2] of finite values far outside the image, on its edges, and just beyond them."""
    rng = np.random.default_rng(11)
    vals = np.float32([-1e30, -3e9, -70000.25, -1.0, -0.5, -1e-7, 0.0, h - 1, h - 0.5, h, h + 1, h + 1.5, w - 1, w - 0.5, w, w + 0.25,
                       2.5 * w, 65536.75, 3e9, 1e30, 3.4e38, -3.4e38])
    plane = rng.choice(vals, (fw, 6 * fw, 2)).astype(np.float32)
    plane.reshape(-1, 2)[:len(vals), 0] = vals
    plane.reshape(-1, 2)[:len(vals), 1] = vals[::-1]
    return plane


@pytest.mark.parametrize("boundary", ["reference", "periodic"])
@pytest.mark.parametrize("wild", [False, True], ids=["module-plane", "wild-plane"])
def test_c_abi_writes_every_output_element_and_nothing_else(gpu, boundary, wild):
    shape, b, c = (12, 24, 5), 3, 5
    h, w, fw = shape
    bnd = E.BOUNDARIES[boundary]
    plane = _wild_plane(fw, h, w) if wild else E.coordinates_numpy(h, w, fw)
    coor = torch.from_numpy(np.ascontiguousarray(plane).copy()).to(gpu)
    cos = torch.from_numpy(E.cosmap_numpy(fw).copy()).to(gpu)
    x = torch.from_numpy(_erp(shape, b, c).copy()).to(gpu)
    n_out, n_in = b * c * fw * 6 * fw, b * c * h * w
    layouts = ((None, None), (E.RENDERED_FACE_MAP, (6 * c * fw * fw, c * fw * fw, fw * fw, fw)))
    for mode, scale in ((0, None), (1, None), (1, cos)):
        name = "nearest" if mode else "bilinear"
        offs, ents = (torch.from_numpy(a).to(gpu) for a in E.adjoint_plan(plane, h, w, boundary, name))
        for face_map, strides in layouts:
            whole, out = _guarded(n_out, gpu)
            assert _abi_forward(x, coor, scale, out, fw, mode, bnd, face_map, strides) == 0
            torch.cuda.synchronize()
            assert _guards_intact(whole, n_out) and bool(torch.isfinite(out).all())
            if mode == 1 and scale is None:       # a copy of the clamped tap: the kernel's index rule is the plan's, wild values included
                tex = torch.from_numpy(E.tap_texels(plane, h, w, boundary, "nearest")[:, 0]).to(gpu)
                want = x.reshape(b, c, h * w)[:, :, tex].reshape(b, c, fw, 6 * fw)
                got = out.view(b, c, fw, 6 * fw) if strides is None else None
                assert got is None or torch.equal(got, want)
                if strides is not None:
                    assert torch.equal(out.view(b, 6, c, fw, fw), _to_faces(want, "rendered"))
            g = torch.from_numpy(np.random.default_rng(5).standard_normal(n_out).astype(np.float32)).to(gpu)
            whole, d = _guarded(n_in, gpu)
            assert _abi_backward(g, coor, scale, offs, ents, d, b, c, h, w, fw, mode, bnd, face_map, strides) == 0
            torch.cuda.synchronize()
            assert _guards_intact(whole, n_in) and bool(torch.isfinite(d).all())
            if mode == 1 and scale is None and strides is None:
                zeros = torch.zeros(b * c, h * w, dtype=torch.float64, device=gpu)
                want = zeros.index_add(1, tex, g.view(b * c, -1).double())
                terms = zeros.index_add(1, tex, g.view(b * c, -1).double().abs())
                assert bool(((d.view(b * c, -1).double() - want).abs() <= FWD_BAR * want.abs() + 1e-12 * terms).all())


def test_cpu_tensors_raise(gpu):
    m = E.Equirec2Cube(12, 24, 5)
    for call in (lambda: m(torch.zeros(1, 3, 12, 24)), lambda: m.faces(torch.zeros(1, 3, 12, 24, dtype=torch.uint8)),
                 lambda: m.depth_faces(torch.zeros(1, 1, 12, 24)), lambda: m.run(torch.zeros(12, 24, 3))):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        m.to(gpu)(torch.zeros(1, 3, 12, 25, device=gpu))
