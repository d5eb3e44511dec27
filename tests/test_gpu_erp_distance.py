"""GPU tests of the z-depth -> distance kernels and of the fused depth-faces -> ERP distance stitch (splatter360_amd/stitch.py
depth_to_distance, Cube2Equirec.stitch_distance_rendered), on the shapes of tests/golden/erp_distance.npz only.

"ulp" is the float32 spacing at the float64 value.  The bars are derived, not tuned:
  - a value rounded once is within 0.5 ulp of the float64 restatement (tests/erp_distance_reference.py); 1 ulp allows for the
    device's float64 sqrt and division;
  - against the reference's recorded float32 values: |native - ref| <= |ref - f64| + 1 ulp pointwise (the triangle inequality);
  - the fused kernels against the native two-step: equal, by construction (the same device functions in the same order);
  - end to end against the recorded ERP: 2e-6 Dmax (the colour stitch's bar for unit-range inputs,
    tests/test_gpu_stitch_and_decoder.py:23, scaled by the largest finite distance) + the largest tap difference the first bar
    allows; the inf case is compared for its non-finite pattern only."""
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import erp_distance_reference as R
from splatter360_amd import plugin, stitch

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:invalid value encountered")]
GOLD = Path(__file__).resolve().parent / "golden" / "erp_distance.npz"
CLOSURES = [(2, 8, 16, 32), (3, 24, 48, 96)]
FACE_MAP = stitch.CHANGE_ORDER_FACE_MAP


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def modules(gpu):
    return {(fw, eh, ew): stitch.Cube2Equirec(fw, eh, ew).to(gpu) for _, fw, eh, ew in CLOSURES}


def _case(gold, gpu, shape, kind):
    v, fw, eh, ew = shape
    p = f"closure_{fw}_{eh}_{ew}_{kind}_"
    depth = torch.tensor(gold[p + "depth"], device=gpu)
    k4 = torch.tensor(gold[p + "fxfycxcy"], device=gpu).view(v, 6, 4)
    return p, depth, k4


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _equal(a, b):
    """torch.equal, with a NaN equal to a NaN at the same place (an inf texel under a weight 0 gives NaN in both paths)."""
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def _ulp_err(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    return np.abs(got.astype(np.float64) - want)[fin] / R.ulp32(want[fin]), fin


def _reorder(d):
    """change_order_batch without the in-place write: [N,6,fw,fw] rendered -> slot order, faces 0 and 5 flipped on both axes."""
    return torch.stack([d[:, c & 7].flip(-1, -2) if c & 8 else d[:, c & 7] for c in FACE_MAP], 1)


def _two_step(mod, depth, k4, convention):
    """The native two-step the fused kernel must equal bit for bit."""
    n, fw = depth.shape[0], depth.shape[-1]
    if convention == "reference":       # reorder, convert slot s with row s, then Cube2Equirec.forward on the faces side by side
        dist = stitch.depth_to_distance(_reorder(depth), k4.reshape(n * 6, 4), "reference")
        return mod(dist.permute(0, 2, 1, 3).reshape(n, 1, fw, 6 * fw))[:, 0]
    dist = stitch.depth_to_distance(depth, k4.reshape(n * 6, 4), "pixel")      # each face in its own image, then the rendered stitch
    return torch.stack([mod.stitch_rendered(dist[i][:, None])[0] for i in range(n)])


# ---------------------------------------------------------------------------- 1, 2: the stand-alone map and its gradient
@pytest.mark.parametrize("h", [8, 24])
@pytest.mark.parametrize("convention", ["reference", "pixel"])
def test_distance_map_against_float64_and_the_recorded_values(gpu, gold, h, convention):
    p = f"dist_{h}_"
    d, k4 = gold[p + "depth"], gold[p + "fxfycxcy"]
    dt = torch.tensor(d, device=gpu)
    before = _bits(dt).clone()
    got = stitch.depth_to_distance(dt, torch.tensor(k4, device=gpu), convention).cpu().numpy()
    assert torch.equal(_bits(dt), before) and got.dtype == np.float32 and got.shape == d.shape
    want = R.distance64(d, k4, convention)
    err, fin = _ulp_err(got, want)
    print(f"h={h} {convention}: native vs float64 worst {err.max():.3f} ulp")
    assert err.max() <= 1.0
    assert got[d == 0] == 0 and (got[d < 0] > 0).all() and np.isposinf(got[np.isinf(d)]).all()
    if convention == "reference":
        ref = gold[p + "out"].astype(np.float64)
        m = fin & np.isfinite(ref)
        assert m.sum() == d.size - 1
        assert (np.abs(got - ref)[m] <= np.abs(ref - want)[m] + R.ulp32(want[m])).all()


def test_distance_map_non_square_under_pixel_and_leading_dimensions(gpu):
    rng = np.random.default_rng(11)
    d = rng.uniform(-4.0, 9.0, (2, 3, 5, 9)).astype(np.float32)
    k4 = np.stack([rng.uniform(3, 6, 6), rng.uniform(6, 9, 6), rng.uniform(2, 4, 6), rng.uniform(4, 6, 6)], 1).astype(np.float32)
    dt, kt = torch.tensor(d, device=gpu), torch.tensor(k4, device=gpu)
    got = stitch.depth_to_distance(dt, kt, "pixel")
    assert got.shape == dt.shape
    err, _ = _ulp_err(got.cpu().numpy().reshape(6, 5, 9), R.distance64(d.reshape(6, 5, 9), k4, "pixel"))
    assert err.max() <= 1.0
    # a non-contiguous view gives the same bits; the reference convention refuses the shape; N = 0 launches nothing
    assert torch.equal(stitch.depth_to_distance(dt.transpose(0, 1), kt.view(2, 3, 4).transpose(0, 1).reshape(6, 4), "pixel"), got.transpose(0, 1))
    with pytest.raises(ValueError, match="square"):
        stitch.depth_to_distance(dt, kt, "reference")
    with pytest.raises(ValueError):
        stitch.depth_to_distance(dt, kt[:5], "pixel")
    with pytest.raises(ValueError, match="float32"):
        stitch.depth_to_distance(dt.double(), kt, "pixel")
    with pytest.raises(ValueError):
        stitch.depth_to_distance(dt, kt.view(6, 2, 2), "pixel")
    with pytest.raises(RuntimeError, match="GPU only"):
        stitch.depth_to_distance(dt, kt.cpu(), "pixel")
    assert stitch.depth_to_distance(dt[:0], kt[:0], "pixel").shape == (0, 3, 5, 9)


@pytest.mark.parametrize("h", [8, 24])
@pytest.mark.parametrize("convention", ["reference", "pixel"])
def test_distance_gradient_against_float64_and_the_recorded_autograd(gpu, gold, h, convention):
    p = f"dist_{h}_"
    d, k4, g = gold[p + "depth"], gold[p + "fxfycxcy"], gold[p + "gout"]
    leaf = torch.tensor(d, device=gpu, requires_grad=True)
    out = stitch.depth_to_distance(leaf, torch.tensor(k4, device=gpu), convention)
    got = torch.autograd.grad(out, leaf, torch.tensor(g, device=gpu))[0].cpu().numpy()
    want = R.distance_grad64(g, d, k4, convention)
    err, fin = _ulp_err(got, want)
    print(f"h={h} {convention}: native gradient vs float64 worst {err.max():.3f} ulp")
    assert err.max() <= 1.0
    ref = gold[p + "grad"]
    assert np.isnan(ref[d == 0]).all() and (got[d == 0] == 0).all()             # finite where torch's autograd gives NaN
    if convention == "reference":
        m = fin & np.isfinite(ref)
        assert m.sum() >= d.size - 2
        assert (np.abs(got - ref.astype(np.float64))[m] <= np.abs(ref - want)[m] + R.ulp32(want[m])).all()


# ---------------------------------------------------------------------------- 3, 4: the fused stitch is the two-step, bit for bit
@pytest.mark.parametrize("kind", ["hm3d", "pert"])
@pytest.mark.parametrize("convention", ["reference", "pixel"])
@pytest.mark.parametrize("shape", CLOSURES)
def test_fused_forward_equals_the_two_step(gpu, gold, modules, shape, convention, kind):
    _, depth, k4 = _case(gold, gpu, shape, kind)
    mod = modules[shape[1:]]
    before = _bits(depth).clone()
    got = mod.stitch_distance_rendered(depth, k4, convention)
    assert torch.equal(_bits(depth), before)                                    # change_order_batch would have flipped faces 0 and 5
    want = _two_step(mod, depth, k4, convention)
    assert got.shape == (shape[0], shape[2], shape[3]) and got.dtype == torch.float32
    assert _equal(got, want)
    if kind == "hm3d":
        assert torch.equal(got, want) and torch.isfinite(got).all()
    # one panorama as [6, fw, fw], with [6, 4] and with [1, 6, 4] intrinsics
    one = mod.stitch_distance_rendered(depth[1], k4[1], convention)
    assert one.shape == got.shape[1:] and _equal(one, got[1])
    assert _equal(mod.stitch_distance_rendered(depth[1], k4[1:2], convention), got[1])
    # a non-contiguous input gives the bits of its contiguous copy
    dt = depth.transpose(-1, -2)
    assert not dt.is_contiguous() and _equal(mod.stitch_distance_rendered(dt, k4, convention), mod.stitch_distance_rendered(dt.contiguous(), k4, convention))


@pytest.mark.parametrize("kind", ["hm3d", "pert"])
@pytest.mark.parametrize("convention", ["reference", "pixel"])
@pytest.mark.parametrize("shape", CLOSURES)
def test_fused_backward_equals_the_two_steps_autograd(gpu, gold, modules, shape, convention, kind):
    _, depth, k4 = _case(gold, gpu, shape, kind)
    mod = modules[shape[1:]]
    gen = torch.Generator(device=gpu).manual_seed(7)
    g = torch.randn(shape[0], shape[2], shape[3], device=gpu, generator=gen)
    before = _bits(depth).clone()
    leaf = depth.clone().requires_grad_(True)
    got = torch.autograd.grad(mod.stitch_distance_rendered(leaf, k4, convention), leaf, g)[0]
    assert torch.equal(_bits(leaf), before)
    leaf2 = depth.clone().requires_grad_(True)
    want = torch.autograd.grad(_two_step(mod, leaf2, k4, convention), leaf2, g)[0]
    assert got.shape == depth.shape and torch.isfinite(got).all()               # sign(d) s is finite at the inf depth too
    assert torch.equal(got, want)
    assert (got[depth == 0] == 0).all()
    # against float64: a texel's m products and m float32 additions in plan order each round once (<= (m + 1) 2^-24 of the sum of
    # |terms| to first order; + 1 for the higher orders), then the product with sign(d) s rounds once (2^-24 of the value, stated as
    # 2^-23).  The restatement takes the same float32 weights.
    grid = stitch.sample_grid_numpy(*shape[1:])
    m = int(np.diff(stitch.adjoint_plan_numpy(*shape[1:])[0]).max())
    d64 = depth.cpu().numpy()
    d64 = np.where(np.isfinite(d64), d64, 1.0)
    want64 = R.stitch_distance_grad64(g.cpu().numpy(), d64, k4.cpu().numpy(), grid, convention)
    terms = R.stitch_distance_grad64(np.abs(g.cpu().numpy()), np.abs(d64), k4.cpu().numpy(), grid, convention)
    assert (np.abs(got.cpu().numpy() - want64) <= 2.0 ** -23 * np.abs(want64) + (m + 2) * 2.0 ** -24 * terms).all()
    if shape[0] > 1:                                                            # one panorama as [6, fw, fw]
        leaf3 = depth[1].clone().requires_grad_(True)
        one = torch.autograd.grad(mod.stitch_distance_rendered(leaf3, k4[1], convention), leaf3, g[1])[0]
        assert torch.equal(one, got[1])


# ---------------------------------------------------------------------------- 5: end to end against the reference's recorded ERP
@pytest.mark.parametrize("kind", ["hm3d", "pert"])
@pytest.mark.parametrize("shape", CLOSURES)
def test_fused_stitch_against_the_recorded_erp(gpu, gold, modules, shape, kind):
    p, depth, k4 = _case(gold, gpu, shape, kind)
    v, fw = shape[0], shape[1]
    # intrinsics as a user makes them: the reference's float32 products of the normalised matrices
    k_user = stitch.fxfycxcy_from_intrinsics(torch.tensor(gold[p + "intrinsics"], device=gpu), fw, fw)
    assert torch.equal(k_user, k4)
    got = modules[shape[1:]].stitch_distance_rendered(depth, k_user, "reference").cpu().numpy()
    ref_erp, ref_dist = gold[p + "erp"], gold[p + "dist"].astype(np.float64)
    want_dist = R.slot_distance64(gold[p + "depth"], gold[p + "fxfycxcy"].reshape(v, 6, 4), "reference").reshape(v * 6, fw, fw)
    fin_d = np.isfinite(ref_dist)
    assert np.array_equal(fin_d, np.isfinite(want_dist)) and (~fin_d).sum() == (kind == "pert")
    dmax = np.abs(ref_dist[fin_d]).max()
    tap = (np.abs(ref_dist - want_dist)[fin_d] + R.ulp32(want_dist[fin_d])).max()
    fin = np.isfinite(ref_erp)
    assert np.array_equal(fin, np.isfinite(got))                                # the inf texel's footprint: pattern only
    err = np.abs(got.astype(np.float64) - ref_erp)[fin].max()
    print(f"{p}: worst |erp - recorded| {err:.3g}, bar {2e-6 * dmax + tap:.3g} (Dmax {dmax:.4g})")
    assert err <= 2e-6 * dmax + tap


# ---------------------------------------------------------------------------- 6: determinism
def test_forward_and_backward_are_bit_identical_run_to_run(gpu, gold, modules):
    shape = CLOSURES[1]
    _, depth, k4 = _case(gold, gpu, shape, "pert")
    mod = modules[shape[1:]]
    g = torch.randn(shape[0], shape[2], shape[3], device=gpu, generator=torch.Generator(device=gpu).manual_seed(9))
    runs = []
    for _ in range(2):
        for convention in ("reference", "pixel"):
            leaf = depth.clone().requires_grad_(True)
            erp = mod.stitch_distance_rendered(leaf, k4, convention)
            grad = torch.autograd.grad(erp, leaf, g)[0]
            leaf_d = depth.clone().requires_grad_(True)
            dist = stitch.depth_to_distance(leaf_d, k4.reshape(-1, 4), convention)
            grad_d = torch.autograd.grad(dist, leaf_d, torch.ones_like(dist))[0]
            runs.append([_bits(t).clone() for t in (erp, grad, dist, grad_d)])
    for a, b in zip(runs[:2], runs[2:]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_stitch_argument_checks(gpu, gold, modules):
    shape = CLOSURES[0]
    _, depth, k4 = _case(gold, gpu, shape, "hm3d")
    mod = modules[shape[1:]]
    with pytest.raises(ValueError):
        mod.stitch_distance_rendered(depth[:, :5], k4)
    with pytest.raises(ValueError):
        mod.stitch_distance_rendered(depth, k4[:1])
    with pytest.raises(ValueError, match="float32"):
        mod.stitch_distance_rendered(depth.double(), k4)
    with pytest.raises(RuntimeError, match="GPU only"):
        mod.stitch_distance_rendered(depth, k4.cpu())
    with pytest.raises(ValueError):
        modules[CLOSURES[1][1:]].stitch_distance_rendered(depth, k4)            # another face width
    assert mod.stitch_distance_rendered(depth[:0], k4[:0]).shape == (0, shape[2], shape[3])


# ---------------------------------------------------------------------------- 7: the seam
def test_installed_function_returns_the_kernels_bits(gpu, gold, monkeypatch):
    """install(erp_distance=True)'s replacement with the reference-shaped call (model_wrapper_erp.py:454-457: [N, 4] rows broadcast
    to [N, 4, h, w] with strides (4, 1, 0, 0)) runs the kernel; any other input goes to the replaced function."""
    def replaced(depth_maps, fxfycxcy):
        return torch.full_like(depth_maps, -7.0)

    zmod = types.ModuleType(plugin.ERP_DISTANCE_MODULE)
    zmod.depth_to_distance_map_batch = replaced
    user = types.ModuleType(plugin.ERP_DISTANCE_USERS[0])
    user.depth_to_distance_map_batch = replaced
    for m in (zmod, user):
        monkeypatch.setitem(sys.modules, m.__name__, m)
    fn = plugin.install_erp_distance()
    try:
        assert zmod.depth_to_distance_map_batch is fn and user.depth_to_distance_map_batch is fn and fn.replaced is replaced
        p = "dist_24_"
        d = torch.tensor(gold[p + "depth"], device=gpu)
        rows = torch.tensor(gold[p + "fxfycxcy"], device=gpu)
        try:
            from einops import repeat
            broadcast = repeat(rows, "vc r -> vc r h w", h=24, w=24)
        except ImportError:
            broadcast = rows[:, :, None, None].expand(-1, -1, 24, 24)
        assert broadcast.stride() == (4, 1, 0, 0)
        before = _bits(d).clone()
        got = fn(d, broadcast)
        assert _equal(got, stitch.depth_to_distance(d, rows, "reference")) and torch.equal(_bits(d), before)
        ref = gold[p + "out"]
        m = np.isfinite(ref)
        np.testing.assert_allclose(got.cpu().numpy()[m], ref[m], rtol=4 * 2.0 ** -23, atol=0)
        # not the reference's broadcast, another dtype, another device, a non-square map: the replaced function
        assert (fn(d, broadcast.contiguous()) == -7).all()
        assert (fn(d.double(), broadcast.double()) == -7).all()
        assert (fn(d.cpu(), broadcast.cpu()) == -7).all()
        assert (fn(d[:, :20], broadcast[:, :, :20]) == -7).all()
    finally:
        plugin.uninstall()
    assert zmod.depth_to_distance_map_batch is replaced and user.depth_to_distance_map_batch is replaced
