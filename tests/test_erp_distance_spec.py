"""The z-depth -> distance map and the fused depth-faces -> ERP distance stitch, on CPU: the float64 restatement
(tests/erp_distance_reference.py) against the values recorded from the reference (tests/golden/erp_distance.npz, made by
tests/golden/make_golden_erp_distance.py), the C ABI's argument checks, the Python argument checks and the install(erp_distance=True)
seam on a stand-in module tree.  The GPU half is tests/test_gpu_erp_distance.py.

"ulp" is the float32 spacing at the float64 value.  The reference's float32 statement was measured within 1.35 - 1.71 ulp of the
restatement with u = the row index (8^2, 16^2, 256^2 maps, fx != fy, cx != cy): the bar is the next integer, 2.  With u = the column
index it is 5e5 - 5e6 ulp away, so the fixture tells the two conventions apart."""
import ctypes as C
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import numpy as np
import pytest
import torch

import erp_distance_reference as R
import stitch_reference as SR
from splatter360_amd import _lib, stitch
from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "erp_distance.npz"
NAMES = ("s360_depth_to_distance_forward", "s360_depth_to_distance_backward", "s360_cube2erp_distance_forward",
         "s360_cube2erp_distance_backward")
BADARG, UNSUPPORTED = -1, -4
pytestmark = pytest.mark.filterwarnings("ignore:invalid value encountered")     # inf - inf at the fixture's inf depth, masked out


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _closures(gold):
    for v, fw, eh, ew in gold["closure_shapes"]:
        for kind in ("hm3d", "pert"):
            yield int(v), int(fw), int(eh), int(ew), kind, f"closure_{fw}_{eh}_{ew}_{kind}_"


# ---------------------------------------------------------------------------- the restatement against the reference's values
def test_fixture_holds_the_cases(gold):
    assert GOLD.stat().st_size < 400 * 1024
    assert gold["dist_shapes"].tolist() == [[5, 8], [6, 24]] and gold["closure_shapes"].tolist() == [[2, 8, 16, 32], [3, 24, 48, 96]]
    for n, h in gold["dist_shapes"]:
        p = f"dist_{h}_"
        d, k4 = gold[p + "depth"], gold[p + "fxfycxcy"]
        assert d.shape == (n, h, h) and k4.shape == (n, 4) and d.dtype == k4.dtype == np.float32
        assert (d == 0).sum() == 1 and (d < 0).sum() == 1 and np.isinf(d).sum() == 1
        assert (k4[:, 0] != k4[:, 1]).all() and (k4[:, 2] != k4[:, 3]).all() and len(np.unique(k4, axis=0)) == n
        assert np.isnan(gold[p + "grad"][d == 0]).all()                  # torch's autograd of the reference at the zero depth
    for v, fw, eh, ew, kind, p in _closures(gold):
        assert gold[p + "depth"].shape == (v, 6, fw, fw) and gold[p + "dist"].shape == (v * 6, fw, fw) and gold[p + "erp"].shape == (v, eh, ew)
        if kind == "hm3d":
            assert (gold[p + "fxfycxcy"] == 0.5 * fw).all()
        else:
            d = gold[p + "depth"]
            assert (d == 0).sum() == 1 and (d < 0).sum() == 1 and np.isinf(d).sum() == 1


@pytest.mark.parametrize("h", [8, 24])
def test_reference_convention_is_the_references_within_2_ulp_and_pixel_is_not(gold, h):
    p = f"dist_{h}_"
    d, k4, ref = gold[p + "depth"], gold[p + "fxfycxcy"], gold[p + "out"].astype(np.float64)
    want = R.distance64(d, k4, "reference")
    fin = np.isfinite(ref)
    assert fin.sum() == d.size - 1 and np.isfinite(want[fin]).all()
    err = np.abs(ref - want)[fin] / R.ulp32(want[fin])
    print(f"h={h}: reference vs float64 (u = row) worst {err.max():.3f} ulp")
    assert err.max() <= 2.0
    assert want[d == 0] == 0 and (want[d < 0] > 0).all() and np.isinf(want[np.isinf(d)]).all()
    other = R.distance64(d, k4, "pixel")
    err_px = np.abs(ref - other)[fin] / R.ulp32(other[fin])
    print(f"h={h}: reference vs float64 (u = column) worst {err_px.max():.3g} ulp")
    assert err_px.max() > 2.0 and (err_px > 2.0).mean() > 0.5     # all but the diagonal (row == column) and the zero
    # a value rounded once is within half an ulp of the restatement: the bar the kernels are held to has room
    assert (np.abs(want.astype(np.float32).astype(np.float64) - want)[fin] <= 0.5 * R.ulp32(want[fin])).all()


@pytest.mark.parametrize("h", [8, 24])
def test_gradient_restatement_against_the_recorded_autograd(gold, h):
    p = f"dist_{h}_"
    d, k4, g, ref = gold[p + "depth"], gold[p + "fxfycxcy"], gold[p + "gout"], gold[p + "grad"].astype(np.float64)
    want = R.distance_grad64(g, d, k4, "reference")
    fin = np.isfinite(ref)
    # torch differentiates the float32 statement term by term (measured 2.3 - 2.9 ulp from float64; reported, the GPU test's
    # bar is pointwise |ref - f64| + 1 ulp); the restatement is the same function to float32 precision
    err = np.abs(ref - want)[fin] / R.ulp32(want[fin])
    print(f"h={h}: recorded autograd vs float64 worst {err.max():.3f} ulp")
    assert fin.sum() >= d.size - 2 and np.allclose(ref[fin], want[fin], rtol=1e-5, atol=0)
    assert want[d == 0] == 0 and np.isnan(ref[d == 0]).all()
    neg = d < 0
    assert (np.sign(want[neg]) == -np.sign(g[neg])).all()


def test_closure_distance_faces_are_dist_of_the_reordered_depths(gold):
    for v, fw, eh, ew, kind, p in _closures(gold):
        depth, k4 = gold[p + "depth"], gold[p + "fxfycxcy"]
        k_want = stitch.fxfycxcy_from_intrinsics(torch.from_numpy(gold[p + "intrinsics"]), fw, fw).numpy()
        assert k_want.dtype == np.float32 and np.array_equal(k_want.reshape(v * 6, 4), k4)
        slots = R.reorder(depth)
        # the reorder is change_order_batch's: slot order (3, 4, 1, 2, 0, 5) of the rendered faces, 0 and 5 flipped on both axes
        assert np.array_equal(slots[:, 4], depth[:, 0, ::-1, ::-1]) and np.array_equal(slots[:, 0], depth[:, 3])
        assert np.array_equal(R.unreorder(slots), depth)
        want = R.slot_distance64(depth, k4.reshape(v, 6, 4), "reference").reshape(v * 6, fw, fw)
        ref = gold[p + "dist"].astype(np.float64)
        fin = np.isfinite(ref)
        assert (~fin).sum() == (kind == "pert") and np.array_equal(fin, np.isfinite(want))
        assert (np.abs(ref - want)[fin] <= 2.0 * R.ulp32(want[fin])).all()
        if kind == "pert":     # the face-space rule is another function of the same inputs
            px = R.slot_distance64(depth, k4.reshape(v, 6, 4), "pixel").reshape(v * 6, fw, fw)
            assert (np.abs(ref - px)[fin] > 2.0 * R.ulp32(px[fin])).mean() > 0.5


def test_closure_erp_is_the_stitch_of_the_distance_faces(gold):
    for v, fw, eh, ew, kind, p in _closures(gold):
        grid = stitch.sample_grid_numpy(fw, eh, ew)
        tp = SR.taps(grid, fw)
        want = R.stitch_distance64(gold[p + "depth"], gold[p + "fxfycxcy"].reshape(v, 6, 4), grid, "reference", tp=tp)
        ref = gold[p + "erp"].astype(np.float64)
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(want))
        dmax = np.abs(gold[p + "dist"][np.isfinite(gold[p + "dist"])]).max()
        assert np.abs(ref - want)[fin].max() <= 2e-6 * dmax + 2.0 * R.ulp32(dmax)


def test_restated_adjoint_is_the_transpose_times_the_scale(gold):
    v, fw, eh, ew, kind, p = next(c for c in _closures(gold) if c[4] == "pert")
    rng = np.random.default_rng(5)
    depth = np.where(np.isfinite(gold[p + "depth"]), gold[p + "depth"], 1.0).astype(np.float32)
    k4 = gold[p + "fxfycxcy"].reshape(v, 6, 4)
    grid = stitch.sample_grid_numpy(fw, eh, ew)
    tp = SR.taps(grid, fw)
    g = rng.standard_normal((v, eh, ew))
    for conv in R.CONVENTIONS:
        grad = R.stitch_distance_grad64(g, depth, k4, grid, conv, tp=tp)
        assert (grad[depth == 0] == 0).all()
        # a directional derivative away from the zero: distance is linear in |d| there
        step = np.where(depth == 0, 0.0, rng.standard_normal(depth.shape) * 1e-3 * np.abs(depth))
        lhs = ((R.stitch_distance64(depth.astype(np.float64) + step, k4, grid, conv, tp=tp)
                - R.stitch_distance64(depth, k4, grid, conv, tp=tp)) * g).sum()
        rhs = (grad * step).sum()
        assert abs(lhs - rhs) <= 1e-9 * (np.abs(grad * step).sum() + 1.0)


# ---------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_additive():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    lib = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and re.search(rf"\bint\s+{name}\s*\(", header) and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25 and "#define S360_ABI_VERSION 25" in header
    assert "#define S360_D2D_REFERENCE 0" in header and "#define S360_D2D_PIXEL 1" in header
    assert stitch.DISTANCE_CONVENTIONS == {"reference": 0, "pixel": 1}


def test_bad_arguments_return_their_code_before_any_gpu_work():
    lib = _lib.lib()
    p = C.c_void_p(64)          # never dereferenced: every call below returns before any GPU work
    ok_map = (C.c_int32 * 6)(*stitch.CHANGE_ORDER_FACE_MAP)
    bad_map = (C.c_int32 * 6)(3, 4, 1, 2, 6, 5)
    strides = (C.c_int64 * 3)(6 * 64, 64, 8)

    fwd, bwd = lib.s360_depth_to_distance_forward, lib.s360_depth_to_distance_backward
    for nulls in ((None, p, p), (p, None, p), (p, p, None)):
        assert fwd(*nulls, 2, 8, 8, 0, None) == BADARG
    for nulls in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert bwd(*nulls, 2, 8, 8, 0, None) == BADARG
    for n, h, w, conv in ((0, 8, 8, 0), (2, 0, 8, 1), (2, 8, 0, 1), (-1, 8, 8, 0), (2, 8, 8, 2), (2, 8, 8, -1), (2, 8, 9, 0), (2, 9, 8, 0)):
        assert fwd(p, p, p, n, h, w, conv, None) == BADARG, (n, h, w, conv)
        assert bwd(p, p, p, p, n, h, w, conv, None) == BADARG, (n, h, w, conv)

    sf, sb = lib.s360_cube2erp_distance_forward, lib.s360_cube2erp_distance_backward
    for i in range(4):
        a = [p] * 4
        a[i] = None
        assert sf(*a, 2, 8, 16, 32, 0, ok_map, None, None) == BADARG
    for i in range(7):
        a = [p] * 7
        a[i] = None
        assert sb(*a, 2, 8, 16, 32, 0, ok_map, None, None) == BADARG
    sizes = ((0, 8, 16, 32, 0), (2, 0, 16, 32, 0), (2, 8, 0, 32, 1), (2, 8, 16, 0, 1), (2, 8, 16, 32, 2), (2, 8, 16, 32, -1),
             (65536, 8, 16, 32, 0),                    # panoramas go in gridDim.y
             (3, 8, 8192, 16384, 0),                   # n eh ew 8 beyond int32 (one panorama of that size fits)
             (1, 18919, 16, 32, 1))                    # 6 fw fw + 1 beyond int32
    for n, fw, eh, ew, conv in sizes:
        assert sf(p, p, p, p, n, fw, eh, ew, conv, ok_map, None, None) == BADARG, (n, fw, eh, ew, conv)
        assert sb(p, p, p, p, p, p, p, n, fw, eh, ew, conv, ok_map, None, None) == BADARG, (n, fw, eh, ew, conv)
    assert sf(p, p, p, p, 2, 8, 16, 32, 0, bad_map, None, None) == BADARG
    assert sb(p, p, p, p, p, p, p, 2, 8, 16, 32, 0, bad_map, None, None) == BADARG
    # strided faces: the adjoint writes dense tensors only, as the colour stitch's does
    assert sb(p, p, p, p, p, p, p, 2, 8, 16, 32, 0, ok_map, strides, None) == UNSUPPORTED
    assert sb(p, p, p, p, p, p, p, 2, 8, 16, 32, 1, None, strides, None) == UNSUPPORTED


# ---------------------------------------------------------------------------- the Python argument checks (no GPU here)
def test_python_api_refuses_cpu_tensors_and_bad_arguments():
    d, k = torch.ones(2, 8, 8), torch.ones(2, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        stitch.depth_to_distance(d, k)
    with pytest.raises(ValueError, match="convention"):
        stitch.depth_to_distance(d, k, convention="opencv")
    mod = stitch.Cube2Equirec(8, 16, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        mod.stitch_distance_rendered(torch.ones(2, 6, 8, 8), torch.ones(2, 6, 4))
    with pytest.raises(ValueError, match="convention"):
        mod.stitch_distance_rendered(torch.ones(2, 6, 8, 8), torch.ones(2, 6, 4), convention="slot")
    with pytest.raises(ValueError):
        stitch.fxfycxcy_from_intrinsics(torch.ones(2, 4), 8, 8)
    k3 = torch.tensor([[0.5, 0.0, 0.25], [0.0, 0.75, 0.125], [0.0, 0.0, 1.0]]).expand(2, 6, 3, 3)
    got = stitch.fxfycxcy_from_intrinsics(k3, 16, 32)
    assert got.shape == (2, 6, 4) and got.dtype == torch.float32 and got[1, 5].tolist() == [16.0, 12.0, 8.0, 2.0]


# ---------------------------------------------------------------------------- the seam, on a stand-in module tree
DEFINER, USER, NAME = "src.geometry.z_depth_to_distance", "src.model.model_wrapper_erp", "depth_to_distance_map_batch"


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_erp_distance_seam")
    _write_standin(root)
    geo = root / "src" / "geometry"
    geo.mkdir(parents=True, exist_ok=True)
    (geo / "__init__.py").touch()
    (geo / "z_depth_to_distance.py").write_text(textwrap.dedent("""
        import torch

        def depth_to_distance_map_batch(depth_maps, fxfycxcy):
            return torch.full_like(depth_maps, -7.0)
    """))
    (root / "src" / "model" / "model_wrapper_erp.py").write_text("from ..geometry.z_depth_to_distance import depth_to_distance_map_batch\n")
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    import torch
    DEFINER, USER, NAME = {definer!r}, {user!r}, {name!r}

    def bound():
        return {{m: getattr(sys.modules[m], NAME) for m in (DEFINER, USER) if m in sys.modules}}

    def native(fns):
        return all(getattr(f, "replaced", None) is not None for f in fns.values())

    def original(fns):
        return all(getattr(f, "replaced", None) is None for f in fns.values())
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT), definer=DEFINER, user=USER, name=NAME)
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_after_import_rebinds_both_names_and_cpu_inputs_fall_through(standin):
    out = _run(standin, """
        importlib.import_module(USER)
        import src.geometry.z_depth_to_distance as Z
        fn0 = Z.depth_to_distance_map_batch
        import splatter360_amd
        splatter360_amd.install(erp_distance=True)
        b = bound()
        assert len(b) == 2 and native(b) and len(set(b.values())) == 1 and Z.depth_to_distance_map_batch.replaced is fn0, b
        d = torch.ones(3, 8, 8)
        rows = torch.ones(3, 4)
        broadcast = rows[:, :, None, None].expand(3, 4, 8, 8)            # the strides einops.repeat yields: (4, 1, 0, 0)
        assert broadcast.stride() == (4, 1, 0, 0)
        for k in (broadcast, broadcast.contiguous(), rows):              # CPU tensors, broadcast or not: the replaced function
            assert (Z.depth_to_distance_map_batch(d, k) == -7).all()
        assert (sys.modules[USER].depth_to_distance_map_batch(d.double(), broadcast.double()) == -7).all()
        splatter360_amd.install(erp_distance=True)                       # idempotent
        assert bound() == b and Z.depth_to_distance_map_batch.replaced is fn0
        splatter360_amd.uninstall()
        assert all(f is fn0 for f in bound().values())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import_and_uninstall_restores(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install()                                        # off by default
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        splatter360_amd.install(erp_distance=True)
        splatter360_amd.install(erp_distance=True)                       # idempotent: one hook
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 1 and DEFINER not in sys.modules
        importlib.import_module(USER)
        assert len(bound()) == 2 and native(bound()) and len(set(bound().values())) == 1
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        splatter360_amd.uninstall()
        assert original(bound()) and len(set(bound().values())) == 1
        splatter360_amd.install(erp_distance=True)
        splatter360_amd.uninstall()                                      # with nothing pending either
        assert original(bound())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_uninstall_drops_a_pending_hook(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(erp_distance=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 1
        splatter360_amd.uninstall()
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        importlib.import_module(USER)
        assert original(bound())
        print("ok")
    """)
    assert out.strip().endswith("ok")
