"""The spherical cost volume's CPU-checkable parts: the restatement of tests/cost_volume_reference.py against values recorded from
the reference (tests/golden/cost_volume.npz, written by tests/golden/make_golden_cost_volume.py), the candidates and poses of
splatter360_amd/cost_volume.py bit for bit, the C ABI's new symbols and the install(cost_volume=True) seam on a fake module."""
import ctypes as C
import sys
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import cost_volume_reference as R
from splatter360_amd import _lib, cost_volume as cv, plugin

GOLDEN = Path(__file__).resolve().parent / "golden" / "cost_volume.npz"
SAMPLINGS = ("inverse_depth", "log_depth", "linear_depth")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize("key", ["v2", "v3"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_candidates_and_poses_are_the_references_bits(golden, key, sampling):
    near, far, ext = golden[f"{key}/near"], golden[f"{key}/far"], golden[f"{key}/extrinsics"]
    cand = golden[f"{key}/{sampling}/candidates"]
    got = cv.depth_candidates(near, far, cand.shape[1], sampling)
    assert got.shape == cand.shape and torch.equal(got, cand)
    poses = cv.relative_poses(ext)
    assert poses.shape == golden[f"{key}/{sampling}/poses"].shape and torch.equal(poses, golden[f"{key}/{sampling}/poses"])
    with pytest.raises(NotImplementedError):
        cv.depth_candidates(near, far, 4, "sqrt_depth")


@pytest.mark.parametrize("key", ["v2", "v3"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_restatement_reproduces_the_recorded_volume_and_gradient(golden, key, sampling):
    """Float32 on the CPU.  Where the fixture was recorded the restatement gives the recorded bits (difference 0 for the volume,
    the gradient and the warped tensor), since it performs the reference's operations in the reference's order; another CPU's
    float32 trigonometry may round differently, and what such a difference can do is bounded by the float32 chain's own distance
    from float64 (observed 9.4e-5 on the volume, values up to 3.6): the bar is twice that, 2e-4, and 1e-3 of the largest entry
    for the gradient."""
    f, g = golden[f"{key}/features"], golden[f"{key}/grad_out"]
    poses, cand = golden[f"{key}/{sampling}/poses"], golden[f"{key}/{sampling}/candidates"]
    vol = R.cost_volume(f, poses, cand, torch.float32)
    assert (vol - golden[f"{key}/{sampling}/volume"]).abs().max().item() <= 2e-4
    grad = R.feature_gradient(f, poses, cand, g, torch.float32)
    want = golden[f"{key}/{sampling}/grad_features"]
    assert (grad - want).abs().max().item() <= 1e-3 * want.abs().max().item()
    vol64 = R.cost_volume(f, poses, cand, torch.float64)
    assert (vol64 - golden[f"{key}/{sampling}/volume"].double()).abs().max().item() <= 1e-3


@pytest.mark.parametrize("key", ["v2", "v3"])
def test_restatement_reproduces_the_recorded_warped_tensor(golden, key):
    f = golden[f"{key}/features"]
    b, v = f.shape[:2]
    f10 = f[:, R.partner_order(v, 1)].transpose(0, 1).reshape(v * b, *f.shape[2:])
    got = R.warped_features(f10, golden[f"{key}/inverse_depth/poses"][0], golden[f"{key}/inverse_depth/candidates"], torch.float32)[0]
    assert (got - golden[f"{key}/warped0"]).abs().max().item() <= 2e-4


def test_partner_slots_follow_the_rolled_view_order():
    b, v = 2, 3
    slots = cv.partner_slots(b, v, "cpu")
    assert slots.dtype == torch.int32 and slots.shape == (v - 1, v * b)
    ids = torch.arange(b * v).view(b, v)                                 # ids[i, k] names (batch i, view k)
    own = ids.transpose(0, 1).reshape(-1)                                # "b v -> (v b)"
    for idx in range(1, v):
        partner = ids[:, R.partner_order(v, idx)].transpose(0, 1).reshape(-1)
        assert torch.equal(own[slots[idx - 1].long()], partner)


def test_abi_has_the_cost_volume_entry_points_and_they_reject_bad_arguments():
    lib = _lib.lib()
    for name in ("s360_cost_volume_forward", "s360_cost_volume_backward", "s360_cost_volume_warp"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 25 and "s360_cost_volume.hip" in _lib.SOURCES
    n = C.c_size_t(0)
    dims = (2, 2, 1, 128, 128, 256, 128)
    # the workspace query: a null workspace with a size pointer; channels-last copies only, nothing with C * D elements
    assert lib.s360_cost_volume_forward(None, None, None, None, None, *dims, 0, 1.0, None, None, C.byref(n), None) == 0
    assert n.value == 2 * 2 * 128 * 128 * 256 * 4
    assert lib.s360_cost_volume_backward(None, None, None, None, None, *dims, 0, 1.0, None, None, None, None, C.byref(n), None) == 0
    assert n.value == 4 * 2 * 128 * 128 * 256 * 4
    # bad arguments come back as -1 before any GPU work: another convention, a zero size, no size pointer, null data pointers
    assert lib.s360_cost_volume_forward(None, None, None, None, None, *dims, 1, 1.0, None, None, C.byref(n), None) == -1
    assert lib.s360_cost_volume_forward(None, None, None, None, None, 2, 2, 0, 128, 128, 256, 128, 0, 1.0, None, None, C.byref(n), None) == -1
    assert lib.s360_cost_volume_forward(None, None, None, None, None, *dims, 0, 1.0, None, None, None, None) == -1
    assert lib.s360_cost_volume_forward(None, None, None, None, None, *dims, 0, 1.0, None, C.c_void_p(16), C.byref(n), None) == -1
    assert lib.s360_cost_volume_backward(None, None, None, None, None, *dims, 0, 1.0, None, None, None, C.c_void_p(16), C.byref(n), None) == -1
    assert lib.s360_cost_volume_warp(None, None, None, None, 2, 2, 128, 128, 256, 128, 0, None, None) == -1
    assert lib.s360_cost_volume_warp(None, None, None, None, 2, 2, 128, 128, 70000, 128, 0, None, None) == -1


def test_python_layer_refuses_what_it_cannot_run():
    f, e, near, far = R.random_inputs(1, 2, 4, 8, 16, seed=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        cv.spherical_cost_volume(f, e, near, far, 4)
    with pytest.raises(ValueError, match="dataset_name"):
        cv.spherical_cost_volume(f, e, near, far, 4, dataset_name="m3d")
    with pytest.raises(ValueError):
        cv.relative_poses(e[:, :1])


def _fake_module():
    calls = []

    def warp_with_pose_depth_candidates(utils360, feature1, pose, depth, clamp_min_depth=1e-3, warp_padding_mode="zeros", debug=False, **kw):
        calls.append((tuple(feature1.shape), warp_padding_mode))
        return R.warped_features(feature1, pose, depth[:, :, 0, 0], feature1.dtype)

    mod = types.ModuleType(plugin.COST_VOLUME_MODULE)
    mod.warp_with_pose_depth_candidates = warp_with_pose_depth_candidates
    return mod, warp_with_pose_depth_candidates, calls


def test_install_cost_volume_rebinds_keeps_replaced_and_falls_back(golden):
    import inspect
    assert inspect.signature(plugin.install).parameters["cost_volume"].default is False
    mod, original, calls = _fake_module()
    sys.modules[plugin.COST_VOLUME_MODULE] = mod
    try:
        fn = plugin.install_cost_volume()
        assert fn is mod.warp_with_pose_depth_candidates and fn is not original and fn.replaced is original
        assert plugin.install_cost_volume() is fn and fn.replaced is original          # idempotent
        # CPU tensors: the replaced function runs, with the caller's arguments, and its tensor comes back
        f = golden["v2/features"]
        poses, cand = golden["v2/inverse_depth/poses"], golden["v2/inverse_depth/candidates"]
        b, v, c, h, w = f.shape
        f01 = f.transpose(0, 1).reshape(v * b, c, h, w)
        f10 = f[:, [1, 0]].transpose(0, 1).reshape(v * b, c, h, w)
        utils = types.SimpleNamespace(dataset="hm3d")
        warped = mod.warp_with_pose_depth_candidates(utils, f10, poses[0], cand[:, :, None, None].repeat(1, 1, h, w), warp_padding_mode="zeros")
        assert isinstance(warped, torch.Tensor) and calls == [((v * b, c, h, w), "zeros")]
        vol = (f01.unsqueeze(2) * warped).sum(1) / c ** 0.5
        assert (vol - golden["v2/inverse_depth/volume"]).abs().max().item() <= 2e-4
        # a lazy handle that cannot fuse (CPU tensors) materialises through the replaced function, for the product and for any other use
        handle = cv.LazyWarp(utils, f10, poses[0], cand[:, :, None, None].repeat(1, 1, h, w), original, {})
        assert handle.shape == warped.shape
        assert torch.equal((f01.unsqueeze(2) * handle).sum(1), (f01.unsqueeze(2) * warped).sum(1))
        assert torch.equal(torch.stack([handle])[0], warped) and torch.equal(handle.mean(dim=1), warped.mean(dim=1))
        assert len(calls) == 2                                                          # materialised once
    finally:
        plugin.uninstall()
        assert mod.warp_with_pose_depth_candidates is original
        del sys.modules[plugin.COST_VOLUME_MODULE]


def test_install_cost_volume_before_the_module_is_imported_uses_the_import_hook():
    assert plugin.COST_VOLUME_MODULE not in sys.modules
    try:
        assert plugin.install_cost_volume() is None
        assert any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.COST_VOLUME_SEAM for f in sys.meta_path)
    finally:
        plugin.uninstall()
    assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
