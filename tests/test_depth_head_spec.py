"""The softmax depth head's CPU-checkable parts: the statement of tests/depth_head_reference.py against central differences and
against the closed form the backward kernel evaluates, the C ABI's two new symbols, and the install(depth_head=True) seam on a
stand-in module.  The GPU half is tests/test_gpu_depth_head.py."""
import ctypes as C
import inspect
import re
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest
import torch

import depth_head_reference as R
from splatter360_amd import _lib, depth_head as dh, plugin
from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("s360_depth_head_forward", "s360_depth_head_backward")


def test_reference_gradient_agrees_with_central_differences_and_the_closed_form():
    """Pins the reference itself: float64 autograd of the statement against central differences at one tiny shape (the
    tolerance of tests/test_gpu_cost_volume.py's test of the same kind), and against
    g_z[d] = p_d (g_depth (c_d - depth) - g_pmax pmax) + [d == a] g_pmax pmax, the formula of the backward kernel."""
    logits, cand, g_depth, g_pmax = R.random_case((2, 5, 2, 3), 1.0, "inverse_depth", seed=3)
    grad = R.logits_gradient(logits, cand, g_depth, g_pmax)
    z64, eps = logits.double(), 1e-6

    def loss(z):
        depth, pmax = R.head(z, cand)
        return (depth * g_depth.double()).sum() + (pmax * g_pmax.double()).sum()

    for idx in [(0, 0, 0, 0), (1, 4, 1, 2), (0, 2, 1, 1), (1, 1, 0, 2), (0, 3, 0, 1)]:
        hi, lo = z64.clone(), z64.clone()
        hi[idx] += eps
        lo[idx] -= eps
        num = (loss(hi) - loss(lo)) / (2 * eps)
        assert abs(num.item() - grad[idx].item()) <= 1e-7 * max(1.0, abs(num.item()))
    for gd, gp in ((g_depth, g_pmax), (g_depth, None), (None, g_pmax)):
        want = R.logits_gradient(logits, cand, gd, gp)
        assert (R.formula_gradient(logits, cand, gd, gp) - want).abs().max().item() <= 1e-14 * max(1.0, want.abs().max().item())


def test_abi_has_the_depth_head_entry_points_and_they_reject_bad_arguments():
    lib = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "s360.h").read_text(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and re.search(rf"\bint\s+{name}\s*\(", header)
    assert "s360_depth_head.hip" in _lib.SOURCES and (ROOT / "splatter360_amd" / "csrc" / "s360_depth_head.hip").exists()
    assert _lib.ABI_VERSION == 25 and lib.s360_abi_version() == 25                  # additive: the version stays
    p = C.c_void_p(16)                                                              # never dereferenced: every call below is refused
    # null required pointers and non-positive sizes come back as -1 before any GPU work
    assert lib.s360_depth_head_forward(None, None, 2, 128, 128, 256, None, None, None, None, None) == -1
    assert lib.s360_depth_head_forward(None, p, 2, 128, 128, 256, p, p, p, p, None) == -1
    assert lib.s360_depth_head_forward(p, p, 2, 128, 128, 256, p, p, p, None, None) == -1
    for dims in ((0, 128, 128, 256), (2, 0, 128, 256), (2, 128, -1, 256), (2, 128, 128, 0)):
        assert lib.s360_depth_head_forward(p, p, *dims, p, p, p, p, None) == -1
    assert lib.s360_depth_head_backward(None, None, None, None, None, None, None, 2, 128, 128, 256, None, None) == -1
    assert lib.s360_depth_head_backward(p, p, p, p, p, None, None, 2, 128, 128, 256, None, None) == -1
    assert lib.s360_depth_head_backward(p, p, None, p, p, p, p, 2, 128, 128, 256, p, None) == -1
    assert lib.s360_depth_head_backward(p, p, p, p, p, p, p, 2, 128, 0, 256, p, None) == -1


def test_python_layer_refuses_what_it_cannot_run():
    logits, cand, _, _ = R.random_case((2, 4, 3, 5), 1.0, "log_depth", seed=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        dh.softmax_depth_head(logits, cand)
    with pytest.raises(ValueError):
        dh.softmax_depth_head(logits[0], cand)
    with pytest.raises(RuntimeError, match="GPU only"):
        dh.coarse_depth_head(logits, cand, 4)


@pytest.fixture
def standin():
    assert plugin.COST_VOLUME_MODULE not in sys.modules
    mod = R.standin_module(plugin.COST_VOLUME_MODULE)
    sys.modules[plugin.COST_VOLUME_MODULE] = mod
    try:
        yield mod
    finally:
        plugin.uninstall()
        del sys.modules[plugin.COST_VOLUME_MODULE]


def test_install_depth_head_rebinds_f_keeps_replaced_and_falls_back_on_cpu(standin):
    mod = standin
    assert inspect.signature(plugin.install).parameters["depth_head"].default is False
    logits, cand, _, _ = R.random_case((2, 6, 4, 5), 1.0, "inverse_depth", seed=2)
    c4 = cand[:, :, None, None]
    before = mod.depth_head(logits, c4)
    assert plugin.install(lazy=True, depth_head=True) is None                      # lazy: no decoder registry is imported here
    proxy = mod.F
    assert isinstance(proxy, dh.FunctionalProxy) and proxy.replaced is torch.nn.functional
    assert proxy is not torch.nn.functional and plugin.install_depth_head() is proxy and mod.F is proxy          # idempotent
    plugin.install(lazy=True, depth_head=True)
    assert mod.F is proxy and proxy.replaced is torch.nn.functional
    # every other attribute is torch.nn.functional's own
    assert mod.F.interpolate is torch.nn.functional.interpolate and mod.F.grid_sample is torch.nn.functional.grid_sample
    assert torch.equal(mod.upsample(logits, 2), torch.nn.functional.interpolate(logits, scale_factor=2))
    # CPU tensors: the replaced softmax runs and the three statements give the bits they gave before
    after = mod.depth_head(logits, c4)
    assert all(isinstance(t, torch.Tensor) for t in after) and all(torch.equal(x, y) for x, y in zip(before, after))
    assert isinstance(mod.F.softmax(logits, dim=1), torch.Tensor)
    # so does everything the native head does not take: another dim, another dtype, another rank, extra arguments
    for args, kwargs in (((logits,), {"dim": 2}), ((logits.half(),), {"dim": 1}), ((logits[0],), {"dim": 1}),
                         ((logits, 1), {"dtype": torch.float64})):
        assert torch.equal(mod.F.softmax(*args, **kwargs), torch.nn.functional.softmax(*args, **kwargs))
    # a lazy handle that cannot fuse (CPU tensors) goes dense through the replaced softmax, with autograd intact
    z = logits.clone().requires_grad_(True)
    handle = dh.LazyPdf(z, torch.nn.functional.softmax)
    assert handle.shape == z.shape
    depth = (c4 * handle).sum(dim=1, keepdim=True)
    pmax = torch.max(handle, dim=1, keepdim=True)[0]
    assert torch.equal(depth, before[0]) and torch.equal(pmax, before[1])
    assert torch.equal(handle[:, 0], torch.softmax(logits, 1)[:, 0]) and torch.equal(handle.sum(), torch.softmax(logits, 1).sum())
    (depth.sum() + pmax.sum()).backward()
    assert torch.isfinite(z.grad).all() and z.grad.abs().max().item() > 0
    plugin.uninstall()
    assert mod.F is torch.nn.functional


def test_install_depth_head_coexists_with_the_cost_volume_seam(standin):
    mod = standin

    def warp_with_pose_depth_candidates(utils360, feature1, pose, depth, **kw):
        return feature1

    mod.warp_with_pose_depth_candidates = warp_with_pose_depth_candidates
    plugin.install(lazy=True, cost_volume=True, depth_head=True)
    assert mod.warp_with_pose_depth_candidates.replaced is warp_with_pose_depth_candidates
    assert isinstance(mod.F, dh.FunctionalProxy) and mod.F.replaced is torch.nn.functional
    x = torch.ones(1, 2, 3, 4)
    assert mod.warp_with_pose_depth_candidates(None, x, None, None) is x           # CPU: the replaced warp
    plugin.uninstall()
    assert mod.warp_with_pose_depth_candidates is warp_with_pose_depth_candidates and mod.F is torch.nn.functional


def test_install_depth_head_before_the_module_is_imported_uses_the_import_hook():
    assert plugin.COST_VOLUME_MODULE not in sys.modules
    try:
        assert plugin.install_depth_head() is None and plugin.install_cost_volume() is None
        hooks = [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher)]
        assert plugin.DEPTH_HEAD_SEAM in hooks and plugin.COST_VOLUME_SEAM in hooks
    finally:
        plugin.uninstall()
    assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)


def test_import_hook_patches_the_module_on_first_import(tmp_path):
    """In a fresh interpreter, with the stand-in `src` package of tests/test_install_ref.py plus the predictor's module:
    install(depth_head=True) first, the import afterwards; the module then holds the proxy, and uninstall() puts
    torch.nn.functional back."""
    _write_standin(tmp_path)
    path = tmp_path.joinpath(*plugin.COST_VOLUME_MODULE.split(".")).with_suffix(".py")
    path.parent.mkdir(parents=True, exist_ok=True)
    for parent in path.parents:
        if parent == tmp_path:
            break
        (parent / "__init__.py").touch()
    path.write_text(R.STANDIN_SOURCE + "\n\ndef warp_with_pose_depth_candidates(utils360, feature1, pose, depth, **kw):\n    return feature1\n")
    body = textwrap.dedent(f"""
        import importlib, sys
        sys.path.insert(0, {str(tmp_path)!r})
        sys.path.insert(0, {str(ROOT)!r})
        import torch
        import splatter360_amd
        from splatter360_amd import plugin, depth_head
        splatter360_amd.install(depth_head=True, cost_volume=True)
        assert plugin.COST_VOLUME_MODULE not in sys.modules
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 2
        mod = importlib.import_module(plugin.COST_VOLUME_MODULE)
        assert isinstance(mod.F, depth_head.FunctionalProxy) and mod.F.replaced is torch.nn.functional
        assert mod.warp_with_pose_depth_candidates.replaced is not None
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        z, c = torch.randn(2, 5, 3, 4), torch.rand(2, 5, 1, 1) + 1
        depth, pmax = mod.depth_head(z, c)
        pdf = torch.softmax(z, 1)
        assert torch.equal(depth, (c * pdf).sum(1, keepdim=True)) and torch.equal(pmax, pdf.max(1, keepdim=True)[0])
        splatter360_amd.uninstall()
        assert mod.F is torch.nn.functional and getattr(mod.warp_with_pose_depth_candidates, "replaced", None) is None
        print("ok")
    """)
    r = subprocess.run([sys.executable, "-c", body], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
