"""`splatter360_amd.install(depth_smoothness=True)`: LossDepth.forward rebound in the unchanged reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's, plus src/loss/loss_depth.py under the reference's name: a LossDepth
with the reference's constructor fields (cfg.weight, cfg.sigma_image, cfg.use_second_derivative) whose forward counts its calls
and returns -1.  Each case runs in a fresh interpreter.  The GPU half (the rebound method running the kernels) is in
tests/test_gpu_depth_smooth.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent

LOSS_DEPTH_SOURCE = textwrap.dedent("""
    import dataclasses
    import torch
    from torch import nn

    @dataclasses.dataclass
    class LossDepthCfg:
        weight: float
        sigma_image: object
        use_second_derivative: bool

    class LossDepth(nn.Module):
        calls = 0

        def __init__(self, cfg):
            super().__init__()
            self.cfg = cfg

        def forward(self, prediction, batch, gaussians, global_step):
            type(self).calls += 1
            batch["target"]["near"][..., None, None].log() + prediction.depth      # the reference's broadcast: raises on a mismatch
            return torch.tensor(-1.0)
""")


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_depth_smooth_seam")
    _write_standin(root)
    loss = root / "src" / "loss"
    loss.mkdir(parents=True, exist_ok=True)
    (loss / "__init__.py").touch()
    (loss / "loss_depth.py").write_text(LOSS_DEPTH_SOURCE)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, inspect, sys, types
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    import torch
    import splatter360_amd
    from splatter360_amd import plugin
    MOD = plugin.DEPTH_SMOOTH_MODULE

    def method():
        return sys.modules[MOD].LossDepth.__dict__["forward"]

    def hooks():
        return [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher) and f.seam is plugin.DEPTH_SMOOTH_SEAM]

    def call(loss, depth, near, far, image=None):
        return loss(types.SimpleNamespace(depth=depth), {{"target": {{"near": near, "far": far, "image": image}}}}, None, 0)
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_keyword_is_off_by_default():
    import inspect
    from splatter360_amd import plugin
    assert inspect.signature(plugin.install).parameters["depth_smoothness"].default is False
    seam = plugin.DEPTH_SMOOTH_SEAM
    assert (seam.keyword, seam.module, seam.cls_name, seam.names) == ("depth_smoothness", "src.loss.loss_depth", "LossDepth", ("forward",))


def test_install_rebinds_forward_falls_back_and_uninstall_restores(standin):
    out = _run(standin, """
        M = importlib.import_module(MOD)
        original = method()
        splatter360_amd.install(depth_smoothness=True)
        fn = method()
        assert fn is not original and fn.replaced is original
        loss = M.LossDepth(M.LossDepthCfg(1.0, None, False))
        bilateral = M.LossDepth(M.LossDepthCfg(1.0, 2.0, True))
        depth, near, image = torch.rand(2, 6, 5, 7), torch.rand(2, 1) + 0.5, torch.rand(2, 6, 3, 5, 7)
        # CPU tensors reach the replaced method
        assert call(loss, depth, near, near + 10).item() == -1.0 and M.LossDepth.calls == 1
        assert call(bilateral, depth, near, near + 10, image).item() == -1.0 and M.LossDepth.calls == 2
        # so do mismatched near shapes: the reference's own error is raised
        try:
            call(loss, depth, torch.rand(2, 4) + 0.5, torch.rand(2, 4) + 10)
            raise AssertionError("a [B,4] near against V = 6 must raise in the replaced method")
        except RuntimeError:
            pass
        assert M.LossDepth.calls == 3
        # and an image that requires grad
        assert call(bilateral, depth, near, near + 10, image.clone().requires_grad_(True)).item() == -1.0 and M.LossDepth.calls == 4
        # installing twice wraps only once
        splatter360_amd.install(depth_smoothness=True)
        assert method() is fn and plugin.install_depth_smoothness() is fn and fn.replaced is original
        splatter360_amd.uninstall()
        assert method() is original
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_which_calls_the_native_path_takes_and_leaves(standin):
    """The decision reads only the configuration and the tensors' device, dtype and shape, so CPU tensors that claim to be on
    the GPU show it here."""
    out = _run(standin, """
        class Fake(torch.Tensor):
            is_cuda = True
        def fake(*shape):
            return torch.rand(*shape).as_subclass(Fake)
        take = plugin._native_depth_smooth_call
        cfg = lambda sigma=None, second=False, weight=0.25: types.SimpleNamespace(weight=weight, sigma_image=sigma, use_second_derivative=second)
        pred = lambda d: types.SimpleNamespace(depth=d)
        batch = lambda near, far, image=None: {"target": {"near": near, "far": far, "image": image}}
        d, n1, n6, img = fake(2, 6, 5, 7), fake(2, 1), fake(2, 6), fake(2, 6, 3, 5, 7)
        args, kwargs = take(cfg(), pred(d), batch(n1, n1))
        assert args[0] is d and args[1] is n1 and args[3] is None and kwargs == dict(sigma_image=None, use_second_derivative=False, weight=0.25)
        args, kwargs = take(cfg(2.0, True), pred(d), batch(n6, n6, img))
        assert args[3] is img and kwargs == dict(sigma_image=2.0, use_second_derivative=True, weight=0.25)
        assert take(cfg(), pred(fake(1, 1, 2, 2)), batch(fake(1, 1), fake(1, 1))) is not None
        leaves = [
            (cfg(), pred(torch.rand(2, 6, 5, 7)), batch(n1, n1)),                       # CPU depth
            (cfg(), pred(d), batch(torch.rand(2, 1), n1)),                              # CPU near
            (cfg(), pred(d), batch(n1, torch.rand(2, 1))),                              # CPU far
            (cfg(), pred(d.double()), batch(n1, n1)),                                   # another dtype
            (cfg(), pred(d[0]), batch(n1, n1)),                                         # another rank
            (cfg(), pred(d), batch(fake(2, 3), fake(2, 3))),                            # Vn = 3 divides V but does not broadcast
            (cfg(), pred(d), batch(fake(2, 4), fake(2, 4))),                            # mismatched near
            (cfg(), pred(d), batch(n1, n6)),                                            # near and far differ
            (cfg(), pred(d), batch(fake(1, 1), fake(1, 1))),                            # another batch size
            (cfg(second=True), pred(fake(1, 1, 2, 2)), batch(fake(1, 1), fake(1, 1))),  # too small for the mode
            (cfg(), pred(fake(1, 1, 1, 5)), batch(fake(1, 1), fake(1, 1))),
            (cfg(2.0), pred(d), batch(n1, n1)),                                         # sigma without an image
            (cfg(2.0), pred(d), batch(n1, n1, torch.rand(2, 6, 3, 5, 7))),              # CPU image
            (cfg(2.0), pred(d), batch(n1, n1, fake(2, 6, 3, 5, 8))),                    # mismatched image
            (cfg(2.0), pred(d), batch(n1, n1, fake(2, 6, 5, 7))),                       # an image without channels
            (cfg(2.0), pred(d), batch(n1, n1, fake(2, 6, 3, 5, 7).requires_grad_(True))),   # an image that takes a gradient
            (cfg(), pred(None), batch(n1, n1)),
            (cfg(), pred(d), {}),
        ]
        for i, (c, p, b) in enumerate(leaves):
            assert take(c, p, b) is None, i
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import_and_uninstall_drops_the_hook(standin):
    out = _run(standin, """
        splatter360_amd.install(lazy=True, depth_smoothness=True)
        assert MOD not in sys.modules and [s.keyword for s in hooks()] == ["depth_smoothness"]
        M = importlib.import_module(MOD)
        assert method().replaced is not None and not hooks()
        splatter360_amd.uninstall()
        assert getattr(method(), "replaced", None) is None
        splatter360_amd.install(lazy=True)                        # the default leaves the method alone
        assert getattr(method(), "replaced", None) is None and not hooks()
        print("ok")
    """)
    assert out.strip().endswith("ok")
    out = _run(standin, """
        splatter360_amd.install(lazy=True, depth_smoothness=True)
        assert hooks()
        splatter360_amd.uninstall()
        assert not hooks()
        importlib.import_module(MOD)
        assert getattr(method(), "replaced", None) is None
        print("ok")
    """)
    assert out.strip().endswith("ok")
