"""`splatter360_amd.install(metrics=True)`: the evaluation step's compute_ssim rebound in the unchanged reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's (decoder registry and adapter from the committed interface capture),
plus the metrics layout of the reference: src/evaluation/metrics.py defines compute_ssim (:38-54), and three modules bind it
with `from ... import` — src/model/model_wrapper_erp.py:18, src/model/model_wrapper_cubemaps.py:19,
src/evaluation/metric_computer.py:12.  The stand-in compute_ssim returns -1 per image, so a call shows which function ran.
The GPU half (the patched function returning the kernel's score) is in tests/test_gpu_ssim.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent
USERS = ("src.model.model_wrapper_erp", "src.model.model_wrapper_cubemaps", "src.evaluation.metric_computer")


def _write_metrics(root: Path) -> None:
    ev = root / "src" / "evaluation"
    ev.mkdir(parents=True, exist_ok=True)
    (ev / "__init__.py").touch()
    (ev / "metrics.py").write_text(textwrap.dedent("""
        import torch

        def compute_psnr(ground_truth, predicted):
            return torch.zeros(ground_truth.shape[0])

        def compute_ssim(ground_truth, predicted):
            return torch.full((ground_truth.shape[0],), -1.0, dtype=predicted.dtype, device=predicted.device)
    """))
    (ev / "metric_computer.py").write_text("from .metrics import compute_psnr, compute_ssim\n")
    for name in ("model_wrapper_erp", "model_wrapper_cubemaps"):
        (root / "src" / "model" / f"{name}.py").write_text("from ..evaluation.metrics import compute_psnr, compute_ssim\n")


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_metrics_seam")
    _write_standin(root)
    _write_metrics(root)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    USERS = {users!r}
    import torch

    def bound():
        mods = ["src.evaluation.metrics", *USERS]
        return {{m: sys.modules[m].compute_ssim for m in mods if m in sys.modules}}

    def all_native(fns):
        return all(getattr(f, "replaced", None) is not None for f in fns.values())
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT), users=USERS)
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_after_import_rebinds_every_user(standin):
    out = _run(standin, """
        for m in USERS:
            importlib.import_module(m)
        import src.evaluation.metrics as M
        original = M.compute_ssim
        import splatter360_amd
        splatter360_amd.install(metrics=True)
        fns = bound()
        assert len(fns) == 4 and all_native(fns) and len(set(fns.values())) == 1, fns
        assert M.compute_ssim.replaced is original
        # CPU tensors go to the replaced function
        assert M.compute_ssim(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)).tolist() == [-1.0, -1.0]
        splatter360_amd.install(metrics=True)                   # idempotent
        assert bound() == fns and M.compute_ssim.replaced is original
        splatter360_amd.uninstall()
        assert all(f is original for f in bound().values()), bound()
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import(standin):
    out = _run(standin, """
        import splatter360_amd
        splatter360_amd.install(metrics=True)
        assert "src.evaluation.metrics" not in sys.modules
        import src.model.model_wrapper_erp
        fns = bound()
        assert len(fns) == 2 and all_native(fns), fns
        import src.model.model_wrapper_cubemaps, src.evaluation.metric_computer
        fns = bound()
        assert len(fns) == 4 and all_native(fns) and len(set(fns.values())) == 1, fns
        # the hook is gone once it has patched
        from splatter360_amd import plugin
        assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.SSIM_SEAM for f in sys.meta_path)
        splatter360_amd.uninstall()
        original = sys.modules["src.evaluation.metrics"].compute_ssim
        assert getattr(original, "replaced", None) is None and all(f is original for f in bound().values())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (the reference's src/main.py:22-36) sits at sys.meta_path[0] and resolves `src.*` with
    PathFinder itself: the hook never sees the metrics module.  The next import it is asked about patches it late."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        import splatter360_amd
        splatter360_amd.install(metrics=True)
        class Competing(importlib.abc.MetaPathFinder):
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        import src.model.model_wrapper_erp, src.evaluation.metric_computer
        fns = bound()
        assert len(fns) == 3 and not all_native(fns)            # imported behind the hook's back
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hook is asked about
        fns = bound()
        assert len(fns) == 3 and all_native(fns) and len(set(fns.values())) == 1, fns
        import src.model.model_wrapper_cubemaps
        assert all_native(bound()) and len(bound()) == 4
        splatter360_amd.uninstall()
        assert not all_native(bound()) and len(set(bound().values())) == 1
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_uninstall_drops_a_pending_hook(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(metrics=True)
        assert any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.SSIM_SEAM for f in sys.meta_path)
        splatter360_amd.uninstall()
        assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.SSIM_SEAM for f in sys.meta_path)
        import src.model.model_wrapper_erp
        assert not all_native(bound()) and len(bound()) == 2
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_default_install_leaves_compute_ssim_alone(standin):
    out = _run(standin, """
        import src.model.model_wrapper_erp, src.evaluation.metrics as M
        original = M.compute_ssim
        import splatter360_amd
        splatter360_amd.install()
        from src.model.decoder import DECODERS
        assert DECODERS["splatting_cuda"].__name__ == "DecoderSplattingFusedMI355X"
        assert all(f is original for f in bound().values())
        from splatter360_amd import plugin
        assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.SSIM_SEAM for f in sys.meta_path)
        import src.model.model_wrapper_cubemaps
        assert all(f is original for f in bound().values()) and len(bound()) == 3
        print("ok")
    """)
    assert out.strip().endswith("ok")
