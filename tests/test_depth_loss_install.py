"""`splatter360_amd.install(depth_loss=True)`: the training step's compute_l1_sphere_loss and erode rebound in the unchanged
reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's, plus the reference's layout of the two names:
src/model/model_wrapper_helper.py defines erode (:4-24) and compute_l1_sphere_loss (:63-90), and src/model/model_wrapper_erp.py
binds both with `from .model_wrapper_helper import compute_l1_sphere_loss, erode` (:45).  The stand-in functions return -1 /
-2, so a call shows which function ran.  The GPU half (the patched functions running the kernels) is in
tests/test_gpu_depth_loss.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent


def _write_helper(root: Path) -> None:
    model = root / "src" / "model"
    model.mkdir(parents=True, exist_ok=True)
    (model / "model_wrapper_helper.py").write_text(textwrap.dedent("""
        import torch

        def erode(bin_img, ksize=5):
            return torch.full_like(bin_img, -2.0)

        def compute_l1_sphere_loss(y_pred, y_true, mask=None, keep_batch=False):
            if mask is None:
                raise NotImplementedError
            return torch.full((y_pred.shape[0],) if keep_batch else (), -1.0, dtype=y_pred.dtype)
    """))
    (model / "model_wrapper_erp.py").write_text("from .model_wrapper_helper import compute_l1_sphere_loss, erode\n")


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_depth_loss_seam")
    _write_standin(root)
    _write_helper(root)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    import torch
    MODS = ("src.model.model_wrapper_helper", "src.model.model_wrapper_erp")
    NAMES = ("compute_l1_sphere_loss", "erode")

    def bound():
        return {{(m, n): getattr(sys.modules[m], n) for m in MODS if m in sys.modules for n in NAMES}}

    def all_native(fns):
        return all(getattr(f, "replaced", None) is not None for f in fns.values())

    def none_native(fns):
        return not any(getattr(f, "replaced", None) is not None for f in fns.values())

    def hooks():
        from splatter360_amd import plugin
        return [f for f in sys.meta_path if isinstance(f, plugin._SeamPatcher) and f.seam is plugin.DEPTH_LOSS_SEAM]
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_after_import_rebinds_both_names_and_falls_back_on_cpu(standin):
    out = _run(standin, """
        import src.model.model_wrapper_erp as E, src.model.model_wrapper_helper as Hm
        originals = {n: getattr(Hm, n) for n in NAMES}
        import splatter360_amd
        splatter360_amd.install(depth_loss=True)
        fns = bound()
        assert len(fns) == 4 and all_native(fns), fns
        for n in NAMES:
            assert getattr(E, n) is getattr(Hm, n) and getattr(Hm, n).replaced is originals[n]
        # CPU tensors (and every other unsupported call) go to the replaced functions
        x = torch.ones(2, 1, 8, 8)
        assert (E.erode(x) == -2.0).all()
        assert E.compute_l1_sphere_loss(x, x, mask=x).item() == -1.0
        assert E.compute_l1_sphere_loss(x, x, x, True).tolist() == [-1.0, -1.0]
        try:
            E.compute_l1_sphere_loss(x, x)
            raise AssertionError("mask=None must raise")
        except NotImplementedError:
            pass
        splatter360_amd.install(depth_loss=True)                 # idempotent
        assert bound() == fns
        splatter360_amd.uninstall()
        assert all(f is originals[n] for (m, n), f in bound().items()), bound()
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import(standin):
    out = _run(standin, """
        import splatter360_amd
        splatter360_amd.install(depth_loss=True)
        assert "src.model.model_wrapper_helper" not in sys.modules and len(hooks()) == 1
        import src.model.model_wrapper_erp
        fns = bound()
        assert len(fns) == 4 and all_native(fns), fns
        assert not hooks()                                       # the hook is gone once it has patched
        splatter360_amd.uninstall()
        assert len(bound()) == 4 and none_native(bound())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (the reference's src/main.py:22-36) sits at sys.meta_path[0] and resolves `src.*` with
    PathFinder itself: the hook never sees the helper module.  The next import it is asked about patches it late."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        import splatter360_amd
        splatter360_amd.install(depth_loss=True)
        class Competing(importlib.abc.MetaPathFinder):
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        import src.model.model_wrapper_erp
        fns = bound()
        assert len(fns) == 4 and none_native(fns)                # imported behind the hook's back
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hook is asked about
        fns = bound()
        assert len(fns) == 4 and all_native(fns), fns
        assert not hooks()
        splatter360_amd.uninstall()
        assert none_native(bound())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_with_only_the_helper_imported_then_the_user(standin):
    out = _run(standin, """
        import src.model.model_wrapper_helper
        import splatter360_amd
        splatter360_amd.install(depth_loss=True)
        import src.model.model_wrapper_erp                       # binds the replacements itself
        fns = bound()
        assert len(fns) == 4 and all_native(fns), fns
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_uninstall_drops_a_pending_hook(standin):
    out = _run(standin, """
        import splatter360_amd
        splatter360_amd.install(depth_loss=True)
        assert hooks()
        splatter360_amd.uninstall()
        assert not hooks()
        import src.model.model_wrapper_erp
        assert len(bound()) == 4 and none_native(bound())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_default_install_leaves_both_names_alone(standin):
    out = _run(standin, """
        import src.model.model_wrapper_erp
        before = bound()
        import splatter360_amd
        splatter360_amd.install()
        from src.model.decoder import DECODERS
        assert DECODERS["splatting_cuda"].__name__ == "DecoderSplattingFusedMI355X"
        assert bound() == before and none_native(before) and not hooks()
        splatter360_amd.install(metrics=True)                    # the metrics seam does not touch them either
        assert bound() == before
        print("ok")
    """)
    assert out.strip().endswith("ok")
