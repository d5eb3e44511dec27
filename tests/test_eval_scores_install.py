"""`splatter360_amd.install(depth_metrics=True, psnr=True)`: the evaluation step's compute_depth_metrics_batched and compute_psnr
rebound in the unchanged reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's plus the layout of the reference: src/evaluation/metrics.py defines
compute_psnr (:11-21) and compute_ssim, bound with `from ... import` by src/model/model_wrapper_erp.py:18,
src/model/model_wrapper_cubemaps.py:19 and src/evaluation/metric_computer.py:12; src/scripts/compute_depth_metrics.py defines
compute_depth_metrics_batched (:47-116), bound by src/model/model_wrapper_erp.py:47.  The stand-in functions return -1 / -2 / -3,
so a call shows which function ran.  The GPU half (the patched functions returning the kernels' numbers) is in
tests/test_gpu_eval_scores.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent
PSNR_USERS = ("src.model.model_wrapper_erp", "src.model.model_wrapper_cubemaps", "src.evaluation.metric_computer")
DEPTH_USERS = ("src.model.model_wrapper_erp",)


def _write_scores(root: Path) -> None:
    ev = root / "src" / "evaluation"
    ev.mkdir(parents=True, exist_ok=True)
    (ev / "__init__.py").touch()
    (ev / "metrics.py").write_text(textwrap.dedent("""
        import torch

        def compute_psnr(ground_truth, predicted):
            return torch.full((ground_truth.shape[0],), -2.0)

        def compute_ssim(ground_truth, predicted):
            return torch.full((ground_truth.shape[0],), -1.0, dtype=predicted.dtype, device=predicted.device)
    """))
    (ev / "metric_computer.py").write_text("from .metrics import compute_psnr, compute_ssim\n")
    sc = root / "src" / "scripts"
    sc.mkdir(parents=True, exist_ok=True)
    (sc / "__init__.py").touch()
    (sc / "compute_depth_metrics.py").write_text(textwrap.dedent("""
        import torch

        def compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a=False):
            return {"abs_diff": torch.full((gt_bN.shape[0],), -3.0), "mult_a": mult_a}
    """))
    (root / "src" / "model" / "model_wrapper_cubemaps.py").write_text("from ..evaluation.metrics import compute_psnr, compute_ssim\n")
    (root / "src" / "model" / "model_wrapper_erp.py").write_text(
        "from ..evaluation.metrics import compute_psnr, compute_ssim\n"
        "from ..scripts.compute_depth_metrics import compute_depth_metrics_batched\n")


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_scores_seam")
    _write_standin(root)
    _write_scores(root)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    PSNR_USERS, DEPTH_USERS = {psnr_users!r}, {depth_users!r}
    ALL = sorted(set(PSNR_USERS + DEPTH_USERS))
    import torch

    def bound(name):
        definer = "src.evaluation.metrics" if name != "compute_depth_metrics_batched" else "src.scripts.compute_depth_metrics"
        users = PSNR_USERS if name != "compute_depth_metrics_batched" else DEPTH_USERS
        return {{m: getattr(sys.modules[m], name) for m in (definer, *users) if m in sys.modules}}

    def native(fns):
        return all(getattr(f, "replaced", None) is not None for f in fns.values())

    def original(fns):
        return all(getattr(f, "replaced", None) is None for f in fns.values())

    P, D, S = "compute_psnr", "compute_depth_metrics_batched", "compute_ssim"
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT), psnr_users=PSNR_USERS, depth_users=DEPTH_USERS)
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_after_import_rebinds_every_user(standin):
    out = _run(standin, """
        for m in ALL:
            importlib.import_module(m)
        import src.evaluation.metrics as M, src.scripts.compute_depth_metrics as DM
        psnr0, depth0, ssim0 = M.compute_psnr, DM.compute_depth_metrics_batched, M.compute_ssim
        import splatter360_amd
        splatter360_amd.install(depth_metrics=True, psnr=True)
        p, d = bound(P), bound(D)
        assert len(p) == 4 and native(p) and len(set(p.values())) == 1, p
        assert len(d) == 2 and native(d) and len(set(d.values())) == 1, d
        assert M.compute_psnr.replaced is psnr0 and DM.compute_depth_metrics_batched.replaced is depth0
        assert all(f is ssim0 for f in bound(S).values())        # psnr=True does not touch compute_ssim
        # CPU tensors go to the replaced functions, arguments passed through
        assert M.compute_psnr(torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)).tolist() == [-2.0, -2.0]
        r = DM.compute_depth_metrics_batched(torch.ones(3, 8), torch.ones(3, 8), torch.ones(3, 8, dtype=torch.bool), mult_a=True)
        assert r["abs_diff"].tolist() == [-3.0] * 3 and r["mult_a"] is True
        assert DM.compute_depth_metrics_batched(torch.ones(3, 8), torch.ones(3, 8), torch.ones(3, 8, dtype=torch.bool))["mult_a"] is False
        splatter360_amd.install(depth_metrics=True, psnr=True)   # idempotent
        assert bound(P) == p and bound(D) == d and M.compute_psnr.replaced is psnr0
        splatter360_amd.uninstall()
        assert all(f is psnr0 for f in bound(P).values()) and all(f is depth0 for f in bound(D).values())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(depth_metrics=True, psnr=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 2
        splatter360_amd.install(depth_metrics=True, psnr=True)   # idempotent: no second pair of hooks
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 2
        assert "src.evaluation.metrics" not in sys.modules and "src.scripts.compute_depth_metrics" not in sys.modules
        import src.model.model_wrapper_erp
        assert len(bound(P)) == 2 and native(bound(P)) and len(bound(D)) == 2 and native(bound(D))
        import src.model.model_wrapper_cubemaps, src.evaluation.metric_computer
        p = bound(P)
        assert len(p) == 4 and native(p) and len(set(p.values())) == 1, p
        assert original(bound(S))
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)      # the hooks are gone once they have patched
        splatter360_amd.uninstall()
        assert original(bound(P)) and original(bound(D)) and len(set(bound(P).values())) == 1 and len(set(bound(D).values())) == 1
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (the reference's src/main.py:22-36) sits at sys.meta_path[0] and resolves `src.*` with
    PathFinder itself: the hooks never see the modules.  The next import they are asked about patches them late."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        import splatter360_amd
        splatter360_amd.install(depth_metrics=True, psnr=True)
        class Competing(importlib.abc.MetaPathFinder):
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        import src.model.model_wrapper_erp, src.evaluation.metric_computer
        assert len(bound(P)) == 3 and original(bound(P)) and len(bound(D)) == 2 and original(bound(D))   # behind the hooks' back
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hooks are asked about
        p, d = bound(P), bound(D)
        assert len(p) == 3 and native(p) and len(set(p.values())) == 1, p
        assert len(d) == 2 and native(d) and len(set(d.values())) == 1, d
        import src.model.model_wrapper_cubemaps
        assert native(bound(P)) and len(bound(P)) == 4
        splatter360_amd.uninstall()
        assert original(bound(P)) and original(bound(D))
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_uninstall_drops_pending_hooks(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(depth_metrics=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 1
        splatter360_amd.install(psnr=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 2
        splatter360_amd.uninstall()
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        import src.model.model_wrapper_erp
        assert original(bound(P)) and original(bound(D))
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_each_keyword_binds_its_own_function_only(standin):
    out = _run(standin, """
        for m in ALL:
            importlib.import_module(m)
        import splatter360_amd
        splatter360_amd.install(metrics=True)                    # still compute_ssim only
        assert native(bound(S)) and original(bound(P)) and original(bound(D))
        splatter360_amd.uninstall()
        splatter360_amd.install()                                # neither by default
        assert original(bound(S)) and original(bound(P)) and original(bound(D))
        splatter360_amd.install(psnr=True)
        assert native(bound(P)) and original(bound(S)) and original(bound(D))
        splatter360_amd.uninstall()
        splatter360_amd.install(depth_metrics=True)
        assert native(bound(D)) and original(bound(S)) and original(bound(P))
        splatter360_amd.install(metrics=True, psnr=True)         # the two seams of one module side by side
        assert native(bound(S)) and native(bound(P)) and native(bound(D))
        splatter360_amd.uninstall()
        assert original(bound(S)) and original(bound(P)) and original(bound(D))
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_metrics_and_psnr_hooks_share_the_module_before_import(standin):
    out = _run(standin, """
        import splatter360_amd
        splatter360_amd.install(metrics=True, psnr=True)
        import src.evaluation.metric_computer
        assert native(bound(S)) and native(bound(P)) and len(bound(P)) == 2
        splatter360_amd.uninstall()
        assert original(bound(S)) and original(bound(P))
        print("ok")
    """)
    assert out.strip().endswith("ok")
