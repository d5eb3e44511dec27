"""`splatter360_amd.install(visualization=True)`: the evaluation step's depth_map, prep_image and apply_color_map rebound in the
unchanged reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's plus the layout of the reference: src/model/model_wrapper_erp.py
defines depth_map (:122-133) and calls it as a module global; src/misc/image_io.py defines prep_image (:38-54), which its own
save_image calls as a global and which model_wrapper_erp.py:22 and model_wrapper_cubemaps.py:23 bind with `from ... import`;
src/visualization/color_map.py defines apply_color_map (:9-19), which its own apply_color_map_to_image calls as a global and
which src/model/encoder/visualization/encoder_visualizer_costvolume.py:15 binds by name.  The stand-in functions return strings,
so a call shows which function ran.  The GPU half (the patched functions returning the kernels' pictures) is in
tests/test_gpu_depth_vis.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent
PREP_USERS = ("src.model.model_wrapper_erp", "src.model.model_wrapper_cubemaps")
COLOR_USERS = ("src.model.encoder.visualization.encoder_visualizer_costvolume",)


def _write_visualization(root: Path) -> None:
    def put(rel: str, text: str) -> None:
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        for parent in path.parents:
            if parent == root:
                break
            (parent / "__init__.py").touch()
        path.write_text(textwrap.dedent(text))

    put("src/misc/image_io.py", """
        def prep_image(image):
            return "reference prep_image"

        def save_image(image, path):
            return prep_image(image)
    """)
    put("src/visualization/color_map.py", """
        def apply_color_map(x, color_map="inferno"):
            return "reference apply_color_map " + color_map

        def apply_color_map_to_image(image, color_map="inferno"):
            return apply_color_map(image, color_map)
    """)
    put("src/model/model_wrapper_erp.py", """
        from ..misc.image_io import prep_image, save_image
        from ..visualization.color_map import apply_color_map_to_image

        def depth_map(result):
            return "reference depth_map"

        def test_step(depth):
            return depth_map(depth)
    """)
    put("src/model/model_wrapper_cubemaps.py", "from ..misc.image_io import prep_image, save_image\n")
    put("src/model/encoder/visualization/encoder_visualizer_costvolume.py",
        "from ....visualization.color_map import apply_color_map, apply_color_map_to_image\n")


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_visualization_seam")
    _write_standin(root)
    _write_visualization(root)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    PREP_USERS, COLOR_USERS = {prep_users!r}, {color_users!r}
    ERP, IO, CM = "src.model.model_wrapper_erp", "src.misc.image_io", "src.visualization.color_map"
    ALL = sorted(set(PREP_USERS + COLOR_USERS))
    import torch

    def bound(name):
        definer, users = {{"depth_map": (ERP, ()), "prep_image": (IO, PREP_USERS), "apply_color_map": (CM, COLOR_USERS)}}[name]
        return {{m: getattr(sys.modules[m], name) for m in (definer, *users) if m in sys.modules}}

    def native(fns):
        return all(getattr(f, "replaced", None) is not None for f in fns.values())

    def original(fns):
        return all(getattr(f, "replaced", None) is None for f in fns.values())

    D, P, A = "depth_map", "prep_image", "apply_color_map"
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT), prep_users=PREP_USERS, color_users=COLOR_USERS)
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_after_import_rebinds_every_user(standin):
    out = _run(standin, """
        for m in ALL:
            importlib.import_module(m)
        erp, io, cm = sys.modules[ERP], sys.modules[IO], sys.modules[CM]
        d0, p0, a0 = erp.depth_map, io.prep_image, cm.apply_color_map
        import splatter360_amd
        splatter360_amd.install(visualization=True)
        d, p, a = bound(D), bound(P), bound(A)
        assert len(d) == 1 and native(d), d
        assert len(p) == 3 and native(p) and len(set(p.values())) == 1, p
        assert len(a) == 2 and native(a) and len(set(a.values())) == 1, a
        assert erp.depth_map.replaced is d0 and io.prep_image.replaced is p0 and cm.apply_color_map.replaced is a0
        # CPU tensors, and colour maps without a table, go to the replaced functions: through the module globals too
        x = torch.rand(4, 5)
        assert erp.depth_map(x) == "reference depth_map" and erp.test_step(x) == "reference depth_map"
        assert io.prep_image(x) == "reference prep_image" and io.save_image(x, "p") == "reference prep_image"
        assert erp.prep_image(x) == "reference prep_image"
        assert cm.apply_color_map(x) == "reference apply_color_map inferno"
        assert cm.apply_color_map(x, "magma") == "reference apply_color_map magma"
        assert cm.apply_color_map(x, color_map="turbo") == "reference apply_color_map turbo"
        assert cm.apply_color_map_to_image(x, "viridis") == "reference apply_color_map viridis"
        assert erp.depth_map("not a tensor") == "reference depth_map" and io.prep_image(None) == "reference prep_image"
        splatter360_amd.install(visualization=True)              # idempotent
        assert bound(D) == d and bound(P) == p and bound(A) == a and io.prep_image.replaced is p0
        splatter360_amd.uninstall()
        assert erp.depth_map is d0 and all(f is p0 for f in bound(P).values()) and all(f is a0 for f in bound(A).values())
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_on_first_import(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(visualization=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 3
        splatter360_amd.install(visualization=True)              # idempotent: no second set of hooks
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 3
        assert ERP not in sys.modules and IO not in sys.modules and CM not in sys.modules
        import src.model.model_wrapper_erp
        assert native(bound(D)) and len(bound(P)) == 2 and native(bound(P)) and len(bound(A)) == 1 and native(bound(A))
        import src.model.model_wrapper_cubemaps, src.model.encoder.visualization.encoder_visualizer_costvolume
        p, a = bound(P), bound(A)
        assert len(p) == 3 and native(p) and len(set(p.values())) == 1, p
        assert len(a) == 2 and native(a) and len(set(a.values())) == 1, a
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)      # the hooks are gone once they have patched
        assert sys.modules[ERP].test_step(torch.rand(3, 3)) == "reference depth_map"
        splatter360_amd.uninstall()
        assert original(bound(D)) and original(bound(P)) and original(bound(A))
        assert len(set(bound(P).values())) == 1 and len(set(bound(A).values())) == 1
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (the reference's src/main.py:22-36) sits at sys.meta_path[0] and resolves `src.*` with
    PathFinder itself: the hooks never see the modules.  The next import they are asked about patches them late."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        import splatter360_amd
        splatter360_amd.install(visualization=True)
        class Competing(importlib.abc.MetaPathFinder):
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        import src.model.model_wrapper_erp, src.model.encoder.visualization.encoder_visualizer_costvolume
        assert original(bound(D)) and original(bound(P)) and original(bound(A))        # behind the hooks' back
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hooks are asked about
        d, p, a = bound(D), bound(P), bound(A)
        assert native(d) and len(p) == 2 and native(p) and len(set(p.values())) == 1, p
        assert len(a) == 2 and native(a) and len(set(a.values())) == 1, a
        import src.model.model_wrapper_cubemaps
        assert native(bound(P)) and len(bound(P)) == 3
        splatter360_amd.uninstall()
        assert original(bound(D)) and original(bound(P)) and original(bound(A))
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_off_by_default_and_uninstall_drops_pending_hooks(standin):
    out = _run(standin, """
        import splatter360_amd
        from splatter360_amd import plugin
        splatter360_amd.install(visualization=True)
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 3
        splatter360_amd.uninstall()
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        for m in ALL:
            importlib.import_module(m)
        assert original(bound(D)) and original(bound(P)) and original(bound(A))
        splatter360_amd.install()                                # off by default
        assert original(bound(D)) and original(bound(P)) and original(bound(A))
        splatter360_amd.install(psnr=True, erp_distance=True)    # the other seams leave these alone
        assert original(bound(D)) and original(bound(P)) and original(bound(A))
        splatter360_amd.uninstall()
        print("ok")
    """)
    assert out.strip().endswith("ok")
