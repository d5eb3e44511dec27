"""`splatter360_amd.install(depth_tail=True)`: the predictor module's `F` and EncoderCostVolume.map_pdf_to_opacity rebound in the
unchanged reference, on CPU.

The stand-in `src` package is tests/test_install_ref.py's, plus the two modules of tests/depth_tail_reference.py under the
reference's names: src/model/encoder/costvolume/depth_predictor_multiview_360.py binds torch.nn.functional as `F` and calls
F.softmax and F.interpolate through it, and src/model/encoder/encoder_costvolume.py defines EncoderCostVolume with its
map_pdf_to_opacity.  Each case runs in a fresh interpreter.  The GPU half (the rebound names running the kernels) is in
tests/test_gpu_depth_tail.py."""
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

import depth_tail_reference as R
from splatter360_amd import plugin
from test_install_ref import _write_standin

ROOT = Path(__file__).resolve().parent.parent


def _put(root: Path, module: str, text: str) -> None:
    path = root.joinpath(*module.split(".")).with_suffix(".py")
    path.parent.mkdir(parents=True, exist_ok=True)
    for parent in path.parents:
        if parent == root:
            break
        (parent / "__init__.py").touch()
    path.write_text(text)


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_depth_tail_seam")
    _write_standin(root)
    _put(root, plugin.COST_VOLUME_MODULE, R.PREDICTOR_SOURCE)
    _put(root, plugin.DEPTH_TAIL_MODULE, R.ENCODER_SOURCE)
    return root


PRELUDE = textwrap.dedent("""
    import importlib, sys
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    import torch
    import torch.nn.functional as TF
    import splatter360_amd
    from splatter360_amd import plugin, depth_head, depth_tail
    PRED, ENC = plugin.COST_VOLUME_MODULE, plugin.DEPTH_TAIL_MODULE

    def layers(F):
        out = []
        while getattr(F, "replaced", None) is not None:
            out.append(type(F))
            F = F.replaced
        return out, F

    def hooks():
        return [f.seam for f in sys.meta_path if isinstance(f, plugin._SeamPatcher)]

    def method():
        return sys.modules[ENC].EncoderCostVolume.__dict__["map_pdf_to_opacity"]
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(standin=str(standin), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_install_rebinds_method_and_proxy_falls_back_on_cpu_and_uninstall_restores_by_identity(standin):
    out = _run(standin, """
        import inspect
        assert inspect.signature(plugin.install).parameters["depth_tail"].default is False
        P, E = importlib.import_module(PRED), importlib.import_module(ENC)
        original = method()
        assert P.F is TF
        depth, pmax = 0.5 + torch.rand(2, 1, 3, 5), torch.rand(2, 1, 3, 5)
        pdf = torch.rand(2, 2, 15, 1, 1)
        enc = E.EncoderCostVolume(initial=0.0, final=2.0, warm_up=100)
        before = (*P.fullres(depth, pmax, 4), P.half_pixel(depth, 2), enc.map_pdf_to_opacity(pdf, 50))
        splatter360_amd.install(depth_tail=True)
        assert layers(P.F) == ([depth_tail.InterpolateProxy], TF)
        assert method().replaced is original and method() is not original
        assert P.F.softmax is TF.softmax and P.F.grid_sample is TF.grid_sample     # every other attribute: torch's own
        # CPU tensors go through the replaced functions and give their exact results
        after = (*P.fullres(depth, pmax, 4), P.half_pixel(depth, 2), enc.map_pdf_to_opacity(pdf, 50))
        assert all(torch.equal(x, y) for x, y in zip(before, after))
        assert torch.equal(P.F.interpolate(depth, None, 2.0), TF.interpolate(depth, None, 2.0))
        assert torch.equal(P.F.interpolate(depth, size=(7, 9), mode="bicubic"), TF.interpolate(depth, size=(7, 9), mode="bicubic"))
        proxy, fn = P.F, method()
        assert splatter360_amd.plugin.install_depth_tail() == (proxy, fn) and P.F is proxy and method() is fn      # idempotent
        splatter360_amd.uninstall()
        assert P.F is TF and method() is original
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_interpolate_calls_the_native_path_takes_and_leaves(standin):
    """Which F.interpolate calls would run the kernel.  The decision reads only the arguments and the input's device, dtype and
    shape, so a CPU tensor that claims to be on the GPU shows it here."""
    out = _run(standin, """
        class Fake(torch.Tensor):
            is_cuda = True
        x = torch.rand(2, 1, 3, 5).as_subclass(Fake)
        take = depth_tail._native_interpolate_call
        assert take((x,), dict(scale_factor=4))[0] is x and take((x,), dict(scale_factor=4))[1:] == (4, "nearest")
        assert take((x,), dict(scale_factor=4.0, mode="bilinear", align_corners=True))[1:] == (4, "bilinear")
        assert take((x, None, 3), {})[1:] == (3, "nearest")
        assert take((), dict(input=x, scale_factor=2, mode="nearest"))[1:] == (2, "nearest")
        for args, kwargs in (((x,), dict(scale_factor=4, mode="bilinear", align_corners=False)),
                             ((x,), dict(scale_factor=4, mode="bilinear")),
                             ((x,), dict(scale_factor=1.5)), ((x,), dict(scale_factor=(2, 2))), ((x,), dict(size=(6, 10))),
                             ((x,), dict(scale_factor=2, mode="bicubic", align_corners=True)),
                             ((x,), dict(scale_factor=2, recompute_scale_factor=True)), ((x,), dict(scale_factor=2, antialias=False)),
                             ((x.double(),), dict(scale_factor=2)), ((x[0],), dict(scale_factor=2)),
                             ((x.expand(2, 3, 3, 5),), dict(scale_factor=2)), ((torch.rand(2, 1, 3, 5),), dict(scale_factor=2)),
                             ((x,), dict(scale_factor=True)), ((x,), dict(scale_factor=0)), ((x,), {})):
            assert take(args, kwargs) is None, (args[0].shape, kwargs)
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_default_install_touches_neither(standin):
    out = _run(standin, """
        P, E = importlib.import_module(PRED), importlib.import_module(ENC)
        original = method()
        splatter360_amd.install()
        assert P.F is TF and method() is original and not hooks()
        splatter360_amd.install(lazy=True, depth_head=True, cost_volume=False)
        assert layers(P.F) == ([depth_head.FunctionalProxy], TF) and method() is original
        assert P.F.interpolate is TF.interpolate
        print("ok")
    """)
    assert out.strip().endswith("ok")


@pytest.mark.parametrize("order", ["head_first", "tail_first", "one_call"])
def test_depth_head_and_depth_tail_compose_in_either_order(standin, order):
    out = _run(standin, f"""
        ORDER = {order!r}
        P, E = importlib.import_module(PRED), importlib.import_module(ENC)
        original = method()
        z, c = torch.randn(2, 5, 3, 4), torch.rand(2, 5, 1, 1) + 1
        before = (*P.depth_head(z, c), *P.fullres(*P.depth_head(z, c), 4))
        if ORDER == "head_first":
            plugin.install_depth_head(); plugin.install_depth_tail()
        elif ORDER == "tail_first":
            plugin.install_depth_tail(); plugin.install_depth_head()
        else:
            splatter360_amd.install(lazy=True, depth_head=True, depth_tail=True)
        kinds, base = layers(P.F)
        assert sorted(k.__name__ for k in kinds) == ["FunctionalProxy", "InterpolateProxy"] and base is TF
        plugin.install_depth_head(); plugin.install_depth_tail()                  # idempotent: no third layer
        assert layers(P.F)[0] == kinds
        # both answers are reachable through the stack, whichever proxy is outermost
        assert P.F.softmax.__func__ is depth_head.FunctionalProxy.softmax
        assert P.F.interpolate.__func__ is depth_tail.InterpolateProxy.interpolate
        assert P.F.grid_sample is TF.grid_sample
        after = (*P.depth_head(z, c), *P.fullres(*P.depth_head(z, c), 4))          # CPU: the replaced functions, exact results
        assert all(torch.equal(x, y) for x, y in zip(before, after))
        splatter360_amd.uninstall()
        assert P.F is TF and method() is original
        # each seam takes out its own layer alone, wherever it sits
        plugin.install_depth_tail(); plugin.install_depth_head()
        plugin.DEPTH_TAIL_F_SEAM.restore()
        assert layers(P.F) == ([depth_head.FunctionalProxy], TF)
        plugin.install_depth_tail()
        plugin.DEPTH_TAIL_F_SEAM.restore()
        assert layers(P.F) == ([depth_head.FunctionalProxy], TF)
        plugin.install_depth_tail()
        plugin.DEPTH_HEAD_SEAM.restore()
        assert layers(P.F) == ([depth_tail.InterpolateProxy], TF)
        splatter360_amd.uninstall()
        assert P.F is TF
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_before_import_patches_both_modules_on_first_import(standin):
    out = _run(standin, """
        splatter360_amd.install(depth_tail=True, depth_head=True)
        assert PRED not in sys.modules and ENC not in sys.modules
        assert sorted(s.keyword for s in hooks()) == ["depth_head", "depth_tail", "depth_tail"]
        P = importlib.import_module(PRED)
        assert sorted(k.__name__ for k in layers(P.F)[0]) == ["FunctionalProxy", "InterpolateProxy"] and layers(P.F)[1] is TF
        assert [s.keyword for s in hooks()] == ["depth_tail"]
        E = importlib.import_module(ENC)
        assert method().replaced is not None and not hooks()
        enc = E.EncoderCostVolume(initial=1.0, final=1.0)
        pdf = torch.rand(7)
        assert torch.equal(enc.map_pdf_to_opacity(pdf, 3), method().replaced(enc, pdf, 3))
        splatter360_amd.uninstall()
        assert P.F is TF and getattr(method(), "replaced", None) is None
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (the reference's src/main.py:22-36) sits at sys.meta_path[0] and resolves `src.*` with
    PathFinder itself: the hooks never see the two modules.  The next import they are asked about patches both late."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        splatter360_amd.install(depth_tail=True)
        class Competing(importlib.abc.MetaPathFinder):
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        P, E = importlib.import_module(PRED), importlib.import_module(ENC)
        original = method()
        assert P.F is TF and getattr(original, "replaced", None) is None and len(hooks()) == 2      # imported behind the hooks' backs
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hooks are asked about
        assert layers(P.F) == ([depth_tail.InterpolateProxy], TF) and method().replaced is original
        assert not hooks()
        splatter360_amd.uninstall()
        assert P.F is TF and method() is original
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_uninstall_drops_pending_hooks(standin):
    out = _run(standin, """
        splatter360_amd.install(depth_tail=True)
        assert len(hooks()) == 2
        splatter360_amd.uninstall()
        assert not hooks()
        P, E = importlib.import_module(PRED), importlib.import_module(ENC)
        assert P.F is TF and getattr(method(), "replaced", None) is None
        print("ok")
    """)
    assert out.strip().endswith("ok")
