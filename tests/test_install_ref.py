"""`splatter360_amd.install()` against the reference's plugin seam, on a stand-in of the reference's own package layout.

The stand-in `src` package is written at test time from tests/golden/reference_seam.json (captured from the reference by
tests/golden/make_golden_seam.py: interface facts only, no source): the registry `DECODERS` / `get_decoder` of
src/model/decoder/__init__.py:5-13, the `Decoder` base and `DecoderOutput` with the reference's forward parameters, the Gaussians
containers, and GaussianAdapterERP with its config, forward parameters and non-persistent sh_mask buffer.  It is a real on-disk
package, so the import hooks of install(lazy=True) see the very import sequence the reference makes; the rasteriser its decoder
module imports is THIS repository's drop-in `diff_gaussian_rasterization`.  Runs on CPU: construction and registry only — the
forward of the registered class is exercised on the GPU from the committed capture (tests/test_gpu_install.py)."""
import json
import subprocess
import sys
import textwrap
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SEAM = json.loads((ROOT / "tests" / "golden" / "reference_seam.json").read_text())


def _write_standin(root: Path) -> None:
    """The stand-in package: every module, class, field and parameter name comes from the capture."""
    d, a = SEAM["decoder"], SEAM["adapter"]

    def put(module: str, text: str = "", package: bool = False) -> None:
        path = root.joinpath(*module.split("."))
        path = path / "__init__.py" if package else path.with_suffix(".py")
        path.parent.mkdir(parents=True, exist_ok=True)
        for parent in list(path.parents)[1 if package else 0:]:     # every enclosing directory up to root is a package
            if parent == root:
                break
            (parent / "__init__.py").touch()
        path.write_text(textwrap.dedent(text))

    def dataclass_src(name, names):
        return f"@dataclasses.dataclass\nclass {name}:\n" + "".join(f"    {n}: object = None\n" for n in names)

    put(d["types_module"], "import dataclasses\n" + dataclass_src("Gaussians", d["gaussians_fields"]))
    put(d["base_module"], f"""
        import abc, dataclasses
        from torch import nn
        {dataclass_src(d["output"], d["output_fields"]).replace(chr(10), chr(10) + "        ")}
        class {d["base"]}(nn.Module, abc.ABC):
            def __init__({", ".join(d["base_init_params"])}):
                super().__init__()
                self.cfg, self.dataset_cfg = cfg, dataset_cfg

            @abc.abstractmethod
            def forward({", ".join(d["forward_params"])}):
                ...
    """)
    put(d["class_module"], f"""
        import diff_gaussian_rasterization   # the rasteriser the reference's decoder imports
        from {d["base_module"]} import {d["base"]}

        class {d["class"]}({d["base"]}):
            def forward({", ".join(d["forward_params"])}):
                raise NotImplementedError("stand-in")
    """)
    put(d["registry_module"], f"""
        from {d["class_module"]} import {d["class"]}
        {d["registry_name"]} = {{{d["key"]!r}: {d["class"]}}}

        def {d["factory"]}(decoder_cfg, dataset_cfg):
            return {d["registry_name"]}[decoder_cfg.name](decoder_cfg, dataset_cfg)
    """, package=True)
    buffers = {n: (b["values"], b["persistent"]) for n, b in a["buffers"].items()}
    put(a["module"], f"""
        import dataclasses
        import torch
        from torch import nn
        {dataclass_src(a["cfg_class"], a["cfg_fields"]).replace(chr(10), chr(10) + "        ")}
        {dataclass_src(a["container"], a["container_fields"]).replace(chr(10), chr(10) + "        ")}
        class {a["class"]}(nn.Module):
            def __init__({", ".join(a["init_params"])}):
                super().__init__()
                self.cfg = cfg
                for name, (values, persistent) in {buffers!r}.items():
                    self.register_buffer(name, torch.tensor(values, dtype=torch.float32), persistent=persistent)

            @property
            def d_sh(self):
                return {a["d_sh"]}

            @property
            def d_in(self):
                return {a["d_in"]}

            def forward({", ".join(a["forward_params"])}):
                raise NotImplementedError("stand-in")
    """)


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    root = tmp_path_factory.mktemp("reference_seam")
    _write_standin(root)
    return root


PRELUDE = textwrap.dedent("""
    import sys, types
    from types import SimpleNamespace
    SEAM = {seam!r}
    sys.path.insert(0, {standin!r})
    sys.path.insert(0, {root!r})
    cfg, dcfg = SimpleNamespace(name=SEAM["decoder"]["key"]), SimpleNamespace(background_color=[0.1, 0.2, 0.3])
""")


def _run(standin: Path, body: str) -> str:
    prelude = PRELUDE.format(seam=SEAM, standin=str(standin), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", prelude + textwrap.dedent(body)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_the_standin_has_the_reference_layout(standin):
    """The stand-in is what the capture says the reference is (registry, class names, signatures, containers, buffers)."""
    out = _run(standin, """
        import dataclasses, inspect, importlib
        d, a = SEAM["decoder"], SEAM["adapter"]
        reg = importlib.import_module(d["registry_module"])
        cls = getattr(reg, d["registry_name"])[d["key"]]
        assert cls.__name__ == d["class"] and cls.__module__ == d["class_module"]
        base = importlib.import_module(d["base_module"])
        assert issubclass(cls, getattr(base, d["base"]))
        assert list(inspect.signature(getattr(base, d["base"]).forward).parameters) == d["forward_params"]
        assert [f.name for f in dataclasses.fields(getattr(base, d["output"]))] == d["output_fields"]
        assert [f.name for f in dataclasses.fields(importlib.import_module(d["types_module"]).Gaussians)] == d["gaussians_fields"]
        amod = importlib.import_module(a["module"])
        ref = getattr(amod, a["class"])(getattr(amod, a["cfg_class"])(**a["cfg"]))
        assert list(inspect.signature(ref.forward).parameters) == a["forward_params"][1:]
        assert list(ref.state_dict().keys()) == a["state_dict_keys"] and (ref.d_sh, ref.d_in) == (a["d_sh"], a["d_in"])
        assert [f.name for f in dataclasses.fields(getattr(amod, a["container"]))] == a["container_fields"]
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_install_registers_the_fused_decoder_under_the_reference_key(standin):
    out = _run(standin, """
        import splatter360_amd
        cls = splatter360_amd.install()
        from src.model.decoder import DECODERS, get_decoder
        from src.model.decoder.decoder import Decoder, DecoderOutput
        import diff_gaussian_rasterization, splatter360_amd.rasterizer as R
        assert diff_gaussian_rasterization.GaussianRasterizer is R.GaussianRasterizer     # the reference imports THIS drop-in
        dec = get_decoder(cfg, dcfg)
        assert type(dec) is cls and DECODERS["splatting_cuda"] is cls and isinstance(dec, Decoder)
        assert cls.replaced.__name__ == "DecoderSplattingCUDA"
        assert [round(float(x), 4) for x in dec.background_color] == [0.1, 0.2, 0.3]
        assert dec.cfg is cfg and dec.dataset_cfg is dcfg
        # the forward contract is the reference's (decoder.py:37-48): same parameter names, in order
        import inspect
        want = list(inspect.signature(Decoder.forward).parameters)
        assert list(inspect.signature(cls.forward).parameters) == want, want
        # no CPU path: a CPU call fails loudly instead of falling back
        import torch
        from src.model.types import Gaussians
        g = Gaussians(torch.zeros(1, 4, 3), torch.eye(3).expand(1, 4, 3, 3).contiguous(), torch.zeros(1, 4, 3, 25), torch.ones(1, 4))
        e = torch.eye(4).expand(1, 6, 4, 4).contiguous(); k = torch.eye(3).expand(1, 6, 3, 3).contiguous()
        try:
            dec.forward(g, e, k, torch.full((1, 6), 0.1), torch.full((1, 6), 10.0), (16, 16))
            raise SystemExit("a CPU call must raise")
        except RuntimeError as ex:
            assert "GPU" in str(ex) or "libs360" in str(ex), ex
        splatter360_amd.uninstall()
        assert DECODERS["splatting_cuda"].__name__ == "DecoderSplattingCUDA"
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_lazy_install_patches_when_the_reference_imports_its_decoder_package(standin):
    out = _run(standin, """
        import splatter360_amd
        assert splatter360_amd.install(lazy=True) is None
        assert "src.model.decoder" not in sys.modules
        from src.model.decoder import get_decoder            # the reference's own import (src/main.py:33)
        dec = get_decoder(cfg, dcfg)
        assert type(dec).__name__ == "DecoderSplattingFusedMI355X", type(dec)
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_lazy_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """jaxtyping's install_import_hook (src/main.py:22-36) puts its own finder at sys.meta_path[0] and resolves `src.*`
    through PathFinder directly, so the lazy patcher never sees `src.model.decoder`.  Emulated here; the registry must still be
    patched by the time the imports of that `with` block are over (any non-`src` import after the package triggers it)."""
    out = _run(standin, """
        import importlib.abc, importlib.machinery
        import splatter360_amd
        assert splatter360_amd.install(lazy=True) is None
        class Competing(importlib.abc.MetaPathFinder):          # what jaxtyping's hook does: first in line, PathFinder for src.*
            def find_spec(self, fullname, path, target=None):
                if fullname == "src" or fullname.startswith("src."):
                    return importlib.machinery.PathFinder.find_spec(fullname, path, target)
                return None
        sys.meta_path.insert(0, Competing())
        from src.model.decoder import DECODERS, get_decoder
        assert DECODERS["splatting_cuda"].__name__ == "DecoderSplattingCUDA"      # not patched yet: the patcher was bypassed
        import colorsys                                                            # any later non-src import (main.py: the encoder's)
        dec = get_decoder(cfg, dcfg)
        assert type(dec).__name__ == "DecoderSplattingFusedMI355X", type(dec)
        from splatter360_amd import plugin
        assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.DECODER_SEAM for f in sys.meta_path)
        print("ok")
    """)
    assert out.strip().endswith("ok")


COMPETING = textwrap.dedent("""
    import importlib.abc, importlib.machinery
    class Competing(importlib.abc.MetaPathFinder):          # what jaxtyping's hook does: first in line, PathFinder for src.*
        def find_spec(self, fullname, path, target=None):
            if fullname == "src" or fullname.startswith("src."):
                return importlib.machinery.PathFinder.find_spec(fullname, path, target)
            return None
""")


def test_adapter_install_survives_a_competing_finder_that_resolves_src_itself(standin):
    """behind jaxtyping's finder the adapter's hook never sees the adapter module either.  The next import it is asked
    about replaces the class, in the defining module and in the encoder module that already bound the name, and the hook leaves
    sys.meta_path."""
    out = _run(standin, COMPETING + textwrap.dedent("""
        import splatter360_amd
        from splatter360_amd import plugin
        assert splatter360_amd.install(lazy=True, adapter=True) is None
        sys.meta_path.insert(0, Competing())
        import src.model.encoder.common.gaussian_adapter_erp as amod
        ref_cls = amod.GaussianAdapterERP
        assert ref_cls.__name__ == "GaussianAdapterERP" and getattr(ref_cls, "replaced", None) is None    # the hook was bypassed
        # a stand-in for the encoder module that already executed its `from .common.gaussian_adapter_erp import GaussianAdapterERP`
        enc = types.ModuleType("src.model.encoder.encoder_costvolume"); enc.GaussianAdapterERP = ref_cls
        sys.modules["src.model.encoder.encoder_costvolume"] = enc
        assert "colorsys" not in sys.modules
        import colorsys                                          # any later import the hook is asked about
        assert amod.GaussianAdapterERP.__name__ == "GaussianAdapterERPFusedMI355X", amod.GaussianAdapterERP
        assert amod.GaussianAdapterERP.replaced is ref_cls and enc.GaussianAdapterERP is amod.GaussianAdapterERP
        assert not any(isinstance(f, plugin._SeamPatcher) and f.seam is plugin.ADAPTER_SEAM for f in sys.meta_path)
        splatter360_amd.uninstall()
        assert amod.GaussianAdapterERP is ref_cls and enc.GaussianAdapterERP is ref_cls
        print("ok")
    """))
    assert out.strip().endswith("ok")


def test_every_pending_hook_is_served_at_the_same_import(standin):
    """A hook that patches late leaves sys.meta_path while the import system walks it, and the walk skips the next entry: the
    hook serves the other pending ones itself, so the registry and the adapter are both patched after ONE later import."""
    out = _run(standin, COMPETING + textwrap.dedent("""
        import splatter360_amd
        from splatter360_amd import plugin
        assert splatter360_amd.install(lazy=True, adapter=True) is None
        assert sum(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path) == 2
        sys.meta_path.insert(0, Competing())
        from src.model.decoder import DECODERS
        import src.model.encoder.common.gaussian_adapter_erp as amod
        ref_dec, ref_cls = DECODERS["splatting_cuda"], amod.GaussianAdapterERP
        assert ref_dec.__name__ == "DecoderSplattingCUDA" and ref_cls.__name__ == "GaussianAdapterERP"   # both hooks were bypassed
        assert "colorsys" not in sys.modules
        import colorsys
        assert DECODERS["splatting_cuda"].__name__ == "DecoderSplattingFusedMI355X" and DECODERS["splatting_cuda"].replaced is ref_dec
        assert amod.GaussianAdapterERP.__name__ == "GaussianAdapterERPFusedMI355X" and amod.GaussianAdapterERP.replaced is ref_cls
        assert not any(isinstance(f, plugin._SeamPatcher) for f in sys.meta_path)
        print("ok")
    """))
    assert out.strip().endswith("ok")


def test_install_twice_uninstall_once_restores_the_reference_decoder(standin):
    """A repeated install() rebuilds the fused class from the reference's class with the latest call's options: `.replaced` never
    is a fused class, and one uninstall() puts the reference's class back."""
    out = _run(standin, """
        import splatter360_amd
        first = splatter360_amd.install()
        from src.model.decoder import DECODERS, get_decoder
        ref_dec = first.replaced
        assert ref_dec.__name__ == "DecoderSplattingCUDA" and get_decoder(cfg, dcfg).fused.check == "sync"
        second = splatter360_amd.install(check="lazy")
        assert DECODERS["splatting_cuda"] is second and second is not first
        assert second.replaced is ref_dec, second.replaced
        assert get_decoder(cfg, dcfg).fused.check == "lazy"
        splatter360_amd.uninstall()
        assert DECODERS["splatting_cuda"] is ref_dec
        print("ok")
    """)
    assert out.strip().endswith("ok")


def test_the_option_table_holds_every_seam_and_every_keyword():
    """uninstall() restores the seams of plugin.OPTION_SEAMS and the decoder seam, nothing else: a seam defined in the module but
    missing from the table would never be undone, and a keyword of install() missing from it would never be installed."""
    import inspect

    from splatter360_amd import plugin
    defined = []
    for value in vars(plugin).values():
        defined += [s for s in (value if isinstance(value, tuple) else (value,)) if isinstance(s, plugin._Seam)]
    table = [s for seams in plugin.OPTION_SEAMS.values() for s in seams]
    assert len(set(map(id, table))) == len(table) and plugin.DECODER_SEAM not in table
    assert {id(s) for s in defined} == {id(s) for s in table} | {id(plugin.DECODER_SEAM)}
    assert all(s.keyword == keyword for keyword, seams in plugin.OPTION_SEAMS.items() for s in seams)
    params = inspect.signature(plugin.install).parameters.values()
    assert {p.name for p in params if p.kind is p.KEYWORD_ONLY} == set(plugin.OPTION_SEAMS) | {"lazy", "adapter_options"}


ADAPTER_PRELUDE = textwrap.dedent("""
    import torch
""")


def test_install_adapter_replaces_the_class_the_encoder_instantiates(standin):
    """install(adapter=True) BEFORE the reference imports its encoder: the module that defines GaussianAdapterERP
    (gaussian_adapter_erp.py:33) is patched as it loads, so the encoder's own `from .common.gaussian_adapter_erp import
    GaussianAdapterERP` (encoder_costvolume.py:19, instantiated at :185) binds the replacement — a subclass of the reference's class
    with its constructor, `d_sh` / `d_in` and `sh_mask`, returning the reference's own adapter-side container."""
    out = _run(standin, ADAPTER_PRELUDE + textwrap.dedent("""
        import splatter360_amd
        splatter360_amd.install(lazy=True, adapter=True)
        assert "src.model.encoder.common.gaussian_adapter_erp" not in sys.modules
        # what encoder_costvolume.py:19 executes
        from src.model.encoder.common.gaussian_adapter_erp import GaussianAdapterERP, GaussianAdapterERPCfg
        amod = sys.modules["src.model.encoder.common.gaussian_adapter_erp"]
        assert GaussianAdapterERP.__name__ == "GaussianAdapterERPFusedMI355X", GaussianAdapterERP
        ref_cls = GaussianAdapterERP.replaced
        assert ref_cls.__name__ == "GaussianAdapterERP" and issubclass(GaussianAdapterERP, ref_cls)
        cfg_a = GaussianAdapterERPCfg(gaussian_scale_min=0.5, gaussian_scale_max=15.0, sh_degree=4)       # config/model/encoder/costvolume.yaml:14-16
        mod = GaussianAdapterERP(cfg_a)                                                                    # encoder_costvolume.py:185
        ref = ref_cls(cfg_a)
        assert isinstance(mod, ref_cls) and mod.cfg is cfg_a and mod.d_sh == ref.d_sh == 25 and mod.d_in == ref.d_in == 82
        assert torch.equal(mod.sh_mask, ref.sh_mask) and "sh_mask" not in mod.state_dict()                # non-persistent, like the reference's
        assert list(mod.state_dict().keys()) == list(ref.state_dict().keys())                             # checkpoints load unchanged
        import inspect
        assert list(inspect.signature(mod.forward).parameters) == list(inspect.signature(ref.forward).parameters)
        try:
            mod.forward("hm3d", torch.eye(4).reshape(1, 1, 1, 1, 1, 4, 4), torch.ones(1, 1, 8, 1, 1), torch.ones(1, 1, 8, 1, 1), torch.zeros(1, 1, 8, 1, 1, 82), (2, 4))
            raise SystemExit("a CPU call must raise")
        except RuntimeError as ex:
            assert "GPU" in str(ex), ex
        # installing again is idempotent; uninstall puts the reference's class back
        splatter360_amd.install(lazy=True, adapter=True)
        assert amod.GaussianAdapterERP is GaussianAdapterERP
        splatter360_amd.uninstall()
        assert amod.GaussianAdapterERP is ref_cls
        print("ok")
    """))
    assert out.strip().endswith("ok")


def test_install_adapter_after_the_encoder_was_imported_patches_the_bound_name_too(standin):
    out = _run(standin, ADAPTER_PRELUDE + textwrap.dedent("""
        import importlib
        amod = importlib.import_module("src.model.encoder.common.gaussian_adapter_erp")
        # a stand-in for the encoder module that already executed its `from .common.gaussian_adapter_erp import GaussianAdapterERP`
        enc = types.ModuleType("src.model.encoder.encoder_costvolume"); enc.GaussianAdapterERP = amod.GaussianAdapterERP
        sys.modules["src.model.encoder.encoder_costvolume"] = enc
        import splatter360_amd
        splatter360_amd.install(lazy=True, adapter=True, adapter_options=dict(sh_rotation="identity"))
        assert amod.GaussianAdapterERP.__name__ == "GaussianAdapterERPFusedMI355X" and enc.GaussianAdapterERP is amod.GaussianAdapterERP
        # the lazy fields pass through the reference's own containers: the adapter-side dataclass and src/model/types.py's Gaussians
        from splatter360_amd import lazy
        from src.model.types import Gaussians
        from einops import rearrange
        bd = lazy.RawBundle(None, "hm3d", torch.eye(4).expand(1, 2, 4, 4), torch.ones(1, 2, 8, 1, 1), torch.ones(1, 2, 8, 1, 1), torch.zeros(1, 2, 8, 1, 1, 82), (2, 4), 1e-8)
        f = lambda n, t: lazy.LazyField(bd, n, (1, 2, 8, 1, 1) + t)
        a = amod.Gaussians(means=f("means", (3,)), covariances=f("covariances", (3, 3)), scales=f("scales", (3,)), rotations=f("rotations", (4,)),
                           harmonics=f("harmonics", (3, 25)), opacities=bd.opacities)
        g = Gaussians(rearrange(a.means, "b v r srf spp xyz -> b (v r srf spp) xyz"), rearrange(a.covariances, "b v r srf spp i j -> b (v r srf spp) i j"),
                      rearrange(a.harmonics, "b v r srf spp c d_sh -> b (v r srf spp) c d_sh"), rearrange(1 * a.opacities, "b v r srf spp -> b (v r srf spp)"))   # encoder_costvolume.py:490-507
        assert lazy.bundle_of(g) is bd
        print("ok")
    """))
    assert out.strip().endswith("ok")
