"""Plug the fused MI355X decoder into the UNCHANGED reference through the reference's own plugin seam.

The reference builds its decoder with `get_decoder(cfg.model.decoder, cfg.dataset)` (/root/reference/src/main.py:168), which looks
the class up in the registry `DECODERS = {"splatting_cuda": DecoderSplattingCUDA}` (/root/reference/src/model/decoder/__init__.py:5-13)
under the key `config/model/decoder/splatting_cuda.yaml:1` names.  `install()` replaces that registry entry with a subclass of the
reference's own `Decoder` base (src/model/decoder/decoder.py:26-48: same constructor `(cfg, dataset_cfg)`, same `forward`
contract, returns the reference's `DecoderOutput`) whose forward renders every target panorama's six faces — colour and depth
together — in ONE rasteriser call of this library instead of twelve Python-looped drop-in calls
(decoder_splatting_cuda.py:47-59,72-97).  Encoder, losses, Lightning wrapper, configs: untouched.

    import splatter360_amd; splatter360_amd.install()        # one line before the reference's `main` runs, or
    PYTHONPATH=/path/to/repo/examples/site python -m src.main +experiment=hm3d ...   # examples/site/sitecustomize.py does it lazily

install(metrics=True) also rebinds the evaluation step's `compute_ssim` (src/evaluation/metrics.py:38-54: skimage, one image at a
time on the host) to metrics.compute_ssim (one SSIM kernel per batch on the GPU; CPU tensors still go to the replaced function),
in src.evaluation.metrics and in every module that imported the name: now if they are imported, else by an import hook.
install(depth_loss=True) likewise rebinds the training step's compute_l1_sphere_loss and erode (src/model/model_wrapper_helper.py)
to depth_loss.compute_l1_sphere_loss / depth_loss.erode, in that module and in src.model.model_wrapper_erp.
install(psnr=True) rebinds compute_psnr (src/evaluation/metrics.py:11-21) to metrics.compute_psnr in the same modules as
compute_ssim, and install(depth_metrics=True) rebinds compute_depth_metrics_batched (src/scripts/compute_depth_metrics.py:47-116)
to metrics.compute_depth_metrics_batched in that module and in src.model.model_wrapper_erp.
install(cost_volume=True) rebinds the encoder's warp_with_pose_depth_candidates
(src/model/encoder/costvolume/depth_predictor_multiview_360.py:73-214) to a lazy handle, so that the predictor's own forward
builds its correlation volume with the fused kernels of cost_volume.py and never forms the [v b, C, D, h, w] warped tensor.
install(depth_head=True) rebinds the name `F` (torch.nn.functional) of that same module to a proxy whose softmax(x, dim=1) returns
a lazy handle, so that the predictor's softmax, expected depth and pdf maximum (:643-651) run as the one fused reduction of
depth_head.py and the [v b, D, h, w] softmax is never stored; every other attribute of the proxy is torch.nn.functional's own.
install(depth_tail=True) rebinds the same `F` to a proxy whose interpolate runs the upsampling kernels of depth_tail.py for the
predictor's two calls (:652-658), and EncoderCostVolume.map_pdf_to_opacity (src/model/encoder/encoder_costvolume.py:228-241) to the
opacity-map kernel; the two `F` proxies stack in either order.  The predictor's :694-719 have no seam; depth_tail.fine_depth_tail
is the direct API for them.
install(erp_distance=True) rebinds depth_to_distance_map_batch (src/geometry/z_depth_to_distance.py:4-34) to the z-depth -> distance
kernel of stitch.py, in that module and in src.model.model_wrapper_erp (:48), for the call the evaluation step makes (:457: square
float32 GPU maps, intrinsics broadcast by einops.repeat).  The step's reorder, conversion and stitch (:446-463) are inline
statements with no seam of their own; stitch.Cube2Equirec.stitch_distance_rendered is the direct API for the three as one kernel.
install(depth_smoothness=True) rebinds LossDepth.forward (src/loss/loss_depth.py:27-60) to the depth-smoothness kernels of
depth_smooth.py for float32 GPU batches; every other call reaches the replaced method.
install(group_norm=True) rebinds ResBlock._forward and AttentionBlock._forward (src/model/encoder/costvolume/ldm_unet/unet.py),
ResidualBlock.forward (src/model/encoder/backbone/unimatch/backbone.py) and DepthPredictorMultiView360.__init__ so that the
encoder's norm + activation (+ residual) sites run the fused kernels of group_norm.py; every form the wrappers do not recognise
reaches the replaced method.
install(unet_attention=True) rebinds QKVAttentionLegacy.forward and QKVAttention.forward (ldm_unet/unet.py:527-599) to the fused
QKV-attention kernels of qkv_attention.py for float32 GPU qkv with 32 channels per head; every other call reaches the
replaced method.
install(transformer_ffn=True) rebinds TransformerLayer.forward (src/model/encoder/backbone/multiview_transformer.py:334-414) so that
everything behind the layer's attention — norm1, the concatenation, the two-Linear GELU mlp, norm2 and the residual — runs the fused
kernels of transformer_ffn.py; the projections and merge stay the layer's own nn.Linears and the attention is called through the
module's globals, so window_attention=True composes in either order; every form the wrapper does not recognise reaches the
replaced method.
install(window_attention=True) rebinds that module's single_head_split_window_attention and single_head_full_attention to the fused
kernels of window_attention.py; window_attention_precision="high" runs their bf16x3 products, "torch" whatever
torch.get_float32_matmul_precision() asks for at the call (the reference's main sets 'high').

Without install() the reference still runs on this library through the drop-in module `diff_gaussian_rasterization`
 — per face, per pass, with upstream's host synchronisations; bench.py prints both step times.
"""
from __future__ import annotations

import importlib
import importlib.abc
import importlib.util
import sys
from typing import Optional

import torch

from . import precision as _precision

REGISTRY_MODULE = "src.model.decoder"
REGISTRY_KEY = "splatting_cuda"
ADAPTER_MODULE = "src.model.encoder.common.gaussian_adapter_erp"      # defines GaussianAdapterERP (:33-119)
ADAPTER_USERS = ("src.model.encoder.encoder_costvolume",)             # `from .common.gaussian_adapter_erp import GaussianAdapterERP` (:19), used at :185
ADAPTER_NAME = "GaussianAdapterERP"


def make_decoder_class(base_cls, output_cls, *, views_per_group: int = 6, shared_campos: Optional[bool] = None, check: str = "sync",
                       glue: str = "native", name: str = "DecoderSplattingFusedMI355X"):
    """A decoder class with the reference's constructor and forward contract (decoder.py:26-48) on the fused path.
    base_cls / output_cls: the reference's `Decoder` / `DecoderOutput` (install()), or this package's mirrors (tests on a box
    without the reference).  The options are those of decoder.DecoderSplattingFused."""
    from . import decoder as _dec

    class _Fused(base_cls):
        def __init__(self, cfg, dataset_cfg) -> None:
            try:
                super().__init__(cfg, dataset_cfg)
            except TypeError:        # a plain nn.Module base (the mirror): no (cfg, dataset_cfg) constructor
                torch.nn.Module.__init__(self)
                self.cfg, self.dataset_cfg = cfg, dataset_cfg
            bg = tuple(float(c) for c in dataset_cfg.background_color)
            self.fused = _dec.DecoderSplattingFused(background_color=bg, views_per_group=views_per_group, shared_campos=shared_campos,
                                                    check=check, glue=glue)

        @property
        def background_color(self):          # the attribute the reference's own decoder exposes (decoder_splatting_cuda.py:28-32)
            return self.fused.background_color

        def forward(self, gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode=None):
            out = self.fused(gaussians, extrinsics, intrinsics, near, far, tuple(int(x) for x in image_shape), depth_mode=depth_mode)
            return output_cls(out.color, out.depth)

        def render_depth(self, gaussians, extrinsics, intrinsics, near, far, image_shape, mode="depth"):
            """decoder_splatting_cuda.py:72-97 (used by the visualisation scripts): the depth channel of the same fused pass."""
            return self.forward(gaussians, extrinsics, intrinsics, near, far, image_shape, depth_mode=mode).depth

    _Fused.__name__ = _Fused.__qualname__ = name
    return _Fused


class _Seam:
    """One rebinding seam: functions `names` defined in `module` and bound with `from ... import` by `users`; wrappers[name](replaced)
    builds the replacement (which keeps the original as `.replaced`).  With context=True the wrapper is called as
    wrappers[name](replaced, defining module, **options), options being those of the install() call that placed the seam."""

    def __init__(self, keyword, module, names, users, wrappers, context=False):
        self.keyword, self.module, self.names, self.users, self.wrappers = keyword, module, tuple(names), tuple(users), wrappers
        self.context, self.options = context, {}

    def ready(self, mod) -> bool:
        return mod is not None and all(hasattr(mod, n) for n in self.names)

    def patch(self, mod) -> dict:
        """Rebind the names in the defining module and in every already-imported user that still holds the original (modules
        imported later bind the replacements themselves).  Idempotent."""
        out = {}
        for name in self.names:
            cur = getattr(mod, name)
            if getattr(cur, "replaced", None) is not None:
                fn = cur
            else:
                fn = self.wrappers[name](cur, mod, **self.options) if self.context else self.wrappers[name](cur)
            setattr(mod, name, fn)
            for user in self.users:
                um = sys.modules.get(user)
                if um is not None and getattr(um, name, None) is fn.replaced:
                    setattr(um, name, fn)
            out[name] = fn
        return out

    def restore(self) -> None:
        mod = sys.modules.get(self.module)
        if mod is None:
            return
        for name in self.names:
            cur = getattr(mod, name, None)
            if getattr(cur, "replaced", None) is not None:
                setattr(mod, name, cur.replaced)
                for user in self.users:
                    um = sys.modules.get(user)
                    if um is not None and getattr(um, name, None) is cur:
                        setattr(um, name, cur.replaced)

    def install(self, **options):
        """Patch now if the module is imported, else put a _SeamPatcher on sys.meta_path.  Returns {name: function} or None.
        A pending hook keeps the options of the call that placed it.  A wrapper that an earlier call built with other options
        is taken out first and built again (patch() keeps a wrapper it finds), so `options` is what the bound wrapper runs with."""
        mod = sys.modules.get(self.module)
        if self.ready(mod):
            if self.context and options != self.options:
                self.restore()
            self.options = options
            return self.patch(mod)
        if not any(isinstance(f, _SeamPatcher) and f.seam is self for f in sys.meta_path):
            self.options = options
            sys.meta_path.insert(0, _SeamPatcher(self))
        return None


class _SeamPatcher(importlib.abc.MetaPathFinder):
    """The import hook of a _Seam installed before its module is imported: patch the module as it is first loaded, and — for an
    import made through a finder ahead of this one — at the next import this finder is asked about, before a step can call the
    functions.  ANY later import is a chance to patch: the reference imports its packages inside jaxtyping's install_import_hook
    (the reference's src/main.py:22-36), whose own finder is inserted at sys.meta_path[0] afterwards and resolves every `src.*`
    module by calling PathFinder directly — this finder is then never asked for the seam's module itself, but it is
    asked for the first non-`src` module imported after it (the encoder's third-party imports, still inside that `with` block and
    long before get_decoder runs at main.py:168).  A failure on that late path warns and never surfaces from the unrelated
    third-party import; a failure while the seam's own module loads through this finder's loader propagates."""

    def __init__(self, seam):
        self.seam, self.busy = seam, False

    def _done(self, mod):
        if self in sys.meta_path:
            sys.meta_path.remove(self)
        self.seam.patch(mod)

    def _late(self) -> bool:
        """Patch now if the module was imported behind this finder's back.  True if it was."""
        seam = self.seam
        mod = sys.modules.get(seam.module)
        if self.busy or not seam.ready(mod):
            return False
        self.busy = True
        try:
            self._done(mod)
        except Exception as ex:      # never let the failure surface from an unrelated import
            import warnings
            warnings.warn(f"splatter360_amd.install({seam.keyword}=True): patching {seam.module} failed ({ex!r}); the "
                          "reference keeps its own functions.", RuntimeWarning)
        finally:
            self.busy = False
        return True

    def find_spec(self, fullname, path, target=None):
        if self.busy:
            return None
        seam = self.seam
        if self._late():
            # this finder has just left sys.meta_path, the list the import system is walking: the walk skips the entry after
            # it, so the other pending seams are served here and not at some later import
            for other in [f for f in sys.meta_path if isinstance(f, _SeamPatcher)]:
                other._late()
            return None
        if fullname != seam.module:
            return None
        self.busy = True
        try:
            spec = importlib.util.find_spec(fullname)
        finally:
            self.busy = False
        if spec is None or spec.loader is None:
            return None
        loader, finder = spec.loader, self

        class _Loader(importlib.abc.Loader):
            def create_module(self, s):
                return loader.create_module(s)

            def exec_module(self, module):
                loader.exec_module(module)
                finder._done(module)

        spec.loader = _Loader()
        return spec


class _RegistrySeam(_Seam):
    """The seam on the reference's decoder registry: the patched thing is the dict entry DECODERS[REGISTRY_KEY] of `module`, and
    the options are those of make_decoder_class."""

    def __init__(self, keyword, module, key):
        super().__init__(keyword, module, (key,), (), {})

    def ready(self, mod) -> bool:
        return isinstance(getattr(mod, "DECODERS", None), dict) and self.names[0] in mod.DECODERS

    def patch(self, mod) -> dict:
        """Register a fused class built with the latest options from the reference's own class, which stays reachable as
        `.replaced` however often the registry is patched."""
        key = self.names[0]
        cur = mod.DECODERS.get(key)
        base = importlib.import_module(self.module + ".decoder")
        cls = make_decoder_class(base.Decoder, base.DecoderOutput, **self.options)
        cls.replaced = getattr(cur, "replaced", None) or cur
        mod.DECODERS[key] = cls
        return {key: cls}

    def restore(self) -> None:
        mod = sys.modules.get(self.module)
        cur = mod.DECODERS[self.names[0]] if self.ready(mod) else None
        if getattr(cur, "replaced", None) is not None:
            mod.DECODERS[self.names[0]] = cur.replaced


DECODER_SEAM = _RegistrySeam("lazy", REGISTRY_MODULE, REGISTRY_KEY)


def _native_adapter(replaced, mod, **aopts):
    """The class the reference's encoder instantiates (encoder_costvolume.py:185) on the lazy-field path of lazy.py: a subclass of
    the replaced class that returns the defining module's own adapter-side container."""
    from . import lazy as _lz
    cls = _lz.make_adapter_class(replaced, getattr(mod, "Gaussians", None), **aopts)
    cls.replaced = replaced
    return cls


ADAPTER_SEAM = _Seam("adapter", ADAPTER_MODULE, (ADAPTER_NAME,), ADAPTER_USERS, {ADAPTER_NAME: _native_adapter}, context=True)


METRICS_MODULE = "src.evaluation.metrics"                              # defines compute_ssim (:38-54)
METRICS_USERS = ("src.model.model_wrapper_erp",                        # `from ..evaluation.metrics import ... compute_ssim` (:18)
                 "src.model.model_wrapper_cubemaps",                   # (:19)
                 "src.evaluation.metric_computer")                     # (:12)
METRICS_NAME = "compute_ssim"


def _native_compute_ssim(replaced):
    """compute_ssim with the reference's signature: the SSIM kernel for GPU tensors, the replaced function otherwise."""
    from . import metrics as _metrics

    def compute_ssim(ground_truth, predicted):
        if ground_truth.is_cuda and predicted.is_cuda:
            return _metrics.compute_ssim(ground_truth, predicted)
        return replaced(ground_truth, predicted)

    compute_ssim.replaced = replaced
    compute_ssim.__doc__ = _metrics.compute_ssim.__doc__
    return compute_ssim


DEPTH_MODULE = "src.model.model_wrapper_helper"                       # defines erode (:4-24) and compute_l1_sphere_loss (:63-90)
DEPTH_USERS = ("src.model.model_wrapper_erp",)                         # `from .model_wrapper_helper import compute_l1_sphere_loss, erode` (:45)
DEPTH_NAMES = ("compute_l1_sphere_loss", "erode")


def _is_cuda_f32(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def _native_l1_sphere_loss(replaced):
    """compute_l1_sphere_loss with the reference's signature: the depth-loss kernels for float32 GPU tensors of one [B,V,H,W]
    shape with a mask that takes no gradient, the replaced function otherwise (mask=None included: it raises there)."""
    from . import depth_loss as _dl

    def compute_l1_sphere_loss(y_pred, y_true, mask=None, keep_batch=False):
        if (mask is not None and all(_is_cuda_f32(t) for t in (y_pred, y_true, mask)) and y_pred.dim() == 4
                and y_true.shape == y_pred.shape and mask.shape == y_pred.shape and not mask.requires_grad
                and y_pred.numel() > 0 and y_pred.device == y_true.device == mask.device):
            return _dl.compute_l1_sphere_loss(y_pred, y_true, mask, keep_batch)
        return replaced(y_pred, y_true, mask=mask, keep_batch=keep_batch)

    compute_l1_sphere_loss.replaced = replaced
    compute_l1_sphere_loss.__doc__ = _dl.compute_l1_sphere_loss.__doc__
    return compute_l1_sphere_loss


def _native_erode(replaced):
    """erode with the reference's signature: the erosion kernel for [C,H,W] / [N,C,H,W] float32 GPU tensors that take no gradient,
    an odd ksize and a reflect pad below H and W; the replaced function otherwise."""
    from . import depth_loss as _dl

    def erode(bin_img, ksize=5):
        if (_is_cuda_f32(bin_img) and bin_img.dim() in (3, 4) and not bin_img.requires_grad and isinstance(ksize, int)
                and ksize >= 1 and ksize % 2 == 1 and (ksize - 1) // 2 < min(bin_img.shape[-2], bin_img.shape[-1])):
            return _dl.erode(bin_img, ksize)
        return replaced(bin_img, ksize)

    erode.replaced = replaced
    erode.__doc__ = _dl.erode.__doc__
    return erode


_DEPTH_WRAPPERS = {"compute_l1_sphere_loss": _native_l1_sphere_loss, "erode": _native_erode}
DEPTH_LOSS_SEAM = _Seam("depth_loss", DEPTH_MODULE, DEPTH_NAMES, DEPTH_USERS, _DEPTH_WRAPPERS)


DEPTH_METRICS_MODULE = "src.scripts.compute_depth_metrics"            # defines compute_depth_metrics_batched (:47-116)
DEPTH_METRICS_USERS = ("src.model.model_wrapper_erp",)                 # `from ..scripts.compute_depth_metrics import compute_depth_metrics_batched` (:47)
DEPTH_METRICS_NAME = "compute_depth_metrics_batched"
PSNR_NAME = "compute_psnr"                                            # src/evaluation/metrics.py:11-21; METRICS_USERS bind it too


def _native_depth_metrics(replaced):
    """compute_depth_metrics_batched with the reference's signature: the depth-metrics kernels for float32 GPU gt / pred of one
    [B,N] shape with a bool mask on the same device, the replaced function otherwise."""
    from . import metrics as _metrics

    def compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a=False):
        if (_is_cuda_f32(gt_bN) and _is_cuda_f32(pred_bN) and isinstance(valid_masks_bN, torch.Tensor) and valid_masks_bN.is_cuda
                and valid_masks_bN.dtype == torch.bool and gt_bN.dim() == 2 and gt_bN.shape == pred_bN.shape == valid_masks_bN.shape
                and gt_bN.device == pred_bN.device == valid_masks_bN.device):
            return _metrics.compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a)
        return replaced(gt_bN, pred_bN, valid_masks_bN, mult_a)

    compute_depth_metrics_batched.replaced = replaced
    compute_depth_metrics_batched.__doc__ = _metrics.compute_depth_metrics_batched.__doc__
    return compute_depth_metrics_batched


def _native_compute_psnr(replaced):
    """compute_psnr with the reference's signature: the PSNR kernels for GPU float tensors of one 4-D shape on one device, the
    replaced function otherwise."""
    from . import metrics as _metrics

    def compute_psnr(ground_truth, predicted):
        if (isinstance(ground_truth, torch.Tensor) and isinstance(predicted, torch.Tensor) and ground_truth.is_cuda and predicted.is_cuda
                and ground_truth.is_floating_point() and predicted.is_floating_point() and ground_truth.dim() == 4
                and ground_truth.shape == predicted.shape and ground_truth.device == predicted.device):
            return _metrics.compute_psnr(ground_truth, predicted)
        return replaced(ground_truth, predicted)

    compute_psnr.replaced = replaced
    compute_psnr.__doc__ = _metrics.compute_psnr.__doc__
    return compute_psnr


DEPTH_METRICS_SEAM = _Seam("depth_metrics", DEPTH_METRICS_MODULE, (DEPTH_METRICS_NAME,), DEPTH_METRICS_USERS,
                           {DEPTH_METRICS_NAME: _native_depth_metrics})
SSIM_SEAM = _Seam("metrics", METRICS_MODULE, (METRICS_NAME,), METRICS_USERS, {METRICS_NAME: _native_compute_ssim})
PSNR_SEAM = _Seam("psnr", METRICS_MODULE, (PSNR_NAME,), METRICS_USERS, {PSNR_NAME: _native_compute_psnr})


ERP_DISTANCE_MODULE = "src.geometry.z_depth_to_distance"              # defines depth_to_distance_map_batch (:4-34)
ERP_DISTANCE_USERS = ("src.model.model_wrapper_erp",)                  # `from ..geometry.z_depth_to_distance import depth_to_distance_map_batch` (:48)
ERP_DISTANCE_NAME = "depth_to_distance_map_batch"


def _native_depth_to_distance(replaced):
    """depth_to_distance_map_batch with the reference's signature: the z-depth -> distance kernel (convention "reference") for
    float32 GPU depth maps [N, h, h] with fxfycxcy a float32 [N, 4, h, h] tensor on the same device whose last two strides are 0 —
    what the reference's einops.repeat of the [N, 4] rows yields (model_wrapper_erp.py:454-455), so one row per map is the whole
    content; the replaced function otherwise."""
    from . import stitch as _st

    def depth_to_distance_map_batch(depth_maps, fxfycxcy):
        if (_is_cuda_f32(depth_maps) and _is_cuda_f32(fxfycxcy) and depth_maps.dim() == 3 and depth_maps.numel() > 0
                and depth_maps.shape[1] == depth_maps.shape[2] and fxfycxcy.device == depth_maps.device
                and tuple(fxfycxcy.shape) == (depth_maps.shape[0], 4, depth_maps.shape[1], depth_maps.shape[2])
                and tuple(fxfycxcy.stride()[2:]) == (0, 0)):
            return _st.depth_to_distance(depth_maps, fxfycxcy[:, :, 0, 0], "reference")
        return replaced(depth_maps, fxfycxcy)

    depth_to_distance_map_batch.replaced = replaced
    depth_to_distance_map_batch.__doc__ = _st.depth_to_distance.__doc__
    return depth_to_distance_map_batch


ERP_DISTANCE_SEAM = _Seam("erp_distance", ERP_DISTANCE_MODULE, (ERP_DISTANCE_NAME,), ERP_DISTANCE_USERS,
                          {ERP_DISTANCE_NAME: _native_depth_to_distance})


VIS_DEPTH_MODULE = "src.model.model_wrapper_erp"                      # defines depth_map (:122-133) and calls it as a global
VIS_DEPTH_NAME = "depth_map"
VIS_PREP_MODULE = "src.misc.image_io"                                 # defines prep_image (:38-54); save_image / save_video call it as a global
VIS_PREP_USERS = ("src.model.model_wrapper_erp", "src.model.model_wrapper_cubemaps")   # `from ..misc.image_io import prep_image, ...` (:22, :23)
VIS_PREP_NAME = "prep_image"
VIS_COLOR_MODULE = "src.visualization.color_map"                      # defines apply_color_map (:9-19); apply_color_map_to_image calls it as a global
VIS_COLOR_USERS = ("src.model.encoder.visualization.encoder_visualizer_costvolume",)   # binds apply_color_map by name (:15)
VIS_COLOR_NAME = "apply_color_map"


def _native_depth_map(replaced):
    """depth_map with the reference's signature: the depth colour-map kernels for a float32 GPU tensor of at least two dims and
    at most 16 000 000 elements -> float32 [..., 3, h, w] on the device; the reference normalises over the WHOLE argument, so a
    [lead, h, w] argument is one map of lead h w elements (visualize.depth_map_whole).  The replaced function otherwise."""
    from . import visualize as _vis

    def depth_map(result):
        if _is_cuda_f32(result) and result.dim() >= 2 and 0 < result.numel() <= _vis.MAX_MAP_ELEMENTS:
            return _vis.depth_map_whole(result)
        return replaced(result)

    depth_map.replaced = replaced
    depth_map.__doc__ = _vis.depth_map_whole.__doc__
    return depth_map


def _native_prep_image(replaced):
    """prep_image with the reference's signature: for a float32 GPU tensor [h, w], [c, h, w] or [b, c, h, w] with c in
    {1, 3, 4} the frame is made on the device and crosses the bus as bytes (visualize.prep_image(...).cpu().numpy(), the
    uint8 [h, b w, c] array save_image / save_video consume); the replaced function otherwise."""
    from . import visualize as _vis

    def prep_image(image):
        if (_is_cuda_f32(image) and image.dim() in (2, 3, 4) and image.numel() > 0
                and (image.dim() == 2 or image.shape[-3] in (1, 3, 4))):
            return _vis.prep_image(image).cpu().numpy()
        return replaced(image)

    prep_image.replaced = replaced
    prep_image.__doc__ = _vis.prep_image.__doc__
    return prep_image


def _native_apply_color_map(replaced):
    """apply_color_map with the reference's signature: the colour-table kernel for a float32 GPU tensor and one of the tables
    turbo, viridis, inferno -> float32 [..., 3] on the device; the replaced function otherwise (CPU, other dtypes, any other
    matplotlib map)."""
    from . import visualize as _vis

    def apply_color_map(x, color_map="inferno"):
        if _is_cuda_f32(x) and x.numel() > 0 and isinstance(color_map, str) and color_map in _vis.COLOR_MAPS:
            return _vis.colorize(x, color_map)
        return replaced(x, color_map)

    apply_color_map.replaced = replaced
    apply_color_map.__doc__ = _vis.colorize.__doc__
    return apply_color_map


VIS_DEPTH_SEAM = _Seam("visualization", VIS_DEPTH_MODULE, (VIS_DEPTH_NAME,), (), {VIS_DEPTH_NAME: _native_depth_map})
VIS_PREP_SEAM = _Seam("visualization", VIS_PREP_MODULE, (VIS_PREP_NAME,), VIS_PREP_USERS, {VIS_PREP_NAME: _native_prep_image})
VIS_COLOR_SEAM = _Seam("visualization", VIS_COLOR_MODULE, (VIS_COLOR_NAME,), VIS_COLOR_USERS, {VIS_COLOR_NAME: _native_apply_color_map})
VIS_SEAMS = (VIS_DEPTH_SEAM, VIS_PREP_SEAM, VIS_COLOR_SEAM)


COST_VOLUME_MODULE = "src.model.encoder.costvolume.depth_predictor_multiview_360"   # defines warp_with_pose_depth_candidates (:73-214)
COST_VOLUME_NAME = "warp_with_pose_depth_candidates"                  # DepthPredictorMultiView360.forward calls the module-level name (:606)
COST_VOLUME_DATASETS = ("hm3d", "replica")


def _native_cost_volume_warp(replaced):
    """warp_with_pose_depth_candidates with the reference's signature: for float32 GPU features, pose and candidates of the
    'hm3d' / 'replica' convention with zeros padding it returns a cost_volume.LazyWarp, whose product with feat01.unsqueeze(2)
    summed over dim 1 is the fused kernel (DepthPredictorMultiView360.forward :621-625 then divides, stacks and averages
    [v b, D, h, w] tensors unchanged); the replaced function otherwise.  With wo_cost_volume the reference never calls it."""
    from . import cost_volume as _cv

    def warp_with_pose_depth_candidates(utils360, feature1, pose, depth, *args, **kwargs):
        if (not args and all(_is_cuda_f32(t) for t in (feature1, pose, depth)) and feature1.device == pose.device == depth.device
                and getattr(utils360, "dataset", None) in COST_VOLUME_DATASETS and feature1.dim() == 4 and depth.dim() == 4
                and tuple(pose.shape) == (feature1.shape[0], 4, 4) and depth.shape[0] == feature1.shape[0]
                and tuple(depth.shape[2:]) == tuple(feature1.shape[2:]) and feature1.numel() > 0
                and kwargs.get("warp_padding_mode", "zeros") == "zeros" and not kwargs.get("debug", False)):
            return _cv.LazyWarp(utils360, feature1, pose, depth, replaced, kwargs)
        return replaced(utils360, feature1, pose, depth, *args, **kwargs)

    warp_with_pose_depth_candidates.replaced = replaced
    warp_with_pose_depth_candidates.__doc__ = _cv.LazyWarp.__doc__
    return warp_with_pose_depth_candidates


COST_VOLUME_SEAM = _Seam("cost_volume", COST_VOLUME_MODULE, (COST_VOLUME_NAME,), (), {COST_VOLUME_NAME: _native_cost_volume_warp})


DEPTH_HEAD_NAME = "F"                                                 # `import torch.nn.functional as F` (:5); F.softmax at :643


def _native_functional(replaced):
    """The proxy for the predictor module's `F`: softmax(x, dim=1) of a 4-D float32 GPU tensor returns a depth_head.LazyPdf, whose
    product with the [v b, D, 1, 1] candidates summed over dim 1 and whose torch.max over dim 1 (both keepdim=True,
    DepthPredictorMultiView360.forward :646-651) are one run of the fused kernel; every other call of softmax (another dim or
    dtype, CPU, extra arguments) and every other attribute (interpolate, grid_sample, ...) is the replaced module's own."""
    from . import depth_head as _dh
    return _dh.FunctionalProxy(replaced)


class _LayerSeam(_Seam):
    """A seam on a name that two options share (the predictor module's `F`): each option wraps whatever is bound in a proxy of
    its own class, whose `.replaced` is what it wrapped, so the proxies stack in either order of installation.  patch() adds this
    seam's layer unless the stack holds one already; restore() takes this seam's layer out of the stack wherever it sits."""

    def __init__(self, keyword, module, name, wrapper, layer_type):
        super().__init__(keyword, module, (name,), (), {name: wrapper})
        self.layer_type = layer_type                              # () -> the proxy's class (imported on demand)

    def _layers(self, mod):
        cur = getattr(mod, self.names[0], None)
        while getattr(cur, "replaced", None) is not None:
            yield cur
            cur = cur.replaced

    def patch(self, mod) -> dict:
        name = self.names[0]
        if not any(type(layer) is self.layer_type() for layer in self._layers(mod)):
            setattr(mod, name, self.wrappers[name](getattr(mod, name)))
        return {name: getattr(mod, name)}

    def restore(self) -> None:
        mod = sys.modules.get(self.module)
        if mod is None:
            return
        name, above = self.names[0], None
        for layer in list(self._layers(mod)):
            if type(layer) is self.layer_type():
                if above is None:
                    setattr(mod, name, layer.replaced)
                else:
                    above.replaced = layer.replaced
            else:
                above = layer


def _depth_head_layer():
    from . import depth_head as _dh
    return _dh.FunctionalProxy


DEPTH_HEAD_SEAM = _LayerSeam("depth_head", COST_VOLUME_MODULE, DEPTH_HEAD_NAME, _native_functional, _depth_head_layer)


DEPTH_TAIL_MODULE = "src.model.encoder.encoder_costvolume"            # defines EncoderCostVolume (:228-241 map_pdf_to_opacity, used at :420)
DEPTH_TAIL_CLASS = "EncoderCostVolume"
DEPTH_TAIL_METHOD = "map_pdf_to_opacity"


def _native_interpolate(replaced):
    """The proxy for the predictor module's `F` whose interpolate runs depth_tail.upsample for the predictor's two calls
    (:652-658: a float32 GPU [v b, 1, h, w] map, an integer scale_factor, nearest or bilinear with align_corners=True) and the
    replaced interpolate for every other call; every other attribute is the replaced object's own."""
    from . import depth_tail as _dt
    return _dt.InterpolateProxy(replaced)


def _depth_tail_layer():
    from . import depth_tail as _dt
    return _dt.InterpolateProxy


def _native_map_pdf_to_opacity(replaced):
    """EncoderCostVolume.map_pdf_to_opacity with the reference's signature: the exponent from self.cfg.opacity_mapping exactly as
    the method computes it, then the opacity-map kernel for a float32 GPU pdf; the replaced method otherwise."""
    from . import depth_tail as _dt

    def map_pdf_to_opacity(self, pdf, global_step):
        if _is_cuda_f32(pdf) and pdf.numel() > 0:
            cfg = self.cfg.opacity_mapping
            return _dt.map_pdf_to_opacity(pdf, _dt.opacity_exponent(cfg.initial, cfg.final, cfg.warm_up, global_step))
        return replaced(self, pdf, global_step)

    map_pdf_to_opacity.replaced = replaced
    map_pdf_to_opacity.__doc__ = _dt.map_pdf_to_opacity.__doc__
    return map_pdf_to_opacity


class _MethodSeam(_Seam):
    """A seam on a method: `names` are attributes of the class `cls_name` that `module` defines.  context=True: as in _Seam, the
    wrapper takes the defining module and the seam's options."""

    def __init__(self, keyword, module, cls_name, names, wrappers, context=False):
        super().__init__(keyword, module, names, (), wrappers, context)
        self.cls_name = cls_name

    def ready(self, mod) -> bool:
        cls = getattr(mod, self.cls_name, None) if mod is not None else None
        return cls is not None and all(hasattr(cls, n) for n in self.names)

    def patch(self, mod) -> dict:
        cls, out = getattr(mod, self.cls_name), {}
        for name in self.names:
            cur = cls.__dict__.get(name, getattr(cls, name))
            if getattr(cur, "replaced", None) is not None:
                out[name] = cur
            else:
                out[name] = self.wrappers[name](cur, mod, **self.options) if self.context else self.wrappers[name](cur)
            setattr(cls, name, out[name])
        return out

    def restore(self) -> None:
        cls = getattr(sys.modules.get(self.module), self.cls_name, None)
        for name in self.names if cls is not None else ():
            cur = cls.__dict__.get(name)
            if getattr(cur, "replaced", None) is not None:
                setattr(cls, name, cur.replaced)


DEPTH_TAIL_F_SEAM = _LayerSeam("depth_tail", COST_VOLUME_MODULE, DEPTH_HEAD_NAME, _native_interpolate, _depth_tail_layer)
DEPTH_TAIL_METHOD_SEAM = _MethodSeam("depth_tail", DEPTH_TAIL_MODULE, DEPTH_TAIL_CLASS, (DEPTH_TAIL_METHOD,),
                                     {DEPTH_TAIL_METHOD: _native_map_pdf_to_opacity})


DEPTH_SMOOTH_MODULE = "src.loss.loss_depth"                          # defines LossDepth (:26-60)
DEPTH_SMOOTH_CLASS = "LossDepth"
DEPTH_SMOOTH_METHOD = "forward"


def _native_depth_smooth_call(cfg, prediction, batch):
    """The arguments of depth_smooth.depth_smoothness_loss for a LossDepth.forward call the kernels can take, else None:
    prediction.depth a float32 CUDA [B,V,H,W] tensor with H, W above the derivative order; batch["target"]["near"] / ["far"]
    float32 CUDA [B,Vn] on the same device with Vn in {1, V} (the shapes the reference's own broadcast accepts); with
    cfg.sigma_image not None, batch["target"]["image"] a float32 CUDA [B,V,C,H,W] tensor on that device that takes no gradient.
    The decision reads only configuration, devices, dtypes and shapes."""
    try:
        depth, target = prediction.depth, batch["target"]
        near, far = target["near"], target["far"]
        sigma, second, weight = cfg.sigma_image, bool(cfg.use_second_derivative), cfg.weight
        image = target["image"] if sigma is not None else None
    except (AttributeError, KeyError, TypeError):
        return None
    order = 2 if second else 1
    if not (_is_cuda_f32(depth) and depth.dim() == 4 and depth.numel() > 0 and min(depth.shape[2:]) > order):
        return None
    b, v, h, w = depth.shape
    if not (_is_cuda_f32(near) and _is_cuda_f32(far) and near.dim() == 2 and near.shape == far.shape and near.shape[0] == b
            and near.shape[1] in (1, v) and near.device == far.device == depth.device):
        return None
    if sigma is not None:
        if not (isinstance(sigma, (int, float)) and _is_cuda_f32(image) and image.dim() == 5 and image.shape[2] >= 1
                and (image.shape[0], image.shape[1], image.shape[3], image.shape[4]) == (b, v, h, w)
                and image.device == depth.device and not image.requires_grad):
            return None
    if not isinstance(weight, (int, float)):
        return None
    return (depth, near, far, image), dict(sigma_image=sigma, use_second_derivative=second, weight=weight)


def _native_loss_depth_forward(replaced):
    """LossDepth.forward with the reference's signature: the depth-smoothness kernels of depth_smooth.py for the calls
    _native_depth_smooth_call accepts, the replaced method otherwise (so every error the reference raises is still raised)."""
    from . import depth_smooth as _ds

    def forward(self, prediction, batch, gaussians, global_step):
        call = _native_depth_smooth_call(self.cfg, prediction, batch)
        if call is not None:
            return _ds.depth_smoothness_loss(*call[0], **call[1])
        return replaced(self, prediction, batch, gaussians, global_step)

    forward.replaced = replaced
    forward.__doc__ = _ds.depth_smoothness_loss.__doc__
    return forward


DEPTH_SMOOTH_SEAM = _MethodSeam("depth_smoothness", DEPTH_SMOOTH_MODULE, DEPTH_SMOOTH_CLASS, (DEPTH_SMOOTH_METHOD,),
                                {DEPTH_SMOOTH_METHOD: _native_loss_depth_forward})


WINDOW_ATTENTION_MODULE = "src.model.encoder.backbone.multiview_transformer"   # defines the attention functions (:8-289)
WINDOW_ATTENTION_SPLIT = "single_head_split_window_attention"         # :60-210; TransformerLayer.forward reads the module globals (:358-405)
WINDOW_ATTENTION_FULL = "single_head_full_attention"                  # :8-16
WINDOW_ATTENTION_MASK = "generate_shift_window_attn_mask"             # :19-57, called once per backbone forward (:597)
WINDOW_ATTENTION_MULTI = "multi_head_split_window_attention"          # :213-289: takes attn_mask, stays torch
WINDOW_ATTENTION_NAMES = (WINDOW_ATTENTION_SPLIT, WINDOW_ATTENTION_FULL, WINDOW_ATTENTION_MASK, WINDOW_ATTENTION_MULTI)


def _window_attention_call(q, k, v, h, w, num_splits) -> bool:
    """True if the window-attention kernels take the call: q [B, L, C] and k, v of one shape [B, L, C] or [B, m, L, C], all
    float32 CUDA tensors on one device, L = h w, num_splits dividing h and w, a supported C.  Reads devices, dtypes and shapes."""
    from . import window_attention as _wa
    if not all(_is_cuda_f32(t) for t in (q, k, v)) or not (q.device == k.device == v.device):
        return False
    if q.dim() != 3 or k.dim() not in (3, 4) or tuple(k.shape) != tuple(v.shape) or q.numel() == 0 or k.numel() == 0:
        return False
    if (k.shape[0], k.shape[-2], k.shape[-1]) != tuple(q.shape) or not _wa.supported_channels(int(q.shape[2])):
        return False
    if not all(isinstance(x, int) and not isinstance(x, bool) for x in (h, w, num_splits)):
        return False
    return h >= 1 and w >= 1 and num_splits >= 1 and h * w == q.shape[1] and h % num_splits == 0 and w % num_splits == 0


def _dense_mask(attn_mask):
    """What torch code may see of a mask argument: a ShiftMask handle's dense tensor, anything else as it is."""
    from . import window_attention as _wa
    return attn_mask.dense() if isinstance(attn_mask, _wa.ShiftMask) else attn_mask


def _native_split_window_attention(replaced, mod=None, precision="highest"):
    """single_head_split_window_attention with the reference's signature: the fused kernels for float32 GPU q, k, v of agreeing
    shapes and a supported C — with_shift only with the ShiftMask handle of this grid and split (or without a mask argument the
    reference would refuse anyway); the replaced function otherwise, with a handle made dense first.  precision: the seam's
    option, "torch" resolved per call."""
    from . import window_attention as _wa
    _precision.seam_option("window_attention_precision", precision)

    def single_head_split_window_attention(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None):
        if _window_attention_call(q, k, v, h, w, num_splits) and (
                not with_shift or (isinstance(attn_mask, _wa.ShiftMask) and attn_mask.matches(h, w, num_splits))):
            return _wa.window_attention(q, k, v, height=h, width=w, num_splits=num_splits, with_shift=bool(with_shift),
                                        precision=_precision.resolve(precision))
        return replaced(q, k, v, num_splits=num_splits, with_shift=with_shift, h=h, w=w, attn_mask=_dense_mask(attn_mask))

    single_head_split_window_attention.replaced = replaced
    single_head_split_window_attention.precision = precision
    single_head_split_window_attention.__doc__ = _wa.window_attention.__doc__
    return single_head_split_window_attention


def _native_full_attention(replaced, mod=None, precision="highest"):
    """single_head_full_attention with the reference's signature: the fused kernels (one window, no shift) for float32 GPU
    q, k, v [B, L, C] of one shape and a supported C; the replaced function otherwise.  precision: as above."""
    from . import window_attention as _wa
    _precision.seam_option("window_attention_precision", precision)

    def single_head_full_attention(q, k, v):
        if (all(_is_cuda_f32(t) for t in (q, k, v)) and q.dim() == 3 and tuple(q.shape) == tuple(k.shape)
                and _window_attention_call(q, k, v, 1, int(q.shape[1]), 1)):
            return _wa.full_attention(q, k, v, precision=_precision.resolve(precision))
        return replaced(q, k, v)

    single_head_full_attention.replaced = replaced
    single_head_full_attention.precision = precision
    single_head_full_attention.__doc__ = _wa.full_attention.__doc__
    return single_head_full_attention


def _native_shift_mask(replaced, mod=None, **_):
    """generate_shift_window_attn_mask with the reference's signature: returns a window_attention.ShiftMask — the arguments and
    no [K^2, Lw, Lw] tensor; its dense() calls the replaced generator, for the torch paths only."""
    from . import window_attention as _wa

    def generate_shift_window_attn_mask(input_resolution, window_size_h, window_size_w, shift_size_h, shift_size_w,
                                        device=torch.device("cuda")):
        h, w = input_resolution
        return _wa.ShiftMask(h, w, window_size_h, window_size_w, shift_size_h, shift_size_w, device,
                             build=lambda: replaced(input_resolution, window_size_h, window_size_w, shift_size_h, shift_size_w,
                                                    device=device))

    generate_shift_window_attn_mask.replaced = replaced
    generate_shift_window_attn_mask.__doc__ = _wa.ShiftMask.__doc__
    return generate_shift_window_attn_mask


def _native_multi_head_attention(replaced, mod=None, **_):
    """multi_head_split_window_attention stays the reference's torch code; the wrapper only makes a ShiftMask handle dense, so
    that a handle never reaches torch."""
    import functools

    @functools.wraps(replaced)
    def multi_head_split_window_attention(q, k, v, num_splits=1, with_shift=False, h=None, w=None, attn_mask=None, num_head=1):
        return replaced(q, k, v, num_splits=num_splits, with_shift=with_shift, h=h, w=w, attn_mask=_dense_mask(attn_mask),
                        num_head=num_head)

    multi_head_split_window_attention.replaced = replaced
    return multi_head_split_window_attention


WINDOW_ATTENTION_SEAM = _Seam("window_attention", WINDOW_ATTENTION_MODULE, WINDOW_ATTENTION_NAMES, (),
                              {WINDOW_ATTENTION_SPLIT: _native_split_window_attention, WINDOW_ATTENTION_FULL: _native_full_attention,
                               WINDOW_ATTENTION_MASK: _native_shift_mask, WINDOW_ATTENTION_MULTI: _native_multi_head_attention},
                              context=True)


GROUP_NORM_UNET_MODULE = "src.model.encoder.costvolume.ldm_unet.unet"   # defines ResBlock (:176-307) and AttentionBlock (:310-380)
GROUP_NORM_RESBLOCK = "ResBlock"
GROUP_NORM_ATTENTION = "AttentionBlock"
GROUP_NORM_UNET_METHOD = "_forward"                                   # both forwards reach it through util.checkpoint, looked up per call
GROUP_NORM_PREDICTOR_CLASS = "DepthPredictorMultiView360"             # COST_VOLUME_MODULE :405-520 builds the two U-Nets' heads
GROUP_NORM_PREDICTOR_METHOD = "__init__"
GROUP_NORM_PREDICTOR_NETS = ("corr_refine_net", "refine_unet")        # :424-444, :479-497: Conv2d -> nn.GroupNorm -> GELU -> UNetModel
GROUP_NORM_BACKBONE_MODULE = "src.model.encoder.backbone.unimatch.backbone"   # defines ResidualBlock (:6-36)
GROUP_NORM_RESIDUAL = "ResidualBlock"
GROUP_NORM_BACKBONE_METHOD = "forward"


def _norm_pair(layers):
    """(conv, norm) if `layers` is the postnorm ResBlock's nn.Sequential(conv, GroupNorm, SiLU) — or what group_norm.fuse_pairs
    makes of it, (conv, FusedGroupNormAct with silu, Identity) — else None."""
    from . import group_norm as _gn
    nn = torch.nn
    if not isinstance(layers, nn.Sequential) or len(layers) != 3 or not isinstance(layers[1], nn.GroupNorm) or isinstance(layers[0], nn.GroupNorm):
        return None
    if isinstance(layers[1], _gn.FusedGroupNormAct):
        ok = (layers[1].activation == "silu" and isinstance(layers[2], nn.Identity)) or \
             (layers[1].activation == "none" and isinstance(layers[2], nn.SiLU))
    else:
        ok = isinstance(layers[2], nn.SiLU)
    return (layers[0], layers[1]) if ok else None


def _native_resblock_forward(replaced):
    """ResBlock._forward with the reference's signature: for a block without up / down sampling whose in_layers and out_layers are
    (conv, GroupNorm, SiLU), h = gn_silu(conv(x)) and skip_connection(x) + gn_silu(conv(h)) with the add inside the second
    kernel; the replaced method otherwise (prenorm, updown).  group_norm.norm_act runs the kernels for contiguous float32 GPU
    tensors and the block's own modules for everything else."""
    from . import group_norm as _gn

    def _forward(self, x, emb=None):
        first = _norm_pair(getattr(self, "in_layers", None)) if not getattr(self, "updown", True) else None
        second = _norm_pair(getattr(self, "out_layers", None)) if first is not None else None
        if second is None:
            return replaced(self, x, emb)
        h = _gn.norm_act(first[1], first[0](x), "silu")
        return _gn.norm_act(second[1], second[0](h), "silu", residual=self.skip_connection(x))

    _forward.replaced = replaced
    _forward.__doc__ = _gn.group_norm_act.__doc__
    return _forward


def _native_attention_block_forward(replaced):
    """AttentionBlock._forward with the reference's signature: for a postnorm block, x + norm(proj_out(attention(qkv(x)))) with
    the norm and the add as one kernel (activation none, residual x); qkv, attention and proj_out are the module's own.  The
    replaced method otherwise (prenorm)."""
    from . import group_norm as _gn

    def _forward(self, x):
        if not getattr(self, "postnorm", False) or not isinstance(getattr(self, "norm", None), torch.nn.GroupNorm) or x.dim() < 2:
            return replaced(self, x)
        b, c, *spatial = x.shape
        x = x.reshape(b, c, -1)
        h = self.proj_out(self.attention(self.qkv(x)))
        return _gn.norm_act(self.norm, h, "none", residual=x).reshape(b, c, *spatial)

    _forward.replaced = replaced
    _forward.__doc__ = _gn.group_norm_act.__doc__
    return _forward


def _native_predictor_init(replaced):
    """DepthPredictorMultiView360.__init__ with the reference's signature: the replaced constructor, then group_norm.fuse_pairs on
    corr_refine_net and refine_unet where they are nn.Sequential (the ablations build a bare Conv2d): Conv2d -> nn.GroupNorm ->
    GELU becomes Conv2d -> FusedGroupNormAct -> Identity with the same Parameter objects at the same indices, so the reference's
    checkpoints load unchanged."""
    import functools

    from . import group_norm as _gn

    @functools.wraps(replaced)
    def __init__(self, *args, **kwargs):
        replaced(self, *args, **kwargs)
        for name in GROUP_NORM_PREDICTOR_NETS:
            net = getattr(self, name, None)
            if isinstance(net, torch.nn.Sequential):
                _gn.fuse_pairs(net)

    __init__.replaced = replaced
    return __init__


def _native_residual_block_forward(replaced):
    """ResidualBlock.forward with the reference's signature: for norm1 and norm2 an nn.InstanceNorm2d without affine and without
    running statistics and a 4-D input, y = in_relu(conv1(x)), y = in_relu(conv2(y)) with the instance norm and the ReLU as one
    kernel; the downsample branch and the final relu(x + y) stay torch.  The replaced method otherwise (BatchNorm, affine)."""
    from . import group_norm as _gn

    def plain(norm) -> bool:
        return isinstance(norm, torch.nn.InstanceNorm2d) and not norm.affine and not norm.track_running_stats

    def forward(self, x):
        if not (plain(getattr(self, "norm1", None)) and plain(getattr(self, "norm2", None)) and isinstance(x, torch.Tensor) and x.dim() == 4):
            return replaced(self, x)
        y = _gn.norm_act(self.norm1, self.conv1(x), "relu")
        y = _gn.norm_act(self.norm2, self.conv2(y), "relu")
        if self.downsample is not None:
            x = self.downsample(x)
        return self.relu(x + y)

    forward.replaced = replaced
    forward.__doc__ = _gn.instance_norm_act.__doc__
    return forward


GROUP_NORM_RESBLOCK_SEAM = _MethodSeam("group_norm", GROUP_NORM_UNET_MODULE, GROUP_NORM_RESBLOCK, (GROUP_NORM_UNET_METHOD,),
                                       {GROUP_NORM_UNET_METHOD: _native_resblock_forward})
GROUP_NORM_ATTENTION_SEAM = _MethodSeam("group_norm", GROUP_NORM_UNET_MODULE, GROUP_NORM_ATTENTION, (GROUP_NORM_UNET_METHOD,),
                                        {GROUP_NORM_UNET_METHOD: _native_attention_block_forward})
GROUP_NORM_PREDICTOR_SEAM = _MethodSeam("group_norm", COST_VOLUME_MODULE, GROUP_NORM_PREDICTOR_CLASS, (GROUP_NORM_PREDICTOR_METHOD,),
                                        {GROUP_NORM_PREDICTOR_METHOD: _native_predictor_init})
GROUP_NORM_RESIDUAL_SEAM = _MethodSeam("group_norm", GROUP_NORM_BACKBONE_MODULE, GROUP_NORM_RESIDUAL, (GROUP_NORM_BACKBONE_METHOD,),
                                       {GROUP_NORM_BACKBONE_METHOD: _native_residual_block_forward})
GROUP_NORM_SEAMS = (GROUP_NORM_RESBLOCK_SEAM, GROUP_NORM_ATTENTION_SEAM, GROUP_NORM_PREDICTOR_SEAM, GROUP_NORM_RESIDUAL_SEAM)


UNET_ATTENTION_MODULE = GROUP_NORM_UNET_MODULE                        # defines QKVAttentionLegacy (:527-565) and QKVAttention (:572-599)
UNET_ATTENTION_LEGACY = "QKVAttentionLegacy"
UNET_ATTENTION_NEW = "QKVAttention"
UNET_ATTENTION_METHOD = "forward"                                     # AttentionBlock._forward calls self.attention(qkv) (:372, :377)


def _unet_attention_call(qkv, n_heads, views) -> bool:
    """True if the QKV-attention kernels take the call: qkv a float32 CUDA [N, heads 3 ch, T] tensor outside autocast, a supported
    ch, `views` dividing N.  Reads devices, dtypes and shapes."""
    from . import qkv_attention as _qa
    if not _is_cuda_f32(qkv) or qkv.dim() != 3 or qkv.numel() == 0 or torch.is_autocast_enabled():
        return False
    if not all(isinstance(x, int) and not isinstance(x, bool) and x >= 1 for x in (n_heads, views)):
        return False
    width = int(qkv.shape[1])
    return width % (3 * n_heads) == 0 and _qa.supported_head_channels(width // (3 * n_heads)) and qkv.shape[0] % views == 0


def _native_qkv_attention_forward(order):
    """QKVAttentionLegacy.forward (order "legacy": n_heads, n_frames, use_cross_view_self_attn of the module) or
    QKVAttention.forward (order "new": n_heads) with the reference's signature: the fused kernels of qkv_attention.py for the calls
    _unet_attention_call accepts, the replaced method otherwise (half precision, autocast, CPU, other ch — and every error the
    reference raises).  `forward.native_calls` counts the calls the kernels took.  precision: the seam's option, resolved at every
    call — the recomputation under the reference's checkpoint included; `forward.precision` holds it."""
    def wrapper(replaced, mod=None, precision="highest"):
        from . import qkv_attention as _qa
        _precision.seam_option("unet_attention_precision", precision)

        def forward(self, qkv):
            heads = getattr(self, "n_heads", None)
            cross = bool(getattr(self, "use_cross_view_self_attn", False)) if order == "legacy" else False
            frames = getattr(self, "n_frames", 1) if cross else 1
            if _unet_attention_call(qkv, heads, frames):
                forward.native_calls += 1
                return _qa.qkv_attention(qkv, heads, n_frames=frames, cross_view=cross, order=order,
                                         precision=_precision.resolve(precision))
            return replaced(self, qkv)

        forward.replaced = replaced
        forward.precision = precision
        forward.native_calls = 0
        forward.__doc__ = _qa.qkv_attention.__doc__
        return forward

    return wrapper


UNET_ATTENTION_LEGACY_SEAM = _MethodSeam("unet_attention", UNET_ATTENTION_MODULE, UNET_ATTENTION_LEGACY, (UNET_ATTENTION_METHOD,),
                                         {UNET_ATTENTION_METHOD: _native_qkv_attention_forward("legacy")}, context=True)
UNET_ATTENTION_NEW_SEAM = _MethodSeam("unet_attention", UNET_ATTENTION_MODULE, UNET_ATTENTION_NEW, (UNET_ATTENTION_METHOD,),
                                      {UNET_ATTENTION_METHOD: _native_qkv_attention_forward("new")}, context=True)
UNET_ATTENTION_SEAMS = (UNET_ATTENTION_LEGACY_SEAM, UNET_ATTENTION_NEW_SEAM)


TRANSFORMER_FFN_MODULE = WINDOW_ATTENTION_MODULE                      # defines TransformerLayer (:292-414)
TRANSFORMER_FFN_CLASS = "TransformerLayer"
TRANSFORMER_FFN_METHOD = "forward"


def _plain_linear(layer, n_in, n_out) -> bool:
    return type(layer) is torch.nn.Linear and layer.bias is None and (layer.in_features, layer.out_features) == (n_in, n_out)


def _affine_norm(norm, c) -> bool:
    return (type(norm) is torch.nn.LayerNorm and tuple(norm.normalized_shape) == (c,) and norm.elementwise_affine
            and norm.weight is not None and norm.bias is not None)


def _transformer_ffn_call(layer, source, target, kwargs) -> bool:
    """True if the wrapper takes the call: a single-head layer without per-view attention and without an attn_type keyword,
    float32 CUDA source [B, L, C] and target on one device outside autocast, d_model = C = 128, norm1 (and, with an FFN, norm2 of
    the same eps) a LayerNorm with affine parameters, and the mlp (Linear 2C -> 8C without bias, erf GELU, Linear 8C -> C without
    bias).  Reads attributes, devices, dtypes and shapes."""
    from . import transformer_ffn as _tf
    if "attn_type" in kwargs or getattr(layer, "nhead", None) != 1 or getattr(layer, "add_per_view_attn", True):
        return False
    if not (_is_cuda_f32(source) and _is_cuda_f32(target) and source.device == target.device) or torch.is_autocast_enabled():
        return False
    c = getattr(layer, "dim", None)
    if source.dim() != 3 or source.numel() == 0 or source.shape[-1] != c or not _tf.supported_widths(c, 8 * c):
        return False
    if not _affine_norm(getattr(layer, "norm1", None), c) or not all(_plain_linear(getattr(layer, n, None), c, c)
                                                                      for n in ("q_proj", "k_proj", "v_proj", "merge")):
        return False
    if getattr(layer, "no_ffn", None) is True:
        return True
    mlp = getattr(layer, "mlp", None)
    if layer.no_ffn is not False or not isinstance(mlp, torch.nn.Sequential) or len(mlp) != 3:
        return False
    if not (_plain_linear(mlp[0], 2 * c, 8 * c) and type(mlp[1]) is torch.nn.GELU and mlp[1].approximate == "none"
            and _plain_linear(mlp[2], 8 * c, c)):
        return False
    return _affine_norm(getattr(layer, "norm2", None), c) and layer.norm2.eps == layer.norm1.eps


def _native_transformer_layer_forward(replaced, mod=None, precision="highest"):
    """TransformerLayer.forward with the reference's signature: for the calls _transformer_ffn_call accepts, the layer's own
    q_proj / k_proj / v_proj, the attention function the replaced method would call — looked up in the module's globals at call
    time, so the window-attention seam composes in either installation order — the layer's own merge, and then
    transformer_ffn.ffn_tail (layer_norm_residual with no_ffn) in place of :408-414.  The replaced method otherwise (several
    heads, per-view attention, the epipolar path's attn_type, CPU or half precision, another width or mlp).
    `forward.native_calls` counts the calls the kernels took.  precision: the seam's option for ffn_tail's products, resolved
    at every call (layer_norm_residual has no product); `forward.precision` holds it."""
    from . import transformer_ffn as _tf
    _precision.seam_option("transformer_ffn_precision", precision)

    def forward(self, source, target, height=None, width=None, shifted_window_attn_mask=None, attn_num_splits=None, **kwargs):
        if not _transformer_ffn_call(self, source, target, kwargs):
            return replaced(self, source, target, height=height, width=width, shifted_window_attn_mask=shifted_window_attn_mask,
                            attn_num_splits=attn_num_splits, **kwargs)
        g = sys.modules[TRANSFORMER_FFN_MODULE].__dict__
        query, key, value = self.q_proj(source), self.k_proj(target), self.v_proj(target)
        if self.attention_type == "swin" and attn_num_splits > 1:
            message = g[WINDOW_ATTENTION_SPLIT](query, key, value, num_splits=attn_num_splits, with_shift=self.with_shift, h=height,
                                                w=width, attn_mask=shifted_window_attn_mask)
        else:
            message = g[WINDOW_ATTENTION_FULL](query, key, value)
        message = self.merge(message)
        forward.native_calls += 1
        n1 = self.norm1
        if self.no_ffn:
            return _tf.layer_norm_residual(message, n1.weight, n1.bias, source, n1.eps)
        return _tf.ffn_tail(source, message, n1.weight, n1.bias, self.mlp[0].weight, self.mlp[2].weight, self.norm2.weight,
                            self.norm2.bias, n1.eps, precision=_precision.resolve(precision))

    forward.replaced = replaced
    forward.precision = precision
    forward.native_calls = 0
    forward.__doc__ = _tf.ffn_tail.__doc__
    return forward


TRANSFORMER_FFN_SEAM = _MethodSeam("transformer_ffn", TRANSFORMER_FFN_MODULE, TRANSFORMER_FFN_CLASS, (TRANSFORMER_FFN_METHOD,),
                                   {TRANSFORMER_FFN_METHOD: _native_transformer_layer_forward}, context=True)


MONO_FUSION_MODULE = DEPTH_TAIL_MODULE                                 # defines EncoderCostVolume (:119-125 rgbd_fusion, :297 c2e, :351-354)
MONO_FUSION_CLASS = DEPTH_TAIL_CLASS
MONO_FUSION_METHOD = "__init__"
MONO_FUSION_NETS = ("rgbd_fusion", "c2e")


def _native_encoder_init(replaced, mod=None, precision="highest"):
    """EncoderCostVolume.__init__ with the reference's signature: the replaced constructor, then — only for an instance that has
    rgbd_fusion (add_mono_feat) — rgbd_fusion becomes a mono_fusion.FusedMonoFusion over the same four child modules (the same
    Parameter objects at the same indices: state-dict keys and the reference's checkpoints unchanged) and c2e.forward is rebound on
    the instance (mono_fusion.wrap_stitch; c2e.sample_grid stays where it is) so that the no-grad mono stitch returns a
    MonoStitchHandle.  precision: the seam's option; the encoder's FusedMonoFusion is stamped with it (and resolves "torch" at
    every call); `__init__.precision` holds it."""
    import functools

    from . import mono_fusion as _mf
    _precision.seam_option("mono_fusion_precision", precision)

    @functools.wraps(replaced)
    def __init__(self, *args, **kwargs):
        replaced(self, *args, **kwargs)
        fusion, c2e = (getattr(self, name, None) for name in MONO_FUSION_NETS)
        if isinstance(fusion, torch.nn.Sequential) and isinstance(c2e, torch.nn.Module):
            if not isinstance(fusion, _mf.FusedMonoFusion):
                self.rgbd_fusion = _mf.FusedMonoFusion.from_sequential(fusion)
            self.rgbd_fusion.precision = precision
            _mf.wrap_stitch(c2e, self.rgbd_fusion)

    __init__.replaced = replaced
    __init__.precision = precision
    return __init__


MONO_FUSION_SEAM = _MethodSeam("mono_fusion", MONO_FUSION_MODULE, MONO_FUSION_CLASS, (MONO_FUSION_METHOD,),
                               {MONO_FUSION_METHOD: _native_encoder_init}, context=True)


# install()'s option keywords -> their seams, in installation order; the decoder registry (DECODER_SEAM) comes after them.
# uninstall() restores exactly these, so a new seam is a new entry here and nothing else.
OPTION_SEAMS = {
    "adapter": (ADAPTER_SEAM,),
    "metrics": (SSIM_SEAM,),
    "depth_loss": (DEPTH_LOSS_SEAM,),
    "depth_metrics": (DEPTH_METRICS_SEAM,),
    "psnr": (PSNR_SEAM,),
    "cost_volume": (COST_VOLUME_SEAM,),
    "depth_head": (DEPTH_HEAD_SEAM,),
    "depth_tail": (DEPTH_TAIL_F_SEAM, DEPTH_TAIL_METHOD_SEAM),
    "erp_distance": (ERP_DISTANCE_SEAM,),
    "visualization": VIS_SEAMS,
    "depth_smoothness": (DEPTH_SMOOTH_SEAM,),
    "window_attention": (WINDOW_ATTENTION_SEAM,),
    "group_norm": GROUP_NORM_SEAMS,
    "unet_attention": UNET_ATTENTION_SEAMS,
    "transformer_ffn": (TRANSFORMER_FFN_SEAM,),
    "mono_fusion": (MONO_FUSION_SEAM,),
}


def _installed(keyword, **options) -> list:
    """Install every seam of one option; per seam, what its first name is bound to now, or None while its hook is pending."""
    bound = []
    for seam in OPTION_SEAMS[keyword]:
        out = seam.install(**options)
        bound.append(None if out is None else out[seam.names[0]])
    return bound


def install_adapter(**aopts):
    """The adapter half of install(adapter=True): see lazy.py.  Patches now if the reference's adapter module is already imported,
    else as soon as it is (import hook).  Returns the class or None.  aopts: sh_rotation ("native"), differentiable_means (False),
    lazy (True)."""
    return _installed("adapter", **aopts)[0]


def install_metrics():
    """The metrics half of install(metrics=True): rebind compute_ssim now if the reference's metrics module is imported, else as
    soon as it is (import hook).  Returns the patched function or None."""
    return _installed("metrics")[0]


def install_depth_loss():
    """The depth-loss half of install(depth_loss=True): rebind compute_l1_sphere_loss and erode now if the reference's helper
    module is imported, else as soon as it is (import hook).  Returns {name: patched function} or None."""
    return DEPTH_LOSS_SEAM.install()


def install_window_attention(precision: str = "highest"):
    """The half of install(window_attention=True): rebind the backbone module's single_head_split_window_attention,
    single_head_full_attention, generate_shift_window_attn_mask and multi_head_split_window_attention now if the module is
    imported, else as soon as it is (import hook).  Returns {name: patched function} or None.  precision: "highest" (exact
    float32 products), "high" (bf16x3 products, window_attention.py) or "torch" (torch.get_float32_matmul_precision() at every
    call: 'highest' is "highest", 'high' and 'medium' are "high")."""
    return WINDOW_ATTENTION_SEAM.install(precision=_precision.seam_option("window_attention_precision", precision))


def install_group_norm():
    """The half of install(group_norm=True): rebind ResBlock._forward and AttentionBlock._forward (ldm_unet/unet.py),
    DepthPredictorMultiView360.__init__ and the CNN backbone's ResidualBlock.forward to the wrappers around the fused
    norm + activation (+ residual) kernels of group_norm.py, each now if its module is imported, else as soon as it is (import
    hooks).  Returns {"Class.method": patched method or None}.  Modules built before the call keep their (norm, activation) pairs;
    group_norm.fuse_pairs(module) is the direct API for them."""
    return dict(zip((f"{seam.cls_name}.{seam.names[0]}" for seam in GROUP_NORM_SEAMS), _installed("group_norm")))


def install_unet_attention(precision: str = "highest"):
    """The half of install(unet_attention=True): rebind QKVAttentionLegacy.forward and QKVAttention.forward (ldm_unet/unet.py:527-599)
    to the wrappers around the fused QKV-attention kernels of qkv_attention.py now if the module is imported, else as soon as it
    is (import hook).  Returns {"Class.forward": patched method or None}.  precision: "highest" (exact float32 products), "high"
    (bf16x3 products, qkv_attention.py) or "torch" (torch.get_float32_matmul_precision() at every call: 'highest' is "highest",
    'high' and 'medium' are "high")."""
    return dict(zip((f"{seam.cls_name}.{seam.names[0]}" for seam in UNET_ATTENTION_SEAMS),
                    _installed("unet_attention", precision=_precision.seam_option("unet_attention_precision", precision))))


def install_transformer_ffn(precision: str = "highest"):
    """The half of install(transformer_ffn=True): rebind TransformerLayer.forward (multiview_transformer.py:334-414) to the wrapper
    around the fused kernels of transformer_ffn.py now if the module is imported, else as soon as it is (import hook).  Returns the
    patched method or None.  precision: "highest" (exact float32 products), "high" (bf16x3 products, transformer_ffn.py) or
    "torch" (torch.get_float32_matmul_precision() at every call: 'highest' is "highest", 'high' and 'medium' are "high")."""
    return _installed("transformer_ffn", precision=_precision.seam_option("transformer_ffn_precision", precision))[0]


def install_mono_fusion(precision: str = "highest"):
    """The half of install(mono_fusion=True): rebind EncoderCostVolume.__init__ (encoder_costvolume.py) to the wrapper that turns a
    new encoder's rgbd_fusion into a mono_fusion.FusedMonoFusion and wraps its c2e, now if the module is imported, else as soon as
    it is (import hook).  Returns the patched method or None.  Encoders built before the call keep their modules (and the
    precision they were built with); mono_fusion.FusedMonoFusion.from_sequential and mono_fusion.wrap_stitch are the direct API
    for them.  precision: "highest" (exact float32 products), "high" (bf16x3 products, mono_fusion.py) or "torch"
    (torch.get_float32_matmul_precision() at every call: 'highest' is "highest", 'high' and 'medium' are "high")."""
    return _installed("mono_fusion", precision=_precision.seam_option("mono_fusion_precision", precision))[0]


def install_depth_smoothness():
    """The half of install(depth_smoothness=True): rebind LossDepth.forward (src/loss/loss_depth.py:27-60) to the wrapper around
    the depth-smoothness kernels now if the reference's module is imported, else as soon as it is (import hook).  Returns the
    patched method or None."""
    return _installed("depth_smoothness")[0]


def install_depth_tail():
    """The half of install(depth_tail=True): rebind the predictor module's `F` to the interpolate proxy and
    EncoderCostVolume.map_pdf_to_opacity to the opacity-map wrapper, each now if its module is imported, else as soon as it is
    (import hooks).  Returns (proxy or None, method or None).  The predictor's :694-719 have no seam (inline arithmetic that ends in
    einops.repeat): depth_tail.fine_depth_tail is the direct API for them."""
    return tuple(_installed("depth_tail"))


def install_erp_distance():
    """The half of install(erp_distance=True): rebind depth_to_distance_map_batch now if the reference's module is imported, else
    as soon as it is (import hook).  Returns the patched function or None.  The evaluation step's reorder + conversion + stitch
    (model_wrapper_erp.py:446-463) are inline statements: stitch.Cube2Equirec.stitch_distance_rendered is the direct API for them."""
    return _installed("erp_distance")[0]


def install_visualization():
    """The half of install(visualization=True): rebind the evaluation step's depth_map (model_wrapper_erp.py:122-133), prep_image
    (image_io.py:38-54) and apply_color_map (color_map.py:9-19), each now if its module is imported, else as soon as it is (import
    hooks).  Returns {name: patched function or None}.  convert_single_colormap returns a CPU tensor by contract and the per-frame
    loops of test_step are inline: visualize.error_map and the batched visualize.depth_map are the direct API for them."""
    return dict(zip((seam.names[0] for seam in VIS_SEAMS), _installed("visualization")))


def install_depth_head():
    """The half of install(depth_head=True): rebind the encoder module's `F` to the softmax proxy now if the module is imported,
    else as soon as it is (import hook).  Returns the proxy or None."""
    return _installed("depth_head")[0]


def install_cost_volume():
    """The half of install(cost_volume=True): rebind the encoder module's warp_with_pose_depth_candidates now if the module is
    imported, else as soon as it is (import hook).  Returns the patched function or None."""
    return _installed("cost_volume")[0]


def install_depth_metrics():
    """The half of install(depth_metrics=True): rebind compute_depth_metrics_batched now if the reference's module is imported,
    else as soon as it is (import hook).  Returns the patched function or None."""
    return _installed("depth_metrics")[0]


def install_psnr():
    """The half of install(psnr=True): rebind compute_psnr now if the reference's metrics module is imported, else as soon as it
    is (import hook).  Returns the patched function or None."""
    return _installed("psnr")[0]



def install(*, lazy: bool = False, adapter: bool = False, adapter_options: Optional[dict] = None, metrics: bool = False,
            depth_loss: bool = False, depth_metrics: bool = False, psnr: bool = False, cost_volume: bool = False, depth_head: bool = False, depth_tail: bool = False,
            erp_distance: bool = False, visualization: bool = False, depth_smoothness: bool = False, window_attention: bool = False,
            group_norm: bool = False, unet_attention: bool = False, transformer_ffn: bool = False, mono_fusion: bool = False, **opts):
    """Register the fused decoder under the reference's registry key "splatting_cuda".  Returns the class (lazy=False) or None.
    adapter=True: ALSO replace the encoder's GaussianAdapterERP (gaussian_adapter_erp.py:33-119) by the lazy-field adapter of lazy.py,
    so that the registered decoder renders straight from the encoder's raw outputs (no [G,3,25] harmonics / [G,3,3] covariances in
    HBM); adapter_options: sh_rotation / differentiable_means / lazy of lazy.make_adapter_class.
    metrics=True: ALSO rebind the evaluation step's compute_ssim to the SSIM kernel (install_metrics; off by default).
    depth_loss=True: ALSO rebind the training step's compute_l1_sphere_loss and erode to the depth-loss kernels
    (install_depth_loss; off by default).
    depth_metrics=True: ALSO rebind the evaluation step's compute_depth_metrics_batched to the depth-metrics kernels
    (install_depth_metrics; off by default).
    psnr=True: ALSO rebind compute_psnr (evaluation and training step) to the PSNR kernels (install_psnr; off by default;
    metrics=True alone keeps meaning compute_ssim only).
    cost_volume=True: ALSO rebind the encoder's warp_with_pose_depth_candidates so that DepthPredictorMultiView360.forward builds
    raw_correlation_in with the fused cost-volume kernels (install_cost_volume; off by default).
    depth_head=True: ALSO rebind that module's `F` so that its softmax, expected depth and pdf maximum run as the fused depth-head
    kernels (install_depth_head; off by default).
    depth_tail=True: ALSO rebind that module's `F` so that its two F.interpolate calls run the upsampling kernels, and
    EncoderCostVolume.map_pdf_to_opacity to the opacity-map kernel (install_depth_tail; off by default; composes with depth_head in
    either order).
    erp_distance=True: ALSO rebind the evaluation step's depth_to_distance_map_batch (z_depth_to_distance.py:4-34, bound by
    model_wrapper_erp.py:48) to the z-depth -> distance kernel (install_erp_distance; off by default).
    visualization=True: ALSO rebind the evaluation step's depth_map, prep_image and apply_color_map to the kernels of
    splatter360_amd.visualize, so that a depth picture takes no sort and a frame crosses the bus as bytes (install_visualization;
    off by default).
    depth_smoothness=True: ALSO rebind the training step's LossDepth.forward (src/loss/loss_depth.py:27-60, the `depth` entry of
    the reference's loss registry) to the depth-smoothness kernels of splatter360_amd.depth_smooth (install_depth_smoothness;
    off by default).
    window_attention=True: ALSO rebind the multi-view transformer's single_head_split_window_attention and
    single_head_full_attention (src/model/encoder/backbone/multiview_transformer.py:8-16, :60-210) to the fused window-attention
    kernels of splatter360_amd.window_attention, and generate_shift_window_attn_mask to return a ShiftMask handle in place of
    the [K^2, Lw, Lw] tensor (install_window_attention; off by default).  window_attention_precision: "highest" (the default:
    exact float32 products), "high" (bf16x3 products on the bf16 MFMA) or "torch" (what torch.get_float32_matmul_precision() says
    at every call — the reference's main sets 'high', so with "torch" the unchanged reference runs the "high" kernels).
    group_norm=True: ALSO rebind the two U-Nets' ResBlock._forward and AttentionBlock._forward (ldm_unet/unet.py), the CNN
    backbones' ResidualBlock.forward and DepthPredictorMultiView360.__init__ so that every conv -> GroupNorm / InstanceNorm2d ->
    SiLU / GELU / ReLU (-> + skip) of the encoder runs the fused kernels of splatter360_amd.group_norm (install_group_norm; off
    by default).
    unet_attention=True: ALSO rebind the two U-Nets' QKVAttentionLegacy.forward and QKVAttention.forward (ldm_unet/unet.py:527-599)
    to the fused QKV-attention kernels of splatter360_amd.qkv_attention, which read the channel-major qkv tensor in place and form
    no [b heads, L, L] weight tensor (install_unet_attention; off by default; composes with group_norm, whose AttentionBlock._forward
    calls self.attention, and with the reference's checkpoint).  unet_attention_precision: "highest" (the default), "high" (bf16x3
    products on the bf16 MFMA, forward and backward) or "torch" (torch's setting at every call, the checkpoint's recomputation
    included); independent of the other precisions.
    transformer_ffn=True: ALSO rebind the multi-view transformer's TransformerLayer.forward (multiview_transformer.py:334-414) so
    that norm1, cat([source, message]), the mlp, norm2 and the residual behind the layer's attention run the fused kernels of
    splatter360_amd.transformer_ffn, which form no [T, 2C] or [T, 8C] tensor (install_transformer_ffn; off by default; composes
    with window_attention in either order; state_dict keys are unchanged).  transformer_ffn_precision: "highest" (the default),
    "high" (bf16x3 products on the bf16 MFMA in ffn_tail, forward and backward) or "torch" (torch's setting at every call);
    independent of window_attention_precision.
    mono_fusion=True: ALSO rebind EncoderCostVolume.__init__ (encoder_costvolume.py) so that an encoder built with add_mono_feat
    gets a mono_fusion.FusedMonoFusion as rgbd_fusion (the same four children and Parameter objects: state-dict keys 0.weight,
    1.weight, 1.bias, 3.weight unchanged) and a c2e whose forward, called with grad disabled on a 4-D float32 GPU tensor of
    rgbd_fusion[0].in_features - out_features channels at widths the kernels take (C = 128, Cm a multiple of 64 in 64 .. 1024),
    returns a mono_fusion.MonoStitchHandle in place of the stitched [(b v), Cm, h, w] map (:297) — metadata and no data; every other
    call runs the module's own forward and returns its bits; c2e.sample_grid and its state-dict key are unchanged.  The handle stays
    lazy through exactly what the reference does next: torch.cat([trans_features, handle], dim=1) (:351), the permute(0, 2, 3, 1)
    that einops' rearrange issues for "bv c h w -> bv h w c" (:353), same-shape reshapes and metadata queries.  FusedMonoFusion then
    runs the fused kernels of splatter360_amd.mono_fusion — the stitch, the concatenation, Linear, LayerNorm, ReLU, Linear in one
    forward kernel and a three-launch backward that form neither the stitched map nor the [(b v), C + Cm, h, w] concatenation — and
    returns out.permute(0, 2, 3, 1), so the rearrange back (:354) yields a dense NCHW tensor.  Any other operation on a handle
    first materialises it (the stitch by c2e's own forward under no_grad, then torch's cat and permute) and runs on the real tensor
    with the reference's values.  install_mono_fusion; off by default; composes with depth_tail, whose method seam sits on the same
    class, in either order; uninstall() restores the class (encoders built meanwhile keep their modules).
    mono_fusion_precision: "highest" (the default), "high" (bf16x3 products on the bf16 MFMA, forward and backward) or "torch"
    (torch's setting at every call); stamped on each new encoder's FusedMonoFusion, independent of the other three precisions.

    lazy=False: imports `src.model.decoder` now (the reference must be importable: its repository root on sys.path) and patches
    its DECODERS dict in place — `get_decoder` reads the dict at call time, so every later `get_decoder(cfg, dataset_cfg)` builds
    the fused decoder.  lazy=True: only installs an import hook that patches the registry when the reference itself first imports
    the package (for a sitecustomize that runs before sys.path is set up).  Idempotent.
    opts: window_attention_precision, unet_attention_precision, transformer_ffn_precision, mono_fusion_precision (above); for the decoder views_per_group (6), shared_campos (None = checked per group with one small read per forward), check ("sync"), glue."""
    given = locals()
    # an option of a seam, not a seam: taken out of opts (the decoder's options) before they reach the decoder
    for seam in ("window_attention", "unet_attention", "transformer_ffn", "mono_fusion"):
        option = seam + "_precision"
        given[seam + "_options"] = {"precision": _precision.seam_option(option, opts.pop(option, "highest"))}
    for keyword, seams in OPTION_SEAMS.items():
        if given[keyword]:
            for seam in seams:
                seam.install(**(given.get(keyword + "_options") or {}))
    if lazy:
        out = DECODER_SEAM.install(**opts)
        return None if out is None else out[REGISTRY_KEY]
    DECODER_SEAM.options = opts
    return DECODER_SEAM.patch(importlib.import_module(REGISTRY_MODULE))[REGISTRY_KEY]      # any error propagates


def uninstall() -> None:
    """Put the reference's own decoder class, adapter, compute_ssim, compute_psnr, compute_depth_metrics_batched,
    compute_l1_sphere_loss, erode, warp_with_pose_depth_candidates, depth_to_distance_map_batch, depth_map, prep_image,
    apply_color_map, EncoderCostVolume.map_pdf_to_opacity, LossDepth.forward, the backbone module's four attention functions,
    ResBlock._forward, AttentionBlock._forward, ResidualBlock.forward, DepthPredictorMultiView360.__init__,
    QKVAttentionLegacy.forward, QKVAttention.forward, TransformerLayer.forward, EncoderCostVolume.__init__ and the predictor
    module's `F` (torch.nn.functional itself) back (and drop pending import hooks)."""
    sys.meta_path[:] = [f for f in sys.meta_path if not isinstance(f, _SeamPatcher)]
    for seams in (*OPTION_SEAMS.values(), (DECODER_SEAM,)):
        for seam in seams:
            seam.restore()
