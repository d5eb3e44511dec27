"""MI355X-native panoramic Gaussian-splat render path.  Importing the package loads nothing heavy; the HIP
library is loaded on first use (splatter360_amd._lib) and there is no CPU fallback."""


def install(**opts):
    """Register the fused decoder in the unchanged reference's decoder registry (splatter360_amd.plugin.install).  Keywords
    switch the other native seams on, each off by default: adapter, metrics, depth_loss, depth_metrics, psnr, cost_volume,
    depth_head (the encoder's softmax depth head, splatter360_amd.depth_head) and depth_tail (its two interpolations and
    map_pdf_to_opacity, splatter360_amd.depth_tail, whose fine_depth_tail is the direct API for the rest of that stretch),
    erp_distance, visualization (the evaluation step's depth_map, prep_image and apply_color_map, splatter360_amd.visualize),
    depth_smoothness (the training step's LossDepth.forward, splatter360_amd.depth_smooth), window_attention (the multi-view
    transformer's attention, splatter360_amd.window_attention; window_attention_precision = "highest", "high" for its bf16x3
    products, or "torch" to follow torch.get_float32_matmul_precision() at every call), group_norm (the encoder's norm + activation + residual sites,
    splatter360_amd.group_norm), unet_attention (the two U-Nets' multi-head QKV attention, splatter360_amd.qkv_attention) and
    transformer_ffn (the multi-view transformer layers' norm / mlp / norm tail, splatter360_amd.transformer_ffn)."""
    from .plugin import install as _install
    return _install(**opts)


def uninstall():
    from .plugin import uninstall as _uninstall
    return _uninstall()


def __getattr__(name):
    """splatter360_amd.Equirec2Cube: the ERP -> cube resampler (splatter360_amd.equirec2cube), imported on first use so that
    importing the package stays light.  It has no install() seam: the reference calls it in data-loader workers on numpy arrays."""
    if name == "visualize":                                   # depth_map, depth_range, colorize, prep_image, error_map
        import importlib
        return importlib.import_module(".visualize", __name__)
    if name == "Equirec2Cube":
        from .equirec2cube import Equirec2Cube
        return Equirec2Cube
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
