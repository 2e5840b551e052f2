"""richsem_amd -- MI355X (gfx950) native multi-scale deformable attention for RichSem.

Scope: the one data-parallel hot path of the reference (MengLcool/RichSem), i.e. the operator
behind ``models/richsem/ops`` -- hand-written HIP kernels behind a C ABI
(include/richsem_msda.h, richsem_amd/csrc), a drop-in for the reference's compiled module
``MultiScaleDeformableAttention`` and host-side mirrors of ``MSDeformAttnFunction`` /
``MSDeformAttn`` with the reference's names, arguments and state-dict keys.

There is no CPU / PyTorch fallback: a missing HIP library raises.
"""
import sys

__version__ = "0.1.0"


def __getattr__(name):      # PostProcess is exported from the package without importing torch at `import richsem_amd`
    if name == "PostProcess":
        from .postprocess import PostProcess
        return PostProcess
    if name in ("batch_geometry", "sizes_from_targets"):      # the batch-geometry tensors from the image sizes (geometry.py), likewise
        from . import geometry
        return getattr(geometry, name)
    if name in ("denoising_queries", "dn_capacity", "DenoisingQueriesFunction"):      # the denoising queries from the counts on the device (dn.py)
        from . import dn
        return getattr(dn, name)
    if name in ("window_attention", "swin_linear", "swin_layernorm", "swin_mlp", "swin_merge_norm", "swin_norm_nchw", "swin_patch_rows",
                "WindowAttention", "SwinTransformerBlock", "PatchMerging", "BasicLayer", "PatchEmbed", "SwinTransformer"):      # the Swin backbone and its kernels (swin.py)
        from . import swin
        return getattr(swin, name)
    if name in ("dwconv7", "layer_scale", "convnext_block", "ConvNeXt", "build_convnext"):      # the ConvNeXt backbone and its kernels (convnext.py)
        from . import convnext
        return getattr(convnext, name)
    if name in ("focal_context", "modulate", "FocalModulation", "FocalModulationBlock", "FocalNet", "build_focalnet"):      # the FocalNet backbone and its kernels (focalnet.py)
        from . import focalnet
        return getattr(focalnet, name)
    if name in ("MaskTargets", "mask_losses", "mask_losses_torch", "mask_losses_and_grads", "PostProcessSegm"):      # the criterion's mask terms and the mask post-processor (masks.py)
        from . import masks
        return getattr(masks, name)
    if name in ("dynamic_masks", "dynamic_masks_torch", "dynamic_masks_and_grads", "MaskBranch", "MaskHeadSmallConv"):      # the CondInst dynamic mask head (cond_inst.py)
        from . import cond_inst
        return getattr(cond_inst, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def install_dropin():
    """Register the drop-in under the reference's extension name, so that the reference's own
    ``import MultiScaleDeformableAttention as MSDA`` (ops/functions/ms_deform_attn_func.py:18) resolves to it."""
    from . import MultiScaleDeformableAttention as shim
    sys.modules.setdefault("MultiScaleDeformableAttention", shim)
    return shim
