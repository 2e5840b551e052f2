"""The ConvNeXt backbone on the library's kernels.

Reference: models/richsem/convnext.py (``build_backbone`` takes it for ``convnext_xlarge_22k``: models/richsem/backbone.py:291-293).  A block
is ``x + gamma * pwconv2(GELU(pwconv1(LayerNorm(dwconv7x7(x)))))``.  Almost all of it runs on the shared row operators of
:mod:`richsem_amd.backbone_ops` (the linear layer with its GELU epilogues, the LayerNorms, the layer scale, the patch rows); the operator
that is this backbone's alone is here: :func:`dwconv7` (csrc/convnext_dw.hip; C ABI ``msda_dwconv7_*``), the depthwise 7 x 7 convolution
of a channels-last map (B, H, W, C), zero padding per image; its backward is the same kernel with the taps flipped plus a weight-gradient
kernel with a fixed summation order.

bf16 tensors on the device take the kernels and never fall back: a missing library or a width outside the kernels' limits raises.  CPU
tensors and fp32 / fp64 tensors run a torch composition of the same formulas (what makes the mirrors testable in float64).

The classes mirror the reference's -- constructor arguments and state-dict keys -- so a reference checkpoint loads with ``strict=True``
both ways.  On a bf16 device tensor a stage runs channels-last from the stem to the output norms, with :func:`dwconv7` always.  The plain
attribute ``fused`` (``Block.set_fused`` / ``ConvNeXt.set_fused``; False by default, not a constructor argument, not in the state dict)
chooses the rest of that path: with it the LayerNorms, the two products (GELU epilogue, saved pre-activation), the layer scale, the stem as
patch rows, the downsampling products and the output norms (``swin_norm_nchw``) run on library kernels, :func:`convnext_block` being ONE
autograd function per block; without it they run on torch ops on the same channels-last tensors.  CPU, fp32 and fp64 tensors run the
reference's order of operations in NCHW either way.

The stem (4 x 4, stride 4) and the downsampling convolutions (2 x 2, stride 2) have no padding: they DROP trailing rows and columns
(45 x 54 -> 11 x 13 -> 5 x 6 -> 2 x 3 -> 1 x 1), where the Swin layers pad.  The map is cropped to a multiple of the stride before the
gather.  In the downsampling the LayerNorm over C comes first and the 2 x 2 gather second (``swin_merge_norm`` is the other order over
4 C: not this operator); the gather of a channels-last map is a view, a permute and a reshape, and the matching weight is
``conv.weight.permute(0, 2, 3, 1).flatten(1)``.

Nothing here downloads anything: ``build_convnext(..., pretrained=True)`` raises; the caller loads a state dict.  Capturing the device path
into a HIP graph is untested.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .backbone_ops import (EPI_BIAS, EPI_RESIDUAL, MAX_C, DropPath, cached_forms, cast, check_bf16, check_vector, depthwise_weight_grads, f32,
                           gelu_mlp_backward, gelu_mlp_forward, layer_scale, layer_scale_backward_kernel, layer_scale_kernel,
                           layernorm_backward_kernel, layernorm_kernel, linear_forms, linear_on_forms, mask_pyramid, need_erf_gelu, on_kernels,
                           patch_linear, ptr, refuse_drop_path_in_training, swin_layernorm, swin_norm_nchw, swin_patch_rows)
from .param_cache import VersionCache

__all__ = ["dwconv7", "layer_scale", "convnext_block", "dwconv7_weight_form", "LayerNorm", "Block", "ConvNeXt", "build_convnext"]


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
def _check_map(x, what):
    """a (B, H, W, C) bf16 map on the device, C a multiple of 32 in [32, 4096] -> contiguous"""
    if x.dim() != 4:
        raise RuntimeError(f"{what}: a channels-last map (B, H, W, C), got {tuple(x.shape)}")
    check_bf16(x, x.shape[-1], what)
    return x.contiguous()


def dwconv7_weight_form(weight):
    """the parameter (C, 1, 7, 7) -> the form the kernels read: (49, C) float32, tap-major (row 7 ky + kx)"""
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (1, 7, 7):
        raise RuntimeError(f"dwconv7: weight (C, 1, 7, 7), got {tuple(weight.shape)}")
    return weight.detach().float().reshape(weight.shape[0], 49).t().contiguous()


def dwconv7_kernel(x, w49, bias=None, add=None, flip=0):
    """One call of ``msda_dwconv7_bf16`` (no autograd): x, add (B, H, W, C) bf16 on the device, w49 (49, C) and bias (C) float32"""
    x = _check_map(x, "dwconv7")
    B, H, W, C = x.shape
    if w49.dtype != torch.float32 or tuple(w49.shape) != (49, C) or w49.device != x.device or not w49.is_contiguous():
        raise RuntimeError(f"dwconv7: weight form float32 (49, {C}) contiguous on {x.device}, got {w49.dtype} {tuple(w49.shape)} on {w49.device}")
    check_vector(bias, C, x.device, "dwconv7 (bias)")
    if add is not None:
        add = _check_map(add, "dwconv7 (add)")
        if add.shape != x.shape or add.device != x.device:
            raise RuntimeError(f"dwconv7: add {tuple(x.shape)} on {x.device}, got {tuple(add.shape)} on {add.device}")
    out = torch.empty_like(x)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_dwconv7_bf16(x.data_ptr(), w49.data_ptr(), ptr(bias), ptr(add), int(flip), B, H, W, C, out.data_ptr(),
                                                 _lib.raw_stream(x.device)))
    return out


def dwconv7_workspace_bytes(B, H, W, C):
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_dwconv7_workspace_bytes(B, H, W, C, ctypes.byref(n)))
    return n.value


def dwconv7_wgrad_kernel(dy, x, want_bias=True):
    """``msda_dwconv7_wgrad_bf16``: dy, x (B, H, W, C) bf16 on the device -> (dw (49, C) float32, dbias (C) float32 or None)"""
    x = _check_map(x, "dwconv7 (weight gradient)")
    dy = _check_map(dy, "dwconv7 (weight gradient)")
    if dy.shape != x.shape or dy.device != x.device:
        raise RuntimeError(f"dwconv7: dy {tuple(x.shape)} on {x.device}, got {tuple(dy.shape)} on {dy.device}")
    B, H, W, C = x.shape
    dw = torch.empty((49, C), dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device) if want_bias else None
    ws = torch.empty(dwconv7_workspace_bytes(B, H, W, C) // 4, dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_dwconv7_wgrad_bf16(dy.data_ptr(), x.data_ptr(), B, H, W, C, dw.data_ptr(), ptr(db), ws.data_ptr(),
                                                       _lib.raw_stream(x.device)))
    return dw, db


def _dwconv7_wgrads(want_w, want_b, dy, x, wdt, wshape, bdt):
    """(dweight, dbias) as the parameters are, from ONE call of the weight-gradient kernel -- none when neither is wanted"""
    if not (want_w or want_b):
        return None, None
    dw, db = dwconv7_wgrad_kernel(dy, x, want_bias=want_b)
    return depthwise_weight_grads(dw, [(wdt, wshape)], [want_w])[0], cast(db, bdt)


class _DwConv7Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, w49):
        out = dwconv7_kernel(x, w49, f32(bias) if bias is not None else None)
        ctx.save_for_backward(x, w49)
        ctx.meta = (weight.dtype, weight.shape, bias.dtype if bias is not None else None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w49 = ctx.saved_tensors
        wdt, wshape, bdt = ctx.meta
        dy = dy.contiguous()
        dx = dwconv7_kernel(dy, w49, flip=1) if ctx.needs_input_grad[0] else None
        dw, db = _dwconv7_wgrads(ctx.needs_input_grad[1], bdt is not None and ctx.needs_input_grad[2], dy, x, wdt, wshape, bdt)
        return dx, dw, db, None


def dwconv7(x, weight, bias=None, cache=None):
    """The depthwise 7 x 7 convolution with zero padding 3 of a channels-last map: x (B, H, W, C), ``weight`` the parameter (C, 1, 7, 7),
    ``bias`` (C) or None -> (B, H, W, C).  A bf16 device map takes ``msda_dwconv7_bf16`` (C a multiple of 32 up to 4096; the input gradient
    is the same kernel with the taps flipped, weight and bias gradients ``msda_dwconv7_wgrad_bf16``'s, returned in the parameters' dtypes)
    and never falls back; any other tensor runs ``F.conv2d(groups=C)`` on the permuted map.  ``cache``: a VersionCache that keeps the
    (49, C) float32 form of the weight per parameter version."""
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (x.shape[-1], 1, 7, 7):
        raise RuntimeError(f"dwconv7: a map (B, H, W, C) and a weight (C, 1, 7, 7), got {tuple(x.shape)} and {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (x.shape[-1],):
        raise RuntimeError(f"dwconv7: bias ({x.shape[-1]}), got {tuple(bias.shape)}")
    if not on_kernels(x):
        return F.conv2d(x.permute(0, 3, 1, 2), weight, bias, padding=3, groups=x.shape[-1]).permute(0, 2, 3, 1)
    w49 = dwconv7_weight_form(weight) if cache is None else cache.get([weight], lambda: dwconv7_weight_form(weight))
    return _DwConv7Function.apply(x, weight, bias, w49)


class _ConvNeXtBlockFunction(torch.autograd.Function):
    """the whole block on kernels; argument order: x, dwconv (w, b), norm (w, b), eps, pwconv1 (w, b), pwconv2 (w, b), gamma, forms"""

    @staticmethod
    def forward(ctx, x, dw_w, dw_b, nw, nb, eps, w1, b1, w2, b2, gamma, w49, f1, f2):
        x = _check_map(x, "convnext_block")
        C = x.shape[-1]
        need = any(ctx.needs_input_grad)
        y = dwconv7_kernel(x, w49, f32(dw_b) if dw_b is not None else None).view(-1, C)
        g32 = f32(nw)
        xn, mean, rstd = layernorm_kernel(y, g32, f32(nb), eps, want_stats=need)
        x2 = x.view(-1, C)
        if gamma is None:
            out, u = gelu_mlp_forward(xn, f1, f2, need, EPI_RESIDUAL, x2)
            z = gam32 = None
        else:
            z, u = gelu_mlp_forward(xn, f1, f2, need, EPI_BIAS)
            gam32 = f32(gamma)
            out = layer_scale_kernel(z, gam32, x2)
        if need:
            ctx.save_for_backward(x, y, xn, mean, rstd, u, z if ctx.needs_input_grad[10] else None, g32, gam32, w49)
            ctx.forms = (f1, f2)
            ctx.meta = tuple(p.dtype if p is not None else None for p in (dw_w, dw_b, nw, nb, w1, b1, w2, b2, gamma)) + (dw_w.shape,)
        return out.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x, y, xn, mean, rstd, u, z, g32, gam32, w49 = ctx.saved_tensors
        (f1, f2), (dwdt, dbdt, nwdt, nbdt, *dtypes, gdt, wshape) = ctx.forms, ctx.meta
        need = ctx.needs_input_grad
        C = x.shape[-1]
        dout = dout.contiguous()
        d2 = dout.view(-1, C)
        dgam = None
        if gam32 is not None:
            dz, dgam = layer_scale_backward_kernel(d2, z, gam32, want_gamma=need[10])
        else:
            dz = d2
        dxn, dw1, db1, dw2, db2 = gelu_mlp_backward(ctx, (6, 7, 8, 9), dtypes, dz, xn, u, f1, f2)      # pwconv1 (w, b), pwconv2 (w, b)
        dy, dg, db = layernorm_backward_kernel(dxn, y, mean, rstd, g32, want_gamma=need[3], want_beta=need[4])
        dy = dy.view(x.shape)
        dx = dwconv7_kernel(dy, w49, add=dout, flip=1) if need[0] else None      # dout + dwconv^T(dy), rounded once
        ddw, ddb = _dwconv7_wgrads(need[1], dbdt is not None and need[2], dy, x, dwdt, wshape, dbdt)
        return dx, ddw, ddb, cast(dg, nwdt), cast(db, nbdt), None, dw1, db1, dw2, db2, cast(dgam, gdt), None, None, None


def convnext_block(x, block):
    """A :class:`Block` as ONE autograd function on library kernels: x (B, H, W, C) bfloat16 on the device, channels-last.  Forward:
    ``msda_dwconv7_bf16``; LayerNorm; pwconv1 and pwconv2 under the GELU-MLP policy of ``backbone_ops``; the layer scale with the residual
    (or, without ``gamma``, pwconv2's residual epilogue).  Saved for the backward: x, the convolution's output, norm(.), the statistics, the
    pre-activation and pwconv2's output.  The backward ends with the flipped convolution with ``dout`` as its ``add``: the input gradient
    is rounded once.  Stochastic depth is not part of it (``drop_path > 0`` in training mode raises NotImplementedError)."""
    refuse_drop_path_in_training(block, "convnext")
    need_erf_gelu(block.act, "convnext")
    dw, norm, p1, p2 = block.dwconv, block.norm, block.pwconv1, block.pwconv2
    w49 = block._forms["dwconv"].get([dw.weight], lambda: dwconv7_weight_form(dw.weight))
    return _ConvNeXtBlockFunction.apply(x, dw.weight, dw.bias, norm.weight, norm.bias, float(norm.eps), p1.weight, p1.bias, p2.weight, p2.bias,
                                        block.gamma, w49, cached_forms(block._forms["pwconv1"], p1.weight, p1.bias),
                                        cached_forms(block._forms["pwconv2"], p2.weight, p2.bias))


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
class LayerNorm(nn.Module):
    """LayerNorm over the channels of a channels-last (..., C) or channels-first (B, C, H, W) tensor (``data_format``), eps 1e-6"""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError(f"richsem_amd.convnext: data_format {data_format!r}")
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        if self.data_format == "channels_last":
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        mean = x.mean(1, keepdim=True)
        var = (x - mean).pow(2).mean(1, keepdim=True)
        return self.weight[:, None, None] * ((x - mean) / torch.sqrt(var + self.eps)) + self.bias[:, None, None]

    def on_map(self, x, fused):
        """the same norm of a channels-last map, whatever ``data_format`` says about the tensors ``forward`` takes"""
        if fused:
            return swin_layernorm(x, self.weight, self.bias, self.eps)
        return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)


class Block(nn.Module):
    """The reference's block: ``forward(x)`` on (B, C, H, W).  A bf16 device tensor runs :meth:`forward_map` on the channels-last map:
    :func:`dwconv7` always, and with ``fused`` (a plain attribute, False by default; not a constructor argument, not in the state dict) the
    rest as :func:`convnext_block`, which never falls back.  CPU, fp32 and fp64 tensors run the torch formula either way."""

    fused = False

    def __init__(self, dim, drop_path=0., layer_scale_init_value=1e-6):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if layer_scale_init_value > 0 else None
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self._forms = {k: VersionCache() for k in ("dwconv", "pwconv1", "pwconv2")}      # derived weight forms of the device path

    def set_fused(self, flag=True):
        self.fused = bool(flag)
        return self

    def forward_map(self, x):
        """x (B, H, W, C) bf16 on the device -> the same shape"""
        if self.fused:
            return convnext_block(x, self)
        z = dwconv7(x, self.dwconv.weight, self.dwconv.bias, cache=self._forms["dwconv"])
        z = self.pwconv2(self.act(self.pwconv1(self.norm(z))))
        if self.gamma is not None:
            z = self.gamma * z
        return x + self.drop_path(z)

    def forward(self, x):
        if on_kernels(x):
            return self.forward_map(x.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
        z = self.dwconv(x).permute(0, 2, 3, 1)
        z = self.pwconv2(self.act(self.pwconv1(self.norm(z))))
        if self.gamma is not None:
            z = self.gamma * z
        return x + self.drop_path(z.permute(0, 3, 1, 2))


class ConvNeXt(nn.Module):
    """``forward_features(images)`` -> the tuple of (B, C_i, H_i, W_i) features of ``out_indices``; ``forward(images, mask)`` -> a list of
    (feature, mask) pairs with the padding mask (B, H, W) bool interpolated to each level, as ``SwinTransformer.forward`` does.
    ``num_classes`` and ``head_init_scale`` are accepted for the reference's call and not used (it builds no head either)."""

    def __init__(self, in_chans=3, num_classes=1000, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), drop_path_rate=0.,
                 layer_scale_init_value=1e-6, head_init_scale=1., out_indices=(0, 1, 2, 3)):
        super().__init__()
        if len(depths) != 4 or len(dims) != 4:
            raise ValueError(f"richsem_amd.convnext: four stages, got depths {tuple(depths)} and dims {tuple(dims)}")
        self.dims = dims
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4),
                                                    LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(3):
            self.downsample_layers.append(nn.Sequential(LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                                                        nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        rates = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.stages = nn.ModuleList()
        for i in range(4):
            first = sum(depths[:i])
            self.stages.append(nn.Sequential(*[Block(dim=dims[i], drop_path=rates[first + j], layer_scale_init_value=layer_scale_init_value)
                                               for j in range(depths[i])]))
        self.out_indices = out_indices
        for i in range(4):
            self.add_module(f"norm{i}", LayerNorm(dims[i], eps=1e-6, data_format="channels_first"))
        self.fused = False
        self._forms = [VersionCache() for _ in range(4)]      # the stem's and the downsampling products' weight forms (fused path)

    def set_fused(self, flag=True):
        """``fused`` of every block, of the stem, the downsampling layers and the output norms"""
        self.fused = bool(flag)
        for stage in self.stages:
            for blk in stage:
                blk.fused = self.fused
        return self

    # -- the device path: channels-last from the stem to the output norms --
    def _stem_map(self, img):
        conv, norm = self.downsample_layers[0]
        B, _, H, W = img.shape
        ph, pw = conv.kernel_size
        Hs, Ws = H // ph, W // pw
        if Hs < 1 or Ws < 1:
            raise RuntimeError(f"richsem_amd.convnext: an image of {H} x {W} is smaller than the stem's {ph} x {pw} patch")
        if not self.fused:
            return norm.on_map(F.conv2d(img, conv.weight, conv.bias, stride=conv.stride).permute(0, 2, 3, 1), False)
        rows = swin_patch_rows(img[:, :, :Hs * ph, :Ws * pw], (ph, pw))      # no padding: trailing rows and columns are dropped
        return norm.on_map(patch_linear(rows, conv.weight, conv.bias, self._forms[0]), True).view(B, Hs, Ws, -1)

    def _downsample_map(self, i, x):
        norm, conv = self.downsample_layers[i]
        B, H, W, C = x.shape
        H2, W2 = H // 2, W // 2
        if H2 < 1 or W2 < 1:
            raise RuntimeError(f"richsem_amd.convnext: a map of {H} x {W} cannot be downsampled")
        x = norm.on_map(x, self.fused)[:, :2 * H2, :2 * W2]      # the norm first, then the gather; trailing row / column dropped
        rows = x.reshape(B, H2, 2, W2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H2, W2, 4 * C)
        w2d = conv.weight.permute(0, 2, 3, 1).flatten(1)      # (N, dy, dx, C): the order of the gathered row
        if not self.fused:
            return F.linear(rows, w2d, conv.bias)
        return linear_on_forms(rows, w2d, conv.bias, cached_forms(self._forms[i], conv.weight, conv.bias, lambda: linear_forms(w2d, conv.bias)))

    def _features_map(self, x):
        outs = []
        for i in range(4):
            x = self._stem_map(x) if i == 0 else self._downsample_map(i, x)
            for blk in self.stages[i]:
                x = blk.forward_map(x)
            if i in self.out_indices:
                norm = getattr(self, f"norm{i}")
                B, H, W, C = x.shape
                if self.fused:
                    outs.append(swin_norm_nchw(x.reshape(B, H * W, C), H, W, norm.weight, norm.bias, norm.eps))
                else:
                    outs.append(norm.on_map(x, False).permute(0, 3, 1, 2).contiguous())
        return tuple(outs)

    def forward_features(self, x):
        if on_kernels(x):
            return self._features_map(x)
        outs = []
        for i in range(4):
            x = self.stages[i](self.downsample_layers[i](x))
            if i in self.out_indices:
                outs.append(getattr(self, f"norm{i}")(x))
        return tuple(outs)

    def forward(self, images, mask):
        return mask_pyramid(self.forward_features(images), mask)


def build_convnext(modelname, pretrained, backbone_dir=None, **kw):
    """The reference's builder (``convnext_xlarge_22k``: depths (3, 3, 27, 3), dims (256, 512, 1024, 2048)).  ``pretrained=True`` raises:
    this module never downloads anything; build with ``pretrained=False`` and load a state dict."""
    if modelname not in ("convnext_xlarge_22k",):
        raise ValueError(f"richsem_amd.convnext: unknown model {modelname!r} (convnext_xlarge_22k)")
    if pretrained:
        raise NotImplementedError("richsem_amd.convnext: pretrained=True is not supported: nothing is downloaded here; build with "
                                  "pretrained=False and load_state_dict() a checkpoint")
    cfg = dict(depths=[3, 3, 27, 3], dims=[256, 512, 1024, 2048])
    cfg.update(kw)
    return ConvNeXt(**cfg)
