"""The Swin backbone with its shifted-window attention as one kernel per direction.

Reference: models/richsem/swin_transformer.py.  :func:`window_attention` computes, per (image, window, head),
``softmax(q k^T / sqrt(32) + relative-position bias + region mask) v`` on MAP-layout operands -- ``qkv`` (B, Hp, Wp, 3 C) with the last
dimension ordered (3, heads, 32) -- and returns (B, Hp, Wp, C): the reference's ``torch.roll``, ``window_partition``, bias gather, mask
tensor, ``window_reverse`` and second roll are index arithmetic inside the kernels (csrc/swin_attn_mfma.hip; C ABI ``msda_swin_attn_*``).
Its backward writes ``dqkv`` once and ``dtable`` with a fixed summation order (bitwise reproducible).

The classes mirror the reference's -- constructor arguments and state-dict keys (``relative_position_index`` included), so a reference
checkpoint loads with ``strict=True`` both ways.  bf16 tensors on the device take the kernels; CPU tensors and fp32 / fp64 tensors run
:func:`window_attention_torch`, the same formula as a plain torch composition over map indices (what makes the mirrors testable in
float64).  A bf16 device tensor never falls back to the composition: a missing library or a head dimension other than 32 raises.

The rest of a block -- norm1, qkv, proj + residual, norm2, fc1, GELU, fc2 + residual -- runs on torch ops unless the block's plain
attribute ``fused`` is set (``BasicLayer.set_fused`` / ``SwinTransformer.set_fused``; off by default, not a constructor argument and not
in the state dict).  With it a bf16 device tensor takes the shared row operators of :mod:`richsem_amd.backbone_ops` (``swin_layernorm``,
``swin_linear``) and :func:`swin_mlp`, ONE autograd function for ``x + fc2(GELU(fc1(norm(x))))`` under that module's GELU-MLP policy.  CPU,
fp32 and fp64 tensors run the torch formula with ``fused`` set too.  Where the backbone changes layout -- the patch embedding, the three
PatchMerging layers and the output norms -- a second switch, ``SwinTransformer.set_fused_stages`` (``PatchEmbed.fused``,
``PatchMerging.fused``, ``SwinTransformer.fused_stages``; off by default like ``fused``), puts the index arithmetic into kernels
(csrc/swin_stage.hip): :func:`swin_merge_norm`, here, is the LayerNorm of the 2 x 2 gathered rows read straight from the map (C ABI
``msda_swin_merge_norm_*``); the output norms and the patch rows are ``backbone_ops.swin_norm_nchw`` and ``swin_patch_rows``.
``set_fused`` keeps meaning the blocks only.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
# (the operators that lived here before backbone_ops.py stay reachable as swin.<name>: tests and tools call swin.linear_kernel and others)
from .backbone_ops import (BF16, EPI_BIAS, EPI_GELU, EPI_GELU_BACKWARD, EPI_RESIDUAL, DropPath, bf16_rows, cached_forms, cast,      # noqa: F401
                           check_bf16, column_sums, f32, gelu_mlp_backward, gelu_mlp_forward, layernorm_backward_kernel, layernorm_kernel,
                           layernorm_workspace_bytes, linear_forms, linear_kernel, mask_pyramid, need_erf_gelu, need_layernorm,
                           norm_nchw_backward_kernel, norm_nchw_kernel, on_kernels, output_norm_nchw, pair, patch_grid, patch_linear, patch_width,
                           ptr, refuse_drop_path_in_training, swin_layernorm, swin_linear, swin_norm_nchw, swin_patch_rows, token_norm_operands)
from .param_cache import VersionCache

__all__ = ["window_attention", "window_attention_torch", "swin_linear", "swin_layernorm", "swin_mlp", "swin_merge_norm", "swin_norm_nchw",
           "swin_patch_rows", "WindowAttention",
           "SwinTransformerBlock", "PatchMerging", "BasicLayer", "PatchEmbed", "SwinTransformer", "Mlp", "DropPath"]

HEAD_DIM = 32      # what the kernels are built for (every Swin variant of the reference: swin_transformer.py:676-710)


# ---- the map <-> window index arithmetic ---------------------------------------------------------------------------------------------
def window_pixels(Hp, Wp, window, shift, device=None):
    """-> (pix, region), both (windows, window^2) int64: token t = i * window + j of window (wy, wx) has rolled coordinates
    (py, px) = (wy * window + i, wx * window + j), lives at pixel ((py + shift) % Hp) * Wp + (px + shift) % Wp of the map and belongs to
    region 3 r(py, Hp) + r(px, Wp), r(c, n) = [c >= n - window] + [c >= n - shift] (all zero for shift = 0)"""
    py, px = torch.arange(Hp, device=device), torch.arange(Wp, device=device)
    pix = ((py + shift) % Hp)[:, None] * Wp + ((px + shift) % Wp)[None, :]
    if shift > 0:
        ry = (py >= Hp - window).long() + (py >= Hp - shift).long()
        rx = (px >= Wp - window).long() + (px >= Wp - shift).long()
        region = 3 * ry[:, None] + rx[None, :]
    else:
        region = torch.zeros(Hp, Wp, dtype=torch.long, device=device)

    def cut(m):
        return m.view(Hp // window, window, Wp // window, window).permute(0, 2, 1, 3).reshape(-1, window * window)
    return cut(pix), cut(region)


def bias_index(window, device=None):
    """(window^2, window^2) int64: (i - i' + window - 1) (2 window - 1) + (j - j' + window - 1) for tokens t = i window + j, t' = i' window + j'"""
    t = torch.arange(window * window, device=device)
    i, j = t // window, t % window
    return (i[:, None] - i[None, :] + window - 1) * (2 * window - 1) + (j[:, None] - j[None, :] + window - 1)


def window_attention_torch(qkv, table, num_heads, window, shift, scale=None):
    """The formula of :func:`window_attention` as torch operations in the operands' dtype (any device): gathers the windows' tokens by
    pixel index, adds bias and the -100 region mask, and scatters the result back.  Differentiable by autograd."""
    B, Hp, Wp, C3 = qkv.shape
    C, N = C3 // 3, window * window
    hd = C // num_heads
    scale = hd ** -0.5 if scale is None else scale
    pix, region = window_pixels(Hp, Wp, window, shift, qkv.device)
    tok = qkv.reshape(B, Hp * Wp, 3, num_heads, hd)[:, pix]                      # (B, windows, N, 3, heads, hd)
    q, k, v = tok[:, :, :, 0], tok[:, :, :, 1], tok[:, :, :, 2]
    score = torch.einsum("bwnhd,bwmhd->bwhnm", q * scale, k)
    score = score + table[bias_index(window, qkv.device)].permute(2, 0, 1)      # (heads, N, N)
    if shift > 0:
        differ = region[:, :, None] != region[:, None, :]                        # (windows, N, N)
        score = score + (differ.to(score.dtype) * -100.0)[None, :, None]
    o = torch.einsum("bwhnm,bwmhd->bwnhd", score.softmax(-1), v).reshape(B, -1, C)
    out = torch.empty(B, Hp * Wp, C, dtype=o.dtype, device=o.device)
    out = out.index_copy(1, pix.reshape(-1), o)
    return out.view(B, Hp, Wp, C)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
def workspace_bytes(B, Hp, Wp, channels, num_heads, window):
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_swin_attn_workspace_bytes(B, Hp, Wp, channels, num_heads, window, ctypes.byref(n)))
    return n.value


def _check_operands(qkv, table, num_heads, window):
    check_bf16(qkv, qkv.shape[-1], "window_attention (qkv)", limited=False)
    if qkv.dim() != 4 or qkv.shape[-1] % 3:
        raise RuntimeError(f"window_attention: qkv (B, Hp, Wp, 3 C), got {tuple(qkv.shape)}")
    if not qkv.is_contiguous():
        raise RuntimeError("window_attention: qkv must be contiguous")
    if table.dim() != 2 or tuple(table.shape) != ((2 * window - 1) ** 2, num_heads):
        raise RuntimeError(f"window_attention: table ((2 window - 1)^2, heads) = {((2 * window - 1) ** 2, num_heads)}, got {tuple(table.shape)}")
    if table.device != qkv.device:
        raise RuntimeError("window_attention: table and qkv on different devices")


class _WindowAttentionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, num_heads, window, shift):
        _check_operands(qkv, table, num_heads, window)
        B, Hp, Wp, C3 = qkv.shape
        C = C3 // 3
        tab = table.detach().float().contiguous()
        out = torch.empty(B, Hp, Wp, C, dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(B, Hp, Wp, num_heads, dtype=torch.float32, device=qkv.device)
        with _lib.on_device(qkv.device):
            _lib.check(_lib.load().msda_swin_attn_forward_bf16(qkv.data_ptr(), tab.data_ptr(), B, Hp, Wp, C, num_heads, window, shift,
                                                               out.data_ptr(), lse.data_ptr(), _lib.raw_stream(qkv.device)))
        ctx.save_for_backward(qkv, tab, out, lse)
        ctx.args = (num_heads, window, shift, table.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, tab, out, lse = ctx.saved_tensors
        num_heads, window, shift, table_dtype = ctx.args
        B, Hp, Wp, C3 = qkv.shape
        C = C3 // 3
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dtable = torch.empty_like(tab)
        ws = torch.empty(workspace_bytes(B, Hp, Wp, C, num_heads, window) // 4, dtype=torch.float32, device=qkv.device)
        with _lib.on_device(qkv.device):
            _lib.check(_lib.load().msda_swin_attn_backward_bf16(qkv.data_ptr(), tab.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(),
                                                                B, Hp, Wp, C, num_heads, window, shift, dqkv.data_ptr(), dtable.data_ptr(),
                                                                ws.data_ptr(), _lib.raw_stream(qkv.device)))
        return dqkv, dtable.to(table_dtype), None, None, None


def window_attention(qkv, table, num_heads, window, shift):
    """qkv (B, Hp, Wp, 3 * 32 * num_heads) bfloat16 on the device, contiguous, Hp and Wp multiples of ``window``; table
    ((2 window - 1)^2, num_heads) -> (B, Hp, Wp, 32 * num_heads) bfloat16.  Gradients for ``qkv`` and ``table``."""
    return _WindowAttentionFunction.apply(qkv, table, num_heads, window, shift)


# ---- the second half of a block ---------------------------------------------------------------------------------------------------------------
class _SwinMlpFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nw, nb, eps, w1, b1, w2, b2, f1, f2):
        x2 = bf16_rows(x, nw.shape[0], "swin_mlp")
        g32 = f32(nw)
        need = any(ctx.needs_input_grad)
        xn, mean, rstd = layernorm_kernel(x2, g32, f32(nb), eps, want_stats=need)
        out, u = gelu_mlp_forward(xn, f1, f2, need, EPI_RESIDUAL, x2)
        if need:
            ctx.save_for_backward(x2, xn, mean, rstd, u, g32)
            ctx.forms = (f1, f2)
            ctx.meta = (x.shape,) + tuple(p.dtype if p is not None else None for p in (nw, nb, w1, b1, w2, b2))
        return out.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x2, xn, mean, rstd, u, g32 = ctx.saved_tensors
        (f1, f2), (shape, nwdt, nbdt, *dtypes) = ctx.forms, ctx.meta
        d2 = bf16_rows(dout, x2.shape[1], "swin_mlp (gradient)")      # (4, 5, 6, 7): w1, b1, w2, b2 among forward's arguments
        dxn, dw1, db1, dw2, db2 = gelu_mlp_backward(ctx, (4, 5, 6, 7), dtypes, d2, xn, u, f1, f2)
        dx, dg, db = layernorm_backward_kernel(dxn, x2, mean, rstd, g32, add=d2, want_gamma=ctx.needs_input_grad[1],
                                               want_beta=ctx.needs_input_grad[2])
        return dx.view(shape) if ctx.needs_input_grad[0] else None, cast(dg, nwdt), cast(db, nbdt), None, dw1, db1, dw2, db2, None, None


def swin_mlp(x, norm, fc1, fc2, caches=(None, None)):
    """``x + fc2(GELU(fc1(norm(x))))`` as ONE autograd function: x (..., C) bfloat16 on the device, ``norm`` an ``nn.LayerNorm(C)``, ``fc1``
    / ``fc2`` ``nn.Linear`` layers (C -> hidden -> C).  Forward: LayerNorm, then ``backbone_ops.gelu_mlp_forward`` with fc2's residual
    epilogue.  Saved for the backward: x, norm(x), the statistics and the pre-activation u -- not h = GELU(u) (the policy of
    ``backbone_ops``); under ``no_grad`` neither u nor the statistics are written."""
    need_layernorm(norm, "swin", "swin_mlp")
    return _SwinMlpFunction.apply(x, norm.weight, norm.bias, float(norm.eps), fc1.weight, fc1.bias, fc2.weight, fc2.bias,
                                  cached_forms(caches[0], fc1.weight, fc1.bias), cached_forms(caches[1], fc2.weight, fc2.bias))


# ---- the merging norm ---------------------------------------------------------------------------------------------------------------------
def merge_norm_kernel(x, H, W, g32, b32, eps, want_stats=True):
    """``msda_swin_merge_norm_forward_bf16``: x (B, H * W, C) bf16 contiguous -> (out (B, H2 * W2, 4 C), mean, rstd)"""
    B, _, C = x.shape
    rows = ((H + 1) // 2) * ((W + 1) // 2)
    out = torch.empty((B, rows, 4 * C), dtype=BF16, device=x.device)
    mean = torch.empty(B * rows, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty_like(mean) if want_stats else None
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_swin_merge_norm_forward_bf16(x.data_ptr(), g32.data_ptr(), b32.data_ptr(), eps, B, H, W, C, out.data_ptr(),
                                                                 ptr(mean), ptr(rstd), _lib.raw_stream(x.device)))
    return out, mean, rstd


def merge_norm_backward_kernel(dy, x, H, W, mean, rstd, g32, want_gamma=True, want_beta=True):
    """``msda_swin_merge_norm_backward_bf16``: dy (B, H2 * W2, 4 C), x (B, H * W, C) -> (dx as x, dgamma, dbeta (4 C) float32 or None)"""
    B, _, C = x.shape
    dx = torch.empty_like(x)
    dg, db, ws = column_sums(want_gamma, want_beta, mean.numel(), 4 * C, x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_swin_merge_norm_backward_bf16(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g32.data_ptr(),
                                                                  B, H, W, C, dx.data_ptr(), ptr(dg), ptr(db), ptr(ws),
                                                                  _lib.raw_stream(x.device)))
    return dx, dg, db


class _SwinMergeNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W, weight, bias, eps):
        x, g32, b32 = token_norm_operands(x, H, W, weight, bias, 4, "swin_merge_norm")
        need = any(ctx.needs_input_grad)
        out, mean, rstd = merge_norm_kernel(x, H, W, g32, b32, eps, want_stats=need)
        if need:
            ctx.save_for_backward(x, mean, rstd, g32)
            ctx.meta = (H, W, weight.dtype, bias.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, mean, rstd, g32 = ctx.saved_tensors
        H, W, wdt, bdt = ctx.meta
        dx, dg, db = merge_norm_backward_kernel(dy.contiguous(), x, H, W, mean, rstd, g32, want_gamma=ctx.needs_input_grad[3],
                                                want_beta=ctx.needs_input_grad[4])
        return dx if ctx.needs_input_grad[0] else None, None, None, cast(dg, wdt), cast(db, bdt), None


def swin_merge_norm(x, H, W, weight, bias, eps=1e-5):
    """The norm of PatchMerging on ``msda_swin_merge_norm_*``: x (B, H * W, C) bfloat16 on the device, C a multiple of 32 up to 1024,
    weight and bias (4 C) -> (B, H2 * W2, 4 C) bfloat16 with H2 = (H + 1) // 2, W2 = (W + 1) // 2: the LayerNorm of the rows whose channel
    q C + c is pixel (2 i + (q & 1), 2 j + (q >> 1)), pixels outside the map being zeros that take part in the statistics (the reference
    pads before the norm).  Saves x and the fp32 statistics (nothing under ``no_grad``); gradients in the parameters' dtypes."""
    return _SwinMergeNormFunction.apply(x, int(H), int(W), weight, bias, float(eps))


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
def _refuse(name, value):
    if value:
        raise NotImplementedError(f"richsem_amd.swin: {name}={value!r} is not supported (only {name}=0 / False)")


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _refuse("drop", drop)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class WindowAttention(nn.Module):
    """``forward(x, shift)``: x (B, Hp, Wp, dim) in map layout, Hp and Wp multiples of the window -> the same shape (qkv, windowed
    attention, proj: proj acts per token, so it commutes with window_reverse)"""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        _refuse("attn_drop", attn_drop)
        _refuse("drop", proj_drop)
        self.dim = dim
        self.window_size = pair(window_size)
        if self.window_size[0] != self.window_size[1]:
            raise NotImplementedError("richsem_amd.swin: square windows only")
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        w = self.window_size[0]
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * w - 1) * (2 * w - 1), num_heads))
        self.register_buffer("relative_position_index", bias_index(w))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    def attend(self, qkv, shift):
        """the kernels on a bf16 device ``qkv`` map (B, Hp, Wp, 3 dim) -> (B, Hp, Wp, dim)"""
        if self.dim != HEAD_DIM * self.num_heads:
            raise RuntimeError(f"richsem_amd.swin: the kernels need head dimension {HEAD_DIM}, got {self.dim // self.num_heads}")
        ratio = self.scale * HEAD_DIM ** 0.5
        if abs(ratio - 1.) > 1e-12:      # a qk_scale of the caller's: into q
            qkv = torch.cat([qkv[..., :self.dim] * ratio, qkv[..., self.dim:]], -1)
        return window_attention(qkv.contiguous(), self.relative_position_bias_table, self.num_heads, self.window_size[0], shift)

    def forward(self, x, shift=0):
        qkv = self.qkv(x)
        if on_kernels(x):
            attn = self.attend(qkv, shift)
        else:
            attn = window_attention_torch(qkv, self.relative_position_bias_table, self.num_heads, self.window_size[0], shift, self.scale)
        return self.proj(attn)


class SwinTransformerBlock(nn.Module):
    """The reference's block.  ``fused`` (a plain attribute, False by default; not a constructor argument, not in the state dict): a bf16
    device tensor runs norm1, qkv, proj + residual and the whole second half on the library's kernels (:func:`swin_layernorm`,
    :func:`swin_linear`, :func:`swin_mlp`) and never falls back -- a missing library or a width outside the kernels' limits raises.  CPU,
    fp32 and fp64 tensors run the torch formula either way.  Stochastic depth is not fused: ``drop_path > 0`` in training mode raises
    NotImplementedError under ``fused`` (``drop_path_rate=0.`` works; so does eval mode)."""

    fused = False

    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        _refuse("drop", drop)
        _refuse("attn_drop", attn_drop)
        self.dim = dim
        self.num_heads = num_heads
        self.window_size = window_size
        self.shift_size = shift_size
        self.mlp_ratio = mlp_ratio
        assert 0 <= self.shift_size < self.window_size, "shift_size must in 0-window_size"
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=pair(window_size), num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                    attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.H = None
        self.W = None
        self._forms = {k: VersionCache() for k in ("qkv", "proj", "fc1", "fc2")}      # derived weight forms of the fused path

    def _forward_fused(self, x):
        B, L, C = x.shape
        H, W, w = self.H, self.W, self.window_size
        refuse_drop_path_in_training(self, "swin")
        need_layernorm(self.norm1, "swin", "block")
        need_erf_gelu(self.mlp.act, "swin")
        attn, shortcut = self.attn, x.contiguous()
        x = swin_layernorm(shortcut, self.norm1.weight, self.norm1.bias, self.norm1.eps).view(B, H, W, C)
        pad_r, pad_b = (w - W % w) % w, (w - H % w) % w
        if pad_r or pad_b:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        x = attn.attend(swin_linear(x, attn.qkv.weight, attn.qkv.bias, cache=self._forms["qkv"]), self.shift_size)
        if pad_r or pad_b:
            x = x[:, :H, :W, :].contiguous()      # proj acts per token: on the cropped map
        x = swin_linear(x.view(B, L, C), attn.proj.weight, attn.proj.bias, epilogue="residual", aux=shortcut, cache=self._forms["proj"])
        return swin_mlp(x, self.norm2, self.mlp.fc1, self.mlp.fc2, caches=(self._forms["fc1"], self._forms["fc2"]))

    def forward(self, x, mask_matrix=None):
        """x (B, H * W, C) with self.H, self.W set by the layer.  ``mask_matrix`` is accepted for the reference's call and not used: the
        regions are computed from the coordinates."""
        B, L, C = x.shape
        H, W, w = self.H, self.W, self.window_size
        assert L == H * W, "input feature has wrong size"
        if self.fused and on_kernels(x):
            return self._forward_fused(x)
        shortcut = x
        x = self.norm1(x).view(B, H, W, C)
        pad_r, pad_b = (w - W % w) % w, (w - H % w) % w
        if pad_r or pad_b:
            x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))      # zeros AFTER the norm: padded tokens carry the qkv bias, as the reference's
        x = self.attn(x, self.shift_size)
        if pad_r or pad_b:
            x = x[:, :H, :W, :].contiguous()
        x = shortcut + self.drop_path(x.view(B, H * W, C))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    """The reference's layer.  ``fused`` (a plain attribute, False by default; ``SwinTransformer.set_fused_stages``): a bf16 device tensor
    takes :func:`swin_merge_norm` -- pad, 2 x 2 gather and LayerNorm in one pass over the map -- and :func:`swin_linear` for the reduction,
    and never falls back: a ``norm_layer`` other than nn.LayerNorm or a width outside the kernels' limits raises."""

    fused = False

    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)
        self._forms = VersionCache()      # derived weight forms of the fused path

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        if self.fused and on_kernels(x):
            need_layernorm(self.norm, "swin", "PatchMerging")
            xn = swin_merge_norm(x, H, W, self.norm.weight, self.norm.bias, self.norm.eps)
            return swin_linear(xn, self.reduction.weight, None, cache=self._forms)
        x = x.view(B, H, W, C)
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        H2, W2 = (H + 1) // 2, (W + 1) // 2
        # (B, H2, dy, W2, dx, C) -> channels ordered (dx, dy, C): the reference's cat of (0,0), (1,0), (0,1), (1,1) as (row, column) offsets
        x = x.view(B, H2, 2, W2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(B, H2 * W2, 4 * C)
        return self.reduction(self.norm(x))


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        _refuse("use_checkpoint", use_checkpoint)
        _refuse("drop", drop)
        _refuse("attn_drop", attn_drop)
        self.window_size = window_size
        self.shift_size = window_size // 2
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size, shift_size=0 if i % 2 == 0 else window_size // 2,
                                 mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path, norm_layer=norm_layer)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def set_fused(self, flag=True):
        """``fused`` of every block (:class:`SwinTransformerBlock`)"""
        for blk in self.blocks:
            blk.fused = bool(flag)
        return self

    def forward(self, x, H, W):
        """x (B, H * W, C) -> (x, H, W, x_down, Wh, Ww) as the reference"""
        for blk in self.blocks:
            blk.H, blk.W = H, W
            x = blk(x)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    """The reference's layer: ``forward(x)`` -> (B, embed_dim, Wh, Ww); ``tokens(x)`` -> (x (B, Wh * Ww, embed_dim), Wh, Ww), the same
    numbers in the layout the first block reads.  ``fused`` (a plain attribute, False by default; ``SwinTransformer.set_fused_stages``): a
    bf16 device image takes :func:`swin_patch_rows`, the projection as :func:`swin_linear` on the zero-padded (embed_dim, Kp) form of the
    convolution weight, and :func:`swin_layernorm`; it never falls back (a ``norm_layer`` other than nn.LayerNorm, or an ``embed_dim`` that
    is no multiple of 32, raises)."""

    fused = False

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = pair(patch_size)
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None
        self._forms = VersionCache()      # the zero-padded (embed_dim, Kp) weight forms of the fused path

    def tokens(self, x):
        """x (B, in_chans, H, W) -> (tokens (B, Wh * Ww, embed_dim), Wh, Ww): projection and norm, without the NCHW detour"""
        if self.fused and on_kernels(x):
            if self.norm is not None:
                need_layernorm(self.norm, "swin", "PatchEmbed")
            Wh, Ww = patch_grid(x.shape[2], x.shape[3], self.patch_size)
            t = patch_linear(swin_patch_rows(x, self.patch_size), self.proj.weight, self.proj.bias, self._forms)
            if self.norm is not None:
                t = swin_layernorm(t, self.norm.weight, self.norm.bias, self.norm.eps)
            return t, Wh, Ww
        _, _, H, W = x.shape
        ph, pw = self.patch_size
        if W % pw or H % ph:
            x = F.pad(x, (0, (pw - W % pw) % pw, 0, (ph - H % ph) % ph))
        x = self.proj(x)
        Wh, Ww = x.shape[2], x.shape[3]
        x = x.flatten(2).transpose(1, 2)
        return (self.norm(x) if self.norm is not None else x), Wh, Ww

    def forward(self, x):
        t, Wh, Ww = self.tokens(x)
        return t.transpose(1, 2).reshape(-1, self.embed_dim, Wh, Ww)


class SwinTransformer(nn.Module):
    """``forward_raw(images)`` -> the tuple of (B, C_i, H_i, W_i) features of ``out_indices``; ``forward(images, mask)`` -> a list of
    (feature, mask) pairs with the padding mask (B, H, W) bool interpolated to each level as the reference's NestedTensor wrapper does.
    ``fused_stages`` (a plain attribute, False by default; :meth:`set_fused_stages`): on a bf16 device tensor the output norms take
    :func:`swin_norm_nchw` and, with ``ape`` off, the patch embedding's tokens go straight to the first layer."""

    fused_stages = False

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1, dilation=False,
                 use_checkpoint=False):
        super().__init__()
        _refuse("use_checkpoint", use_checkpoint)
        _refuse("drop_rate", drop_rate)
        _refuse("attn_drop_rate", attn_drop_rate)
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.ape = ape
        self.patch_norm = patch_norm
        self.out_indices = out_indices
        self.frozen_stages = frozen_stages
        self.dilation = dilation
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None)
        if ape:
            size, patch = pair(pretrain_img_size), pair(patch_size)
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, size[0] // patch[0], size[1] // patch[1]))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=.02)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        downsample = [PatchMerging] * self.num_layers
        downsample[-1] = None
        num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        if dilation:
            downsample[-2] = None
            num_features[-1] = int(embed_dim * 2 ** (self.num_layers - 1)) // 2
        self.layers = nn.ModuleList([
            BasicLayer(dim=num_features[i], depth=depths[i], num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio,
                       qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer, downsample=downsample[i],
                       use_checkpoint=use_checkpoint)
            for i in range(self.num_layers)])
        self.num_features = num_features
        for i in out_indices:
            self.add_module(f"norm{i}", norm_layer(num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 1 and self.ape:
            self.absolute_pos_embed.requires_grad = False
        if self.frozen_stages >= 2:
            for i in range(0, self.frozen_stages - 1):
                m = self.layers[i]
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def set_fused(self, flag=True):
        """``fused`` of every block of every layer (:class:`SwinTransformerBlock`)"""
        for layer in self.layers:
            layer.set_fused(flag)
        return self

    def set_fused_stages(self, flag=True):
        """the stage boundaries' switch: ``fused`` of the patch embedding and of every layer's ``downsample`` and ``fused_stages`` (the
        output norms).  The blocks' ``fused`` is :meth:`set_fused`'s alone."""
        flag = bool(flag)
        self.patch_embed.fused = flag
        for layer in self.layers:
            if layer.downsample is not None:
                layer.downsample.fused = flag
        self.fused_stages = flag
        return self

    def forward_raw(self, x):
        if self.fused_stages and not self.ape:      # the tokens go straight to the first layer
            x, Wh, Ww = self.patch_embed.tokens(x)
        else:
            x = self.patch_embed(x)
            Wh, Ww = x.shape[2], x.shape[3]
            if self.ape:
                x = x + F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode="bicubic")
            x = x.flatten(2).transpose(1, 2)
        outs = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                outs.append(output_norm_nchw(getattr(self, f"norm{i}"), x_out, H, W, self.fused_stages, "swin"))
        return tuple(outs)

    def forward(self, images, mask):
        return mask_pyramid(self.forward_raw(images), mask)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self
