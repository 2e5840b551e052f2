"""The operators more than one backbone runs on: the leaf module under swin.py, convnext.py and focalnet.py, which import from it and never
from one another ("The Python host layer"; tests/test_backbone_host_layer.py holds the layering).

* the raw calls of ``msda_swin_linear_bf16``, ``msda_swin_layernorm_*``, ``msda_swin_norm_nchw_*``, ``msda_swin_patch_rows_*`` and
  ``msda_layer_scale_*``, each the ONE call site of its entry point, and the autograd functions over them;
* THE GELU-MLP POLICY, stated once (:func:`gelu_mlp_forward`, :func:`gelu_mlp_backward`): the pre-activation ``u`` is saved, the hidden
  activation ``h = GELU(u)`` is not; the backward regenerates it, and only when fc2's weight gradient needs it;
* the host plumbing: the operand check of bf16 rows, the predicate :func:`on_kernels`, :func:`wgrad`, :func:`cast`, the fused-path guards.

bf16 tensors on the device take the kernels and never fall back: a missing library or a width outside the kernels' limits raises.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_GELU_BACKWARD = 0, 1, 2, 3      # `epilogue` of msda_swin_linear_bf16 (include/richsem_msda.h)
BF16 = torch.bfloat16
MAX_C = 4096      # the widest rows of the norm, scale, convolution and modulate kernels (include/richsem_msda.h)


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def ptr(t):
    return t.data_ptr() if t is not None else None


def f32(p):
    return p.detach().float().contiguous()


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def cast(g, dtype):
    """a gradient in its parameter's dtype; None (not wanted) stays None"""
    return g.to(dtype) if g is not None else None


def on_kernels(x):
    """THE predicate of the device paths: a bfloat16 tensor on the device"""
    return x.is_cuda and x.dtype == BF16


def kernel_width(C):
    """the width rule of the norm, scale, convolution and modulate kernels"""
    return C % 32 == 0 and 32 <= C <= MAX_C


def check_bf16(t, width, what, limited=True):
    """THE operand check of the row kernels: t (..., width) bfloat16 on the device, or it raises.  ``limited``: the width obeys
    :func:`kernel_width`; the linear layer's K and N do not (the library checks them: multiples of 32 up to 8192)"""
    if t.dim() < 1 or t.shape[-1] != width or (limited and not kernel_width(width)):
        rule = f" with C a multiple of 32 in [32, {MAX_C}]" if limited else ""
        raise RuntimeError(f"{what}: (..., C){rule}, got {tuple(t.shape)} for C = {width}")
    if t.dtype != BF16:
        raise RuntimeError(f"{what}: bfloat16, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError("Not implemented on the CPU")


def bf16_rows(t, width, what, limited=True):
    """t, checked (:func:`check_bf16`) -> (rows, width) contiguous"""
    check_bf16(t, width, what, limited)
    return t.reshape(-1, width).contiguous()


def check_vector(v, C, device, what):
    if v is not None and (v.dtype != torch.float32 or tuple(v.shape) != (C,) or v.device != device or not v.is_contiguous()):
        raise RuntimeError(f"{what}: float32 ({C}) on {device}, got {v.dtype} {tuple(v.shape)} on {v.device}")


# ---- the raw calls: one call site per entry point ---------------------------------------------------------------------------------------------
def linear_kernel(x2, w16, b32=None, epilogue=EPI_BIAS, aux=None, want_out2=False):
    """One call of ``msda_swin_linear_bf16`` (no autograd): x2 (tokens, K), w16 (N, K), aux (tokens, N) bf16 contiguous on the device, b32 (N)
    float32 or None -> (out, out2), both (tokens, N) bf16; out2 is None unless ``want_out2`` (epilogues 1 and 3 write it)."""
    T, K = x2.shape
    N = w16.shape[0]
    bias_ok = b32 is None or (b32.dtype == torch.float32 and b32.numel() == N and b32.is_contiguous())
    if w16.dtype != BF16 or w16.shape[1] != K or not w16.is_contiguous() or not bias_ok:
        raise RuntimeError(f"swin_linear: weight bfloat16 (N, {K}) contiguous and bias float32 (N), got {w16.dtype} {tuple(w16.shape)}")
    if aux is not None and (aux.dtype != BF16 or tuple(aux.shape) != (T, N) or not aux.is_contiguous()):
        raise RuntimeError(f"swin_linear: aux bfloat16 ({T}, {N}) contiguous, got {aux.dtype} {tuple(aux.shape)}")
    out = torch.empty((T, N), dtype=BF16, device=x2.device)
    out2 = torch.empty_like(out) if want_out2 else None
    with _lib.on_device(x2.device):
        _lib.check(_lib.load().msda_swin_linear_bf16(x2.data_ptr(), w16.data_ptr(), ptr(b32), ptr(aux), epilogue, T, K, N, out.data_ptr(),
                                                     ptr(out2), _lib.raw_stream(x2.device)))
    return out, out2


def layernorm_workspace_bytes(tokens, C):
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_swin_layernorm_workspace_bytes(tokens, C, ctypes.byref(n)))
    return n.value


def column_sums(want_gamma, want_beta, tokens, C, device):
    """(dgamma, dbeta, workspace) of a backward with column sums over ``tokens`` rows: float32, None where not wanted"""
    dg = torch.empty(C, dtype=torch.float32, device=device) if want_gamma else None
    db = torch.empty(C, dtype=torch.float32, device=device) if want_beta else None
    ws = torch.empty(layernorm_workspace_bytes(tokens, C) // 4, dtype=torch.float32, device=device) if want_gamma or want_beta else None
    return dg, db, ws


def layernorm_kernel(x2, g32, b32, eps, want_stats=True):
    """``msda_swin_layernorm_forward_bf16``: x2 (tokens, C) bf16 -> (out, mean, rstd); the statistics are None unless ``want_stats``"""
    T, C = x2.shape
    out = torch.empty_like(x2)
    mean = torch.empty(T, dtype=torch.float32, device=x2.device) if want_stats else None
    rstd = torch.empty_like(mean) if want_stats else None
    with _lib.on_device(x2.device):
        _lib.check(_lib.load().msda_swin_layernorm_forward_bf16(x2.data_ptr(), g32.data_ptr(), b32.data_ptr(), eps, T, C, out.data_ptr(),
                                                                ptr(mean), ptr(rstd), _lib.raw_stream(x2.device)))
    return out, mean, rstd


def layernorm_backward_kernel(dy2, x2, mean, rstd, g32, add=None, want_gamma=True, want_beta=True):
    """``msda_swin_layernorm_backward_bf16`` -> (dx bf16, dgamma float32 or None, dbeta float32 or None)"""
    T, C = x2.shape
    dx = torch.empty_like(x2)
    dg, db, ws = column_sums(want_gamma, want_beta, T, C, x2.device)
    with _lib.on_device(x2.device):
        _lib.check(_lib.load().msda_swin_layernorm_backward_bf16(dy2.data_ptr(), x2.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g32.data_ptr(),
                                                                 ptr(add), T, C, dx.data_ptr(), ptr(dg), ptr(db), ptr(ws),
                                                                 _lib.raw_stream(x2.device)))
    return dx, dg, db


def norm_nchw_kernel(x, g32, b32, eps, want_stats=True):
    """``msda_swin_norm_nchw_forward_bf16``: x (B, HW, C) bf16 contiguous -> (out (B, C, HW), mean, rstd)"""
    B, HW, C = x.shape
    out = torch.empty((B, C, HW), dtype=BF16, device=x.device)
    mean = torch.empty(B * HW, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty_like(mean) if want_stats else None
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_swin_norm_nchw_forward_bf16(x.data_ptr(), g32.data_ptr(), b32.data_ptr(), eps, B, HW, C, out.data_ptr(),
                                                                ptr(mean), ptr(rstd), _lib.raw_stream(x.device)))
    return out, mean, rstd


def norm_nchw_backward_kernel(dy, x, mean, rstd, g32, want_gamma=True, want_beta=True):
    """``msda_swin_norm_nchw_backward_bf16``: dy (B, C, HW), x (B, HW, C) -> (dx as x, dgamma, dbeta (C) float32 or None)"""
    B, HW, C = x.shape
    dx = torch.empty_like(x)
    dg, db, ws = column_sums(want_gamma, want_beta, B * HW, C, x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_swin_norm_nchw_backward_bf16(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g32.data_ptr(),
                                                                 B, HW, C, dx.data_ptr(), ptr(dg), ptr(db), ptr(ws),
                                                                 _lib.raw_stream(x.device)))
    return dx, dg, db


def layer_scale_kernel(z, g32, res):
    """``msda_layer_scale_forward_bf16``: z, res (..., C) bf16 on the device, g32 (C) float32 -> rnd(res + gamma z) in z's shape"""
    C = g32.shape[0]
    z2, r2 = bf16_rows(z, C, "layer_scale"), bf16_rows(res, C, "layer_scale (res)")
    check_vector(g32, C, z.device, "layer_scale (gamma)")
    if r2.shape != z2.shape or res.device != z.device:
        raise RuntimeError(f"layer_scale: res {tuple(z.shape)} on {z.device}, got {tuple(res.shape)} on {res.device}")
    out = torch.empty_like(z2)
    with _lib.on_device(z.device):
        _lib.check(_lib.load().msda_layer_scale_forward_bf16(z2.data_ptr(), g32.data_ptr(), r2.data_ptr(), z2.shape[0], C, out.data_ptr(),
                                                             _lib.raw_stream(z.device)))
    return out.view(z.shape)


def layer_scale_backward_kernel(dout, z, g32, want_gamma=True):
    """``msda_layer_scale_backward_bf16`` -> (dz = rnd(gamma dout) in dout's shape, dgamma (C) float32 or None)"""
    C = g32.shape[0]
    d2 = bf16_rows(dout, C, "layer_scale (gradient)")
    z2 = bf16_rows(z, C, "layer_scale") if want_gamma else None
    check_vector(g32, C, dout.device, "layer_scale (gamma)")
    if z2 is not None and (z2.shape != d2.shape or z.device != dout.device):
        raise RuntimeError(f"layer_scale: z {tuple(dout.shape)} on {dout.device}, got {tuple(z.shape)} on {z.device}")
    T = d2.shape[0]
    dz = torch.empty_like(d2)
    dg, _, ws = column_sums(want_gamma, False, T, C, dout.device)
    with _lib.on_device(dout.device):
        _lib.check(_lib.load().msda_layer_scale_backward_bf16(d2.data_ptr(), ptr(z2), g32.data_ptr(), T, C, dz.data_ptr(), ptr(dg), ptr(ws),
                                                              _lib.raw_stream(dout.device)))
    return dz.view(dout.shape), dg


# ---- weight forms and gradients ---------------------------------------------------------------------------------------------------------------
def linear_forms(weight, bias):
    """the forms the kernels read a linear layer from: ``w16`` (N, K) bf16, ``wt16`` (K, N) bf16 (the input gradient is the same kernel on
    the transposed weight), ``b32`` float32 or None.  Kept per parameter version in a :class:`richsem_amd.param_cache.VersionCache`."""
    w16 = weight.detach().to(BF16).contiguous()
    return {"w16": w16, "wt16": w16.t().contiguous(), "b32": f32(bias) if bias is not None else None}


def cached_forms(cache, weight, bias, build=None):
    """:func:`linear_forms` of a layer, kept in ``cache`` (a VersionCache, or None) per version of its parameters.  ``build``: what makes the
    forms where they are not the parameters' own (a convolution weight flattened and zero-padded)"""
    build = build or (lambda: linear_forms(weight, bias))
    return build() if cache is None else cache.get([weight] + ([bias] if bias is not None else []), build)


def wgrad(ctx, iw, ib, dy2, x2, weight_dtype, bias_dtype):
    """(dW, db) of one layer by the package's weight-gradient rule, in the parameters' dtypes; None where ``ctx.needs_input_grad`` at the
    positions ``iw``, ``ib`` does not want them"""
    from .functions.linear import linear_bgrad, linear_wgrad
    want_b = bias_dtype is not None and ctx.needs_input_grad[ib]
    dw = db = None
    if ctx.needs_input_grad[iw]:
        dw, db = linear_wgrad(dy2, x2, want_b)
        dw = dw.to(weight_dtype)
    elif want_b:
        db = linear_bgrad(dy2)
    return dw, (db.to(bias_dtype) if want_b else None)


def depthwise_weight_grads(dw, metas, wanted):
    """the inverse of ``dwconv7_weight_form`` / ``focal_weight_form``: dw (sum K_l^2, C) float32, tap-major, level after level -> per level the
    gradient as its parameter is, (C, 1, K_l, K_l) in its dtype (``metas``: (dtype, shape) per level); None where not ``wanted``"""
    grads, row = [], 0
    for (dtype, shape), want in zip(metas, wanted):
        taps = shape[-2] * shape[-1]
        grads.append(dw[row:row + taps].t().reshape(shape).to(dtype) if want else None)
        row += taps
    return tuple(grads)


# ---- the GELU MLP: u is saved, h = GELU(u) regenerated ----------------------------------------------------------------------------------------
def gelu_mlp_forward(xn, f1, f2, need, epilogue, aux=None):
    """fc1 with the GELU epilogue, fc2 with ``epilogue`` (bias, or residual with ``aux`` the rows to add): xn (tokens, C) -> (out, u).  The
    pre-activation u is written only when a backward will run (``need``); h = GELU(u) is never returned: nobody may save it"""
    h, u = linear_kernel(xn, f1["w16"], f1["b32"], EPI_GELU, want_out2=need)
    out, _ = linear_kernel(h, f2["w16"], f2["b32"], epilogue, aux)
    return out, u


def gelu_mlp_backward(ctx, where, dtypes, d2, xn, u, f1, f2, want_dxn=True):
    """-> (dxn, dw1, db1, dw2, db2) from d2, the gradient of fc2's output rows.  ``where``: the positions of (w1, b1, w2, b2) in the caller's
    ``ctx.needs_input_grad`` -- each caller states its layout once, here; ``dtypes``: theirs.  (du, h) come from ONE call, the epilogue
    du = (d2 W2) gelu'(u), which writes h = GELU(u) only when fc2's weight gradient needs it"""
    iw1, ib1, iw2, ib2 = where
    du, h = linear_kernel(d2, f2["wt16"], None, EPI_GELU_BACKWARD, u, want_out2=ctx.needs_input_grad[iw2])
    dw2, db2 = wgrad(ctx, iw2, ib2, d2, h, dtypes[2], dtypes[3])
    dw1, db1 = wgrad(ctx, iw1, ib1, du, xn, dtypes[0], dtypes[1])
    dxn = linear_kernel(du, f1["wt16"])[0] if want_dxn else None
    return dxn, dw1, db1, dw2, db2


# ---- the autograd functions -------------------------------------------------------------------------------------------------------------------
class _SwinLinearFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, aux, forms):
        K = forms["w16"].shape[1]      # (weight.shape[1], or the padded width of a convolution weight's form: PatchEmbed)
        x2 = bf16_rows(x, K, "swin_linear", limited=False)
        aux2 = bf16_rows(aux, weight.shape[0], "swin_linear (aux)", limited=False) if aux is not None else None
        out, _ = linear_kernel(x2, forms["w16"], forms["b32"], EPI_RESIDUAL if aux is not None else EPI_BIAS, aux2)
        ctx.save_for_backward(x2)
        ctx.forms = forms
        ctx.meta = (x.shape, aux.shape if aux is not None else None, weight.dtype, bias.dtype if bias is not None else None, weight.shape)
        return out.view(x.shape[:-1] + (weight.shape[0],))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x2, = ctx.saved_tensors
        shape, aux_shape, wdt, bdt, wshape = ctx.meta
        dy2 = bf16_rows(dy, ctx.forms["w16"].shape[0], "swin_linear (gradient)", limited=False)
        dx = linear_kernel(dy2, ctx.forms["wt16"])[0].view(shape) if ctx.needs_input_grad[0] else None
        dw, db = wgrad(ctx, 1, 2, dy2, x2, wdt, bdt)
        if dw is not None and dw.shape != wshape:      # the columns of padding are dropped
            dw = dw[:, :wshape.numel() // wshape[0]].reshape(wshape)
        return dx, dw, db, dy.reshape(aux_shape) if ctx.needs_input_grad[3] else None, None


def linear_on_forms(x, weight, bias, forms, aux=None):
    """:func:`swin_linear` on forms the caller made (:func:`cached_forms` with a ``build``): ``forms["w16"]`` (N, Kp) may be wider than
    ``weight.flatten(1)`` -- x then has Kp columns and the weight gradient's columns of padding are dropped -- and ``weight`` may be a
    differentiable view or padding of the parameter, whose gradient autograd carries on"""
    return _SwinLinearFunction.apply(x, weight, bias, aux, forms)


def swin_linear(x, weight, bias=None, epilogue=None, aux=None, cache=None):
    """``x weight^T + bias`` (``epilogue=None``) or ``x weight^T + bias + aux`` (``epilogue="residual"``, the sum rounded once) on
    ``msda_swin_linear_bf16``: x (..., K) bfloat16 on the device, weight (N, K), K and N multiples of 32 up to 8192 -> (..., N) bfloat16.
    The input gradient is the same kernel on ``weight^T``; weight and bias gradients are ``functions.linear.linear_wgrad``'s, returned in
    the parameters' dtypes.  ``cache``: a VersionCache that keeps the derived weight forms (:func:`linear_forms`) per parameter version.
    The GELU epilogues belong to :func:`gelu_mlp_forward` (raw: :func:`linear_kernel`)."""
    if epilogue not in (None, "residual") or (epilogue == "residual") != (aux is not None):
        raise ValueError(f"swin_linear: epilogue None or 'residual' (with aux), got {epilogue!r}" + (" with aux" if aux is not None else ""))
    return _SwinLinearFunction.apply(x, weight, bias, aux, cached_forms(cache, weight, bias))


class _SwinLayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x2 = bf16_rows(x, weight.shape[0], "swin_layernorm")
        g32 = f32(weight)
        need = any(ctx.needs_input_grad)
        out, mean, rstd = layernorm_kernel(x2, g32, f32(bias), eps, want_stats=need)
        if need:
            ctx.save_for_backward(x2, mean, rstd, g32)
            ctx.meta = (x.shape, weight.dtype, bias.dtype)
        return out.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x2, mean, rstd, g32 = ctx.saved_tensors
        shape, wdt, bdt = ctx.meta
        dx, dg, db = layernorm_backward_kernel(bf16_rows(dy, x2.shape[1], "swin_layernorm (gradient)"), x2, mean, rstd, g32,
                                               want_gamma=ctx.needs_input_grad[1], want_beta=ctx.needs_input_grad[2])
        return dx.view(shape) if ctx.needs_input_grad[0] else None, cast(dg, wdt), cast(db, bdt), None


def swin_layernorm(x, weight, bias, eps=1e-5):
    """LayerNorm over the last dimension (C a multiple of 32 up to 4096) on ``msda_swin_layernorm_*``: x (..., C) bfloat16 on the device,
    weight and bias (C) -> bfloat16.  Saves x and the fp32 statistics (nothing under ``no_grad``); gradients in the parameters' dtypes."""
    return _SwinLayerNormFunction.apply(x, weight, bias, float(eps))


def token_norm_operands(x, H, W, weight, bias, pixels, what):
    """the operands of a norm over ``pixels`` gathered pixels of a token map: x (B, H * W, C) bfloat16 on the device, weight and bias
    (pixels C) -> (x contiguous, weight and bias float32)"""
    check_bf16(x, x.shape[-1], what, limited=False)
    if x.dim() != 3 or x.shape[1] != H * W:
        raise RuntimeError(f"{what}: (B, {H} * {W}, C), got {tuple(x.shape)}")
    width = pixels * x.shape[2]
    if weight is None or bias is None or tuple(weight.shape) != (width,) or tuple(bias.shape) != (width,):
        raise RuntimeError(f"{what}: weight and bias ({width})")
    return x.contiguous(), f32(weight), f32(bias)


class _SwinNormNchwFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, H, W, weight, bias, eps):
        x, g32, b32 = token_norm_operands(x, H, W, weight, bias, 1, "swin_norm_nchw")
        need = any(ctx.needs_input_grad)
        out, mean, rstd = norm_nchw_kernel(x, g32, b32, eps, want_stats=need)
        if need:
            ctx.save_for_backward(x, mean, rstd, g32)
            ctx.meta = (weight.dtype, bias.dtype)
        return out.view(x.shape[0], x.shape[2], H, W)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, mean, rstd, g32 = ctx.saved_tensors
        wdt, bdt = ctx.meta
        dx, dg, db = norm_nchw_backward_kernel(dy.contiguous(), x, mean, rstd, g32, want_gamma=ctx.needs_input_grad[3],
                                               want_beta=ctx.needs_input_grad[4])
        return dx if ctx.needs_input_grad[0] else None, None, None, cast(dg, wdt), cast(db, bdt), None


def swin_norm_nchw(x, H, W, weight, bias, eps=1e-5):
    """An output norm of a backbone on ``msda_swin_norm_nchw_*``: x (B, H * W, C) bfloat16 on the device, C a multiple of 32 up to 4096,
    weight and bias (C) -> (B, C, H, W) bfloat16 contiguous: LayerNorm over C, stored transposed (any H * W).  Saves x and the fp32
    statistics (nothing under ``no_grad``); gradients in the parameters' dtypes."""
    return _SwinNormNchwFunction.apply(x, int(H), int(W), weight, bias, float(eps))


def patch_grid(H, W, patch_size):
    """-> (Wh, Ww) = (ceil(H / ph), ceil(W / pw))"""
    ph, pw = pair(patch_size)
    return -(-H // ph), -(-W // pw)


def patch_width(in_chans, patch_size):
    """Kp: in_chans ph pw rounded up to a multiple of 32"""
    ph, pw = pair(patch_size)
    return -(-in_chans * ph * pw // 32) * 32


class _SwinPatchRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, ph, pw):
        check_bf16(img, img.shape[-1], "swin_patch_rows", limited=False)
        if img.dim() != 4:
            raise RuntimeError(f"swin_patch_rows: an image (B, Cin, H, W), got {tuple(img.shape)}")
        img = img.contiguous()
        B, Cin, H, W = img.shape
        Wh, Ww = patch_grid(H, W, (ph, pw))
        rows = torch.empty((B, Wh * Ww, patch_width(Cin, (ph, pw))), dtype=BF16, device=img.device)
        with _lib.on_device(img.device):
            _lib.check(_lib.load().msda_swin_patch_rows_bf16(img.data_ptr(), B, Cin, H, W, ph, pw, rows.data_ptr(), _lib.raw_stream(img.device)))
        ctx.meta = (tuple(img.shape), ph, pw)
        return rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, drows):
        (B, Cin, H, W), ph, pw = ctx.meta
        drows = drows.contiguous()
        dimg = torch.empty((B, Cin, H, W), dtype=BF16, device=drows.device)
        with _lib.on_device(drows.device):
            _lib.check(_lib.load().msda_swin_patch_rows_backward_bf16(drows.data_ptr(), B, Cin, H, W, ph, pw, dimg.data_ptr(),
                                                                      _lib.raw_stream(drows.device)))
        return dimg, None, None


def swin_patch_rows(img, patch_size):
    """The image as rows of patches on ``msda_swin_patch_rows_*``: img (B, Cin, H, W) bfloat16 on the device -> (B, Wh * Ww, Kp) bfloat16,
    Wh = ceil(H / ph), Ww = ceil(W / pw), Kp = Cin ph pw rounded up to a multiple of 32 (at most 8192); column (c ph + dy) pw + dx is the
    image element (the order of ``proj.weight.flatten(1)``), columns of padding and pixels past the image are exact zeros.  Saves nothing;
    the backward (run only when the image needs a gradient) is the inverse movement."""
    ph, pw = pair(patch_size)
    return _SwinPatchRowsFunction.apply(img, int(ph), int(pw))


def patch_linear(rows, weight, bias, cache):
    """a patch convolution as a product over the rows (B, tokens, Kp) of :func:`swin_patch_rows`: on ``weight.flatten(1)`` zero-padded to (N, Kp)"""
    def build():
        flat = weight.detach().to(BF16).flatten(1)
        return linear_forms(F.pad(flat, (0, rows.shape[-1] - flat.shape[1])), bias)
    return linear_on_forms(rows, weight, bias, cached_forms(cache, weight, bias, build))


class _LayerScaleFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, gamma, res):
        g32 = f32(gamma)
        out = layer_scale_kernel(z, g32, res)
        ctx.save_for_backward(z if ctx.needs_input_grad[1] else None, g32)
        ctx.meta = gamma.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        z, g32 = ctx.saved_tensors
        dz = dg = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dz, dg = layer_scale_backward_kernel(dout, z, g32, want_gamma=ctx.needs_input_grad[1])
        return dz if ctx.needs_input_grad[0] else None, cast(dg, ctx.meta), dout if ctx.needs_input_grad[2] else None


def layer_scale(z, gamma, res):
    """``res + gamma * z``, the sum rounded once: z, res (..., C), gamma (C).  bf16 device tensors take ``msda_layer_scale_*`` (dz = gamma
    dout, dgamma = sum dout z in a fixed order, the residual's gradient is dout itself); any other tensor runs the torch formula."""
    if gamma.dim() != 1 or z.shape[-1] != gamma.shape[0] or res.shape != z.shape:
        raise RuntimeError(f"layer_scale: z and res (..., C) and gamma (C), got {tuple(z.shape)}, {tuple(res.shape)} and {tuple(gamma.shape)}")
    if not on_kernels(z):
        return res + gamma * z
    return _LayerScaleFunction.apply(z, gamma, res)


# ---- the mirrors' shared pieces ---------------------------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """per-sample stochastic depth on the residual branch (timm's DropPath, which the reference imports)"""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1. - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x / keep * mask


def need_layernorm(norm, module, what):
    if not isinstance(norm, nn.LayerNorm) or not norm.elementwise_affine or norm.bias is None:
        raise NotImplementedError(f"richsem_amd.{module}: the fused {what} needs an nn.LayerNorm with weight and bias, got {type(norm).__name__}")


def need_erf_gelu(act, module):
    if not isinstance(act, nn.GELU) or getattr(act, "approximate", "none") != "none":
        raise NotImplementedError(f"richsem_amd.{module}: fused blocks need the erf form of nn.GELU, got {act!r}")


def refuse_drop_path_in_training(block, module):
    """stochastic depth is not fused: ``drop_path > 0`` in training mode raises (``drop_path_rate=0.`` works; so does eval mode)"""
    if isinstance(block.drop_path, DropPath) and block.drop_path.drop_prob > 0. and block.training:
        raise NotImplementedError(f"richsem_amd.{module}: fused blocks do not implement stochastic depth in training mode (drop_path_rate=0.)")


def output_norm_nchw(norm, x, H, W, fused, module):
    """an output norm of a backbone: x (B, H * W, C) -> (B, C, H, W) contiguous.  ``fused`` on a bf16 device tensor: :func:`swin_norm_nchw`,
    never a fallback (a ``norm`` other than nn.LayerNorm raises); else ``norm`` itself and a permuted copy"""
    if fused and on_kernels(x):
        need_layernorm(norm, module, "output norm")
        return swin_norm_nchw(x, H, W, norm.weight, norm.bias, norm.eps)
    return norm(x).view(-1, H, W, x.shape[-1]).permute(0, 3, 1, 2).contiguous()


def mask_pyramid(outs, mask):
    """the features with the padding mask (B, H, W) bool interpolated to each level, as the reference's NestedTensor wrapper does"""
    assert mask is not None
    return [(o, F.interpolate(mask[None].float(), size=o.shape[-2:]).to(torch.bool)[0]) for o in outs]
