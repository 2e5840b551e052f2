"""The FocalNet backbone on the library's kernels.

Reference: models/richsem/focal.py (``build_backbone`` takes it for ``focalnet_L_384_22k``, ``focalnet_L_384_22k_fl4``,
``focalnet_XL_384_22k`` and ``focalnet_H_224_22k_fl4_fd``: models/richsem/backbone.py:238-244).  (The file is not called ``focal.py``: that
is the focal loss here.)  A block is ``x + gamma_1 * norm1(modulation(x))`` and ``x + gamma_2 * norm2(mlp(x))`` (post-LN; pre-LN with the
norms in front), and the modulation is ``proj(q * h(A))`` with ``q, ctx0, gates = split(f(x))`` and the hierarchical context aggregation

    u_l = dwconv_{K_l}(ctx_{l-1}),  ctx_l = GELU(u_l),  K_l = focal_window + 2 l,  l = 0 .. L-1        (no bias, zero padding per image)
    m   = mean over the image of ctx_{L-1},  g = GELU(m)
    A   = s (sum_{l<L} gate_l ctx_l + gate_L g),   s = 1 / (L + 1) with normalize_modulator, else 1

* :func:`focal_context` -- ``A`` from ``ctx0``, ``gates`` and the depthwise weights, one autograd function over csrc/focalnet_ctx.hip (C ABI
  ``msda_fmod_context_*``): only the pre-activations ``u_l`` are kept between levels, the backward runs the flipped convolutions with the
  gate and ``GELU'`` epilogues and the weight gradients with a fixed summation order.
* :func:`modulate` -- ``q * mod`` and its two gradients (``msda_fmod_modulate_*``).

THE RULE, stated once (:func:`kernel_path`): a bfloat16 tensor on the device whose shape the kernels support -- ``C`` a multiple of 32 in
[32, 4096], 1 <= L <= 4 and every ``K_l`` in {3, 5, 7, 9} -- takes the kernels ALWAYS and never falls back (a missing library raises).
Everything else -- CPU tensors, fp32 / fp64 tensors, other widths, other kernel sizes (the bare classes' default ``focal_window=9`` with two
levels has K = 11 at the second) -- takes the torch composition of the same formulas (:func:`focal_context_torch`), which is also the
float64 definition the tests compare with the reference.  Stochastic depth lives outside the modulation, so the default ``drop_path_rate``
trains on the kernel path.

The classes mirror the reference's -- constructor arguments and state-dict keys -- so a reference checkpoint loads with ``strict=True``
both ways.  Without ``fused`` the linear layers, the norms and the layer scale run on torch ops.  The plain attribute ``fused``
(``set_fused`` of the modulation, the block, the layer and the network; False by default, not a constructor argument, not in the state
dict, bf16 on the device only) routes ``f``, ``h``, ``proj``, ``fc1`` + GELU and ``fc2``, the norms and ``shortcut + gamma x`` through the
shared row operators of :mod:`richsem_amd.backbone_ops` (``f``'s output rows padded to 2 C + 32, from which q, ctx0 and the gates are read
in place and into whose gradient rows dq, dctx0 and the gate gradients are written in place); it raises under ``drop_path > 0`` in
training mode.  The stem and downsampling convolutions stay torch's on every
path.  ``forward(images, mask)`` returns (feature, mask) pairs as ``swin.py`` and ``convnext.py`` do.  Nothing here downloads
anything: a pretrained path raises.  Capturing the device path into a HIP graph is untested.
"""
import ctypes

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from . import _lib
from .backbone_ops import (BF16, EPI_BIAS, MAX_C, DropPath, bf16_rows, cached_forms, check_bf16, depthwise_weight_grads, gelu_mlp_backward,
                           gelu_mlp_forward, kernel_width, layer_scale, linear_forms, linear_kernel, linear_on_forms, mask_pyramid, need_erf_gelu,
                           need_layernorm, on_kernels, output_norm_nchw, pair, refuse_drop_path_in_training, swin_layernorm, swin_linear, wgrad)
from .param_cache import VersionCache

__all__ = ["focal_context", "focal_context_torch", "modulate", "kernel_path", "focal_weight_form", "Mlp", "FocalModulation",
           "FocalModulationBlock", "BasicLayer", "PatchEmbed", "FocalNet", "build_focalnet"]

KERNEL_SIZES = (3, 5, 7, 9)
MODELS = ("focalnet_L_384_22k", "focalnet_L_384_22k_fl4", "focalnet_XL_384_22k", "focalnet_H_224_22k_fl4_fd")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def kernel_shape(C, sizes):
    """do the kernels support width ``C`` and the levels' kernel sizes ``sizes`` (K_0, K_0 + 2, ...)?"""
    sizes = tuple(sizes)
    return (kernel_width(C) and 1 <= len(sizes) <= 4 and all(k in KERNEL_SIZES for k in sizes)
            and all(b - a == 2 for a, b in zip(sizes, sizes[1:])))


def kernel_path(x, sizes):
    """THE RULE of the module docstring: bf16 on the device and a supported shape -> the kernels, always; everything else -> torch"""
    return on_kernels(x) and kernel_shape(x.shape[-1], sizes)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
def focal_weight_form(weights):
    """the parameters (C, 1, K_l, K_l), l = 0 .. L-1 -> the form the kernels read: (sum K_l^2, C) float32, tap-major, level after level"""
    return torch.cat([w.detach().float().reshape(w.shape[0], -1).t() for w in weights], 0).contiguous()


def workspace_bytes(B, H, W, C):
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_fmod_workspace_bytes(B, H, W, C, ctypes.byref(n)))
    return n.value


def _pixel_rows(t, multiple, align):
    """a (B, H, W, n) tensor whose pixels lie ``ld`` elements apart (a slice of wider rows) -> (t, ld) as it is where the kernels can read
    it in place (ld a multiple of ``multiple``, the pointer ``align``-byte aligned), else a contiguous copy"""
    B, H, W, n = t.shape
    ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if B > 1 else n))
    if (t.stride(3) == 1 and ld >= n and ld % multiple == 0 and t.data_ptr() % align == 0 and (W == 1 or t.stride(2) == ld)
            and (H == 1 or t.stride(1) == W * ld) and (B == 1 or t.stride(0) == H * W * ld)):
        return t, ld
    return t.contiguous(), n


def _check_context(ctx0, gates, wform, sizes):
    if ctx0.dim() != 4 or gates.dim() != 4 or gates.shape[:3] != ctx0.shape[:3] or gates.shape[3] != len(sizes) + 1:
        raise RuntimeError(f"focal_context: ctx0 (B, H, W, C) and gates (B, H, W, L + 1) with L = {len(sizes)}, got {tuple(ctx0.shape)} and "
                           f"{tuple(gates.shape)}")
    C = ctx0.shape[-1]
    if not kernel_shape(C, sizes):
        raise RuntimeError(f"focal_context: C a multiple of 32 in [32, {MAX_C}] and 1 to 4 kernel sizes from {KERNEL_SIZES} growing by 2, got "
                           f"C = {C} and {tuple(sizes)}")
    rows = sum(k * k for k in sizes)
    if wform.dtype != torch.float32 or tuple(wform.shape) != (rows, C) or not wform.is_contiguous():
        raise RuntimeError(f"focal_context: weight form float32 ({rows}, {C}) contiguous, got {wform.dtype} {tuple(wform.shape)}")
    check_bf16(ctx0, C, "focal_context (ctx0)")
    check_bf16(gates, len(sizes) + 1, "focal_context (gates)", limited=False)
    if wform.device != ctx0.device:
        raise RuntimeError(f"focal_context: weight form on {ctx0.device}, got {wform.device}")
    if gates.device != ctx0.device:
        raise RuntimeError(f"focal_context: gates on {ctx0.device}, got {gates.device}")


def context_forward_kernel(ctx0, gates, wform, sizes, normalize):
    """``msda_fmod_context_forward_bf16`` (no autograd): ctx0 (B, H, W, C) and gates (B, H, W, L + 1) bf16 on the device (slices of wider
    rows are read in place), wform :func:`focal_weight_form` -> (A (B, H, W, C) bf16, u (L, B, H, W, C) bf16, mg (2, B, C) float32)"""
    _check_context(ctx0, gates, wform, sizes)
    B, H, W, C = ctx0.shape
    L = len(sizes)
    ctx0, ld0 = _pixel_rows(ctx0, 8, 16)
    gates, ldg = _pixel_rows(gates, 1, 2)
    u = torch.empty((L, B, H, W, C), dtype=BF16, device=ctx0.device)
    mg = torch.empty((2, B, C), dtype=torch.float32, device=ctx0.device)
    A = torch.empty((B, H, W, C), dtype=BF16, device=ctx0.device)
    ws = torch.empty(workspace_bytes(B, H, W, C) // 4, dtype=torch.float32, device=ctx0.device)
    with _lib.on_device(ctx0.device):
        _lib.check(_lib.load().msda_fmod_context_forward_bf16(ctx0.data_ptr(), ld0, gates.data_ptr(), ldg, wform.data_ptr(), B, H, W, C, L,
                                                              int(sizes[0]), int(bool(normalize)), u.data_ptr(), mg.data_ptr(), A.data_ptr(),
                                                              ws.data_ptr(), _lib.raw_stream(ctx0.device)))
    return A, u, mg


def context_backward_kernel(dA, ctx0, gates, wform, u, mg, sizes, normalize, want_weights=True, into=None):
    """``msda_fmod_context_backward_bf16`` -> (dctx0 (B, H, W, C) bf16, dgates (B, H, W, L + 1) bf16, dw (sum K_l^2, C) float32 or None,
    du (L, B, H, W, C) bf16).  ``into``: (dctx0, dgates), views of wider contiguous gradient rows (B, H, W, ld) that are written in place"""
    _check_context(ctx0, gates, wform, sizes)
    B, H, W, C = ctx0.shape
    L = len(sizes)
    if dA.dtype != BF16 or dA.shape != ctx0.shape or dA.device != ctx0.device:
        raise RuntimeError(f"focal_context: dA bfloat16 {tuple(ctx0.shape)} on {ctx0.device}, got {dA.dtype} {tuple(dA.shape)} on {dA.device}")
    if u.dtype != BF16 or tuple(u.shape) != (L, B, H, W, C) or not u.is_contiguous() or mg.dtype != torch.float32 or tuple(mg.shape) != (2, B, C) \
            or not mg.is_contiguous() or u.device != ctx0.device or mg.device != ctx0.device:
        raise RuntimeError("focal_context: u and mg as context_forward_kernel returned them")
    dA = dA.contiguous()
    ctx0, ld0 = _pixel_rows(ctx0, 8, 16)
    gates, ldg = _pixel_rows(gates, 1, 2)
    du = torch.empty_like(u)
    if into is None:
        dctx0 = torch.empty((B, H, W, C), dtype=BF16, device=ctx0.device)
        dgates = torch.empty((B, H, W, L + 1), dtype=BF16, device=ctx0.device)
        ldd0, lddg = C, L + 1
    else:
        (dctx0, ldd0), (dgates, lddg) = _pixel_rows(into[0], 8, 16), _pixel_rows(into[1], 1, 2)
        if dctx0 is not into[0] or dgates is not into[1] or dctx0.shape != ctx0.shape or dgates.shape != gates.shape or dctx0.dtype != BF16 \
                or dgates.dtype != BF16 or dctx0.device != ctx0.device or dgates.device != ctx0.device:
            raise RuntimeError("focal_context: gradient rows that cannot be written in place")
    dw = torch.empty_like(wform) if want_weights else None
    ws = torch.empty(workspace_bytes(B, H, W, C) // 4, dtype=torch.float32, device=ctx0.device)
    with _lib.on_device(ctx0.device):
        _lib.check(_lib.load().msda_fmod_context_backward_bf16(dA.data_ptr(), ctx0.data_ptr(), ld0, gates.data_ptr(), ldg, wform.data_ptr(),
                                                               u.data_ptr(), mg.data_ptr(), B, H, W, C, L, int(sizes[0]), int(bool(normalize)),
                                                               du.data_ptr(), dctx0.data_ptr(), ldd0, dgates.data_ptr(), lddg,
                                                               dw.data_ptr() if dw is not None else None, ws.data_ptr(),
                                                               _lib.raw_stream(ctx0.device)))
    return dctx0, dgates, dw, du


def _token_rows(t, C, what):
    """(..., C) bf16 on the device -> (t, ld): a (B, H, W, C) slice of wider rows as it is where the kernels can read it in place"""
    check_bf16(t, C, what)
    if t.dim() == 4:
        return _pixel_rows(t, 8, 16)
    return t.reshape(-1, C).contiguous(), C


def modulate_kernel(q, mod):
    """``msda_fmod_modulate_forward_bf16``: q, mod (..., C) bf16 on the device (q may be a (B, H, W, C) slice of wider rows, read in place)
    -> rnd(q mod) in q's shape"""
    C = q.shape[-1]
    (q2, ldq), m2 = _token_rows(q, C, "modulate"), bf16_rows(mod, C, "modulate (mod)")
    if mod.shape != q.shape or mod.device != q.device:
        raise RuntimeError(f"modulate: mod {tuple(q.shape)} on {q.device}, got {tuple(mod.shape)} on {mod.device}")
    out = torch.empty_like(m2)
    with _lib.on_device(q.device):
        _lib.check(_lib.load().msda_fmod_modulate_forward_bf16(q2.data_ptr(), ldq, m2.data_ptr(), m2.shape[0], C, out.data_ptr(),
                                                               _lib.raw_stream(q.device)))
    return out.view(q.shape)


def modulate_backward_kernel(dout, q, mod, into=None):
    """``msda_fmod_modulate_backward_bf16`` -> (dq = rnd(dout mod), dmod = rnd(dout q)) in q's shape.  ``into``: a (B, H, W, C) view of wider
    contiguous gradient rows that dq is written into in place"""
    C = q.shape[-1]
    d2, (q2, ldq), m2 = bf16_rows(dout, C, "modulate (gradient)"), _token_rows(q, C, "modulate"), bf16_rows(mod, C, "modulate (mod)")
    if not (dout.shape == q.shape == mod.shape) or not (dout.device == q.device == mod.device):
        raise RuntimeError(f"modulate: dout, q and mod of one shape on one device, got {tuple(dout.shape)}, {tuple(q.shape)}, {tuple(mod.shape)}")
    if into is None:
        dq, lddq = torch.empty_like(m2), C
    else:
        dq, lddq = _token_rows(into, C, "modulate (dq)")
        if dq is not into or into.shape != q.shape or into.device != q.device:
            raise RuntimeError("modulate: gradient rows that cannot be written in place")
    dmod = torch.empty_like(m2)
    with _lib.on_device(q.device):
        _lib.check(_lib.load().msda_fmod_modulate_backward_bf16(d2.data_ptr(), q2.data_ptr(), ldq, m2.data_ptr(), m2.shape[0], C, dq.data_ptr(),
                                                                lddq, dmod.data_ptr(), _lib.raw_stream(q.device)))
    return dq.view(q.shape), dmod.view(q.shape)


class _FocalContextFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ctx0, gates, normalize, wform, *weights):
        sizes = tuple(w.shape[-1] for w in weights)
        A, u, mg = context_forward_kernel(ctx0, gates, wform, sizes, normalize)
        ctx.save_for_backward(ctx0, gates, wform, u, mg)
        ctx.meta = (sizes, bool(normalize), tuple((w.dtype, w.shape) for w in weights))
        return A

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dA):
        ctx0, gates, wform, u, mg = ctx.saved_tensors
        sizes, normalize, wmeta = ctx.meta
        want_w = any(ctx.needs_input_grad[4:])
        dctx0, dgates, dw, _ = context_backward_kernel(dA, ctx0, gates, wform, u, mg, sizes, normalize, want_weights=want_w)
        return ((dctx0 if ctx.needs_input_grad[0] else None, dgates if ctx.needs_input_grad[1] else None, None, None)
                + depthwise_weight_grads(dw, wmeta, ctx.needs_input_grad[4:]))


def focal_context_torch(ctx0, gates, weights, normalize):
    """The torch composition of the module docstring's formulas, in the tensors' dtype (the float64 definition): ctx0 (B, H, W, C), gates
    (B, H, W, L + 1), ``weights`` the L parameters (C, 1, K_l, K_l) -> A (B, H, W, C)"""
    L, C = len(weights), ctx0.shape[-1]
    ctx, g, acc = ctx0.permute(0, 3, 1, 2), gates.permute(0, 3, 1, 2), 0
    for l, w in enumerate(weights):
        ctx = F.gelu(F.conv2d(ctx, w, None, padding=w.shape[-1] // 2, groups=C))
        acc = acc + ctx * g[:, l:l + 1]
    acc = acc + F.gelu(ctx.mean((2, 3), keepdim=True)) * g[:, L:]
    if normalize:
        acc = acc / (L + 1)
    return acc.permute(0, 2, 3, 1)


def focal_context(ctx0, gates, weights, normalize=False, cache=None):
    """The hierarchical context aggregation ``A``: ctx0 (B, H, W, C), gates (B, H, W, L + 1), ``weights`` the L depthwise parameters
    (C, 1, K_l, K_l), K_l growing by 2.  Where :func:`kernel_path` holds it is ONE autograd function over ``msda_fmod_context_*`` (gradients
    of ctx0 and gates in bf16, of the weights in the parameters' dtypes, every reduction in a fixed order) and never falls back; anything
    else runs :func:`focal_context_torch`.  ``cache``: a VersionCache that keeps the weight form per parameter version."""
    weights = list(weights)
    sizes = tuple(w.shape[-1] for w in weights)
    if ctx0.dim() != 4 or gates.dim() != 4 or gates.shape[:3] != ctx0.shape[:3] or gates.shape[3] != len(weights) + 1:
        raise RuntimeError(f"focal_context: ctx0 (B, H, W, C) and gates (B, H, W, L + 1) with L = {len(weights)}, got {tuple(ctx0.shape)} and "
                           f"{tuple(gates.shape)}")
    for w in weights:
        if w.dim() != 4 or tuple(w.shape) != (ctx0.shape[-1], 1, w.shape[-1], w.shape[-1]):
            raise RuntimeError(f"focal_context: weights (C, 1, K, K) with C = {ctx0.shape[-1]}, got {tuple(w.shape)}")
    if not kernel_path(ctx0, sizes):
        return focal_context_torch(ctx0, gates, weights, normalize)
    wform = focal_weight_form(weights) if cache is None else cache.get(weights, lambda: focal_weight_form(weights))
    return _FocalContextFunction.apply(ctx0, gates, bool(normalize), wform, *weights)


class _ModulateFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, mod):
        ctx.save_for_backward(q, mod)
        return modulate_kernel(q, mod)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, mod = ctx.saved_tensors
        dq, dmod = modulate_backward_kernel(dout, q, mod)
        return dq if ctx.needs_input_grad[0] else None, dmod if ctx.needs_input_grad[1] else None


def modulate(q, mod):
    """``q * mod``: bf16 device tensors of a width the kernels support take ``msda_fmod_modulate_*``, anything else the torch product"""
    if q.shape != mod.shape:
        raise RuntimeError(f"modulate: q and mod of one shape, got {tuple(q.shape)} and {tuple(mod.shape)}")
    if not (on_kernels(q) and kernel_width(q.shape[-1]) and mod.dtype == BF16):
        return q * mod
    return _ModulateFunction.apply(q, mod)


# ---- ``fused``: the rest of a block on library kernels --------------------------------------------------------------------------------------
F_PAD = 32      # the padded width of ``f``'s output rows is 2 C + 32: q | ctx0 | the L + 1 gates | zeros (rows of 16-byte multiples)


class _FusedModulationFunction(torch.autograd.Function):
    """``q * h(A)`` from the padded output rows of ``f`` (B, H, W, 2 C + 32): q, ctx0 and the gates are read in place; the backward writes dq,
    dctx0 and the gate gradients in place into one gradient row tensor whose padding columns are zero.  No split or cat is materialised."""

    @staticmethod
    def forward(ctx, rows, normalize, wform, hw, hb, hforms, *weights):
        C, L = hw.shape[0], len(weights)
        sizes = tuple(w.shape[-1] for w in weights)
        rows = rows.contiguous()
        q, ctx0, gates = rows[..., :C], rows[..., C:2 * C], rows[..., 2 * C:2 * C + L + 1]
        A, u, mg = context_forward_kernel(ctx0, gates, wform, sizes, normalize)
        mod, _ = linear_kernel(A.view(-1, C), hforms["w16"], hforms["b32"], EPI_BIAS)
        mod = mod.view(A.shape)
        ctx.save_for_backward(rows, wform, u, mg, A, mod)
        ctx.hforms = hforms
        ctx.meta = (sizes, bool(normalize), tuple((w.dtype, w.shape) for w in weights), hw.dtype, hw.shape, hb.dtype if hb is not None else None)
        return modulate_kernel(q, mod)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        rows, wform, u, mg, A, mod = ctx.saved_tensors
        sizes, normalize, wmeta, hwdt, hwshape, hbdt = ctx.meta
        C, L = A.shape[-1], len(sizes)
        q, ctx0, gates = rows[..., :C], rows[..., C:2 * C], rows[..., 2 * C:2 * C + L + 1]
        drows = torch.empty_like(rows)
        drows[..., 2 * C + L + 1:] = 0
        _, dmod = modulate_backward_kernel(dout.contiguous(), q, mod, into=drows[..., :C])
        dmod2 = dmod.view(-1, C)
        dA, _ = linear_kernel(dmod2, ctx.hforms["wt16"])
        dhw, dhb = wgrad(ctx, 3, 4, dmod2, A.view(-1, C), hwdt, hbdt)
        want_w = any(ctx.needs_input_grad[6:])
        _, _, dw, _ = context_backward_kernel(dA.view(A.shape), ctx0, gates, wform, u, mg, sizes, normalize, want_weights=want_w,
                                              into=(drows[..., C:2 * C], drows[..., 2 * C:2 * C + L + 1]))
        return ((drows, None, None, dhw.reshape(hwshape) if dhw is not None else None, dhb, None)
                + depthwise_weight_grads(dw, wmeta, ctx.needs_input_grad[6:]))


class _FocalMlpFunction(torch.autograd.Function):
    """``fc2(GELU(fc1(x)))`` under the GELU-MLP policy of ``backbone_ops`` (``swin_mlp`` without its norm and residual: a post-LN block norms
    the OUTPUT): saves x and the pre-activation u"""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, f1, f2):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        need = any(ctx.needs_input_grad)
        out, u = gelu_mlp_forward(x2, f1, f2, need, EPI_BIAS)
        if need:
            ctx.save_for_backward(x2, u)
            ctx.forms = (f1, f2)
            ctx.meta = (x.shape,) + tuple(p.dtype if p is not None else None for p in (w1, b1, w2, b2))
        return out.view(x.shape[:-1] + (w2.shape[0],))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        x2, u = ctx.saved_tensors
        (f1, f2), (shape, *dtypes) = ctx.forms, ctx.meta
        d2 = dout.reshape(-1, dout.shape[-1]).contiguous()
        dx, dw1, db1, dw2, db2 = gelu_mlp_backward(ctx, (1, 2, 3, 4), dtypes, d2, x2, u, f1, f2, want_dxn=ctx.needs_input_grad[0])      # w1, b1, w2, b2
        return dx.view(shape) if dx is not None else None, dw1, db1, dw2, db2, None, None


def _need_fused(x, what):
    if not on_kernels(x):
        raise RuntimeError(f"richsem_amd.focalnet: fused {what} needs a bfloat16 tensor on the device, got {x.dtype} on {x.device}")


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class FocalModulation(nn.Module):
    """The reference's module: ``forward(x)`` on (B, H, W, C) -> (B, H, W, C).  ``use_postln`` is accepted as the reference accepts it
    (it is the block's switch).  The context aggregation and the product follow THE RULE of the module docstring.  ``fused`` (a plain
    attribute, False by default; not a constructor argument, not in the state dict; bf16 on the device only, a shape the kernels support):
    ``f`` -- its output rows padded to 2 C + 32 by zero rows in a derived weight form --, ``h`` and ``proj`` run on ``msda_swin_linear_bf16``
    and ``ln`` on ``msda_swin_layernorm_*``; q, ctx0 and the gates are read in place from f's rows, their gradients written in place."""

    fused = False

    def __init__(self, dim, proj_drop=0., focal_level=2, focal_window=7, focal_factor=2, use_postln=False, use_postln_in_modulation=False,
                 normalize_modulator=False):
        super().__init__()
        self.dim = dim
        self.focal_level = focal_level
        self.focal_window = focal_window
        self.focal_factor = focal_factor
        self.use_postln_in_modulation = use_postln_in_modulation
        self.normalize_modulator = normalize_modulator
        self.f = nn.Linear(dim, 2 * dim + (focal_level + 1), bias=True)
        self.h = nn.Conv2d(dim, dim, kernel_size=1, stride=1, padding=0, groups=1, bias=True)
        self.act = nn.GELU()
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.focal_layers = nn.ModuleList()
        if use_postln_in_modulation:
            self.ln = nn.LayerNorm(dim)
        for k in range(focal_level):
            size = focal_factor * k + focal_window
            self.focal_layers.append(nn.Sequential(nn.Conv2d(dim, dim, kernel_size=size, stride=1, groups=dim, padding=size // 2, bias=False),
                                                   nn.GELU()))
        self._form = VersionCache()      # the kernels' weight form
        self._forms = {k: VersionCache() for k in ("f", "h", "proj")}      # derived forms of the fused path

    def set_fused(self, flag=True):
        self.fused = bool(flag)
        return self

    def _forward_fused(self, x):
        C, L = x.shape[-1], self.focal_level
        weights = [layer[0].weight for layer in self.focal_layers]
        _need_fused(x, "modulation")
        if not kernel_shape(C, [w.shape[-1] for w in weights]):
            raise RuntimeError(f"richsem_amd.focalnet: fused modulation needs a shape the kernels support, got C = {C} and kernel sizes "
                               f"{[w.shape[-1] for w in weights]}")
        pad = F_PAD - (L + 1)
        wpad, bpad = F.pad(self.f.weight, (0, 0, 0, pad)), F.pad(self.f.bias, (0, pad))      # (differentiable: their gradients' padding is dropped)
        rows = linear_on_forms(x, wpad, bpad, cached_forms(self._forms["f"], self.f.weight, self.f.bias, lambda: linear_forms(wpad, bpad)))
        hw = self.h.weight
        hforms = cached_forms(self._forms["h"], hw, self.h.bias, lambda: linear_forms(hw.view(C, C), self.h.bias))
        wform = self._form.get(weights, lambda: focal_weight_form(weights))
        out = _FusedModulationFunction.apply(rows, self.normalize_modulator, wform, hw, self.h.bias, hforms, *weights)
        if self.use_postln_in_modulation:
            out = swin_layernorm(out, self.ln.weight, self.ln.bias, self.ln.eps)
        return self.proj_drop(swin_linear(out, self.proj.weight, self.proj.bias, cache=self._forms["proj"]))

    def forward(self, x):
        if self.fused:
            return self._forward_fused(x)
        C, L = x.shape[-1], self.focal_level
        q, ctx0, gates = torch.split(self.f(x), (C, C, L + 1), -1)
        A = focal_context(ctx0, gates, [layer[0].weight for layer in self.focal_layers], self.normalize_modulator, cache=self._form)
        out = modulate(q, F.linear(A, self.h.weight.view(C, C), self.h.bias))
        if self.use_postln_in_modulation:
            out = self.ln(out)
        return self.proj_drop(self.proj(out))


class FocalModulationBlock(nn.Module):
    """The reference's block: ``forward(x)`` on (B, H * W, C) with ``H`` and ``W`` set as attributes by the layer.  ``fused`` (a plain
    attribute, False by default; :meth:`set_fused`): the modulation's ``fused``, the norms on ``msda_swin_layernorm_*``, ``fc1`` + GELU and
    ``fc2`` on ``msda_swin_linear_bf16`` and ``shortcut + gamma x`` on ``msda_layer_scale_*``; raises under ``drop_path > 0`` in training
    mode, like the other two backbones."""

    fused = False

    def __init__(self, dim, mlp_ratio=4., drop=0., drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, focal_level=2, focal_window=9,
                 use_postln=False, use_postln_in_modulation=False, normalize_modulator=False, use_layerscale=False, layerscale_value=1e-4):
        super().__init__()
        self.dim = dim
        self.mlp_ratio = mlp_ratio
        self.focal_window = focal_window
        self.focal_level = focal_level
        self.use_postln = use_postln
        self.use_layerscale = use_layerscale
        self.norm1 = norm_layer(dim)
        self.modulation = FocalModulation(dim, focal_window=focal_window, focal_level=focal_level, proj_drop=drop,
                                          use_postln_in_modulation=use_postln_in_modulation, normalize_modulator=normalize_modulator)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.H = None
        self.W = None
        self._forms = {k: VersionCache() for k in ("fc1", "fc2")}      # derived weight forms of the fused path
        self.gamma_1 = 1.0
        self.gamma_2 = 1.0
        if use_layerscale:
            self.gamma_1 = nn.Parameter(layerscale_value * torch.ones(dim), requires_grad=True)
            self.gamma_2 = nn.Parameter(layerscale_value * torch.ones(dim), requires_grad=True)

    def set_fused(self, flag=True):
        self.fused = self.modulation.fused = bool(flag)
        return self

    def _forward_fused(self, x):
        refuse_drop_path_in_training(self, "focalnet")
        need_erf_gelu(self.mlp.act, "focalnet")
        if self.mlp.drop.p > 0.:
            raise NotImplementedError("richsem_amd.focalnet: fused blocks need drop=0.")
        for norm in (self.norm1, self.norm2):
            need_layernorm(norm, "focalnet", "block")
        _need_fused(x, "block")
        B, N, C = x.shape
        H, W = self.H, self.W
        ln = lambda t, norm: swin_layernorm(t, norm.weight, norm.bias, norm.eps)      # noqa: E731
        scale = lambda z, gamma, res: layer_scale(z, gamma, res) if self.use_layerscale else res + z      # noqa: E731
        mlp = lambda t: _FocalMlpFunction.apply(t, self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight, self.mlp.fc2.bias,      # noqa: E731
                                                cached_forms(self._forms["fc1"], self.mlp.fc1.weight, self.mlp.fc1.bias),
                                                cached_forms(self._forms["fc2"], self.mlp.fc2.weight, self.mlp.fc2.bias))
        z = self.modulation((x if self.use_postln else ln(x, self.norm1)).view(B, H, W, C)).reshape(B, N, C)
        x = scale(ln(z, self.norm1) if self.use_postln else z, self.gamma_1, x)
        return scale(ln(mlp(x), self.norm2) if self.use_postln else mlp(ln(x, self.norm2)), self.gamma_2, x)

    def forward(self, x):
        B, N, C = x.shape
        H, W = self.H, self.W
        if N != H * W:
            raise RuntimeError(f"richsem_amd.focalnet: {N} tokens for a map of {H} x {W}")
        if self.fused:
            return self._forward_fused(x)
        shortcut = x
        if not self.use_postln:
            x = self.norm1(x)
        x = self.modulation(x.view(B, H, W, C)).reshape(B, H * W, C)
        if self.use_postln:
            x = self.norm1(x)
        x = shortcut + self.drop_path(self.gamma_1 * x)
        if self.use_postln:
            return x + self.drop_path(self.gamma_2 * self.norm2(self.mlp(x)))
        return x + self.drop_path(self.gamma_2 * self.mlp(self.norm2(x)))


class BasicLayer(nn.Module):
    """One stage: ``forward(x, H, W)`` -> (x, H, W, x_down, Wh, Ww) as the reference.  ``use_checkpoint`` recomputes each block in the
    backward (non-reentrant checkpointing: the gradients are those of the plain run)."""

    def __init__(self, dim, depth, mlp_ratio=4., drop=0., drop_path=0., norm_layer=nn.LayerNorm, downsample=None, focal_window=9,
                 focal_level=2, use_conv_embed=False, use_postln=False, use_postln_in_modulation=False, normalize_modulator=False,
                 use_layerscale=False, use_checkpoint=False):
        super().__init__()
        self.depth = depth
        self.use_checkpoint = use_checkpoint
        self.blocks = nn.ModuleList([
            FocalModulationBlock(dim=dim, mlp_ratio=mlp_ratio, drop=drop, drop_path=drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path,
                                 focal_window=focal_window, focal_level=focal_level, use_postln=use_postln,
                                 use_postln_in_modulation=use_postln_in_modulation, normalize_modulator=normalize_modulator,
                                 use_layerscale=use_layerscale, norm_layer=norm_layer)
            for i in range(depth)])
        if downsample is not None:
            self.downsample = downsample(patch_size=2, in_chans=dim, embed_dim=2 * dim, use_conv_embed=use_conv_embed, norm_layer=norm_layer,
                                         is_stem=False)
        else:
            self.downsample = None

    def set_fused(self, flag=True):
        """``fused`` of every block and of the downsampling layer's norm"""
        for blk in self.blocks:
            blk.set_fused(flag)
        if self.downsample is not None:
            self.downsample.fused = bool(flag)
        return self

    def forward(self, x, H, W):
        for blk in self.blocks:
            blk.H, blk.W = H, W
            x = checkpoint.checkpoint(blk, x, use_reentrant=False) if self.use_checkpoint else blk(x)
        if self.downsample is None:
            return x, H, W, x, H, W
        down = self.downsample(x.transpose(1, 2).reshape(x.shape[0], x.shape[-1], H, W))
        Wh, Ww = down.shape[2], down.shape[3]
        return x, H, W, down.flatten(2).transpose(1, 2), Wh, Ww


class PatchEmbed(nn.Module):
    """Image (or map) to patch embedding, (B, C, H, W) -> (B, embed_dim, Wh, Ww).  With ``use_conv_embed`` the stem is a 7 x 7 convolution
    of stride 4 with padding 2 and the downsampling a 3 x 3 one of stride 2 with padding 1; else a ``patch_size`` convolution of that
    stride on the map padded to a multiple of it.  torch's convolutions on every path; with ``fused`` (a plain attribute) the norm of a
    bf16 device tensor runs on ``msda_swin_layernorm_*``."""

    fused = False

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None, use_conv_embed=False, is_stem=False):
        super().__init__()
        self.patch_size = pair(patch_size)
        self.in_chans = in_chans
        self.embed_dim = embed_dim
        if use_conv_embed:
            size, padding, stride = (7, 2, 4) if is_stem else (3, 1, 2)
            self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=size, stride=stride, padding=padding)
        else:
            self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        H, W = x.shape[2], x.shape[3]
        if W % self.patch_size[1] != 0:
            x = F.pad(x, (0, self.patch_size[1] - W % self.patch_size[1]))
        if H % self.patch_size[0] != 0:
            x = F.pad(x, (0, 0, 0, self.patch_size[0] - H % self.patch_size[0]))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.shape[2], x.shape[3]
            t = x.flatten(2).transpose(1, 2)
            if self.fused and on_kernels(t):
                need_layernorm(self.norm, "focalnet", "PatchEmbed")
                t = swin_layernorm(t, self.norm.weight, self.norm.bias, self.norm.eps)
            else:
                t = self.norm(t)
            x = t.transpose(1, 2).reshape(-1, self.embed_dim, Wh, Ww)
        return x


class FocalNet(nn.Module):
    """``forward_features(images)`` -> the tuple of (B, C_i, H_i, W_i) features of ``out_indices``; ``forward(images, mask)`` -> a list of
    (feature, mask) pairs with the padding mask (B, H, W) bool interpolated to each level, as ``SwinTransformer.forward`` does.
    :meth:`set_fused` (off by default): ``fused`` of every block, the embedding norms and the output norms (``swin_norm_nchw``)."""

    fused = False

    def __init__(self, pretrain_img_size=1600, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), mlp_ratio=4., drop_rate=0.,
                 drop_path_rate=0.2, norm_layer=nn.LayerNorm, patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                 focal_levels=(2, 2, 2, 2), focal_windows=(9, 9, 9, 9), use_conv_embed=False, use_postln=False, use_postln_in_modulation=False,
                 use_layerscale=False, normalize_modulator=False, use_checkpoint=False):
        super().__init__()
        self.pretrain_img_size = pretrain_img_size
        self.num_layers = len(depths)
        self.embed_dim = embed_dim
        self.patch_norm = patch_norm
        self.out_indices = out_indices
        self.frozen_stages = frozen_stages
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      norm_layer=norm_layer if patch_norm else None, use_conv_embed=use_conv_embed, is_stem=True)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList([
            BasicLayer(dim=int(embed_dim * 2 ** i), depth=depths[i], mlp_ratio=mlp_ratio, drop=drop_rate,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                       downsample=PatchEmbed if i < self.num_layers - 1 else None, focal_window=focal_windows[i], focal_level=focal_levels[i],
                       use_conv_embed=use_conv_embed, use_postln=use_postln, use_postln_in_modulation=use_postln_in_modulation,
                       normalize_modulator=normalize_modulator, use_layerscale=use_layerscale, use_checkpoint=use_checkpoint)
            for i in range(self.num_layers)])
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i in out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                m = self.layers[i]
                m.eval()
                for p in m.parameters():
                    p.requires_grad = False

    def set_fused(self, flag=True):
        self.fused = self.patch_embed.fused = bool(flag)
        for layer in self.layers:
            layer.set_fused(flag)
        return self

    def forward_features(self, x):
        x = self.patch_embed(x)
        Wh, Ww = x.shape[2], x.shape[3]
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                outs.append(output_norm_nchw(getattr(self, f"norm{i}"), x_out, H, W, self.fused, "focalnet"))
        return tuple(outs)

    def forward(self, images, mask):
        return mask_pyramid(self.forward_features(images), mask)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self


def focalnet_config(modelname, **kw):
    """the reference's arguments of a named model (``focal_levels`` / ``focal_windows`` given as one number are repeated per stage)"""
    if modelname not in MODELS:
        raise ValueError(f"richsem_amd.focalnet: unknown model {modelname!r} {MODELS}")
    kw = dict(kw)
    for k in ("focal_levels", "focal_windows"):
        if k in kw:
            kw[k] = [kw[k]] * 4
    fl4 = modelname in ("focalnet_L_384_22k_fl4", "focalnet_H_224_22k_fl4_fd")
    cfg = dict(embed_dim={"focalnet_L_384_22k": 192, "focalnet_L_384_22k_fl4": 192, "focalnet_XL_384_22k": 256}.get(modelname, 352),
               depths=[2, 2, 18, 2], focal_levels=[4] * 4 if fl4 else [3] * 4, focal_windows=[3] * 4 if fl4 else [5] * 4,
               use_conv_embed=True, use_postln=True, use_postln_in_modulation=modelname == "focalnet_H_224_22k_fl4_fd", use_layerscale=True,
               normalize_modulator=modelname == "focalnet_L_384_22k_fl4")
    if modelname == "focalnet_L_384_22k_fl4":
        cfg["drop_path_rate"] = 0.3
    cfg.update(kw)
    return cfg


def build_focalnet(modelname, pretrained=False, **kw):
    """The reference's builder for its four named models.  ``pretrained`` (True or a path) raises: this module never downloads or reads a
    checkpoint; build with ``pretrained=False`` and load a state dict."""
    if pretrained:
        raise NotImplementedError("richsem_amd.focalnet: pretrained weights are not supported: nothing is downloaded here; build with "
                                  "pretrained=False and load_state_dict() a checkpoint")
    return FocalNet(**focalnet_config(modelname, **kw))
