"""The CondInst dynamic mask head (``msda_dynmask_*``, csrc/dynamic_masks.hip): the producer of the ``pred_masks`` that :mod:`richsem_amd.masks`
consumes.

``MaskBranch`` of the reference (models/richsem/cond_inst.py) turns every decoder query into the weights of a three-layer 1x1-conv network
(169 or 233 numbers), repeats the stride-8 mask features once per instance, runs three grouped convolutions over that tensor and up-samples
the result by ``aligned_bilinear``.  :func:`dynamic_masks` computes the same logits from the features, the parameter rows and the reference
points alone: which rows are computed is read on the device from an int32 table, the repeated input and the two hidden maps never exist, and
the backward recomputes the chain.  :func:`dynamic_masks_torch` is the torch composition of the definition: the float64 definition, the CPU
path, and the comparator of tools/dynamic_masks_timing.py.

The definition, for image n, query q and stride-8 pixel (y, x) of the (H, W) feature map:
    in  = [ref_x size_w - (8 x + 4), ref_y size_h - (8 y + 4), feats[n, :, y, x]]        (rel_coord=False: the features alone)
    t   = w2 . relu(W1 relu(W0 in + b0) + b1) + b2
    row = W0 (8, Cin) row-major, W1 (8, 8), w2 (8), b0 (8), b1 (8), b2 (1)                (all weights, then all biases)
    out = aligned_bilinear(t, 8 // mask_out_stride)
"""
import collections
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .masks import MaskTargets

HIDDEN = 8                     # the dynamic width (the reference's dy_mask_channel)
KERNEL_CHANNELS = (8, 16)      # the template instances of csrc/dynamic_masks.hip
FEAT_STRIDE = 8

Saved = collections.namedtuple("Saved", ("feats", "params", "ref", "sizes", "inst", "dims"))


def num_params(C, rel_coord=True):
    """the length of a parameter row: 169 for C = 8, 233 for C = 16 with the coordinates"""
    return HIDDEN * (C + (2 if rel_coord else 0)) + HIDDEN * HIDDEN + HIDDEN + 2 * HIDDEN + 1


def workspace_bytes(N, C, H, W, Q, R):
    """``msda_dynmask_workspace_bytes``: the library's own figure"""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_dynmask_workspace_bytes(N, C, H, W, Q, R, ctypes.byref(n)))
    return n.value


def workspace_bytes_host(N, C, H, W, Q, R):
    """the same figure from the shapes alone (the mirror of ``dm_plan``, csrc/dynamic_masks.hip): one partial row of 108 + 8 C fp32 per image,
    tile of 8 x 32 pixels and output row, rounded up to 256 bytes"""
    return (N * ((H + 7) // 8) * ((W + 31) // 32) * R * (108 + 8 * C) * 4 + 255) // 256 * 256


def aligned_bilinear(t, factor):
    """the closed form of the reference's ``aligned_bilinear`` for factor 1 and 2 over the last two axes: F[0] = T[0], F[2 k + 1] = T[k],
    F[2 k] = (T[k - 1] + T[k]) / 2"""
    if factor == 1:
        return t
    if factor != 2:
        raise ValueError(f"aligned_bilinear: factor 1 or 2, got {factor}")
    for dim in (-1, -2):
        t = t.transpose(dim, -1)
        left = torch.cat([t[..., :1], t[..., :-1]], dim=-1)
        t = torch.stack([0.5 * (left + t), t], dim=-1).flatten(-2).transpose(dim, -1)
    return t


def _checked(fn, feats, params, ref, sizes, rel_coord, mask_out_stride, use_relative_hw):
    """the argument checks every entry shares: -> (sizes (N, 2) float32 on feats' device, (N, C, H, W, Q), factor)"""
    if not all(torch.is_tensor(t) for t in (feats, params)) or (rel_coord and not torch.is_tensor(ref)):
        raise TypeError(f"{fn}: feats (N, C, H, W), params (N, Q, P) and ref (N, Q, 2 or 4) are tensors")
    if mask_out_stride not in (4, 8):
        raise ValueError(f"{fn}: mask_out_stride is 4 or 8, got {mask_out_stride}")
    if feats.dim() != 4 or min(feats.shape) < 1:
        raise ValueError(f"{fn}: feats is (N, C, H, W), got {tuple(feats.shape)}")
    N, C, H, W = feats.shape
    P = num_params(C, rel_coord)
    if params.dim() != 3 or params.shape[0] != N or params.shape[1] < 1 or params.shape[2] != P:
        raise ValueError(f"{fn}: params is (N, Q, P) with N = {N} and P = {P} for {C} channels, got {tuple(params.shape)}")
    if params.dtype != feats.dtype or params.device != feats.device:
        raise TypeError(f"{fn}: feats and params share their type and device")
    Q = params.shape[1]
    if rel_coord:
        need = 4 if use_relative_hw else 2
        if ref.dim() != 3 or tuple(ref.shape[:2]) != (N, Q) or ref.shape[2] < need or ref.device != feats.device:
            raise ValueError(f"{fn}: ref is (N, Q, >= {need}) = ({N}, {Q}, ...) on feats' device, got {tuple(ref.shape)}")
        sizes = torch.as_tensor(sizes)
        if tuple(sizes.shape) != (N, 2):
            raise ValueError(f"{fn}: sizes is (N, 2) = (height, width) per image, got {tuple(sizes.shape)}")
        sizes = sizes.detach().to(device=feats.device, dtype=torch.float32).contiguous()
    else:
        sizes = None
    return sizes, (N, C, H, W, Q), FEAT_STRIDE // mask_out_stride


def _table_args(fn, dims, mask_targets, query_of_target, rows, device):
    N, Q = dims[0], dims[4]
    if (mask_targets is None) != (query_of_target is None):
        raise TypeError(f"{fn}: mask_targets and query_of_target come together")
    if rows is not None and mask_targets is not None:
        raise TypeError(f"{fn}: rows= or mask_targets= / query_of_target=, not both")
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 2 or rows.shape[0] != N or rows.shape[1] < 1 or \
                rows.device != device:
            raise TypeError(f"{fn}: rows is an int64 (N, R) tensor on feats' device with N = {N}")
    if mask_targets is not None:
        if not isinstance(mask_targets, MaskTargets):
            raise TypeError(f"{fn}: mask_targets is a MaskTargets")
        if len(mask_targets.sizes) != N:
            raise ValueError(f"{fn}: the mask buffers were built for {len(mask_targets.sizes)} images, feats has {N}")
        if not torch.is_tensor(query_of_target) or query_of_target.dtype != torch.int64 or \
                tuple(query_of_target.shape) != (mask_targets.capacity,) or not query_of_target.is_contiguous():
            raise ValueError(f"{fn}: query_of_target is a contiguous int64 ({mask_targets.capacity},) tensor: one query per target slot")
        if query_of_target.device != device or mask_targets.offsets_dev.device != device:
            raise ValueError(f"{fn}: feats, query_of_target and the mask buffers live on one device")


def table_torch(N, Q, device, mask_targets=None, query_of_target=None, rows=None):
    """the table ``inst`` (N, R) int64 as torch ops: the query of every output row, -1 = none"""
    if rows is not None:
        return torch.where((rows >= 0) & (rows < Q), rows, torch.full_like(rows, -1))
    inst = torch.arange(Q, device=device).expand(N, Q).contiguous()
    if mask_targets is None:
        return inst
    offs, cap = mask_targets.offsets_dev, mask_targets.capacity
    slots = torch.arange(cap, device=device)
    ok = (slots < offs[-1]) & (query_of_target >= 0) & (query_of_target < Q)
    img = torch.bucketize(slots, offs[1:].contiguous(), right=True).clamp(max=N - 1)
    inst = torch.full((N, Q), -1, dtype=torch.int64, device=device)
    inst[img[ok], query_of_target[ok]] = query_of_target[ok]
    return inst


def table_device(dims, device, mask_targets=None, query_of_target=None, rows=None):
    """``msda_dynmask_table``: the table as an int32 (N, R) device tensor, built by a kernel -- nothing waits on the host"""
    N, Q = dims[0], dims[4]
    R = Q if rows is None else int(rows.shape[1])
    inst = torch.empty((N, R), dtype=torch.int32, device=device)
    rows_c = None if rows is None else rows.contiguous()
    with _lib.on_device(device):
        _lib.check(_lib.load().msda_dynmask_table(
            None if rows_c is None else rows_c.data_ptr(), None if mask_targets is None else mask_targets.offsets_dev.data_ptr(),
            None if mask_targets is None else query_of_target.data_ptr(), N, R, Q, 1 if mask_targets is None else mask_targets.capacity,
            inst.data_ptr(), _lib.raw_stream(device)))
    return inst


def _relative_coords(ref, sizes, H, W, use_relative_hw, dtype):
    """(K, 2, H, W): the reference's relative_coords of K instances, ref (K, 2 or 4) normalised, sizes (K, 2) = (h, w)"""
    wh = sizes[:, [1, 0]].to(ref.dtype)
    loc = ref[:, :2] * wh
    xs = torch.arange(W, device=ref.device, dtype=torch.float32) * FEAT_STRIDE + FEAT_STRIDE // 2
    ys = torch.arange(H, device=ref.device, dtype=torch.float32) * FEAT_STRIDE + FEAT_STRIDE // 2
    rel = torch.stack([(loc[:, 0, None, None] - xs[None, None, :]).expand(-1, H, -1), (loc[:, 1, None, None] - ys[None, :, None]).expand(-1, -1, W)],
                      dim=1)
    if use_relative_hw:      # the reference's formula as it stands (cond_inst.py:358-362)
        whs = (ref[:, 2:4] * wh)[:, :, None, None]
        hws = whs.flip(1)
        rel = 1 - (rel / hws * 2).abs()
        rel = 1 - rel.abs()
        rel = rel / whs * 2
    return rel.to(dtype)


def _compose(feats, params, ref, sizes, inst, rel_coord, factor, use_relative_hw=False):
    """the definition as torch ops over the live rows of ``inst`` (one host read: their number); differentiable by autograd"""
    N, C, H, W = feats.shape
    R = inst.shape[1]
    out = feats.new_zeros((N, R, factor * H, factor * W))
    cin = C + 2 if rel_coord else C
    a, b, c = HIDDEN * cin, HIDDEN * cin + HIDDEN * HIDDEN, HIDDEN * cin + HIDDEN * HIDDEN + HIDDEN
    for n in range(N):
        r_idx = (inst[n] >= 0).nonzero().flatten()
        if r_idx.numel() == 0:
            continue
        q_idx = inst[n][r_idx]
        p = params[n][q_idx]
        K = p.shape[0]
        W0, W1, w2 = p[:, :a].reshape(K, HIDDEN, cin), p[:, a:b].reshape(K, HIDDEN, HIDDEN), p[:, b:c]
        b0, b1, b2 = p[:, c:c + HIDDEN], p[:, c + HIDDEN:c + 2 * HIDDEN], p[:, c + 2 * HIDDEN]
        if rel_coord:
            rel = _relative_coords(ref[n][q_idx], sizes[n][None].expand(K, 2), H, W, use_relative_hw, feats.dtype)
            z0 = torch.einsum("kic,kchw->kihw", W0[:, :, :2], rel) + torch.einsum("kic,chw->kihw", W0[:, :, 2:], feats[n])
        else:
            z0 = torch.einsum("kic,chw->kihw", W0, feats[n])
        h0 = F.relu(z0 + b0[:, :, None, None])
        h1 = F.relu(torch.einsum("kji,kihw->kjhw", W1, h0) + b1[:, :, None, None])
        t = torch.einsum("kj,kjhw->khw", w2, h1) + b2[:, None, None]
        out = out.index_put((torch.full_like(r_idx, n), r_idx), aligned_bilinear(t, factor))
    if out.grad_fn is None and torch.is_grad_enabled() and (feats.requires_grad or params.requires_grad):
        out = out + (feats.sum() + params.sum()) * 0      # (no live row at all: zeros that autograd can still walk back from)
    return out


def dynamic_masks_torch(feats, params, ref, sizes, *, mask_targets=None, query_of_target=None, rows=None, rel_coord=True, mask_out_stride=4,
                        use_relative_hw=False):
    """The reference's dynamic mask head as a torch composition, on any device and in ``feats``'s type; the same arguments and result as
    :func:`dynamic_masks`.  It never repeats the features: a live row costs its two hidden maps."""
    sizes, dims, factor = _checked("dynamic_masks_torch", feats, params, ref, sizes, rel_coord, mask_out_stride, use_relative_hw)
    _table_args("dynamic_masks_torch", dims, mask_targets, query_of_target, rows, feats.device)
    inst = table_torch(dims[0], dims[4], feats.device, mask_targets, query_of_target, rows)
    return _compose(feats, params, ref, sizes, inst, rel_coord, factor, use_relative_hw)


def _sfx(t):
    return "bf16" if t.dtype == torch.bfloat16 else "f32"


def _ptr(t):
    return None if t is None else t.data_ptr()


def dynmask_forward(feats, params, ref, sizes, inst, dims, rel_coord, factor):
    """the forward half on checked tensors: -> (out (N, R, F H, F W), saved); ``saved`` (a :class:`Saved`) is what :func:`dynmask_backward`
    takes.  ``ref`` (N, Q, 2) float32 contiguous or None, ``inst`` (N, R) int32."""
    dev = feats.device
    N, C, H, W, Q = dims
    R = int(inst.shape[1])
    f, p = feats.detach().contiguous(), params.detach().contiguous()
    out = torch.empty((N, R, factor * H, factor * W), dtype=f.dtype, device=dev)
    full = (N, C, H, W, Q, R, int(bool(rel_coord)), factor)
    with _lib.on_device(dev):
        _lib.check(getattr(_lib.load(), "msda_dynmask_forward_" + _sfx(f))(
            f.data_ptr(), p.data_ptr(), _ptr(ref), _ptr(sizes), inst.data_ptr(), *full, out.data_ptr(), _lib.raw_stream(dev)))
    return out, Saved(f, p, ref, sizes, inst, full)


def dynmask_backward(saved, grad_out, want_ref=True):
    """the backward half: -> (grad_feats, grad_params in their type, grad_ref (N, Q, 2) float32 or None); every element written by the kernels"""
    f, p = saved.feats, saved.params
    dev = f.device
    N, C, H, W, Q, R = saved.dims[:6]
    g = grad_out.detach().to(f.dtype).contiguous()
    gf, gp = torch.empty_like(f), torch.empty_like(p)
    gr = torch.empty((N, Q, 2), dtype=torch.float32, device=dev) if want_ref and saved.ref is not None else None
    ws = torch.empty(workspace_bytes(N, C, H, W, Q, R), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(getattr(_lib.load(), "msda_dynmask_backward_" + _sfx(f))(
            g.data_ptr(), f.data_ptr(), p.data_ptr(), _ptr(saved.ref), _ptr(saved.sizes), saved.inst.data_ptr(), *saved.dims, gp.data_ptr(),
            gf.data_ptr(), _ptr(gr), ws.data_ptr(), _lib.raw_stream(dev)))
    return gf, gp, gr


class DynamicMaskFunction(torch.autograd.Function):
    """:func:`dynamic_masks` as one autograd node: gradients for ``feats``, ``params`` and ``ref``"""

    @staticmethod
    def forward(ctx, feats, params, ref, sizes, inst, dims, rel_coord, factor):
        out, saved = dynmask_forward(feats, params, ref, sizes, inst, dims, rel_coord, factor)
        ctx.has_ref = ref is not None
        ctx.save_for_backward(*(t for t in (saved.feats, saved.params, saved.ref, saved.sizes, saved.inst) if t is not None))
        ctx.dims = saved.dims
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        t = ctx.saved_tensors
        saved = Saved(t[0], t[1], t[2] if ctx.has_ref else None, t[3] if ctx.has_ref else None, t[-1], ctx.dims)
        gf, gp, gr = dynmask_backward(saved, grad_out, want_ref=ctx.has_ref and ctx.needs_input_grad[2])
        return gf, gp, gr, None, None, None, None, None


def on_kernels(feats, rel_coord=True, use_relative_hw=False):
    """the dispatch rule: float32 or bfloat16 device tensors of 8 or 16 channels take the kernels -- always --, everything else the
    composition"""
    return feats.is_cuda and feats.dtype in (torch.float32, torch.bfloat16) and feats.dim() == 4 and feats.shape[1] in KERNEL_CHANNELS and \
        not (rel_coord and use_relative_hw)


def _ref_xy(ref):
    """the two coordinates the kernels read, float32 and contiguous; autograd carries the gradient back through the slice and the cast"""
    return ref[..., :2].to(torch.float32).contiguous()


def _with_table(feats, params, ref, sizes, inst, rel_coord=True, mask_out_stride=4, use_relative_hw=False):
    """:func:`dynamic_masks` with the table given: ``inst`` (N, R) integers, -1 = a row of zeros.  With gradients, for any table."""
    sizes, dims, factor = _checked("dynamic_masks", feats, params, ref, sizes, rel_coord, mask_out_stride, use_relative_hw)
    if not on_kernels(feats, rel_coord, use_relative_hw):
        return _compose(feats, params, ref, sizes, inst.to(torch.int64), rel_coord, factor, use_relative_hw)
    return DynamicMaskFunction.apply(feats, params, _ref_xy(ref) if rel_coord else None, sizes, inst.to(torch.int32).contiguous(), dims,
                                     rel_coord, factor)


def dynamic_masks(feats, params, ref, sizes, *, mask_targets=None, query_of_target=None, rows=None, rel_coord=True, mask_out_stride=4,
                  use_relative_hw=False):
    """The mask logits of the dynamic head: -> (N, R, F H, F W) in ``feats``'s type, F = 8 // mask_out_stride, with gradients for ``feats``,
    ``params`` and ``ref``.

    ``feats`` (N, C, H, W): the stride-8 mask features; ``params`` (N, Q, P): the controller's output; ``ref`` (N, Q, 2 or 4): the
    normalised reference points (x, y first); ``sizes`` (N, 2): the images' (height, width).  Which rows are computed:
      * neither ``rows`` nor ``mask_targets``: all queries, R = Q;
      * ``rows`` (N, R) int64 on the device: output row r of image n is query ``rows[n, r]`` (outside [0, Q): a row of zeros), e.g. the
        ``topk_boxes`` of ``PostProcess``.  Forward only: with gradients enabled on an input it raises;
      * ``mask_targets`` (a :class:`~richsem_amd.masks.MaskTargets`) and ``query_of_target`` (capacity,) int64, the operands of
        ``mask_losses``: R = Q, the rows of matched queries are computed, every other row is exact zeros.

    float32 and bfloat16 device tensors of 8 or 16 channels take the kernels, always: nothing waits, no allocation depends on the counts, so
    it is capturable after one eager call; bitwise reproducible.  CPU tensors, float64, other channel counts and ``use_relative_hw=True``
    take :func:`dynamic_masks_torch`."""
    sizes_f, dims, factor = _checked("dynamic_masks", feats, params, ref, sizes, rel_coord, mask_out_stride, use_relative_hw)
    _table_args("dynamic_masks", dims, mask_targets, query_of_target, rows, feats.device)
    if rows is not None and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (feats, params, ref)):
        raise RuntimeError("dynamic_masks: rows= is forward-only; call it under torch.no_grad() or on detached inputs")
    if not on_kernels(feats, rel_coord, use_relative_hw):
        inst = table_torch(dims[0], dims[4], feats.device, mask_targets, query_of_target, rows)
        return _compose(feats, params, ref, sizes_f, inst, rel_coord, factor, use_relative_hw)
    inst = table_device(dims, feats.device, mask_targets, query_of_target, rows)
    return DynamicMaskFunction.apply(feats, params, _ref_xy(ref) if rel_coord else None, sizes_f, inst, dims, rel_coord, factor)


@torch.no_grad()
def dynamic_masks_and_grads(feats, params, ref, sizes, grad_out, *, mask_targets=None, query_of_target=None, rel_coord=True, mask_out_stride=4):
    """:func:`dynamic_masks` and its backward in one call, WITHOUT the autograd engine: -> (out, grad_feats, grad_params, grad_ref) for the
    cotangent ``grad_out`` (N, Q, F H, F W) -- a tensor, or a callable that takes ``out`` and returns it (e.g. the mask terms' gradient).
    ``grad_ref`` (N, Q, 2) float32 is the gradient for ``ref[..., :2]``.  Device-only: float32 or bfloat16 device tensors of 8 or 16
    channels; anything else raises."""
    sizes_f, dims, factor = _checked("dynamic_masks_and_grads", feats, params, ref, sizes, rel_coord, mask_out_stride, False)
    if not feats.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if not on_kernels(feats, rel_coord):
        raise TypeError("dynamic_masks_and_grads: feats is a float32 or bfloat16 (N, C, H, W) tensor with C = 8 or 16")
    _table_args("dynamic_masks_and_grads", dims, mask_targets, query_of_target, None, feats.device)
    inst = table_device(dims, feats.device, mask_targets, query_of_target)
    out, saved = dynmask_forward(feats, params, _ref_xy(ref) if rel_coord else None, sizes_f, inst, dims, rel_coord, factor)
    g = grad_out(out) if callable(grad_out) else grad_out
    if tuple(g.shape) != tuple(out.shape):
        raise ValueError(f"dynamic_masks_and_grads: grad_out is {tuple(out.shape)}, got {tuple(g.shape)}")
    return (out,) + dynmask_backward(saved, g)


class MLP(nn.Module):
    """the reference's MLP (models/richsem/utils.py): ``layers.{i}`` Linear, ReLU between"""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


class MaskHeadSmallConv(nn.Module):
    """The reference's ``MaskHeadSmallConv`` (drop-in: constructor arguments and state-dict keys ``lay1 .. lay4``, ``dcn`` and, with
    ``fpn_dims``, ``adapter1 .. adapter3``): the conv tower that turns the three finest memory maps into the stride-8 mask features."""

    def __init__(self, dim, fpn_dims, context_dim, dim_div=32):
        super().__init__()
        self.lay1 = nn.Conv2d(dim, dim // 4, 3, padding=1)
        self.lay2 = nn.Conv2d(dim // 4, dim // dim_div, 3, padding=1)
        self.lay3 = nn.Conv2d(context_dim, context_dim, 3, padding=1)
        self.lay4 = nn.Conv2d(context_dim, context_dim, 3, padding=1)
        self.dcn = nn.Conv2d(context_dim, context_dim, 3, padding=1)
        self.dim = dim
        if fpn_dims is not None:
            self.adapter1 = nn.Conv2d(fpn_dims[0], context_dim, 1)
            self.adapter2 = nn.Conv2d(fpn_dims[1], context_dim, 1)
            self.adapter3 = nn.Conv2d(fpn_dims[2], context_dim, 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                nn.init.constant_(m.bias, 0)

    def _level(self, x, adapter, fpn):
        if fpn is None:
            return x
        cur = adapter(fpn)
        if cur.size(0) != x.size(0):
            cur = cur.unsqueeze(1).repeat(1, x.size(0) // cur.size(0), 1, 1, 1).flatten(0, 1)
        return (cur + x) / 2

    def forward(self, x, fpns=None):
        fp = fpns if fpns is not None else (None, None, None)
        ad = (self.adapter1, self.adapter2, self.adapter3) if fpns is not None else (None, None, None)
        y = F.relu(self.lay3(self._level(x[-1], ad[0], fp[0])))
        cur = self._level(x[-2], ad[1], fp[1])
        y = F.relu(self.lay4(cur + F.interpolate(y, size=cur.shape[-2:], mode="nearest")))
        cur = self._level(x[-3], ad[2], fp[2])
        y = F.relu(self.dcn(cur + F.interpolate(y, size=cur.shape[-2:], mode="nearest")))
        return F.relu(self.lay2(F.relu(self.lay1(y))))


class MaskBranch(nn.Module):
    """The reference's ``MaskBranch`` (drop-in: constructor arguments, state-dict keys ``controller.layers.{0,1,2}.*`` and ``mask_head.*``,
    and what ``forward`` returns) on :func:`dynamic_masks`.  The controller and the conv tower are torch modules."""

    def __init__(self, hidden_dim, rel_coord=True, use_relative_hw=False, channel_div=32, dy_mask_channel=8, is_concat=True):
        super().__init__()
        if dy_mask_channel != HIDDEN:
            raise ValueError(f"MaskBranch: the dynamic width is {HIDDEN}, got dy_mask_channel = {dy_mask_channel}")
        self.rel_coord, self.is_concat, self.use_relative_hw = rel_coord, is_concat, use_relative_hw
        self.in_channels = hidden_dim // channel_div * (2 if is_concat else 1)
        self.dynamic_mask_channels = dy_mask_channel
        self.mask_out_stride = 4
        self.num_gen_params = num_params(self.in_channels, rel_coord)
        self.controller = MLP(hidden_dim, hidden_dim, self.num_gen_params, 3)
        mask_dim = hidden_dim * 2 if is_concat else hidden_dim
        self.mask_head = MaskHeadSmallConv(mask_dim, None, mask_dim, dim_div=channel_div)

    @staticmethod
    def _sizes(targets, device):
        return torch.stack([torch.as_tensor(t["size"]) for t in targets]).to(device)

    def forward(self, hs, memory, references, indices_list, targets):
        """-> (masks per decoder layer, parameters per decoder layer).  Training: per layer the matched queries' masks of all images
        concatenated, (sum of the counts, 1, 2 H, 2 W), in the order of ``indices``; eval: every query's, (N, Q, 1, 2 H, 2 W)."""
        feats = self.mask_head(memory)
        sizes = self._sizes(targets, feats.device)
        outputs_masks, output_params = [], []
        for lvl, indices in enumerate(indices_list):
            params = self.controller(hs[lvl])
            N, Q = params.shape[:2]
            if self.training:
                counts = [int(i.numel()) for i, _ in indices]
                table = torch.full((N, max(max(counts), 1)), -1, dtype=torch.int64)
                for n, (pred_i, _) in enumerate(indices):
                    table[n, :counts[n]] = pred_i.detach().cpu()
                inst = table.to(feats.device)
            else:
                counts = None
                inst = torch.arange(Q, device=feats.device).expand(N, Q)
            out = _with_table(feats, params.to(feats.dtype), references[lvl], sizes, inst, self.rel_coord, self.mask_out_stride,
                              self.use_relative_hw)
            if counts is None:
                outputs_masks.append(out.unsqueeze(2))
            else:
                outputs_masks.append(torch.cat([out[n, :c] for n, c in enumerate(counts)]).unsqueeze(1))
            output_params.append(params)
        return outputs_masks, output_params

    def forward_capacity(self, hs_l, memory, reference_l, sizes, mask_targets, query_of_target):
        """one decoder layer over capacity buffers: -> (N, Q, 2 H, 2 W), the ``pred_masks`` that ``mask_losses`` takes -- the rows of the
        queries matched in (``mask_targets``, ``query_of_target``) computed, every other row zeros; nothing waits on the host"""
        feats = self.mask_head(memory)
        params = self.controller(hs_l).to(feats.dtype)
        return dynamic_masks(feats, params, reference_l, sizes, mask_targets=mask_targets, query_of_target=query_of_target,
                             rel_coord=self.rel_coord, mask_out_stride=self.mask_out_stride, use_relative_hw=self.use_relative_hw)
