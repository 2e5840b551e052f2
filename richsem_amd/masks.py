"""The criterion's mask terms and the mask post-processor over CAPACITY buffers (``msda_mask_*``, csrc/mask_terms.hip).

``SetCriterion.loss_masks`` of the reference (models/richsem/richsem.py:1073-1100) gathers the matched predictions, resizes each to the padded
target size as a float tensor, casts the padded targets to float and runs ``sigmoid_focal_loss`` and ``dice_loss`` (segmentation.py:168-211)
over both.  :func:`mask_losses` computes the same two numbers from the low-resolution logits and one byte per target pixel: the pairs are read
on the device from the target prefix of a :class:`MaskTargets` and the matcher's ``query_of_target``, the resized logit exists in a register
only, and the backward gathers into ``pred_masks`` without atomics.  :class:`PostProcessSegm` is the reference's post-processor
(segmentation.py:214-242) as one launch: the x4 float map, its boolean copy on the host and the host resize do not exist.

:func:`mask_losses_torch` is the torch composition of the reference's formula from the same buffers: the float64 definition, the CPU path,
and the comparator of tools/mask_terms_timing.py.
"""
import collections
import ctypes

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

Saved = collections.namedtuple("Saved", ("pred", "target", "offsets", "qot", "num_boxes", "sums", "ws", "dims", "alpha"))


def _round_up(v, m):
    return (int(v) + m - 1) // m * m


class MaskTargets:
    """The capacity form of the reference's padded mask tensor (``nested_tensor_from_tensor_list(masks)``, util/misc.py:400-428): ``masks``
    uint8 (capacity, Hp, Wp) on the device, one canvas per target slot in the slot order of :class:`~richsem_amd.matcher.TargetBuffers` (the
    images' targets one after the other), a target's mask in the top left corner and zeros elsewhere; ``offsets_dev`` (n_images + 1) int64 the
    exclusive prefix of the per-image counts.  Slots from ``offsets_dev[-1]`` on are dead and zero.  ``canvas`` = (Hp, Wp) is fixed at
    construction -- the launches are shaped by it --, so a batch whose masks are smaller is padded further than the reference pads it; build
    with :meth:`canvas_of` of the largest batch to be served, or per batch for the reference's numbers."""

    def __init__(self, n_images, capacity, canvas, device, offsets_dev=None):
        n_images, capacity = int(n_images), int(capacity)
        Hp, Wp = (int(v) for v in canvas)
        if n_images < 1 or capacity < 1:
            raise ValueError(f"MaskTargets: n_images and capacity must be >= 1, got {n_images} and {capacity}")
        if Hp < 1 or Wp < 16 or Wp % 16:
            raise ValueError(f"MaskTargets: the canvas is (Hp >= 1, Wp a multiple of 16), got ({Hp}, {Wp})")
        if offsets_dev is not None and (offsets_dev.dtype != torch.int64 or offsets_dev.numel() != n_images + 1):
            raise ValueError(f"MaskTargets: offsets_dev is an int64 tensor of {n_images + 1} elements")
        self.device = torch.device(device)
        self.capacity = self.total = capacity
        self.canvas = (Hp, Wp)
        self.sizes = [0] * n_images
        self.offsets = [0] * (n_images + 1)
        self.live = 0
        self.offsets_dev = torch.zeros(n_images + 1, dtype=torch.int64, device=device) if offsets_dev is None else offsets_dev
        self.masks = torch.zeros((capacity, Hp, Wp), dtype=torch.uint8, device=device)

    @classmethod
    def like(cls, target_buffers, canvas):
        """mask buffers for the images, capacity and device of a ``TargetBuffers``, SHARING its ``offsets_dev``"""
        return cls(len(target_buffers.sizes), target_buffers.capacity, canvas, target_buffers.device, offsets_dev=target_buffers.offsets_dev)

    @staticmethod
    def canvas_of(targets):
        """the reference's padded size of a batch: the largest mask height and width over the images, each rounded up to a multiple of 32"""
        return (_round_up(max(int(t["masks"].shape[-2]) for t in targets), 32), _round_up(max(int(t["masks"].shape[-1]) for t in targets), 32))

    @torch.no_grad()
    def update_(self, targets):
        """write a batch -- a list over the images of dicts with "masks" (T_b, H_b, W_b), bool or 0 / 1 integers -- into the buffers: host ->
        device copies on the current stream, between replays and not in a capture, as ``TargetBuffers.update_``.  Another image count, more
        targets than ``capacity``, or a mask larger than the canvas raise ValueError and leave the buffers alone."""
        masks = [t["masks"] for t in targets]
        sizes = [int(m.shape[0]) for m in masks]
        if len(sizes) != len(self.sizes):
            raise ValueError(f"MaskTargets.update_: {len(sizes)} images, the buffers were built for {len(self.sizes)}")
        if sum(sizes) > self.capacity:
            raise ValueError(f"MaskTargets.update_: {sum(sizes)} targets in all, the capacity is {self.capacity}")
        Hp, Wp = self.canvas
        for m in masks:
            if m.dim() != 3 or m.shape[-2] > Hp or m.shape[-1] > Wp:
                raise ValueError(f"MaskTargets.update_: masks are (T_b, H_b, W_b) with H_b <= {Hp} and W_b <= {Wp}, got {tuple(m.shape)}")
        offsets = [0]
        for n in sizes:
            offsets.append(offsets[-1] + n)
        host = torch.zeros((self.capacity, Hp, Wp), dtype=torch.uint8)
        for m, o, n in zip(masks, offsets, sizes):
            if n:
                host[o:o + n, :m.shape[-2], :m.shape[-1]] = m.detach().cpu().to(torch.uint8)
        self.sizes, self.offsets, self.live = sizes, offsets, offsets[-1]
        self.offsets_dev.copy_(torch.tensor(offsets, dtype=torch.int64), non_blocking=True)
        self.masks.copy_(host, non_blocking=True)
        return self


def workspace_bytes(N, Q, h, w, Hp, Wp, capacity):
    """``msda_mask_loss_workspace_bytes``: the library's own figure"""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_mask_loss_workspace_bytes(N, Q, h, w, Hp, Wp, capacity, ctypes.byref(n)))
    return n.value


def workspace_bytes_host(N, Q, h, w, Hp, Wp, capacity):
    """the same figure from the shapes alone (the mirror of ``ml_plan``, csrc/mask_terms.hip): one partial row of 4 fp32 per slot and band of 8
    canvas rows, rounded up to 256 bytes, then one int32 per query"""
    return _round_up(capacity * ((Hp + 7) // 8) * 16, 256) + 4 * N * Q


def _checked(fn, pred_masks, mask_targets, query_of_target, num_boxes, device_only):
    """the argument checks of the mask-loss entries: -> (num_boxes as a (1,) float32 tensor on pred's device, dims)"""
    if not isinstance(mask_targets, MaskTargets):
        raise TypeError(f"{fn}: mask_targets is a MaskTargets")
    if not torch.is_tensor(pred_masks) or not torch.is_tensor(query_of_target):
        raise TypeError(f"{fn}: pred_masks (N, Q, h, w) and query_of_target (capacity) are tensors")
    tensors = (pred_masks, query_of_target, mask_targets.masks, mask_targets.offsets_dev) + ((num_boxes,) if torch.is_tensor(num_boxes) else ())
    if device_only and not all(t.is_cuda for t in tensors):
        raise RuntimeError("Not implemented on the CPU")
    if any(t.device != pred_masks.device for t in tensors):
        raise ValueError(f"{fn}: pred_masks, query_of_target, num_boxes and the mask buffers live on one device")
    if not pred_masks.is_floating_point():
        raise TypeError(f"{fn}: pred_masks is a floating-point (N, Q, h, w) tensor")
    if query_of_target.dtype != torch.int64:
        raise TypeError(f"{fn}: query_of_target is an int64 tensor")
    N, cap = len(mask_targets.sizes), mask_targets.capacity
    if pred_masks.dim() != 4 or pred_masks.shape[0] != N or min(pred_masks.shape) < 1:
        raise ValueError(f"{fn}: pred_masks is (N, Q, h, w) with N = {N}, the image count of the mask buffers, got {tuple(pred_masks.shape)}")
    if tuple(query_of_target.shape) != (cap,) or not query_of_target.is_contiguous():
        raise ValueError(f"{fn}: query_of_target is a contiguous ({cap},) tensor: one query per target slot (the LAST output's row of "
                         "match_many_device's result)")
    if torch.is_tensor(num_boxes):
        if num_boxes.numel() != 1:
            raise TypeError(f"{fn}: num_boxes is a number or a one-element tensor")
        nb = num_boxes.detach().reshape(1).to(torch.float32)
    else:
        nb = torch.full((1,), float(num_boxes), dtype=torch.float32, device=pred_masks.device)
    _, Q, h, w = pred_masks.shape
    return nb, (N, Q, h, w) + mask_targets.canvas + (cap,)


def mask_losses_torch(pred_masks, mask_targets, query_of_target, num_boxes, *, alpha=0.25):
    """The reference's ``loss_masks`` as a torch composition over the same buffers, on any device and in ``pred_masks``'s type: the pairs from
    ``mask_targets.offsets_dev`` and ``query_of_target`` (one host read: their number), ``F.interpolate(..., mode="bilinear",
    align_corners=False)`` to the canvas, ``sigmoid_focal_loss`` and ``dice_loss``.  Differentiable by autograd."""
    nb, (N, Q, h, w, Hp, Wp, cap) = _checked("mask_losses_torch", pred_masks, mask_targets, query_of_target, num_boxes, False)
    offs = mask_targets.offsets_dev
    slots = torch.arange(cap, device=pred_masks.device)
    idx = ((slots < offs[-1]) & (query_of_target >= 0) & (query_of_target < Q)).nonzero().flatten()
    if idx.numel() == 0:
        zero = pred_masks.sum() * 0
        return {"loss_mask": zero, "loss_dice": zero.clone()}
    img = torch.bucketize(idx, offs[1:].contiguous(), right=True)
    x = F.interpolate(pred_masks[img, query_of_target[idx]][:, None], size=(Hp, Wp), mode="bilinear", align_corners=False)[:, 0].flatten(1)
    t = mask_targets.masks[idx].to(x.dtype).flatten(1)
    nb = nb.to(x.dtype)
    p = x.sigmoid()
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    focal = ce * (1 - (p * t + (1 - p) * (1 - t))) ** 2
    if alpha >= 0:
        focal = (alpha * t + (1 - alpha) * (1 - t)) * focal
    dice = 1 - (2 * (p * t).sum(1) + 1) / (p.sum(-1) + t.sum(-1) + 1)
    return {"loss_mask": (focal.mean(1).sum() / nb)[0], "loss_dice": (dice.sum() / nb)[0]}


def _sfx(t):
    return "bf16" if t.dtype == torch.bfloat16 else "f32"


def mask_loss_forward(pred_masks, mask_targets, query_of_target, nb, dims, alpha):
    """the forward half on checked tensors: -> (losses (2,) float32 = (loss_mask, loss_dice), saved); ``saved`` (a :class:`Saved`) is what
    :func:`mask_loss_backward` takes"""
    dev = pred_masks.device
    pred = pred_masks.detach().contiguous()
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    sums = torch.empty((dims[-1], 4), dtype=torch.float32, device=dev)
    ws = torch.empty(workspace_bytes(*dims), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(getattr(_lib.load(), "msda_mask_loss_forward_" + _sfx(pred))(
            pred.data_ptr(), mask_targets.masks.data_ptr(), mask_targets.offsets_dev.data_ptr(), query_of_target.data_ptr(), nb.data_ptr(), *dims,
            float(alpha), losses.data_ptr(), sums.data_ptr(), ws.data_ptr(), _lib.raw_stream(dev)))
    return losses, Saved(pred, mask_targets.masks, mask_targets.offsets_dev, query_of_target, nb, sums, ws, dims, float(alpha))


def mask_loss_backward(saved, g):
    """the backward half: ``g`` (2,) float32 on the device = d / d loss_mask, d / d loss_dice -> grad_pred (N, Q, h, w) in pred's type, every
    element written by the kernel (exact zeros for queries without a pair)"""
    pred = saved.pred
    dev = pred.device
    g = g.detach().reshape(2).to(torch.float32).contiguous()
    grad = torch.empty_like(pred)
    with _lib.on_device(dev):
        _lib.check(getattr(_lib.load(), "msda_mask_loss_backward_" + _sfx(pred))(
            pred.data_ptr(), saved.target.data_ptr(), saved.offsets.data_ptr(), saved.qot.data_ptr(), saved.num_boxes.data_ptr(),
            saved.sums.data_ptr(), g.data_ptr(), *saved.dims, saved.alpha, grad.data_ptr(), saved.ws.data_ptr(), _lib.raw_stream(dev)))
    return grad


class MaskLossFunction(torch.autograd.Function):
    """:func:`mask_losses` as one autograd node: the gradient for ``pred_masks``"""

    @staticmethod
    def forward(ctx, pred_masks, mask_targets, query_of_target, nb, dims, alpha):
        losses, saved = mask_loss_forward(pred_masks, mask_targets, query_of_target, nb, dims, alpha)
        ctx.save_for_backward(saved.pred, saved.target, saved.offsets, saved.qot, saved.num_boxes, saved.sums, saved.ws)
        ctx.values = (saved.dims, saved.alpha)
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_mask, g_dice):
        saved = Saved(*ctx.saved_tensors, *ctx.values)
        return (mask_loss_backward(saved, torch.stack([g_mask.reshape(()).float(), g_dice.reshape(()).float()])),) + (None,) * 5


def _on_kernels(pred_masks):
    return pred_masks.is_cuda and pred_masks.dtype in (torch.float32, torch.bfloat16)


def mask_losses(pred_masks, mask_targets, query_of_target, num_boxes, *, alpha=0.25):
    """The mask terms of the criterion, pairs found on the device: -> ``{"loss_mask", "loss_dice"}``, 0-dim tensors with a gradient for
    ``pred_masks``.

    ``pred_masks`` (N, Q, h, w): the LAST decoder output's mask logits (the reference skips the mask terms on auxiliary outputs);
    ``mask_targets``: a :class:`MaskTargets` holding the batch; ``query_of_target`` (capacity,) int64: the last output's row of
    ``match_many_device``'s result on the ``TargetBuffers`` the mask buffers share their offsets with; ``num_boxes``: a number or a
    one-element tensor, the reference's normaliser.  Pixels of the canvas outside a target's own mask are target 0 and count in every mean
    and sum, as in the reference.

    float32 and bfloat16 device tensors take the kernels -- float32 losses, the gradient in ``pred_masks``'s type --; nothing waits and no
    allocation depends on the counts, so it is capturable after one eager call; bitwise reproducible.  CPU tensors and float64 take
    :func:`mask_losses_torch`."""
    if not (torch.is_tensor(pred_masks) and _on_kernels(pred_masks)):
        return mask_losses_torch(pred_masks, mask_targets, query_of_target, num_boxes, alpha=alpha)
    nb, dims = _checked("mask_losses", pred_masks, mask_targets, query_of_target, num_boxes, True)
    loss_mask, loss_dice = MaskLossFunction.apply(pred_masks, mask_targets, query_of_target, nb, dims, alpha)
    return {"loss_mask": loss_mask, "loss_dice": loss_dice}


@torch.no_grad()
def mask_losses_and_grads(pred_masks, mask_targets, query_of_target, num_boxes, *, alpha=0.25, grad_losses=None):
    """:func:`mask_losses` and its backward in one call, WITHOUT the autograd engine, as ``device_criterion_and_grads``: -> (losses dict,
    grad_pred) for d / d (loss_mask, loss_dice) = ``grad_losses`` (a (2,) device tensor; default ones).  Device-only: float32 or bfloat16
    device tensors, CPU tensors raise."""
    nb, dims = _checked("mask_losses_and_grads", pred_masks, mask_targets, query_of_target, num_boxes, True)
    if pred_masks.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("mask_losses_and_grads: pred_masks is a float32 or bfloat16 (N, Q, h, w) tensor")
    losses, saved = mask_loss_forward(pred_masks, mask_targets, query_of_target, nb, dims, alpha)
    g = torch.ones(2, dtype=torch.float32, device=pred_masks.device) if grad_losses is None else grad_losses
    return {"loss_mask": losses[0], "loss_dice": losses[1]}, mask_loss_backward(saved, g)


def postprocess_masks(pred_masks, img_sizes, out_sizes, item_indices=None, threshold=0.5):
    """``msda_mask_postprocess_*``: per image b the rows ``item_indices[b]`` (int64 device tensors; None: all Q) of ``pred_masks`` (N, Q, h, w)
    -> a list of uint8 (rows, 1, oh, ow) device tensors: ``sigmoid(x4) > threshold`` of the bilinear x4 map, cropped to ``img_sizes[b]`` =
    (img_h, img_w) and resized by the nearest rule to ``out_sizes[b]`` = (oh, ow).  The sizes are host numbers.  One launch per 8 images."""
    if not torch.is_tensor(pred_masks) or not pred_masks.is_cuda or (item_indices is not None and not all(i.is_cuda for i in item_indices)):
        raise RuntimeError("Not implemented on the CPU")
    if pred_masks.dim() != 4 or min(pred_masks.shape) < 1:
        raise ValueError(f"postprocess_masks: pred_masks is (N, Q, h, w), got {tuple(pred_masks.shape)}")
    N, Q, h, w = pred_masks.shape
    if len(img_sizes) != N or len(out_sizes) != N or (item_indices is not None and len(item_indices) != N):
        raise ValueError(f"postprocess_masks: one (img_h, img_w), one (oh, ow) and one row list per image of the {N}")
    if pred_masks.dtype not in (torch.float32, torch.bfloat16):
        pred_masks = pred_masks.float()
    pred, dev = pred_masks.detach().contiguous(), pred_masks.device
    items = None if item_indices is None else [i.detach().to(torch.int64).reshape(-1).contiguous() for i in item_indices]
    rows = [Q] * N if items is None else [int(i.numel()) for i in items]
    sizes = [int(v) for a, b in zip(img_sizes, out_sizes) for v in (a[0], a[1], b[0], b[1])]
    if min(sizes) < 1:
        raise ValueError("postprocess_masks: every size is >= 1")
    outs = [torch.empty((r, 1, sizes[4 * b + 2], sizes[4 * b + 3]), dtype=torch.uint8, device=dev) for b, r in enumerate(rows)]
    c_items = None if items is None else (ctypes.c_void_p * N)(*[i.data_ptr() or None for i in items])
    c_outs = (ctypes.c_void_p * N)(*[o.data_ptr() or None for o in outs])
    with _lib.on_device(dev):
        _lib.check(getattr(_lib.load(), "msda_mask_postprocess_" + _sfx(pred))(
            pred.data_ptr(), N, Q, h, w, c_items, (ctypes.c_int * N)(*rows), (ctypes.c_int * (4 * N))(*sizes), float(threshold), c_outs,
            _lib.raw_stream(dev)))
    return outs


class PostProcessSegm(nn.Module):
    """The reference's ``PostProcessSegm`` (``postprocessors['segm']``; drop-in): fills ``results[i]["masks"]`` with uint8 (rows, 1, oh, ow)
    DEVICE tensors of the reference's values.  The reference thresholds the x4 map, moves it to the host and resizes it there; here one
    kernel writes the resized bytes."""

    def __init__(self, threshold=0.5, processor_dct=None):
        super().__init__()
        self.threshold = threshold
        self.processor_dct = processor_dct

    @torch.no_grad()
    def forward(self, results, outputs, orig_target_sizes, max_target_sizes):
        if self.processor_dct:
            return results
        assert len(orig_target_sizes) == len(max_target_sizes)
        pred = outputs["pred_masks"]
        if pred.dim() == 5:
            pred = pred.squeeze(2)
        img_sizes = torch.as_tensor(max_target_sizes).tolist()      # the host reads, one each, as the reference's .tolist()
        out_sizes = torch.as_tensor(orig_target_sizes).tolist()
        masks = postprocess_masks(pred, img_sizes, out_sizes, outputs.get("item_indices", None), self.threshold)
        for res, m in zip(results, masks):
            res["masks"] = m
        return results
