"""The criterion's classification and box terms over CAPACITY buffers (``msda_criterion_pairs_ex_f32``, csrc/msda_criterion.h).

``SetCriterion.forward`` of the reference (models/richsem/richsem.py:1124-1298) decides on the host which (prediction, target) pairs carry a
loss: the matcher's index lists, ``num_boxes`` (:1143-1147), the denoising positive indices from ``pad_size`` and the group count
(:1158-1171, ``prep_for_dn`` :1300-1306).  The composed step (bench_step.py ``Step.loss_part``) does the same with index tensors of the
batch's exact size.  :func:`device_criterion` reads all of it on the device instead -- the target prefix ``cum`` of a
:class:`~richsem_amd.matcher.TargetBuffers`, the solver's ``query_of_target``, the ``meta`` of ``denoising_queries`` -- so that ONE captured
graph of cost blocks -> assignment -> criterion (+ backward) serves any batch that fits the capacities.

Launches: forward -- the pair kernel (slots, row weights, per-workgroup partials), its reduction, ``focal.neg_sum`` over the decoder logits
and over the two-stage logits, and a few scalar torch ops that add the parts up; backward -- ``focal.neg_grad`` twice (the only dense passes
over the logits) and one scatter kernel.  No gather, no index tensor, no dense zero-fill of a logit-shaped tensor.

:func:`device_set_criterion` is the same criterion with the reference's two remaining switches: the federated loss (``use_fed_loss``: the
class subset of every get_loss call is drawn on the device from the appeared classes of the batch the buffers hold,
``msda_fed_class_mask_slots_f32``, and the all-negative term runs through the masked focal kernels with row groups the pair kernel
writes) and ``enc_cls_agn`` (the two-stage output scored against class 0).  Two launches more.  Both functions are front ends of ONE path
-- :func:`set_criterion_forward`, :func:`set_criterion_backward`, :class:`DeviceCriterionFunction` --, whose switches are optional arguments.
"""
import collections
import ctypes

import torch

from . import _lib, focal
from .fed_loss import FedClassSampler
from .matcher import LateStatus

STATUS = ("dn_overflow", "targets_without_query", "labels_out_of_range", "bad_prefix")      # the int32[4] ``status``

# what the forward half keeps for the backward half; ``g_rows``, ``g_int`` and ``class_mask`` are None where no class mask was given.  An
# autograd node keeps the host values in ctx and hands the rest, the tensors, to save_for_backward.
Saved = collections.namedtuple("Saved", ("x", "xi", "w_rows", "w_int", "ws", "cum", "dims", "alpha", "c_cls", "g_rows", "g_int", "class_mask"))
_SAVED_VALUES = ("dims", "alpha", "c_cls")
_SAVED_TENSORS = tuple(k for k in Saved._fields if k not in _SAVED_VALUES)


def _dims(logits, il, pad_cap, capacity):
    nl, N, QT, C = logits.shape
    return nl, N, QT - pad_cap, il.shape[1], C, int(capacity), int(pad_cap)


def _workspace(dims, device):
    nl, N, Q, Qi, _, cap, pad_cap = dims
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_criterion_workspace_bytes(nl, N, Q, Qi, cap, pad_cap, ctypes.byref(n)))
    return torch.empty(n.value, dtype=torch.uint8, device=device)


def set_criterion_forward(logits, coords, il, ib, cum, tgt_ids, tgt_boxes, qot, dn_meta, num_boxes, cfg, class_mask=None, enc_cls_agn=False):
    """the forward half on checked, contiguous tensors: -> (loss, terms, status, saved); ``saved`` (a :class:`Saved`) is what
    :func:`set_criterion_backward` takes.  ``cfg`` = (pad_cap, capacity, alpha, c_cls, c_l1, c_giou).  The two switches: ``class_mask``
    (2 nl + 1, C) float32 or None -- the class subset of each get_loss call, which the all-negative term is restricted to (the masked focal
    kernels with the row groups the pair kernel writes) --, and ``enc_cls_agn`` -- the two-stage output's positives take label 0.  Without
    either, ``msda_criterion_pairs_ex_f32`` gets flags = 0 and no row groups: the launches of ``msda_criterion_pairs_f32``
    (csrc/criterion_api.hip).  :class:`DeviceCriterionFunction` is the two halves as an autograd node; a caller that schedules the backward
    itself (a whole step captured without the autograd engine) calls them directly."""
    pad_cap, capacity, alpha, c_cls, c_l1, c_giou = cfg
    dev = logits.device
    dims = _dims(logits, il, pad_cap, capacity)
    nl, N, Q, Qi, C, cap, _ = dims
    x, p, xi, pi = logits.contiguous(), coords.contiguous(), il.contiguous(), ib.contiguous()
    ws = _workspace(dims, dev)
    w_rows = torch.empty(x.shape[:3], dtype=torch.float32, device=dev)
    w_int = torch.empty(xi.shape[:2], dtype=torch.float32, device=dev)
    fed = class_mask is not None
    g_rows = torch.empty(x.shape[:3], dtype=torch.int32, device=dev) if fed else None
    g_int = torch.empty(xi.shape[:2], dtype=torch.int32, device=dev) if fed else None
    terms = torch.empty((2 * nl + 1, 3), dtype=torch.float32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.load().msda_criterion_pairs_ex_f32(
            x.data_ptr(), p.data_ptr(), xi.data_ptr(), pi.data_ptr(), cum.data_ptr(), tgt_ids.data_ptr(), tgt_boxes.data_ptr(), qot.data_ptr(),
            None if dn_meta is None else dn_meta.data_ptr(), None if num_boxes is None else num_boxes.data_ptr(), nl, N, Q, Qi, C, cap, pad_cap,
            alpha, c_cls, c_l1, c_giou, 1 if enc_cls_agn else 0, w_rows.data_ptr(), w_int.data_ptr(), g_rows.data_ptr() if fed else None,
            g_int.data_ptr() if fed else None, terms.data_ptr(), status.data_ptr(), ws.data_ptr(), _lib.raw_stream(dev)))
        neg = focal.neg_sum(x, w_rows, alpha, g_rows, class_mask).sum() + focal.neg_sum(xi, w_int, alpha, g_int, class_mask).sum()
    tsum = terms.double().sum(0)      # (float64 scalars from here on; the coefficients are host numbers: nothing is copied)
    loss = (c_cls * (neg + tsum[0]) + c_l1 * tsum[1] + c_giou * tsum[2]).float()
    return loss, terms, status, Saved(x, xi, w_rows, w_int, ws, cum, dims, alpha, c_cls, g_rows, g_int, class_mask)


def set_criterion_backward(saved, g):
    """the backward half: ``g`` = d / d loss (0-dim or (1,) float32 on the device) -> (grad_logits, grad_coords, grad_il, grad_ib); with a
    class mask the logit gradients are exactly 0 off each row's class subset (``enc_cls_agn`` alone changes the records, not the launches)"""
    nl, N, Q, Qi, C, cap, pad_cap = saved.dims
    x, xi = saved.x, saved.xi
    dev = x.device
    gs = g.detach().reshape(1).float().contiguous()
    gs_cls = gs * saved.c_cls
    g_coords = torch.empty(x.shape[:3] + (4,), dtype=torch.float32, device=dev)
    g_ib = torch.empty(xi.shape[:2] + (4,), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        g_logits = focal.neg_grad(x, saved.w_rows, saved.alpha, gs_cls, saved.g_rows, saved.class_mask)      # (the dense passes: every element written)
        g_il = focal.neg_grad(xi, saved.w_int, saved.alpha, gs_cls, saved.g_int, saved.class_mask)
        _lib.check(_lib.load().msda_criterion_pairs_backward_f32(
            saved.ws.data_ptr(), saved.cum.data_ptr(), gs.data_ptr(), nl, N, Q, Qi, C, cap, pad_cap, g_logits.data_ptr(), g_il.data_ptr(),
            g_coords.data_ptr(), g_ib.data_ptr(), _lib.raw_stream(dev)))
    return g_logits, g_coords, g_il, g_ib


criterion_forward, criterion_backward = set_criterion_forward, set_criterion_backward      # (the names from before the switches)


class DeviceCriterionFunction(torch.autograd.Function):
    """:func:`device_criterion` / :func:`device_set_criterion` as one autograd node: gradients for logits, coords, il and ib.  ``cfg`` =
    (pad_cap, capacity, alpha, c_cls, c_l1, c_giou)."""

    @staticmethod
    def forward(ctx, logits, coords, il, ib, cum, tgt_ids, tgt_boxes, qot, dn_meta, num_boxes, cfg, class_mask, enc_cls_agn):
        loss, terms, status, saved = set_criterion_forward(logits, coords, il, ib, cum, tgt_ids, tgt_boxes, qot, dn_meta, num_boxes, cfg,
                                                           class_mask, enc_cls_agn)
        ctx.save_for_backward(*(getattr(saved, k) for k in _SAVED_TENSORS))
        ctx.values = {k: getattr(saved, k) for k in _SAVED_VALUES}
        ctx.mark_non_differentiable(terms, status)
        return loss, terms, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_terms, _g_status):
        saved = Saved(**dict(zip(_SAVED_TENSORS, ctx.saved_tensors)), **ctx.values)
        return set_criterion_backward(saved, g) + (None,) * 9


def _checked(logits, coords, il, ib, targets, query_of_target, dn_meta, pad_cap, alpha, c_cls, c_l1, c_giou, num_boxes, fed_loss, enc_cls_agn, distill):
    """the argument checks of :func:`device_criterion`: -> the tensor arguments and ``cfg`` of :func:`set_criterion_forward`"""
    if fed_loss:
        raise NotImplementedError("device_criterion: the federated loss over capacity buffers is device_set_criterion(fed=...)")
    if enc_cls_agn:
        raise NotImplementedError("device_criterion: class-agnostic two-stage targets are device_set_criterion(enc_cls_agn=True)")
    if distill:
        raise NotImplementedError("device_criterion: the distillation term over capacity buffers is not built (the teacher's ROI rows are one "
                                  "per target)")
    tensors = (logits, coords, il, ib, query_of_target, targets.offsets_dev, targets.tgt_ids, targets.tgt_boxes)
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors) or any(t is not None and not t.is_cuda for t in (dn_meta, num_boxes)):
        raise RuntimeError("Not implemented on the CPU")
    if any(t.dtype != torch.float32 for t in (logits, coords, il, ib, targets.tgt_boxes)):
        raise TypeError("device_criterion: logits, coords, il, ib and the target boxes are float32 tensors")
    if query_of_target.dtype != torch.int64 or targets.offsets_dev.dtype != torch.int64 or targets.tgt_ids.dtype != torch.int64:
        raise TypeError("device_criterion: query_of_target, the target prefix and the target labels are int64 tensors")
    pad_cap, cap = int(pad_cap), int(targets.total)
    if logits.dim() != 4 or il.dim() != 3 or pad_cap < 0 or logits.shape[2] <= pad_cap or cap < 1:
        raise ValueError("device_criterion: logits is (nl, N, pad_cap + Q, C) with Q >= 1, il is (N, Qi, C), the target capacity >= 1")
    nl, N, QT, C = logits.shape
    if tuple(coords.shape) != (nl, N, QT, 4) or il.shape[0] != N or il.shape[2] != C or tuple(ib.shape) != (N, il.shape[1], 4):
        raise ValueError("device_criterion: coords is (nl, N, pad_cap + Q, 4), il (N, Qi, C) and ib (N, Qi, 4) for logits (nl, N, pad_cap + Q, C)")
    if tuple(query_of_target.shape) != (nl + 1, cap) or not query_of_target.is_contiguous():
        raise ValueError(f"device_criterion: query_of_target is a contiguous ({nl + 1}, {cap}) tensor: one row per output, one column per target slot")
    if targets.offsets_dev.numel() != N + 1 or tuple(targets.tgt_ids.shape) != (cap,) or tuple(targets.tgt_boxes.shape) != (cap, 4):
        raise ValueError("device_criterion: the target buffers were built for another image count or capacity")
    if dn_meta is not None and (dn_meta.dtype != torch.int64 or dn_meta.numel() != 5 or not dn_meta.is_contiguous()):
        raise TypeError("device_criterion: dn_meta is the contiguous int64[5] meta of denoising_queries")
    if num_boxes is not None and (num_boxes.dtype != torch.float32 or num_boxes.numel() != 1):
        raise TypeError("device_criterion: num_boxes is a (1,) float32 tensor")
    cfg = (pad_cap, cap, float(alpha), float(c_cls), float(c_l1), float(c_giou))
    return (logits, coords, il, ib, targets.offsets_dev, targets.tgt_ids.contiguous(), targets.tgt_boxes.contiguous(), query_of_target, dn_meta,
            num_boxes, cfg)


def _apply(args, class_mask, enc_cls_agn, late_status):
    """the autograd form of the four front ends: -> (loss, terms, status); outside a capture the status goes to ``late_status``"""
    loss, terms, status = DeviceCriterionFunction.apply(*args, class_mask, enc_cls_agn)
    if late_status is not None and not torch.cuda.is_current_stream_capturing():
        late_status.push(status.view(1, 4))
    return loss, terms, status


def _forward_and_backward(args, class_mask, enc_cls_agn, grad_loss):
    """the form WITHOUT the autograd engine: -> (loss, terms, status, (grad_logits, grad_coords, grad_il, grad_ib))"""
    loss, terms, status, saved = set_criterion_forward(*args, class_mask, enc_cls_agn)
    g = torch.ones(1, dtype=torch.float32, device=loss.device) if grad_loss is None else grad_loss
    return loss, terms, status, set_criterion_backward(saved, g)


def device_criterion(logits, coords, il, ib, targets, query_of_target, dn_meta=None, *, pad_cap, alpha=0.25, c_cls=1.0, c_l1=5.0, c_giou=2.0,
                     num_boxes=None, fed_loss=False, enc_cls_agn=False, distill=False, late_status=None):
    """The classification (sigmoid focal) and box (L1, GIoU) terms of the criterion over all outputs of a step, pairs found on the device.

    ``logits`` (nl, N, pad_cap + Q, C) / ``coords`` (nl, N, pad_cap + Q, 4) float32: the nl decoder outputs, ``pad_cap`` denoising rows before the
    Q matching rows; ``il`` (N, Qi, C) / ``ib`` (N, Qi, 4): the two-stage output; ``targets``: a :class:`~richsem_amd.matcher.TargetBuffers` (or
    a ``CostPlan``: the exact-size case); ``query_of_target`` (nl + 1, targets.total) int64: ``match_many_device``'s result for the nl + 1
    outputs on the same ``targets``; ``dn_meta``: the int64[5] ``meta`` of ``denoising_queries`` run with the same ``pad_cap`` (None: no
    denoising part -- the first ``pad_cap`` rows then carry no loss); ``num_boxes``: a (1,) float32 device tensor used as the normaliser instead
    of the kernel's own count (a DDP caller's all-reduced value).

    -> ``(loss, terms, status)``: ``loss`` 0-dim float32 = c_cls * focal + c_l1 * L1 + c_giou * (1 - GIoU) summed over the reference's
    2 nl + 1 ``get_loss`` calls, each normalised as there (what ``Step.loss_part`` forms for these terms); ``terms`` (2 nl + 1, 3): per call --
    matching parts of layers 0..nl-1, their denoising parts, the two-stage output -- the positive entries' focal correction, L1 and 1 - GIoU
    (no gradient); ``status`` int32[4] = ``STATUS``, zeros when all is well.  Outside a capture the status goes to ``late_status`` (a
    ``matcher.LateStatus``) when one is given: it raises one step late.  Nothing waits, no allocation depends on the counts: capturable
    after one eager call.  Bitwise reproducible.  CPU tensors raise: there is no CPU fallback."""
    args = _checked(logits, coords, il, ib, targets, query_of_target, dn_meta, pad_cap, alpha, c_cls, c_l1, c_giou, num_boxes, fed_loss,
                    enc_cls_agn, distill)
    return _apply(args, None, False, late_status)


@torch.no_grad()
def device_criterion_and_grads(logits, coords, il, ib, targets, query_of_target, dn_meta=None, *, pad_cap, alpha=0.25, c_cls=1.0, c_l1=5.0,
                               c_giou=2.0, num_boxes=None, grad_loss=None):
    """:func:`device_criterion` and its backward in one call, WITHOUT the autograd engine: -> (loss, terms, status, (grad_logits, grad_coords,
    grad_il, grad_ib)) for d / d loss = ``grad_loss`` (a device scalar; default 1).  For a caller that schedules the backward itself -- a
    whole step captured into one graph on the capturing thread.  Same arguments, checks and launches as :func:`device_criterion`."""
    args = _checked(logits, coords, il, ib, targets, query_of_target, dn_meta, pad_cap, alpha, c_cls, c_l1, c_giou, num_boxes, False, False, False)
    return _forward_and_backward(args, None, False, grad_loss)


# ---- the reference's remaining switches: the federated loss (use_fed_loss) and class-agnostic two-stage targets ------------------------
def _checked_set(logits, il, targets, query_of_target, dn_meta, pad_cap, fed, enc_cls_agn, generator):
    """the checks of :func:`device_set_criterion` beyond :func:`_checked`, and the draw: -> (class_mask or None, fed_out)"""
    if fed is None:
        return None, None
    nl, C = logits.shape[0], logits.shape[-1]
    if isinstance(fed, FedClassSampler):
        if fed.num_classes != C:
            raise ValueError(f"device_set_criterion: the sampler draws from {fed.num_classes} classes, the logits have {C}")
        mask, n_chosen = fed.sample_slots(targets, query_of_target, dn_meta, nl=nl, Q=logits.shape[2] - int(pad_cap), Qi=il.shape[1],
                                          enc_cls_agn=enc_cls_agn, generator=generator)
        return mask, (mask, n_chosen)
    if not torch.is_tensor(fed):
        raise TypeError("device_set_criterion: fed is a FedClassSampler, a float32 (2 nl + 1, C) tensor of class masks, or None")
    if not fed.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if fed.dtype != torch.float32 or tuple(fed.shape) != (2 * nl + 1, C):
        raise ValueError(f"device_set_criterion: the class masks are a float32 ({2 * nl + 1}, {C}) tensor: one class subset per get_loss call")
    mask = fed.detach().contiguous()
    return mask, (mask, (mask != 0).sum(1, dtype=torch.int32))


def device_set_criterion(logits, coords, il, ib, targets, query_of_target, dn_meta=None, *, pad_cap, fed=None, enc_cls_agn=False, generator=None,
                         alpha=0.25, c_cls=1.0, c_l1=5.0, c_giou=2.0, num_boxes=None, late_status=None):
    """:func:`device_criterion` with the two remaining switches of the reference's ``SetCriterion``, over the same capacity buffers.

    ``fed`` -- the federated loss (``use_fed_loss``, richsem.py:938-964 with fed_loss.py:15-25): every get_loss call takes the focal loss over
    a class subset only.  A :class:`~richsem_amd.fed_loss.FedClassSampler`: ``torch.rand((2 nl + 1, C), generator=generator)`` on the current
    stream, then ``msda_fed_class_mask_slots_f32`` reads each call's appeared classes from the slot space -- the live pairs of THAT call in the
    batch the buffers hold now, so a captured call draws for the batch of each replay, with fresh uniforms -- and tops them up to
    ``num_sample_cats``.  A float32 (2 nl + 1, C) tensor: those subsets, nothing is drawn (frozen draws; the caller answers for every
    positive class lying inside its row).  Rows are numbered as ``terms``.  ``enc_cls_agn`` -- class-agnostic two-stage targets
    (richsem.py:1249-1255): the two-stage output's positives are class 0, in the loss and in its appeared classes; match it against
    ``targets.class_agnostic()`` (``match_many_device(..., last_plan=...)``).

    -> ``(loss, terms, status, fed_out)``: the first three as :func:`device_criterion`; ``fed_out`` = ``(class_mask (2 nl + 1, C) float32,
    n_chosen (2 nl + 1) int32)`` or None without ``fed``.  Without either switch: the launches and bits of :func:`device_criterion`.  One
    autograd node; the logit gradients are exactly 0 off the subsets.  Nothing waits: capturable after one eager call (which also copies the
    sampler's weights to the device); bitwise reproducible for given uniforms.  CPU tensors raise: there is no CPU fallback."""
    args = _checked(logits, coords, il, ib, targets, query_of_target, dn_meta, pad_cap, alpha, c_cls, c_l1, c_giou, num_boxes, False, False, False)
    mask, fed_out = _checked_set(logits, il, targets, query_of_target, dn_meta, pad_cap, fed, bool(enc_cls_agn), generator)
    return _apply(args, mask, bool(enc_cls_agn), late_status) + (fed_out,)


@torch.no_grad()
def device_set_criterion_and_grads(logits, coords, il, ib, targets, query_of_target, dn_meta=None, *, pad_cap, fed=None, enc_cls_agn=False,
                                   generator=None, alpha=0.25, c_cls=1.0, c_l1=5.0, c_giou=2.0, num_boxes=None, grad_loss=None):
    """:func:`device_set_criterion` and its backward in one call, WITHOUT the autograd engine, as :func:`device_criterion_and_grads`:
    -> (loss, terms, status, fed_out, (grad_logits, grad_coords, grad_il, grad_ib))"""
    args = _checked(logits, coords, il, ib, targets, query_of_target, dn_meta, pad_cap, alpha, c_cls, c_l1, c_giou, num_boxes, False, False, False)
    mask, fed_out = _checked_set(logits, il, targets, query_of_target, dn_meta, pad_cap, fed, bool(enc_cls_agn), generator)
    loss, terms, status, grads = _forward_and_backward(args, mask, bool(enc_cls_agn), grad_loss)
    return loss, terms, status, fed_out, grads


class CriterionStatus(LateStatus):
    """``matcher.LateStatus`` for the status of :func:`device_criterion`: the error text names the entry of ``STATUS`` that was set"""

    @staticmethod
    def _message(host):
        what = ", ".join(f"{name} = {int(v)}" for name, v in zip(STATUS, host.reshape(-1).tolist()) if v)
        return f"device_criterion (the previous step): {what}"
