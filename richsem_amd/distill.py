"""The criterion's CLIP distillation term (reference ``SetCriterion.loss_labels``, models/richsem/richsem.py:967-1024): the detector's
CLIP-space outputs pulled toward the frozen CLIP teacher's -- a KL divergence of class distributions (``distill_type='clip_logits'``) or an L1
distance of unit vectors (``'clip_l1'``) -- for the objectives ``'gt'`` (the matched queries against their targets' teacher rows), ``'pred'``
(the matched queries against the teacher's rows for the same queries) and ``'pred_all'`` (every query), with the reference's
``use_dynamic_distill_weight`` and ``use_fed_on_kd`` switches.

The reference forms it as gathers, two softmaxes, ``kl_div`` and their autograd chain -- about a dozen small launches each way -- on a float32
copy of the student's logits.  Here it is one row kernel (csrc/msda_distill.h, ``msda_distill_kl_{f32,bf16}`` / ``msda_distill_l1_f32``): the
gather is part of the kernel, value and compact gradient come from the same launch, the student's logits may stay in bf16, nothing
synchronises and nothing uses a floating-point atomic.  Two differences from the reference, both where it would return NaN: an underflowed
teacher probability contributes 0 to the dynamic weight's entropy (the reference's ``p * p.log()`` is NaN there), and rows whose index lies
outside the tensor are skipped (the reference's indexing raises).
"""
import math

import torch

from . import _lib

DISTILL_TYPES = ("clip_logits", "clip_l1")
OBJECTIVES = ("gt", "pred", "pred_all")


def _rows(t, what):
    if t.dim() < 2:
        raise ValueError(f"{what}: at least (rows, channels)")
    return t.reshape(-1, t.shape[-1])


def _index(t, dev):
    return t.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _common(name, pred, tgt, pred_row, tgt_row, row_weight, dtypes):
    if not pred.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if pred.dtype not in dtypes:
        raise TypeError(f"{name}: pred must be {' or '.join(str(d) for d in dtypes)}, not {pred.dtype}")
    dev = pred.device
    x, y = _rows(pred.detach(), "pred").contiguous(), _rows(tgt.detach(), "tgt").to(device=dev, dtype=torch.float32).contiguous()
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"{name}: pred has {x.shape[1]} channels, tgt {y.shape[1]}")
    pr, tr = _index(pred_row, dev), _index(tgt_row, dev)
    w = row_weight.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if tr.numel() != pr.numel() or w.numel() != pr.numel():
        raise ValueError(f"{name}: pred_row, tgt_row and row_weight must have one entry per row")
    return x, y, pr, tr, w


def _launch(fn, x, K, *args):
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    grad_rows = torch.empty((K, x.shape[1]), dtype=torch.float32, device=x.device)
    # the workgroups' f64 partials: the caller's memory (here the caching allocator's, which orders its reuse by stream and keeps a
    # captured graph's buffers in the graph's pool)
    workspace = torch.empty(_lib.DISTILL_WORKSPACE_BYTES // 8 if K else 0, dtype=torch.float64, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(fn(*args, _ptr(workspace), loss.data_ptr(), _ptr(grad_rows), _lib.raw_stream(x.device)))
    return loss, grad_rows


def kl_rows(pred, tgt, pred_row, tgt_row, row_weight, row_group=None, class_mask=None, dynamic_weight=False):
    """``msda_distill_kl_f32`` / ``_bf16`` (by ``pred``'s dtype) as they are: -> ``(loss (1) float32, grad_rows (K, C) float32, pred_row (K)
    int64 on the device)``.  No autograd: :class:`DistillKL` is this with the scatter as its backward."""
    x, y, pr, tr, w = _common("DistillKL", pred, tgt, pred_row, tgt_row, row_weight, (torch.float32, torch.bfloat16))
    K, C = pr.numel(), x.shape[1]
    if (row_group is None) != (class_mask is None):
        raise ValueError("DistillKL: row_group and class_mask go together")
    grp = m = None
    if class_mask is not None:
        m = class_mask.detach().to(device=x.device, dtype=torch.float32).contiguous()
        grp = row_group.to(device=x.device, dtype=torch.int32).reshape(-1).contiguous()
        if m.dim() != 2 or m.shape[1] != C or m.shape[0] < 1 or grp.numel() != K:
            raise ValueError("DistillKL: class_mask is (groups, C), row_group (K)")
    L = _lib.load()
    fn = L.msda_distill_kl_bf16 if x.dtype == torch.bfloat16 else L.msda_distill_kl_f32
    loss, grad_rows = _launch(fn, x, K, _ptr(x), x.shape[0], _ptr(y), y.shape[0], C, _ptr(pr), _ptr(tr), _ptr(w), K,
                              grp.data_ptr() if grp is not None else None, m.data_ptr() if m is not None else None,
                              m.shape[0] if m is not None else 0, int(bool(dynamic_weight)))
    return loss, grad_rows, pr


def l1_rows(pred, tgt, pred_row, tgt_row, row_weight, normalize_target=False):
    """``msda_distill_l1_f32`` as it is: -> ``(loss (1) float32, grad_rows (K, D) float32, pred_row (K) int64 on the device)``"""
    x, y, pr, tr, w = _common("DistillL1", pred, tgt, pred_row, tgt_row, row_weight, (torch.float32,))
    K = pr.numel()
    loss, grad_rows = _launch(_lib.load().msda_distill_l1_f32, x, K, _ptr(x), x.shape[0], _ptr(y), y.shape[0], x.shape[1], _ptr(pr), _ptr(tr),
                              _ptr(w), K, int(bool(normalize_target)))
    return loss, grad_rows, pr


class _RowLoss(torch.autograd.Function):
    """value and compact gradient from one launch (like matcher._PairSum); the backward scatters ``grad_out * grad_rows`` into a zero
    gradient of ``pred``'s shape with ``index_add_`` on ``pred_row``: rows that repeat add"""

    @staticmethod
    def _keep(ctx, pred, n_inputs, loss, grad_rows, pred_row):
        ctx.save_for_backward(grad_rows, pred_row)
        ctx.pred_shape, ctx.pred_dtype, ctx.n_inputs = pred.shape, pred.dtype, n_inputs
        return loss[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        grad_rows, pred_row = ctx.saved_tensors
        rows = math.prod(ctx.pred_shape[:-1])
        gp = grad_rows.new_zeros((rows, ctx.pred_shape[-1]))
        # A row outside [0, rows) has a zero gradient row -- the kernel's guard, held by tests/test_gpu_distill.py -- so clamped it adds 0.
        # (Masking it here as well was measured: five more launches per backward, 7 -> 12 per call.)
        if rows and pred_row.numel():
            gp.index_add_(0, pred_row.clamp(0, rows - 1), grad_rows * g)
        return (gp.reshape(ctx.pred_shape).to(ctx.pred_dtype),) + (None,) * (ctx.n_inputs - 1)


class DistillKL(_RowLoss):
    """``sum_k w_k dw_k KL(softmax(tgt[tgt_row[k]] over S_k) || softmax(pred[pred_row[k]] over S_k))`` as one kernel
    (``msda_distill_kl_f32`` / ``_bf16``, include/richsem_msda.h).

    ``apply(pred (..., C) float32 or bfloat16, tgt (..., C) float32, pred_row (K) int64, tgt_row (K) int64, row_weight (K) float32,
    row_group (K) int32 or None, class_mask (G, C) float32 or None, dynamic_weight)`` -> the 0-dim float32 sum.  Rows index the tensors
    flattened to (rows, C).  ``S_k`` = every class, or those with ``class_mask[row_group[k]] != 0``; ``dw_k`` = 1 or, with
    ``dynamic_weight``, twice the entropy of the teacher's full-row softmax over ``ln C``.  Gradient for ``pred`` only (in ``pred``'s dtype)."""

    @staticmethod
    def forward(ctx, pred, tgt, pred_row, tgt_row, row_weight, row_group=None, class_mask=None, dynamic_weight=False):
        return _RowLoss._keep(ctx, pred, 8, *kl_rows(pred, tgt, pred_row, tgt_row, row_weight, row_group, class_mask, dynamic_weight))


class DistillL1(_RowLoss):
    """``sum_k w_k |pred[pred_row[k]] / |.|_2 - v_k|_1`` with ``v_k = tgt[tgt_row[k]]`` (objective 'gt') or that row over its 2-norm
    (``normalize_target``: 'pred', 'pred_all'), as one kernel (``msda_distill_l1_f32``).  ``apply(pred (..., D) float32, tgt (..., D) float32,
    pred_row (K) int64, tgt_row (K) int64, row_weight (K) float32, normalize_target)`` -> 0-dim float32; gradient for ``pred``."""

    @staticmethod
    def forward(ctx, pred, tgt, pred_row, tgt_row, row_weight, normalize_target=False):
        return _RowLoss._keep(ctx, pred, 6, *l1_rows(pred, tgt, pred_row, tgt_row, row_weight, normalize_target))


class DistillLoss:
    """``loss_distill`` of the reference's ``loss_labels`` (richsem.py:967-1024), branch by branch.

    ``DistillLoss(distill_type, objective, dynamic_weight=False, fed_on_kd=False)``: ``distill_type`` 'clip_logits' (KL; student
    ``outputs['pred_clip_logits']``) or 'clip_l1' (student ``outputs['pred_hs']``); ``objective`` 'gt', 'pred' or 'pred_all';
    ``dynamic_weight`` = use_dynamic_distill_weight and ``fed_on_kd`` = use_fed_on_kd (both act on the KL form only, as in the reference).

    ``loss(outputs, num_boxes, batch_idx=None, src_idx=None, teacher=None, teacher_idx=None, fed_mask=None)`` -> 0-dim float32:

    * 'gt': ``teacher`` holds the targets' teacher rows -- ``t['clip_logits']`` (KL) or ``t['clip_prompt']`` (L1) of every image concatenated,
      (T, C) -- and ``teacher_idx`` (K) the row of each matched pair in it (None: the rows are already in matched order); the student rows
      are ``outputs[...][batch_idx, src_idx]`` (the packed ``_get_src_permutation_idx``).  Normalised by ``num_boxes``.
    * 'pred': student and teacher (``outputs['clip_logits']`` / ``outputs['hs_prompt']``, normalised for L1) at the same ``[batch_idx,
      src_idx]``; by ``num_boxes``.
    * 'pred_all': every query against the teacher's row for it (identity row indices); by ``bs * nq``.
    * ``fed_mask`` (C) or (1, C), 0 / 1: the class subset of ``use_fed_on_kd`` (the ``fed_ids`` of the same ``loss_labels`` call, as
      ``fed_loss.FedClassSampler`` draws them).  ``fed_on_kd`` without it raises, as the reference fails on an undefined ``fed_ids``.

    ``stacked(...)``: the rows of several outputs in one call."""

    def __init__(self, distill_type, objective, dynamic_weight=False, fed_on_kd=False):
        if distill_type not in DISTILL_TYPES:
            raise NotImplementedError(f"distill_type {distill_type!r}: one of {DISTILL_TYPES}")
        if objective not in OBJECTIVES:
            raise NotImplementedError(f"clip_distill_objective {objective!r}: one of {OBJECTIVES}")
        self.distill_type, self.objective = distill_type, objective
        self.dynamic_weight, self.fed_on_kd = bool(dynamic_weight), bool(fed_on_kd)

    @property
    def kl(self):
        return self.distill_type == "clip_logits"

    def _mask(self, fed_mask, dev):
        if not (self.kl and self.fed_on_kd):
            return None
        if fed_mask is None:
            raise ValueError("fed_on_kd needs the class subset of this loss_labels call (fed_mask)")
        return fed_mask.detach().to(device=dev, dtype=torch.float32).reshape(-1, fed_mask.shape[-1])

    def loss(self, outputs, num_boxes, batch_idx=None, src_idx=None, teacher=None, teacher_idx=None, fed_mask=None):
        pred = outputs["pred_clip_logits" if self.kl else "pred_hs"]
        if not pred.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        if pred.dim() != 3:
            raise ValueError("the student's output is (bs, nq, channels)")
        dev = pred.device
        bs, nq = pred.shape[:2]
        if self.objective == "pred_all":
            rows = torch.arange(bs * nq, device=dev)
            tgt, tgt_rows, norm = outputs["clip_logits" if self.kl else "hs_prompt"], rows, float(bs * nq)
        else:
            if batch_idx is None or src_idx is None:
                raise ValueError(f"objective {self.objective!r} needs the matched (batch_idx, src_idx)")
            rows = _index(batch_idx, dev) * nq + _index(src_idx, dev)
            norm = float(num_boxes)
            if self.objective == "pred":
                tgt, tgt_rows = outputs["clip_logits" if self.kl else "hs_prompt"], rows
            else:
                if teacher is None:
                    raise ValueError("objective 'gt' needs the targets' teacher rows")
                tgt = teacher
                tgt_rows = torch.arange(rows.numel(), device=dev) if teacher_idx is None else _index(teacher_idx, dev)
        w = torch.full((rows.numel(),), 1.0 / norm, dtype=torch.float32, device=dev)
        if not self.kl:
            return DistillL1.apply(pred, tgt, rows, tgt_rows, w, self.objective != "gt")
        mask = self._mask(fed_mask, dev)
        grp = None if mask is None else torch.zeros(rows.numel(), dtype=torch.int32, device=dev)
        return DistillKL.apply(pred, tgt, rows, tgt_rows, w, grp, mask, self.dynamic_weight)

    __call__ = loss

    def stacked(self, pred, tgt, pred_row, tgt_row, row_weight, row_group=None, class_mask=None):
        """The rows of several outputs -- the decoder layers of ``distill_aux_layers``, their denoising parts -- in ONE call: ``pred``
        (..., C) stacked over the outputs (rows index it flattened), ``tgt`` (..., C) the teacher rows, and per row k its student row,
        teacher row, weight (1 / that output's normaliser) and, with ``fed_on_kd``, the draw ``row_group[k]`` of ``class_mask`` (G, C) its
        ``loss_labels`` call uses.  The sum over the outputs of what :meth:`loss` returns for each."""
        if not pred.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        if not self.kl:
            return DistillL1.apply(pred, tgt, pred_row, tgt_row, row_weight, self.objective != "gt")
        if self.fed_on_kd:
            if class_mask is None or row_group is None:
                raise ValueError("fed_on_kd needs the class subsets (class_mask) and each row's draw (row_group)")
        else:
            row_group = class_mask = None
        return DistillKL.apply(pred, tgt, pred_row, tgt_row, row_weight, row_group, class_mask, self.dynamic_weight)


# ---- the term over CAPACITY buffers: pairs found on the device (csrc/msda_distill_pairs.h) ---------------------------------------------------

def _capacity_checked(pred, teacher, targets, query_of_target, dn_meta, pad_cap, layers, distill_type, objective, class_mask, num_boxes):
    """the argument checks of :func:`device_distill`: -> ``cfg`` = (nl, N, Q, pad_cap, capacity, C, layer_mask, n_d, kl, objective index)"""
    if distill_type not in DISTILL_TYPES:
        raise NotImplementedError(f"distill_type {distill_type!r}: one of {DISTILL_TYPES}")
    if objective == "pred_all":
        raise ValueError("device_distill: objective 'pred_all' pairs every query with the teacher's row for it -- no per-batch shape, nothing "
                         "to find on the device: use DistillLoss('...', 'pred_all')")
    if objective not in ("gt", "pred"):
        raise NotImplementedError(f"clip_distill_objective {objective!r}: one of {OBJECTIVES}")
    kl = distill_type == "clip_logits"
    if pred.dtype not in ((torch.float32, torch.bfloat16) if kl else (torch.float32,)):
        raise TypeError(f"device_distill: the student's tensor is float32{' or bfloat16' if kl else ''}, not {pred.dtype}")
    if teacher.dtype != torch.float32:
        raise TypeError("device_distill: the teacher's rows are float32")
    if query_of_target.dtype != torch.int64 or targets.offsets_dev.dtype != torch.int64:
        raise TypeError("device_distill: query_of_target and the target prefix are int64 tensors")
    tensors = (pred, teacher, query_of_target, targets.offsets_dev)
    if not all(t.is_cuda for t in tensors) or any(t is not None and not t.is_cuda for t in (dn_meta, num_boxes, class_mask)):
        raise RuntimeError("Not implemented on the CPU")
    pad_cap, cap = int(pad_cap), int(targets.total)
    if pred.dim() != 4 or pad_cap < 0 or pred.shape[2] <= pad_cap or cap < 1:
        raise ValueError("device_distill: pred is (n_d, N, pad_cap + Q, C) with Q >= 1, the target capacity >= 1")
    n_d, N, QT, C = pred.shape
    if query_of_target.dim() != 2 or query_of_target.shape[1] != cap or query_of_target.shape[0] < 2 or not query_of_target.is_contiguous():
        raise ValueError(f"device_distill: query_of_target is a contiguous (nl + 1, {cap}) tensor: one row per output, one column per target slot")
    nl = query_of_target.shape[0] - 1
    layers = sorted(set(int(l) for l in layers))
    if len(layers) != n_d or not layers or layers[0] < 0 or layers[-1] >= nl or nl > 63:
        raise ValueError(f"device_distill: layers names {len(layers)} distinct decoder layers in 0..{nl - 1}, pred stacks {n_d}")
    if targets.offsets_dev.numel() != N + 1:
        raise ValueError("device_distill: the target buffers were built for another image count")
    want = (cap, C) if objective == "gt" else tuple(pred.shape)
    if tuple(teacher.shape) != want:
        raise ValueError(f"device_distill: objective {objective!r} takes a teacher of shape {want}, not {tuple(teacher.shape)}")
    if dn_meta is not None and (dn_meta.dtype != torch.int64 or dn_meta.numel() != 5 or not dn_meta.is_contiguous()):
        raise TypeError("device_distill: dn_meta is the contiguous int64[5] meta of denoising_queries")
    if num_boxes is not None and (num_boxes.dtype != torch.float32 or num_boxes.numel() != 1):
        raise TypeError("device_distill: num_boxes is a (1,) float32 tensor")
    if class_mask is not None:
        if not kl:
            raise ValueError("device_distill: class_mask (use_fed_on_kd) acts on the KL form only")
        if class_mask.dtype != torch.float32 or tuple(class_mask.shape) != (2 * n_d, C):
            raise ValueError(f"device_distill: class_mask is a float32 ({2 * n_d}, {C}) tensor: one class subset per get_loss call")
    return nl, N, QT - pad_cap, pad_cap, cap, C, sum(1 << l for l in layers), n_d, kl, OBJECTIVES.index(objective)


def distill_pairs(targets, query_of_target, dn_meta, num_boxes, cfg):
    """the one call of ``msda_distill_pairs``: -> (pred_row (K) int64, tgt_row (K) int64, row_weight (K) float32, row_group (K) int32, status
    int32[4]) for the K = n_d * capacity + n_d * N * pad_cap slots of ``cfg`` (:func:`_capacity_checked`)"""
    nl, N, Q, pad_cap, cap, _, mask, n_d, _, obj = cfg
    dev = query_of_target.device
    K = n_d * (cap + N * pad_cap)
    pred_row, tgt_row = torch.empty(K, dtype=torch.int64, device=dev), torch.empty(K, dtype=torch.int64, device=dev)
    w, grp = torch.empty(K, dtype=torch.float32, device=dev), torch.empty(K, dtype=torch.int32, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.load().msda_distill_pairs(targets.offsets_dev.data_ptr(), query_of_target.data_ptr(), _ptr(dn_meta), _ptr(num_boxes), nl, N, Q,
                                                  pad_cap, cap, mask, obj, pred_row.data_ptr(), tgt_row.data_ptr(), w.data_ptr(), grp.data_ptr(),
                                                  status.data_ptr(), _lib.raw_stream(dev)))
    return pred_row, tgt_row, w, grp, status


def distill_capacity_forward(pred, teacher, targets, query_of_target, dn_meta, num_boxes, class_mask, dynamic_weight, cfg):
    """the forward half on checked tensors: pairs launch + the existing row kernel -> (loss (1) float32, status, saved); ``saved`` is what
    :func:`distill_capacity_backward` takes"""
    kl, obj = cfg[8], cfg[9]
    pred_row, tgt_row, w, grp, status = distill_pairs(targets, query_of_target, dn_meta, num_boxes, cfg)
    x = pred.detach().contiguous()
    if kl:
        loss, grad_rows, _ = kl_rows(x, teacher, pred_row, tgt_row, w, grp if class_mask is not None else None, class_mask, dynamic_weight)
    else:
        loss, grad_rows, _ = l1_rows(x, teacher, pred_row, tgt_row, w, normalize_target=obj != 0)
    return loss, status, (grad_rows, pred_row, targets.offsets_dev, cfg, pred.dtype)


def distill_capacity_backward(saved, g):
    """the backward half (``msda_distill_scatter_f32`` / ``_bf16``): ``g`` = d / d loss (a float32 device scalar) -> the gradient of ``pred``,
    written whole by one launch"""
    grad_rows, pred_row, cum, cfg, dtype = saved
    _, N, Q, pad_cap, cap, C, _, n_d, _, _ = cfg
    dev = grad_rows.device
    gs = g.detach().reshape(1).float().contiguous()
    gp = torch.empty((n_d, N, pad_cap + Q, C), dtype=dtype, device=dev)
    fn = _lib.load().msda_distill_scatter_bf16 if dtype == torch.bfloat16 else _lib.load().msda_distill_scatter_f32
    with _lib.on_device(dev):
        _lib.check(fn(grad_rows.data_ptr(), pred_row.data_ptr(), cum.data_ptr(), gs.data_ptr(), n_d, N, Q, pad_cap, cap, C, gp.data_ptr(),
                      _lib.raw_stream(dev)))
    return gp


class DeviceDistillFunction(torch.autograd.Function):
    """:func:`device_distill` as one autograd node: gradient for ``pred`` only"""

    @staticmethod
    def forward(ctx, pred, teacher, targets, query_of_target, dn_meta, num_boxes, class_mask, dynamic_weight, cfg):
        loss, status, saved = distill_capacity_forward(pred, teacher, targets, query_of_target, dn_meta, num_boxes, class_mask, dynamic_weight, cfg)
        ctx.save_for_backward(*saved[:3])
        ctx.rest = saved[3:]
        ctx.mark_non_differentiable(status)
        return loss[0], status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_status):
        return (distill_capacity_backward(tuple(ctx.saved_tensors) + ctx.rest, g),) + (None,) * 8


def device_distill(pred, teacher, targets, query_of_target, dn_meta=None, *, pad_cap, layers, distill_type, objective, dynamic_weight=False,
                   class_mask=None, num_boxes=None, late_status=None):
    """The distillation term of the criterion over all distilled outputs of a step, pairs found on the device: what
    :meth:`DistillLoss.stacked` returns on the index rows of ``pairs_from_query_of_target`` and the denoising positives, without a tensor whose
    shape follows the batch -- so ONE captured graph serves every batch that fits the capacities.  The caller adds it to
    ``criterion.device_criterion``'s loss (times its coefficient).

    ``pred`` (n_d, N, pad_cap + Q, C) float32 (KL: or bfloat16): the student's CLIP-space output of the ``n_d`` decoder layers ``layers``
    names (distinct, stacked in increasing order), ``pad_cap`` denoising rows before the Q matching rows; ``teacher`` float32: for objective
    'gt' (targets.total, C), the target slots' teacher rows (``clip_box_targets_capacity``: logits for 'clip_logits', prompts for 'clip_l1'),
    for 'pred' the teacher's output for every query, shaped like ``pred``; ``targets``: a ``matcher.TargetBuffers`` (or ``CostPlan``);
    ``query_of_target`` (nl + 1, targets.total) int64 and ``dn_meta``: as for ``device_criterion``; ``class_mask`` (2 n_d, C) float32: the
    class subsets of ``use_fed_on_kd``, one per get_loss call -- the matching parts of the distilled layers, then their denoising parts;
    ``num_boxes``: a (1,) float32 device tensor instead of the kernel's own count.  'pred_all' raises ValueError (:class:`DistillLoss`).

    -> ``(loss, status)``: the 0-dim float32 sum over the 2 n_d calls, each normalised as the reference does (num_boxes, num_boxes *
    num_dn_group); ``status`` int32[4] = ``criterion.STATUS`` (word 2 stays 0), pushed to ``late_status`` outside a capture.  Launches:
    the pair kernel, the row kernel and its total; backward: one scatter that writes the gradient whole with plain stores.  Nothing waits,
    no atomic, bitwise reproducible.  CPU tensors raise: there is no CPU fallback."""
    cfg = _capacity_checked(pred, teacher, targets, query_of_target, dn_meta, pad_cap, layers, distill_type, objective, class_mask, num_boxes)
    loss, status = DeviceDistillFunction.apply(pred, teacher.contiguous(), targets, query_of_target, dn_meta, num_boxes,
                                               None if class_mask is None else class_mask.contiguous(), bool(dynamic_weight), cfg)
    if late_status is not None and not torch.cuda.is_current_stream_capturing():
        late_status.push(status.view(1, 4))
    return loss, status


@torch.no_grad()
def device_distill_and_grads(pred, teacher, targets, query_of_target, dn_meta=None, *, pad_cap, layers, distill_type, objective,
                             dynamic_weight=False, class_mask=None, num_boxes=None, grad_loss=None):
    """:func:`device_distill` and its backward in one call, WITHOUT the autograd engine: -> (loss, status, grad_pred) for d / d loss =
    ``grad_loss`` (a device scalar; default 1).  For a caller that schedules the backward itself -- a whole step captured into one graph on
    the capturing thread (``criterion.device_criterion_and_grads``).  Same arguments, checks and launches."""
    cfg = _capacity_checked(pred, teacher, targets, query_of_target, dn_meta, pad_cap, layers, distill_type, objective, class_mask, num_boxes)
    loss, status, saved = distill_capacity_forward(pred, teacher.contiguous(), targets, query_of_target, dn_meta, num_boxes,
                                                   None if class_mask is None else class_mask.contiguous(), bool(dynamic_weight), cfg)
    g = torch.ones(1, dtype=torch.float32, device=loss.device) if grad_loss is None else grad_loss
    return loss[0], status, distill_capacity_backward(saved, g)


_MASK_ROWS = {}      # (layers, nl, device) -> the static row index of distill_class_mask


def distill_class_mask(class_mask, layers, nl):
    """The (2 n_d, C) ``class_mask`` of :func:`device_distill` from the (2 nl + 1, C) subsets ``criterion.device_set_criterion`` returns
    (``fed_out[0]``): the matching-part rows of the distilled ``layers``, then their denoising-part rows -- so ``use_fed_on_kd`` sees the
    subsets ``loss_ce`` of the same get_loss call saw, as in the reference (richsem.py:959, :990-991).  One ``index_select`` with an index
    that depends on ``layers`` and ``nl`` only: it is built on the first call for a device (a host -> device copy: outside a capture), a
    captured call replays the select."""
    nl = int(nl)
    layers = tuple(sorted(set(int(l) for l in layers)))
    if not layers or layers[0] < 0 or layers[-1] >= nl:
        raise ValueError(f"distill_class_mask: layers names distinct decoder layers in 0..{nl - 1}")
    if class_mask.dim() != 2 or class_mask.shape[0] != 2 * nl + 1:
        raise ValueError(f"distill_class_mask: class_mask is ({2 * nl + 1}, C): one class subset per get_loss call")
    key = (layers, nl, class_mask.device)
    rows = _MASK_ROWS.get(key)
    if rows is None:
        rows = _MASK_ROWS[key] = torch.tensor(list(layers) + [nl + l for l in layers], dtype=torch.int64).to(class_mask.device)
    return class_mask.index_select(0, rows)
