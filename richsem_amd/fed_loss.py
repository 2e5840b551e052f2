"""The criterion's federated loss (reference ``models/richsem/fed_loss.py:15-25`` through ``SetCriterion.loss_labels``, richsem.py:930-961,
``use_fed_loss=True, fed_num_sample_cats=50``): every ``loss_labels`` call takes the sigmoid focal loss over a class subset only -- the classes
among the matched targets, topped up to ``num_sample_cats`` by weighted draws without replacement (``get_fed_loss_inds``) -- with a fresh
draw per call.

The reference draws on the host (``torch.unique``, ``len``, ``torch.multinomial`` on a CPU weight): three or more blocking waits per call,
and nothing a graph can hold.  Here the draw is one kernel with fixed shapes (``msda_fed_class_mask_f32``, csrc/msda_fed.h: the
exponential race, the same distribution as ``torch.multinomial(w, m, replacement=False)``) on uniforms from ``torch.rand`` on the current
stream -- PyTorch's RNG is graph-safe, so a captured draw replays with fresh numbers -- and the focal loss over the drawn classes is the
all-negative kernel with a class mask per row (:class:`MaskedFocalNegativeSum`); the positive entries need no change, every positive class
is an appeared class and so always in the mask (matcher.FocalPositiveSum).

One difference: where fewer classes are eligible (weight > 0, not appeared) than are to be drawn, ``torch.multinomial`` raises; a graph
cannot, so every eligible class is taken, and ``n_chosen`` tells.
"""
import torch

from . import _lib, focal

MAX_CLASSES = 4096      # msda::kFedMaxClasses: one group's keys sort in LDS


def class_weights_from_image_counts(counts, C, power=0.5):
    """The reference's ``SetCriterion.set_cats`` weight (richsem.py:930-936): ``image_count ** power`` per class id, as float32 (C).
    ``counts``: a ``{class_id: image_count}`` mapping -- or the dataset's ``cats`` itself, ``{class_id: {'image_count': n, ...}}`` -- or a dense
    tensor / sequence of counts.  Ids without a category get weight 0, as ``cats.get(x, {'image_count': 0})`` gives them; ids >= C are an error."""
    if isinstance(counts, dict):
        dense = torch.zeros(C, dtype=torch.int64)
        for k, v in counts.items():
            k = int(k)
            if not 0 <= k < C:
                raise ValueError(f"class id {k} outside [0, {C})")
            dense[k] = int(v["image_count"] if isinstance(v, dict) else v)
    else:
        dense = torch.as_tensor(counts).detach().cpu().reshape(-1)
        if dense.numel() > C:
            raise ValueError(f"{dense.numel()} counts for {C} classes")
        dense = torch.cat((dense, dense.new_zeros(C - dense.numel())))
    if bool((dense < 0).any()):
        raise ValueError("negative image count")
    return dense.float() ** power      # (the reference: an int64 tensor ** 0.5 -> float32)


class FedClassSampler:
    """``get_fed_loss_inds`` (fed_loss.py:15-25) for ``groups`` calls at once, on the device, without a host sync.

    ``FedClassSampler(num_sample_cats=50, class_weight=None, num_classes=None)``: ``class_weight`` (C) as
    :func:`class_weights_from_image_counts` gives it; ``None`` = uniform over ``num_classes`` classes, as ``get_fed_loss_inds(weight=None)``.
    ``sample(labels, groups, generator=None)`` -> ``(mask (groups, C) float32, n_chosen (groups) int32)``: row g holds 1 at the classes of
    ``labels`` (the matched targets' classes, any shape, may be empty) and at ``max(num_sample_cats - appeared, 0)`` classes drawn with
    probability proportional to the weight, independently per row; ``n_chosen[g] = max(num_sample_cats, appeared)`` unless fewer classes are
    eligible."""

    def __init__(self, num_sample_cats=50, class_weight=None, num_classes=None):
        if class_weight is None:
            if num_classes is None:
                raise ValueError("uniform weights need num_classes")
            class_weight = torch.ones(int(num_classes), dtype=torch.float32)
        w = torch.as_tensor(class_weight).detach().float().reshape(-1)
        if not 1 <= w.numel() <= MAX_CLASSES:
            raise ValueError(f"{w.numel()} classes: the sampler takes 1 .. {MAX_CLASSES}")
        if int(num_sample_cats) < 0:
            raise ValueError("num_sample_cats < 0")
        self.num_sample_cats = int(num_sample_cats)
        self.num_classes = w.numel()
        self.class_weight = w.cpu()
        self._dev_weight = {}      # device -> the weight there (copied once, outside any capture: the first call on a device warms it up)

    def weight_on(self, dev):
        w = self._dev_weight.get(dev)
        if w is None:
            w = self._dev_weight[dev] = self.class_weight.to(dev).contiguous()
        return w

    def sample(self, labels, groups, generator=None):
        if not labels.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        dev, C, groups = labels.device, self.num_classes, int(groups)
        lab = labels.reshape(-1).to(torch.int64).contiguous()
        u = torch.rand((groups, C), device=dev, generator=generator)
        mask = torch.empty((groups, C), dtype=torch.float32, device=dev)
        n_chosen = torch.empty(groups, dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().msda_fed_class_mask_f32(lab.data_ptr() if lab.numel() else None, lab.numel(), self.weight_on(dev).data_ptr(),
                                                           u.data_ptr(), groups, C, self.num_sample_cats, mask.data_ptr(), n_chosen.data_ptr(),
                                                           _lib.raw_stream(dev)))
        return mask, n_chosen

    def sample_slots(self, targets, query_of_target, dn_meta, *, nl, Q, Qi, enc_cls_agn=False, generator=None):
        """:meth:`sample` for the 2 nl + 1 get_loss calls of a step over CAPACITY buffers (``msda_fed_class_mask_slots_f32``): the appeared
        classes of each call are read on the device from ``targets`` (a ``matcher.TargetBuffers``), ``query_of_target`` (nl + 1, capacity) and
        ``dn_meta`` (or None) -- the live pairs ``criterion.device_set_criterion`` counts in that call, of the batch the buffers hold when the
        launch RUNS -- so a captured call serves every batch.  Rows: matching parts of layers 0..nl-1, their denoising parts, the two-stage
        output (``enc_cls_agn``: its class is 0).  -> ``(mask (2 nl + 1, C) float32, n_chosen (2 nl + 1) int32)``."""
        cum, ids = targets.offsets_dev, targets.tgt_ids
        if not all(torch.is_tensor(t) and t.is_cuda for t in (cum, ids, query_of_target)) or (dn_meta is not None and not dn_meta.is_cuda):
            raise RuntimeError("Not implemented on the CPU")
        dev, C, nl, cap = query_of_target.device, self.num_classes, int(nl), int(targets.total)
        if any(t.dtype != torch.int64 for t in (cum, ids, query_of_target)) or (dn_meta is not None and dn_meta.dtype != torch.int64):
            raise TypeError("sample_slots: the target prefix, the labels, query_of_target and dn_meta are int64 tensors")
        if tuple(query_of_target.shape) != (nl + 1, cap) or not query_of_target.is_contiguous() or tuple(ids.shape) != (cap,) or cum.numel() < 2:
            raise ValueError(f"sample_slots: query_of_target is a contiguous ({nl + 1}, {cap}) tensor, the labels ({cap},)")
        if dn_meta is not None and (dn_meta.numel() != 5 or not dn_meta.is_contiguous()):
            raise ValueError("sample_slots: dn_meta is the contiguous int64[5] meta of denoising_queries")
        groups = 2 * nl + 1
        u = torch.rand((groups, C), device=dev, generator=generator)
        mask = torch.empty((groups, C), dtype=torch.float32, device=dev)
        n_chosen = torch.empty(groups, dtype=torch.int32, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.load().msda_fed_class_mask_slots_f32(
                cum.data_ptr(), ids.contiguous().data_ptr(), query_of_target.data_ptr(), None if dn_meta is None else dn_meta.data_ptr(),
                self.weight_on(dev).data_ptr(), u.data_ptr(), nl, cum.numel() - 1, int(Q), int(Qi), C, cap, self.num_sample_cats,
                1 if enc_cls_agn else 0, mask.data_ptr(), n_chosen.data_ptr(), _lib.raw_stream(dev)))
        return mask, n_chosen


class MaskedFocalNegativeSum(torch.autograd.Function):
    """:class:`richsem_amd.matcher.FocalNegativeSum` with the classes of each row restricted to a class subset:
    ``sum_rows w[row] * sum_c mask[group[row], c] * (1 - alpha) * sigmoid(x)^2 * softplus(x)`` -- the all-negative term of the reference's
    ``sigmoid_focal_loss(src_logits[..., fed_ids], ...)`` (richsem.py:956-961) for many outputs and draws at once.  One kernel forward, one
    backward (``msda_focal_neg_sum_masked_f32 / msda_focal_neg_grad_masked_f32``); the gradient is exactly 0 off the mask, and an all-ones
    mask gives FocalNegativeSum's bits.  ``apply(logits (..., C) float32, row_weight (...) float32, row_group (...) int32, class_mask (G, C)
    float32 0 / 1, alpha)`` -> 0-dim float32."""

    @staticmethod
    def forward(ctx, logits, row_weight, row_group, class_mask, alpha):
        if not logits.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert logits.dtype == torch.float32 and row_weight.dtype == torch.float32 and row_weight.numel() * logits.shape[-1] == logits.numel()
        assert row_group.dtype == torch.int32 and row_group.numel() == row_weight.numel()
        assert class_mask.dtype == torch.float32 and class_mask.dim() == 2 and class_mask.shape[1] == logits.shape[-1]
        x, w, grp, m = logits.contiguous(), row_weight.contiguous(), row_group.contiguous(), class_mask.detach().contiguous()
        ctx.save_for_backward(x, w, grp, m)
        ctx.alpha = float(alpha)
        with _lib.on_device(x.device):
            return focal.neg_sum(x, w, ctx.alpha, grp, m).sum().float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w, grp, m = ctx.saved_tensors
        with _lib.on_device(x.device):
            return focal.neg_grad(x, w, ctx.alpha, g.reshape(1).float().contiguous(), grp, m), None, None, None, None


def fed_ids(mask_row):
    """the class ids one mask row selects, ascending, on the host (tests, debugging: it synchronises)"""
    return torch.nonzero(mask_row.detach().cpu() != 0).flatten()
