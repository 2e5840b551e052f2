"""Host-side mirror of the integer part of the reference's ``prepare_for_cdn`` (models/richsem/dn_components.py:11-193): the
denoising-group arithmetic on the host (plain Python ints, as the reference) and the index / mask tensors on the device
(kernels richsem_amd/csrc/msda_dn.h, C ABI ``msda_dn_indices_i64`` / ``msda_dn_attn_mask_u8``).  SURVEY.md section 8 row a12:
int64 / bool work, bit-exact.  ``prepare_dn_layout`` leaves the noisy labels / boxes and the embeddings to its caller.

``denoising_queries`` is the whole of ``prepare_for_cdn`` from the target counts ON THE DEVICE (kernels richsem_amd/csrc/msda_dn_noise.h,
C ABI ``msda_dn_queries_f32`` / ``msda_dn_queries_backward_f32``): noised labels and boxes, the label embedding, the padded query block,
the mask and the meta data in one launch into buffers of a fixed capacity, with no host synchronisation -- a captured call follows the
batch whose counts its ``cum`` tensor holds at the replay.
"""
import torch

from . import _lib


def dn_group_count(dn_number, known_num, add_gt=False):
    """dn_components.py:27-41: denoising groups from the configured dn_number and the per-image ground-truth counts."""
    dn_number = dn_number * 2
    mx = int(max(known_num)) if len(known_num) else 0
    if mx == 0:
        dn_number = 1
    elif dn_number >= 100:
        dn_number = dn_number // (mx * 2)
    elif dn_number < 1:
        dn_number = 1
    if dn_number == 0:
        dn_number = 1
    if add_gt:
        dn_number += 1
    return dn_number


def prepare_dn_layout(known_num, dn_number, num_queries, use_cdn=True, add_gt=False, device="cuda"):
    """known_num: ground-truth boxes per image; dn_number as configured (before the reference's scaling).  Returns a dict with
    the reference's names: ``known_bid``, ``map_known_indice`` (int64), ``attn_mask`` (bool (tgt, tgt)), ``positive_idx`` /
    ``negative_idx`` (int64), ``pad_size``, ``num_dn_group``, ``single_pad``, ``group_pad``."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("Not implemented on the CPU")
    known_num = [int(k) for k in known_num]
    batch = len(known_num)
    groups = dn_group_count(dn_number, known_num, add_gt)
    total = sum(known_num)
    single_pad = int(max(known_num)) if batch else 0
    pad_size = single_pad * 2 * groups
    lib = _lib.load()
    stream = _lib.raw_stream(dev)
    cum = torch.tensor([0] + list(torch.tensor(known_num, dtype=torch.int64).cumsum(0).tolist()) if batch else [0], dtype=torch.int64,
                       device=dev)
    n = total * 2 * groups
    known_bid = torch.empty(n, dtype=torch.int64, device=dev)
    map_known_indice = torch.empty(n, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        if batch and n:
            _lib.check(lib.msda_dn_indices_i64(cum.data_ptr(), batch, total, 2 * groups, single_pad, known_bid.data_ptr(),
                                               map_known_indice.data_ptr(), stream))
        # dn_components.py:58-61: positive_idx = arange(total) + 2 * total * group, negative_idx = positive_idx + total
        grp = torch.arange(groups, dtype=torch.int64, device=dev)[:, None]
        positive_idx = (torch.arange(total, dtype=torch.int64, device=dev)[None, :] + grp * (total * 2)).flatten()
        negative_idx = positive_idx + total
        if use_cdn:
            group_pad = single_pad * 2
        else:   # dn_components.py:144-151: the negative halves are dropped; positive_idx now selects the padded slots of the
            # positive halves (single_pad per group), the caller applies it to the padded query tensors
            positive_idx = (torch.arange(single_pad, dtype=torch.int64, device=dev)[None, :] + grp * (single_pad * 2)).flatten()
            pad_size = pad_size // 2
            group_pad = single_pad
        tgt = pad_size + num_queries
        mask = torch.empty((tgt, tgt), dtype=torch.uint8, device=dev)
        _lib.check(lib.msda_dn_attn_mask_u8(mask.data_ptr(), tgt, pad_size, group_pad, stream))
    return {"known_bid": known_bid, "map_known_indice": map_known_indice, "attn_mask": mask.view(torch.bool),
            "positive_idx": positive_idx, "negative_idx": negative_idx, "pad_size": pad_size, "num_dn_group": groups,
            "single_pad": single_pad, "group_pad": group_pad}


def dn_capacity(dn_number, max_targets, add_gt=False, use_cdn=True):
    """the largest ``pad_size`` the reference can produce for any batch whose largest per-image target count is <= ``max_targets``: the
    capacity (``pad_cap``) that ``denoising_queries`` never overflows on such batches.  For the shipped dn_number = 100:
    max(200, 2 * max_targets)."""
    best = 0
    for m in range(int(max_targets) + 1):
        pad = m * 2 * dn_group_count(dn_number, [m], add_gt)
        best = max(best, pad if use_cdn else pad // 2)
    return best


META = ("single_pad", "num_dn_group", "pad_size", "total", "overflow")      # the int64[5] ``meta`` of denoising_queries


def _dn_backward(grad_q_label, noised_label, V):
    """the one call site of ``msda_dn_queries_backward_f32``"""
    g = grad_q_label.contiguous()
    D = g.shape[-1]
    grad_table = torch.empty((V, D), dtype=torch.float32, device=g.device)
    with _lib.on_device(g.device):
        _lib.check(_lib.load().msda_dn_queries_backward_f32(g.data_ptr(), noised_label.data_ptr(), noised_label.numel(), D, V,
                                                            grad_table.data_ptr(), _lib.raw_stream(g.device)))
    return grad_table


class DenoisingQueriesFunction(torch.autograd.Function):
    """``denoising_queries`` as an autograd node: a gradient for ``table`` only (labels, boxes and the uniforms get none, as in the
    reference, whose boxes are detached targets).  ``cfg`` = (pad_cap, num_queries, num_classes, dn_number, label_noise_ratio,
    box_noise_scale, use_cdn, add_gt); ``bufs`` = the output buffers (q_label, q_bbox, noised_label, noised_box, attn_mask, meta)."""

    @staticmethod
    def forward(ctx, table, cum, labels, boxes, uniform, cfg, bufs):
        pad_cap, num_queries, num_classes, dn_number, label_noise_ratio, box_noise_scale, use_cdn, add_gt = cfg
        q_label, q_bbox, noised_label, noised_box, attn_mask, meta = bufs
        N, (V, D), dev = cum.numel() - 1, table.shape, table.device
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        with _lib.on_device(dev):
            _lib.check(_lib.load().msda_dn_queries_f32(
                cum.data_ptr(), ptr(labels), ptr(boxes), labels.shape[0], ptr(uniform), table.data_ptr(), N, pad_cap, D, V, num_classes,
                num_queries, dn_number, label_noise_ratio, box_noise_scale, int(use_cdn), int(add_gt), ptr(q_label), ptr(q_bbox),
                ptr(noised_label), ptr(noised_box), ptr(attn_mask), meta.data_ptr(), _lib.raw_stream(dev)))
        ctx.save_for_backward(noised_label)
        ctx.V = V
        ctx.mark_non_differentiable(q_bbox, noised_label, attn_mask, meta)
        # (a new tensor on the buffer's storage takes this call's history: the buffer itself stays a plain tensor for the next call)
        return q_label.detach(), q_bbox, noised_label, attn_mask, meta

    @staticmethod
    def backward(ctx, grad_q_label, *unused):
        noised_label, = ctx.saved_tensors
        return _dn_backward(grad_q_label, noised_label, ctx.V), None, None, None, None, None, None


def denoising_queries(cum, labels, boxes, table, uniform, *, pad_cap, num_queries, num_classes, dn_number, label_noise_ratio,
                      box_noise_scale, use_cdn=True, add_gt=False, check_pos_dn=False, out=None):
    """The reference's ``prepare_for_cdn`` (training branch) from device tensors, in one launch and with no host synchronisation.

    ``cum`` (N + 1) int64: exclusive prefix of the per-image target counts; ``labels`` (cap) int64 and ``boxes`` (cap, 4) float32 cxcywh:
    the targets of all images one after the other, in buffers of any capacity >= cum[N]; ``table`` (V, D) float32: the rows ``label_enc``
    looks up (``nn.Embedding.weight``); ``uniform`` (N, pad_cap, 10) float32 in [0, 1), drawn by the caller (``torch.rand``: inside a
    captured region every replay draws anew): p, u_label, u_sign[4], u_part[4] per slot.  ``pad_cap``: the capacity of the query block
    (``dn_capacity``, or the exact ``pad_size`` of a batch).

    Returns ``(q_label (N, pad_cap, D), q_bbox (N, pad_cap, 4), attn_mask (pad_cap + num_queries)^2 bool, noised_label (N, pad_cap) int64,
    meta int64[5])`` -- ``meta`` = ``META``: single_pad, num_dn_group, pad_size, total, overflow, all on the device.  Slots past
    ``pad_size`` and slots of images with fewer targets are zero rows with label -1; a layout that does not fit ``pad_cap`` sets
    ``overflow`` and leaves every slot empty (a graph cannot raise: read ``meta`` late, as the matcher's status).  ``q_label`` carries the
    gradient for ``table``.  ``out``: the dict of buffers of an earlier call (``out=`` of ``dn_buffers``), written again: the call then
    allocates nothing.  CPU tensors raise: there is no CPU fallback."""
    if check_pos_dn:
        raise NotImplementedError("denoising_queries: check_pos_dn=True (the reference's iterative IoU check) is not built; every shipped "
                                  "config has it False")
    if not all(torch.is_tensor(t) and t.is_cuda for t in (cum, labels, boxes, table, uniform)):
        raise RuntimeError("Not implemented on the CPU")
    N, pad_cap, num_queries = cum.numel() - 1, int(pad_cap), int(num_queries)
    if cum.dtype != torch.int64 or cum.dim() != 1 or N < 1 or not cum.is_contiguous():
        raise TypeError("denoising_queries: cum is a contiguous (N + 1) int64 tensor, N >= 1")
    if labels.dtype != torch.int64 or labels.dim() != 1 or boxes.dtype != torch.float32 or tuple(boxes.shape) != (labels.shape[0], 4) or \
            not labels.is_contiguous() or not boxes.is_contiguous():
        raise TypeError("denoising_queries: labels is a contiguous (cap) int64 tensor and boxes a contiguous (cap, 4) float32 tensor")
    if table.dtype != torch.float32 or table.dim() != 2 or not table.is_contiguous():
        raise TypeError("denoising_queries: table is a contiguous (V, D) float32 tensor")
    if uniform.dtype != torch.float32 or tuple(uniform.shape) != (N, pad_cap, 10) or not uniform.is_contiguous():
        raise TypeError(f"denoising_queries: uniform is a contiguous ({N}, {pad_cap}, 10) float32 tensor")
    if out is None:
        out = dn_buffers(N, pad_cap, num_queries, table.shape[1], table.device)
    elif tuple(out["q_label"].shape) != (N, pad_cap, table.shape[1]) or out["attn_mask"].shape[0] != pad_cap + num_queries or \
            out["q_label"].device != table.device:
        raise ValueError("denoising_queries: `out` was made for another batch size, capacity, width, query count or device")
    cfg = (pad_cap, num_queries, int(num_classes), int(dn_number), float(label_noise_ratio), float(box_noise_scale), bool(use_cdn),
           bool(add_gt))
    bufs = tuple(out[k] for k in ("q_label", "q_bbox", "noised_label", "noised_box", "attn_mask", "meta"))
    q_label, q_bbox, noised_label, attn_mask, meta = DenoisingQueriesFunction.apply(table, cum, labels, boxes, uniform, cfg, bufs)
    return q_label, q_bbox, attn_mask.view(torch.bool), noised_label, meta


def dn_buffers(N, pad_cap, num_queries, D, device):
    """the output buffers of ``denoising_queries`` (its ``out=``): allocated once, written by every call -- the static outputs of a graph.
    ``noised_box`` (N, pad_cap, 4), the noised boxes before ``inverse_sigmoid``, is kept here for tests and inspection."""
    f32, tgt = dict(dtype=torch.float32, device=device), pad_cap + num_queries
    return {"q_label": torch.empty((N, pad_cap, D), **f32), "q_bbox": torch.empty((N, pad_cap, 4), **f32),
            "noised_label": torch.empty((N, pad_cap), dtype=torch.int64, device=device), "noised_box": torch.empty((N, pad_cap, 4), **f32),
            "attn_mask": torch.empty((tgt, tgt), dtype=torch.uint8, device=device), "meta": torch.empty(5, dtype=torch.int64, device=device)}


def topk_indices(scores, k, return_values=False):
    """``torch.topk(scores, k, dim=1)[1]`` for a (rows, n) float32 tensor on the GPU (deformable_transformer.py:370-372: the 900
    encoder proposals with the largest class score), one workgroup per row: indices in descending order of the score, equal scores
    lowest index first.  Rows too long for the kernel (n > 36864) or k > 1024 go to ``torch.topk``."""
    if not scores.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    assert scores.dim() == 2 and scores.dtype == torch.float32
    rows, n = scores.shape
    if n > 36864 or k > 1024:
        v, i = torch.topk(scores, k, dim=1)
        return (i, v) if return_values else i
    s = scores.contiguous()
    idx = torch.empty((rows, k), dtype=torch.int64, device=s.device)
    val = torch.empty((rows, k), dtype=torch.float32, device=s.device) if return_values else None
    with _lib.on_device(s.device):
        _lib.check(_lib.load().msda_topk_f32(s.data_ptr(), rows, n, k, idx.data_ptr(), val.data_ptr() if val is not None else None,
                                             _lib.raw_stream(s.device)))
    return (idx, val) if return_values else idx
