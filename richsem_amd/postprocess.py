"""The reference's ``PostProcess`` (models/richsem/richsem.py:1309-1367; what ``build_richsem`` returns as ``postprocessors['bbox']``) on the
device: the top ``num_select`` of an image's query x class scores, their boxes in absolute coordinates and, optionally, ``nms`` /
``batched_nms`` of those boxes.  Kernels: richsem_amd/csrc/msda_postproc.h behind ``msda_postprocess_select`` / ``msda_nms_f32``.

The selection runs on the raw logits (sigmoid is monotone): no probability tensor is made and only the winners get a sigmoid.  Equal logits
are taken lowest flat index first, so the result is determined by the input (``torch.topk`` leaves that order open).  torchvision is not
needed: both NMS forms of the reference are the library's.
"""
import ctypes

import torch
from torch import nn

from . import _lib

MAX_SELECT = 1024      # msda_postprocess_select: k <= 1024; msda_nms_f32: K <= 1024

_workspaces = {}       # (device, B, Q, C, k) -> uint8 tensor of msda_postprocess_workspace_bytes() bytes


def _workspace(dev, B, Q, C, k):
    """The cached workspace of a shape.  Under stream capture a call never takes it from, or puts it into, the cache: memory
    allocated while capturing lives in the graph's private pool and goes back to the allocator with the graph, so a cached tensor from
    there would dangle; and a cached tensor from outside would tie the graph's replays to the eager calls' workspace.  A capture
    therefore gets a workspace of its own from the graph's pool (the call zeroes what it counts in, so its contents do not matter).  It
    is freed on return, so later allocations of the same capture may reuse it -- behind the selection's kernels in stream order only:
    the captured forms must stay on the capturing stream."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.load().msda_postprocess_workspace_bytes(B, Q, C, k, ctypes.byref(n)))
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n.value, dtype=torch.uint8, device=dev)
    key = (dev, B, Q, C, k)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.empty(n.value, dtype=torch.uint8, device=dev)
    return ws


def release_workspaces():
    """Drop the cached workspaces (a few hundred KB per shape seen); the next call of a shape allocates its own again."""
    _workspaces.clear()


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def select(pred_logits, pred_boxes, target_sizes, k, box_mode=1):
    """Per image the ``k`` largest of the (Q, C) logits in descending order: ``(scores (B, k) f32, labels (B, k) i64, boxes (B, k, 4) f32,
    query_idx (B, k) i64)``.  ``box_mode`` 0: the boxes as they are (cx, cy, w, h), 1: xyxy, 2: xywh -- each times (w, h, w, h) of
    ``target_sizes`` (B, 2) = (height, width).  float32 or bfloat16 logits are read as they are, other types as float32.  Device work only:
    no synchronisation, capturable without a rehearsal.  The workspace is cached per (device, B, Q, C, k) and belongs to one stream at a
    time: eager calls of one shape on two streams that may overlap are the caller's to order.  A captured call does not use the cache: it
    owns a workspace in its graph's pool, so replays and eager calls never share one."""
    if not (pred_logits.is_cuda and pred_boxes.is_cuda and target_sizes.is_cuda):
        raise RuntimeError("Not implemented on the CPU")
    assert pred_logits.dim() == 3 and pred_boxes.dim() == 3 and pred_boxes.shape[-1] == 4 and pred_boxes.shape[:2] == pred_logits.shape[:2]
    B, Q, C = pred_logits.shape
    assert tuple(target_sizes.shape) == (B, 2)
    dev = pred_logits.device
    if pred_logits.dtype not in (torch.float32, torch.bfloat16):
        pred_logits = pred_logits.float()
    logits, boxes = _aligned(pred_logits), _aligned(pred_boxes.float())
    sizes = target_sizes.to(torch.float32).contiguous()
    scores = torch.empty((B, k), dtype=torch.float32, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    query_idx = torch.empty((B, k), dtype=torch.int64, device=dev)
    out_boxes = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        ws = _workspace(dev, B, Q, C, k)
        _lib.check(_lib.load().msda_postprocess_select(logits.data_ptr(), int(logits.dtype == torch.bfloat16), boxes.data_ptr(), sizes.data_ptr(),
                                                       B, Q, C, k, box_mode, scores.data_ptr(), labels.data_ptr(), out_boxes.data_ptr(),
                                                       query_idx.data_ptr(), ws.data_ptr(), _lib.raw_stream(dev)))
    return scores, labels, out_boxes, query_idx


def nms_padded(boxes, labels=None, iou_threshold=0.5):
    """torchvision's ``nms`` (``labels`` None) / ``batched_nms`` of (B, K, 4) xyxy boxes that are in descending score order, K <= 1024:
    ``(keep (B, K) bool, kept_idx (B, K) i64: the kept positions in that order, then -1, n_kept (B) i32)``.  Device work only."""
    if not boxes.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    assert boxes.dim() == 3 and boxes.shape[-1] == 4
    B, K = boxes.shape[:2]
    dev = boxes.device
    bx = _aligned(boxes.float())
    lb = None
    if labels is not None:
        assert tuple(labels.shape) == (B, K)
        lb = labels.to(torch.int64).contiguous()
    keep = torch.empty((B, K), dtype=torch.uint8, device=dev)
    kept_idx = torch.empty((B, K), dtype=torch.int64, device=dev)
    n_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(_lib.load().msda_nms_f32(bx.data_ptr(), lb.data_ptr() if lb is not None else None, B, K, float(iou_threshold),
                                            keep.data_ptr(), kept_idx.data_ptr(), n_kept.data_ptr(), _lib.raw_stream(dev)))
    return keep.view(torch.bool), kept_idx, n_kept


class PostProcess(nn.Module):
    """ This module converts the model's output into the format expected by the coco api (drop-in for the reference's class)"""

    def __init__(self, num_select=100, nms_iou_threshold=-1, use_opt=False) -> None:
        super().__init__()
        self.num_select = num_select
        self.nms_iou_threshold = nms_iou_threshold
        self.use_opt = use_opt

    def select(self, pred_logits, pred_boxes, target_sizes, box_mode=1):
        return select(pred_logits, pred_boxes, target_sizes, self.num_select, box_mode)

    @staticmethod
    def nms_padded(boxes, labels=None, iou_threshold=0.5):
        return nms_padded(boxes, labels, iou_threshold)

    @torch.no_grad()
    def forward(self, outputs, target_sizes, not_to_xyxy=False, test=False):
        """outputs: the model's ``pred_logits`` (B, Q, C) and ``pred_boxes`` (B, Q, 4); target_sizes (B, 2): (height, width) of each image.
        Returns the reference's list of ``{'scores', 'labels', 'boxes'}`` per image."""
        out_logits, out_bbox = outputs['pred_logits'], outputs['pred_boxes']

        assert len(out_logits) == len(target_sizes)
        assert target_sizes.shape[1] == 2
        if test:
            assert not not_to_xyxy
        if not (out_logits.is_cuda and target_sizes.is_cuda):
            raise RuntimeError("Not implemented on the CPU")

        scores, labels, boxes, topk_boxes = self.select(out_logits, out_bbox, target_sizes, 0 if not_to_xyxy else (2 if test else 1))
        if 'pred_masks' in outputs:
            bs, nq_topk = topk_boxes.shape
            outputs['pred_masks'] = torch.gather(outputs['pred_masks'], 1, topk_boxes.view(
                bs, nq_topk, 1, 1, 1).expand(-1, -1, -1, *outputs['pred_masks'].shape[-2:]))

        if self.use_opt or self.nms_iou_threshold > 0:
            if self.use_opt:
                _, kept_idx, n_kept = nms_padded(boxes, labels, 0.7)
            else:
                _, kept_idx, n_kept = nms_padded(boxes, None, self.nms_iou_threshold)
            counts = n_kept.tolist()      # the one host read: the results have variable lengths
            item_indices = [kept_idx[b, :n] for b, n in enumerate(counts)]
            results = [{'scores': s[i], 'labels': l[i], 'boxes': b[i]} for s, l, b, i in zip(scores, labels, boxes, item_indices)]
            if self.use_opt:
                outputs['item_indices'] = item_indices
        else:
            results = [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, boxes)]
        return results
