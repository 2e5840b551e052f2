"""Plain-torch restatement of the reference's ``PostProcess`` (models/richsem/richsem.py:1309-1367) and of torchvision's ``nms`` /
``batched_nms`` (their published definitions: greedy suppression in descending score order; a per-class loop for the batched form), in
float32 on whatever device the inputs are on.  The comparator of tests/test_postprocess_abi.py (against the committed fixture) and of
tests/test_gpu_postprocess.py (for inputs that are not in the fixture).  Test helper only: the package never imports it."""
import numpy as np
import torch


def box_cxcywh_to_xyxy(x):
    x_c, y_c, w, h = x.unbind(-1)
    return torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)


def iou_matrix(boxes):
    """(K, K) IoU of xyxy boxes in the boxes' dtype, torchvision's operation order: inter / (area_a + area_b - inter)"""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lt = torch.max(boxes[:, None, :2], boxes[None, :, :2])
    rb = torch.min(boxes[:, None, 2:], boxes[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area[:, None] + area[None, :] - inter)


def nms(boxes, scores, iou_threshold):
    """indices of the kept boxes, in descending score order"""
    order = torch.sort(scores, descending=True, stable=True)[1]
    above = (iou_matrix(boxes[order]) > iou_threshold).cpu().numpy()      # (NaN > thr is False: a 0 / 0 suppresses nothing)
    n = len(order)
    dead = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= above[i, i + 1:]
    return order[torch.as_tensor(keep, dtype=torch.int64, device=boxes.device)]


def batched_nms(boxes, scores, labels, iou_threshold):
    keep_mask = torch.zeros_like(scores, dtype=torch.bool)
    for class_id in torch.unique(labels):
        idx = torch.where(labels == class_id)[0]
        keep_mask[idx[nms(boxes[idx], scores[idx], iou_threshold)]] = True
    keep = torch.where(keep_mask)[0]
    return keep[torch.sort(scores[keep], descending=True, stable=True)[1]]


def postprocess(logits, boxes, target_sizes, num_select, nms_iou_threshold=-1, use_opt=False, not_to_xyxy=False, test=False):
    """the body of the reference's forward; returns (results, query_idx (B, k), item_indices or None)"""
    prob = logits.float().sigmoid()
    scores, topk_indexes = torch.topk(prob.view(logits.shape[0], -1), num_select, dim=1)
    topk_boxes = topk_indexes // logits.shape[2]
    labels = topk_indexes % logits.shape[2]
    bx = boxes if not_to_xyxy else box_cxcywh_to_xyxy(boxes)
    if test:
        assert not not_to_xyxy
        bx = torch.cat((bx[:, :, :2], bx[:, :, 2:] - bx[:, :, :2]), -1)
    bx = torch.gather(bx, 1, topk_boxes.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = target_sizes.unbind(1)
    bx = bx * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]
    item_indices = None
    if use_opt:
        item_indices = [batched_nms(b, s, l, 0.7) for b, s, l in zip(bx, scores, labels)]
    elif nms_iou_threshold > 0:
        item_indices = [nms(b, s, nms_iou_threshold) for b, s in zip(bx, scores)]
    if item_indices is not None:
        results = [{'scores': s[i], 'labels': l[i], 'boxes': b[i]} for s, l, b, i in zip(scores, labels, bx, item_indices)]
    else:
        results = [{'scores': s, 'labels': l, 'boxes': b} for s, l, b in zip(scores, labels, bx)]
    return results, topk_boxes, item_indices


def decode_boxes(boxes, query_idx, target_sizes, box_mode):
    """the float32 torch composition of the box part alone, for given winners: box_mode 0 cxcywh, 1 xyxy, 2 xywh, times (w, h, w, h)"""
    bx = boxes if box_mode == 0 else box_cxcywh_to_xyxy(boxes)
    if box_mode == 2:
        bx = torch.cat((bx[:, :, :2], bx[:, :, 2:] - bx[:, :, :2]), -1)
    bx = torch.gather(bx, 1, query_idx.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = target_sizes.float().unbind(1)
    return bx * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :]


def stable_topk(x, k):
    """(rows, k) int64: per row of a float32 numpy array the k largest in descending order, equal values lowest index first
    (-0.0 == +0.0; NaN is not handled)"""
    return np.stack([np.argsort(-row, kind="stable")[:k] for row in x]).astype(np.int64)


def shuffled_linspace(lo, hi, B, n, seed):
    """(B, n) float32: every row a random permutation of linspace(lo, hi, n)"""
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(lo, hi, n, dtype=torch.float32)
    return torch.stack([base[torch.randperm(n, generator=g)] for _ in range(B)])


def clustered_boxes(K, seed, clusters=None, size=1000.0):
    """(K, 4) float32 xyxy boxes drawn around a few centres, so that many pairs overlap strongly"""
    g = torch.Generator().manual_seed(seed)
    clusters = clusters or max(1, K // 6)
    centre = torch.rand(clusters, 2, generator=g) * 0.6 + 0.2
    extent = torch.rand(clusters, 2, generator=g) * 0.15 + 0.08
    which = torch.randint(0, clusters, (K,), generator=g)
    c = centre[which] + (torch.rand(K, 2, generator=g) - 0.5) * 0.25 * extent[which]
    e = extent[which] * (1 + (torch.rand(K, 2, generator=g) - 0.5) * 0.5)
    return (torch.cat((c - 0.5 * e, c + 0.5 * e), -1) * size).float()


def decidable_clustered_boxes(K, seed, thresholds, margin=1e-5, **kw):
    """clustered_boxes of the first seed in seed, seed + 1000, ... whose draw has no pair's IoU within `margin` of a threshold (a property
    of the input alone: float32 IoU rounding is of order 1e-7, so every correct implementation agrees on such a draw)"""
    for s in range(seed, seed + 50000, 1000):
        boxes = clustered_boxes(K, s, **kw)
        if iou_margin(boxes, thresholds) > margin:
            return boxes
    raise AssertionError("no decidable draw")


def iou_margin(boxes, thresholds):
    """smallest |IoU - t| over all pairs i < j and all t, IoU in float64 from the float32 boxes"""
    iou = iou_matrix(boxes.double().cpu())
    iu = torch.triu_indices(len(boxes), len(boxes), 1)
    v = iou[iu[0], iu[1]]
    v = v[~torch.isnan(v)]
    return min(float((v - t).abs().min()) for t in thresholds) if len(v) else float("inf")
