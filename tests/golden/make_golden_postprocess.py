#!/usr/bin/env python3
"""Golden vectors for the on-device PostProcess (richsem_amd/postprocess.py; ``msda_postprocess_select`` / ``msda_nms_f32``), generated
from the REFERENCE's own class.  Run in the build container only (it reads the reference checkout; the fixture is committed, the GPU box
never sees the reference):

    python tests/golden/make_golden_postprocess.py

What is executed is the reference's code:
  * ``PostProcess`` of ``models/richsem/richsem.py:1309-1367``, cut out of the source with ``ast`` (the file imports the whole model);
  * ``box_cxcywh_to_xyxy`` of ``util/box_ops.py:9-13``, cut out the same way.
torchvision is absent: ``nms`` / ``batched_nms`` are restated from their published definitions (greedy suppression in descending score
order with ``inter / (area_a + area_b - inter) > threshold``; a per-class loop for the batched form).  Everything runs in float32, as the
reference does.

The generator asserts what makes the fixture decidable by any correct implementation:
  * the logits of an image are a permutation of linspace(-8, 6, Q * C): the top k + 1 probabilities differ pairwise by >= 2e-5 in float32
    (no sigmoid can reorder them) and their order equals the order of the logits;
  * no pair of selected boxes has an IoU within 1e-5 of a threshold in use (float32 IoU rounding is of order 1e-7), and every NMS case
    suppresses at least one pair and keeps at least one box per image.
"""
import ast
import os
import types

import numpy as np
import torch
from torch import nn

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

B, Q, C, NUM_SELECT = 2, 30, 57, 100
MARGIN = 1e-5


def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def box_iou(a, b):
    lt = torch.max(a[:, None, :2], b[None, :, :2])
    rb = torch.min(a[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (box_area(a)[:, None] + box_area(b)[None, :] - inter)


NMS_CALLS = []      # what the reference's forward got back from nms (it returns the indices only with use_opt)


def nms(boxes, scores, iou_threshold):      # torchvision.ops.nms (published definition)
    order = scores.argsort(descending=True, stable=True)
    iou = box_iou(boxes[order], boxes[order])
    n = len(order)
    dead = torch.zeros(n, dtype=torch.bool)
    keep = []
    for i in range(n):
        if dead[i]:
            continue
        keep.append(i)
        dead[i + 1:] |= iou[i, i + 1:] > iou_threshold
    out = order[torch.tensor(keep, dtype=torch.int64)]
    NMS_CALLS.append(out)
    return out


def batched_nms(boxes, scores, idxs, iou_threshold):      # torchvision.ops.batched_nms, its per-class loop (_batched_nms_vanilla)
    keep_mask = torch.zeros_like(scores, dtype=torch.bool)
    for class_id in torch.unique(idxs):
        curr = torch.where(idxs == class_id)[0]
        keep_mask[curr[nms(boxes[curr], scores[curr], iou_threshold)]] = True
    keep = torch.where(keep_mask)[0]
    return keep[scores[keep].sort(descending=True, stable=True)[1]]


def cut(path, names, kind):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, kind) and n.name in names]
    assert len(body) == len(names), (path, names)
    return compile(ast.Module(body=body, type_ignores=[]), path, "exec")


def reference_postprocess():
    ops = {"torch": torch}
    exec(cut(f"{REF}/util/box_ops.py", ["box_cxcywh_to_xyxy"], ast.FunctionDef), ops)
    ns = {"torch": torch, "nn": nn, "box_ops": types.SimpleNamespace(box_cxcywh_to_xyxy=ops["box_cxcywh_to_xyxy"]), "nms": nms,
          "batched_nms": batched_nms}
    exec(cut(f"{REF}/models/richsem/richsem.py", ["PostProcess"], ast.ClassDef), ns)
    return ns["PostProcess"], ops["box_cxcywh_to_xyxy"]


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.linspace(-8, 6, Q * C, dtype=torch.float32)
    logits = torch.stack([base[torch.randperm(Q * C, generator=g)] for _ in range(B)]).view(B, Q, C)
    # clustered cxcywh boxes in [0, 1]: six centres, five boxes around each
    centre = torch.rand(B, 6, 2, generator=g) * 0.5 + 0.25
    extent = torch.rand(B, 6, 2, generator=g) * 0.2 + 0.1
    which = torch.arange(Q) % 6
    c = centre[:, which] + (torch.rand(B, Q, 2, generator=g) - 0.5) * 0.2 * extent[:, which]
    e = extent[:, which] * (1 + (torch.rand(B, Q, 2, generator=g) - 0.5) * 0.4)
    boxes = torch.cat((c, e), -1).float()
    sizes = torch.tensor([[480.0, 640.0], [333.0, 500.0]], dtype=torch.float32)      # (h, w), different per image
    masks = torch.randn(B, Q, 1, 5, 7, generator=g)
    return logits, boxes, sizes, masks


def decidable(logits, boxes, sizes, to_xyxy):
    """the conditions of the module docstring; returns a description of what fails, or None"""
    flat = logits.view(B, -1)
    prob = flat.sigmoid()
    pv, pi = torch.topk(prob, NUM_SELECT + 1, dim=1)
    li = torch.topk(flat, NUM_SELECT + 1, dim=1)[1]
    if not torch.equal(pi, li):
        return "order by probability != order by logit"
    if float((pv[:, :-1] - pv[:, 1:]).min()) < 2e-5:
        return "top probabilities closer than 2e-5"
    q, lab = pi[:, :NUM_SELECT] // C, pi[:, :NUM_SELECT] % C
    scale = torch.stack([sizes[:, 1], sizes[:, 0], sizes[:, 1], sizes[:, 0]], 1)
    for b in range(B):
        bx = (to_xyxy(boxes)[b][q[b]] * scale[b]).float()
        iou = box_iou(bx.double(), bx.double())
        upper = torch.triu(torch.ones(NUM_SELECT, NUM_SELECT, dtype=torch.bool), 1)
        for thr in (0.5, 0.7):
            if float((iou[upper] - thr).abs().min()) < MARGIN:
                return f"an IoU within {MARGIN} of {thr}"
            if not bool((iou[upper] > thr).any()):
                return f"nothing to suppress at {thr}"
        same = upper & (lab[b][:, None] == lab[b][None, :])
        if not bool((iou[same] > 0.7).any()):
            return "nothing to suppress per class at 0.7"
    return None


# name, constructor arguments, forward arguments, with pred_masks
CASES = [
    ("plain", {}, {}, False),
    ("not_to_xyxy", {}, {"not_to_xyxy": True}, False),
    ("test", {}, {"test": True}, False),
    ("nms05", {"nms_iou_threshold": 0.5}, {}, False),
    ("nms07", {"nms_iou_threshold": 0.7}, {}, False),
    ("use_opt", {"use_opt": True}, {}, False),
    ("masks", {}, {}, True),
]


def main():
    PostProcess, to_xyxy = reference_postprocess()
    for seed in range(100, 200):      # the first seed whose draw is decidable
        logits, boxes, sizes, masks = make_inputs(seed)
        why = decidable(logits, boxes, sizes, to_xyxy)
        if why is None:
            break
        print(f"seed {seed}: {why}")
    assert why is None
    out = {"seed": np.int64(seed), "logits": logits.numpy(), "boxes": boxes.numpy(), "sizes": sizes.numpy(), "masks": masks.numpy(),
           "case_names": np.array([c[0] for c in CASES]),
           # per case: num_select, nms_iou_threshold, use_opt, not_to_xyxy, test, with pred_masks
           "case_table": np.array([[NUM_SELECT, kw.get("nms_iou_threshold", -1), kw.get("use_opt", False), fw.get("not_to_xyxy", False),
                                    fw.get("test", False), m] for _, kw, fw, m in CASES], dtype=np.float64)}
    flat = logits.view(B, -1)
    out["query_idx"] = (torch.topk(flat.sigmoid(), NUM_SELECT, dim=1)[1] // C).numpy()      # richsem.py:1333-1335 (not part of the return value)
    for name, kw, fw, with_masks in CASES:
        del NMS_CALLS[:]
        outputs = {"pred_logits": logits.clone(), "pred_boxes": boxes.clone()}
        if with_masks:
            outputs["pred_masks"] = masks.clone()
        results = PostProcess(num_select=NUM_SELECT, **kw)(outputs, sizes.clone(), **fw)
        assert len(results) == B
        for b, r in enumerate(results):
            for key in ("scores", "labels", "boxes"):
                out[f"{name}.{key}.{b}"] = r[key].numpy()
            assert r["scores"].dtype == torch.float32 and r["boxes"].dtype == torch.float32 and r["labels"].dtype == torch.int64
        if kw.get("use_opt"):
            items = outputs["item_indices"]
        elif kw.get("nms_iou_threshold", -1) > 0:
            items = list(NMS_CALLS)
        else:
            items = None
        if items is not None:
            assert len(items) == B
            for b, i in enumerate(items):
                assert 0 < len(i) < NUM_SELECT, (name, b, len(i))      # something suppressed, something kept
                assert torch.equal(results[b]["scores"], torch.topk(flat[b].sigmoid(), NUM_SELECT)[0][i])
                out[f"{name}.item_indices.{b}"] = i.numpy()
        if with_masks:
            out[f"{name}.pred_masks"] = outputs["pred_masks"].numpy()
        print(name, [len(r["scores"]) for r in results])
    path = os.path.join(OUT, "postprocess", "postprocess_reference.npz")      # (a directory of its own: tests/conftest.py takes every .npz directly under tests/golden that
    os.makedirs(os.path.dirname(path), exist_ok=True)                         #  it has no prefix rule for as a fixture of the operator)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
