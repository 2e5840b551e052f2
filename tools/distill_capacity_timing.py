#!/usr/bin/env python3
"""Time the distillation term and the teacher's box targets in their exact-size and capacity forms, in ONE process, alternating:

  * ``term``      forward + backward of the KL distillation over the distilled layers: ``exact`` = ``DistillLoss.stacked`` on index tensors of
                  the batch's exact size (built beforehand), backward by ``index_add_`` (the composition a step runs today); ``capacity`` =
                  ``richsem_amd.distill.device_distill`` with targets capacity 600 and pad_cap 600 (pairs on the device, scatter backward);
  * ``teacher``   ``clip_box_targets`` (one ROI per target box) against ``clip_box_targets_capacity`` (600 slots), on a 2048 x 25 x 42 map;
  * ``roi``       the ROI kernel alone: ``msda_roi_align_forward_f32`` at 24 ROIs against ``msda_roi_align_targets_f32`` at 24 live of 600 slots;
  * ``pool``      the attention pool at the live row count against 600 rows;
  * ``scatter``   the backward alone on the capacity-sized rows: zero-fill + ``index_add_`` with the dead rows clamped to row 0 (what
                  ``_RowLoss.backward`` would do with these slots) against ``msda_distill_scatter_f32``.

    python tools/distill_capacity_timing.py [--calls 10] [--blocks 12] [--out FILE.md]

Shape: nl = 6 decoder outputs of which layers 4 and 5 are distilled, N = 2 images, 900 + pad queries, C = 1203 classes, dn_number 100; 12 and
100 boxes per image.  Method (that of tools/geometry_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms
alternating, each block ``--calls`` calls between two HIP events on the stream; a row is the median block and the range over the blocks, in
microseconds per call.  Launches per call are counted by torch.profiler in a pass of its own, after the timing.
There is no CPU path: without a GPU this fails."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometry_timing import block_us, launches                             # noqa: E402
from richsem_amd.distill import DistillLoss, device_distill, distill_capacity_backward, distill_capacity_forward, _capacity_checked      # noqa: E402
from richsem_amd.dn import dn_capacity, dn_group_count                     # noqa: E402
from richsem_amd.matcher import TargetBuffers                              # noqa: E402
from richsem_amd.modules.attnpool import AttentionPool2d, clip_box_targets, clip_box_targets_capacity      # noqa: E402
from richsem_amd.roi import roi_align, roi_align_targets                   # noqa: E402

NL, LAYERS, N, Q, C, DN = 6, (4, 5), 2, 900, 1203, 100
CAPACITY, PAD_CAP = 600, dn_capacity(DN, 300)
MAP, EMBED, HEADS, OUT_DIM, IMAGE = (2048, 25, 42), 2048, 32, 1024, (800, 1344)


def forms(K, dev):
    gen = torch.Generator().manual_seed(K)
    counts, total, n_d = [K] * N, K * N, len(LAYERS)
    groups = dn_group_count(DN, counts)
    pad = 2 * K * groups
    boxes = torch.cat((torch.rand(total, 2, generator=gen) * 0.6 + 0.2, torch.rand(total, 2, generator=gen) * 0.3 + 0.05), 1)
    targets = [{"labels": torch.randint(0, C, (K,), generator=gen).to(dev), "boxes": boxes[b * K: (b + 1) * K].to(dev),
                "size": torch.tensor(IMAGE, device=dev)} for b in range(N)]
    qot = torch.stack([torch.cat([torch.randperm(Q, generator=gen)[:K] for _ in range(N)]) for _ in range(NL + 1)]).to(dev)
    meta = torch.tensor([K, groups, pad, total, 0], dtype=torch.int64, device=dev)
    bufs = TargetBuffers(N, CAPACITY, dev).update_(targets)
    q_cap = torch.full((NL + 1, CAPACITY), -1, dtype=torch.int64, device=dev)
    q_cap[:, :total] = qot
    fns = {}

    # ---- the term: exact-size composition against the capacity form ---------------------------------------------------------------------------
    x_exact = (torch.randn(n_d, N, pad + Q, C, generator=gen) * 4).to(dev).requires_grad_(True)
    x_cap = (torch.randn(n_d, N, PAD_CAP + Q, C, generator=gen) * 4).to(dev).requires_grad_(True)
    teacher_exact = (torch.randn(total, C, generator=gen) * 4).to(dev)
    teacher_cap = torch.zeros(CAPACITY, C, device=dev)
    teacher_cap[:total] = teacher_exact
    img = torch.arange(N, device=dev).repeat_interleave(K)
    tj = torch.arange(total, device=dev)
    pos = (torch.arange(groups, device=dev)[:, None] * 2 * K + torch.arange(K, device=dev)[None]).flatten()      # one image's positive slots
    pr, tr, w = [], [], []
    for i, l in enumerate(LAYERS):
        pr.append((i * N + img) * (pad + Q) + pad + qot[l])
        tr.append(tj)
        w.append(torch.full((total,), 1.0 / total, device=dev))
    for i in range(n_d):
        for b in range(N):
            pr.append((i * N + b) * (pad + Q) + pos)
            tr.append(b * K + (pos % (2 * K)))
            w.append(torch.full((pos.numel(),), 1.0 / (total * groups), device=dev))
    pr, tr, w = torch.cat(pr), torch.cat(tr), torch.cat(w)
    crit = DistillLoss("clip_logits", "gt", dynamic_weight=True)

    def term_exact():
        x_exact.grad = None
        loss = crit.stacked(x_exact, teacher_exact, pr, tr, w)
        loss.backward()
        return loss

    def term_capacity():
        x_cap.grad = None
        loss, _ = device_distill(x_cap, teacher_cap, bufs, q_cap, meta, pad_cap=PAD_CAP, layers=LAYERS, distill_type="clip_logits", objective="gt",
                                 dynamic_weight=True)
        loss.backward()
        return loss
    fns["term exact"], fns["term capacity"] = term_exact, term_capacity

    # ---- the backward alone, on the capacity-sized rows ------------------------------------------------------------------------------------------
    cfg = _capacity_checked(x_cap, teacher_cap, bufs, q_cap, meta, PAD_CAP, LAYERS, "clip_logits", "gt", None, None)
    with torch.no_grad():
        _, _, saved = distill_capacity_forward(x_cap, teacher_cap, bufs, q_cap, meta, None, None, True, cfg)
    grad_rows, pred_row = saved[0], saved[1]
    rows = n_d * N * (PAD_CAP + Q)
    g = torch.ones(1, device=dev)

    def scatter_index_add():
        gp = grad_rows.new_zeros((rows, C))
        gp.index_add_(0, pred_row.clamp(0, rows - 1), grad_rows * g)
        return gp

    def scatter_kernel():
        return distill_capacity_backward(saved, g)
    fns["scatter index_add_"], fns["scatter kernel"] = scatter_index_add, scatter_kernel

    # ---- the teacher's box targets -------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    pool = AttentionPool2d(7, EMBED, HEADS, OUT_DIM).to(dev)
    feats = torch.randn(N, *MAP, generator=gen).to(dev)
    text = torch.randn(C, OUT_DIM, generator=gen).to(dev)
    scale = torch.tensor(math.log(100.0), device=dev)
    sizes = torch.tensor([IMAGE] * N, dtype=torch.int32, device=dev)
    fns["teacher exact"] = lambda: clip_box_targets(feats, targets, pool, text, scale)[1][0]
    fns["teacher capacity"] = lambda: clip_box_targets_capacity(feats, bufs, sizes, pool, text, scale)[1]
    # ---- its two parts alone ---------------------------------------------------------------------------------------------------------------------
    cx, cy, bw, bh = boxes.to(dev).unbind(-1)
    whwh = torch.tensor([IMAGE[1], IMAGE[0]] * 2, dtype=torch.float32, device=dev)
    rois = torch.cat((img[:, None].float(), whwh * torch.stack([cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh], -1)), -1)
    fns["roi exact"] = lambda: roi_align(feats, rois, 7, 1.0 / 32, 0, True)
    fns["roi capacity"] = lambda: roi_align_targets(feats, bufs, sizes, 7, 1.0 / 32, 0)
    roi_live, roi_cap = fns["roi exact"](), fns["roi capacity"]()
    fns["pool live rows"] = lambda: pool(roi_live)
    fns["pool 600 rows"] = lambda: pool(roi_cap)
    return pad, groups, fns


def measure(K, calls, blocks):
    pad, groups, fns = forms(K, torch.device("cuda", 0))
    for fn in fns.values():      # untimed rehearsal
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            t[k].append(block_us(fn, calls))
    row = {"boxes_per_image": K, "pad_size": pad, "groups": groups}
    for k in fns:
        row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k]), "launches": launches(fns[k])}
    print(json.dumps(row), flush=True)
    return row


def table(row):
    lines = [f"### {row['boxes_per_image']} boxes per image ({2 * row['boxes_per_image']} live targets, pad_size {row['pad_size']}, {row['groups']} groups)", "",
             "| form | us per call, median (min .. max over blocks) | launches per call |", "|---|---|---|"]
    for k, d in row.items():
        if isinstance(d, dict):
            lines.append(f"| {k} | {d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f}) | {d['launches'] or 'not measured'} |")
    lines.append("")
    for a, b in (("term capacity", "term exact"), ("scatter kernel", "scatter index_add_"), ("teacher capacity", "teacher exact"),
                 ("roi capacity", "roi exact"), ("pool 600 rows", "pool live rows")):
        lines.append(f"{a} / {b}: {row[a]['median_us'] / row[b]['median_us']:.3f}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_capacity_timing: no GPU; nothing is measured on a CPU")
    rows = [measure(K, a.calls, a.blocks) for K in (12, 100)]
    text = "\n\n".join([f"device: {torch.cuda.get_device_name(0)}; nl = {NL}, distilled layers {LAYERS}, N = {N}, {Q} + pad queries, C = {C}; map "
                        f"{MAP[0]} x {MAP[1]} x {MAP[2]}; capacity form: {CAPACITY} targets, pad_cap {PAD_CAP}; {a.blocks} blocks of {a.calls} calls "
                        "per form, alternating; term = forward + backward"] + [table(r) for r in rows])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
