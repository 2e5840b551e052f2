#!/usr/bin/env python3
"""Time the denoising queries: the device form (richsem_amd/dn.py ``denoising_queries``: ONE launch from the target counts on the device,
into static buffers) against the torch composition it replaces -- the denoising lines of ``bench_step.Step`` (two repeats, four random
draws, a dozen element-wise ops, the embedding lookup, two index scatters) plus the mask call on the host's layout --, in ONE process,
alternating.  Forward, and forward + backward (the gradient of the label table from a fixed gradient of the query block).

    python tools/dn_timing.py [--calls 20] [--blocks 16] [--out FILE.md]

Shapes: N = 2 images, 12 boxes each, D = 256, 900 queries, 1204 classes, dn_number 100 (8 groups, pad_size 192).  Method (that of
tools/geometry_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block ``--calls``
calls between two HIP events on the stream; a row is the median block and the range over the blocks, in microseconds per call.  Both forms
draw fresh random numbers in every call (the device form one ``torch.rand`` of (N, pad, 10)).  Launches per call are counted by
torch.profiler in a pass of its own, after the timing.  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_step                                                          # noqa: E402
from geometry_timing import block_us, launches                             # noqa: E402
from richsem_amd.dn import denoising_queries, dn_buffers, prepare_dn_layout      # noqa: E402

N, BOXES, D, NQ, NCLS, DN = 2, 12, 256, 900, 1204, 100


def torch_composition(labels, boxes, counts, table, dev):
    """the denoising lines of bench_step.Step._torch_dn_queries as they are there, plus the layout / mask call they lean on"""
    lay = prepare_dn_layout(counts, DN, NQ, use_cdn=True)
    pad, groups = lay["pad_size"], lay["num_dn_group"]
    known_labels, known_boxes = labels.repeat(2 * groups), boxes.repeat(2 * groups, 1)
    p = torch.rand(known_labels.shape, device=dev)
    rnd_lab = torch.randint(0, NCLS, known_labels.shape, device=dev)
    noised = torch.where(p < 0.25, rnd_lab, known_labels)
    xyxy = bench_step.box_cxcywh_to_xyxy(known_boxes)
    diff = torch.cat((known_boxes[:, 2:] / 2, known_boxes[:, 2:] / 2), 1)
    sign = torch.randint(0, 2, xyxy.shape, device=dev).float() * 2 - 1
    rand_part = torch.rand(xyxy.shape, device=dev)
    neg = (torch.arange(known_labels.numel(), device=dev) // labels.numel()) % 2 == 1
    rand_part = torch.where(neg[:, None], rand_part + 1.0, rand_part) * sign
    xyxy = (xyxy + rand_part * diff).clamp(0.0, 1.0)
    nb = torch.cat(((xyxy[:, :2] + xyxy[:, 2:]) / 2, xyxy[:, 2:] - xyxy[:, :2]), 1)
    q_label = torch.zeros(len(counts), pad, D, device=dev)
    q_bbox = torch.zeros(len(counts), pad, 4, device=dev)
    q_label[lay["known_bid"], lay["map_known_indice"]] = torch.nn.functional.embedding(noised, table)
    q_bbox[lay["known_bid"], lay["map_known_indice"]] = bench_step.inverse_sigmoid(nb)
    return q_label, q_bbox, lay["attn_mask"]


def forms(dev):
    g = torch.Generator().manual_seed(0)
    counts = [BOXES] * N
    boxes = torch.cat((torch.rand(N * BOXES, 2, generator=g) * 0.6 + 0.2, torch.rand(N * BOXES, 2, generator=g) * 0.35 + 0.05), 1).to(dev)
    labels = torch.randint(1, NCLS, (N * BOXES,), generator=g).to(dev)
    table = torch.randn(NCLS + 1, D, generator=g).to(dev).requires_grad_(True)
    cum = torch.tensor([0] + [BOXES * (i + 1) for i in range(N)], dtype=torch.int64, device=dev)
    pad = prepare_dn_layout(counts, DN, NQ)["pad_size"]
    out = dn_buffers(N, pad, NQ, D, dev)
    grad = torch.randn(N, pad, D, device=dev)
    kw = dict(pad_cap=pad, num_queries=NQ, num_classes=NCLS, dn_number=DN, label_noise_ratio=0.5, box_noise_scale=1.0, out=out)

    def device():
        return denoising_queries(cum, labels, boxes, table, torch.rand((N, pad, 10), device=dev), **kw)

    def torch_():
        return torch_composition(labels, boxes, counts, table, dev)

    def with_backward(fn):
        def run():
            table.grad = None
            fn()[0].backward(grad)
        return run
    return pad, {"device fwd": device, "torch fwd": torch_, "device fwd+bwd": with_backward(device), "torch fwd+bwd": with_backward(torch_)}


def measure(calls, blocks):
    pad, fns = forms(torch.device("cuda", 0))
    for fn in fns.values():      # untimed rehearsal
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            t[k].append(block_us(fn, calls))
    row = {"pad_size": pad}
    for k in fns:
        row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k]), "launches": launches(fns[k])}
    print(json.dumps(row), flush=True)
    return row


def table(row):
    lines = ["| form | us per call, median (min .. max over blocks) | launches per call |", "|---|---|---|"]
    for k, d in row.items():
        if isinstance(d, dict):
            lines.append(f"| {k} | {d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f}) | {d['launches'] or 'not measured'} |")
    for kind in ("fwd", "fwd+bwd"):
        lines.append(f"\ndevice / torch, {kind}: {row['device ' + kind]['median_us'] / row['torch ' + kind]['median_us']:.3f}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dn_timing: no GPU; nothing is measured on a CPU")
    row = measure(a.calls, a.blocks)
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; N = {N}, {BOXES} boxes per image, D = {D}, {NQ} queries, pad_size {row['pad_size']}; "
                      f"{a.blocks} blocks of {a.calls} calls per form, alternating", "", table(row)])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
