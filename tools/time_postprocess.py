#!/usr/bin/env python3
"""A/B timing of the on-device PostProcess selection (richsem_amd/postprocess.py: ``select``) against the torch composition of the
reference's ``PostProcess`` body on the same device in the same process, at the LVIS size (B = 2, Q = 900, C = 1203, k = 300), for
float32 and bfloat16 logits; and the time of the NMS at K = 300, which has no on-device comparator here (torchvision is absent).

    python tools/time_postprocess.py [--blocks 16] [--calls 25] [--out profiles/r09_postprocess_timing.md]

Method: an untimed rehearsal of both sides; then ``blocks`` blocks of ``calls`` calls per side, the two sides alternated block by block,
HIP events around each block (not around single calls: an event pair costs about as much as one of these calls); per side the median, the
smallest and the largest per-call time over its blocks.  The result of the two sides is compared on the timed input first.  Needs a GPU.

The calls are issued from Python inside the event pair, so a block's time is the larger of the host's issue time and the GPU's execution
time, and both sides are a dozen short launches per call.  Which of the two it is shows in a kernel trace of a short run, taken on its own
(``rocprofv3 --kernel-trace --stats -- python tools/time_postprocess.py --blocks 2 --calls 10``): the sum of a side's kernel durations per
call is its GPU time.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from richsem_amd.postprocess import nms_padded, select      # noqa: E402


def torch_composition(logits, boxes, sizes, k):
    """the reference's PostProcess.forward without NMS (richsem.py:1332-1354)"""
    prob = logits.sigmoid()
    scores, idx = torch.topk(prob.view(logits.shape[0], -1), k, dim=1)
    q = idx // logits.shape[2]
    labels = idx % logits.shape[2]
    x_c, y_c, w, h = boxes.unbind(-1)
    xyxy = torch.stack([(x_c - 0.5 * w), (y_c - 0.5 * h), (x_c + 0.5 * w), (y_c + 0.5 * h)], dim=-1)
    bx = torch.gather(xyxy, 1, q.unsqueeze(-1).repeat(1, 1, 4))
    img_h, img_w = sizes.unbind(1)
    return scores, labels, bx * torch.stack([img_w, img_h, img_w, img_h], dim=1)[:, None, :], q


def time_blocks(sides, blocks, calls):
    """sides: {name: callable}; returns {name: [per-call microseconds of each block]}"""
    out = {name: [] for name in sides}
    for _ in range(blocks):
        for name, fn in sides.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            stop.record()
            stop.synchronize()
            out[name].append(start.elapsed_time(stop) * 1000.0 / calls)
    return out


def row(name, t):
    return f"| {name} | {statistics.median(t):.1f} | {min(t):.1f} | {max(t):.1f} | {len(t)} |"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_postprocess.py needs a GPU: a CPU run says nothing about these times")
    dev = torch.device("cuda", 0)
    B, Q, C, k = 2, 900, 1203, 300
    g = torch.Generator().manual_seed(0)
    base = torch.linspace(-12, 2, Q * C)
    logits32 = torch.stack([base[torch.randperm(Q * C, generator=g)] for _ in range(B)]).view(B, Q, C).to(dev)
    boxes = torch.cat((torch.rand(B, Q, 2, generator=g) * 0.6 + 0.2, torch.rand(B, Q, 2, generator=g) * 0.3 + 0.02), -1).to(dev)
    sizes = torch.tensor([[480.0, 640.0], [333.0, 500.0]], device=dev)
    lines = [f"PostProcess selection, B = {B}, Q = {Q}, C = {C}, k = {k}; {a.blocks} blocks x {a.calls} calls per side, sides alternated; "
             f"microseconds per call ({torch.cuda.get_device_name(0)})", "",
             "| side | median | min | max | blocks |", "|---|---|---|---|---|"]
    for tag, logits in (("f32", logits32), ("bf16", logits32.to(torch.bfloat16))):
        sides = {f"device path, {tag} logits": lambda lg=logits: select(lg, boxes, sizes, k),
                 f"torch composition, {tag} logits": lambda lg=logits: torch_composition(lg, boxes, sizes, k)}
        got, want = [fn() for fn in sides.values()]
        torch.cuda.synchronize()
        if tag == "f32":      # pairwise different probabilities: the two sides must agree exactly on the indices and the boxes
            assert torch.equal(got[1], want[1]) and torch.equal(got[3], want[3]) and torch.equal(got[2], want[2])
            assert float((got[0] - want[0]).abs().max()) <= 1e-6
        time_blocks(sides, 2, a.calls)      # rehearsal, untimed
        t = time_blocks(sides, a.blocks, a.calls)
        names = list(t)
        lines += [row(n, t[n]) for n in names]
        ratio = statistics.median(t[names[0]]) / statistics.median(t[names[1]])
        lines.append(f"| ratio device / torch, {tag} | {ratio:.3f} | | | |")
    # NMS at K = 300 on the boxes of the selection: no comparator on this stack
    s, l, bx, q = select(logits32, boxes, sizes, k)
    for name, lab, thr in (("nms, class-agnostic, 0.5", None, 0.5), ("batched nms (per label), 0.7", l, 0.7)):
        sides = {f"{name}, K = {k} (no comparator)": lambda lab=lab, thr=thr: nms_padded(bx, lab, thr)}
        time_blocks(sides, 2, a.calls)
        lines += [row(n, v) for n, v in time_blocks(sides, a.blocks, a.calls).items()]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
