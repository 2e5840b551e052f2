#!/usr/bin/env python3
"""Time the class head: the library form (richsem_amd/class_head.py: three MFMA kernels on the collapsed operands) against the torch
composition it replaces -- ``bench_step.Step.class_logits`` as it stands (F.linear, norm, division, the product against the text,
``.float()``, autograd's backward) --, in ONE process, the forms alternating.

    python tools/class_head_timing.py [--calls 20] [--blocks 12] [--out FILE.md]

Method: every form runs untimed first (code objects, allocator, hipBLASLt's choice); then ``--blocks`` blocks per form, the forms
alternating, each block ``--calls`` calls between two HIP events on the stream; a row of the table is the median block and the range over
the blocks, in microseconds per call.  Launches per call are counted by torch.profiler in a pass of its own, after the timing.  Shapes: the
benchmark step's two call sites -- the stacked decoder outputs (6, 2, 1092, 256) bf16 = 13 104 rows, and the two-stage rows (2, 900, 256)
fp32 = 1 800 rows --, 1204 classes, projection 256 -> 1024.  ``forward`` is timed under ``torch.no_grad``; ``forward + backward`` with a
fixed dense g, gradients for the rows and the projection.  The forward's bytes (logits written, x read) are held against the HBM peak.
There is no CPU path: without a GPU this fails."""
import argparse
import functools
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_step                                                  # noqa: E402
from richsem_amd.class_head import ClassHead                       # noqa: E402
from tools.geometry_timing import HBM_BYTES_PER_S, block_us, launches      # noqa: E402

CLASSES, PROJ = bench_step.NUM_CLASSES, bench_step.PROJ
SHAPES = {"decoder outputs (6, 2, 1092, 256) bf16": ((6, 2, 1092, 256), torch.bfloat16), "two-stage rows (2, 900, 256) fp32": ((2, 900, 256), torch.float32)}


def torch_head(weight, text_embed, logit_scale):
    """``bench_step.Step.class_logits`` / ``Step.text_logits`` THEMSELVES, bound to a stand-in that holds what they read"""
    me = SimpleNamespace(dino_visual_proj=SimpleNamespace(weight=weight), text_embed=text_embed, logit_scale=logit_scale)
    me.text_logits = functools.partial(bench_step.Step.text_logits, me)
    return functools.partial(bench_step.Step.class_logits, me)


def head_cases(dev):
    gen = torch.Generator().manual_seed(0)
    weight = (torch.randn(PROJ, 256, generator=gen) / 16).to(dev).requires_grad_(True)
    text, ls = torch.randn(CLASSES, PROJ, generator=gen).to(dev), torch.tensor(2.6593, device=dev)
    forms = {"library": ClassHead(2).prepare(weight, text, ls), "torch": torch_head(weight, text, ls)}
    out = []
    for name, (shape, dtype) in SHAPES.items():
        x = torch.randn(*shape, generator=gen).to(dtype).to(dev).requires_grad_(True)
        g = torch.randn(*shape[:-1], CLASSES, generator=gen).to(dev)
        fns = {}
        for k, head in forms.items():
            def fwd(head=head, x=x):
                with torch.no_grad():
                    return head(x)

            def fwd_bwd(head=head, x=x, g=g):
                x.grad = weight.grad = None
                head(x).backward(g)
            fns[k + " forward"], fns[k + " forward + backward"] = fwd, fwd_bwd
        a, b = fns["library forward"](), fns["torch forward"]()
        torch.cuda.synchronize()
        out.append((name, x.numel() // 256, x.element_size(), fns, float((a - b).abs().max())))
    return out


def measure_heads(calls, blocks):
    rows = []
    for name, R, xbytes, fns, diff in head_cases(torch.device("cuda", 0)):
        for fn in fns.values():      # untimed rehearsal
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                t[k].append(block_us(fn, calls))
        row = {"name": name, "rows": R, "max_abs_logit_difference_between_the_forms": diff}
        for k in fns:
            row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k])}
        row["launches"] = {k: launches(fns[k]) for k in fns}
        row["forward_bytes"] = R * CLASSES * 4 + R * 256 * xbytes
        row["roofline_us"] = row["forward_bytes"] / HBM_BYTES_PER_S * 1e6
        row["forward_bytes_per_s"] = row["forward_bytes"] / (row["library forward"]["median_us"] * 1e-6)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def head_table(rows):
    f = lambda d: f"{d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f})"
    lines = ["| call site | rows | pass | library: us per call, median (min .. max over blocks) | torch composition | library / torch | "
             "launches library | launches torch |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for what in ("forward", "forward + backward"):
            a, b = r["library " + what], r["torch " + what]
            lines.append(f"| {r['name']} | {r['rows']} | {what} | {f(a)} | {f(b)} | {a['median_us'] / b['median_us']:.3f} | "
                         f"{r['launches']['library ' + what] or 'not measured'} | {r['launches']['torch ' + what] or 'not measured'} |")
    lines += ["", "| call site | forward bytes (logits written + x read) | at 8 TB/s: us | library forward: us | achieved bytes/s | share of HBM peak |",
              "|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['forward_bytes']} | {r['roofline_us']:.2f} | {r['library forward']['median_us']:.1f} | "
                     f"{r['forward_bytes_per_s']:.3g} | {r['forward_bytes_per_s'] / HBM_BYTES_PER_S:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("class_head_timing: no GPU; nothing is measured on a CPU")
    parts = [f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "",
             head_table(measure_heads(a.calls, a.blocks))]
    text = "\n".join(parts)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
