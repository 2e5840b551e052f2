#!/usr/bin/env python3
"""Time the distillation term: forward + backward of the device form (richsem_amd/distill.py: one row kernel + the scatter) against the
PyTorch composition it replaces (gathers, softmaxes, kl_div / normalise, l1_loss and their autograd chain), in ONE process, alternating.

    python tools/distill_timing.py [--calls 50] [--blocks 9] [--out FILE.md] [--full-step [--step-runs 2]]

Method: every form of every shape runs untimed first (code objects, allocator, workspaces); then ``--blocks`` blocks per form, the two forms
alternating, each block ``--calls`` calls between two HIP events on the stream; a row of the table is the median block and the range over
the blocks, in microseconds per call.  Launches per call are counted by torch.profiler in a pass of its own, after the timing.  The
kernel-only line (``kl_rows`` / ``l1_rows``: no autograd, no scatter) is what the HBM roofline is held against: the kernel reads 2 K C and
writes K C elements.  ``--full-step``: bench_step.run (what bench.py reports as full_step) without and with device_distill, alternating,
each in a fresh model; the default form twice or more gives the run-to-run range the other is compared with.
There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd.distill import DistillKL, DistillL1, kl_rows, l1_rows   # noqa: E402

C, D = 1204, 1024
HBM_BYTES_PER_S = 8e12      # MI355X peak HBM bandwidth


def block_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def launches(fn):
    """device kernels + copies of one call, by torch.profiler; None where the profiler gives nothing"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:      # noqa: BLE001
        return None


def cases(dev):
    """(name, K, elements per row, bytes of the student's element, device fn, torch fn, kernel-only fn)"""
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for K in (24, 200, 10800):
        rows_total = 10800 if K == 10800 else 2 * 1092      # pred_all at 6 x 2 x 900; else the step's (N, 1092, C) logits
        pr = torch.arange(K, device=dev) if K == 10800 else torch.randperm(rows_total, device=dev, generator=g)[:K]
        tj = torch.arange(K, device=dev)
        w = torch.full((K,), 0.5 / K, device=dev)
        for kind, width in (("kl f32", C), ("kl bf16", C), ("l1 f32", D)):
            x32 = torch.randn(rows_total, width, device=dev, generator=g) * (6 if kind != "l1 f32" else 1)
            t = torch.randn(K, width, device=dev, generator=g) * (6 if kind != "l1 f32" else 1)
            x = (x32.bfloat16() if kind == "kl bf16" else x32).requires_grad_(True)

            def dev_fn(x=x, t=t, pr=pr, tj=tj, w=w, kind=kind):
                x.grad = None
                (DistillKL.apply(x, t, pr, tj, w, None, None, False) if kind != "l1 f32" else DistillL1.apply(x, t, pr, tj, w, True)).backward()

            def torch_fn(x=x, t=t, pr=pr, tj=tj, K=K, kind=kind):
                x.grad = None
                if kind == "l1 f32":      # the reference's 'pred' / 'pred_all' branch: normalise both tensors, gather, l1_loss
                    u, v = x / x.norm(dim=-1, keepdim=True), t / t.norm(dim=-1, keepdim=True)
                    loss = 0.5 * F.l1_loss(u[pr], v[tj], reduction="sum") / K
                else:                     # bench_step.Step.loss_part's line (on bf16 logits: after the float32 copy it needs)
                    loss = 0.5 * F.kl_div(F.log_softmax(x.float()[pr], -1), F.softmax(t[tj], -1), reduction="batchmean")
                loss.backward()

            def kernel_fn(x=x, t=t, pr=pr, tj=tj, w=w, kind=kind):
                kl_rows(x, t, pr, tj, w) if kind != "l1 f32" else l1_rows(x, t, pr, tj, w, True)

            out.append((f"{kind} K={K}", K, width, 2 if kind == "kl bf16" else 4, dev_fn, torch_fn, kernel_fn))
    return out


def measure(calls, blocks):
    dev = torch.device("cuda", 0)
    rows = []
    for name, K, width, elem, dev_fn, torch_fn, kernel_fn in cases(dev):
        fns = {"device": dev_fn, "torch": torch_fn, "kernel": kernel_fn}
        for fn in fns.values():      # untimed rehearsal
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                t[k].append(block_us(fn, calls))
        row = {"name": name, "K": K}
        for k in fns:
            row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k])}
        row["launches"] = {k: launches(fns[k]) for k in ("device", "torch")}
        row["kernel_bytes"] = K * width * (elem + 4 + 4)      # student row + teacher row read, gradient row written
        row["roofline_us"] = row["kernel_bytes"] / HBM_BYTES_PER_S * 1e6
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def full_step(runs):
    import bench_step
    dev = torch.device("cuda", 0)
    out = []
    for i in range(2 * runs):
        on = bool(i % 2)
        r = bench_step.run(2, dev, steps=5, warmup=3, **({"device_distill": True} if on else {}))
        rec = {"device_distill": on, "eager_ms": r.get("ms"), "graph_replay_ms": (r.get("graph_replay") or {}).get("ms"),
               "graphed_sections_ms": (r.get("graphed_sections") or {}).get("ms"), "loss": r.get("loss")}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    return out


def table(rows):
    f = lambda d: f"{d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f})"
    lines = ["| form, rows | device: us per forward + backward (range over blocks) | torch composition | device / torch | launches device | launches torch |"
             " kernel only: us | kernel bytes | at 8 TB/s: us | share of HBM peak |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {f(r['device'])} | {f(r['torch'])} | {r['device']['median_us'] / r['torch']['median_us']:.2f} | "
                     f"{r['launches']['device'] or 'not measured'} | {r['launches']['torch'] or 'not measured'} | {f(r['kernel'])} | {r['kernel_bytes']} | "
                     f"{r['roofline_us']:.2f} | {r['roofline_us'] / r['kernel']['median_us']:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--full-step", action="store_true")
    ap.add_argument("--step-runs", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_timing: no GPU; nothing is measured on a CPU")
    text = [f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "", table(measure(a.calls, a.blocks))]
    if a.full_step:
        text += ["", "full_step (bench_step.run, steps=5, warmup=3), alternating:", "", "```"] + [json.dumps(r) for r in full_step(a.step_runs)] + ["```"]
    text = "\n".join(text)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
