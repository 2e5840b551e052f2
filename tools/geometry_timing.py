#!/usr/bin/env python3
"""Time the batch-geometry tensors: the device form (richsem_amd/geometry.py: ONE kernel from the image sizes, into static buffers) against the
torch composition it replaces -- ``Step.prepare``'s geometry lines (F.interpolate per level, valid ratios, get_reference_points,
sine_position per level, encoder_output_proposals) on the GPU, from the image mask --, in ONE process, alternating.

    python tools/geometry_timing.py [--calls 20] [--blocks 16] [--out FILE.md]

Method: both forms of both canvases run untimed first (code objects, allocator); then ``--blocks`` blocks per form, the forms alternating, each
block ``--calls`` calls between two HIP events on the stream; a row of the table is the median block and the range over the blocks, in
microseconds per call.  Launches per call are counted by torch.profiler in a pass of its own, after the timing.  ``pos only`` is the kernel
with ``want=("pos_sine",)``: pos_sine is the only output with real bytes (N S 256 float32 written, nothing read), so that line is what the
HBM peak is held against.  Canvases: E (800 x 1344) and Em (1280 x 1280), N = 2, full-size images.
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
import bench_step                                                  # noqa: E402
from richsem_amd import workload as W                              # noqa: E402
from richsem_amd.geometry import batch_geometry                    # noqa: E402
from richsem_amd.modules import get_reference_points               # noqa: E402

HBM_BYTES_PER_S = 8e12      # MI355X peak HBM bandwidth
CANVASES = {"E 800x1344": ((800, 1344), [(800, 1333), (800, 1333)]), "Em 1280x1280": ((1280, 1280), [(1280, 1280), (1280, 1280)])}


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


def torch_composition(mask, shapes):
    """the geometry lines of bench_step.Step.prepare, as they are there"""
    dev = mask.device
    masks = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in shapes]
    st = {"masks": masks, "mask_flat": torch.cat([m.flatten(1) for m in masks], 1),
          "valid_ratios": torch.stack([torch.stack([(~m[:, 0, :]).sum(1) / m.shape[2], (~m[:, :, 0]).sum(1) / m.shape[1]], -1)
                                       for m in masks], 1).float()}
    st["ref"] = get_reference_points(shapes, st["valid_ratios"], dev)
    st["pos_sine"] = torch.cat([bench_step.sine_position(m) for m in masks], 1)
    st["proposals"], st["zeroed"] = bench_step.encoder_output_proposals(st["mask_flat"], shapes)
    return st


def cases(dev):
    out = []
    for name, (canvas, sizes) in CANVASES.items():
        shapes = list(W.pyramid_shapes(*canvas))
        mask = torch.ones((len(sizes),) + canvas, dtype=torch.bool, device=dev)
        for n, (h, w) in enumerate(sizes):
            mask[n, :h, :w] = False
        sz = torch.tensor(sizes, dtype=torch.int32).to(dev)
        full, pos = batch_geometry(sz, canvas, shapes), batch_geometry(sz, canvas, shapes, want=("pos_sine",))
        want = torch_composition(mask, shapes)
        torch.cuda.synchronize()
        err = float((full["pos_sine"] - want["pos_sine"]).abs().max())      # (the timed forms compute the same thing: tests/test_gpu_geometry.py)
        assert torch.equal(full["mask_flat"], want["mask_flat"]) and err <= 4e-6, err
        del want
        fns = {"device": lambda sz=sz, canvas=canvas, shapes=shapes, full=full: batch_geometry(sz, canvas, shapes, out=full),
               "torch": lambda mask=mask, shapes=shapes: torch_composition(mask, shapes),
               "pos only": lambda sz=sz, canvas=canvas, shapes=shapes, pos=pos: batch_geometry(sz, canvas, shapes, want=("pos_sine",), out=pos)}
        out.append((name, len(sizes), sum(h * w for h, w in shapes), fns, err))
    return out


def measure(calls, blocks):
    rows = []
    for name, N, S, fns, err in cases(torch.device("cuda", 0)):
        for fn in fns.values():      # untimed rehearsal
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                t[k].append(block_us(fn, calls))
        row = {"name": name, "N": N, "S": S, "pos_sine_max_abs_err": err}
        for k in fns:
            row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k])}
        row["launches"] = {k: launches(fns[k]) for k in ("device", "torch")}
        row["pos_bytes"] = N * S * 256 * 4
        row["roofline_us"] = row["pos_bytes"] / HBM_BYTES_PER_S * 1e6
        row["pos_bytes_per_s"] = row["pos_bytes"] / (row["pos only"]["median_us"] * 1e-6)
        rows.append(row)
        print(json.dumps(row), flush=True)
        torch.cuda.empty_cache()
    return rows


def table(rows):
    f = lambda d: f"{d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f})"
    lines = ["| canvas, N = 2 | S | device: us per call, median (min .. max over blocks) | torch composition | device / torch | launches device | "
             "launches torch | pos_sine only: us | pos_sine bytes | at 8 TB/s: us | achieved bytes/s | share of HBM peak |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['name']} | {r['S']} | {f(r['device'])} | {f(r['torch'])} | {r['device']['median_us'] / r['torch']['median_us']:.3f} | "
                     f"{r['launches']['device'] or 'not measured'} | {r['launches']['torch'] or 'not measured'} | {f(r['pos only'])} | {r['pos_bytes']} | "
                     f"{r['roofline_us']:.2f} | {r['pos_bytes_per_s']:.3g} | {r['pos_bytes_per_s'] / HBM_BYTES_PER_S:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometry_timing: no GPU; nothing is measured on a CPU")
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "",
                      table(measure(a.calls, a.blocks))])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
