#!/usr/bin/env python3
"""Time the library path of a Swin block (``SwinTransformerBlock.fused``: csrc/swin_block_mfma.hip through ``swin_layernorm``,
``swin_linear`` and ``swin_mlp``) against the torch bf16 ops it replaces, in ONE process, the forms alternating.

    python tools/swin_block_timing.py [--calls 10] [--blocks 8] [--out FILE.md]

Per shape (B = 1; the four Swin-L stages with C = 192, 384, 768, 1536 on 204 x 336, 108 x 168, 60 x 84 and 36 x 48 tokens, w = 12, and the first
Swin-T stage, C = 96 on 203 x 336 tokens, w = 7; mlp_ratio 4):
  * the second half of a block, ``x + fc2(GELU(fc1(norm2(x))))``: ``swin_mlp`` against the torch modules, forward under ``no_grad`` and
    forward + backward (gradients for x and all six parameters);
  * the whole block, forward + backward, ``fused = True`` against ``fused = False`` (shifted windows; both use the window-attention kernels);
  * its four linear layers alone (qkv, proj, fc1, fc2; bias epilogue): ``linear_kernel`` against ``torch.addmm`` on the same bf16 operands;
  * the peak bytes a forward + backward of one block allocates, both forms (``torch.cuda.max_memory_allocated`` above the level before).

Method (tools/swin_attention_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls between two HIP events on the stream; a cell is the median block and the range over the blocks, in microseconds per
call.  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import swin                                       # noqa: E402
from tools.geometry_timing import block_us                         # noqa: E402

BF = torch.bfloat16
# (name, H, W, C, heads, window)
STAGES = (("Swin-L stage 1", 204, 336, 192, 6, 12), ("Swin-L stage 2", 108, 168, 384, 12, 12), ("Swin-L stage 3", 60, 84, 768, 24, 12),
          ("Swin-L stage 4", 36, 48, 1536, 48, 12), ("Swin-T stage 1", 203, 336, 96, 3, 7))


def pairs(H, W, C, nH, w, dev):
    """-> {row name: (library callable, torch callable)}, and the block for the memory figure"""
    torch.manual_seed(C)
    blk = swin.SwinTransformerBlock(C, nH, window_size=w, shift_size=w // 2, mlp_ratio=4.).to(BF).to(dev)
    blk.H, blk.W = H, W
    L = H * W
    x = torch.randn(1, L, C, device=dev).to(BF).requires_grad_(True)
    dout = torch.randn(1, L, C, device=dev).to(BF)
    params = list(blk.parameters())

    def clear():
        x.grad = None
        for p in params:
            p.grad = None

    def mlp_torch(t):
        return t + blk.mlp(blk.norm2(t))

    def mlp_lib(t):
        return swin.swin_mlp(t, blk.norm2, blk.mlp.fc1, blk.mlp.fc2, caches=(blk._forms["fc1"], blk._forms["fc2"]))

    def fwd(form):
        def run():
            with torch.no_grad():
                return form(x)
        return run

    def fwd_bwd(form):
        def run():
            clear()
            form(x).backward(dout)
        return run

    def block(fused):
        def form(t):
            blk.fused = fused
            return blk(t)
        return form

    rows = {"swin_mlp forward": (fwd(mlp_lib), fwd(mlp_torch)), "swin_mlp forward + backward": (fwd_bwd(mlp_lib), fwd_bwd(mlp_torch)),
            "block forward + backward": (fwd_bwd(block(True)), fwd_bwd(block(False)))}
    xs = {C: x.detach().view(L, C), 4 * C: torch.randn(L, 4 * C, device=dev).to(BF)}
    for name, lin in (("qkv", blk.attn.qkv), ("proj", blk.attn.proj), ("fc1", blk.mlp.fc1), ("fc2", blk.mlp.fc2)):
        w16, b16, b32 = lin.weight.detach(), lin.bias.detach(), lin.bias.detach().float()
        xin = xs[w16.shape[1]]
        rows[f"linear {name} {w16.shape[1]} -> {w16.shape[0]}"] = (
            lambda xin=xin, w16=w16, b32=b32: swin.linear_kernel(xin, w16, b32)[0], lambda xin=xin, w16=w16, b16=b16: torch.addmm(b16, xin, w16.t()))
    return rows, fwd_bwd(block(True)), fwd_bwd(block(False)), clear


def peak_bytes(run, clear):
    clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    clear()
    return peak


def measure(calls, blocks):
    out = []
    dev = torch.device("cuda", 0)
    for name, H, W, C, nH, w in STAGES:
        rows, blk_lib, blk_torch, clear = pairs(H, W, C, nH, w, dev)
        for lib, ref in rows.values():      # untimed rehearsal
            for _ in range(3):
                lib()
                ref()
        torch.cuda.synchronize()
        mem = {"library": peak_bytes(blk_lib, clear), "torch": peak_bytes(blk_torch, clear)}
        t = {k: ([], []) for k in rows}
        for _ in range(blocks):
            for k, (lib, ref) in rows.items():
                t[k][0].append(block_us(lib, calls))
                t[k][1].append(block_us(ref, calls))
        stat = lambda v: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        rec = {"name": f"{name}: {H} x {W} tokens, C = {C}", "peak_bytes_block_forward_backward": mem,
               "rows": {k: {"library": stat(a), "torch": stat(b)} for k, (a, b) in t.items()}}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del rows, blk_lib, blk_torch, clear
        torch.cuda.empty_cache()
    return out


def table_of(recs):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"
    lines = ["| shape | what | library: us per call, median (min .. max over blocks) | torch | library / torch |", "|---|---|---|---|---|"]
    for r in recs:
        for k, v in r["rows"].items():
            lines.append(f"| {r['name']} | {k} | {f(v['library'])} | {f(v['torch'])} | {v['library']['median_us'] / v['torch']['median_us']:.3f} |")
    lines += ["", "| shape | peak bytes of a block's forward + backward: library | torch | library / torch |", "|---|---|---|---|"]
    for r in recs:
        m = r["peak_bytes_block_forward_backward"]
        lines.append(f"| {r['name']} | {m['library'] / 2 ** 20:.1f} MiB | {m['torch'] / 2 ** 20:.1f} MiB | {m['library'] / m['torch']:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin_block_timing: no GPU; nothing is measured on a CPU")
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "",
                      table_of(measure(a.calls, a.blocks))])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
