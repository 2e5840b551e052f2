#!/usr/bin/env python3
"""Time the library path of the Swin stage boundaries (``SwinTransformer.set_fused_stages``: csrc/swin_stage.hip through ``swin_patch_rows``,
``swin_merge_norm`` and ``swin_norm_nchw``) against the torch bf16 ops it replaces, in ONE process, the forms alternating.

    python tools/swin_stage_timing.py [--calls 10] [--blocks 8] [--net-calls 3] [--out FILE.md]

Rows (B = 1, an 800 x 1344 image):
  * patch embedding, image -> the contiguous tokens the first block reads: ``PatchEmbed.tokens`` with ``fused`` against the convolution,
    flatten / transpose, LayerNorm and ``.contiguous()``; Swin-L (C = 192) and Swin-T (C = 96), 200 x 336 tokens;
  * merging norm, tokens -> normalised 4 C rows: ``swin_merge_norm`` against pad, the six-dimensional permute copy and ``F.layer_norm``; and
    the whole ``PatchMerging`` (with the reduction), ``fused`` against not; Swin-L C = 192, 384, 768 on 200 x 336, 100 x 168, 50 x 84 and Swin-T
    stage 1 (C = 96);
  * output norm, tokens -> (B, C, H, W): ``swin_norm_nchw`` against ``F.layer_norm`` and ``permute(0, 3, 1, 2).contiguous()``; Swin-L
    C = 192 ... 1536 on 200 x 336 ... 25 x 42 and Swin-T stage 1;
  each forward under ``no_grad`` and forward + backward (gradients for the input and the parameters), with the peak bytes a forward +
  backward allocates (``torch.cuda.max_memory_allocated`` above the level before);
  * the whole Swin-L and Swin-T ``forward_raw`` + backward with the blocks fused, stages fused against not.

Method (tools/swin_block_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls (``--net-calls`` for the whole backbones) between two HIP events on the stream; a cell is the median block and the range
over the blocks, in microseconds per call.  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import swin                                       # noqa: E402
from tools.geometry_timing import block_us                         # noqa: E402
from tools.swin_block_timing import peak_bytes                     # noqa: E402

BF = torch.bfloat16
IMAGE = (800, 1344)
# (name, H, W, C) of the token maps
MERGES = (("Swin-L merge 1", 200, 336, 192), ("Swin-L merge 2", 100, 168, 384), ("Swin-L merge 3", 50, 84, 768), ("Swin-T merge 1", 200, 336, 96))
NORMS = (("Swin-L norm 0", 200, 336, 192), ("Swin-L norm 1", 100, 168, 384), ("Swin-L norm 2", 50, 84, 768), ("Swin-L norm 3", 25, 42, 1536),
         ("Swin-T norm 0", 200, 336, 96))
EMBEDS = (("Swin-L embed", 192), ("Swin-T embed", 96))
NETS = (("Swin-L", dict(embed_dim=192, depths=(2, 2, 18, 2), num_heads=(6, 12, 24, 48), window_size=12, drop_path_rate=0.)),
        ("Swin-T", dict(embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24), window_size=7, drop_path_rate=0.)))


def _forms(form_lib, form_torch, x, dout, params):
    """-> {"forward": (lib, torch), "forward + backward": (lib, torch)} and a clear()"""
    def clear():
        x.grad = None
        for p in params:
            p.grad = None

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
    return {"forward": (fwd(form_lib), fwd(form_torch)), "forward + backward": (fwd_bwd(form_lib), fwd_bwd(form_torch))}, clear


def embed_case(C, dev):
    torch.manual_seed(C)
    embed = swin.PatchEmbed(4, 3, C, torch.nn.LayerNorm).to(BF).to(dev)
    img = torch.randn(1, 3, *IMAGE, device=dev).to(BF)      # (the image needs no gradient, as in training)
    dout = torch.randn(1, IMAGE[0] // 4 * (IMAGE[1] // 4), C, device=dev).to(BF)

    def form(fused):
        def run(t):
            embed.fused = fused
            return embed.tokens(t)[0].contiguous()
        return run
    return _forms(form(True), form(False), img, dout, list(embed.parameters()))


def merge_cases(H, W, C, dev):
    torch.manual_seed(C)
    merge = swin.PatchMerging(C).to(BF).to(dev)
    x = torch.randn(1, H * W, C, device=dev).to(BF).requires_grad_(True)
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    norm = merge.norm

    def norm_torch(t):
        t = F.pad(t.view(1, H, W, C), (0, 0, 0, W % 2, 0, H % 2))
        return norm(t.view(1, H2, 2, W2, 2, C).permute(0, 1, 3, 4, 2, 5).reshape(1, H2 * W2, 4 * C))

    def module(fused):
        def run(t):
            merge.fused = fused
            return merge(t, H, W)
        return run
    a, clear = _forms(lambda t: swin.swin_merge_norm(t, H, W, norm.weight, norm.bias, norm.eps), norm_torch, x,
                      torch.randn(1, H2 * W2, 4 * C, device=dev).to(BF), list(merge.parameters()))
    b, _ = _forms(module(True), module(False), x, torch.randn(1, H2 * W2, 2 * C, device=dev).to(BF), list(merge.parameters()))
    return {"merging norm": (a, clear), "PatchMerging": (b, clear)}


def norm_case(H, W, C, dev):
    torch.manual_seed(C)
    norm = torch.nn.LayerNorm(C).to(BF).to(dev)
    x = torch.randn(1, H * W, C, device=dev).to(BF).requires_grad_(True)
    return _forms(lambda t: swin.swin_norm_nchw(t, H, W, norm.weight, norm.bias, norm.eps),
                  lambda t: norm(t).view(-1, H, W, C).permute(0, 3, 1, 2).contiguous(), x, torch.randn(1, C, H, W, device=dev).to(BF),
                  list(norm.parameters()))


def net_case(cfg, dev):
    torch.manual_seed(1)
    net = swin.SwinTransformer(**cfg).to(BF).to(dev).set_fused(True)
    img = torch.randn(1, 3, *IMAGE, device=dev).to(BF)
    params = list(net.parameters())

    def clear():
        for p in params:
            p.grad = None

    def form(stages):
        def run():
            clear()
            net.set_fused_stages(stages)
            sum(f.float().sum() for f in net.forward_raw(img)).backward()
        return run
    return {"forward_raw + backward, blocks fused": (form(True), form(False))}, clear


def time_rows(rows, clear, calls, blocks):
    for lib, ref in rows.values():      # untimed rehearsal
        for _ in range(2):
            lib()
            ref()
    torch.cuda.synchronize()
    last = list(rows.values())[-1]
    mem = {"library": peak_bytes(last[0], clear), "torch": peak_bytes(last[1], clear)}
    t = {k: ([], []) for k in rows}
    for _ in range(blocks):
        for k, (lib, ref) in rows.items():
            t[k][0].append(block_us(lib, calls))
            t[k][1].append(block_us(ref, calls))
    clear()
    stat = lambda v: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
    return {k: {"library": stat(a), "torch": stat(b)} for k, (a, b) in t.items()}, mem


def measure(calls, blocks, net_calls):
    dev = torch.device("cuda", 0)
    cases = []
    for name, C in EMBEDS:
        cases.append((f"{name}: {IMAGE[0]} x {IMAGE[1]} image -> {IMAGE[0] // 4} x {IMAGE[1] // 4} x {C}", lambda C=C: embed_case(C, dev), calls))
    for name, H, W, C in MERGES:
        for what in ("merging norm", "PatchMerging"):
            cases.append((f"{name}, {what}: {H} x {W} x {C}", lambda H=H, W=W, C=C, what=what: merge_cases(H, W, C, dev)[what], calls))
    for name, H, W, C in NORMS:
        cases.append((f"{name} to NCHW: {H} x {W} x {C}", lambda H=H, W=W, C=C: norm_case(H, W, C, dev), calls))
    for name, cfg in NETS:
        cases.append((f"{name} backbone: {IMAGE[0]} x {IMAGE[1]} image", lambda cfg=cfg: net_case(cfg, dev), net_calls))
    out = []
    for name, make, n in cases:
        rows, clear = make()
        res, mem = time_rows(rows, clear, n, blocks)
        rec = {"name": name, "rows": res, "peak_bytes_forward_backward": mem}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        del rows, clear
        torch.cuda.empty_cache()
    return out


def table_of(recs):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"
    lines = ["| boundary | what | library: us per call, median (min .. max over blocks) | torch | library / torch |", "|---|---|---|---|---|"]
    for r in recs:
        for k, v in r["rows"].items():
            lines.append(f"| {r['name']} | {k} | {f(v['library'])} | {f(v['torch'])} | {v['library']['median_us'] / v['torch']['median_us']:.3f} |")
    lines += ["", "| boundary | peak bytes of a forward + backward: library | torch | library / torch |", "|---|---|---|---|"]
    for r in recs:
        m = r["peak_bytes_forward_backward"]
        lines.append(f"| {r['name']} | {m['library'] / 2 ** 20:.1f} MiB | {m['torch'] / 2 ** 20:.1f} MiB | {m['library'] / max(m['torch'], 1):.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--net-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin_stage_timing: no GPU; nothing is measured on a CPU")
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form ({a.net_calls} for the backbones), "
                      "alternating", "", table_of(measure(a.calls, a.blocks, a.net_calls))])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
