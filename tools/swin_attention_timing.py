#!/usr/bin/env python3
"""Time ``richsem_amd.swin.window_attention`` (csrc/swin_attn_mfma.hip: one kernel forward, one + a table reduction backward) against the
torch bf16 composition it replaces -- roll, window partition, q k^T, relative-position bias gather, region mask, softmax, P v, window
reverse, roll back, as the reference's SwinTransformerBlock / WindowAttention do them --, in ONE process, the forms alternating.

    python tools/swin_attention_timing.py [--calls 10] [--blocks 8] [--out FILE.md]

Both forms take the same padded map-layout ``qkv`` (B, Hp, Wp, 3 C) bf16 and return (B, Hp, Wp, C); the qkv / proj products, the norms
and the padding are outside both.  The composition's bias index and (windows, N, N) mask are built once, outside the timed calls, as the
reference builds its mask once per layer.  Shapes: the four Swin-L stages of an 800 x 1344 image at B = 1, w = 12 (token maps 200 x 336,
100 x 168, 50 x 84, 25 x 42 with 6, 12, 24, 48 heads, padded to multiples of 12) and the first Swin-T stage at w = 7 (200 x 336, 3 heads),
each unshifted and shifted by w // 2.

Method: every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block ``--calls`` calls between two
HIP events on the stream; a row is the median block and the range over the blocks, in microseconds per call.  ``forward`` runs under
``torch.no_grad``; ``forward + backward`` with a fixed dout, gradients for qkv and the table.  There is no CPU path."""
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

# (name, H, W, heads, window)
STAGES = (("Swin-L stage 1", 200, 336, 6, 12), ("Swin-L stage 2", 100, 168, 12, 12), ("Swin-L stage 3", 50, 84, 24, 12),
          ("Swin-L stage 4", 25, 42, 48, 12), ("Swin-T stage 1", 200, 336, 3, 7))


class Composition:
    """the reference's sequence on a padded map, in the operands' dtype"""

    def __init__(self, Hp, Wp, nH, w, s, dev):
        self.args = (Hp, Wp, nH, w, s)
        self.index = swin.bias_index(w, dev).reshape(-1)
        self.mask = None
        if s:
            py, px = torch.arange(Hp, device=dev), torch.arange(Wp, device=dev)
            ids = 3 * ((py >= Hp - w).long() + (py >= Hp - s).long())[:, None] + ((px >= Wp - w).long() + (px >= Wp - s).long())[None, :]
            ids = ids.view(Hp // w, w, Wp // w, w).permute(0, 2, 1, 3).reshape(-1, w * w)
            self.mask = ((ids[:, :, None] != ids[:, None, :]).to(torch.bfloat16) * -100.0)

    def __call__(self, qkv, table):
        Hp, Wp, nH, w, s = self.args
        B, C3, N, nW = qkv.shape[0], qkv.shape[-1], w * w, (Hp // w) * (Wp // w)
        x = torch.roll(qkv, shifts=(-s, -s), dims=(1, 2)) if s else qkv
        win = x.view(B, Hp // w, w, Wp // w, w, C3).permute(0, 1, 3, 2, 4, 5).contiguous().view(B * nW, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
        attn = (win[0] * 32 ** -0.5) @ win[1].transpose(-2, -1)
        attn = attn + table[self.index].view(N, N, nH).permute(2, 0, 1).contiguous().unsqueeze(0)
        if self.mask is not None:
            attn = (attn.view(B, nW, nH, N, N) + self.mask.unsqueeze(1).unsqueeze(0)).view(-1, nH, N, N)
        o = (attn.softmax(-1) @ win[2]).transpose(1, 2).reshape(B, Hp // w, Wp // w, w, w, C3 // 3)
        o = o.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, C3 // 3)
        return torch.roll(o, shifts=(s, s), dims=(1, 2)) if s else o


def cases(dev):
    gen = torch.Generator().manual_seed(0)
    for name, H, W, nH, w in STAGES:
        Hp, Wp = -(-H // w) * w, -(-W // w) * w
        for s in (0, w // 2):
            qkv = torch.randn(1, Hp, Wp, 3 * 32 * nH, generator=gen).to(torch.bfloat16).to(dev).requires_grad_(True)
            table = (torch.randn((2 * w - 1) ** 2, nH, generator=gen) * 0.5).to(torch.bfloat16).to(dev).requires_grad_(True)
            dout = torch.randn(1, Hp, Wp, 32 * nH, generator=gen).to(torch.bfloat16).to(dev)
            forms = {"library": lambda q, t, nH=nH, w=w, s=s: swin.window_attention(q, t, nH, w, s), "torch": Composition(Hp, Wp, nH, w, s, dev)}
            fns = {}
            for k, form in forms.items():
                def fwd(form=form, qkv=qkv, table=table):
                    with torch.no_grad():
                        return form(qkv, table)

                def fwd_bwd(form=form, qkv=qkv, table=table, dout=dout):
                    qkv.grad = table.grad = None
                    form(qkv, table).backward(dout)
                fns[k + " forward"], fns[k + " forward + backward"] = fwd, fwd_bwd
            a, b = fns["library forward"](), fns["torch forward"]()
            torch.cuda.synchronize()
            yield f"{name}: {Hp} x {Wp}, {nH} heads, w = {w}, shift {s}", fns, float((a.float() - b.float()).abs().max())


def measure(calls, blocks):
    rows = []
    for name, fns, diff in cases(torch.device("cuda", 0)):
        for fn in fns.values():      # untimed rehearsal
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(blocks):
            for k, fn in fns.items():
                t[k].append(block_us(fn, calls))
        row = {"name": name, "max_abs_difference_between_the_forms": diff}
        for k in fns:
            row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def table_of(rows):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"
    lines = ["| shape | pass | library: us per call, median (min .. max over blocks) | torch composition | library / torch |", "|---|---|---|---|---|"]
    for r in rows:
        for what in ("forward", "forward + backward"):
            a, b = r["library " + what], r["torch " + what]
            lines.append(f"| {r['name']} | {what} | {f(a)} | {f(b)} | {a['median_us'] / b['median_us']:.3f} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swin_attention_timing: no GPU; nothing is measured on a CPU")
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "",
                      table_of(measure(a.calls, a.blocks))])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
