#!/usr/bin/env python3
"""Time the mask-term kernels (csrc/mask_terms.hip through richsem_amd.masks) against the torch compositions they replace, in ONE process, the
forms alternating.

    python tools/mask_terms_timing.py [--calls 5] [--blocks 5] [--out FILE.md] [--json FILE.json]

Sizes: N = 2 images, Q = 300 queries, ``pred_masks`` at stride 8 of an 800 x 1344 canvas (100 x 168), 24 and 200 pairs, float32 and bfloat16.
  * the loss forward (under ``no_grad``) and forward + backward: ``mask_losses`` against ``mask_losses_torch`` (the reference's formula on the
    same buffers, same device, same type);
  * the peak memory either form takes beyond what was allocated before the call (``torch.cuda.max_memory_allocated``), forward + backward;
    the previous call's ``pred_masks.grad`` is allocated then and freed inside the call, so the gradient tensor itself is not in the figure;
  * the share of the HBM peak the forward reaches, counting what it must move: one byte per canvas pixel of every pair and the pair's logits
    once (8.0 TB/s, the specification's figure);
  * the post-processor, 300 rows per image to a 480 x 640 original: ``PostProcessSegm`` against its torch composition on the device (the x4
    bilinear map, sigmoid, threshold, crop, nearest resize of the float copy, byte cast -- the reference's steps without its copy to the host).

Method (tools/convnext_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls between two HIP events on the stream; a cell is the median block and the range over the blocks, in microseconds per call.
There is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import masks                                      # noqa: E402
from tools.convnext_timing import run_rows                         # noqa: E402

HBM_PEAK = 8.0e12      # bytes per second (specification)
N, Q, CANVAS, STRIDE = 2, 300, (800, 1344), 8
H, W = CANVAS[0] // STRIDE, CANVAS[1] // STRIDE
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def loss_setup(pairs, dtype, dev):
    gen = torch.Generator().manual_seed(pairs)
    per = pairs // N
    tg = [{"masks": torch.rand(per, 1, 1, generator=gen).expand(per, CANVAS[0] - 40 * b, CANVAS[1] - 64 * b)
           > torch.rand(1, CANVAS[0] - 40 * b, CANVAS[1] - 64 * b, generator=gen)} for b in range(N)]
    mt = masks.MaskTargets(N, pairs, CANVAS, dev).update_(tg)
    qot = torch.cat([torch.randperm(Q, generator=gen)[:per] for _ in range(N)]).to(dev)
    pred = (torch.randn(N, Q, H, W, generator=gen) * 3).to(dev, dtype).requires_grad_(True)
    return pred, mt, qot, float(pairs)


def loss_rows(pairs, dtype, dev):
    pred, mt, qot, nb = loss_setup(pairs, dtype, dev)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(pred, mt, qot, nb)
        return run

    def fb(fn):
        def run():
            pred.grad = None
            out = fn(pred, mt, qot, nb)
            (out["loss_mask"] + out["loss_dice"]).backward()
        return run
    forms = {"forward": {"library": fwd(masks.mask_losses), "torch composition": fwd(masks.mask_losses_torch)},
             "forward + backward": {"library": fb(masks.mask_losses), "torch composition": fb(masks.mask_losses_torch)}}
    return forms, fb


def peak_extra(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def torch_postprocess(pred, img_sizes, out_sizes, threshold=0.5):
    h, w = pred.shape[-2:]
    m = F.interpolate(pred, size=(h * 4, w * 4), mode="bilinear", align_corners=False).sigmoid() > threshold
    return [F.interpolate(cur[:, :ih, :iw].unsqueeze(1).float(), size=tuple(o), mode="nearest").byte() for cur, (ih, iw), o in zip(m, img_sizes, out_sizes)]


def post_rows(dtype, dev):
    gen = torch.Generator().manual_seed(3)
    pred = (torch.randn(N, Q, H, W, generator=gen) * 3).to(dev, dtype)
    img, out = [(400, 600), (380, 672)], [(480, 640), (480, 640)]
    post = masks.PostProcessSegm()
    sizes = (torch.tensor(out), torch.tensor(img))
    return {"post-process": {"library": lambda: post([{} for _ in range(N)], {"pred_masks": pred}, *sizes),
                             "torch composition": lambda: torch_postprocess(pred, img, out)}}


def measure(calls, blocks):
    dev = torch.device("cuda", 0)
    recs = []
    for name, dtype in DT.items():
        for pairs in (24, 200):
            forms, fb = loss_rows(pairs, dtype, dev)
            rows = run_rows(forms, calls, blocks)
            peaks = {k: peak_extra(fn) for k, fn in forms["forward + backward"].items()}
            need = pairs * (CANVAS[0] * CANVAS[1] + H * W * (2 if dtype == torch.bfloat16 else 4))
            recs.append({"name": f"{pairs} pairs, {name}", "rows": rows, "peak_extra_bytes": peaks, "forward_bytes": need})
            print(json.dumps({"peak_extra_bytes": peaks}), flush=True)
            del forms, fb
            torch.cuda.empty_cache()
        recs.append({"name": f"{Q} rows per image to 480 x 640, {name}", "rows": run_rows(post_rows(dtype, dev), calls, blocks)})
        torch.cuda.empty_cache()
    return recs


def table_of(recs):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"
    lines = ["| shape | what | form | us per call, median (min .. max over blocks) | / first form |", "|---|---|---|---|---|"]
    for r in recs:
        for k, forms in r["rows"].items():
            first = next(iter(forms.values()))["median_us"]
            for form, v in forms.items():
                lines.append(f"| {r['name']} | {k} | {form} | {f(v)} | {v['median_us'] / first:.2f} |")
    lines += ["", "| shape | peak memory beyond the inputs and the gradient tensor, forward + backward: library | torch composition | forward: bytes it must move | GB/s | share of the 8.0 TB/s HBM peak |",
              "|---|---|---|---|---|---|"]
    for r in recs:
        if "peak_extra_bytes" in r:
            us = r["rows"]["forward"]["library"]["median_us"]
            rate = r["forward_bytes"] / (us * 1e-6)
            p = r["peak_extra_bytes"]
            lines.append(f"| {r['name']} | {p['library'] / 1e6:.1f} MB | {p['torch composition'] / 1e6:.1f} MB | {r['forward_bytes'] / 1e6:.1f} MB | "
                         f"{rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_terms_timing: no GPU; nothing is measured on a CPU")
    recs = measure(a.calls, a.blocks)
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating", "", table_of(recs)])
    print(text)
    for path, body in ((a.out, text + "\n"), (a.json, json.dumps(recs, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
