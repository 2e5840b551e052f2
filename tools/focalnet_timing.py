#!/usr/bin/env python3
"""Time the FocalNet context kernels (csrc/focalnet_ctx.hip through richsem_amd.focalnet) against the torch bf16 composition they replace, in
ONE process, the forms alternating.

    python tools/focalnet_timing.py [--part kernels|models|all] [--calls 5] [--blocks 5] [--out FILE.md] [--json FILE.json]

Sizes: ``focalnet_L_384_22k_fl4`` (L = 4, window 3, normalised) and ``focalnet_L_384_22k`` (L = 3, window 5) on an 800 x 1344 image, B = 1 and
2: maps of 200 x 336 x 192, 100 x 168 x 384, 50 x 84 x 768 and 25 x 42 x 1536.

``kernels``, per map and model:
  * the context aggregation alone (:func:`richsem_amd.focalnet.focal_context`), forward (under ``no_grad``) and forward + backward (gradients
    for ctx0, the gates and the depthwise weights), against the torch composition of the same formulas in bf16 on NCHW tensors and on
    ``channels_last`` ones;
  * the share of the HBM peak the forward reaches, counting the bytes the kernels must move: ctx0 read, every u_l written once and read by the
    next level and by the gather, A written -- (6 L + 2) bytes per element (8.0 TB/s, the specification's figure).
``models``:
  * the whole backbone (depths 2, 2, 18, 2), forward + backward from the image: the kernel path with ``fused`` off and on against the
    package's own torch composition (the path every unsupported tensor takes, forced by switching the module's device test off).

Method (tools/convnext_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls between two HIP events on the stream; a cell is the median block and the range over the blocks, in microseconds per
call.  There is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import focalnet                                   # noqa: E402
from tools.convnext_timing import run_rows                         # noqa: E402

BF = torch.bfloat16
HBM_PEAK = 8.0e12      # bytes per second (specification)
IMAGE = (800, 1344)
DIMS = (192, 384, 768, 1536)
MAPS = tuple((IMAGE[0] // (4 << i), IMAGE[1] // (4 << i), DIMS[i]) for i in range(4))
MODELS = {"focalnet_L_384_22k_fl4": (4, 3, True), "focalnet_L_384_22k": (3, 5, False)}      # (L, window, normalize)


def composition_nchw(ctx, gates, weights, normalize):
    """the formulas on NCHW tensors (either memory format): ctx (B, C, H, W), gates (B, L + 1, H, W)"""
    L, C, acc = len(weights), ctx.shape[1], 0
    for l, w in enumerate(weights):
        ctx = F.gelu(F.conv2d(ctx, w, None, padding=w.shape[-1] // 2, groups=C))
        acc = acc + ctx * gates[:, l:l + 1]
    acc = acc + F.gelu(ctx.mean((2, 3), keepdim=True)) * gates[:, L:]
    return acc / (L + 1) if normalize else acc


def kernel_rows(model, B, H, W, C, dev):
    L, window, normalize = MODELS[model]
    torch.manual_seed(C + B + L)
    sizes = [window + 2 * l for l in range(L)]
    ws = [(torch.randn(C, 1, k, k, device=dev) / k).to(BF).requires_grad_(True) for k in sizes]
    ws_cl = [w.detach().clone().to(memory_format=torch.channels_last).requires_grad_(True) for w in ws]
    ctx0 = torch.randn(B, H, W, C, device=dev).to(BF).requires_grad_(True)
    gates = torch.randn(B, H, W, L + 1, device=dev).to(BF).requires_grad_(True)
    cn, gn = (t.detach().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for t in (ctx0, gates))
    ccl, gcl = (t.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in (cn, gn))
    g = torch.randn(B, H, W, C, device=dev).to(BF)
    gN = g.permute(0, 3, 1, 2).contiguous()
    gC = gN.contiguous(memory_format=torch.channels_last)
    cache = focalnet.VersionCache()
    forms = {"library": (lambda: focalnet.focal_context(ctx0, gates, ws, normalize, cache=cache), g, [ctx0, gates] + ws),
             "torch NCHW": (lambda: composition_nchw(cn, gn, ws, normalize), gN, [cn, gn] + ws),
             "torch channels_last": (lambda: composition_nchw(ccl, gcl, ws_cl, normalize), gC, [ccl, gcl] + ws_cl)}

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def fb(fn, cot, leaves):
        def run():
            for t in leaves:
                t.grad = None
            fn().backward(cot)
        return run
    return {"context forward": {k: fwd(fn) for k, (fn, _, _) in forms.items()},
            "context forward + backward": {k: fb(fn, cot, leaves) for k, (fn, cot, leaves) in forms.items()}}


def backbone_rows(model, B, dev):
    torch.manual_seed(B)
    net = focalnet.build_focalnet(model, drop_path_rate=0.).to(BF).to(dev)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "gamma" in k:
                p.fill_(1.)
    img = torch.randn(B, 3, *IMAGE, device=dev).to(BF).requires_grad_(True)
    params = list(net.parameters())
    rule = focalnet.on_kernels

    def fb(on, fused=False):
        def run():
            focalnet.on_kernels = rule if on else (lambda x: False)
            net.set_fused(fused)
            try:
                img.grad = None
                for p in params:
                    p.grad = None
                sum(o.float().sum() for o in net.forward_features(img)).backward()
            finally:
                focalnet.on_kernels = rule
        return run
    return {"backbone forward + backward": {"fused off": fb(True), "fused on": fb(True, True), "torch composition": fb(False)}}


def measure(part, calls, blocks):
    dev = torch.device("cuda", 0)
    recs = []
    for model, (L, _, _) in MODELS.items():
        for B in (1, 2):
            if part in ("kernels", "all"):
                for H, W, C in MAPS:
                    rows = run_rows(kernel_rows(model, B, H, W, C, dev), calls, blocks)
                    recs.append({"name": f"{model}, B = {B}, {H} x {W} x {C}", "elements": B * H * W * C, "L": L, "rows": rows})
                    torch.cuda.empty_cache()
            if part in ("models", "all"):
                recs.append({"name": f"{model}, B = {B}, on {IMAGE[0]} x {IMAGE[1]}", "elements": 0, "L": L,
                             "rows": run_rows(backbone_rows(model, B, dev), 1, max(3, blocks // 2))})
                torch.cuda.empty_cache()
    return recs


def table_of(recs):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"      # noqa: E731
    lines = ["| shape | what | form | us per call, median (min .. max over blocks) | / first form |", "|---|---|---|---|---|"]
    for r in recs:
        for k, forms in r["rows"].items():
            first = next(iter(forms.values()))["median_us"]
            for form, v in forms.items():
                lines.append(f"| {r['name']} | {k} | {form} | {f(v)} | {v['median_us'] / first:.2f} |")
    hbm = [(r["name"], r["elements"], r["L"], r["rows"]["context forward"]["library"]["median_us"]) for r in recs if "context forward" in r["rows"]]
    if hbm:
        lines += ["", "| shape | context forward: bytes at (6 L + 2) B per element | GB/s | share of the 8.0 TB/s HBM peak |", "|---|---|---|---|"]
        for name, n, L, us in hbm:
            nbytes = (6 * L + 2) * n
            rate = nbytes / (us * 1e-6)
            lines.append(f"| {name} | {nbytes / 1e6:.1f} MB | {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "models", "all"), default="all")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focalnet_timing: no GPU; nothing is measured on a CPU")
    recs = measure(a.part, a.calls, a.blocks)
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating "
                      f"(the backbone: {max(3, a.blocks // 2)} blocks of 1)", "", table_of(recs)])
    print(text)
    for path, body in ((a.out, text + "\n"), (a.json, json.dumps(recs, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
