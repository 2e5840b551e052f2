#!/usr/bin/env python3
"""Time the ConvNeXt kernels (csrc/convnext_dw.hip through richsem_amd.convnext) against the torch bf16 ops they replace, in ONE process, the
forms alternating.

    python tools/convnext_timing.py [--part kernels|models|all] [--calls 10] [--blocks 6] [--out FILE.md] [--json FILE.json]

Sizes: ``convnext_xlarge`` on an 800 x 1344 image, B = 1 and 2: maps of 200 x 336 x 256, 100 x 168 x 512, 50 x 84 x 1024 and 25 x 42 x 2048.

``kernels``, per map:
  * ``dwconv7`` forward (under ``no_grad``) and forward + backward (gradients for the map, the weight and the bias) against
    ``F.conv2d(groups=C)`` in bf16 on an NCHW tensor and on a ``channels_last`` one;
  * the share of the HBM peak the forward kernel reaches, counting 2 B read + 2 B written per element (8.0 TB/s, the specification's figure);
  * the two layer-scale kernels (``msda_layer_scale_forward_bf16``, ``msda_layer_scale_backward_bf16`` with dgamma).
``models``:
  * one block, forward + backward, ``fused`` off and on, against the torch-op mirror (the reference's NCHW order on the same parameters);
  * the whole backbone (depths 3, 3, 27, 3), forward + backward from the image, the same three forms.

Method (tools/swin_block_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls between two HIP events on the stream; a cell is the median block and the range over the blocks, in microseconds per
call.  There is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import convnext                                   # noqa: E402
from tools.geometry_timing import block_us                         # noqa: E402

BF = torch.bfloat16
HBM_PEAK = 8.0e12      # bytes per second (specification)
IMAGE = (800, 1344)
DIMS = (256, 512, 1024, 2048)
DEPTHS = (3, 3, 27, 3)
MAPS = tuple((IMAGE[0] // (4 << i), IMAGE[1] // (4 << i), DIMS[i]) for i in range(4))


# ---- the torch-op mirror: the reference's order of operations in NCHW on a module's parameters ---------------------------------------------
def norm_nchw(x, ln):
    mean = x.mean(1, keepdim=True)
    var = (x - mean).pow(2).mean(1, keepdim=True)
    return ln.weight[:, None, None] * ((x - mean) / torch.sqrt(var + ln.eps)) + ln.bias[:, None, None]


def torch_block(blk, x):
    z = blk.dwconv(x).permute(0, 2, 3, 1)
    z = blk.pwconv2(F.gelu(blk.pwconv1(F.layer_norm(z, (z.shape[-1],), blk.norm.weight, blk.norm.bias, blk.norm.eps))))
    return x + (blk.gamma * z).permute(0, 3, 1, 2)


def torch_backbone(net, x):
    outs = []
    for i in range(4):
        a, b = net.downsample_layers[i]
        x = norm_nchw(a(x), b) if i == 0 else b(norm_nchw(x, a))
        for blk in net.stages[i]:
            x = torch_block(blk, x)
        outs.append(norm_nchw(x, getattr(net, f"norm{i}")))
    return outs


def stat(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def run_rows(rows, calls, blocks):
    """rows: {name: {form: callable}} -> {name: {form: stat}}; every form untimed first, then alternating blocks"""
    out = {}
    for name, forms in rows.items():
        for fn in forms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in forms}
        for _ in range(blocks):
            for k, fn in forms.items():
                t[k].append(block_us(fn, calls))
        out[name] = {k: stat(v) for k, v in t.items()}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def kernel_rows(B, H, W, C, dev):
    torch.manual_seed(C + B)
    conv = torch.nn.Conv2d(C, C, 7, padding=3, groups=C).to(BF).to(dev)
    x = torch.randn(B, H, W, C, device=dev).to(BF).requires_grad_(True)           # the map
    xn = x.detach().permute(0, 3, 1, 2).contiguous().requires_grad_(True)        # NCHW
    xcl = xn.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g = torch.randn(B, H, W, C, device=dev).to(BF)
    gn = g.permute(0, 3, 1, 2).contiguous()
    gcl = gn.contiguous(memory_format=torch.channels_last)
    conv_cl = torch.nn.Conv2d(C, C, 7, padding=3, groups=C).to(BF).to(dev).to(memory_format=torch.channels_last)
    cache = convnext.VersionCache()
    w49, b32 = convnext.dwconv7_weight_form(conv.weight), conv.bias.detach().float()

    def clear():
        for t in (x, xn, xcl, conv.weight, conv.bias, conv_cl.weight, conv_cl.bias):
            t.grad = None

    def fb(form, inp, cot):
        def run():
            clear()
            form(inp).backward(cot)
        return run

    lib = lambda t: convnext.dwconv7(t, conv.weight, conv.bias, cache=cache)
    z, res = g.view(-1, C), x.detach().view(-1, C)
    gam = torch.rand(C, device=dev) + 0.5
    return {
        "dwconv7 forward": {"library": lambda: convnext.dwconv7_kernel(x.detach(), w49, b32),
                            "torch NCHW": lambda: F.conv2d(xn.detach(), conv.weight.detach(), conv.bias.detach(), padding=3, groups=C),
                            "torch channels_last": lambda: F.conv2d(xcl.detach(), conv_cl.weight.detach(), conv_cl.bias.detach(), padding=3, groups=C)},
        "dwconv7 forward + backward": {"library": fb(lib, x, g), "torch NCHW": fb(conv, xn, gn), "torch channels_last": fb(conv_cl, xcl, gcl)},
        "layer scale": {"forward kernel": lambda: convnext.layer_scale_kernel(z, gam, res),
                        "backward kernel": lambda: convnext.layer_scale_backward_kernel(z, res, gam),
                        "torch res + gamma * z": lambda: res + gam.to(BF) * z},
    }


def block_rows(B, H, W, C, dev):
    torch.manual_seed(C + B)
    blk = convnext.Block(C, layer_scale_init_value=1.).to(BF).to(dev)
    x = torch.randn(B, C, H, W, device=dev).to(BF)
    xm = x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)      # the block inside a stage: channels-last in, channels-last out
    xn = x.clone().requires_grad_(True)
    gm, gn = torch.randn_like(xm), torch.randn_like(xn)
    params = list(blk.parameters())

    def fb(form, inp, cot):
        def run():
            inp.grad = None
            for p in params:
                p.grad = None
            form(inp).backward(cot)
        return run
    return {"block forward + backward": {"fused off": fb(lambda t: blk.set_fused(False).forward_map(t), xm, gm),
                                         "fused on": fb(lambda t: blk.set_fused(True).forward_map(t), xm, gm),
                                         "torch mirror": fb(lambda t: torch_block(blk, t), xn, gn)}}


def backbone_rows(B, dev):
    torch.manual_seed(B)
    net = convnext.build_convnext("convnext_xlarge_22k", False, layer_scale_init_value=1.).to(BF).to(dev)
    img = torch.randn(B, 3, *IMAGE, device=dev).to(BF).requires_grad_(True)
    params = list(net.parameters())

    def fb(form):
        def run():
            img.grad = None
            for p in params:
                p.grad = None
            sum(o.float().sum() for o in form(img)).backward()
        return run
    return {"backbone forward + backward": {"fused off": fb(lambda t: net.set_fused(False).forward_features(t)),
                                            "fused on": fb(lambda t: net.set_fused(True).forward_features(t)),
                                            "torch mirror": fb(lambda t: torch_backbone(net, t))}}


def measure(part, calls, blocks):
    dev = torch.device("cuda", 0)
    recs = []
    for B in (1, 2):
        for H, W, C in MAPS:
            rows = {}
            if part in ("kernels", "all"):
                rows.update(run_rows(kernel_rows(B, H, W, C, dev), calls, blocks))
            if part in ("models", "all"):
                rows.update(run_rows(block_rows(B, H, W, C, dev), calls, blocks))
            recs.append({"name": f"B = {B}, {H} x {W} x {C}", "elements": B * H * W * C, "rows": rows})
            torch.cuda.empty_cache()
        if part in ("models", "all"):
            recs.append({"name": f"B = {B}, convnext_xlarge on {IMAGE[0]} x {IMAGE[1]}", "elements": 0,
                         "rows": run_rows(backbone_rows(B, dev), max(1, calls // 5), max(3, blocks // 2))})
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
    hbm = [(r["name"], r["elements"], r["rows"]["dwconv7 forward"]["library"]["median_us"]) for r in recs if "dwconv7 forward" in r["rows"]]
    if hbm:
        lines += ["", "| shape | dwconv7 forward: bytes at 2 B read + 2 B written per element | GB/s | share of the 8.0 TB/s HBM peak |", "|---|---|---|---|"]
        for name, n, us in hbm:
            rate = 4 * n / (us * 1e-6)
            lines.append(f"| {name} | {4 * n / 1e6:.1f} MB | {rate / 1e9:.0f} | {100 * rate / HBM_PEAK:.1f} % |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "models", "all"), default="all")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("convnext_timing: no GPU; nothing is measured on a CPU")
    recs = measure(a.part, a.calls, a.blocks)
    text = "\n".join([f"device: {torch.cuda.get_device_name(0)}; {a.blocks} blocks of {a.calls} calls per form, alternating "
                      f"(the backbone: {max(3, a.blocks // 2)} blocks of {max(1, a.calls // 5)})", "", table_of(recs)])
    print(text)
    for path, body in ((a.out, text + "\n"), (a.json, json.dumps(recs, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
