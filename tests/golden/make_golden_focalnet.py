#!/usr/bin/env python3
"""Golden vectors for the FocalNet mirrors (richsem_amd/focalnet.py), generated from the REFERENCE's own classes and autograd in float64.

Run in the build container only (it reads /root/reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_focalnet.py

models/richsem/focal.py is loaded by path with the stand-in modules of make_golden_swin.py for ``timm.models.layers`` and ``util.misc``
(neither package is installed).  Nothing of the reference's text is copied.

Cases: ``mod0..9`` -- a ``FocalModulation`` on the channels-last shapes MAPS, each in the two configurations CONFIGS ((L = 3, window 5)
and (L = 4, window 3, normalize_modulator): the kernel sizes of the named models); ``block0..1`` -- a ``FocalModulationBlock`` with
post-LN and layer scale, without and with ``use_postln_in_modulation``; ``net`` -- a three-stage ``FocalNet`` at a toy size (conv embed,
post-LN, layer scale; the maps are 12 x 14, 6 x 7 and 3 x 4).  Gradients come from ``sum(out * g)``.

Storage as in make_golden_swin.py: parameters, inputs and cotangents are seeded dyadic Gaussians stored as int16 (value * 64); outputs and
gradients are float64, a tensor of more than FULL elements as every ``stride``-th element of its flattened form (``<name>.stride``, odd)
plus the sum of all its elements (``<name>.sum``).  To keep the file under 1 MiB with ten modulation cases, FULL is 128 here and the
values lie on coarser grids, which compress better: matrices and taps multiples of 2^-4, inputs and cotangents multiples of 2^-2 (norm
weights, biases and layer scales stay multiples of 2^-6).  The depthwise weight gradients and the gradient of
``f`` (whose last L + 1 rows are the gates') on a 1 x 1 map are stored WHOLE, for the reason make_golden_convnext.py records: all taps
but the centre one never meet a pixel there, and an error statistic over the few non-zero elements a stride keeps is noise.
"""
import importlib.util
import math
import os

import numpy as np
import torch

import make_golden_swin as S

OUT = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/models/richsem/focal.py"

MAPS = ((2, 1, 1, 32), (2, 2, 3, 32), (2, 13, 9, 96), (1, 16, 17, 64), (2, 17, 15, 32))      # (B, H, W, C)
CONFIGS = (dict(focal_level=3, focal_window=5), dict(focal_level=4, focal_window=3, normalize_modulator=True))
BLOCKS = (dict(use_postln=True, use_layerscale=True), dict(use_postln=True, use_layerscale=True, use_postln_in_modulation=True))
BLOCK_MAP = (2, 7, 10, 64)
BLOCK_LEVELS = dict(focal_level=3, focal_window=5)
NET = dict(embed_dim=32, depths=[1, 2, 1], focal_levels=[3, 4, 3], focal_windows=[5, 3, 5], use_conv_embed=True, use_postln=True,
           use_layerscale=True, normalize_modulator=True, drop_path_rate=0., out_indices=(0, 1, 2), mlp_ratio=1.)
NET_IMAGE = (2, 3, 45, 54)


def load_reference():
    S.load_reference()      # (registers the stand-ins for timm.models.layers and util.misc)
    spec = importlib.util.spec_from_file_location("reference_focal", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dyadic(shape, g, std=1.0, mean=0.0, grid=4):
    """seeded Gaussians rounded to multiples of 1 / grid"""
    return ((torch.randn(*shape, generator=g, dtype=torch.float64) * std + mean) * grid).round().clamp(-255, 255).div(grid)


def record(out, tag, module, x, outs, g):
    """make_golden_swin.record with this file's grid for the cotangents"""
    for k, v in module.state_dict().items():
        S.put_exact(out, f"{tag}.sd.{k}", v)
    S.put_exact(out, f"{tag}.x", x)
    loss = 0.
    for i, o in enumerate(outs):
        cot = dyadic(o.shape, g)
        S.put_exact(out, f"{tag}.g{i}", cot)
        S.put(out, f"{tag}.out{i}", o)
        loss = loss + (o * cot).sum()
    loss.backward()
    S.put(out, f"{tag}.x_grad", x.grad)
    for k, p in module.named_parameters():
        S.put(out, f"{tag}.grad.{k}", p.grad)
        if "focal_layers" in k:
            put_coprime(out, f"{tag}.grad.{k}", p.grad)


def fill(module, g):
    """seeded dyadic values: norm weights and the layer scales around 1, other vectors std 1/4, the depthwise taps std 1/4, matrices 1/8"""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 1 and ("gamma" in name or ("norm" in name or name.endswith("ln.weight")) and name.endswith("weight")):
                p.copy_(S.dyadic(p.shape, g, 0.25, 1.0))
            elif p.dim() == 1:
                p.copy_(S.dyadic(p.shape, g, 0.25))
            elif "focal_layers" in name:
                p.copy_(dyadic(p.shape, g, 0.25, grid=16))
            else:
                p.copy_(dyadic(p.shape, g, 0.125, grid=16))


def put_coprime(out, name, t):
    """a depthwise weight gradient (C, 1, K, K): make_golden_swin.put with the stride raised to the next odd number that shares no factor
    with K -- a stride that is a multiple of K K (81 at C = 128) would keep one and the same tap of every channel, a corner tap that
    never meets a pixel of a small map"""
    a = t.detach().double().contiguous().view(-1)
    if a.numel() <= S.FULL:
        return
    stride = (a.numel() // S.FULL) | 1
    while math.gcd(stride, t.shape[-1]) != 1:
        stride += 2
    out[name] = a[::stride].numpy()
    out[name + ".stride"] = np.int64(stride)


def keep_whole(out, name, t):
    out[name] = t.detach().double().numpy()
    out.pop(name + ".stride", None)
    out.pop(name + ".sum", None)


def main():
    ref = load_reference()
    S.FULL = 128
    out = {}
    n = 0
    for shape in MAPS:
        for cfg in CONFIGS:
            B, H, W, C = shape
            g = torch.Generator().manual_seed(350 + n)
            mod = ref.FocalModulation(C, **cfg).double()
            fill(mod, g)
            x = dyadic(shape, g).requires_grad_(True)
            y = mod(x)
            record(out, f"mod{n}", mod, x, (y,), g)
            if H == 1 and W == 1:
                for k, p in mod.named_parameters():
                    if "focal_layers" in k or k.startswith("f."):
                        keep_whole(out, f"mod{n}.grad.{k}", p.grad)
            out[f"mod{n}.cfg"] = np.array([B, H, W, C, cfg["focal_level"], cfg["focal_window"], int(cfg.get("normalize_modulator", False))],
                                          dtype=np.int64)
            print(f"mod{n}", shape, cfg, tuple(y.shape))
            n += 1
    for n, cfg in enumerate(BLOCKS):
        B, H, W, C = BLOCK_MAP
        g = torch.Generator().manual_seed(370 + n)
        blk = ref.FocalModulationBlock(C, mlp_ratio=1., layerscale_value=1., **BLOCK_LEVELS, **cfg).double()
        fill(blk, g)
        blk.H, blk.W = H, W
        x = dyadic((B, H * W, C), g).requires_grad_(True)
        y = blk(x)
        record(out, f"block{n}", blk, x, (y,), g)
        out[f"block{n}.cfg"] = np.array([B, H, W, C, int(cfg.get("use_postln_in_modulation", False))], dtype=np.int64)
        print(f"block{n}", cfg, tuple(y.shape))
    g = torch.Generator().manual_seed(379)
    net = ref.FocalNet(**NET).double()
    fill(net, g)      # (the layer scales too: their initial 1e-4 would hide the blocks behind the residual stream)
    img = dyadic(NET_IMAGE, g).requires_grad_(True)
    res = net(S.sys.modules["util.misc"].NestedTensor(img, torch.zeros(NET_IMAGE[0], NET_IMAGE[2], NET_IMAGE[3], dtype=torch.bool)))
    feats = tuple(res[i].tensors for i in range(len(res)))
    record(out, "net", net, img, feats, g)
    assert [tuple(f.shape[-2:]) for f in feats] == [(12, 14), (6, 7), (3, 4)]
    print("net", [tuple(f.shape) for f in feats], sum(p.numel() for p in net.parameters()), "parameters")
    path = os.path.join(OUT, "layer_focalnet_reference.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
