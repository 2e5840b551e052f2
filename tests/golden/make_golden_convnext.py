#!/usr/bin/env python3
"""Golden vectors for the ConvNeXt mirrors (richsem_amd/convnext.py), generated from the REFERENCE's own classes and autograd in float64.

Run in the build container only (it reads /root/reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_convnext.py

models/richsem/convnext.py is loaded by path with the stand-in modules of make_golden_swin.py for ``timm.models.layers`` and ``util.misc``
(neither package is installed).  Nothing of the reference's text is copied.

Cases: ``block0..3`` -- a ``Block`` with ``layer_scale_init_value=1`` (so that ``gamma`` exists) on NCHW inputs whose channels-last shapes
are BLOCKS below: a map smaller than the kernel, a single pixel, a width that is no power of two, a map just past a 16-pixel tile;
``net`` -- a whole ``ConvNeXt`` at a toy size (``forward_features``, all four outputs; the maps are 11 x 13, 5 x 6, 2 x 3 and 1 x 1: the
unpadded stem and downsampling convolutions drop trailing rows and columns at every level).  Gradients come from ``sum(out * g)``.

Storage as in make_golden_swin.py: parameters, inputs and cotangents are seeded Gaussians rounded to multiples of 2^-6 and stored as
int16 (value * 64); outputs and gradients are float64, a tensor of more than 256 elements as every ``stride``-th element of its flattened
form (``<name>.stride``, odd) plus the sum of all its elements (``<name>.sum``).  One exception: the depthwise weight gradient on a
1 x 1 map (``block3`` and the network's last stage) is stored WHOLE.  There 48 of the 49 taps never meet a pixel, so the (128, 1, 7, 7)
gradient is zero except its 128 centre taps, and every 25th element would keep 5 of those: an error statistic over 5 values is noise (on
the device a kernel path and a torch composition whose errors over all 128 are equal came out 2.8 apart on those 5).  Whole, the tensor
is mostly zeros and costs the compressed file 2 KB.
"""
import importlib.util
import os

import numpy as np
import torch

import make_golden_swin as S

OUT = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/models/richsem/convnext.py"

BLOCKS = ((2, 3, 5, 32), (2, 13, 9, 96), (1, 16, 17, 64), (2, 1, 1, 128))      # (B, H, W, C)
NET = dict(depths=(1, 1, 2, 1), dims=(32, 64, 96, 128), layer_scale_init_value=1., out_indices=(0, 1, 2, 3))
NET_IMAGE = (2, 3, 45, 54)


def load_reference():
    S.load_reference()      # (registers the stand-ins for timm.models.layers and util.misc)
    spec = importlib.util.spec_from_file_location("reference_convnext", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def fill(module, g):
    """seeded dyadic values: norm weights and gamma around 1, other vectors std 1/4, the 7 x 7 taps std 1/4, matrices std 1/8"""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 1 and (name.endswith("gamma") or ("norm" in name or "downsample_layers" in name) and name.endswith("weight")):
                p.copy_(S.dyadic(p.shape, g, 0.25, 1.0))
            elif p.dim() == 1:
                p.copy_(S.dyadic(p.shape, g, 0.25))
            elif name.endswith("dwconv.weight"):
                p.copy_(S.dyadic(p.shape, g, 0.25))
            else:
                p.copy_(S.dyadic(p.shape, g, 0.125))


def keep_whole(out, name, t):
    out[name] = t.detach().double().numpy()
    out.pop(name + ".stride", None)
    out.pop(name + ".sum", None)


def main():
    ref = load_reference()
    out = {}
    for n, (B, H, W, C) in enumerate(BLOCKS):
        g = torch.Generator().manual_seed(340 + n)
        blk = ref.Block(dim=C, layer_scale_init_value=1.).double()
        fill(blk, g)
        x = S.dyadic((B, C, H, W), g).requires_grad_(True)
        y = blk(x)
        S.record(out, f"block{n}", blk, x, (y,), g)
        if H == 1 and W == 1:
            keep_whole(out, f"block{n}.grad.dwconv.weight", blk.dwconv.weight.grad)
        out[f"block{n}.cfg"] = np.array([B, H, W, C], dtype=np.int64)
        print(f"block{n}", (B, H, W, C), tuple(y.shape))
    g = torch.Generator().manual_seed(349)
    net = ref.ConvNeXt(**NET).double()
    fill(net, g)
    img = S.dyadic(NET_IMAGE, g).requires_grad_(True)
    feats = net.forward_features(img)
    S.record(out, "net", net, img, feats, g)
    assert tuple(feats[3].shape[-2:]) == (1, 1)
    keep_whole(out, "net.grad.stages.3.0.dwconv.weight", net.stages[3][0].dwconv.weight.grad)
    print("net", [tuple(f.shape) for f in feats])
    path = os.path.join(OUT, "layer_convnext_reference.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
