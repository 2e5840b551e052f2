#!/usr/bin/env python3
"""Golden vectors for the Swin mirrors (richsem_amd/swin.py), generated from the REFERENCE's own classes and autograd in float64.

Run in the build container only (it reads /root/reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_swin.py

models/richsem/swin_transformer.py is loaded by path.  It imports ``timm.models.layers`` (DropPath, to_2tuple, trunc_normal_) and
``util.misc`` (NestedTensor); neither package is installed, so stand-in modules with those four names are registered first.  Nothing of
the reference's text is copied.

Cases: ``layer0..2`` -- a ``BasicLayer`` of depth 2 (an unshifted and a shifted block) with ``PatchMerging`` on maps that need padding;
``net`` -- a whole ``SwinTransformer`` at a toy size (``forward_raw``).  Gradients come from ``sum(out * g)`` over every output.

Storage.  Parameters, inputs and cotangents are seeded Gaussians rounded to multiples of 2^-6 and stored as int16 (value * 64: exact in
every dtype, and the file compresses); the bias tables have std 0.5 so that a wrong index shows.  Outputs and gradients are float64.  To
keep the file under 1 MB a float64 tensor of more than 256 elements is stored as every ``stride``-th element of its flattened form
(``<name>`` with ``<name>.stride``, stride odd) together with the sum of ALL its elements (``<name>.sum``); smaller ones are whole.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
from torch import nn

OUT = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/models/richsem/swin_transformer.py"
FULL = 256

LAYERS = ((13, 9, 7, 1), (14, 21, 7, 2), (5, 20, 12, 2))      # (H, W, window, heads), batch 2, mlp_ratio 1
NET = dict(embed_dim=32, depths=(2, 2), num_heads=(1, 2), window_size=7, out_indices=(0, 1), mlp_ratio=2., drop_path_rate=0.)
NET_IMAGE = (2, 3, 40, 52)


def load_reference():
    class DropPath(nn.Module):
        def __init__(self, drop_prob=0.):
            super().__init__()
            self.drop_prob = drop_prob

        def forward(self, x):
            assert self.drop_prob == 0. or not self.training
            return x

    class NestedTensor:
        def __init__(self, tensors, mask):
            self.tensors, self.mask = tensors, mask

    layers = types.ModuleType("timm.models.layers")
    layers.DropPath, layers.to_2tuple = DropPath, lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    layers.trunc_normal_ = nn.init.trunc_normal_
    misc = types.ModuleType("util.misc")
    misc.NestedTensor = NestedTensor
    for name, mod in (("timm", types.ModuleType("timm")), ("timm.models", types.ModuleType("timm.models")), ("timm.models.layers", layers),
                      ("util", types.ModuleType("util")), ("util.misc", misc)):
        sys.modules.setdefault(name, mod)
    spec = importlib.util.spec_from_file_location("reference_swin_transformer", REFERENCE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def dyadic(shape, g, std=1.0, mean=0.0):
    return ((torch.randn(*shape, generator=g, dtype=torch.float64) * std + mean) * 64).round().clamp(-255, 255).div(64)


def fill(module, g):
    """seeded dyadic values for every parameter: bias tables std 0.5, norm weights around 1, matrices std 1/8, biases std 1/4"""
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("relative_position_bias_table"):
                p.copy_(dyadic(p.shape, g, 0.5))
            elif p.dim() == 1 and "norm" in name and name.endswith("weight"):
                p.copy_(dyadic(p.shape, g, 0.25, 1.0))
            elif p.dim() == 1:
                p.copy_(dyadic(p.shape, g, 0.25))
            else:
                p.copy_(dyadic(p.shape, g, 0.125))


def put_exact(out, name, t):
    v = (t.detach().double() * 64).round()
    assert torch.equal(v / 64, t.detach().double()) and float(v.abs().max()) < 32768, name
    out[name] = v.numpy().astype(np.int16)


def put(out, name, t):
    a = t.detach().double().contiguous().view(-1)
    if a.numel() <= FULL:
        out[name] = t.detach().double().numpy()
        return
    stride = (a.numel() // FULL) | 1
    out[name] = a[::stride].numpy()
    out[name + ".stride"] = np.int64(stride)
    out[name + ".sum"] = np.float64(a.sum())


def record(out, tag, module, x, outs, g):
    """state dict, input, outputs, cotangents, and the gradients of sum(out * cotangent)"""
    for k, v in module.state_dict().items():
        if v.dtype.is_floating_point:
            put_exact(out, f"{tag}.sd.{k}", v)
        else:
            out[f"{tag}.sd.{k}"] = v.numpy()
    put_exact(out, f"{tag}.x", x)
    loss = 0.
    for i, o in enumerate(outs):
        cot = dyadic(o.shape, g)
        put_exact(out, f"{tag}.g{i}", cot)
        put(out, f"{tag}.out{i}", o)
        loss = loss + (o * cot).sum()
    loss.backward()
    put(out, f"{tag}.x_grad", x.grad)
    for k, p in module.named_parameters():
        put(out, f"{tag}.grad.{k}", p.grad)


def main():
    ref = load_reference()
    out = {}
    for n, (H, W, w, nH) in enumerate(LAYERS):
        g = torch.Generator().manual_seed(310 + n)
        layer = ref.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=ref.PatchMerging).double()
        fill(layer, g)
        x = dyadic((2, H * W, 32 * nH), g).requires_grad_(True)
        x_out, _, _, x_down, _, _ = layer(x, H, W)
        record(out, f"layer{n}", layer, x, (x_out, x_down), g)
        out[f"layer{n}.cfg"] = np.array([H, W, w, nH], dtype=np.int64)
        print(f"layer{n}", (H, W, w, nH), tuple(x_out.shape), tuple(x_down.shape))
    g = torch.Generator().manual_seed(319)
    net = ref.SwinTransformer(**NET).double()
    fill(net, g)
    img = dyadic(NET_IMAGE, g).requires_grad_(True)
    feats = net.forward_raw(img)
    record(out, "net", net, img, feats, g)
    print("net", [tuple(f.shape) for f in feats])
    path = os.path.join(OUT, "layer_swin_reference.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
