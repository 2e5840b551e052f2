#!/usr/bin/env python3
"""Golden vectors for the class head (richsem_amd/class_head.py), generated from the REFERENCE's own ``CLIPAlign.forward_hs`` and autograd.

Run in the build container only (it reads /root/reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_cls_head.py

``CLIPAlign`` (richsem.py:38-205) is cut out of the source with ``ast`` and instantiated without CLIP, exactly as
tests/golden/make_golden_cls.py does.  What runs is the reference's ``forward_hs`` on a list of two ``hs`` tensors, then
``logits.backward(g)``.  The inputs are seeded Gaussians rounded to multiples of 2^-6 (the file compresses; they are exact in every dtype);
in the float32 configuration g is non-zero on ``cls_idx`` only -- 200 of the 1204 classes, the first, the last and the tile edges among
them -- and ``logits`` / ``g`` are stored on that slice: the full tensors are not needed.
"""
import os

import numpy as np
import torch
from torch import nn

from make_golden_cls import reference_class

OUT = os.path.dirname(os.path.abspath(__file__))


def dyadic(shape, g, dtype, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale * 64).round().div(64).to(dtype)


def main():
    CLIPAlign = reference_class()
    out = {}
    for tag, dtype, seed, rows, classes, proj in (("f64", torch.float64, 15, 37, 97, 48), ("f32", torch.float32, 16, 24, 1204, 64)):
        g = torch.Generator().manual_seed(seed)
        m = CLIPAlign.__new__(CLIPAlign)
        nn.Module.__init__(m)
        m.dino_visual_proj = nn.Linear(256, proj, bias=False).to(dtype)
        with torch.no_grad():
            m.dino_visual_proj.weight.copy_(dyadic((proj, 256), g, dtype))             # spread 1: x . (A x) stays well conditioned
        m.text_proj = None
        m.text_embed = dyadic((classes, proj), g, dtype)
        m.logit_scale = nn.Parameter(torch.tensor(np.log(1 / 0.07), dtype=dtype), requires_grad=False)
        hs = [dyadic((1, rows, 256), g, dtype).requires_grad_(True) for _ in range(2)]
        if classes > 200:
            edges = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, classes - 17, classes - 16, classes - 5, classes - 4, classes - 2, classes - 1]
            rest = np.setdiff1d(np.arange(classes), edges)
            pick = rest[torch.randperm(len(rest), generator=g)[:200 - len(edges)].numpy()]
            cls_idx = np.sort(np.concatenate([edges, pick]))
        else:
            cls_idx = np.arange(classes)
        grad = torch.zeros(2, 1, rows, classes, dtype=dtype)
        grad[..., cls_idx] = dyadic((2, 1, rows, len(cls_idx)), g, dtype)
        logits = m.forward_hs(hs)                                          # the reference's CLIPAlign.forward_hs: (2, 1, rows, classes)
        logits.backward(grad)
        out.update({f"{tag}.hs": torch.stack([h.detach() for h in hs]).numpy(), f"{tag}.proj_weight": m.dino_visual_proj.weight.detach().numpy(),
                    f"{tag}.text_embed": m.text_embed.numpy(), f"{tag}.logit_scale": m.logit_scale.detach().numpy(),
                    f"{tag}.cls_idx": cls_idx.astype(np.int64), f"{tag}.g": grad[..., cls_idx].numpy(),
                    f"{tag}.logits": logits.detach()[..., cls_idx].numpy(), f"{tag}.hs_grad": torch.stack([h.grad for h in hs]).numpy(),
                    f"{tag}.proj_weight_grad": m.dino_visual_proj.weight.grad.numpy()})
        print(tag, tuple(logits.shape), len(cls_idx))
    path = os.path.join(OUT, "cls_head_reference.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
