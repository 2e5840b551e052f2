#!/usr/bin/env python3
"""Golden vectors for the batch-geometry tensors (richsem_amd/geometry.py, csrc/msda_geometry.h), generated from the REFERENCE's own code.

Run in the build container only (it reads /root/reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_geometry.py

What is executed is the reference's code, on the CPU, in float32 as the model runs it:
  * ``PositionEmbeddingSineHW`` (models/richsem/position_encoding.py:46-92) -- the class is cut out of its file with ``ast`` (the file imports
    ``util.misc``, which imports torchvision) and built as the reference's config builds it: num_pos_feats 128, temperatureH = temperatureW =
    20, normalize=True;
  * ``gen_encoder_output_proposals`` (models/richsem/utils.py:10-65), cut out the same way; it is given a memory of ones, so the rows it zeroes
    are read off its first output;
  * ``DeformableTransformer.get_valid_ratio`` (deformable_transformer.py:253-260) and ``TransformerEncoder.get_reference_points`` (:513-525),
    the two methods cut out of their classes and run as plain functions;
  * the level masks as richsem.py:607-608 forms them: ``F.interpolate(mask[None].float(), size=level).to(torch.bool)[0]`` of the image mask
    ``nested_tensor_from_tensor_list`` would build for images of the recorded sizes (padding = bottom / right).

tests/golden/geometry/geometry_reference.npz (a directory of its own, like postprocess/: tests/conftest.py takes every .npz directly under
tests/golden for a fixture of the operator) holds, per case ``<canvas>.<set>``: ``sizes`` (N, 2) int32, ``canvas`` (2), ``shapes`` (L, 2), the level
masks ``mask<l>`` (N, h, w) bool, ``valid_ratios`` (N, L, 2), ``ref`` (N, S, L, 2), ``pos_sine`` (N, S, 256: permuted to channels-last and
flattened over (h, w), levels concatenated), ``proposals`` (N, S, 4) and ``zeroed`` (N, S) bool.
"""
import ast
import math
import os
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

# canvas -> the pyramid's levels (workload.pyramid_shapes of it): the smallest one, with a 1-row level; one whose strides do not divide it
CANVASES = {(64, 96): [(8, 12), (4, 6), (2, 3), (1, 2)], (72, 104): [(9, 13), (5, 7), (3, 4), (2, 2)]}


def size_sets(H, W):
    return {"main": [(H, W), (H // 2 + 3, W // 3 + 5), (1, 1)], "edge": [(H, 17), (31, W)]}


def _cut(path, owner, names, ns):
    """the named functions of ``path`` -- top-level ones (``owner`` None) or methods of the class ``owner`` -- or, with ``names`` None, the class
    ``owner`` itself, executed on their own: none of the file's imports run.  Decorators are dropped (a staticmethod becomes a function)."""
    tree = ast.parse(open(path).read())
    body = tree.body
    if owner is not None:
        cls = [n for n in body if isinstance(n, ast.ClassDef) and n.name == owner]
        assert len(cls) == 1, (path, owner)
        if names is None:
            exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), ns)
            return ns[owner]
        body = cls[0].body
    fns = [n for n in body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == len(names), (path, owner, names)
    for f in fns:
        f.decorator_list = []
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return [ns[n] for n in names]


def reference_functions():
    ns = {"torch": torch, "nn": nn, "math": math, "F": F, "Tensor": torch.Tensor, "NestedTensor": types.SimpleNamespace}
    pe = _cut(f"{REF}/models/richsem/position_encoding.py", "PositionEmbeddingSineHW", None, dict(ns))
    proposals, = _cut(f"{REF}/models/richsem/utils.py", None, ["gen_encoder_output_proposals"], dict(ns))
    valid_ratio, = _cut(f"{REF}/models/richsem/deformable_transformer.py", "DeformableTransformer", ["get_valid_ratio"], dict(ns))
    ref_points, = _cut(f"{REF}/models/richsem/deformable_transformer.py", "TransformerEncoder", ["get_reference_points"], dict(ns))
    return pe(num_pos_feats=128, temperatureH=20, temperatureW=20, normalize=True), proposals, valid_ratio, ref_points


def main():
    position, gen_proposals, get_valid_ratio, get_reference_points = reference_functions()
    out = {}
    for (H, W), shapes in CANVASES.items():
        for tag, sizes in size_sets(H, W).items():
            key = f"c{H}x{W}.{tag}."
            N = len(sizes)
            mask = torch.ones(N, H, W, dtype=torch.bool)
            for n, (h, w) in enumerate(sizes):
                mask[n, :h, :w] = False
            masks = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in shapes]
            spatial = torch.tensor(shapes, dtype=torch.int64)
            valid_ratios = torch.stack([get_valid_ratio(None, m) for m in masks], 1)
            ref = get_reference_points(spatial, valid_ratios, "cpu")
            pos = torch.cat([position(types.SimpleNamespace(tensors=torch.zeros(N, 1, *m.shape[1:]), mask=m)).permute(0, 2, 3, 1).flatten(1, 2)
                             for m in masks], 1)
            mask_flat = torch.cat([m.flatten(1) for m in masks], 1)
            memory, prop = gen_proposals(torch.ones(N, mask_flat.shape[1], 1), mask_flat, spatial)
            assert valid_ratios.dtype == ref.dtype == pos.dtype == prop.dtype == torch.float32
            out.update({key + "sizes": np.asarray(sizes, dtype=np.int32), key + "canvas": np.asarray((H, W), dtype=np.int32),
                        key + "shapes": np.asarray(shapes, dtype=np.int32), key + "valid_ratios": valid_ratios.numpy(), key + "ref": ref.numpy(),
                        key + "pos_sine": pos.numpy(), key + "proposals": prop.numpy(), key + "zeroed": (memory[..., 0] == 0).numpy()})
            out.update({f"{key}mask{l}": m.numpy() for l, m in enumerate(masks)})
    path = os.path.join(OUT, "geometry", "geometry_reference.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(out), "arrays")


if __name__ == "__main__":
    main()
