#!/usr/bin/env python3
"""Golden vectors for the criterion's mask terms and the mask post-processor (``msda_mask_*``; richsem_amd/masks.py), generated from the
REFERENCE's own code.  Run in the build container only (it reads /root/reference; the fixture is committed, the GPU box never sees the
reference):

    python tests/golden/make_golden_mask_terms.py

``models/richsem/richsem.py``, ``models/richsem/segmentation.py`` and ``util/misc.py`` do not import here (torchvision and the compiled ops are
absent), so the pieces are cut out of their source with ``ast`` and executed as they stand:
  * from ``SetCriterion``: ``loss_masks``, ``_get_src_permutation_idx``, ``_get_tgt_permutation_idx`` -- as methods of a stand-in class;
  * ``dice_loss`` of ``models/richsem/segmentation.py`` and ``sigmoid_focal_loss`` of ``models/richsem/utils.py`` (the two richsem.py
    imports; utils.py is loaded by path);
  * ``_max_by_axis``, ``NestedTensor``, ``nested_tensor_from_tensor_list`` and ``interpolate`` of ``util/misc.py``; ``interpolate`` runs with
    its compatibility flag False, i.e. its torchvision branch, and ``torchvision.ops.misc.interpolate`` is ``F.interpolate`` (what
    torchvision's function forwards to for a non-empty input);
  * from ``PostProcessSegm``: ``forward``, called on a stand-in ``self`` with ``threshold`` and ``processor_dct``.
Nothing of their text is copied.  A stub matcher supplies prescribed indices, stored as ``qot`` (query of target per slot, -1: the target is
not matched).  Everything runs in float64 on logits that are exactly representable in bfloat16; the gradient is autograd's, of
``g[0] * loss_mask + g[1] * loss_dice``.

The fixture, tests/golden/mask_terms/mask_terms_reference.npz (a directory of its own: every .npz directly under tests/golden is taken for an
operator fixture by the suite's collection): ``loss_cases`` / ``post_cases`` the case names; per loss case ``<name>/pred`` (N, Q, h, w),
``<name>/counts`` (N), ``<name>/mask_hw`` (N, 2) the images' own mask sizes, ``<name>/canvas`` the reference's padded size,
``<name>/masks`` uint8 (sum counts, Hp, Wp) the padded targets in slot order, ``<name>/qot``, ``<name>/num_boxes``, ``<name>/g`` and the
results ``<name>/loss_mask``, ``<name>/loss_dice``, ``<name>/grad``; per post-process case ``<name>/pred``, ``<name>/max_sizes``,
``<name>/orig_sizes``, ``<name>/threshold``, ``<name>/items`` with ``<name>/item_counts`` (absent: no ``item_indices``) and the results
``<name>/out<i>`` uint8 (rows, 1, oh, ow).
"""
import ast
import importlib.util
import os
import sys
import types
from typing import List, Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))

# name -> ((h, w), Q, per image (count, (H_b, W_b)), qot per slot)
LOSS_CASES = {
    "s1x1": ((1, 1), 3, [(2, (20, 32)), (1, (32, 17))], [2, 0, 1]),
    "s8x8_empty_image": ((8, 8), 3, [(0, (20, 30)), (2, (31, 17))], [1, 2]),
    "s7x10_unmatched": ((7, 10), 4, [(2, (30, 60)), (2, (64, 40))], [3, 0, -1, 2]),
    "s5x3": ((5, 3), 3, [(1, (30, 60)), (2, (20, 96))], [1, 2, 0]),
    "s40x40_down": ((40, 40), 2, [(1, (30, 20)), (1, (25, 31))], [1, 0]),
    "s9x13_inside": ((9, 13), 3, [(2, (40, 52)), (1, (60, 90))], [0, 2, 1]),
    "no_pair": ((8, 8), 3, [(0, (20, 32)), (0, (32, 17))], []),
}
# name -> ((h, w), Q, max sizes, orig sizes, item_indices or None, threshold)
POST_CASES = {
    "p9x13": ((9, 13), 4, [(40, 60), (30, 45)], [(75, 101), (17, 23)], None, 0.5),
    "p7x10_items": ((7, 10), 5, [(28, 33), (20, 40)], [(56, 66), (20, 40)], [[3, 0, 3], [1]], 0.5),
    "p1x1": ((1, 1), 3, [(3, 4)], [(9, 7)], None, 0.3),
}


def _functions(path, names, ns, classes=()):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name in names) or (isinstance(n, ast.ClassDef) and n.name in classes)]
    assert len(body) == len(names) + len(classes), (path, [n.name for n in body])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def _methods(path, cls_name, names, ns):
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), (cls_name, [n.name for n in body])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return {n: ns[n] for n in names}


def reference_misc():
    tv = types.SimpleNamespace(ops=types.SimpleNamespace(misc=types.SimpleNamespace(interpolate=F.interpolate)))
    ns = {"torch": torch, "Tensor": Tensor, "List": List, "Optional": Optional, "torchvision": tv, "__torchvision_need_compat_flag": False}
    return _functions(f"{REF}/util/misc.py", ["_max_by_axis", "nested_tensor_from_tensor_list", "interpolate"], ns, classes=["NestedTensor"])


def reference_utils():
    spec = importlib.util.spec_from_file_location("_ref_utils", f"{REF}/models/richsem/utils.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_pieces():
    misc = reference_misc()
    seg = f"{REF}/models/richsem/segmentation.py"
    dice = _functions(seg, ["dice_loss"], {"torch": torch, "F": F})["dice_loss"]
    ns = {"torch": torch, "F": F, "nested_tensor_from_tensor_list": misc["nested_tensor_from_tensor_list"], "interpolate": misc["interpolate"],
          "sigmoid_focal_loss": reference_utils().sigmoid_focal_loss, "dice_loss": dice}
    crit = type("SetCriterionPieces", (), _methods(f"{REF}/models/richsem/richsem.py", "SetCriterion",
                                                   ["loss_masks", "_get_src_permutation_idx", "_get_tgt_permutation_idx"], ns))()
    post = _methods(seg, "PostProcessSegm", ["forward"], {"torch": torch, "F": F, "nn": nn})["forward"]
    return crit, post


def bf16exact(t):
    return t.bfloat16().double()


def loss_case(crit, gen, hw, Q, images, qot):
    (h, w), N = hw, len(images)
    pred = bf16exact(torch.randn(N, Q, h, w, generator=gen) * 3).requires_grad_(True)
    targets = [{"masks": torch.rand(c, H, W, generator=gen) < 0.4} for c, (H, W) in images]
    indices, slot = [], 0
    for c, _ in images:      # the stub matcher: (queries, targets) per image, matched targets only
        tgt = [j for j in range(c) if qot[slot + j] >= 0]
        indices.append((torch.tensor([qot[slot + j] for j in tgt], dtype=torch.int64), torch.tensor(tgt, dtype=torch.int64)))
        slot += c
    num_boxes = float(max(sum(len(i) for i, _ in indices), 1))
    g = torch.tensor([0.75, 1.5], dtype=torch.float64)
    Hp, Wp = (max(H for _, (H, _) in images) + 31) // 32 * 32, (max(W for _, (_, W) in images) + 31) // 32 * 32      # (checked below)
    if sum(c for c, _ in images):
        losses = crit.loss_masks({"pred_masks": pred}, targets, indices, num_boxes)
        (g[0] * losses["loss_mask"] + g[1] * losses["loss_dice"]).backward()
        grad, lm, ld = pred.grad, losses["loss_mask"].detach(), losses["loss_dice"].detach()
        padded = crit.loss_masks.__globals__["nested_tensor_from_tensor_list"]([t["masks"] for t in targets]).tensors
        assert tuple(padded.shape[-2:]) == (Hp, Wp)
        masks = torch.cat([padded[b, :c] for b, (c, _) in enumerate(images)]).to(torch.uint8)
    else:      # no target at all: the reference's padded tensor has no channel and its sums are empty -- both losses 0, no gradient
        grad, lm, ld = torch.zeros_like(pred), torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        masks = torch.zeros((0, Hp, Wp), dtype=torch.uint8)
    return {"pred": pred.detach().numpy(), "counts": np.array([c for c, _ in images], dtype=np.int64),
            "mask_hw": np.array([s for _, s in images], dtype=np.int64), "canvas": np.array([Hp, Wp], dtype=np.int64), "masks": masks.numpy(),
            "qot": np.array(qot, dtype=np.int64), "num_boxes": np.float64(num_boxes), "g": g.numpy(), "loss_mask": lm.numpy(),
            "loss_dice": ld.numpy(), "grad": grad.numpy()}


def post_case(post, gen, hw, Q, max_sizes, orig_sizes, items, threshold):
    (h, w), N = hw, len(max_sizes)
    pred = bf16exact(torch.randn(N, Q, h, w, generator=gen) * 3)
    outputs = {"pred_masks": pred[:, :, None]}
    if items is not None:
        outputs["item_indices"] = [torch.tensor(i, dtype=torch.int64) for i in items]
    me = types.SimpleNamespace(threshold=threshold, processor_dct=None)
    results = post(me, [{} for _ in range(N)], outputs, torch.tensor(orig_sizes), torch.tensor(max_sizes))
    out = {"pred": pred.numpy(), "max_sizes": np.array(max_sizes, dtype=np.int64), "orig_sizes": np.array(orig_sizes, dtype=np.int64),
           "threshold": np.float64(threshold)}
    if items is not None:
        out["items"] = np.array([v for i in items for v in i], dtype=np.int64)
        out["item_counts"] = np.array([len(i) for i in items], dtype=np.int64)
    for i, r in enumerate(results):
        assert r["masks"].dtype == torch.uint8 and r["masks"].dim() == 4
        out[f"out{i}"] = r["masks"].numpy()
    return out


def main():
    crit, post = reference_pieces()
    gen = torch.Generator().manual_seed(20240612)
    arrays = {"loss_cases": np.array(list(LOSS_CASES)), "post_cases": np.array(list(POST_CASES))}
    for name, (hw, Q, images, qot) in LOSS_CASES.items():
        for k, v in loss_case(crit, gen, hw, Q, images, qot).items():
            arrays[f"{name}/{k}"] = v
    # the post-process logits come from a generator of their own, seeded so that no pixel of any case lies within the float32 margin of the
    # threshold (tests/mask_terms_ref.py ``postprocess``): the GPU test leaves such pixels out, and the reference alone must use none of its cap
    sys.path.insert(0, os.path.dirname(OUT))
    import mask_terms_ref as R
    gen = torch.Generator().manual_seed(20240613)
    for name, args in POST_CASES.items():
        case = post_case(post, gen, *args)
        items = None if args[4] is None else [np.array(i) for i in args[4]]
        for i, (mask, near) in enumerate(R.postprocess(case["pred"], case["max_sizes"], case["orig_sizes"], args[5], items)):
            assert (mask == case[f"out{i}"]).all() and not near.any(), (name, i, int(near.sum()))
        for k, v in case.items():
            arrays[f"{name}/{k}"] = v
    os.makedirs(os.path.join(OUT, "mask_terms"), exist_ok=True)
    path = os.path.join(OUT, "mask_terms", "mask_terms_reference.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
