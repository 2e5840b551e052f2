#!/usr/bin/env python3
"""Golden vectors for the criterion over capacity buffers (``msda_criterion_pairs_f32``; richsem_amd/criterion.py ``device_criterion``),
generated from the REFERENCE's own ``SetCriterion``.  Run in the build container only (it reads /root/reference; the fixture is committed, the
GPU box never sees the reference):

    python tests/golden/make_golden_criterion_capacity.py

``models/richsem/richsem.py`` does not import here (torchvision and the compiled ops are absent), so the pieces are cut out of its source
with ``ast`` and executed as they stand:
  * from ``SetCriterion``: ``loss_labels`` (its non-federated branch runs: ``use_fed_loss`` False, no ``pred_hs``, ``log=False``),
    ``loss_boxes``, ``_get_src_permutation_idx``, ``prep_for_dn``, ``get_loss`` -- as methods of a stand-in class that carries the three
    attributes they read (``num_classes``, ``focal_alpha``, ``use_fed_loss``);
  * from ``SetCriterion.forward``: the denoising index block (the statements from ``prep_for_dn`` to the end of the loop that fills
    ``dn_pos_idx``), with ONE change: the ``.cuda()`` calls are taken out of the syntax tree (there is no GPU here);
  * ``sigmoid_focal_loss`` of ``models/richsem/utils.py`` (loaded by path) and ``box_cxcywh_to_xyxy`` / ``box_iou`` /
    ``generalized_box_iou`` of ``util/box_ops.py`` (cut out; ``torchvision.ops.boxes.box_area`` is restated from its published definition,
    as in make_golden_criterion.py).
What is restated here, not executed: the ORDER of ``forward``'s get_loss calls and their key suffixes (last decoder output, its denoising
part, the auxiliary outputs 0..nl-2 each followed by its denoising part, the two-stage output; ``num_boxes`` = the last decoder output's
matched pairs clamped to 1; the denoising calls take ``num_boxes * num_dn_group``), and ``prepare_for_cdn``'s integer layout
(``pad_size = 2 * max count * groups``, groups by richsem_amd.dn.dn_group_count, the host mirror the dn tests hold to the reference).  A
batch without any target has ``pad_size`` 0: the reference's focal loss then takes the mean over an empty dimension (NaN); the fixture
stores zeros for those denoising calls, which is what the reference's own branch without a denoising part stores.
A stub matcher returns prescribed indices, stored in the fixture as ``qot`` (query of target, one row per output).
Everything runs in float64 on inputs that are exactly representable in float16 (logits) / float32 (boxes); gradients by autograd.
The weighted total uses loss_ce 1, loss_bbox 5, loss_giou 2 for every call.
"""
import ast
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

NL, N, Q, C, QI = 2, 3, 10, 37, 13
CASES = [((0, 5, 2), 3), ((0, 5, 2), 100), ((1, 0, 0), 3), ((1, 0, 0), 100), ((0, 0, 0), 3), ((0, 0, 0), 100)]
W_CE, W_BBOX, W_GIOU = 1.0, 5.0, 2.0


def box_area(boxes):      # torchvision.ops.boxes.box_area (published definition; torchvision is absent from the image)
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def reference_box_ops():
    names = ["box_cxcywh_to_xyxy", "box_iou", "generalized_box_iou"]
    path = f"{REF}/util/box_ops.py"
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names)
    ns = {"torch": torch, "box_area": box_area}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return types.SimpleNamespace(**{k: ns[k] for k in names})


def reference_utils():
    spec = importlib.util.spec_from_file_location("_ref_utils", f"{REF}/models/richsem/utils.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _DropCuda(ast.NodeTransformer):
    """x.cuda() -> x"""

    def visit_Call(self, node):
        self.generic_visit(node)
        if isinstance(node.func, ast.Attribute) and node.func.attr == "cuda" and not node.args and not node.keywords:
            return node.func.value
        return node


def reference_criterion():
    """-> (a stand-in SetCriterion with the reference's methods, the code object of forward's denoising index block)"""
    path = f"{REF}/models/richsem/richsem.py"
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SetCriterion")
    want = ["loss_labels", "loss_boxes", "_get_src_permutation_idx", "prep_for_dn", "get_loss"]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(methods) == len(want)
    # (get_loss builds a table of all four losses: the two that are not cut out get a None stand-in below)
    ns = {"torch": torch, "F": F, "box_ops": reference_box_ops(), "sigmoid_focal_loss": reference_utils().sigmoid_focal_loss}
    exec(compile(ast.Module(body=methods, type_ignores=[]), path, "exec"), ns)
    attrs = {m.name: ns[m.name] for m in methods}
    attrs.update(loss_cardinality=None, loss_masks=None)
    crit = type("SetCriterionPieces", (), attrs)()
    crit.num_classes, crit.focal_alpha, crit.use_fed_loss = C, 0.25, False
    forward = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    block = next(n for n in ast.walk(forward) if isinstance(n, ast.If) and "output_known_lbs_bboxes" in ast.unparse(n.test))
    stop = next(i for i, s in enumerate(block.body) if isinstance(s, ast.For))
    body = [_DropCuda().visit(s) for s in block.body[:stop + 1]]
    assert "prep_for_dn" in ast.unparse(body[0]) and "dn_pos_idx" in ast.unparse(body[-1])
    mod = ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))
    return crit, compile(mod, path, "exec")


def f16exact(t):
    return t.half().double()


def f32exact(t):
    return t.float().double()


def main():
    from richsem_amd.dn import dn_group_count
    crit, dn_block = reference_criterion()
    out = {"dims": np.array([NL, N, Q, C, QI]), "weights": np.array([W_CE, W_BBOX, W_GIOU]),
           "cases": np.array([list(c) + [d] for c, d in CASES])}
    for ci, (counts, dn_number) in enumerate(CASES):
        g = torch.Generator().manual_seed(700 + ci)
        total = sum(counts)
        targets = []
        for tb in counts:
            cxcy, wh = torch.rand(tb, 2, generator=g) * 0.6 + 0.2, torch.rand(tb, 2, generator=g) * 0.3 + 0.05
            targets.append({"labels": torch.randint(0, C, (tb,), generator=g), "boxes": f32exact(torch.cat((cxcy, wh), 1))})
        groups = dn_group_count(dn_number, list(counts))
        pad_size = 2 * max(counts) * groups

        def boxes_like(*shape):
            return f32exact(torch.cat((torch.rand(*shape, 2, generator=g) * 0.6 + 0.2, torch.rand(*shape, 2, generator=g) * 0.4 + 0.03), -1))
        leaves = {"logits": f16exact(torch.randn(NL, N, Q, C, generator=g) * 3), "coords": boxes_like(NL, N, Q),
                  "dn_logits": f16exact(torch.randn(NL, N, pad_size, C, generator=g) * 3), "dn_coords": boxes_like(NL, N, pad_size),
                  "il": f16exact(torch.randn(N, QI, C, generator=g) * 3), "ib": boxes_like(N, QI)}
        leaves["logits"][0, 1, 0, :4] = torch.tensor([24.0, -24.0, 20.5, 0.0], dtype=torch.float64)      # softplus's branches
        leaves = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
        # ---- the stub matcher's result: per output and image, T_b distinct queries in a random order against the targets in order -------
        indices, qot = [], torch.full((NL + 1, max(total, 1)), -1, dtype=torch.int64)
        for o in range(NL + 1):
            nq, per_image, at = (QI if o == NL else Q), [], 0
            for tb in counts:
                src = torch.randperm(nq, generator=g)[:tb]
                order = torch.argsort(src)      # (the matcher returns its pairs in query order)
                per_image.append((src[order], torch.arange(tb)[order]))
                qot[o, at: at + tb] = src
                at += tb
            indices.append(per_image)
        # ---- SetCriterion.forward's sequence of get_loss calls (order and key suffixes: see the docstring) --------------------------------
        num_boxes = max(float(sum(len(t[1]) for t in indices[NL - 1])), 1.0)
        ns = {"self": crit, "torch": torch, "targets": targets, "range": range, "len": len,
              "dn_meta": {"output_known_lbs_bboxes": None, "num_dn_group": groups, "pad_size": pad_size}}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (torch.range is deprecated)
            exec(dn_block, ns)
        dn_pos_idx, scalar = ns["dn_pos_idx"], ns["scalar"]
        assert scalar == groups and (pad_size == 0 or ns["single_pad"] == pad_size // groups)
        losses = {}

        def call(outputs, idx, nb, suffix):
            if outputs["pred_logits"].shape[1] == 0:      # pad_size 0 (see the docstring)
                z = torch.zeros((), dtype=torch.float64)
                losses.update({f"loss_ce{suffix}": z, f"loss_bbox{suffix}": z, f"loss_giou{suffix}": z})
                return
            d = dict(crit.get_loss("labels", outputs, targets, idx, nb, log=False))
            d.update(crit.get_loss("boxes", outputs, targets, idx, nb))
            losses.update({k + suffix: v for k, v in d.items()})

        def layer(l):
            return ({"pred_logits": leaves["logits"][l], "pred_boxes": leaves["coords"][l]},
                    {"pred_logits": leaves["dn_logits"][l], "pred_boxes": leaves["dn_coords"][l]})
        main_out, main_dn = layer(NL - 1)
        call(main_dn, dn_pos_idx, num_boxes * scalar, "_dn")
        call(main_out, indices[NL - 1], num_boxes, "")
        for l in range(NL - 1):
            aux, aux_dn = layer(l)
            call(aux, indices[l], num_boxes, f"_{l}")
            call(aux_dn, dn_pos_idx, num_boxes * scalar, f"_dn_{l}")
        call({"pred_logits": leaves["il"], "pred_boxes": leaves["ib"]}, indices[NL], num_boxes, "_interm")
        # the 2 nl + 1 calls in the order of `terms`: matching parts of layers 0..nl-1, their denoising parts, the two-stage output
        sfx = [f"_{l}" for l in range(NL - 1)] + [""] + [f"_dn_{l}" for l in range(NL - 1)] + ["_dn", "_interm"]
        per_call = torch.stack([torch.stack([losses[f"loss_ce{s}"], losses[f"loss_bbox{s}"], losses[f"loss_giou{s}"]]) for s in sfx])
        total_loss = (per_call * torch.tensor([W_CE, W_BBOX, W_GIOU], dtype=torch.float64)).sum()
        assert sorted(k for k in losses if k.split("_")[1] in ("ce", "bbox", "giou")) == sorted(f"loss_{n}{s}" for s in sfx for n in ("ce", "bbox", "giou"))
        total_loss.backward()
        p = f"c{ci}."
        out[p + "counts"], out[p + "dn_number"] = np.array(counts), np.int64(dn_number)
        out[p + "groups"], out[p + "pad_size"], out[p + "num_boxes"] = np.int64(groups), np.int64(pad_size), np.float64(num_boxes)
        out[p + "labels"] = torch.cat([t["labels"] for t in targets]).numpy()
        out[p + "boxes"] = torch.cat([t["boxes"] for t in targets]).float().numpy().reshape(-1, 4)
        out[p + "qot"] = qot[:, :total].numpy()
        for k, v in leaves.items():
            out[p + k] = v.detach().numpy().astype(np.float16 if "logits" in k or k == "il" else np.float32)
            grad = v.grad if v.grad is not None else torch.zeros_like(v)
            out[p + "grad_" + k] = grad.numpy().astype(np.float32)
        out[p + "per_call"], out[p + "loss"] = per_call.detach().numpy(), total_loss.detach().numpy()
        out[p + "keys"] = np.array(sfx)
        print(counts, dn_number, "groups", groups, "pad", pad_size, "num_boxes", num_boxes, "loss", float(total_loss))
    path = os.path.join(OUT, "criterion_capacity_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
