#!/usr/bin/env python3
"""Golden vectors for the criterion over capacity buffers WITH the federated loss and class-agnostic two-stage targets
(richsem_amd/criterion.py ``device_set_criterion``; ``msda_fed_class_mask_slots_f32``, ``msda_criterion_pairs_ex_f32``), generated from the
REFERENCE's own ``SetCriterion``.  Run in the build container only (it reads /root/reference; the fixture is committed):

    python tests/golden/make_golden_criterion_fed_capacity.py

It drives the reference exactly as make_golden_criterion_capacity.py does -- the same pieces cut out of ``models/richsem/richsem.py`` with
``ast`` and executed as they stand, the same restated order of ``forward``'s get_loss calls; its helpers are imported from that file -- with
``use_fed_loss=True``, ``fed_num_sample_cats=50`` and a ``fed_weight``.  ``loss_labels``' own ``from .fed_loss import get_fed_loss_inds``
resolves to a module that RECORDS what the reference's function (models/richsem/fed_loss.py, loaded by path) is given and returns, in the
pattern of make_golden_distill.py: per call the ``fed_ids`` and ``unique(target_classes_o)``.  With ``enc_cls_agn`` the two-stage call gets
the reference's ``enc_targets`` (richsem.py:1249-1255: every label 0), restated here.

Cases: counts (0, 5, 2), (1, 0, 0), (0, 0, 0) x dn_number 3 / 100 x enc_cls_agn off / on; nl = 2, N = 3, Q = 10, Qi = 13, C = 70.  The class
weight is image_count ** 0.5 with image counts 0 at classes 0 and 17; the first two labels of a batch with at least two targets are 17 and
0, so a zero-weight class that appears stays in the subset, and one that does not appear is never drawn.  ``get_fed_loss_inds`` draws with
the global RNG: it is seeded per case, the same for enc_cls_agn off and on -- the two-stage call is the last one, so the two differ in
that call only, and the enc_cls_agn case stores only what differs (fed_ids, appeared, per_call, loss, grad_il, grad_ib; the generator asserts
that the rest is equal).  A call the reference does not make (the denoising part of a batch without targets, see
make_golden_criterion_capacity.py) has fed_ids / appeared rows of -1.
The denoising logits lie on a grid of 0.5 (the matching and two-stage logits are float16-exact normal draws as before): with dn_number 100
there are 200 denoising rows per image and layer, and their float32 gradients on arbitrary logits would take the fixture past the size a
committed file may have; values on a grid repeat, so the file compresses.
Checked while generating, and printed: every call has fewer than 50 appeared classes and at least 50 eligible ones -- torch.multinomial
would raise otherwise, and the fixture must not depend on that path.
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
sys.path.insert(0, OUT)
import make_golden_criterion_capacity as base      # noqa: E402

NL, N, Q, C, QI = 2, 3, 10, 70, 13
NUM_SAMPLE = 50
CASES = [(counts, dn, agn) for counts in ((0, 5, 2), (1, 0, 0), (0, 0, 0)) for dn in (3, 100) for agn in (0, 1)]
W_CE, W_BBOX, W_GIOU = 1.0, 5.0, 2.0


def class_weight():
    counts = (torch.arange(C) * 7) % 23 + 1
    counts[0] = counts[17] = 0
    return counts ** 0.5      # (set_cats: an int64 tensor ** 0.5 -> float32)


def reference_criterion():
    """-> (a stand-in SetCriterion with the reference's methods and use_fed_loss, forward's denoising index block, the record of the draws)"""
    path = f"{REF}/models/richsem/richsem.py"
    spec = importlib.util.spec_from_file_location("_ref_fed_loss", f"{REF}/models/richsem/fed_loss.py")
    fed = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fed)
    drawn = []

    def recording(gt_classes, *a, **kw):
        ids = fed.get_fed_loss_inds(gt_classes, *a, **kw)
        drawn.append((torch.unique(gt_classes), ids))
        return ids

    pkg = types.ModuleType("_ref_richsem")
    pkg.__path__ = []
    sub = types.ModuleType("_ref_richsem.fed_loss")
    sub.get_fed_loss_inds = recording
    sys.modules["_ref_richsem"], sys.modules["_ref_richsem.fed_loss"] = pkg, sub
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "SetCriterion")
    want = ["loss_labels", "loss_boxes", "_get_src_permutation_idx", "prep_for_dn", "get_loss"]
    methods = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(methods) == len(want)
    ns = {"torch": torch, "F": F, "box_ops": base.reference_box_ops(), "sigmoid_focal_loss": base.reference_utils().sigmoid_focal_loss,
          "__name__": "_ref_richsem.richsem", "__package__": "_ref_richsem"}
    exec(compile(ast.Module(body=methods, type_ignores=[]), path, "exec"), ns)
    attrs = {m.name: ns[m.name] for m in methods}
    attrs.update(loss_cardinality=None, loss_masks=None)
    crit = type("SetCriterionPieces", (), attrs)()
    crit.num_classes, crit.focal_alpha, crit.use_fed_loss, crit.fed_num_sample_cats, crit.fed_weight = C, 0.25, True, NUM_SAMPLE, class_weight()
    forward = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "forward")
    block = next(n for n in ast.walk(forward) if isinstance(n, ast.If) and "output_known_lbs_bboxes" in ast.unparse(n.test))
    stop = next(i for i, s in enumerate(block.body) if isinstance(s, ast.For))
    body = [base._DropCuda().visit(s) for s in block.body[:stop + 1]]
    mod = ast.fix_missing_locations(ast.Module(body=body, type_ignores=[]))
    return crit, compile(mod, path, "exec"), drawn


def main():
    from richsem_amd.dn import dn_group_count
    crit, dn_block, drawn = reference_criterion()
    weight = crit.fed_weight
    eligible_all = int((weight > 0).sum())
    out = {"dims": np.array([NL, N, Q, C, QI]), "weights": np.array([W_CE, W_BBOX, W_GIOU]), "num_sample_cats": np.int64(NUM_SAMPLE),
           "class_weight": weight.numpy().astype(np.float32), "cases": np.array([list(c) + [d, a] for c, d, a in CASES])}
    f16exact, f32exact = base.f16exact, base.f32exact
    kept = None      # the enc_cls_agn = 0 twin's arrays
    for ci, (counts, dn_number, agn) in enumerate(CASES):
        g = torch.Generator().manual_seed(900 + ci // 2)      # (the twins share everything but the two-stage call's labels)
        total = sum(counts)
        targets = []
        for tb in counts:
            cxcy, wh = torch.rand(tb, 2, generator=g) * 0.6 + 0.2, torch.rand(tb, 2, generator=g) * 0.3 + 0.05
            targets.append({"labels": torch.randint(1, C, (tb,), generator=g), "boxes": f32exact(torch.cat((cxcy, wh), 1))})
        if total >= 2:
            first = next(t for t in targets if len(t["labels"]) >= 2)
            first["labels"][0], first["labels"][1] = 17, 0
        enc_targets = [{"labels": torch.zeros_like(t["labels"]), "boxes": t["boxes"]} for t in targets] if agn else targets
        groups = dn_group_count(dn_number, list(counts))
        pad_size = 2 * max(counts) * groups

        def boxes_like(*shape):
            return f32exact(torch.cat((torch.rand(*shape, 2, generator=g) * 0.6 + 0.2, torch.rand(*shape, 2, generator=g) * 0.4 + 0.03), -1))
        leaves = {"logits": f16exact(torch.randn(NL, N, Q, C, generator=g) * 3), "coords": boxes_like(NL, N, Q),
                  "dn_logits": torch.round(torch.randn(NL, N, pad_size, C, generator=g) * 6).double() / 2, "dn_coords": boxes_like(NL, N, pad_size),
                  "il": f16exact(torch.randn(N, QI, C, generator=g) * 3), "ib": boxes_like(N, QI)}
        leaves["logits"][0, 1, 0, :4] = torch.tensor([24.0, -24.0, 20.5, 0.0], dtype=torch.float64)      # softplus's branches
        leaves = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
        indices, qot = [], torch.full((NL + 1, max(total, 1)), -1, dtype=torch.int64)
        for o in range(NL + 1):
            nq, per_image, at = (QI if o == NL else Q), [], 0
            for tb in counts:
                src = torch.randperm(nq, generator=g)[:tb]
                order = torch.argsort(src)
                per_image.append((src[order], torch.arange(tb)[order]))
                qot[o, at: at + tb] = src
                at += tb
            indices.append(per_image)
        num_boxes = max(float(sum(len(t[1]) for t in indices[NL - 1])), 1.0)
        ns = {"self": crit, "torch": torch, "targets": targets, "range": range, "len": len,
              "dn_meta": {"output_known_lbs_bboxes": None, "num_dn_group": groups, "pad_size": pad_size}}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exec(dn_block, ns)
        dn_pos_idx, scalar = ns["dn_pos_idx"], ns["scalar"]
        assert scalar == groups
        losses, draws = {}, {}
        torch.manual_seed(4000 + ci // 2)      # (get_fed_loss_inds draws with the global RNG)

        def call(outputs, idx, nb, suffix, tg):
            if outputs["pred_logits"].shape[1] == 0:      # pad_size 0: the call is not made (make_golden_criterion_capacity.py)
                z = torch.zeros((), dtype=torch.float64)
                losses.update({f"loss_ce{suffix}": z, f"loss_bbox{suffix}": z, f"loss_giou{suffix}": z})
                return
            n0 = len(drawn)
            d = dict(crit.get_loss("labels", outputs, tg, idx, nb, log=False))
            assert len(drawn) == n0 + 1
            draws[suffix] = drawn[-1]
            d.update(crit.get_loss("boxes", outputs, tg, idx, nb))
            losses.update({k + suffix: v for k, v in d.items()})

        def layer(l):
            return ({"pred_logits": leaves["logits"][l], "pred_boxes": leaves["coords"][l]},
                    {"pred_logits": leaves["dn_logits"][l], "pred_boxes": leaves["dn_coords"][l]})
        main_out, main_dn = layer(NL - 1)
        call(main_dn, dn_pos_idx, num_boxes * scalar, "_dn", targets)
        call(main_out, indices[NL - 1], num_boxes, "", targets)
        for l in range(NL - 1):
            aux, aux_dn = layer(l)
            call(aux, indices[l], num_boxes, f"_{l}", targets)
            call(aux_dn, dn_pos_idx, num_boxes * scalar, f"_dn_{l}", targets)
        call({"pred_logits": leaves["il"], "pred_boxes": leaves["ib"]}, indices[NL], num_boxes, "_interm", enc_targets)
        sfx = [f"_{l}" for l in range(NL - 1)] + [""] + [f"_dn_{l}" for l in range(NL - 1)] + ["_dn", "_interm"]
        per_call = torch.stack([torch.stack([losses[f"loss_ce{s}"], losses[f"loss_bbox{s}"], losses[f"loss_giou{s}"]]) for s in sfx])
        total_loss = (per_call * torch.tensor([W_CE, W_BBOX, W_GIOU], dtype=torch.float64)).sum()
        total_loss.backward()
        fed_ids = np.full((2 * NL + 1, NUM_SAMPLE), -1, dtype=np.int64)
        appeared = np.full((2 * NL + 1, NUM_SAMPLE), -1, dtype=np.int64)
        for k, s in enumerate(sfx):
            if s not in draws:
                continue
            app, ids = draws[s]
            n_app, n_elig = len(app), eligible_all - int((weight[app] > 0).sum())
            print(f"  call {s or '(main)':8s} appeared {n_app} eligible {n_elig} fed_ids {len(ids)}")
            assert n_app < NUM_SAMPLE and n_elig >= NUM_SAMPLE and len(ids) == NUM_SAMPLE
            fed_ids[k], appeared[k, :n_app] = ids.numpy(), app.numpy()
        p = f"c{ci}."
        arrays = {"counts": np.array(counts), "dn_number": np.int64(dn_number), "groups": np.int64(groups), "pad_size": np.int64(pad_size),
                  "num_boxes": np.float64(num_boxes), "labels": torch.cat([t["labels"] for t in targets]).numpy(),
                  "boxes": torch.cat([t["boxes"] for t in targets]).float().numpy().reshape(-1, 4), "qot": qot[:, :total].numpy()}
        for k, v in leaves.items():
            arrays[k] = v.detach().numpy().astype(np.float16 if "logits" in k or k == "il" else np.float32)
            grad = v.grad if v.grad is not None else torch.zeros_like(v)
            arrays["grad_" + k] = grad.numpy().astype(np.float32)
        arrays.update(fed_ids=fed_ids, appeared=appeared, per_call=per_call.detach().numpy(), loss=total_loss.detach().numpy(), keys=np.array(sfx))
        own = ("fed_ids", "appeared", "per_call", "loss", "grad_il", "grad_ib")
        if agn:
            for k, v in arrays.items():
                if k not in own:
                    assert np.array_equal(v, kept[k]), k
            for k in ("fed_ids", "appeared", "per_call"):      # only the two-stage call differs
                assert np.array_equal(arrays[k][:-1], kept[k][:-1]), k
            arrays = {k: arrays[k] for k in own}
            if total:
                assert appeared[-1, 0] == 0 and appeared[-1, 1] == -1
        else:
            kept = arrays
        out.update({p + k: v for k, v in arrays.items()})
        print(counts, dn_number, "agn", agn, "groups", groups, "pad", pad_size, "num_boxes", num_boxes, "loss", float(total_loss))
    path = os.path.join(OUT, "criterion_fed_capacity_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
