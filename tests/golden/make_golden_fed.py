#!/usr/bin/env python3
"""Golden vectors for the federated loss (richsem_amd/fed_loss.py: FedClassSampler + MaskedFocalNegativeSum; ``msda_fed_class_mask_f32``,
``msda_focal_neg_{sum,grad}_masked_f32``), generated from the REFERENCE's own functions.  Run in the build container only (it reads
/root/reference; the fixture is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_fed.py

What is executed is the reference's code, loaded by path (both files need torch / numpy / json only):
  * ``get_fed_loss_inds`` of ``models/richsem/fed_loss.py:15-25`` on seeded class targets, with LVIS-shaped weights for C = 1204:
    ``SetCriterion.set_cats`` (richsem.py:930-936) restated -- ``[cats.get(x, {'image_count': 0})['image_count'] for x in range(max_cid +
    1)] ** 0.5`` -- on a seeded long-tail ``cats`` without id 0 and without a few other ids (weight 0);
  * ``sigmoid_focal_loss`` of ``models/richsem/utils.py:82-108`` called as ``loss_labels`` calls it with use_fed_loss (richsem.py:956-961):
    ``sigmoid_focal_loss(src_logits[..., fed_ids], onehot[..., fed_ids], num_boxes) * src_logits.shape[1]``, for a matching-part shaped and
    a denoising-part shaped output, in float64 on float32-exact logits, gradients by autograd.
Three cases: fewer than 50 appeared classes (the draw tops them up), at least 50 (no draw), no targets at all (50 drawn, num_boxes 1).
Only the fed columns of the logits and of the gradient are stored (the loss does not depend on the others: the test fills them with values
of its own, and the gradient there is 0).  The file is named criterion_fed_reference.npz: tests/conftest.py takes every fixture whose name
does not start with another row's prefix ("criterion_" is the criterion's) for an operator case.
"""
import importlib.util
import os

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
C = 1204


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, f"{REF}/{rel}")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main():
    fed, utils = load("_ref_fed_loss", "models/richsem/fed_loss.py"), load("_ref_utils", "models/richsem/utils.py")
    g = torch.Generator().manual_seed(1204)
    # LVIS-like categories: ids 1..1203, long-tailed image counts, a few ids absent
    absent = {17, 400, 401, 1203}
    counts = (20000.0 / torch.arange(1, C, dtype=torch.float64) ** 1.1)[torch.randperm(C - 1, generator=g)].long() + 1
    cats = {c: {"id": c, "image_count": int(counts[c - 1])} for c in range(1, C) if c not in absent}
    max_cid = max(cats)
    fed_weight = torch.tensor([cats.get(x, {"image_count": 0})["image_count"] for x in range(max_cid + 1)]) ** 0.5      # set_cats
    fed_weight = torch.cat((fed_weight, fed_weight.new_zeros(C - fed_weight.numel())))      # (max_cid < C - 1: the absent tail is weight 0)
    out = {"cats.ids": np.array(sorted(cats), dtype=np.int64), "cats.image_count": np.array([cats[c]["image_count"] for c in sorted(cats)]),
           "fed_weight": fed_weight.float().numpy()}
    present = torch.tensor(sorted(cats))
    for case, seed, per_img in (("few", 31, 9), ("many", 32, 40), ("empty", 33, 0)):
        for part, N, Q, norm_mult in (("match", 2, 60, 1.0), ("dn", 2, 40, 10.0)):
            g = torch.Generator().manual_seed(seed * 10 + (part == "dn"))
            torch.manual_seed(seed * 10 + (part == "dn"))      # (get_fed_loss_inds draws with the global RNG: torch.multinomial)
            labels = [present[torch.randint(0, present.numel(), (per_img,), generator=g)] for _ in range(N)]
            if per_img:
                labels[1][:3] = labels[0][:3]                       # repeats across images
            target_classes = torch.full((N, Q), C, dtype=torch.int64)
            for b in range(N):
                q = torch.randperm(Q, generator=g)[:per_img]
                target_classes[b, q] = labels[b]
            target_classes_o = torch.cat(labels)
            num_boxes = max(float(target_classes_o.numel()), 1.0) * norm_mult
            fed_ids = fed.get_fed_loss_inds(target_classes_o, 50, C, fed_weight)
            logits = (torch.randn(N, Q, C, generator=g) * 4).float().double()
            logits[0, 0, fed_ids[:3]] = torch.tensor([25.0, -25.0, 19.999], dtype=torch.float64)   # softplus's branches
            x = logits.clone().requires_grad_(True)
            onehot = torch.zeros((N, Q, C + 1), dtype=x.dtype)
            onehot.scatter_(2, target_classes.unsqueeze(-1), 1)
            onehot = onehot[:, :, :-1]
            loss = utils.sigmoid_focal_loss(x[..., fed_ids], onehot[..., fed_ids], num_boxes, alpha=0.25, gamma=2) * Q
            loss.backward()
            key = f"{case}_{part}"
            out[f"{key}.labels"] = target_classes_o.numpy()
            out[f"{key}.fed_ids"] = fed_ids.numpy()
            out[f"{key}.logits_fed"] = logits[..., fed_ids].float().numpy()
            out[f"{key}.target_classes"] = target_classes.numpy()
            out[f"{key}.num_boxes"] = np.float64(num_boxes)
            out[f"{key}.loss"] = loss.detach().numpy()
            out[f"{key}.grad_fed"] = x.grad[..., fed_ids].float().numpy()
            print(key, "appeared", int(torch.unique(target_classes_o).numel()), "fed", fed_ids.numel(), "loss", float(loss.detach()))
    np.savez_compressed(os.path.join(OUT, "criterion_fed_reference.npz"), **out)
    print(os.path.getsize(os.path.join(OUT, "criterion_fed_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
