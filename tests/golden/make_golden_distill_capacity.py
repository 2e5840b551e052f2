#!/usr/bin/env python3
"""Golden vectors for the distillation term over capacity buffers (richsem_amd/distill.py ``device_distill``; ``msda_distill_pairs``,
``msda_distill_scatter_*``), generated from the REFERENCE's own method.  Run in the build container only (it reads the reference tree, as
make_golden_distill.py does; the fixture is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_distill_capacity.py

What is executed: the reference's ``SetCriterion.loss_labels`` cut out with ``ast`` and bound to a stub, exactly as make_golden_distill.py
does (its ``reference_methods`` and ``Stub`` are imported), driven as ``SetCriterion.forward`` drives it (models/richsem/richsem.py:1158-1180,
:1197-1231): the matching part of a distilled layer with the matcher's (prescribed) indices and ``num_boxes``, its denoising part with the
reference's own ``dn_pos_idx`` block -- cut out of ``forward`` and executed, as make_golden_criterion_capacity.py does (its
``reference_criterion`` is imported) -- and ``num_boxes * scalar``.  ``prepare_for_cdn``'s integer layout is restated (``pad_size = 2 * max
count * groups``, groups by richsem_amd.dn.dn_group_count).  A batch without any target has ``pad_size`` 0 and no denoising call (loss 0).

nl = 2 decoder layers, N = 3 images, Q = 10 queries; per-image counts (0, 5, 2), (1, 0, 0), (0, 0, 0), each with dn_number 3 and 100;
C = 301 classes and D = 130 embedding channels (both cross the row kernels' 256-thread stride and leave rows unaligned).  Cases: KL 'gt' with
the dynamic weight off and on, KL 'gt' with use_fed_on_kd, KL 'pred', L1 'gt'; every case for the distilled layers {1} and {0, 1}.
Everything runs in float64 on float16-exact student tensors (tests/distill_capacity_ref.py ``expand``: stored as 16-dimensional embeddings;
asserted here to round the same way on any machine) and float32-exact teacher rows; gradients by autograd.  The 'pred' teacher is the
student's tensor with the two layers swapped (no new data).  ``get_fed_loss_inds`` draws with the global RNG, seeded per get_loss call, so
that a call draws the same classes whichever layers are distilled beside it.

Stored per batch config and case, for the four calls (matching parts of layers 0, 1, then their denoising parts): the per-call losses
(float64), the class subsets of the fed case, and the gradient of ALL FOUR calls w.r.t. the student's tensor -- as three float64 checksums
per row (sum, sum of magnitudes, a cosine projection: tests/distill_capacity_ref.py ``checksums``) for every row, and in full (float32) for
the rows of the matched pairs and of the first denoising group.  The generator asserts that the runs with layers {1} give exactly the calls
of layer 1 and the gradient of its rows, so the two layer sets share the stored numbers.

Conditions asserted here (those of make_golden_distill.py): every logit row has max - min <= 80; every |u_j - v_j| >= 1e-5 on the L1 pairs;
nothing stored is non-finite.  The file is named criterion_distill_capacity_reference.npz: the "criterion_" prefix keeps tests/conftest.py
from taking it for an operator case.
"""
import os
import sys
import warnings

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [OUT, os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]

from distill_capacity_ref import CASES, LAYER_SETS, checksums, expand, products      # noqa: E402
from make_golden_criterion_capacity import reference_criterion      # noqa: E402
from make_golden_distill import Stub, reference_methods      # noqa: E402

NL, N, Q, C, D = 2, 3, 10, 301, 130
CFGS = [((0, 5, 2), 3), ((0, 5, 2), 100), ((1, 0, 0), 3), ((1, 0, 0), 100), ((0, 0, 0), 3), ((0, 0, 0), 100)]
MARGIN = 1e-12


def rounds_the_same_everywhere(e, table, kind):
    v = products(e, table, kind)
    d = MARGIN * (np.abs(v) + 1.0)      # (relative for the large values, absolute for those near 0: a 16-term product sum is off by ~1e-14 at most)
    return bool(((v + d).astype(np.float16) == (v - d).astype(np.float16)).all())


def embeddings(rows, table, kind, g):
    """(rows, 16) float32 embeddings whose expansion is safe from float16 rounding boundaries (rows resampled until it is)"""
    e = torch.randn(rows, 16, generator=g).numpy()
    for r in range(rows):
        for _ in range(1000):
            if rounds_the_same_everywhere(e[r: r + 1], table, kind):
                break
            e[r] = torch.randn(16, generator=g).numpy()
        else:
            raise AssertionError("no embedding away from the float16 rounding boundaries")
    return e


def main():
    from richsem_amd.dn import dn_group_count
    loss_labels, perm, drawn = reference_methods()
    crit, dn_block = reference_criterion()
    g = torch.Generator().manual_seed(301)
    text = torch.randn(C, 16, generator=g).numpy()
    basis = (torch.randn(16, D, generator=g) / 4).numpy()
    fed_weight = torch.ones(C)
    fed_weight[[0, 17]] = 0.0
    out = {"dims": np.array([NL, N, Q, C, D]), "cfgs": np.array([list(c) + [d] for c, d in CFGS]), "text": text, "basis": basis}
    for ci, (counts, dn_number) in enumerate(CFGS):
        p = f"c{ci}."
        total = sum(counts)
        groups = dn_group_count(dn_number, list(counts))
        pad = 2 * max(counts) * groups
        QT = pad + Q
        rows = NL * N * QT
        e_kl, e_tgt = embeddings(rows, text, "kl", g), embeddings(total, text, "kl", g)
        kl = torch.from_numpy(expand(e_kl, text, "kl")).view(NL, N, QT, C)
        teacher_gt = torch.from_numpy(expand(e_tgt, text, "kl")).view(total, C)
        for name, v in (("student", kl.view(-1, C)), ("teacher_gt", teacher_gt)):
            if v.numel():
                spread = v.max(-1).values - v.min(-1).values
                assert float(spread.max()) <= 80.0, (name, float(spread.max()))
        labels = torch.randint(0, C, (total,), generator=g)
        # ---- the stub matcher's result: per output and image, T_b distinct queries against the targets in order ------------------------------
        indices, qot = [], torch.full((NL + 1, max(total, 1)), -1, dtype=torch.int64)
        for o in range(NL + 1):
            per_image, at = [], 0
            for tb in counts:
                src = torch.randperm(Q, generator=g)[:tb]
                order = torch.argsort(src)      # (the matcher returns its pairs in query order)
                per_image.append((src[order], torch.arange(tb)[order]))
                qot[o, at: at + tb] = src
                at += tb
            indices.append(per_image)
        num_boxes = max(float(total), 1.0)
        # ---- the reference's denoising positives ---------------------------------------------------------------------------------------------
        targets_plain = [{"labels": labels[sum(counts[:b]): sum(counts[:b + 1])]} for b in range(N)]
        ns = {"self": crit, "torch": torch, "targets": targets_plain, "range": range, "len": len,
              "dn_meta": {"output_known_lbs_bboxes": None, "num_dn_group": groups, "pad_size": pad}}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")      # (torch.range is deprecated)
            exec(dn_block, ns)
        dn_pos_idx, scalar = ns["dn_pos_idx"], ns["scalar"]
        assert scalar == groups
        # ---- the L1 tensors: resampled until no |u - v| on a pair is below 1e-5 ---------------------------------------------------------------
        for attempt in range(100):
            e_l1 = embeddings(rows, basis, "l1", g)
            l1 = torch.from_numpy(expand(e_l1, basis, "l1")).view(NL, N, QT, D)
            prompt_gt = torch.randn(total, D, generator=g, dtype=torch.float64)
            prompt_gt = (prompt_gt / prompt_gt.norm(dim=-1, keepdim=True)).float().double()
            u = l1 / l1.norm(dim=-1, keepdim=True)
            gaps = [torch.ones(1, dtype=torch.float64)]
            for l in range(NL):
                for b in range(N):
                    src, tj = indices[l][b]
                    first = sum(counts[:b])
                    gaps.append((u[l, b, pad + src] - prompt_gt[first + tj]).abs().flatten())
                    if pad:
                        oi, ti = dn_pos_idx[b]
                        gaps.append((u[l, b, oi] - prompt_gt[first + ti]).abs().flatten())
            if float(torch.cat(gaps).min()) >= 1e-5:
                break
        else:
            raise AssertionError("no L1 sample with every |u - v| >= 1e-5")
        pred_logits = torch.randn(NL, N, QT, C, generator=g, dtype=torch.float64) * 4      # (loss_ce runs first; it does not enter loss_distill)
        targets = [{"labels": t["labels"], "clip_logits": teacher_gt[sum(counts[:b]): sum(counts[:b + 1])],
                    "clip_prompt": prompt_gt[sum(counts[:b]): sum(counts[:b + 1])]} for b, t in enumerate(targets_plain)]
        out.update({p + "groups": np.int64(groups), p + "pad_size": np.int64(pad), p + "num_boxes": np.float64(num_boxes),
                    p + "qot": qot[:, :total].numpy(), p + "labels": labels.numpy(), p + "e_kl": e_kl, p + "e_l1": e_l1, p + "e_tgt": e_tgt,
                    p + "prompt_gt": prompt_gt.float().numpy()})
        # the rows kept in full: the matched pairs' and the first denoising group's, of both layers
        sel = []
        for l in range(NL):
            for b in range(N):
                sel += [(l * N + b) * QT + pad + int(q) for q in indices[l][b][0]]
                if pad:
                    sel += [(l * N + b) * QT + j for j in range(counts[b])]
        sel = np.array(sorted(sel), dtype=np.int64)
        out[p + "sel_rows"] = sel

        def run(case, layers):
            kind, objective = case.split("_")[0], case.split("_")[1]
            dynamic, fed = case.endswith("dyn1"), case.endswith("fed")
            student = (kl if kind == "kl" else l1).clone().requires_grad_(True)
            teacher_out = kl.flip(0)
            stub = Stub((loss_labels, perm), "clip_logits" if kind == "kl" else "clip_l1", objective, dynamic, fed, fed_weight)
            stub.num_classes = C
            per_call, masks = torch.zeros(2 * NL, dtype=torch.float64), np.zeros((2 * NL, C), dtype=np.uint8)
            total_loss = torch.zeros((), dtype=torch.float64)
            for l in layers:
                for part, (lo, hi, idx, nb) in enumerate(((pad, QT, indices[l], num_boxes), (0, pad, dn_pos_idx, num_boxes * scalar))):
                    if hi == lo:
                        continue      # no denoising part
                    call = part * NL + l
                    outputs = {"pred_logits": pred_logits[l][:, lo:hi], "pred_hs": student[l][:, lo:hi], "pred_clip_logits": student[l][:, lo:hi],
                               "hs_prompt": None, "clip_logits": teacher_out[l][:, lo:hi]}
                    torch.manual_seed(9000 + 10 * ci + call)
                    n_drawn = len(drawn)
                    loss = stub.loss_labels(outputs, targets, idx, nb, log=False)["loss_distill"]
                    if fed:
                        assert len(drawn) == n_drawn + 1
                        masks[call, drawn[-1].numpy()] = 1
                    per_call[call] = loss.detach()
                    total_loss = total_loss + loss
            grad = torch.zeros_like(student)
            if total_loss.requires_grad:
                total_loss.backward()
                grad = student.grad
            assert bool(torch.isfinite(per_call).all()) and bool(torch.isfinite(grad).all()), case
            return per_call, grad.reshape(rows, -1), masks

        for case in CASES:
            per_call, grad, masks = run(case, (0, 1))
            one_call, one_grad, one_masks = run(case, (1,))
            # the runs with layer 1 alone: its calls and the gradient of its rows, bit for bit; nothing else
            assert torch.equal(one_call[[1, 3]], per_call[[1, 3]]) and not bool(one_call[[0, 2]].any()), case
            assert torch.equal(one_grad[N * QT:], grad[N * QT:]) and not bool(one_grad[: N * QT].any()), case
            assert (one_masks[[1, 3]] == masks[[1, 3]]).all()
            rest = grad.clone()
            rest[sel] = 0
            if pad:      # every other row with a gradient is a later denoising group's
                live = rest.abs().sum(-1).nonzero().flatten() % QT
                assert bool((live < pad).all()) and bool((live >= pad // groups).all()), case
            else:
                assert not bool(rest.any()), case
            out[p + case + ".per_call"] = per_call.numpy()
            out[p + case + ".grad_sums"] = checksums(grad.numpy())
            out[p + case + ".grad_sel"] = grad[sel].float().numpy()
            if case.endswith("fed"):
                out[p + case + ".masks"] = masks
            print(counts, dn_number, case, "groups", groups, "pad", pad, "per call", per_call.tolist())
    for k, v in out.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    path = os.path.join(OUT, "criterion_distill_capacity_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
