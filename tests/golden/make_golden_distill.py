#!/usr/bin/env python3
"""Golden vectors for the criterion's distillation term (richsem_amd/distill.py: DistillKL / DistillL1 / DistillLoss; ``msda_distill_kl_f32``,
``msda_distill_kl_bf16``, ``msda_distill_l1_f32``), generated from the REFERENCE's own method.  Run in the build container only (it reads
/root/reference; the fixture is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_distill.py

What is executed is the reference's ``SetCriterion.loss_labels`` and ``SetCriterion._get_src_permutation_idx`` (models/richsem/richsem.py),
cut out of the file with ``ast`` -- the file itself imports detectron2, which is absent -- compiled unchanged and bound to a stub object that
carries the attributes the method reads.  ``sigmoid_focal_loss`` (models/richsem/utils.py) and ``get_fed_loss_inds``
(models/richsem/fed_loss.py) are loaded by path as make_golden_fed.py loads them; the method's own ``from .fed_loss import
get_fed_loss_inds`` resolves to a module that records the ``fed_ids`` it returns.

Two images, N x Q = 2 x 6, C = 1204, D = 1024; image 0 has three boxes, image 1 none.  Everything runs in float64 on float32-exact inputs,
gradients by autograd w.r.t. the student's output.  Cases:
  * KL (``distill_type='clip_logits'``): objective gt / pred / pred_all x use_dynamic_distill_weight off / on; gt (dynamic weight on) and pred
    (off) with use_fed_loss + use_fed_on_kd.
  * L1 (``'clip_l1'``): the three objectives.
Stored: the student's and the teacher's tensors once (the cases share them), per case the loss (float64) and the gradient -- the matched
rows ``grad[batch_idx, src_idx]`` for gt / pred (the generator asserts that every other row's gradient is 0), the whole (2, 6, .) for
pred_all -- rounded to float32 to keep the file the size of the other criterion fixtures (a relative 2^-24 of each value;
tests/test_distill_host.py ties a float64 restatement of the formulas to these numbers, and the GPU tests compare with that restatement).

Conditions asserted here -- they keep the yardstick finite and the comparison meaningful, they are not measurements:
  * every logit row has max - min <= 80: below that the reference's ``p * log p`` stays finite in float32 as well;
  * every |u_j - v_j| >= 1e-5 in the L1 cases (resampled otherwise), so that no gradient sign hangs on rounding;
  * nothing stored is non-finite.
The file is named criterion_distill_reference.npz: tests/conftest.py takes every fixture whose name does not start with another row's
prefix ("criterion_" is the criterion's) for an operator case.
"""
import ast
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
C, D, N, Q = 1204, 1024, 2, 6
SPREAD = 45.0      # logits = SPREAD * cos: row ranges of 61 .. 71 with 16-dimensional embeddings (CLIP's 100 * cos would overshoot the limit of 80)


def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, f"{REF}/{rel}")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_methods():
    """loss_labels and _get_src_permutation_idx of the reference's SetCriterion, compiled from the reference's source text"""
    fed, utils = load("_ref_fed_loss", "models/richsem/fed_loss.py"), load("_ref_utils", "models/richsem/utils.py")
    src = open(f"{REF}/models/richsem/richsem.py").read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "SetCriterion")
    wanted = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("loss_labels", "_get_src_permutation_idx")]
    assert len(wanted) == 2
    drawn = []

    def recording(*a, **kw):
        ids = fed.get_fed_loss_inds(*a, **kw)
        drawn.append(ids)
        return ids

    pkg = types.ModuleType("_ref_richsem")
    pkg.__path__ = []
    sub = types.ModuleType("_ref_richsem.fed_loss")
    sub.get_fed_loss_inds = recording
    sys.modules["_ref_richsem"], sys.modules["_ref_richsem.fed_loss"] = pkg, sub
    glob = {"torch": torch, "F": F, "math": math, "sigmoid_focal_loss": utils.sigmoid_focal_loss, "__name__": "_ref_richsem.richsem",
            "__package__": "_ref_richsem"}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), f"{REF}/models/richsem/richsem.py", "exec"), glob)
    return glob["loss_labels"], glob["_get_src_permutation_idx"], drawn


class Stub:
    num_classes = C
    focal_alpha = 0.25
    fed_num_sample_cats = 50

    def __init__(self, methods, distill_type, objective, dynamic, fed, fed_weight):
        self._loss_labels, self._perm = methods
        self.distill_type, self.clip_distill_objective, self.use_dynamic_distill_weight = distill_type, objective, dynamic
        self.use_fed_loss = self.use_fed_on_kd = fed
        self.fed_weight = fed_weight

    def _get_src_permutation_idx(self, indices):
        return self._perm(self, indices)

    def loss_labels(self, *a, **kw):
        return self._loss_labels(self, *a, **kw)


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def f32_exact(x):
    return x.float().double()


def main():
    loss_labels, perm, drawn = reference_methods()
    g = torch.Generator().manual_seed(1204)
    text = unit(torch.randn(C, 16, generator=g, dtype=torch.float64))      # (16 dimensions: cosines of about +-0.6 at most)
    logits_of = lambda n: f32_exact(SPREAD * unit(torch.randn(n, 16, generator=g, dtype=torch.float64)) @ text.t())
    labels = [torch.tensor([7, 300, 1100]), torch.zeros(0, dtype=torch.int64)]
    indices = [(torch.tensor([4, 1, 2]), torch.tensor([2, 0, 1])), (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))]
    num_boxes = 3.0
    kl = {"student": logits_of(N * Q).view(N, Q, C), "teacher_out": logits_of(N * Q).view(N, Q, C), "teacher_gt": logits_of(3)}
    for k, v in kl.items():
        spread = v.max(-1).values - v.min(-1).values
        assert float(spread.max()) <= 80.0, (k, float(spread.max()))
        print(k, "row ranges", float(spread.min()), "..", float(spread.max()))
    # L1: resample until no |u - v| is below 1e-5 for any objective
    for attempt in range(100):
        l1 = {"student": f32_exact(torch.randn(N, Q, D, generator=g) * 3), "prompt_out": f32_exact(torch.randn(N, Q, D, generator=g) * 2),
              "prompt_gt": f32_exact(unit(torch.randn(3, D, generator=g, dtype=torch.float64)))}
        u = unit(l1["student"])
        b, s = perm(None, indices)
        gaps = torch.cat(((u[b, s] - l1["prompt_gt"][indices[0][1]]).abs().flatten(), (u - unit(l1["prompt_out"])).abs().flatten()))
        if float(gaps.min()) >= 1e-5:
            break
    else:
        raise AssertionError("no L1 sample with every |u - v| >= 1e-5")
    print("L1: smallest |u - v|", float(gaps.min()), "after", attempt + 1, "draw(s)")
    pred_logits = f32_exact(torch.randn(N, Q, C, generator=g) * 4)      # (loss_ce runs first; it does not enter loss_distill)
    fed_weight = torch.ones(C)
    fed_weight[[0, 17]] = 0.0
    b, s = perm(None, indices)
    out = {"batch_idx": b.numpy(), "src_idx": s.numpy(), "tgt_idx": torch.cat([j for _, j in indices]).numpy(), "num_boxes": np.float64(num_boxes),
           "labels": torch.cat(labels).numpy()}
    out.update({f"kl.{k}": v.float().numpy() for k, v in kl.items()})
    out.update({f"l1.{k}": v.float().numpy() for k, v in l1.items()})

    def run(name, distill_type, objective, dynamic=False, fed=False):
        src = kl if distill_type == "clip_logits" else l1
        student = src["student"].clone().requires_grad_(True)
        outputs = {"pred_logits": pred_logits, "pred_hs": student, "pred_clip_logits": student,
                   "hs_prompt": src.get("prompt_out"), "clip_logits": src.get("teacher_out")}
        targets = [{"labels": labels[0], "clip_logits": kl["teacher_gt"], "clip_prompt": l1["prompt_gt"]},
                   {"labels": labels[1], "clip_logits": kl["teacher_gt"][:0], "clip_prompt": l1["prompt_gt"][:0]}]
        torch.manual_seed(50 + len(drawn))      # (get_fed_loss_inds draws with the global RNG)
        n_drawn = len(drawn)
        losses = Stub((loss_labels, perm), distill_type, objective, dynamic, fed, fed_weight).loss_labels(outputs, targets, indices, num_boxes, log=False)
        loss = losses["loss_distill"]
        loss.backward()
        grad = student.grad
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), name
        if objective != "pred_all":
            rest = grad.clone()
            rest[b, s] = 0
            assert not bool(rest.any()), name      # only the matched rows get a gradient
            grad = grad[b, s]
        out[f"{name}.loss"] = loss.detach().numpy()
        out[f"{name}.grad"] = grad.float().numpy()
        if fed:
            assert len(drawn) == n_drawn + 1
            out[f"{name}.fed_ids"] = drawn[-1].numpy()
        print(name, "loss", float(loss.detach()), "fed classes", drawn[-1].numel() if fed else "-")

    for objective in ("gt", "pred", "pred_all"):
        for dynamic in (False, True):
            run(f"kl_{objective}_dyn{int(dynamic)}", "clip_logits", objective, dynamic)
        run(f"l1_{objective}", "clip_l1", objective)
    run("kl_gt_fed", "clip_logits", "gt", dynamic=True, fed=True)
    run("kl_pred_fed", "clip_logits", "pred", dynamic=False, fed=True)
    for k, v in out.items():
        assert np.isfinite(np.asarray(v, dtype=np.float64)).all(), k
    path = os.path.join(OUT, "criterion_distill_reference.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
