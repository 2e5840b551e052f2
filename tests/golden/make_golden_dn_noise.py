#!/usr/bin/env python3
"""Golden vectors for the floating-point part of the denoising set-up: the REFERENCE's own ``prepare_for_cdn``
(models/richsem/dn_components.py:11-193) run on the CPU in float32, with the four random draws it makes recorded.

Run in the build container only (it reads the reference; the fixture it writes is committed, the GPU box never sees the reference):

    python tests/golden/make_golden_dn_noise.py

The reference is loaded as tests/golden/make_golden_layers.py loads it (``reference_modules``), and ``.cuda()`` / ``.to('cuda')`` are mapped to
the CPU tensor while it runs, as there.  ``torch.rand_like`` / ``torch.randint_like`` are wrapped to keep a copy of what they return -- in call
order: p (dn_components.py:59), new_label (:63, for the chosen rows only: expanded to full length with -1 elsewhere), rand_sign's 0 / 1
(:82), rand_part (:83) -- and the module's ``inverse_sigmoid`` to keep a copy of its argument, the noised boxes (:129).  Written: tests/golden/dn_noise_reference.npz -- per case the targets, the draws, input_query_label,
input_query_bbox, attn_mask, dn_meta and the noised boxes in the reference's row order; once the label table.  The generator also checks that the numpy restatement tests/dn_noise_ref.py,
fed with the draws as uniforms, gives the reference's labels / rows / mask exactly, and that the edge case clamps at 0 and at 1."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dn_noise_ref as R                      # noqa: E402
from make_golden_layers import reference_modules      # noqa: E402

HIDDEN, NUM_QUERIES, NUM_CLASSES = 16, 30, 1204      # table: V = NUM_CLASSES + 1 = 1205 rows
# name: (counts, dn_number, use_cdn, add_gt, label_noise_ratio, box_noise_scale, boxes near the canvas edge)
CASES = {
    "ragged": ((3, 0, 7), 100, True, False, 0.5, 1.0, False),          # an empty image between two others
    "no_cdn": ((4, 2), 100, False, False, 0.5, 1.0, False),            # the positive halves only
    "add_gt": ((3, 7), 100, True, True, 0.5, 1.0, False),              # group-half 0 unnoised
    "one_group": ((101, 3), 100, True, False, 0.5, 1.0, False),        # dn_number * 2 // (2 * max) == 0 -> 1 group
    "small_dn": ((2, 2), 3, True, False, 0.5, 0.4, False),             # dn_number * 2 < 100: taken as it is; a scale that is not 1
    "edge": ((5, 6), 100, True, False, 0.5, 1.0, True),                # the clamp at 0 and at 1
    "empty": ((0, 0), 100, True, False, 0.5, 1.0, False),              # no target at all: pad_size 0
}


class Recorder:
    def __init__(self, dn):
        self.dn, self.rand, self.randint, self.noised_box = dn, [], [], []
        self._rand_like, self._randint_like = torch.rand_like, torch.randint_like

    def __enter__(self):
        def rand_like(*a, **k):
            out = self._rand_like(*a, **k)
            self.rand.append(out.clone())
            return out

        def randint_like(*a, **k):
            out = self._randint_like(*a, **k)
            self.randint.append(out.clone())
            return out
        self._to, self._cuda, self._inv = torch.Tensor.to, torch.Tensor.cuda, self.dn.inverse_sigmoid
        to_ = self._to

        def inverse_sigmoid(x, *a, **k):
            self.noised_box.append(x.clone())
            return self._inv(x, *a, **k)
        self.dn.inverse_sigmoid = inverse_sigmoid

        def to_cpu(t, *a, **k):
            a = tuple("cpu" if isinstance(x, str) and x.startswith("cuda") else x for x in a)
            return to_(t, *a, **k)
        torch.rand_like, torch.randint_like = rand_like, randint_like
        torch.Tensor.to, torch.Tensor.cuda = to_cpu, lambda t, *a, **k: t
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.randint_like = self._rand_like, self._randint_like
        torch.Tensor.to, torch.Tensor.cuda, self.dn.inverse_sigmoid = self._to, self._cuda, self._inv
        return False


def main():
    _, dn, _ = reference_modules()
    rng = np.random.default_rng(1611)
    torch.manual_seed(1611)
    label_enc = torch.nn.Embedding(NUM_CLASSES + 1, HIDDEN)
    table = label_enc.weight.detach().numpy().copy()
    out = {"table": table, "cases": np.array(sorted(CASES)), "dims": np.array([HIDDEN, NUM_QUERIES, NUM_CLASSES], np.int64)}
    for ci, (name, (counts, dn_number, use_cdn, add_gt, ratio, scale, edge)) in enumerate(sorted(CASES.items())):
        targets = []
        for n in counts:
            cxcy, wh = rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.05, 0.4, (n, 2))
            if edge:      # centres at the canvas border, boxes wide enough that the noise leaves the canvas on both sides
                cxcy = np.where(rng.random((n, 2)) < 0.5, rng.uniform(0.0, 0.08, (n, 2)), rng.uniform(0.92, 1.0, (n, 2)))
                wh = rng.uniform(0.1, 0.5, (n, 2))
            targets.append({"labels": torch.as_tensor(rng.integers(1, 1203, n), dtype=torch.long),
                            "boxes": torch.as_tensor(np.concatenate((cxcy, wh), 1), dtype=torch.float32).reshape(n, 4)})
        torch.manual_seed(7000 + ci)
        with Recorder(dn) as rec, torch.no_grad():
            q_label, q_bbox, attn_mask, meta = dn.prepare_for_cdn((targets, dn_number, ratio, scale), True, NUM_QUERIES, NUM_CLASSES, HIDDEN,
                                                                 label_enc, use_cdn=use_cdn, add_gt=add_gt)
        assert len(rec.rand) == 2 and len(rec.randint) == 2 and len(rec.noised_box) == 1, (len(rec.rand), len(rec.randint))
        noised_rows = rec.noised_box[0].numpy().reshape(-1, 4)
        p, rand = rec.rand[0].numpy(), rec.rand[1].numpy()
        chosen_labels, sign01 = rec.randint[0].numpy(), rec.randint[1].numpy()
        total = sum(counts)
        p_used = p.copy()
        if add_gt:
            p_used[:total] = 1      # dn_components.py:60-61
        chosen = np.nonzero(p_used < np.float32(ratio * 0.5))[0]
        assert len(chosen) == len(chosen_labels)
        new_label = np.full(len(p), -1, np.int64)
        new_label[chosen] = chosen_labels
        labels = torch.cat([t["labels"] for t in targets]).numpy()
        boxes = torch.cat([t["boxes"] for t in targets]).numpy().reshape(-1, 4)
        pad_size = int(meta["pad_size"])
        pre = name + "."
        out.update({pre + "counts": np.asarray(counts, np.int64), pre + "labels": labels, pre + "boxes": boxes,
                    pre + "args": np.asarray([dn_number, int(use_cdn), int(add_gt)], np.int64),
                    pre + "noise": np.asarray([ratio, scale], np.float64), pre + "p": p, pre + "new_label": new_label,
                    pre + "sign01": sign01.astype(np.uint8), pre + "rand": rand, pre + "input_query_label": q_label.numpy(),
                    pre + "input_query_bbox": q_bbox.numpy(), pre + "noised_box_rows": noised_rows, pre + "attn_mask": attn_mask.numpy(),
                    pre + "meta": np.asarray([pad_size, int(meta["num_dn_group"])], np.int64)})
        # the restatement on these draws is the reference, exactly (q_bbox: how far the reference's own float32 inverse_sigmoid is from the
        # float64 one, in units of the bound the tests use, is printed)
        u = R.uniform_from_draws(counts, p, new_label, sign01, rand, NUM_CLASSES, pad_size, use_cdn)
        got = R.denoising_queries_ref(counts, labels, boxes, u, table, pad_cap=pad_size, num_queries=NUM_QUERIES, num_classes=NUM_CLASSES,
                                      dn_number=dn_number, label_noise_ratio=ratio, box_noise_scale=scale, use_cdn=use_cdn, add_gt=add_gt,
                                      return_preclamp=True)
        assert got["meta"][2] == pad_size and got["meta"][1] == meta["num_dn_group"], (name, got["meta"], meta)
        assert np.array_equal(got["q_label"], q_label.numpy()) and np.array_equal(got["attn_mask"], attn_mask.numpy()), name
        y64, bound = R.q_bbox_bound(got["noised_box"])
        filled = got["noised_label"] >= 0
        err = np.abs(q_bbox.numpy().astype(np.float64) - y64)[filled]
        assert not q_bbox.numpy()[~filled].any(), name
        rows = R.rows_from_slots(counts, got["noised_box"], len(p) // total if total else 0, use_cdn)
        keep = ~np.isnan(rows[:, 0])
        assert np.array_equal(rows[keep], noised_rows[keep]), name
        if edge:
            assert (got["preclamp"] < 0).any() and (got["preclamp"] > 1).any(), "the edge case must clamp at 0 and at 1"
        print(f"{name}: counts {counts} pad_size {pad_size} groups {int(meta['num_dn_group'])} chosen {len(chosen)} "
              f"reference q_bbox: max err / bound {float((err / bound[filled]).max()) if err.size else 0.0:.3f}, "
              f"{int((err > bound[filled]).sum())} of {err.size} elements outside")
    path = os.path.join(HERE, "dn_noise_reference.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
