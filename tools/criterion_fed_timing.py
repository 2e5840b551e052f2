#!/usr/bin/env python3
"""Time the criterion's classification and box part WITH the federated loss, forward + backward, eager, in ONE process, alternating:

  * ``composition``      the exact-size composition, as ``bench_step.Step.loss_part`` composes it with ``fed_loss``: ``FedClassSampler.sample``
                         on the batch's labels (2 nl + 1 draws), MaskedFocalNegativeSum x 2 with row groups built beforehand, the gathers on
                         index tensors of the batch's exact size, FocalPositiveSum, BoxPairLoss;
  * ``device exact``     ``richsem_amd.criterion.device_set_criterion(fed=sampler)`` with the batch's exact capacities;
  * ``device capacity``  the same with targets capacity 600 and pad_cap = dn_capacity(100, 300) = 600: the form ONE captured graph serves
                         every batch with;
and the two class-subset kernels alone, each behind its ``torch.rand`` of (13, C) uniforms:
  * ``mask kernel``      ``FedClassSampler.sample`` (``msda_fed_class_mask_f32``, 13 groups on the label list);
  * ``slot kernel``      ``FedClassSampler.sample_slots`` (``msda_fed_class_mask_slots_f32``, the same 13 calls from the slot space), with the exact
                         and with the capacity buffers.

    python tools/criterion_fed_timing.py [--calls 10] [--blocks 12] [--out FILE.md]

Shape and method: those of tools/criterion_timing.py (nl = 6, N = 2, 900 + pad queries, C = 1203, dn_number 100; 12 and 100 boxes per
image; every form untimed first, then alternating blocks between two HIP events; median and range over the blocks; launches by
torch.profiler in a pass of its own).  There is no CPU path: without a GPU this fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometry_timing import block_us, launches                             # noqa: E402
from richsem_amd.criterion import device_set_criterion                     # noqa: E402
from richsem_amd.dn import dn_capacity, dn_group_count                     # noqa: E402
from richsem_amd.fed_loss import FedClassSampler, MaskedFocalNegativeSum   # noqa: E402
from richsem_amd.matcher import BoxPairLoss, FocalPositiveSum, TargetBuffers      # noqa: E402

NL, N, Q, QI, C, DN = 6, 2, 900, 900, 1203, 100
G = 2 * NL + 1
CAPACITY, PAD_CAP = 600, dn_capacity(DN, 300)


def _inputs(pad_cap, gen, dev):
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    t = {"logits": torch.randn(NL, N, pad_cap + Q, C, generator=gen) * 3, "coords": rb(NL, N, pad_cap + Q),
         "il": torch.randn(N, QI, C, generator=gen) * 3, "ib": rb(N, QI)}
    return {k: v.to(dev).requires_grad_(True) for k, v in t.items()}


def forms(K, dev):
    gen = torch.Generator().manual_seed(K)
    counts, total = [K] * N, K * N
    groups = dn_group_count(DN, counts)
    pad = 2 * K * groups
    labels = torch.randint(0, C, (total,), generator=gen)
    boxes = torch.cat((torch.rand(total, 2, generator=gen) * 0.6 + 0.2, torch.rand(total, 2, generator=gen) * 0.3 + 0.05), 1)
    targets = [{"labels": labels[b * K: (b + 1) * K], "boxes": boxes[b * K: (b + 1) * K]} for b in range(N)]
    qot = torch.stack([torch.cat([torch.randperm(QI if o == NL else Q, generator=gen)[:K] for _ in range(N)]) for o in range(NL + 1)])
    meta = torch.tensor([K, groups, pad, total, 0], dtype=torch.int64, device=dev)
    sampler = FedClassSampler(50, class_weight=((torch.arange(C) * 7) % 23 + 1).float() ** 0.5)
    fns, small = {}, {}

    # ---- the exact-size composition --------------------------------------------------------------------------------------------------------
    X = _inputs(pad, gen, dev)
    lab_d, box_d, qd = labels.to(dev), boxes.to(dev), qot.to(dev)
    num_boxes = float(max(total, 1))
    nbx = num_boxes * groups
    w_q = torch.empty(pad + Q, dtype=torch.float32, device=dev)
    w_q[:pad], w_q[pad:] = 1.0 / nbx, 1.0 / num_boxes
    w_rows = w_q[None, None].expand(NL, N, pad + Q).contiguous()
    w_int = torch.full((N, QI), 1.0 / num_boxes, dtype=torch.float32, device=dev)
    g_rows = torch.empty((NL, N, pad + Q), dtype=torch.int32, device=dev)
    for l in range(NL):
        g_rows[l, :, :pad], g_rows[l, :, pad:] = NL + l, l
    g_int = torch.full((N, QI), 2 * NL, dtype=torch.int32, device=dev)
    img = torch.arange(N, device=dev).repeat_interleave(K)
    li, bi, tj, si = torch.arange(NL, device=dev).repeat_interleave(total), img.repeat(NL), torch.arange(total, device=dev).repeat(NL), qd[:NL].reshape(-1)
    itj, isi = torch.arange(total, device=dev), qd[NL]
    pos_slots = (torch.arange(groups, device=dev)[:, None] * 2 * K + torch.arange(K, device=dev)[None]).flatten()
    n_slots = pos_slots.numel()
    dn_l = torch.arange(NL, device=dev)[:, None, None].expand(NL, N, n_slots).reshape(-1)
    dn_n = torch.arange(N, device=dev)[None, :, None].expand(NL, N, n_slots).reshape(-1)
    dn_q = pos_slots[None, None, :].expand(NL, N, -1).reshape(-1)
    w_dn = torch.full((dn_l.numel(),), 1.0 / nbx, dtype=torch.float32, device=dev)

    def composition():
        for v in X.values():
            v.grad = None
        logits, coords, il, ib = X["logits"], X["coords"], X["il"], X["ib"]
        mask, _ = sampler.sample(lab_d, G)
        loss = MaskedFocalNegativeSum.apply(logits, w_rows, g_rows, mask, 0.25) + MaskedFocalNegativeSum.apply(il, w_int, g_int, mask, 0.25)
        dn_lab = lab_d.view(N, -1).repeat(1, groups)[None].expand(NL, -1, -1).reshape(-1)
        x_pos = torch.cat((logits[li, bi, si + pad, lab_d[tj]], il[img, isi, lab_d[itj]], logits[dn_l, dn_n, dn_q, dn_lab]))
        w_pair = torch.cat((torch.full((li.numel() + img.numel(),), 1.0 / num_boxes, dtype=torch.float32, device=dev), w_dn))
        loss = loss + FocalPositiveSum.apply(x_pos, w_pair, 0.25)
        pb = torch.cat((coords[li, bi, si + pad], ib[img, isi], coords[dn_l, dn_n, dn_q]))
        tb = torch.cat((box_d[tj], box_d[itj], box_d.view(N, -1, 4).repeat(1, groups, 1)[None].expand(NL, -1, -1, -1).reshape(-1, 4)))
        loss = loss + BoxPairLoss.apply(pb, tb, w_pair, 5.0, 2.0)
        loss.backward()
        return loss
    fns["composition"] = composition

    def device_form(capacity, pad_cap, Y, name):
        bufs = TargetBuffers(N, capacity, dev).update_(targets)
        q = torch.full((NL + 1, capacity), -1, dtype=torch.int64, device=dev)
        q[:, :total] = qd

        def run():
            for v in Y.values():
                v.grad = None
            loss = device_set_criterion(Y["logits"], Y["coords"], Y["il"], Y["ib"], bufs, q, meta, pad_cap=pad_cap, fed=sampler)[0]
            loss.backward()
            return loss
        small["slot kernel, " + name] = lambda: sampler.sample_slots(bufs, q, meta, nl=NL, Q=Q, Qi=QI)[1]
        return run
    fns["device exact"] = device_form(total, pad, X, "exact")
    fns["device capacity"] = device_form(CAPACITY, PAD_CAP, _inputs(PAD_CAP, gen, dev), "capacity")
    small = dict({"mask kernel": lambda: sampler.sample(lab_d, G)[1]}, **small)
    return pad, groups, fns, small


def measure(K, calls, blocks):
    pad, groups, fns, small = forms(K, torch.device("cuda", 0))
    losses = {}
    for k, fn in fns.items():      # untimed rehearsal
        for _ in range(3):
            losses[k] = float(fn().detach())
    for fn in small.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    row = {"boxes_per_image": K, "pad_size": pad, "groups": groups}
    for group, n_calls in ((fns, calls), (small, calls * 10)):
        t = {k: [] for k in group}
        for _ in range(blocks):
            for k, fn in group.items():
                t[k].append(block_us(fn, n_calls))
        for k in group:
            row[k] = {"median_us": statistics.median(t[k]), "min_us": min(t[k]), "max_us": max(t[k]), "launches": launches(group[k]),
                      "loss": losses.get(k)}
    print(json.dumps(row), flush=True)
    return row


def table(row):
    lines = [f"### {row['boxes_per_image']} boxes per image (pad_size {row['pad_size']}, {row['groups']} groups)", "",
             "| form | us per call, median (min .. max over blocks) | launches per call | loss |", "|---|---|---|---|"]
    for k, d in row.items():
        if isinstance(d, dict):
            loss = "" if d["loss"] is None else f"{d['loss']:.6f}"
            lines.append(f"| {k} | {d['median_us']:.1f} ({d['min_us']:.1f} .. {d['max_us']:.1f}) | {d['launches'] or 'not measured'} | {loss} |")
    for k in ("device exact", "device capacity"):
        lines.append(f"\n{k} / composition: {row[k]['median_us'] / row['composition']['median_us']:.3f}")
    for k in ("slot kernel, exact", "slot kernel, capacity"):
        lines.append(f"\n{k} - mask kernel: {row[k]['median_us'] - row['mask kernel']['median_us']:+.1f} us (mask kernel's range over blocks: "
                     f"{row['mask kernel']['max_us'] - row['mask kernel']['min_us']:.1f} us)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("criterion_fed_timing: no GPU; nothing is measured on a CPU")
    rows = [measure(K, a.calls, a.blocks) for K in (12, 100)]
    text = "\n\n".join([f"device: {torch.cuda.get_device_name(0)}; nl = {NL}, N = {N}, {Q} + pad queries, {QI} two-stage queries, C = {C}, 50 sampled "
                        f"classes; capacity form: {CAPACITY} targets, pad_cap {PAD_CAP}; {a.blocks} blocks of {a.calls} calls per form (the subset "
                        f"kernels alone: {a.calls * 10}), alternating; forward + backward for the three criterion forms"] + [table(r) for r in rows])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
