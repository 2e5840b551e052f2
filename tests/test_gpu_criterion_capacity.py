"""The criterion over capacity buffers (richsem_amd/criterion.py ``device_criterion``, ``msda_criterion_pairs_f32``) and the matcher on
``TargetBuffers``:

  * against tests/golden/criterion_capacity_reference.npz -- the reference's own ``SetCriterion`` pieces in float64 on prescribed indices
    (tests/golden/make_golden_criterion_capacity.py) --, with ``pad_cap`` equal to and larger than the batch's ``pad_size``;
  * dead slots (target rows and ``query_of_target`` columns past the live targets, denoising rows past ``pad_size``) are never read;
  * against the exact-size composition ``Step.loss_part`` is made of (FocalNegativeSum + FocalPositiveSum + BoxPairLoss on host-built
    indices), bitwise reproducible;
  * ONE captured graph of cost blocks -> assignment -> denoising meta -> criterion + backward, replayed on batches of other totals and
    per-image counts;
  * the status words.

Bounds: loss 1e-5 relative and gradients 1e-5 (boxes 2e-4) of the largest reference gradient against the float64 fixture, 2e-5 / 2e-5 /
2e-4 against the float32 composition -- the bounds tests/test_gpu_step.py holds the same formulas to.
"""
import os

import numpy as np
import pytest
import torch

from richsem_amd.capture import capture, capture_stream
from richsem_amd.criterion import device_criterion, device_criterion_and_grads
from richsem_amd.dn import denoising_queries, dn_buffers, dn_capacity, dn_group_count
from richsem_amd.matcher import BoxPairLoss, CostPlan, FocalNegativeSum, FocalPositiveSum, HungarianMatcher, TargetBuffers

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAPACITY = 16
_Z = None


def _fixture():
    global _Z
    if _Z is None:
        _Z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_capacity_reference.npz")))
    return _Z


def _targets_of(labels, boxes, counts):
    out, at = [], 0
    for tb in counts:
        out.append({"labels": torch.as_tensor(labels[at: at + tb], dtype=torch.int64), "boxes": torch.as_tensor(boxes[at: at + tb], dtype=torch.float32).reshape(-1, 4)})
        at += tb
    return out


def _lay_out(match, dn, pad_cap, fill=0.0):
    """(nl, N, Q, k) matching rows and (nl, N, pad_size, k) denoising rows -> (nl, N, pad_cap + Q, k): denoising rows first, ``fill`` in
    [pad_size, pad_cap)"""
    nl, N, _, k = match.shape
    pad = dn.shape[2]
    full = torch.full((nl, N, pad_cap - pad, k), fill, dtype=torch.float32, device=DEV)
    return torch.cat((dn, full, match), 2).contiguous()


def _fixture_case(ci, pad_cap, capacity=CAPACITY):
    """case ``ci`` of the fixture in the capacity layout: -> dict of leaves, buffers, query_of_target (nl + 1, capacity), meta, reference"""
    z, p = _fixture(), f"c{ci}."
    t = lambda k: torch.as_tensor(z[p + k].astype(np.float32), device=DEV)
    counts, pad, groups = [int(c) for c in z[p + "counts"]], int(z[p + "pad_size"]), int(z[p + "groups"])
    total = sum(counts)
    bufs = TargetBuffers(len(counts), capacity, DEV).update_(_targets_of(z[p + "labels"], z[p + "boxes"], counts))
    qot = torch.full((z[p + "qot"].shape[0], capacity), -1, dtype=torch.int64, device=DEV)
    qot[:, :total] = torch.as_tensor(z[p + "qot"], device=DEV)
    meta = torch.tensor([max(counts), groups, pad, total, 0], dtype=torch.int64, device=DEV)
    leaves = {"logits": _lay_out(t("logits"), t("dn_logits"), pad_cap), "coords": _lay_out(t("coords"), t("dn_coords"), pad_cap, 0.5),
              "il": t("il"), "ib": t("ib")}
    return {"leaves": {k: v.requires_grad_(True) for k, v in leaves.items()}, "bufs": bufs, "qot": qot, "meta": meta, "pad": pad,
            "total": total, "counts": counts, "groups": groups, "z": {k[len(p):]: v for k, v in z.items() if k.startswith(p)}}


def _run(c, pad_cap, **kw):
    for v in c["leaves"].values():
        v.grad = None
    L = c["leaves"]
    loss, terms, status = device_criterion(L["logits"], L["coords"], L["il"], L["ib"], c["bufs"], c["qot"], kw.pop("meta", c["meta"]), pad_cap=pad_cap, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), terms, status, {k: v.grad.clone() for k, v in L.items()}


def _close(got, want, rel):
    """|got - want| <= rel * max|want| (element-wise against the largest reference entry; an all-zero reference asks for zeros)"""
    if want.numel() == 0:
        return True
    return float((got.double() - want.double()).abs().max()) <= rel * float(want.double().abs().max())


@pytest.mark.parametrize("ci", range(6))
@pytest.mark.parametrize("slack", [0, 9])
def test_against_the_reference_criterion(ci, slack):
    z = _fixture()
    pad = int(z[f"c{ci}.pad_size"])
    pad_cap = pad + slack
    c = _fixture_case(ci, pad_cap)
    loss, terms, status, grads = _run(c, pad_cap)
    ref = c["z"]
    want = float(ref["loss"])
    per_call = torch.as_tensor(ref["per_call"])
    print(f"case {ci} pad_cap {pad_cap}: loss {float(loss):.9g} want {want:.9g} rel {abs(float(loss) - want) / abs(want):.2e}")
    assert status.tolist() == [0, 0, 0, 0]
    assert abs(float(loss) - want) <= 1e-5 * abs(want), (float(loss), want)
    for col, name in ((1, "loss_bbox"), (2, "loss_giou")):
        got = terms[:, col].cpu().double()
        err = (got - per_call[:, col]).abs()
        print(name, "max rel", float((err / per_call[:, col].abs().clamp(min=1e-300)).max()))
        assert bool((err <= 1e-5 * per_call[:, col].abs()).all()), (name, got.tolist(), per_call[:, col].tolist())
    # the total re-derived from terms needs the all-negative term too: it is in `loss`; the positive-entry column is checked through it
    g = lambda k: torch.as_tensor(ref["grad_" + k], device=DEV)
    assert _close(grads["logits"][:, :, pad_cap:], g("logits"), 1e-5) and _close(grads["il"], g("il"), 1e-5)
    assert _close(grads["logits"][:, :, :pad], g("dn_logits"), 1e-5)
    assert _close(grads["coords"][:, :, pad_cap:], g("coords"), 2e-4) and _close(grads["ib"], g("ib"), 2e-4)
    assert _close(grads["coords"][:, :, :pad], g("dn_coords"), 2e-4)
    if slack:
        assert float(grads["logits"][:, :, pad:pad_cap].abs().max()) == 0.0 and float(grads["coords"][:, :, pad:pad_cap].abs().max()) == 0.0


def test_dead_slots_are_exactly_dead():
    pad_cap = 60 + 7
    c = _fixture_case(0, pad_cap)
    loss, terms, status, grads = _run(c, pad_cap)
    pad, total = c["pad"], c["total"]
    with torch.no_grad():
        c["qot"][:, total:] = torch.tensor([1 << 40, -7, 3, 1 << 62, 0, 9, -1, 2, 5], device=DEV)[: CAPACITY - total]
        c["bufs"].tgt_ids[total:] = 10 ** 12
        c["bufs"].tgt_boxes[total:] = float("nan")
        c["leaves"]["logits"][:, :, pad:pad_cap] = float("nan")
        c["leaves"]["coords"][:, :, pad:pad_cap] = 1e30
        c["leaves"]["coords"][:, :, pad:pad_cap, 0] = float("nan")
    loss2, terms2, status2, grads2 = _run(c, pad_cap)
    assert status2.tolist() == [0, 0, 0, 0]
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(terms.view(torch.int32), terms2.view(torch.int32))
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)), k
    assert float(grads2["logits"][:, :, pad:pad_cap].abs().max()) == 0.0 and float(grads2["coords"][:, :, pad:pad_cap].abs().max()) == 0.0


def _composition(logits, coords, il, ib, labels, boxes, counts, qot, groups, alpha=0.25):
    """the exact-size composition of ``Step.loss_part`` (bench_step.py) for ANY per-image counts: logits (nl, N, pad_size + Q, C) in the
    batch's own layout, qot (nl + 1, total) with every target matched.  Host-built index tensors, the three existing kernels."""
    nl, N, QT, _ = logits.shape
    total, single = sum(counts), max(counts) if counts else 0
    pad = 2 * single * groups
    num_boxes = float(max(total, 1))
    nbx = num_boxes * groups
    w_q = torch.empty(QT, dtype=torch.float32, device=DEV)
    w_q[:pad] = 1.0 / nbx
    w_q[pad:] = 1.0 / num_boxes
    loss = FocalNegativeSum.apply(logits, w_q[None, None].expand(nl, N, QT).contiguous(), alpha) + \
        FocalNegativeSum.apply(il, torch.full(il.shape[:2], 1.0 / num_boxes, dtype=torch.float32, device=DEV), alpha)
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    img = np.repeat(np.arange(N), counts)
    li = torch.as_tensor(np.repeat(np.arange(nl), total), device=DEV)
    bi = torch.as_tensor(np.tile(img, nl), device=DEV)
    tj = torch.as_tensor(np.tile(np.arange(total), nl), device=DEV)
    si = qot[:nl].reshape(-1)
    ibi, itj, isi = torch.as_tensor(img, device=DEV), torch.arange(total, device=DEV), qot[nl]
    dl, db, dq, dt = [], [], [], []
    for l in range(nl):
        for b in range(N):
            for g in range(groups):
                for j in range(counts[b]):
                    dl.append(l), db.append(b), dq.append(g * 2 * single + j), dt.append(cum[b] + j)
    dl, db, dq, dt = (torch.as_tensor(np.array(v, dtype=np.int64), device=DEV) for v in (dl, db, dq, dt))
    x_pos = torch.cat((logits[li, bi, si + pad, labels[tj]], il[ibi, isi, labels[itj]], logits[dl, db, dq, labels[dt]]))
    w_pair = torch.cat((torch.full((li.numel() + ibi.numel(),), 1.0 / num_boxes, dtype=torch.float32, device=DEV),
                        torch.full((dl.numel(),), 1.0 / nbx, dtype=torch.float32, device=DEV)))
    pb = torch.cat((coords[li, bi, si + pad], ib[ibi, isi], coords[dl, db, dq]))
    tb = torch.cat((boxes[tj], boxes[itj], boxes[dt]))
    return loss + FocalPositiveSum.apply(x_pos, w_pair, alpha) + BoxPairLoss.apply(pb, tb, w_pair, 5.0, 2.0)


def _exact_leaves(L, pad, pad_cap):
    """the capacity layout's leaves cut down to the batch's own layout, as new leaves"""
    cut = lambda t: torch.cat((t[:, :, :pad], t[:, :, pad_cap:]), 2).detach().clone().requires_grad_(True)
    return cut(L["logits"]), cut(L["coords"]), L["il"].detach().clone().requires_grad_(True), L["ib"].detach().clone().requires_grad_(True)


def _check_against_composition(loss, grads, L, pad, pad_cap, labels, boxes, counts, qot, groups):
    xl, xc, xil, xib = _exact_leaves(L, pad, pad_cap)
    want = _composition(xl, xc, xil, xib, labels, boxes, counts, qot, groups)
    want.backward()
    want = want.detach()
    print(f"counts {counts}: loss {float(loss):.9g} composition {float(want):.9g}")
    assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want)), (float(loss), float(want))
    cut = lambda t: torch.cat((t[:, :, :pad], t[:, :, pad_cap:]), 2)
    assert _close(cut(grads["logits"]), xl.grad, 2e-5) and _close(grads["il"], xil.grad, 2e-5)
    assert _close(cut(grads["coords"]), xc.grad, 2e-4) and _close(grads["ib"], xib.grad, 2e-4)
    assert float(grads["logits"][:, :, pad:pad_cap].abs().max() if pad_cap > pad else 0.0) == 0.0


def _random_batch(counts, gen, C):
    total = sum(counts)
    labels = torch.randint(0, C, (total,), generator=gen)
    boxes = torch.cat((torch.rand(total, 2, generator=gen) * 0.6 + 0.2, torch.rand(total, 2, generator=gen) * 0.3 + 0.05), 1)
    return labels, boxes


def test_against_the_existing_composition_and_bitwise_reproducible():
    """more than one workgroup per call (capacity 300 > 256, N * pad_cap = 1060), unequal counts, random inputs"""
    nl, N, Q, Qi, C, counts, groups, capacity = 3, 2, 300, 140, 91, [130, 97], 2, 300
    gen = torch.Generator().manual_seed(5)
    pad, pad_cap, total = 2 * max(counts) * groups, 2 * max(counts) * groups + 10, sum(counts)
    labels, boxes = _random_batch(counts, gen, C)
    bufs = TargetBuffers(N, capacity, DEV).update_(_targets_of(labels.numpy(), boxes.numpy(), counts))
    qot = torch.full((nl + 1, capacity), -1, dtype=torch.int64)
    for o in range(nl + 1):
        at = 0
        for tb in counts:
            qot[o, at: at + tb] = torch.randperm(Qi if o == nl else Q, generator=gen)[:tb]
            at += tb
    qot = qot.to(DEV)
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    L = {"logits": (torch.randn(nl, N, pad_cap + Q, C, generator=gen) * 4), "coords": rb(nl, N, pad_cap + Q),
         "il": torch.randn(N, Qi, C, generator=gen) * 4, "ib": rb(N, Qi)}
    c = {"leaves": {k: v.to(DEV).requires_grad_(True) for k, v in L.items()}, "bufs": bufs, "qot": qot,
         "meta": torch.tensor([max(counts), groups, pad, total, 0], dtype=torch.int64, device=DEV)}
    loss, terms, status, grads = _run(c, pad_cap)
    loss2, terms2, _, grads2 = _run(c, pad_cap)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(terms.view(torch.int32), terms2.view(torch.int32))
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)), k
    assert status.tolist() == [0, 0, 0, 0]
    _check_against_composition(loss, grads, c["leaves"], pad, pad_cap, labels.to(DEV), boxes.to(DEV), counts, qot[:, :total], groups)
    # the same launches without the autograd engine (what a whole-step capture calls): the same bits
    Lc = c["leaves"]
    loss3, terms3, _, g3 = device_criterion_and_grads(Lc["logits"], Lc["coords"], Lc["il"], Lc["ib"], bufs, qot, c["meta"], pad_cap=pad_cap)
    assert torch.equal(loss3, loss) and torch.equal(terms3, terms)
    for k, g in zip(("logits", "coords", "il", "ib"), g3):
        assert torch.equal(g, grads[k]), k


def _outputs(L, pad_cap):
    nl = L["logits"].shape[0]
    return [{"pred_logits": L["logits"][l][:, pad_cap:], "pred_boxes": L["coords"][l][:, pad_cap:]} for l in range(nl)] + \
        [{"pred_logits": L["il"], "pred_boxes": L["ib"]}]


def test_matcher_over_capacity_buffers():
    c = _fixture_case(0, 60)
    z = c["z"]
    targets = [{k: v.to(DEV) for k, v in t.items()} for t in _targets_of(z["labels"], z["boxes"], c["counts"])]
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    outs = [{k: v.detach() for k, v in o.items()} for o in _outputs(c["leaves"], 60)]
    q_cap, st_cap = matcher.match_many_device(outs, c["bufs"])
    q_ex, st_ex = matcher.match_many_device(outs, CostPlan(targets, DEV, torch.float32))
    assert q_cap.shape == (3, CAPACITY) and q_ex.shape == (3, c["total"])
    assert torch.equal(q_cap[:, :c["total"]], q_ex) and torch.equal(st_cap, st_ex) and not st_ex.any()
    assert bool((q_ex >= 0).all())


def test_one_graph_serves_many_batches():
    """cost blocks -> msda_lsap -> denoising_queries (for its meta) -> device_criterion + backward captured ONCE on capacity buffers;
    replays after ``update_`` on batches with totals 7, 16 (full), 0 and 7 with other per-image counts, each against the eager exact-size
    composition of THAT batch (its own CostPlan, its own layout): ``_one_graph_job`` below, run in a process of its own.  Why a process
    of its own: with this capture made in the suite's process, the whole suite segfaulted in the HIP runtime's replay of a later, unrelated
    graph (tests/test_gpu_fed_loss.py, the graphed federated step), which passes after this file alone; the cause is not known (DESIGN.md
    section 9), so this test leaves the suite's process without a stream, a graph or a graph memory pool of its making."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_criterion_capacity as t; t._one_graph_job(); print('one graph: ok')"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "one graph: ok" in r.stdout, (r.returncode, r.stderr[-2000:])


def _one_graph_job():
    """the body of test_one_graph_serves_many_batches (raises where it does not hold)"""
    nl, N, Q, Qi, C, D, dn_number, max_per = 2, 2, 12, 14, 23, 8, 3, 8
    pad_cap = dn_capacity(dn_number, max_per)
    assert pad_cap == 96
    gen = torch.Generator().manual_seed(9)
    batches = [[3, 4], [8, 8], [0, 0], [6, 1]]
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    preds = [{"logits": torch.randn(nl, N, pad_cap + Q, C, generator=gen) * 3, "coords": rb(nl, N, pad_cap + Q),
              "il": torch.randn(N, Qi, C, generator=gen) * 3, "ib": rb(N, Qi)} for _ in batches]
    data = [_random_batch(counts, gen, C) for counts in batches]
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    table = torch.randn(C + 1, D, generator=gen).to(DEV)
    kw = dict(num_queries=Q, num_classes=C, dn_number=dn_number, label_noise_ratio=0.5, box_noise_scale=1.0)

    with capture_stream() as side:
        bufs = TargetBuffers(N, CAPACITY, DEV, max_per_image=max_per)
        L = {k: v.to(DEV).requires_grad_(True) for k, v in preds[0].items()}
        uni = torch.rand((N, pad_cap, 10), generator=gen).to(DEV)
        dn_out = dn_buffers(N, pad_cap, Q, D, DEV)

        def step():
            qot, st = matcher.match_many_device(_outputs(L, pad_cap), bufs)
            meta = denoising_queries(bufs.offsets_dev, bufs.tgt_ids, bufs.tgt_boxes, table, uni, pad_cap=pad_cap, out=dn_out, **kw)[4]
            # (forward and backward launched from this thread: the capture holds no work of the autograd engine's threads)
            loss, terms, status, grads = device_criterion_and_grads(L["logits"], L["coords"], L["il"], L["ib"], bufs, qot, meta, pad_cap=pad_cap)
            return loss, grads, qot, st, meta, status

        bufs.update_(_targets_of(data[0][0].numpy(), data[0][1].numpy(), batches[0]))
        step()      # eager once, on the capture stream
        torch.cuda.synchronize()
        graph, (loss, grads, qot, st, meta, status) = capture(step, side)
        for i in (1, 2, 3, 0):
            counts, (labels, boxes) = batches[i], data[i]
            bufs.update_(_targets_of(labels.numpy(), boxes.numpy(), counts))
            with torch.no_grad():
                for k in L:
                    L[k].copy_(preds[i][k])
            graph.replay()
            torch.cuda.synchronize()
            total, groups = sum(counts), dn_group_count(dn_number, counts)
            pad = 2 * max(counts) * groups
            assert meta.tolist() == [max(counts), groups, pad, total, 0] and status.tolist() == [0, 0, 0, 0] and not st.any()
            if total:      # the same assignment from the batch's own exact plan
                targets = [{k: v.to(DEV) for k, v in t.items()} for t in _targets_of(labels.numpy(), boxes.numpy(), counts)]
                q_ex, _ = matcher.match_many_device([{k: v.detach() for k, v in o.items()} for o in _outputs(L, pad_cap)],
                                                    CostPlan(targets, DEV, torch.float32))
                assert torch.equal(qot[:, :total], q_ex)
            else:
                q_ex = torch.zeros((nl + 1, 0), dtype=torch.int64, device=DEV)
            g = dict(zip(("logits", "coords", "il", "ib"), grads))
            _check_against_composition(loss, g, L, pad, pad_cap, labels.to(DEV), boxes.to(DEV), counts, q_ex, groups)


def test_update_refuses_what_does_not_fit_on_the_device_too():
    bufs = TargetBuffers(2, 4, DEV, max_per_image=3)
    ok = _targets_of(np.arange(4), np.full((4, 4), 0.25, dtype=np.float32), [1, 3])
    bufs.update_(ok)
    assert bufs.offsets_dev.tolist() == [0, 1, 4] and bufs.tgt_ids.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        bufs.update_(_targets_of(np.arange(5), np.full((5, 4), 0.25, dtype=np.float32), [2, 3]))
    assert bufs.offsets_dev.tolist() == [0, 1, 4]
    bufs.update_(_targets_of(np.arange(1), np.full((1, 4), 0.25, dtype=np.float32), [0, 1]))
    assert bufs.offsets_dev.tolist() == [0, 0, 1] and bufs.tgt_ids.tolist() == [0, 0, 0, 0] and bufs.tgt_boxes[1:].tolist() == [[0.5, 0.5, 1.0, 1.0]] * 3


def test_status_pad_cap_too_small():
    """the layout (pad_size 60) does not fit pad_cap 20: the overflow word is set, the denoising part contributes nothing -- the result is
    bit for bit the one without a denoising part -- and the matching part is the reference's"""
    c = _fixture_case(0, 60)
    L = c["leaves"]
    small = {k: (torch.cat((v[:, :, :20], v[:, :, 60:]), 2) if v.dim() == 4 else v).detach().clone().requires_grad_(True) for k, v in L.items()}
    c["leaves"] = small
    loss, terms, status, grads = _run(c, 20)
    loss0, terms0, status0, grads0 = _run(c, 20, meta=None)
    assert status.tolist() == [1, 0, 0, 0] and status0.tolist() == [0, 0, 0, 0]
    assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)) and torch.equal(terms, terms0)
    nl = 2
    assert float(terms[nl: 2 * nl].abs().max()) == 0.0
    per_call = torch.as_tensor(c["z"]["per_call"])
    for call in (0, 1, 4):
        for col in (1, 2):
            assert abs(float(terms[call, col]) - float(per_call[call, col])) <= 1e-5 * abs(float(per_call[call, col]))
    assert float(grads["logits"][:, :, :20].abs().max()) == 0.0 and float(grads["coords"][:, :, :20].abs().max()) == 0.0
    assert _close(grads["coords"][:, :, 20:], torch.as_tensor(c["z"]["grad_coords"], device=DEV), 2e-4)


def test_status_counts_labels_out_of_range_and_targets_without_a_query():
    c = _fixture_case(0, 60)
    base_loss, base_terms, _, _ = _run(c, 60)
    bad = 2      # target 2: image 1's target 2 (counts 0, 5, 2)
    with torch.no_grad():
        c["bufs"].tgt_ids[bad] = 37 + 5
    loss, terms, status, grads = _run(c, 60)
    assert status.tolist() == [0, 0, 1, 0] and bool(torch.isfinite(loss))
    q_last = int(c["qot"][1, bad])
    assert float(grads["coords"][1, 1, 60 + q_last].abs().max()) == 0.0      # its matched pair is left out ...
    stride = 60 // c["groups"]
    rows = [g * stride + bad for g in range(c["groups"])]
    assert float(grads["coords"][:, 1, rows].abs().max()) == 0.0             # ... and so are its denoising slots
    assert float(grads["coords"][1, 1, 60 + int(c["qot"][1, 3])].abs().max()) > 0.0
    # a target whose query is -1: counted per output; in the last decoder output it also leaves num_boxes (7 -> 6)
    c = _fixture_case(0, 60)
    with torch.no_grad():
        c["qot"][0, 3] = -1
        c["qot"][1, 1] = -1
    loss, terms, status, grads = _run(c, 60)
    assert status.tolist() == [0, 2, 0, 0]
    for col in (0, 1, 2):      # the two-stage call keeps its pairs: only the normaliser changed
        want = float(base_terms[4, col]) * 7.0 / 6.0
        assert abs(float(terms[4, col]) - want) <= 1e-5 * abs(want)
    # the caller's num_boxes instead of the count
    loss7, terms7, _, _ = _run(c, 60, num_boxes=torch.tensor([7.0], device=DEV))
    assert torch.equal(terms7[4], base_terms[4])
    # a prefix that does not describe targets inside the capacity: everything is left out, nothing is read through it
    with torch.no_grad():
        c["bufs"].offsets_dev.copy_(torch.tensor([0, 9, 5, 40], device=DEV))
    loss, terms, status, grads = _run(c, 60)
    assert status[3].item() == 1 and float(terms.abs().max()) == 0.0 and float(grads["coords"].abs().max()) == 0.0


def test_wrong_arguments_raise_before_any_launch():
    c = _fixture_case(2, 12)
    L = c["leaves"]
    with pytest.raises(TypeError):
        device_criterion(L["logits"].double(), L["coords"], L["il"], L["ib"], c["bufs"], c["qot"], c["meta"], pad_cap=12)
    with pytest.raises(ValueError):
        device_criterion(L["logits"], L["coords"], L["il"], L["ib"], c["bufs"], c["qot"][:, :5].contiguous(), c["meta"], pad_cap=12)
    with pytest.raises(ValueError):
        device_criterion(L["logits"], L["coords"][:, :, 1:], L["il"], L["ib"], c["bufs"], c["qot"], c["meta"], pad_cap=12)
    for k in ("fed_loss", "enc_cls_agn", "distill"):
        with pytest.raises(NotImplementedError):
            device_criterion(L["logits"], L["coords"], L["il"], L["ib"], c["bufs"], c["qot"], c["meta"], pad_cap=12, **{k: True})
