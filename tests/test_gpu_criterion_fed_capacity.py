"""The criterion over capacity buffers with the federated loss and class-agnostic two-stage targets (richsem_amd/criterion.py
``device_set_criterion``; ``msda_fed_class_mask_slots_f32``, ``msda_criterion_pairs_ex_f32``):

  * the slot kernel's subsets, bit for bit, against ``msda_fed_class_mask_f32`` on each call's exact label list with the same uniforms, and
    its ``n_chosen`` against the numpy restatement (tests/criterion_fed_capacity_ref.py), over the inputs that change which slots are live;
  * dead slots are never read; every positive class of a call lies inside that call's subset;
  * against tests/golden/criterion_fed_capacity_reference.npz -- the reference's own ``SetCriterion`` pieces with ``use_fed_loss`` in float64
    (tests/golden/make_golden_criterion_fed_capacity.py), the subsets being the recorded ``fed_ids`` --, with and without ``enc_cls_agn``;
  * against the exact-size composition (``FedClassSampler.sample`` + ``MaskedFocalNegativeSum`` + positive and box terms);
  * the class-agnostic matching plan, ``distill_class_mask``, and ONE captured graph replayed on other batches (a process of its own).

Bounds: those tests/test_gpu_criterion_capacity.py holds the same formulas to -- loss 1e-5 relative and gradients 1e-5 (boxes 2e-4) of the
largest reference gradient against the float64 fixture, 2e-5 / 2e-5 / 2e-4 against the float32 composition.
"""
import os

import numpy as np
import pytest
import torch

from criterion_fed_capacity_ref import appeared_sets, case, fixture, label_lists, n_chosen_of
from richsem_amd import _lib
from richsem_amd.criterion import device_criterion, device_set_criterion, device_set_criterion_and_grads
from richsem_amd.distill import device_distill, distill_class_mask
from richsem_amd.dn import denoising_queries, dn_buffers, dn_capacity, dn_group_count
from richsem_amd.fed_loss import FedClassSampler, MaskedFocalNegativeSum
from richsem_amd.matcher import BoxPairLoss, FocalPositiveSum, HungarianMatcher, TargetBuffers
from test_gpu_criterion_capacity import _close, _exact_leaves, _lay_out, _outputs, _random_batch, _targets_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
NL, N, Q, QI, CAPACITY = 2, 3, 10, 13, 16
G = 2 * NL + 1


def _weight(C):
    w = ((torch.arange(C) * 7) % 23 + 1).float() ** 0.5
    w[0] = w[17] = 0.0
    return w


def _qot(counts, gen, capacity=CAPACITY):
    """every target matched once per output, to distinct queries of its image; -1 past the live targets"""
    qot = torch.full((NL + 1, capacity), -1, dtype=torch.int64)
    for o in range(NL + 1):
        at = 0
        for tb in counts:
            qot[o, at: at + tb] = torch.randperm(QI if o == NL else Q, generator=gen)[:tb]
            at += tb
    return qot


def _slots(cum, ids, qot, meta, weight, u, C, num_sample_cats, flags=0, capacity=CAPACITY):
    """msda_fed_class_mask_slots_f32 on given uniforms: -> (mask (G, C), n_chosen (G))"""
    mask = torch.full((G, C), -1.0, dtype=torch.float32, device=DEV)
    n = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().msda_fed_class_mask_slots_f32(cum.data_ptr(), ids.data_ptr(), qot.data_ptr(), None if meta is None else meta.data_ptr(),
                                                         weight.data_ptr(), u.data_ptr(), NL, N, Q, QI, C, capacity, num_sample_cats, flags,
                                                         mask.data_ptr(), n.data_ptr(), _lib.raw_stream(torch.device(DEV, 0))))
    return mask, n


def _exact(labels, weight, u_row, C, num_sample_cats):
    """msda_fed_class_mask_f32 on one call's exact label list and its uniform row"""
    lab = torch.as_tensor(labels, dtype=torch.int64, device=DEV)
    mask = torch.empty((1, C), dtype=torch.float32, device=DEV)
    n = torch.empty(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().msda_fed_class_mask_f32(lab.data_ptr() if lab.numel() else None, lab.numel(), weight.data_ptr(), u_row.data_ptr(), 1, C,
                                                   num_sample_cats, mask.data_ptr(), n.data_ptr(), _lib.raw_stream(torch.device(DEV, 0))))
    return mask[0], n


@pytest.mark.parametrize("C", [33, 64, 70, 1203])
def test_masks_are_those_of_the_exact_size_kernel(C):
    gen = torch.Generator().manual_seed(11 + C)
    counts = [0, 5, 2]
    cum0 = [0, 0, 5, 7]
    base_ids = torch.zeros(CAPACITY, dtype=torch.int64)
    base_ids[:7] = torch.tensor([17, 0, C - 1, 5, 5, 31, 1])      # zero-weight classes, a repeat, the last class (a partial bit word)
    base_qot = _qot(counts, gen)
    live_meta, few = [5, 3, 30, 7, 0], _weight(C)
    few[12:] = 0.0      # 11 classes with a weight: fewer eligible than draws
    variants = {      # name -> (cum, ids, qot, meta, weight, flags)
        "base": (cum0, base_ids, base_qot, live_meta, _weight(C), 0),
        "no targets": ([0, 0, 0, 0], base_ids, base_qot, [0, 1, 0, 0, 0], _weight(C), 0),
        "dn overflow": (cum0, base_ids, base_qot, [5, 3, 30, 7, 1], _weight(C), 0),
        "no dn": (cum0, base_ids, base_qot, None, _weight(C), 0),
        "stride below the counts": (cum0, base_ids, base_qot, [3, 2, 6, 7, 0], _weight(C), 0),
        "class-agnostic two-stage": (cum0, base_ids, base_qot, live_meta, _weight(C), 1),
        "bad prefix": ([0, 9, 5, 40], base_ids, base_qot, live_meta, _weight(C), 0),
        "few eligible": (cum0, base_ids, base_qot, live_meta, few, 0),
    }
    q = base_qot.clone()
    q[0, 2], q[NL, 3], q[1, 4], q[1, 0] = -1, -1, Q, Q + 2      # without a query; a query of the two-stage range in a decoder output
    variants["targets without a query"] = (cum0, base_ids, q, live_meta, _weight(C), 0)
    ids = base_ids.clone()
    ids[2], ids[6] = C + 3, -1
    variants["labels out of range"] = (cum0, ids, base_qot, live_meta, _weight(C), 0)
    u = torch.rand((G, C), generator=gen).to(DEV)
    for name, (cum, ids, qot, meta, weight, flags) in variants.items():
        for num in ((50, 3) if name == "base" else (50,)):
            d = lambda t, dt=torch.int64: None if t is None else torch.as_tensor(t, dtype=dt).to(DEV)
            mask, n = _slots(d(cum), d(ids), d(qot), d(meta), weight.to(DEV), u, C, num, flags)
            lists = label_lists(cum, ids.numpy(), qot.numpy(), meta, NL, Q, QI, CAPACITY, flags)
            sets = appeared_sets(cum, ids.numpy(), qot.numpy(), meta, NL, Q, QI, C, CAPACITY, flags)
            for g in range(G):
                want, n_want = _exact(lists[g], weight.to(DEV), u[g], C, num)
                assert torch.equal(mask[g].view(torch.int32), want.view(torch.int32)), (name, g)
                assert int(n[g]) == int(n_want) == n_chosen_of(sets[g], weight.numpy(), num), (name, g, int(n[g]))
                assert int(mask[g].sum()) == int(n[g]) and bool((mask[g, torch.as_tensor(sets[g], device=DEV)] == 1).all())
            if name == "bad prefix" or name == "no targets":
                assert all(len(s) == 0 for s in sets)
            if name == "few eligible":      # every eligible class is taken, and n_chosen shows it
                assert all(int(n[g]) == len(sets[g]) + int(((weight > 0).numpy() & ~np.isin(np.arange(C), sets[g])).sum()) < 50 for g in range(G))
            if name in ("dn overflow", "no dn"):
                assert all(len(sets[g]) == 0 for g in range(NL, 2 * NL)) and len(sets[0]) > 0
            if name == "class-agnostic two-stage":
                assert sets[2 * NL].tolist() == [0] and float(mask[2 * NL, 0]) == 1.0
            if name == "stride below the counts":
                assert sets[NL].tolist() == sorted({17, 0, C - 1, 31, 1})


# ---- the fixture in the capacity layout --------------------------------------------------------------------------------------------------
def _sampler():
    return FedClassSampler(int(fixture()["num_sample_cats"]), class_weight=torch.as_tensor(fixture()["class_weight"]))


def _fixture_case(ci, pad_cap, capacity=CAPACITY):
    c = case(ci)
    t = lambda k: torch.as_tensor(c[k].astype(np.float32), device=DEV)
    counts, pad, groups = [int(v) for v in c["counts"]], int(c["pad_size"]), int(c["groups"])
    total = sum(counts)
    bufs = TargetBuffers(len(counts), capacity, DEV).update_(_targets_of(c["labels"], c["boxes"], counts))
    qot = torch.full((NL + 1, capacity), -1, dtype=torch.int64, device=DEV)
    qot[:, :total] = torch.as_tensor(c["qot"].reshape(NL + 1, total), device=DEV)
    meta = torch.tensor([max(counts), groups, pad, total, 0], dtype=torch.int64, device=DEV)
    leaves = {"logits": _lay_out(t("logits"), t("dn_logits"), pad_cap), "coords": _lay_out(t("coords"), t("dn_coords"), pad_cap, 0.5),
              "il": t("il"), "ib": t("ib")}
    C = leaves["il"].shape[-1]
    mask = torch.zeros((G, C), dtype=torch.float32)
    for g in range(G):
        ids = c["fed_ids"][g]
        mask[g, torch.as_tensor(ids[ids >= 0])] = 1.0
    return {"leaves": {k: v.requires_grad_(True) for k, v in leaves.items()}, "bufs": bufs, "qot": qot, "meta": meta, "pad": pad, "total": total,
            "counts": counts, "groups": groups, "z": c, "agn": bool(c["agn"]), "mask": mask.to(DEV), "C": C}


def _run(c, pad_cap, fn=device_set_criterion, **kw):
    for v in c["leaves"].values():
        v.grad = None
    L = c["leaves"]
    out = fn(L["logits"], L["coords"], L["il"], L["ib"], c["bufs"], c["qot"], kw.pop("meta", c["meta"]), pad_cap=pad_cap, **kw)
    out[0].backward()
    torch.cuda.synchronize()
    return (out[0].detach(),) + tuple(out[1:]) + ({k: v.grad.clone() for k, v in L.items()},)


def _sets_of(c, flags):
    return appeared_sets(c["bufs"].offsets, c["bufs"].tgt_ids.cpu().numpy(), c["qot"].cpu().numpy(), c["meta"].tolist(), NL, Q, QI, c["C"], CAPACITY,
                         flags)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def test_dead_slots_are_exactly_dead():
    pad_cap = 60 + 7
    c = _fixture_case(1, pad_cap)      # counts (0, 5, 2), dn_number 3, enc_cls_agn
    sampler = _sampler()
    loss, terms, status, (mask, n), grads = _run(c, pad_cap, fed=sampler, enc_cls_agn=True, generator=_gen(3))
    total = c["total"]
    with torch.no_grad():
        c["qot"][:, total:] = torch.tensor([1 << 40, -7, 3, 1 << 62, 0, 9, -1, 2, 5], device=DEV)[: CAPACITY - total]
        c["bufs"].tgt_ids[total:] = torch.tensor([10 ** 12, 1, 2, 3, 4, 5, 6, -1, 69], device=DEV)[: CAPACITY - total]
    loss2, terms2, status2, (mask2, n2), grads2 = _run(c, pad_cap, fed=sampler, enc_cls_agn=True, generator=_gen(3))
    assert status2.tolist() == [0, 0, 0, 0]
    assert torch.equal(mask, mask2) and torch.equal(n, n2) and n.tolist() == [50] * G
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(terms.view(torch.int32), terms2.view(torch.int32))
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)), k


@pytest.mark.parametrize("ci", range(12))
def test_positives_always_fall_inside_the_mask(ci):
    pad = int(case(ci)["pad_size"])
    c = _fixture_case(ci, pad + 9)
    mask, n = _sampler().sample_slots(c["bufs"], c["qot"], c["meta"], nl=NL, Q=Q, Qi=QI, enc_cls_agn=c["agn"], generator=_gen(40 + ci))
    loss, terms, status, (mask2, n2), grads = _run(c, pad + 9, fed=_sampler(), enc_cls_agn=c["agn"], generator=_gen(40 + ci))
    assert torch.equal(mask, mask2) and torch.equal(n, n2)      # the thin wrapper and the criterion draw the same
    assert n.tolist() == [50] * G and mask.sum(1).tolist() == [50.0] * G and bool(((mask == 0) | (mask == 1)).all())
    sets = _sets_of(c, int(c["agn"]))
    rec = c["z"]["appeared"]
    for g in range(G):
        assert np.array_equal(sets[g], rec[g][rec[g] >= 0])      # the live pairs of call g are the reference's
        assert bool((mask[g, torch.as_tensor(sets[g], device=DEV)] == 1).all()), g
    if c["agn"] and c["total"]:
        assert sets[2 * NL].tolist() == [0] and float(mask[2 * NL, 0]) == 1.0
    w = fixture()["class_weight"]
    for g in range(G):      # a zero-weight class is in the subset iff it appeared
        for zc in np.nonzero(w == 0)[0]:
            assert bool(mask[g, zc] == 1) == (zc in sets[g])
    # the gradient is exactly 0 off the subsets, and the rows past pad_size carry none
    off = lambda g: (mask[g] == 0).nonzero().flatten()
    for l in range(NL):
        assert float(grads["logits"][l][:, pad + 9:][..., off(l)].abs().max()) == 0.0
        assert float(grads["logits"][l][:, :pad + 9][..., off(NL + l)].abs().max()) == 0.0
    assert float(grads["il"][..., off(2 * NL)].abs().max()) == 0.0
    assert float(grads["logits"][:, :, pad:pad + 9].abs().max()) == 0.0 and status.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("ci", range(12))
@pytest.mark.parametrize("slack", [0, 9])
def test_against_the_reference_criterion(ci, slack):
    pad = int(case(ci)["pad_size"])
    pad_cap = pad + slack
    c = _fixture_case(ci, pad_cap)
    loss, terms, status, (mask, n), grads = _run(c, pad_cap, fed=c["mask"], enc_cls_agn=c["agn"])
    ref = c["z"]
    want = float(ref["loss"])
    per_call = torch.as_tensor(ref["per_call"])
    print(f"case {ci} pad_cap {pad_cap}: loss {float(loss):.9g} want {want:.9g} rel {abs(float(loss) - want) / abs(want):.2e}")
    assert status.tolist() == [0, 0, 0, 0] and torch.equal(mask, c["mask"]) and n.tolist() == c["mask"].sum(1).int().tolist()
    assert abs(float(loss) - want) <= 1e-5 * abs(want), (float(loss), want)
    for col, name in ((1, "loss_bbox"), (2, "loss_giou")):
        got = terms[:, col].cpu().double()
        err = (got - per_call[:, col]).abs()
        print(name, "max rel", float((err / per_call[:, col].abs().clamp(min=1e-300)).max()))
        assert bool((err <= 1e-5 * per_call[:, col].abs()).all()), (name, got.tolist(), per_call[:, col].tolist())
    g = lambda k: torch.as_tensor(ref["grad_" + k], device=DEV)
    for k, got, rel in (("logits", grads["logits"][:, :, pad_cap:], 1e-5), ("il", grads["il"], 1e-5), ("dn_logits", grads["logits"][:, :, :pad], 1e-5),
                        ("coords", grads["coords"][:, :, pad_cap:], 2e-4), ("ib", grads["ib"], 2e-4), ("dn_coords", grads["coords"][:, :, :pad], 2e-4)):
        w = g(k)
        if w.numel():
            print(k, "max err", float((got.double() - w.double()).abs().max()), "of", float(w.abs().max()))
        assert _close(got, w, rel), k
    # exactly 0 off the subsets
    off = lambda q: (c["mask"][q] == 0).nonzero().flatten()
    for l in range(NL):
        assert float(grads["logits"][l][:, pad_cap:][..., off(l)].abs().max()) == 0.0
        if pad:
            assert float(grads["logits"][l][:, :pad][..., off(NL + l)].abs().max()) == 0.0
    assert float(grads["il"][..., off(2 * NL)].abs().max()) == 0.0
    if slack:
        assert float(grads["logits"][:, :, pad:pad_cap].abs().max()) == 0.0 and float(grads["coords"][:, :, pad:pad_cap].abs().max()) == 0.0


def _fed_composition(logits, coords, il, ib, labels, boxes, counts, qot, groups, mask, alpha=0.25):
    """the exact-size composition with the federated loss, as ``Step.loss_part`` (bench_step.py) composes it: MaskedFocalNegativeSum over the
    decoder rows (each row's draw: its layer's matching or denoising call) and over the two-stage rows, FocalPositiveSum and BoxPairLoss on
    host-built indices.  logits (nl, N, pad_size + Q, C) in the batch's own layout, qot (nl + 1, total) with every target matched."""
    nl, n_img, QT, _ = logits.shape
    total, single = sum(counts), max(counts) if counts else 0
    pad = 2 * single * groups
    num_boxes = float(max(total, 1))
    nbx = num_boxes * groups
    w_q = torch.empty(QT, dtype=torch.float32, device=DEV)
    w_q[:pad] = 1.0 / nbx
    w_q[pad:] = 1.0 / num_boxes
    grp = torch.empty((nl, n_img, QT), dtype=torch.int32, device=DEV)
    for l in range(nl):
        grp[l, :, :pad] = nl + l
        grp[l, :, pad:] = l
    loss = MaskedFocalNegativeSum.apply(logits, w_q[None, None].expand(nl, n_img, QT).contiguous(), grp, mask, alpha) + \
        MaskedFocalNegativeSum.apply(il, torch.full(il.shape[:2], 1.0 / num_boxes, dtype=torch.float32, device=DEV),
                                     torch.full(il.shape[:2], 2 * nl, dtype=torch.int32, device=DEV), mask, alpha)
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    img = np.repeat(np.arange(n_img), counts)
    li = torch.as_tensor(np.repeat(np.arange(nl), total), device=DEV)
    bi = torch.as_tensor(np.tile(img, nl), device=DEV)
    tj = torch.as_tensor(np.tile(np.arange(total), nl), device=DEV)
    si = qot[:nl].reshape(-1)
    ibi, itj, isi = torch.as_tensor(img, device=DEV), torch.arange(total, device=DEV), qot[nl]
    dl, db, dq, dt = [], [], [], []
    for l in range(nl):
        for b in range(n_img):
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


def test_against_the_exact_size_composition_and_bitwise_reproducible():
    """the denoising part is live and every target is matched: every call's appeared classes are the batch's labels, so the same seed gives
    ``FedClassSampler.sample``'s masks"""
    C, counts, groups = 70, [0, 5, 2], 3
    gen = torch.Generator().manual_seed(21)
    pad, total = 2 * max(counts) * groups, sum(counts)
    pad_cap = pad + 9
    labels, boxes = _random_batch(counts, gen, C)
    bufs = TargetBuffers(N, CAPACITY, DEV).update_(_targets_of(labels.numpy(), boxes.numpy(), counts))
    qot = _qot(counts, gen).to(DEV)
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    L = {"logits": torch.randn(NL, N, pad_cap + Q, C, generator=gen) * 4, "coords": rb(NL, N, pad_cap + Q),
         "il": torch.randn(N, QI, C, generator=gen) * 4, "ib": rb(N, QI)}
    c = {"leaves": {k: v.to(DEV).requires_grad_(True) for k, v in L.items()}, "bufs": bufs, "qot": qot,
         "meta": torch.tensor([max(counts), groups, pad, total, 0], dtype=torch.int64, device=DEV)}
    sampler = FedClassSampler(50, class_weight=_weight(C))
    loss, terms, status, (mask, n), grads = _run(c, pad_cap, fed=sampler, generator=_gen(77))
    loss2, terms2, _, (mask2, n2), grads2 = _run(c, pad_cap, fed=sampler, generator=_gen(77))
    assert torch.equal(mask, mask2) and torch.equal(n, n2) and status.tolist() == [0, 0, 0, 0]
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(terms.view(torch.int32), terms2.view(torch.int32))
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), grads2[k].view(torch.int32)), k
    m_exact, n_exact = sampler.sample(labels.to(DEV), G, generator=_gen(77))
    assert torch.equal(mask.view(torch.int32), m_exact.view(torch.int32)) and torch.equal(n, n_exact)
    _, _, _, (mask3, _), _ = _run(c, pad_cap, fed=sampler, generator=_gen(78))
    assert not torch.equal(mask, mask3)      # another seed, another draw
    xl, xc, xil, xib = _exact_leaves(c["leaves"], pad, pad_cap)
    want = _fed_composition(xl, xc, xil, xib, labels.to(DEV), boxes.to(DEV), counts, qot[:, :total], groups, m_exact)
    want.backward()
    want = want.detach()
    print(f"loss {float(loss):.9g} composition {float(want):.9g}")
    assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want)), (float(loss), float(want))
    cut = lambda t: torch.cat((t[:, :, :pad], t[:, :, pad_cap:]), 2)
    assert _close(cut(grads["logits"]), xl.grad, 2e-5) and _close(grads["il"], xil.grad, 2e-5)
    assert _close(cut(grads["coords"]), xc.grad, 2e-4) and _close(grads["ib"], xib.grad, 2e-4)
    assert float(grads["logits"][:, :, pad:pad_cap].abs().max()) == 0.0
    # the same launches without the autograd engine: the same bits
    Lc = c["leaves"]
    loss4, terms4, _, (mask4, _), g4 = device_set_criterion_and_grads(Lc["logits"], Lc["coords"], Lc["il"], Lc["ib"], bufs, qot, c["meta"],
                                                                      pad_cap=pad_cap, fed=sampler, generator=_gen(77))
    assert torch.equal(loss4, loss) and torch.equal(terms4, terms) and torch.equal(mask4, mask)
    for k, g in zip(("logits", "coords", "il", "ib"), g4):
        assert torch.equal(g, grads[k]), k


def test_without_the_switches_it_is_device_criterion():
    c = _fixture_case(0, 60 + 9)
    loss, terms, status, fed_out, grads = _run(c, 69)
    want = _run(c, 69, fn=device_criterion)
    assert fed_out is None
    assert torch.equal(loss.view(torch.int32), want[0].view(torch.int32)) and torch.equal(terms.view(torch.int32), want[1].view(torch.int32))
    assert torch.equal(status, want[2])
    for k in grads:
        assert torch.equal(grads[k].view(torch.int32), want[3][k].view(torch.int32)), k
    # an all-ones mask: the masked kernels give the unmasked bits (msda_fed.h), the row groups select every class
    ones = _run(c, 69, fed=torch.ones((G, c["C"]), device=DEV))
    assert torch.equal(ones[0], loss) and torch.equal(ones[1], terms)
    for k in grads:
        assert torch.equal(ones[4][k].view(torch.int32), grads[k].view(torch.int32)), k


def test_class_agnostic_two_stage_alone():
    """enc_cls_agn without the federated loss: the decoder calls are device_criterion's on the targets as they are, the two-stage call is
    device_criterion's on targets whose labels are all 0 -- bit for bit"""
    c = _fixture_case(0, 60)
    loss, terms, status, fed_out, grads = _run(c, 60, enc_cls_agn=True)
    plain = _run(c, 60, fn=device_criterion)
    with torch.no_grad():
        c["bufs"].tgt_ids.zero_()
    zero = _run(c, 60, fn=device_criterion)
    assert fed_out is None and status.tolist() == [0, 0, 0, 0]
    assert torch.equal(terms[: 2 * NL], plain[1][: 2 * NL]) and torch.equal(terms[2 * NL], zero[1][2 * NL])
    assert not torch.equal(plain[1][2 * NL, 0], zero[1][2 * NL, 0])
    assert torch.equal(grads["logits"], plain[3]["logits"]) and torch.equal(grads["coords"], plain[3]["coords"])
    assert torch.equal(grads["il"], zero[3]["il"]) and torch.equal(grads["ib"], zero[3]["ib"])
    # a label out of range is no reason to leave a two-stage pair out: its class is 0
    c = _fixture_case(0, 60)
    with torch.no_grad():
        c["bufs"].tgt_ids[2] = 70 + 5
    _, terms_bad, status_bad, _, _ = _run(c, 60, enc_cls_agn=True)
    assert status_bad.tolist() == [0, 0, 1, 0] and torch.equal(terms_bad[2 * NL], terms[2 * NL]) and not torch.equal(terms_bad[0], terms[0])


def test_class_agnostic_matching():
    c = _fixture_case(0, 60)
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    outs = [{k: v.detach() for k, v in o.items()} for o in _outputs(c["leaves"], 60)]
    agn = c["bufs"].class_agnostic()
    q_def, st_def = matcher.match_many_device(outs, c["bufs"])
    q_agn, st_agn = matcher.match_many_device(outs, c["bufs"], last_plan=agn)
    q_last, st_last = matcher.match_many_device(outs[-1:], agn)
    t = c["total"]      # (the solver writes the live columns only)
    assert q_agn.shape == (NL + 1, CAPACITY) and not st_agn.any() and not st_last.any() and bool((q_agn[:, :t] >= 0).all())
    assert torch.equal(q_agn[:NL, :t], q_def[:NL, :t]) and torch.equal(q_agn[NL:, :t], q_last[:, :t]) and torch.equal(st_agn[:NL], st_def[:NL])
    # with the labels at 0 on the device the default call finds the same: the plan IS the targets with every label 0
    with torch.no_grad():
        c["bufs"].tgt_ids.zero_()
    q_zero, _ = matcher.match_many_device(outs, c["bufs"])
    assert torch.equal(q_zero[NL, :t], q_agn[NL, :t])
    with pytest.raises(ValueError):
        matcher.match_many_device(outs, c["bufs"], last_plan=TargetBuffers(N, CAPACITY, DEV))


def test_distill_class_mask_feeds_device_distill():
    C, pad_cap = 70, 60 + 9
    c = _fixture_case(0, pad_cap)
    gen = torch.Generator().manual_seed(8)
    pred = (torch.randn(1, N, pad_cap + Q, C, generator=gen) * 2).to(DEV).requires_grad_(True)
    teacher = (torch.randn(1, N, pad_cap + Q, C, generator=gen) * 2).to(DEV)
    mask, _ = _sampler().sample_slots(c["bufs"], c["qot"], c["meta"], nl=NL, Q=Q, Qi=QI, generator=_gen(5))
    kw = dict(pad_cap=pad_cap, layers=(1,), distill_type="clip_logits", objective="pred")
    got, st = device_distill(pred, teacher, c["bufs"], c["qot"], c["meta"], class_mask=distill_class_mask(mask, (1,), NL), **kw)
    want, _ = device_distill(pred, teacher, c["bufs"], c["qot"], c["meta"], class_mask=mask[[1, NL + 1]].contiguous(), **kw)
    other, _ = device_distill(pred, teacher, c["bufs"], c["qot"], c["meta"], class_mask=mask[[0, NL]].contiguous(), **kw)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not st.any() and float(got.detach()) != float(other.detach())
    assert tuple(distill_class_mask(mask, (0, 1), NL).shape) == (2 * NL, C)


def test_wrong_arguments_raise_before_any_launch():
    c = _fixture_case(4, 12)
    L = c["leaves"]
    args = (L["logits"], L["coords"], L["il"], L["ib"], c["bufs"], c["qot"], c["meta"])
    with pytest.raises(ValueError, match="classes"):
        device_set_criterion(*args, pad_cap=12, fed=FedClassSampler(50, num_classes=71))
    with pytest.raises(ValueError):
        device_set_criterion(*args, pad_cap=12, fed=torch.ones((G - 1, 70), device=DEV))
    with pytest.raises(ValueError):
        device_set_criterion(*args, pad_cap=12, fed=torch.ones((G, 70), device=DEV, dtype=torch.float64))
    with pytest.raises(TypeError):
        device_set_criterion(*args, pad_cap=12, fed=True)
    with pytest.raises(TypeError):
        device_set_criterion(L["logits"].double(), *args[1:], pad_cap=12, fed=_sampler())
    with pytest.raises(ValueError):
        device_set_criterion(*args[:5], c["qot"][:, :5].contiguous(), c["meta"], pad_cap=12, fed=_sampler())
    with pytest.raises(ValueError):
        _sampler().sample_slots(c["bufs"], c["qot"][:, :5].contiguous(), c["meta"], nl=NL, Q=Q, Qi=QI)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        device_set_criterion(*args, pad_cap=12, fed=torch.ones((G, 70)))


def test_one_graph_serves_many_batches():
    """cost blocks (the two-stage output against the class-agnostic plan) -> msda_lsap -> denoising_queries -> device_set_criterion with a
    sampler and enc_cls_agn + backward, captured ONCE at C = 1203 and replayed after ``update_`` on totals 7, 16 (full) and 0:
    ``_one_graph_job`` below, in a process of its own -- the suite's process is left without a stream, a graph or a graph memory pool of
    this test's making (tests/test_gpu_criterion_capacity.py ``test_one_graph_serves_many_batches`` says why)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_criterion_fed_capacity as t; t._one_graph_job(); print('one graph: ok')"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "one graph: ok" in r.stdout, (r.returncode, r.stderr[-2000:])


def _one_graph_job():
    """the body of test_one_graph_serves_many_batches (raises where it does not hold)"""
    from richsem_amd.capture import capture, capture_stream
    C, D, dn_number, max_per = 1203, 8, 3, 8
    pad_cap = dn_capacity(dn_number, max_per)
    gen = torch.Generator().manual_seed(9)
    batches = [[0, 5, 2], [8, 8, 0], [0, 0, 0]]
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    preds = [{"logits": torch.randn(NL, N, pad_cap + Q, C, generator=gen) * 3, "coords": rb(NL, N, pad_cap + Q),
              "il": torch.randn(N, QI, C, generator=gen) * 3, "ib": rb(N, QI)} for _ in batches]
    data = [_random_batch(counts, gen, C) for counts in batches]
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    table = torch.randn(C + 1, D, generator=gen).to(DEV)
    kw = dict(num_queries=Q, num_classes=C, dn_number=dn_number, label_noise_ratio=0.5, box_noise_scale=1.0)
    sampler = FedClassSampler(50, class_weight=((torch.arange(C) * 7) % 23 + 1).float() ** 0.5)

    with capture_stream() as side:
        bufs = TargetBuffers(N, CAPACITY, DEV, max_per_image=max_per)
        agn = bufs.class_agnostic()
        L = {k: v.to(DEV) for k, v in preds[0].items()}
        uni = torch.rand((N, pad_cap, 10), generator=gen).to(DEV)
        dn_out = dn_buffers(N, pad_cap, Q, D, DEV)

        def step():
            qot, st = matcher.match_many_device(_outputs(L, pad_cap), bufs, last_plan=agn)
            meta = denoising_queries(bufs.offsets_dev, bufs.tgt_ids, bufs.tgt_boxes, table, uni, pad_cap=pad_cap, out=dn_out, **kw)[4]
            loss, terms, status, (mask, n), grads = device_set_criterion_and_grads(L["logits"], L["coords"], L["il"], L["ib"], bufs, qot, meta,
                                                                                   pad_cap=pad_cap, fed=sampler, enc_cls_agn=True)
            return loss, grads, qot, st, meta, status, mask, n

        bufs.update_(_targets_of(data[0][0].numpy(), data[0][1].numpy(), batches[0]))
        step()      # eager once, on the capture stream (it also takes the sampler's weights to the device)
        torch.cuda.synchronize()
        graph, (loss, grads, qot, st, meta, status, mask, n) = capture(step, side)
        for i in (1, 2, 0, 0):
            counts, (labels, boxes) = batches[i], data[i]
            bufs.update_(_targets_of(labels.numpy(), boxes.numpy(), counts))
            with torch.no_grad():
                for k in L:
                    L[k].copy_(preds[i][k])
            previous = mask.clone()
            graph.replay()
            torch.cuda.synchronize()
            total, groups = sum(counts), dn_group_count(dn_number, counts)
            pad = 2 * max(counts) * groups
            assert meta.tolist() == [max(counts), groups, pad, total, 0] and status.tolist() == [0, 0, 0, 0] and not st.any()
            assert bool((qot[:, :total] >= 0).all())
            # the appeared classes of THIS batch are in the subsets: every layer's matched and denoising labels, class 0 for the two-stage call
            sets = appeared_sets(bufs.offsets, bufs.tgt_ids.cpu().numpy(), qot.cpu().numpy(), meta.tolist(), NL, Q, QI, C, CAPACITY, 1)
            want = np.unique(labels.numpy())
            for g in range(2 * NL):
                assert np.array_equal(sets[g], want), (i, g)
            assert sets[2 * NL].tolist() == ([0] if total else [])
            for g in range(G):
                assert bool((mask[g, torch.as_tensor(sets[g], device=DEV)] == 1).all()), (i, g)
            assert n.tolist() == [50] * G and mask.sum(1).tolist() == [50.0] * G
            assert not torch.equal(mask, previous)      # a replay draws afresh (also on the same batch: the last two rounds)
            # an eager call given the replay's subsets as a tensor: the same bits
            e_loss, e_terms, e_status, (e_mask, _), e_grads = device_set_criterion_and_grads(
                L["logits"], L["coords"], L["il"], L["ib"], bufs, qot.clone(), meta.clone(), pad_cap=pad_cap, fed=mask.clone(), enc_cls_agn=True)
            torch.cuda.synchronize()
            assert torch.equal(e_loss.view(torch.int32), loss.view(torch.int32)), (i, float(e_loss), float(loss))
            for a, b in zip(e_grads, grads):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), i
            for l in range(NL):      # nothing off the subsets
                assert float(grads[0][l][:, pad_cap:][..., (mask[l] == 0)].abs().max()) == 0.0
