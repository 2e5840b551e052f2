"""The federated loss on the GPU (richsem_amd/fed_loss.py; csrc/msda_fed.h): the device class sampler against the distribution of the
reference's ``get_fed_loss_inds`` (models/richsem/fed_loss.py:15-25: the appeared classes + weighted draws without replacement by
``torch.multinomial``), the masked all-negative focal kernels against the reference's ``sigmoid_focal_loss`` over ``fed_ids``
(tests/golden/criterion_fed_reference.npz, made by tests/golden/make_golden_fed.py from the reference's own functions), and the composed
step's opt-in switch (bench_step.Step(fed_loss=True)) eager and graphed.  Every draw is seeded; every statistical bound is derived in the
test from the exact or estimated probabilities, not from a passing run."""
import itertools
import math
import os
import warnings

import numpy as np
import pytest
import torch

from richsem_amd.fed_loss import FedClassSampler, MaskedFocalNegativeSum, fed_ids
from richsem_amd.matcher import FocalNegativeSum, FocalPositiveSum

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_fed_reference.npz")
H, W_IMG, BOXES = 256, 320, 5      # the small composed step of tests/test_gpu_step.py
DEV = "cuda"


def _lvis_weight():
    """the fixture's set_cats weights: C = 1204, long-tailed, weight 0 at id 0 and at the ids without a category"""
    return torch.from_numpy(np.load(FIXTURE)["fed_weight"])


def _check_masks(mask, n_chosen, labels, weight, k=50):
    """the invariants of one draw of ``groups`` masks: 0 / 1 values, every appeared class in every row, max(k, a) classes per row and as
    many in n_chosen, no weight-0 class drawn"""
    C = mask.shape[1]
    appeared = torch.zeros(C, dtype=torch.bool)
    appeared[labels.cpu()] = True
    a = int(appeared.sum())
    m = mask.cpu()
    assert bool(((m == 0) | (m == 1)).all())
    assert bool((m[:, appeared] == 1).all())
    assert torch.equal(m.sum(1), torch.full((m.shape[0],), float(max(k, a))))
    assert torch.equal(n_chosen.cpu(), torch.full((m.shape[0],), max(k, a), dtype=torch.int32))
    assert bool((m[:, (weight.cpu() <= 0) & ~appeared] == 0).all())
    return a


def test_sampler_invariants_at_lvis_size():
    w = _lvis_weight()
    s = FedClassSampler(50, w)
    G = 13
    cases = {"few": torch.tensor([5, 9, 9, 1100, 5, 17, 0, 600]),      # repeats, and two weight-0 classes (17, 0) that appeared
             "many": torch.randperm(1203, generator=torch.Generator().manual_seed(3))[:70] + 1,
             "none": torch.zeros(0, dtype=torch.int64)}
    for name, labels in cases.items():
        lab = labels.to(DEV)
        mask, n = s.sample(lab, G, generator=torch.Generator(device=DEV).manual_seed(5))
        a = _check_masks(mask, n, labels, w)
        again, n2 = s.sample(lab, G, generator=torch.Generator(device=DEV).manual_seed(5))
        assert torch.equal(mask, again) and torch.equal(n, n2), name                      # the same seed draws the same classes
        other, _ = s.sample(lab, G, generator=torch.Generator(device=DEV).manual_seed(6))
        if a >= 50:
            assert torch.equal(mask, other), name                                        # nothing is drawn: the appeared classes only
            continue
        assert not torch.equal(mask, other), name
        # the 13 groups draw independently: no two rows alike (two draws of 42+ classes out of ~1190 coincide with probability < 1e-60)
        rows = {tuple(fed_ids(r).tolist()) for r in mask}
        assert len(rows) == G, name
    # fewer eligible classes than draws: every eligible class, and n_chosen says how many (torch.multinomial would raise)
    w10 = torch.zeros(1204)
    w10[torch.arange(10) * 7 + 3] = torch.arange(1, 11).float()
    mask, n = FedClassSampler(50, w10).sample(torch.tensor([3, 10, 1000], device=DEV), 4)
    want = torch.zeros(1204)
    want[torch.arange(10) * 7 + 3] = 1
    want[[3, 10, 1000]] = 1
    assert torch.equal(mask.cpu(), want[None].expand(4, -1)) and torch.equal(n.cpu(), torch.full((4,), 11, dtype=torch.int32))      # 3 + 8
    # no host synchronisation in the sampler or in the masked focal kernels, forward or backward
    x = torch.randn(2, 30, 1204, device=DEV, requires_grad=True)
    rw, grp = torch.full((2, 30), 0.1, device=DEV), torch.zeros((2, 30), dtype=torch.int32, device=DEV)
    few = cases["few"].to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fm, _ = s.sample(few, 1)
        MaskedFocalNegativeSum.apply(x, rw, grp, fm, 0.25).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


def _subset_probabilities(w, eligible, m):
    """exact probability of every m-subset of `eligible` under m sequential weighted draws without replacement (torch.multinomial's
    scheme): the sum over the subset's orderings of the product of w_i / (the weight still in the urn)"""
    W = sum(w[c] for c in eligible)
    probs = {}
    for sub in itertools.combinations(eligible, m):
        p = 0.0
        for order in itertools.permutations(sub):
            left, q = W, 1.0
            for c in order:
                q *= w[c] / left
                left -= w[c]
            p += q
        probs[sub] = p
    return probs


def test_sampler_draws_subsets_with_the_probabilities_of_sequential_weighted_draws():
    """C = 8, 4 classes per group, 2 appeared -> 2 drawn among the 5 eligible classes (class 4 has weight 0), 200 000 groups in one launch:
    the frequency of each of the 10 possible subsets against its exact probability.  Bounds: per subset 5 sigma of a binomial proportion
    (a union over 10 subsets fails by chance with probability < 1e-5); the total-variation distance below 0.5 sum_i sigma_i (>= its mean)
    + sqrt(ln(1e9) / (2 n)) (McDiarmid: one group moves it by at most 1 / n; a chance failure has probability < 1e-9)."""
    w = [0.5, 1.0, 2.0, 3.0, 0.0, 4.0, 1.5, 6.0]
    appeared = [1, 6]
    n = 200_000
    s = FedClassSampler(4, torch.tensor(w))
    mask, n_chosen = s.sample(torch.tensor(appeared, device=DEV), n, generator=torch.Generator(device=DEV).manual_seed(17))
    _check_masks(mask, n_chosen, torch.tensor(appeared), torch.tensor(w), k=4)
    drawn = mask.clone()
    drawn[:, appeared] = 0
    code = (drawn * (2.0 ** torch.arange(8, device=DEV))).sum(1).long().cpu()
    counts = torch.bincount(code, minlength=256).double()
    probs = _subset_probabilities(w, [0, 2, 3, 5, 7], 2)
    assert abs(sum(probs.values()) - 1.0) < 1e-12
    tv, sig = 0.0, 0.0
    for sub, p in probs.items():
        freq = float(counts[sum(1 << c for c in sub)]) / n
        sigma = math.sqrt(p * (1 - p) / n)
        assert abs(freq - p) <= 5 * sigma, (sub, freq, p, sigma)
        tv += 0.5 * abs(freq - p)
        sig += 0.5 * sigma
    assert float(counts.sum()) == n and sum(float(counts[sum(1 << c for c in sub)]) for sub in probs) == n      # no other subset
    bound = sig + math.sqrt(math.log(1e9) / (2 * n))
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] subset frequencies: total variation {tv:.5f} (bound {bound:.5f})", flush=True)
    assert tv <= bound, (tv, bound)


def test_sampler_inclusion_frequencies_match_torch_multinomial_at_lvis_size():
    """20 000 groups at C = 1204 with the LVIS-like weights and 8 appeared classes (42 drawn per group): each class's inclusion frequency
    against torch.multinomial(w with the appeared classes zeroed, 42, replacement=False) over as many rows -- the reference's own draw.
    Bound per class: Bernstein for the difference of two independent means of 0 / 1 indicators (a per-pair difference in [-1, 1] with
    variance 2 pi (1 - pi), pi bounded above by the pooled frequency + 4 of its standard errors + 1 / n), failure probability 1e-9 per class."""
    w = _lvis_weight()
    C, n = w.numel(), 20_000
    labels = torch.tensor([1, 2, 3, 50, 51, 700, 1100, 1201])
    mask, n_chosen = FedClassSampler(50, w).sample(labels.to(DEV), n, generator=torch.Generator(device=DEV).manual_seed(23))
    _check_masks(mask, n_chosen, labels, w)
    prob = w.clone().to(DEV)
    prob[labels] = 0
    ref = torch.multinomial(prob[None].expand(n, C).contiguous(), 50 - labels.numel(), replacement=False,
                            generator=torch.Generator(device=DEV).manual_seed(29))
    ref_count = torch.zeros(C, dtype=torch.float64, device=DEV).index_add_(0, ref.reshape(-1), torch.ones(ref.numel(), dtype=torch.float64, device=DEV))
    ours = mask.double().sum(0)
    ours[labels.to(DEV)] = 0
    f1, f2 = (ours / n).cpu(), (ref_count / n).cpu()
    pooled = 0.5 * (f1 + f2)
    pi = (pooled + 4 * (pooled / n).sqrt() + 1.0 / n).clamp(max=0.5)
    v = 2 * pi * (1 - pi)
    L = math.log(2 / 1e-9)
    t = ((2 * L / 3) + ((2 * L / 3) ** 2 + 8 * n * L * v).sqrt()) / (2 * n)
    bad = ((f1 - f2).abs() > t).nonzero().flatten()
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] inclusion frequencies: max |ours - multinomial| {float((f1 - f2).abs().max()):.5f}, max / bound "
              f"{float(((f1 - f2).abs() / t).max()):.3f}", flush=True)
    assert bad.numel() == 0, [(int(c), float(f1[c]), float(f2[c]), float(t[c])) for c in bad[:10]]


def test_masked_focal_sum_against_the_reference_fed_loss():
    """criterion_fed_reference.npz: the reference's get_fed_loss_inds + sigmoid_focal_loss(src_logits[..., fed_ids], ...) * Q in float64,
    for < 50 appeared classes, >= 50, and none, matching- and denoising-part shaped: MaskedFocalNegativeSum (mask = the fixture's fed_ids) +
    FocalPositiveSum is that loss and gradient to 1e-5 relative; the gradient off the mask is exactly 0.  The logits off the fed columns do
    not enter the reference's loss: they are filled here with values of the test's own."""
    z = np.load(FIXTURE)
    g = torch.Generator(device=DEV).manual_seed(41)
    for case in ("few", "many", "empty"):
        for part in ("match", "dn"):
            k = f"{case}_{part}"
            ids = torch.from_numpy(z[f"{k}.fed_ids"]).to(DEV)
            tc = torch.from_numpy(z[f"{k}.target_classes"]).to(DEV)
            labels = torch.from_numpy(z[f"{k}.labels"])
            nb, want = float(z[f"{k}.num_boxes"]), float(z[f"{k}.loss"])
            want_g = torch.from_numpy(z[f"{k}.grad_fed"]).to(DEV).double()
            N, Q = tc.shape
            C = 1204
            # the reference's draw has the invariants of ours: every appeared class, max(50, a) classes in all
            a = int(torch.unique(labels).numel())
            assert ids.numel() == max(50, a) and set(labels.tolist()) <= set(ids.tolist()), k
            x = torch.randn(N, Q, C, device=DEV, generator=g) * 4
            x[..., ids] = torch.from_numpy(z[f"{k}.logits_fed"]).to(DEV)
            x.requires_grad_(True)
            mask = torch.zeros(1, C, device=DEV)
            mask[0, ids] = 1.0
            b, q = (tc < C).nonzero(as_tuple=True)
            loss = MaskedFocalNegativeSum.apply(x, torch.full((N, Q), 1.0 / nb, device=DEV), torch.zeros((N, Q), dtype=torch.int32, device=DEV),
                                                mask, 0.25) + \
                FocalPositiveSum.apply(x[b, q, tc[b, q]], torch.full((b.numel(),), 1.0 / nb, device=DEV), 0.25)
            loss.backward()
            assert abs(float(loss.detach()) - want) < 1e-5 * abs(want), (k, float(loss.detach()), want)
            gf = x.grad[..., ids].double()
            assert float((gf - want_g).abs().max()) < 1e-5 * float(want_g.abs().max()), k
            off = torch.ones(C, dtype=torch.bool, device=DEV)
            off[ids] = False
            assert bool((x.grad[..., off] == 0).all()), k


def test_all_ones_mask_gives_focal_negative_sum_bit_for_bit():
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(3, 2, 57, 1204, device=DEV, generator=g) * 6      # (incl. |x| > 20: softplus's linear branch)
    w = torch.rand(3, 2, 57, device=DEV, generator=g)
    w[0, 0, :5] = 0.0
    grp = torch.randint(0, 4, (3, 2, 57), device=DEV, generator=g, dtype=torch.int32)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la = FocalNegativeSum.apply(xa, w, 0.25)
    lb = MaskedFocalNegativeSum.apply(xb, w, grp, torch.ones(4, 1204, device=DEV), 0.25)
    (la * 1.3).backward()
    (lb * 1.3).backward()
    assert torch.equal(la, lb), (float(la), float(lb))
    assert torch.equal(xa.grad, xb.grad)
    # a 0 / 1 mask per group against the formula in float64; rows whose group is outside [0, groups) count nothing
    m = (torch.rand(4, 1204, device=DEV, generator=g) < 0.05).float()
    grp[1, 1, :7] = 4
    grp[2, 0, :3] = -1
    xc = x.clone().requires_grad_(True)
    lc = MaskedFocalNegativeSum.apply(xc, w, grp, m, 0.25)
    (lc * 0.7).backward()
    xd = x.double().requires_grad_(True)
    live = (grp >= 0) & (grp < 4)
    md = m.double()[grp.clamp(0, 3).long()] * live[..., None]
    p = xd.sigmoid()
    ld = (w.double()[..., None] * md * 0.75 * p * p * torch.nn.functional.softplus(xd)).sum()
    (ld * 0.7).backward()
    assert abs(float(lc) - float(ld)) < 1e-5 * abs(float(ld))
    assert float((xc.grad.double() - xd.grad).abs().max()) < 1e-5 * float(xd.grad.abs().max())
    assert bool((xc.grad[md == 0] == 0).all())


@pytest.mark.parametrize("C", [1, 255, 256, 257])
@pytest.mark.parametrize("rows", [1, 4097, 8193])
def test_all_ones_mask_bit_for_bit_where_a_workgroup_takes_a_second_row(rows, C):
    """The masked and the unmasked kernels at the shapes where their loops can drift apart: 4097 and 8193 rows are one past the grid caps of
    the sum kernel (4096) and of the gradient kernel (8192), so workgroup 0 takes a second row; C around 256 is the edge of the 256-thread
    column loop.  Rows 4096 and 8192 (the second rows) are live; every fifth row has weight 0."""
    g = torch.Generator(device=DEV).manual_seed(1000 * rows + C)
    G = 3
    x = torch.randn(rows, C, device=DEV, generator=g) * 6
    w = torch.rand(rows, device=DEV, generator=g) + 0.5
    w[3::5] = 0.0
    grp = torch.randint(0, G, (rows,), device=DEV, generator=g, dtype=torch.int32)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la = FocalNegativeSum.apply(xa, w, 0.25)
    lb = MaskedFocalNegativeSum.apply(xb, w, grp, torch.ones(G, C, device=DEV), 0.25)
    (la * 1.3).backward()
    (lb * 1.3).backward()
    assert torch.equal(la, lb), (float(la), float(lb))
    assert torch.equal(xa.grad, xb.grad)
    assert bool((xb.grad[w == 0] == 0).all()) and bool((xb.grad[w != 0] != 0).any())
    # a 0 / 1 mask, and rows whose group is outside [0, groups): exact zeros in the gradient there, something elsewhere
    m = (torch.rand(G, C, device=DEV, generator=g) < 0.5).float()
    m[0, 0] = 1.0
    grp2 = grp.clone()
    grp2[1::7] = G
    grp2[2::7] = -1
    grp2[rows - 1] = 0      # (the second row of workgroup 0 -- or the only row -- stays live)
    xc = x.clone().requires_grad_(True)
    (MaskedFocalNegativeSum.apply(xc, w, grp2, m, 0.25) * 1.3).backward()
    live = (grp2 >= 0) & (grp2 < G)
    md = m[grp2.clamp(0, G - 1).long()] * live[:, None]
    assert bool((xc.grad[md == 0] == 0).all())
    assert bool(xc.grad[rows - 1, 0] != 0) and bool(live.all()) == (rows == 1)
    # every row out of range: nothing is counted at all
    for dead in (G, -1):
        xd = x.clone().requires_grad_(True)
        ld = MaskedFocalNegativeSum.apply(xd, w, torch.full((rows,), dead, device=DEV, dtype=torch.int32), m, 0.25)
        ld.backward()
        assert float(ld) == 0.0 and bool((xd.grad == 0).all())


def _small_fed_step(seed=0):
    import bench_step
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, seed=seed, dev=torch.device(DEV, 0), fed_loss=True)
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    return model, images, mask, targets


def _sigmoid_focal_loss(inputs, targets, num_boxes, alpha=0.25, gamma=2):
    """the reference's formula (models/richsem/utils.py:82-108)"""
    import torch.nn.functional as F
    prob = inputs.sigmoid()
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = prob * targets + (1 - prob) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean(1).sum() / num_boxes


def _criterion_fed_op_by_op(model, fed, logits, coords, il, ib, clip_logits, t_logits, labels, boxes, m_dec, m_int, m_dis):
    """the criterion as the REFERENCE's loop over the outputs with use_fed_loss (richsem.py:956-961): every loss_labels call slices its
    logits and one-hot targets to its own fed_ids -- here the rows of ``fed``: layer l's matching part row l, its denoising part row 6 + l,
    the two-stage output row 12 -- and L1 + GIoU / KL as without it"""
    import torch.nn.functional as F
    from bench_step import box_cxcywh_to_xyxy, giou_pairs
    st = model.static
    dev = logits.device
    lay = st["lay"]
    pad, groups, single = lay["pad_size"], lay["num_dn_group"], lay["single_pad"]
    num_boxes = float(max(sum(st["known_num"]), 1))
    nl, N, C = logits.shape[0], logits.shape[1], logits.shape[-1]

    def loss_labels(src_logits, bi, si, tl, norm, row):
        ids = fed_ids(fed[row]).to(dev)
        target_classes = torch.full(src_logits.shape[:2], C, dtype=torch.int64, device=dev)
        target_classes[bi, si] = tl
        onehot = torch.zeros(src_logits.shape[:2] + (C + 1,), dtype=src_logits.dtype, device=dev)
        onehot.scatter_(2, target_classes.unsqueeze(-1), 1)
        onehot = onehot[:, :, :-1]
        return _sigmoid_focal_loss(src_logits[..., ids], onehot[..., ids], norm) * src_logits.shape[1]

    def loss_boxes(pb, tb, norm):
        return (5.0 * (pb - tb).abs().sum() + 2.0 * (1 - giou_pairs(box_cxcywh_to_xyxy(pb), box_cxcywh_to_xyxy(tb))).sum()) / norm

    li, bi, si, tj = m_dec
    pos_slots = (torch.arange(groups, device=dev)[:, None] * 2 * single + torch.arange(single, device=dev)[None]).flatten()
    dn_b = torch.arange(N, device=dev)[:, None].expand(N, pos_slots.numel()).reshape(-1)
    dn_q = pos_slots[None].expand(N, -1).reshape(-1)
    dn_lab = labels.view(N, -1).repeat(1, groups).reshape(-1)
    dn_box = boxes.view(N, -1, 4).repeat(1, groups, 1).reshape(-1, 4)
    nbx = num_boxes * groups
    loss = 0.0
    for l in range(nl):
        k = li == l
        loss = loss + loss_labels(logits[l][:, pad:], bi[k], si[k], labels[tj[k]], num_boxes, l)
        loss = loss + loss_boxes(coords[l][bi[k], si[k] + pad], boxes[tj[k]], num_boxes)
        loss = loss + loss_labels(logits[l][:, :pad], dn_b, dn_q, dn_lab, nbx, nl + l)
        loss = loss + loss_boxes(coords[l][dn_b, dn_q], dn_box, nbx)
    _, bi, si, tj = m_int
    loss = loss + loss_labels(il, bi, si, labels[tj], num_boxes, 2 * nl) + loss_boxes(ib[bi, si], boxes[tj], num_boxes)
    _, bi, si, tj = m_dis
    return loss + 0.5 * F.kl_div(F.log_softmax(clip_logits[bi, si + pad], -1), F.softmax(t_logits[tj], -1), reduction="batchmean")


def test_fed_step_criterion_is_the_reference_loss_with_fed_ids():
    """Step(fed_loss=True).loss_part on frozen masks against the reference's per-output loss_labels with the fed_ids slicing (and the
    other terms as the reference forms them): loss to 1e-5 relative, gradients w.r.t. every input as tests/test_gpu_step.py holds the
    unmasked form.  Unfrozen, every call draws fresh masks for the batch's target classes."""
    model, images, mask, targets = _small_fed_step(seed=2)
    labels = torch.cat([t["labels"] for t in targets])
    with torch.no_grad():
        outs = model.model_part(images, mask)
    idx = model.pack_indices(model.match(*outs[:4], targets), targets)
    # fresh draws per call: 13 masks with the invariants, different from the previous call's
    model.loss_part(*outs, *idx)
    first = model.last_fed_mask.clone()
    model.loss_part(*outs, *idx)
    assert first.shape == (13, 1204) and not torch.equal(first, model.last_fed_mask)
    _check_masks(first, first.sum(1).int(), labels, model.fed_sampler.class_weight)
    model.freeze_fed(11)
    fed = model.frozen_fed
    assert fed.shape == (13, 1204)
    res = []
    for fn in (model.loss_part, lambda *a: _criterion_fed_op_by_op(model, fed, *a)):
        leaves = [o.detach().clone().requires_grad_(i < 5) for i, o in enumerate(outs)]
        loss = fn(*leaves, *idx)
        loss.backward()
        res.append((loss.detach(), [t.grad for t in leaves[:5]]))
    assert model.last_fed_mask is fed
    (la, ga), (lb, gb) = res
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] fed criterion: loss_part {float(la):.7g} op-by-op {float(lb):.7g}", flush=True)
    assert abs(float(la) - float(lb)) < 1e-5 * abs(float(lb)), (float(la), float(lb))
    for a, b in zip(ga, gb):
        assert float((a - b).abs().max()) < 2e-5 * float(b.abs().max()) + 1e-12, float((a - b).abs().max()) / float(b.abs().max())
    # the masked-out classes of the matching and two-stage logits get no gradient at all
    assert bool((ga[0][0][:, model.static["lay"]["pad_size"]:][..., fed[0] == 0] == 0).all())
    assert bool((ga[2][..., fed[12] == 0] == 0).all())


def test_graphed_fed_step_draws_fresh_masks_and_matches_the_eager_step():
    """bench_step.run_graphed(fed_loss=True): the class draw is captured with the criterion (no host sync: a synchronising call inside the
    capture fails it; no warning), every replay draws new masks; with freeze_fed the first replay's loss is the eager step's on the same
    parameters, noise, masks, two-stage selection and assignment.  Bound: the relative gap of tests/test_gpu_step.py's graphed-vs-eager
    comparison of the unmasked step (2e-3).  The masks are frozen and the masked kernels have no atomics, so the federated loss adds nothing
    to the gap; what is left is the bf16 step itself, which is not bit-reproducible from run to run: measured on MI355X, the gap was 0 and
    1.1e-5 in two runs of this file alone and 3.9e-5 inside the whole GPU suite."""
    import bench_step
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = bench_step.run_graphed(2, torch.device(DEV, 0), steps=1, warmup=0, optimizer=False, return_model=True, height=H, width=W_IMG,
                                     boxes_per_image=BOXES, seed=0, fed_loss=True)
        model = res["model"]
        m1 = model.last_fed_mask.clone()
        res["step"]()
        m2 = model.last_fed_mask.clone()
    noisy = [str(w.message)[:160] for w in caught if "AccumulateGrad" in str(w.message) or "sync" in str(w.message).lower()]
    assert not noisy, noisy
    labels = torch.cat([t["labels"] for t in model._targets])
    assert not torch.equal(m1, m2)
    for m in (m1, m2):
        _check_masks(m, m.sum(1).int(), labels, model.fed_sampler.class_weight)
    del res, model
    torch.cuda.empty_cache()
    # frozen masks: the graphed step's loss against the eager one
    res = bench_step.run_graphed(2, torch.device(DEV, 0), steps=1, warmup=0, optimizer=False, noise_seed=3, fed_seed=5, return_grads=True,
                                 height=H, width=W_IMG, boxes_per_image=BOXES, seed=0, fed_loss=True)
    model, images, mask, targets = _small_fed_step(seed=0)
    model.freeze_noise(3)
    model.freeze_fed(5)
    for p in model.parameters():
        p.grad = None
    loss = model(images, mask, targets, res["indices"], res["topk"])
    gap = abs(res["loss"] - float(loss)) / abs(float(loss))
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] graphed fed step loss {res['loss']:.8g} eager {float(loss):.8g} relative gap {gap:.3g}", flush=True)
    assert gap < 2e-3, (res["loss"], float(loss))
