"""The loss and matcher kernels against the element-wise bounds and exact probes of tests/loss_ref.py (derivation: its docstring), called
through the project's wrappers: ``matcher.FocalNegativeSum`` / ``FocalPositiveSum`` / ``BoxPairLoss``, ``fed_loss.MaskedFocalNegativeSum``,
``matcher.cost_blocks`` (both layouts, f32 and f64) and ``criterion.device_criterion`` / ``device_criterion_and_grads`` (and their
``device_set_*`` forms for flags bit 0 and the row groups).  One ``ratio`` line per call: worst |kernel - restatement| / bound, <= 1 for
f32 and <= 2 for f64; probes compare bits or closed forms.  tests/test_loss_ref.py shows on the CPU that a float32 evaluation meets the
same bounds on the same inputs and that the wrong variants do not.  Measured figures: profiles/r25_loss_bounds.md."""
import functools

import numpy as np
import pytest
import torch

from richsem_amd import criterion as CR
from richsem_amd.fed_loss import MaskedFocalNegativeSum
from richsem_amd.matcher import BoxPairLoss, FocalNegativeSum, FocalPositiveSum, TargetBuffers, cost_blocks

import loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GS = 1.7
W_CLASS, W_BBOX, W_GIOU = 2.0, 5.0, 2.0


def _r(name, got, ref, limit=1.0):
    r = R.ratio(got, ref)
    print(f"ratio {name}: {r:.3g}")
    assert r <= limit, (name, r)


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _neg(x, w, group=None, mask=None, gs=GS):
    """the plain or the masked all-negative kernels through their wrappers: -> (loss, grad) on the host"""
    xd = x.to(DEV).requires_grad_(True)
    if mask is None:
        loss = FocalNegativeSum.apply(xd, w.to(DEV), R.ALPHA)
    else:
        loss = MaskedFocalNegativeSum.apply(xd, w.to(DEV), group.to(DEV), mask.to(DEV), R.ALPHA)
    loss.backward(torch.tensor(gs, device=DEV))
    return loss.detach().cpu(), xd.grad.cpu()


@functools.lru_cache(maxsize=None)
def _neg_case(rows, C):
    x, w, grp, mask = R.neg_inputs(rows, C)
    return x, w, grp, mask, R.focal_neg(x, w, R.ALPHA, GS, R.B32), R.focal_neg(x, w, R.ALPHA, GS, R.B32, group=grp, mask=mask)


# ---- the all-negative kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", R.NEG_SHAPES)
def test_all_negative_kernels_inside_the_bounds(rows, C):
    x, w, grp, mask, ref, ref_m = _neg_case(rows, C)
    loss, grad = _neg(x, w)
    _r(f"focal_neg_sum_f32 {rows}x{C}", loss, ref[0])
    _r(f"focal_neg_grad_f32 {rows}x{C}", grad, ref[1])
    loss_m, grad_m = _neg(x, w, grp, mask)
    _r(f"focal_neg_sum_masked_f32 {rows}x{C}", loss_m, ref_m[0])
    _r(f"focal_neg_grad_masked_f32 {rows}x{C}", grad_m, ref_m[1])
    # an all-ones mask gives the plain kernel's bits (the claim in msda_fed.h)
    loss_1, grad_1 = _neg(x, w, torch.ones(rows, dtype=torch.int32), torch.ones(3, C))
    assert torch.equal(_bits(loss_1), _bits(loss)) and torch.equal(_bits(grad_1), _bits(grad))


@pytest.mark.parametrize("rows,C,hot", [
    (8200, 3, [(0, 0), (0, 2), (4096, 1), (8192, 1), (8199, 2)]),      # first / last row and class; the first row of the second grid
    (5, 1203, [(0, 255), (1, 256), (2, 257), (3, 1202), (4, 0)]),      # stride of the sum (4096) and of the gradient (8192)
])
def test_all_negative_selection_probes(rows, C, hot):
    """every logit -200 (its term and its gradient are exactly 0) except one per probed row: the loss is the sum of
    fl(fl(term) w_row) (1 - alpha) to the single-term bounds, every other gradient element is exactly 0"""
    x = torch.full((rows, C), -200.0)
    w = 2.0 ** -(torch.arange(rows) % 8).float()
    vals = [1.5, -2.25, 0.75, -0.5, 3.0]
    for (r, c), v in zip(hot, vals):
        x[r, c] = v
    rr, cc = torch.tensor([h[0] for h in hot]), torch.tensor([h[1] for h in hot])
    term, dterm = R.focal_neg_term(R.B32.lift(torch.tensor(vals)), R.B32)
    single = (term * R.B32.lift(w[rr]))
    want = R._to_f32(R._sum_f64(single) * (1.0 - R.ALPHA), R.B32)
    for masked in (False, True):
        grp, mask = (torch.ones(rows, dtype=torch.int32), torch.ones(2, C)) if masked else (None, None)
        loss, grad = _neg(x, w, grp, mask, gs=1.0)
        _r(f"selection {rows}x{C} masked {masked} loss", loss, want)
        g_hot = dterm * (R.B32.lift(w[rr]) * (1.0 - R.ALPHA))
        _r(f"selection {rows}x{C} masked {masked} hot gradients", grad[rr, cc], g_hot)
        rest = grad.clone()
        rest[rr, cc] = 0.0
        assert int((_bits(rest) != 0).sum()) == 0


def test_all_negative_zeros_are_exact():
    """weight 0, a row group outside [0, groups) and a masked class: gradient bits 0, and the loss bit-equal with those entries NaN / 1e30"""
    x, w, grp, mask, _, _ = _neg_case(5, 257)
    w, grp = w.clone(), grp.clone()
    w[2], grp[0], grp[4] = 0.0, 2, 0      # row 0: the random mask, row 1: group -1, row 2: weight 0, row 3: group 3, row 4: the empty mask
    loss, grad = _neg(x, w)
    assert int((_bits(grad[2]) != 0).sum()) == 0
    for poison in (float("nan"), 1e30):
        xp = x.clone()
        xp[2] = poison
        loss_p, grad_p = _neg(xp, w)
        assert torch.equal(_bits(loss_p), _bits(loss)) and torch.equal(_bits(grad_p), _bits(grad))
    loss, grad = _neg(x, w, grp, mask)
    dead = (w == 0)[:, None] | ((grp < 0) | (grp >= 3))[:, None] | (mask[grp.clamp(0, 2).long()] == 0)
    assert bool(dead[1:].all()) and 0 < int(dead[0].sum()) < dead.shape[1]
    assert int((_bits(grad)[dead] != 0).sum()) == 0
    for poison in (float("nan"), 1e30):
        xp = torch.where(dead, torch.full_like(x, poison), x)
        loss_p, grad_p = _neg(xp, w, grp, mask)
        assert torch.equal(_bits(loss_p), _bits(loss)) and torch.equal(_bits(grad_p), _bits(grad))


# ---- the pair kernels --------------------------------------------------------------------------------------------------------------------------
def _pair(p, t, w, c_l1, c_giou):
    pd = p.to(DEV).requires_grad_(True)
    loss = BoxPairLoss.apply(pd, t.to(DEV), w.to(DEV), c_l1, c_giou)
    loss.backward()
    return loss.detach().cpu(), pd.grad.cpu()


def _pos(x, w):
    xd = x.to(DEV).requires_grad_(True)
    loss = FocalPositiveSum.apply(xd, w.to(DEV), R.ALPHA)
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


@pytest.mark.parametrize("K", R.PAIR_K)
def test_pair_kernels_inside_the_bounds(K):
    pb, tb, w, x = R.pair_inputs(K)
    for c in R.PAIR_COEF:
        ref = R.box_pair(pb, tb, w, *c, R.B32)
        loss, grad = _pair(pb, tb, w, *c)
        _r(f"box_pair_loss_f32 K {K} c {c} loss", loss, ref[0])
        _r(f"box_pair_loss_f32 K {K} c {c} grad", grad, ref[1])
    ref = R.focal_pos(x, w, R.ALPHA, R.B32)
    loss, grad = _pos(x, w)
    _r(f"focal_pos_sum_f32 K {K} loss", loss, ref[0])
    _r(f"focal_pos_sum_f32 K {K} grad", grad, ref[1])


def test_kink_boxes_equal_autograd():
    """the dyadic kink pairs (identical, touching, shared edges, nested, disjoint, zero width / height, p == t in one coordinate): the
    gradients element-wise against torch's CPU float64 autograd of the restated box_ops formulas -- the comparison
    tests/test_gpu_step.py leaves out with rows[:5] = False --, and with c_giou = 0 bit for bit"""
    names, kp, kt = R.kink_boxes()
    w = 2.0 ** -(torch.arange(len(names)) % 4).float()
    ref = R.box_pair(kp, kt, w, 5.0, 2.0, R.B32)
    want_l, want_g = R.box_pair_autograd(kp, kt, w, 5.0, 2.0)
    # (the restatement holds 1e-6 as a float32, autograd as a double: 1e-13 of the gradient apart)
    assert float((ref[1].v - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())
    loss, grad = _pair(kp, kt, w, 5.0, 2.0)
    for i, n in enumerate(names):
        e = (grad[i].double() - want_g[i]).abs()
        print(f"kink {n}: worst |err| / bound {float((e / ref[1].e[i].clamp(min=1e-300)).max()):.3g}")
    _r("kink pairs grad against autograd", grad, R.B(want_g, ref[1].e + 1e-12 * want_g.abs(), R.B32))
    _r("kink pairs loss against autograd", loss, R.B(want_l, ref[0].e + 1e-12 * want_l.abs(), R.B32))
    want_l, want_g = R.box_pair_autograd(kp, kt, w, 1.0, 0.0)
    loss, grad = _pair(kp, kt, w, 1.0, 0.0)
    assert torch.equal(grad.double(), want_g) and float(loss) == float(want_l)      # +-c_l1 w or 0, and an exact sum
    assert set(torch.unique(grad.abs() / w[:, None]).tolist()) <= {0.0, 1.0}


def test_softplus_branch_and_saturation_probes():
    x, w = torch.tensor(R.EXPLICIT), torch.ones(len(R.EXPLICIT))
    ref = R.focal_pos(x, w, R.ALPHA, R.B32)
    loss, grad = _pos(x, w)
    _r("probes focal_pos loss", loss, ref[0])
    _r("probes focal_pos grad", grad, ref[1])
    refn = R.focal_neg(x[:, None], w, R.ALPHA, 1.0, R.B32)
    loss_n, grad_n = _neg(x[:, None].contiguous(), w, gs=1.0)
    for i, v in enumerate(R.EXPLICIT):
        print(f"logit {v:+.9g}: pos |err| / bound {abs(float(grad[i]) - float(ref[1].v[i])) / max(float(ref[1].e[i]), 1e-300):.3g}, "
              f"neg {abs(float(grad_n[i, 0]) - float(refn[1].v[i, 0])) / max(float(refn[1].e[i, 0]), 1e-300):.3g}")
    _r("probes focal_neg loss", loss_n, refn[0])
    _r("probes focal_neg grad", grad_n, refn[1])
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(grad_n).all())


# ---- the matcher's cost ------------------------------------------------------------------------------------------------------------------------
SENTINEL = -777.25


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("saturated", [False, True], ids=["n02", "saturated"])
@pytest.mark.parametrize("counts", R.MATCHER_COUNTS)
def test_matcher_cost_inside_the_bounds(counts, saturated, dtype):
    lg, bx, lab, tb, off = R.matcher_inputs(counts, saturated, dtype)
    mode, limit = (R.B32, 1.0) if dtype == torch.float32 else (R.B64, 2.0)
    blocks = R.matcher_blocks(lg, bx, lab, tb, off, W_CLASS, W_BBOX, W_GIOU, R.ALPHA, mode)
    Q, total, cap = lg.shape[1], int(off[-1]), int(off[-1]) + 5
    targets = [{"labels": lab[off[b]: off[b + 1]], "boxes": tb[off[b]: off[b + 1]]} for b in range(len(counts))]
    bufs = TargetBuffers(len(counts), cap, DEV, dtype).update_(targets)
    with torch.no_grad():      # capacity rows past the live targets are never read
        bufs.tgt_ids[total:] = 10 ** 12
        bufs.tgt_boxes[total:] = float("nan")
    outs = {}
    for tm in (False, True):
        out = torch.full((Q * cap,), SENTINEL, dtype=dtype, device=DEV)
        cost_blocks(lg.to(DEV), bx.to(DEV), bufs, W_CLASS, W_BBOX, W_GIOU, R.ALPHA, out=out, target_major=tm)
        out = out.cpu()
        assert bool((out[Q * total:] == SENTINEL).all())      # cost elements past Q * tgt_offsets[B] keep the sentinel
        _r(f"matcher_cost{'_tm' if tm else ''}_{'f32' if dtype == torch.float32 else 'f64'} {counts} saturated {saturated}",
           out[:Q * total], R.flat_blocks(blocks, tm), limit)
        outs[tm] = out
    for b in range(len(counts)):      # the two layouts hold the same bits per entry; NaN in exactly the bad label's column
        n = int(off[b + 1] - off[b])
        rm = outs[False][Q * off[b]: Q * off[b + 1]].view(Q, n)
        tmj = outs[True][Q * off[b]: Q * off[b + 1]].view(n, Q).t()
        assert torch.equal(_bits(rm), _bits(tmj))
        bad = (lab[off[b]: off[b + 1]] < 0) | (lab[off[b]: off[b + 1]] >= lg.shape[2])
        assert torch.equal(torch.isnan(rm), bad[None, :].expand(Q, -1))


# ---- the criterion over capacity buffers -------------------------------------------------------------------------------------------------------
def _layout(nl, N, Q, Qi, cap, pad_cap):
    """csrc/msda_criterion.h crit_layout: -> (slots, byte offsets of the records gb, gx, row, label in the workspace)"""
    S = (nl + 1) * cap + nl * N * pad_cap
    grid_pairs = (nl + 1) * ((cap + 255) // 256) + nl * ((N * pad_cap + 255) // 256)
    off_gb = 0
    off_gx = S * 16 + grid_pairs * 3 * 8
    return S, off_gb, off_gx, off_gx + S * 4, off_gx + 2 * S * 4


def _crit_device(variant):
    a, kw, z = R.crit_args(variant)
    logits, coords, il, ib, cum, ids, boxes, qot, meta, nb, pad_cap = a
    N, total = len(z["counts"]), int(cum[-1])
    targets = [{"labels": ids[cum[b]: cum[b + 1]], "boxes": boxes[cum[b]: cum[b + 1]]} for b in range(N)]
    bufs = TargetBuffers(N, z["cap"], DEV).update_(targets)
    dev = dict(logits=logits.to(DEV), coords=coords.to(DEV), il=il.to(DEV), ib=ib.to(DEV), bufs=bufs, qot=qot.to(DEV),
               meta=None if meta is None else torch.as_tensor(meta, device=DEV),
               nb=None if nb is None else torch.tensor([nb], dtype=torch.float32, device=DEV),
               mask=kw["class_mask"].to(DEV) if "class_mask" in kw else None, agn=bool(kw.get("flags", 0) & 1), pad_cap=pad_cap)
    return dev, z


def _crit_run(d, grad_loss=None):
    """-> (loss, terms, status, grads) through device_criterion_and_grads, or its device_set_ form where a switch is on"""
    args = (d["logits"], d["coords"], d["il"], d["ib"], d["bufs"], d["qot"], d["meta"])
    if d["mask"] is None and not d["agn"]:
        loss, terms, status, grads = CR.device_criterion_and_grads(*args, pad_cap=d["pad_cap"], num_boxes=d["nb"], grad_loss=grad_loss)
    else:
        loss, terms, status, _, grads = CR.device_set_criterion_and_grads(*args, pad_cap=d["pad_cap"], num_boxes=d["nb"], fed=d["mask"],
                                                                          enc_cls_agn=d["agn"], grad_loss=grad_loss)
    torch.cuda.synchronize()
    return loss, terms, status, dict(zip(("logits", "coords", "il", "ib"), grads))


@pytest.mark.parametrize("variant", list(R.CRIT_VARIANTS))
def test_criterion_pairs_inside_the_bounds(variant):
    d, z = _crit_device(variant)
    ref = R.crit_ref(variant)
    nl, N, Q, Qi, C, groups = z["dims"]
    loss, terms, status, grads = _crit_run(d)
    assert status.tolist() == ref["status"]
    _r(f"criterion_pairs {variant} terms", terms, ref["terms"])
    _r(f"criterion_pairs {variant} loss", loss, ref["loss"])
    for k in ("logits", "coords", "il", "ib"):
        _r(f"criterion_pairs_backward {variant} grad_{k}", grads[k].reshape(ref["grads"][k].shape), ref["grads"][k])
    # bit-equal with a second run
    loss2, terms2, status2, grads2 = _crit_run(d)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(terms2), _bits(terms)) and torch.equal(status2, status)
    for k in grads:
        assert torch.equal(_bits(grads2[k]), _bits(grads[k])), k
    # scaling gscale by a power of two scales every gradient bit-exactly (nothing here is near the subnormals)
    _, _, _, grads4 = _crit_run(d, grad_loss=torch.tensor([4.0], device=DEV))
    for k in grads:
        assert torch.equal(_bits(grads4[k]), _bits(grads[k] * 4.0)), k
    # the autograd form: the same launches, the same bits
    if d["mask"] is None and not d["agn"]:
        leaves = [d[k].clone().requires_grad_(True) for k in ("logits", "coords", "il", "ib")]
        la, ta, sa = CR.device_criterion(*leaves, d["bufs"], d["qot"], d["meta"], pad_cap=d["pad_cap"], num_boxes=d["nb"])
        la.backward()
        assert torch.equal(_bits(la), _bits(loss)) and torch.equal(_bits(ta), _bits(terms)) and torch.equal(sa, status)
        for leaf, k in zip(leaves, ("logits", "coords", "il", "ib")):
            assert torch.equal(_bits(leaf.grad), _bits(grads[k])), k
    # the slot space and the row weights / groups: the forward half called as device_set_criterion does, for what it keeps for the backward
    args = CR._checked(d["logits"], d["coords"], d["il"], d["ib"], d["bufs"], d["qot"], d["meta"], d["pad_cap"], R.ALPHA, 1.0, 5.0, 2.0,
                       d["nb"], False, False, False)
    mask = d["mask"] if d["mask"] is not None else torch.ones(2 * nl + 1, C, device=DEV)      # (row groups requested)
    _, terms_g, _, saved = CR.set_criterion_forward(*args, mask, d["agn"])
    x, xi, w_rows, w_int, ws, cum, dims, alpha, c_cls, g_rows, g_int, _ = saved
    torch.cuda.synchronize()
    assert np.array_equal(w_rows.cpu().numpy(), ref["row_weight"]) and np.array_equal(w_int.cpu().numpy(), ref["row_weight_int"])
    assert np.array_equal(g_rows.cpu().numpy(), ref["row_group"]) and np.array_equal(g_int.cpu().numpy(), ref["row_group_int"])
    assert torch.equal(_bits(terms_g), _bits(terms))      # the pair terms do not depend on the mask
    S, off_gb, off_gx, off_row, off_label = _layout(nl, N, Q, Qi, z["cap"], d["pad_cap"])
    raw = ws.cpu()
    rec_row = raw[off_row: off_row + 4 * S].view(torch.int32).numpy()
    rec_label = raw[off_label: off_label + 4 * S].view(torch.int32).numpy()
    rec_gx = raw[off_gx: off_gx + 4 * S].view(torch.float32)
    rec_gb = raw[off_gb: off_gb + 16 * S].view(torch.float32).view(S, 4)
    assert np.array_equal(rec_row, ref["rows"]) and np.array_equal(rec_label, ref["labels"])
    dead = torch.as_tensor(ref["rows"] < 0)
    assert int((_bits(rec_gx)[dead] != 0).sum()) == 0 and int((_bits(rec_gb)[dead] != 0).sum()) == 0
    _r(f"criterion_pairs {variant} rec_gx", rec_gx, ref["rec_gx"])
    _r(f"criterion_pairs {variant} rec_gb", rec_gb, R.B(torch.stack([c.v for c in ref["rec_gb"]], 1), torch.stack([c.e for c in ref["rec_gb"]], 1), R.B32))
