"""CPU: the distillation term's host side (richsem_amd/distill.py; ABI v12) -- the three entry points refuse bad arguments before any launch,
DistillLoss refuses what the reference's branches do not have, and the fixture made from the reference's own ``loss_labels``
(tests/golden/criterion_distill_reference.npz, make_golden_distill.py) agrees with a float64 restatement of the formulas of
include/richsem_msda.h written here: yardstick and specification say the same thing.  tests/test_gpu_distill.py imports the restatement."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from richsem_amd import _lib
from richsem_amd.distill import DistillKL, DistillL1, DistillLoss

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_distill_reference.npz")
EPS32 = 2.0 ** -24


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------------------
def restate_kl(pred, tgt, pred_row, tgt_row, weight, subset=None, dynamic=False):
    """The KL form in float64 from the formulas: per row k, S_k = ``subset[k]`` (K, C) bool (None: every class),
    p = softmax(pred row over S_k), t = softmax(tgt row over S_k), dw = 1 or 2 H(softmax(tgt row over all C)) / ln C,
    row_loss = w dw sum_S t (log t - log p), grad_rows = w dw (p - t) on S_k and 0 elsewhere; 0 * log 0 = 0 throughout.
    Returns a dict: loss, row_loss (K), grad_rows (K, C), and what the rounding bound of the GPU test is made of -- p, t (0 off S_k), dw (K),
    R (K): the larger range of the two rows over S_k, and of the whole teacher row when the weight is dynamic."""
    x, y, w = pred.double()[pred_row], tgt.double()[tgt_row], weight.double()
    K, C = x.shape
    S = torch.ones((K, C), dtype=torch.bool) if subset is None else subset.bool()
    ninf = torch.full((), -math.inf, dtype=torch.float64)

    def log_softmax_over(v, sel):
        vm = torch.where(sel, v, ninf)
        mx = vm.max(-1, keepdim=True).values
        d = vm - mx
        return d - d.exp().sum(-1, keepdim=True).log()

    lp, lt = log_softmax_over(x, S), log_softmax_over(y, S)
    p, t = lp.exp(), lt.exp()
    zero = torch.zeros((), dtype=torch.float64)
    kl = torch.where(S & (t > 0), t * (lt - lp), zero).sum(-1)
    dw = torch.ones(K, dtype=torch.float64)
    if dynamic:
        la = log_softmax_over(y, torch.ones_like(S))
        ta = la.exp()
        dw = 2.0 * torch.where(ta > 0, -ta * la, zero).sum(-1) / math.log(C)
    grad = torch.where(S, (w * dw)[:, None] * (p - t), zero)
    rng = lambda v, sel: (torch.where(sel, v, ninf).max(-1).values - torch.where(sel, v, -ninf).min(-1).values)
    R = torch.maximum(rng(x, S), rng(y, S))
    if dynamic:
        R = torch.maximum(R, rng(y, torch.ones_like(S)))
    row_loss = w * dw * kl
    return {"loss": row_loss.sum(), "row_loss": row_loss, "grad_rows": grad, "p": torch.where(S, p, zero), "t": torch.where(S, t, zero), "dw": dw, "R": R}


def restate_l1(pred, tgt, pred_row, tgt_row, weight, normalize_target):
    """The L1 form in float64: u = pred row / |pred row|_2, v = tgt row (or over its norm), row_loss = w |u - v|_1,
    grad_rows = w (s - u (u . s)) / |pred row|_2 with s = sign(u - v).  Returns loss, row_loss, grad_rows, u, norm (K)."""
    x, y, w = pred.double()[pred_row], tgt.double()[tgt_row], weight.double()
    nu = (x * x).sum(-1, keepdim=True).sqrt()
    u = x / nu
    v = y / (y * y).sum(-1, keepdim=True).sqrt() if normalize_target else y
    s = torch.sign(u - v)
    row_loss = w * (u - v).abs().sum(-1)
    grad = w[:, None] * (s - u * (u * s).sum(-1, keepdim=True)) / nu
    return {"loss": row_loss.sum(), "row_loss": row_loss, "grad_rows": grad, "u": u, "norm": nu[:, 0]}


def fixture_cases():
    """every case of the fixture as a dict: its name, the restatement's arguments for it ("kw": CPU tensors, float32 inputs, the row weights
    1 / num_boxes or 1 / (bs nq) in float64 as the reference divides -- the device takes them rounded to float32), the class mask of the fed
    cases, the stored loss and gradient rows"""
    z = np.load(FIXTURE)
    t = lambda k: torch.from_numpy(z[k])
    b, s, tj, nb = t("batch_idx"), t("src_idx"), t("tgt_idx"), float(z["num_boxes"])
    cases = []
    for kind, student, out_teacher, gt_teacher in (("kl", "kl.student", "kl.teacher_out", "kl.teacher_gt"), ("l1", "l1.student", "l1.prompt_out", "l1.prompt_gt")):
        st = t(student)
        N, Q, C = st.shape
        rows = b * Q + s
        variants = [("_dyn0", False, False), ("_dyn1", True, False)] if kind == "kl" else [("", False, False)]
        for objective in ("gt", "pred", "pred_all"):
            for sfx, dynamic, fed in variants + ([("_fed", objective == "gt", True)] if kind == "kl" and objective != "pred_all" else []):
                name = f"{kind}_{objective}{sfx}"
                if objective == "pred_all":
                    pr = tr = torch.arange(N * Q)
                    tgt, w = t(out_teacher).reshape(N * Q, C), torch.full((N * Q,), 1.0 / (N * Q), dtype=torch.float64)
                elif objective == "pred":
                    pr, tr, tgt, w = rows, rows, t(out_teacher).reshape(N * Q, C), torch.full((rows.numel(),), 1.0 / nb, dtype=torch.float64)
                else:
                    pr, tr, tgt, w = rows, tj, t(gt_teacher), torch.full((rows.numel(),), 1.0 / nb, dtype=torch.float64)
                kw = {"pred": st.reshape(N * Q, C), "tgt": tgt, "pred_row": pr, "tgt_row": tr, "weight": w}
                mask = None
                if kind == "kl":
                    kw["dynamic"] = dynamic
                    if fed:
                        mask = torch.zeros(C)
                        mask[t(f"{name}.fed_ids")] = 1.0
                        kw["subset"] = mask.bool()[None].expand(pr.numel(), C)
                else:
                    kw["normalize_target"] = objective != "gt"
                cases.append({"name": name, "kind": kind, "objective": objective, "kw": kw, "mask": mask, "loss": float(z[f"{name}.loss"]),
                              "grad": t(f"{name}.grad").reshape(-1, C), "shape": (N, Q, C), "num_boxes": nb,
                              "batch_idx": b, "src_idx": s, "tgt_idx": tj})
    return cases


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------
def test_distill_entry_points_check_their_arguments_on_the_host():
    L = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def kl(name, pred=p, pred_rows=8, tgt=p, tgt_rows=8, C=1204, pred_row=p, tgt_row=p, w=p, K=4, grp=None, mask=None, groups=0, dyn=0, ws=p, loss=p, grad=p):
        return getattr(L, name)(pred, pred_rows, tgt, tgt_rows, C, pred_row, tgt_row, w, K, grp, mask, groups, dyn, ws, loss, grad, None)

    def l1(name, pred=p, pred_rows=8, tgt=p, tgt_rows=8, C=1024, pred_row=p, tgt_row=p, w=p, K=4, norm=0, ws=p, loss=p, grad=p):
        return L.msda_distill_l1_f32(pred, pred_rows, tgt, tgt_rows, C, pred_row, tgt_row, w, K, norm, ws, loss, grad, None)

    for name, call in (("msda_distill_kl_f32", kl), ("msda_distill_kl_bf16", kl), ("msda_distill_l1_f32", l1)):
        def refused(code, **kw):
            assert call(name, **kw) == code, (name, kw)
            assert _lib.last_error().startswith(name + ":"), (name, kw, _lib.last_error())

        for arg in ("pred", "tgt", "pred_row", "tgt_row", "w", "ws", "loss", "grad"):
            refused(-1, **{arg: None})                                      # MSDA_ERR_NULL_POINTER
        for kw in ({"K": -1}, {"C": 0}, {"C": -3}, {"pred_rows": -1}, {"tgt_rows": -1}):
            refused(-2, **kw)                                               # MSDA_ERR_BAD_DIMS
        for arg, off in (("tgt", 2), ("w", 2), ("loss", 2), ("grad", 2), ("pred_row", 4), ("tgt_row", 4), ("ws", 4), ("pred", 1 if name.endswith("bf16") else 2)):
            refused(-5, **{arg: p + off})                                   # MSDA_ERR_MISALIGNED
        if call is kl:
            refused(-2, C=1, dyn=1)                                         # the dynamic weight divides by ln C
            refused(-2, dyn=2)
            refused(-2, mask=p, grp=p, groups=0)                            # a mask without groups
            refused(-1, mask=None, grp=p, groups=3)                         # groups without a mask
            refused(-1, mask=p, grp=None, groups=3)                         # a mask without the rows' groups
            refused(-2, groups=-1)
            refused(-5, mask=p + 2, grp=p, groups=3)
            refused(-5, mask=p, grp=p + 2, groups=3)
        else:
            refused(-2, norm=2)
        with pytest.raises(RuntimeError, match=name + ".*BAD_DIMS"):
            _lib.check(call(name, C=0))


def test_workspace_size_is_the_header_s():
    import re
    from conftest import ROOT
    m = re.search(r"#define MSDA_DISTILL_WORKSPACE_BYTES (\d+)", open(os.path.join(ROOT, "include", "richsem_msda.h")).read())
    assert int(m.group(1)) == _lib.DISTILL_WORKSPACE_BYTES and _lib.DISTILL_WORKSPACE_BYTES % 8 == 0


def test_distill_loss_refuses_what_the_reference_does_not_have():
    with pytest.raises(NotImplementedError):
        DistillLoss("l2", "gt")                                             # the reference: raise NotImplementedError
    with pytest.raises(NotImplementedError):
        DistillLoss("clip_logits", "matched")
    x = torch.randn(2, 6, 8)
    rows, w = torch.arange(3), torch.ones(3)
    for typ in ("clip_logits", "clip_l1"):
        for objective in ("gt", "pred", "pred_all"):
            d = DistillLoss(typ, objective, dynamic_weight=True)
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                d({"pred_clip_logits": x, "pred_hs": x, "clip_logits": x, "hs_prompt": x}, 3.0, batch_idx=torch.zeros(3, dtype=torch.int64),
                  src_idx=rows, teacher=torch.randn(3, 8))
            with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
                d.stacked(x, x, rows, rows, w)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        DistillKL.apply(x, x, rows, rows, w, None, None, False)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        DistillL1.apply(x, x, rows, rows, w, True)


def test_fixture_agrees_with_the_restated_formulas():
    """Every case of the reference fixture against the restatement: the loss to 1e-10 relative (float64 on both sides: sums of 1204 terms
    whose logarithms cancel over a range of ~70, 2^-53 * 1204 * 70 ~ 1e-11), the stored gradient to its own float32 rounding (2^-24 of each
    value) plus the same float64 allowance."""
    cases = fixture_cases()
    assert sorted(c["name"] for c in cases) == sorted(
        [f"kl_{o}_dyn{d}" for o in ("gt", "pred", "pred_all") for d in (0, 1)] + ["kl_gt_fed", "kl_pred_fed"] + [f"l1_{o}" for o in ("gt", "pred", "pred_all")])
    for c in cases:
        r = (restate_kl if c["kind"] == "kl" else restate_l1)(**c["kw"])
        assert abs(float(r["loss"]) - c["loss"]) <= 1e-10 * abs(c["loss"]), (c["name"], float(r["loss"]), c["loss"])
        got, want = r["grad_rows"], c["grad"].double()
        assert got.shape == want.shape, c["name"]
        assert bool(((got - want).abs() <= EPS32 * got.abs() + 1e-10 * got.abs().max()).all()), (c["name"], float((got - want).abs().max()))
        if c["mask"] is not None:
            assert bool((c["grad"][:, c["mask"] == 0] == 0).all()) and bool((got[:, c["mask"] == 0] == 0).all()), c["name"]
        # the generator's conditions hold for what is stored
        if c["kind"] == "kl":
            assert float(r["R"].max()) <= 80.0, c["name"]
        else:
            x, y = c["kw"]["pred"].double()[c["kw"]["pred_row"]], c["kw"]["tgt"].double()[c["kw"]["tgt_row"]]
            v = y / y.norm(dim=-1, keepdim=True) if c["kw"]["normalize_target"] else y
            assert float((r["u"] - v).abs().min()) >= 1e-5, c["name"]


def test_restatement_is_torch_kl_div_and_l1_loss_in_float64():
    """the restatement against the op sequence the reference uses (log_softmax / softmax / F.kl_div with the entropy weight, F.l1_loss of
    normalised rows) with autograd, float64, on a case with a class subset, the dynamic weight, repeated rows and per-row weights"""
    g = torch.Generator().manual_seed(7)
    C, K = 37, 9
    pred, tgt = torch.randn(5, C, generator=g, dtype=torch.float64) * 3, torch.randn(6, C, generator=g, dtype=torch.float64) * 3
    pr, tr = torch.randint(0, 5, (K,), generator=g), torch.randint(0, 6, (K,), generator=g)
    w = torch.rand(K, generator=g, dtype=torch.float64)
    ids = torch.randperm(C, generator=g)[:11]
    sub = torch.zeros(C, dtype=torch.bool)
    sub[ids] = True
    x = pred.clone().requires_grad_(True)
    pl, tl = x[pr], tgt[tr]
    prob = tl.softmax(-1)
    dw = (-prob * prob.log()).sum(-1, keepdim=True) / math.log(C) * 2
    loss = (F.kl_div(pl[..., ids].log_softmax(-1), tl[..., ids].softmax(-1), reduction="none") * dw * w[:, None]).sum()
    loss.backward()
    r = restate_kl(pred, tgt, pr, tr, w, subset=sub[None].expand(K, C), dynamic=True)
    assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    scattered = torch.zeros_like(pred).index_add_(0, pr, r["grad_rows"])
    assert float((scattered - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
    for norm in (False, True):
        x = pred.clone().requires_grad_(True)
        u = x / x.norm(dim=-1, keepdim=True)
        v = tgt / tgt.norm(dim=-1, keepdim=True) if norm else tgt
        loss = (F.l1_loss(u[pr], v[tr], reduction="none") * w[:, None]).sum()
        loss.backward()
        r = restate_l1(pred, tgt, pr, tr, w, norm)
        assert abs(float(r["loss"]) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
        scattered = torch.zeros_like(pred).index_add_(0, pr, r["grad_rows"])
        assert float((scattered - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())
