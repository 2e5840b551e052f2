"""The criterion's distillation term on the GPU (richsem_amd/distill.py; csrc/msda_distill.h): the KL and L1 row kernels against the fixture
made from the reference's own ``loss_labels`` (tests/golden/criterion_distill_reference.npz) and against the float64 restatement of
tests/test_distill_host.py (which that file ties to the fixture and to torch's op sequence), edge shapes, the index guard, bit
reproducibility, and the composed step's opt-in switch (bench_step.Step(device_distill=True)) eager and graphed.

Bounds.  The loss: 1e-5 relative, what test_criterion_kernels_against_the_reference_loss_functions allows the other criterion kernels.
KL gradients, per element against float64:  |d| <= 16 * 2^-24 * (1 + R_k) * w_k * (dw_k + 2 / ln C) * (p_c + t_c)  -- the exponent x - max
carries a rounding error of up to R_k 2^-24 (R_k: the larger range of the two rows, of the whole teacher row too when the weight is dynamic),
which is the relative error of p_c and t_c; the 2 / ln C covers the entropy's absolute rounding error where the entropy itself is small; 16
leaves room for the summation order and the device's expf.  L1 gradients:  |d| <= 16 * 2^-24 * w_k * (1 + |u|_1) / |pred row|_2."""
import math
import os
import warnings

import pytest
import torch

from richsem_amd.distill import DistillKL, DistillL1, DistillLoss, kl_rows, l1_rows
from test_distill_host import EPS32, fixture_cases, restate_kl, restate_l1

pytestmark = pytest.mark.gpu

H, W_IMG, BOXES = 256, 320, 5      # the small composed step of tests/test_gpu_step.py
DEV = "cuda"
UNITS = 16.0


def _report(text):
    if os.environ.get("RICHSEM_REPORT"):
        print("[measured] " + text, flush=True)


def _close_loss(got, want, what):
    if want == 0.0:
        assert got == 0.0, (what, got)
    else:
        assert abs(got - want) <= 1e-5 * abs(want), (what, got, want)


def _live_rows(pred, tgt, pr, tr, w, subset):
    live = (w != 0) & (pr >= 0) & (pr < pred.shape[0]) & (tr >= 0) & (tr < tgt.shape[0])
    return live if subset is None else live & subset.any(-1)


def check_kl(pred, tgt, pr, tr, w, grp=None, mask=None, dynamic=False, bf16=False, what=""):
    """one device call against the restatement on the same (float32, or bf16-rounded) inputs: the loss, every gradient element within the
    rounding bound, exact zeros off the subset and in the rows that count nothing.  CPU tensors in; returns (loss, grad_rows) on the CPU."""
    C = pred.shape[1]
    if bf16:
        pred = pred.bfloat16().float()
    subset = None
    if mask is not None:
        ok = (grp >= 0) & (grp < mask.shape[0])
        subset = (mask[grp.clamp(0, mask.shape[0] - 1).long()] != 0) & ok[:, None]
    live = _live_rows(pred, tgt, pr, tr, w, subset)
    loss, grad_rows, _ = kl_rows((pred.bfloat16() if bf16 else pred).to(DEV), tgt.to(DEV), pr.to(DEV), tr.to(DEV), w.to(DEV),
                                 None if grp is None else grp.to(DEV), None if mask is None else mask.to(DEV), dynamic)
    loss, grad_rows = float(loss.cpu()[0]), grad_rows.cpu()
    assert grad_rows.shape == (pr.numel(), C) and grad_rows.dtype == torch.float32
    assert bool((grad_rows[~live] == 0).all()), what
    if subset is not None:
        assert bool((grad_rows[~subset] == 0).all()), what      # bit-zero off the subset
    if not bool(live.any()):
        assert loss == 0.0, (what, loss)
        return loss, grad_rows
    r = restate_kl(pred, tgt, pr[live], tr[live], w[live], None if subset is None else subset[live], dynamic)
    _close_loss(loss, float(r["loss"]), what)
    bound = UNITS * EPS32 * ((1 + r["R"]) * w[live].double() * (r["dw"] + 2.0 / math.log(max(C, 2))))[:, None] * (r["p"] + r["t"])
    err = (grad_rows[live].double() - r["grad_rows"]).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) * UNITS
    _report(f"{what}: loss {loss:.8g} (float64 {float(r['loss']):.8g}), gradient within {worst:.2f} of {UNITS:.0f} units")
    assert bool((err <= bound).all()), (what, worst)
    return loss, grad_rows


def check_l1(pred, tgt, pr, tr, w, normalize_target, what=""):
    live = _live_rows(pred, tgt, pr, tr, w, None)
    loss, grad_rows, _ = l1_rows(pred.to(DEV), tgt.to(DEV), pr.to(DEV), tr.to(DEV), w.to(DEV), normalize_target)
    loss, grad_rows = float(loss.cpu()[0]), grad_rows.cpu()
    assert grad_rows.shape == (pr.numel(), pred.shape[1])
    assert bool((grad_rows[~live] == 0).all()), what
    if not bool(live.any()):
        assert loss == 0.0, (what, loss)
        return loss, grad_rows
    r = restate_l1(pred, tgt, pr[live], tr[live], w[live], normalize_target)
    _close_loss(loss, float(r["loss"]), what)
    bound = UNITS * EPS32 * (w[live].double() * (1 + r["u"].abs().sum(-1)) / r["norm"])[:, None]
    err = (grad_rows[live].double() - r["grad_rows"]).abs()
    worst = float((err / bound).max()) * UNITS
    _report(f"{what}: loss {loss:.8g} (float64 {float(r['loss']):.8g}), gradient within {worst:.2f} of {UNITS:.0f} units")
    assert bool((err <= bound.expand_as(err)).all()), (what, worst)
    return loss, grad_rows


# ---- against the fixture ----------------------------------------------------------------------------------------------------------------------
def _distill_loss_call(c):
    """the case through DistillLoss, as a criterion would call it: -> (loss, gradient of the student's output) on the device"""
    N, Q, C = c["shape"]
    kl = c["kind"] == "kl"
    kw = c["kw"]
    student = kw["pred"].view(N, Q, C).to(DEV).requires_grad_(True)
    teacher_out = kw["tgt"].view(N, Q, C).to(DEV) if c["objective"] != "gt" else None
    outputs = {"pred_clip_logits" if kl else "pred_hs": student, "clip_logits" if kl else "hs_prompt": teacher_out}
    d = DistillLoss("clip_logits" if kl else "clip_l1", c["objective"], dynamic_weight=kw.get("dynamic", False), fed_on_kd=c["mask"] is not None)
    loss = d(outputs, c["num_boxes"], batch_idx=c["batch_idx"].to(DEV), src_idx=c["src_idx"].to(DEV),
             teacher=kw["tgt"].to(DEV) if c["objective"] == "gt" else None, teacher_idx=c["tgt_idx"].to(DEV) if c["objective"] == "gt" else None,
             fed_mask=None if c["mask"] is None else c["mask"].to(DEV))
    loss.backward()
    return loss.detach(), student.grad


def test_kernels_against_the_reference_loss_labels():
    """every case of criterion_distill_reference.npz -- KL: gt / pred / pred_all x dynamic weight off / on, gt and pred with use_fed_on_kd;
    L1: the three objectives -- with the student in f32 and (KL) in bf16 storage: the bf16 expectation is the restatement on the rounded
    logits.  The f32 loss is held against the reference's stored float64 loss directly; DistillLoss, called as a criterion calls it,
    returns that loss and scatters exactly the kernel's gradient rows."""
    for c in fixture_cases():
        kw = c["kw"]
        pr, tr, w = kw["pred_row"], kw["tgt_row"], kw["weight"].float()
        if c["kind"] == "kl":
            mask = None if c["mask"] is None else c["mask"][None]
            grp = None if mask is None else torch.zeros(pr.numel(), dtype=torch.int32)
            loss, grad_rows = check_kl(kw["pred"], kw["tgt"], pr, tr, w, grp, mask, kw["dynamic"], what=c["name"])
            check_kl(kw["pred"], kw["tgt"], pr, tr, w, grp, mask, kw["dynamic"], bf16=True, what=c["name"] + " bf16")
        else:
            loss, grad_rows = check_l1(kw["pred"], kw["tgt"], pr, tr, w, kw["normalize_target"], what=c["name"])
        _close_loss(loss, c["loss"], c["name"] + " against the reference")
        got, student_grad = _distill_loss_call(c)
        _close_loss(float(got), c["loss"], c["name"] + " through DistillLoss")
        g = student_grad.reshape(-1, student_grad.shape[-1]).cpu()
        assert torch.equal(g[pr], grad_rows), c["name"]
        rest = g.clone()
        rest[pr] = 0
        assert not bool(rest.any()), c["name"]
    with pytest.raises(ValueError, match="fed_on_kd"):
        DistillLoss("clip_logits", "pred_all", fed_on_kd=True)({"pred_clip_logits": torch.zeros(1, 2, 4, device=DEV), "clip_logits": torch.zeros(1, 2, 4, device=DEV)}, 1.0)


# ---- edge shapes --------------------------------------------------------------------------------------------------------------------------------
def _rows_case(C, K, seed, pred_rows=7, tgt_rows=6, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    pred, tgt = torch.randn(pred_rows, C, generator=g) * scale, torch.randn(tgt_rows, C, generator=g) * scale
    pr, tr = torch.randint(0, pred_rows, (K,), generator=g), torch.randint(0, tgt_rows, (K,), generator=g)
    w = torch.rand(K, generator=g) + 0.1
    return g, pred, tgt, pr, tr, w


@pytest.mark.parametrize("C", [1, 2, 255, 256, 257, 1204, 2500])
def test_kl_class_counts_around_the_workgroup_width(C):
    """C = 1 (every softmax is 1: loss and gradient exactly 0), below / at / above the 256 threads of a workgroup, the flagship's 1204, and
    2500: past the 2048 elements a workgroup keeps in registers.  All classes, then a random class mask per group, without and with the
    dynamic weight, f32 and bf16 student; a zero weight, a row whose group's mask is empty, a row whose group is out of range."""
    g, pred, tgt, pr, tr, w = _rows_case(C, 6, 100 + C)
    w[1] = 0.0
    mask = (torch.rand(3, C, generator=g) < 0.3).float()
    mask[0, 0] = 1.0
    mask[2] = 0.0                                      # group 2 selects nothing
    grp = torch.tensor([0, 1, 2, 3, 0, -1], dtype=torch.int32)      # 3 and -1: outside [0, 3)
    for dynamic in ([False] if C < 2 else [False, True]):
        for bf16 in (False, True):
            what = f"C={C} dynamic={dynamic} bf16={bf16}"
            loss, grad_rows = check_kl(pred, tgt, pr, tr, w, dynamic=dynamic, bf16=bf16, what=what)
            assert bool((grad_rows[1] == 0).all())
            if C == 1:
                assert loss == 0.0 and not bool(grad_rows.any())
            loss, grad_rows = check_kl(pred, tgt, pr, tr, w, grp, mask, dynamic, bf16, what=what + " masked")
            assert not bool(grad_rows[[1, 2, 3, 5]].any())
    # a mask with one class: p = t = 1 there, loss and gradient exactly 0
    one = torch.zeros(1, C)
    one[0, C // 2] = 1.0
    loss, grad_rows = check_kl(pred, tgt, pr, tr, w, torch.zeros(6, dtype=torch.int32), one, C >= 2, what=f"C={C} one class")
    assert loss == 0.0 and not bool(grad_rows.any())


def test_kl_subsets_on_either_side_of_the_register_cache():
    """C = 2500: a workgroup keeps classes 0 .. 2047 in registers and reads 2048 .. 2499 again from memory, the mask with them.  Groups whose
    classes lie ONLY past the cache (a few, and a single one: loss and gradient exactly 0), only inside it, and on both sides; a group
    that selects nothing.  A subset that lies wholly past the cache is not an empty one."""
    C, cache = 2500, 2048
    g, pred, tgt, pr, tr, w = _rows_case(C, 5, 901)
    mask = torch.zeros(5, C)
    mask[0, torch.tensor([2048, 2049, 2300, 2499])] = 1.0      # only past the cache
    mask[1, 2499] = 1.0                                          # one class, past the cache
    mask[2, torch.tensor([0, 255, 256, 2047])] = 1.0            # only inside it
    mask[3, torch.tensor([5, 2047, 2048, 2400])] = 1.0          # both sides
    grp = torch.arange(5, dtype=torch.int32)                     # (group 4 selects nothing)
    for dynamic in (False, True):
        for bf16 in (False, True):
            what = f"cache sides dynamic={dynamic} bf16={bf16}"
            loss, grad_rows = check_kl(pred, tgt, pr, tr, w, grp, mask, dynamic, bf16, what=what)
            assert loss > 0.0, what
            assert bool(grad_rows[0, cache:].any()) and not bool(grad_rows[0, :cache].any()), what
            assert not bool(grad_rows[1].any()) and not bool(grad_rows[4].any()), what
            assert bool(grad_rows[2, :cache].any()) and not bool(grad_rows[2, cache:].any()), what
            assert bool(grad_rows[3, :cache].any()) and bool(grad_rows[3, cache:].any()), what
    # the tail group alone carries a loss: every row in group 0
    loss, grad_rows = check_kl(pred, tgt, pr, tr, w, torch.zeros(5, dtype=torch.int32), mask, True, what="all rows past the cache")
    assert loss > 0.0 and bool(grad_rows[:, cache:].any(-1).all())


def _l1_case(D, K, seed, norm, **kw):
    """_rows_case without any |u - v| below 1e-5 (reseeded until then): a gradient sign must not hang on rounding"""
    for s in range(seed, seed + 500):
        g, pred, tgt, pr, tr, w = _rows_case(D, K, s, **kw)
        if norm and D == 1:
            tgt = tgt.abs() * -torch.sign(pred[:1])      # (D = 1: u, v = +-1; make the signs differ, or every difference is 0)
            pred = pred.abs() * torch.sign(pred[:1])
        if K == 0:
            return g, pred, tgt, pr, tr, w
        r = restate_l1(pred, tgt, pr, tr, w, norm)
        v = tgt.double()[tr] / (tgt.double()[tr].norm(dim=-1, keepdim=True) if norm else 1.0)
        if float((r["u"] - v).abs().min()) >= 1e-5:
            return g, pred, tgt, pr, tr, w
    raise AssertionError("no sample with every |u - v| >= 1e-5")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 1024, 2500])
def test_l1_channel_counts_around_the_wavefront_width(D):
    """D = 1 (u = +-1: the gradient is 0 to rounding), around the 64 lanes of a wavefront, the flagship's 1024, and 2500: past the 2048 elements
    a workgroup keeps in registers; target as it is and normalised; a zero weight"""
    for norm in (False, True):
        g, pred, tgt, pr, tr, w = _l1_case(D, 6, 200 + D, norm, scale=2.0)
        w[4] = 0.0
        loss, grad_rows = check_l1(pred, tgt, pr, tr, w, norm, what=f"D={D} normalize_target={norm}")
        assert not bool(grad_rows[4].any())


@pytest.mark.parametrize("K", [0, 1, 257])
def test_row_counts_and_repeated_rows(K):
    """no row at all (loss 0, nothing launched but the clear), one row, more rows than one pass of a small grid; through the autograd
    functions with every pred_row drawn from 7 rows, so that at K = 257 each repeats ~37 times and the gradients add"""
    C = 257
    for kind in ("kl", "l1"):
        g, pred, tgt, pr, tr, w = _rows_case(C, K, 300 + K) if kind == "kl" else _l1_case(C, K, 300 + K, True)
        x = pred.to(DEV).requires_grad_(True)
        if kind == "kl":
            loss = DistillKL.apply(x, tgt.to(DEV), pr.to(DEV), tr.to(DEV), w.to(DEV), None, None, True)
            r = restate_kl(pred, tgt, pr, tr, w, None, True) if K else None
            unit = None if r is None else EPS32 * ((1 + r["R"]) * w.double() * (r["dw"] + 2.0 / math.log(C)))[:, None] * (r["p"] + r["t"])
        else:
            loss = DistillL1.apply(x, tgt.to(DEV), pr.to(DEV), tr.to(DEV), w.to(DEV), True)
            r = restate_l1(pred, tgt, pr, tr, w, True) if K else None
            unit = None if r is None else (EPS32 * (w.double() * (1 + r["u"].abs().sum(-1)) / r["norm"])[:, None]).expand(K, C)
        (loss * 1.0).backward()
        assert loss.dim() == 0 and loss.dtype == torch.float32 and x.grad.shape == x.shape
        if K == 0:
            assert float(loss) == 0.0 and not bool(x.grad.any())
            continue
        _close_loss(float(loss), float(r["loss"]), f"{kind} K={K}")
        want = torch.zeros(pred.shape, dtype=torch.float64).index_add_(0, pr, r["grad_rows"])
        # each row within its own bound; adding n float32 rows costs at most (n - 1) 2^-24 of the sum of their magnitudes on top
        bound = torch.zeros_like(want).index_add_(0, pr, UNITS * unit)
        count = torch.zeros(pred.shape[0], dtype=torch.float64).index_add_(0, pr, torch.ones(K, dtype=torch.float64))
        bound += EPS32 * (count - 1).clamp(min=0)[:, None] * torch.zeros_like(want).index_add_(0, pr, r["grad_rows"].abs())
        assert bool(((x.grad.cpu().double() - want).abs() <= bound).all()), (kind, K)


def test_rows_outside_the_tensors_are_skipped():
    """pred and tgt are views that start at row 4 of larger tensors, and pred_row / tgt_row hold -1 and the row count: an unguarded read would
    still land inside the same allocation, so nothing can fault -- the rows must contribute nothing, which check_* asserts (zero gradient
    rows, and the loss of the remaining rows alone)"""
    g = torch.Generator().manual_seed(5)
    for C, kind in ((1204, "kl"), (1204, "kl_bf16"), (1024, "l1")):
        big_p, big_t = (torch.randn(12, C, generator=g) * 3).to(DEV), (torch.randn(12, C, generator=g) * 3).to(DEV)
        if kind == "kl_bf16":
            big_p = big_p.bfloat16()
        pred, tgt = big_p[4:10], big_t[4:10]
        assert pred.data_ptr() == big_p.data_ptr() + 4 * C * big_p.element_size() and pred.is_contiguous()
        pr = torch.tensor([2, -1, 6, 0, 5, 3])
        tr = torch.tensor([1, 0, 2, -1, 6, 5])
        w = torch.full((6,), 0.25)
        if kind == "l1":
            fn = lambda p, t: l1_rows(p, t, pr.to(DEV), tr.to(DEV), w.to(DEV), True)
            ref = restate_l1(pred.float().cpu(), tgt.cpu(), pr[[0, 5]], tr[[0, 5]], w[[0, 5]], True)
        else:
            fn = lambda p, t: kl_rows(p, t, pr.to(DEV), tr.to(DEV), w.to(DEV), None, None, True)
            ref = restate_kl(pred.float().cpu(), tgt.cpu(), pr[[0, 5]], tr[[0, 5]], w[[0, 5]], None, True)
        loss, grad_rows, _ = fn(pred, tgt)
        assert not bool(grad_rows[1:5].any()), kind
        assert bool(grad_rows[0].any()) and bool(grad_rows[5].any()), kind
        _close_loss(float(loss[0]), float(ref["loss"]), kind)
        # the rows around the views do not matter: other values there, the same bits out
        big_p[:4], big_p[10:], big_t[:4], big_t[10:] = 9.0, -9.0, 7.0, -7.0
        loss2, grad_rows2, _ = fn(pred, tgt)
        assert torch.equal(loss, loss2) and torch.equal(grad_rows, grad_rows2), kind
        # through autograd the skipped rows add nothing anywhere
        if kind == "kl":
            x = pred.clone().requires_grad_(True)
            DistillKL.apply(x, tgt, pr.to(DEV), tr.to(DEV), w.to(DEV), None, None, True).backward()
            assert torch.equal(x.grad[2], grad_rows[0]) and torch.equal(x.grad[3], grad_rows[5]) and not bool(x.grad[[0, 1, 4, 5]].any())


def test_two_calls_give_the_same_bits():
    """no floating-point atomic anywhere: 2100 rows (more than the 2048 workgroups of a call, so the grid strides and the total has 2048
    partials) twice, with a mask and the dynamic weight, f32 and bf16; the L1 form too"""
    C, K = 1204, 2100
    g, pred, tgt, pr, tr, w = _rows_case(C, K, 77, pred_rows=300, tgt_rows=40)
    mask = (torch.rand(5, C, generator=g) < 0.1).float().to(DEV)
    grp = torch.randint(0, 5, (K,), generator=g, dtype=torch.int32).to(DEV)
    pred, tgt, pr, tr, w = (t.to(DEV) for t in (pred, tgt, pr, tr, w))
    for p in (pred, pred.bfloat16()):
        a = kl_rows(p, tgt, pr, tr, w, grp, mask, True)
        b = kl_rows(p, tgt, pr, tr, w, grp, mask, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert bool(torch.isfinite(a[0]).all()) and float(a[0]) > 0
    a, b = l1_rows(pred, tgt, pr, tr, w, True), l1_rows(pred, tgt, pr, tr, w, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the total of 2048 partials against the float64 sum of the restated rows
    r = restate_l1(pred.cpu(), tgt.cpu(), pr.cpu(), tr.cpu(), w.cpu(), True)
    _close_loss(float(a[0]), float(r["loss"]), "l1 K=2100")
    # and nothing synchronises, forward or backward
    x = pred.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        DistillKL.apply(x, tgt, pr, tr, w, grp, mask, True).backward()
        DistillL1.apply(x, tgt, pr, tr, w, False).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


# ---- the composed step ------------------------------------------------------------------------------------------------------------------------
def _small_step(seed=0, **kw):
    import bench_step
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, seed=seed, dev=torch.device(DEV, 0), **kw)
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    return model, images, mask, targets


def test_step_with_device_distill_is_the_default_criterion():
    """Step.loss_part with device_distill against the default (gathers + softmaxes + F.kl_div) on the same outputs and indices: the loss to
    1e-5 relative; the gradient of clip_logits -- only the distillation term reaches it -- against the float64 restatement on the same rows
    with the KL rounding bound, and exactly 0 in every row that is not matched"""
    model, images, mask, targets = _small_step(seed=2)
    with torch.no_grad():
        outs = model.model_part(images, mask)
    idx = model.pack_indices(model.match(*outs[:4], targets), targets)
    res = []
    for on in (False, True):
        model.device_distill = on
        leaves = [o.detach().clone().requires_grad_(i < 5) for i, o in enumerate(outs)]
        loss = model.loss_part(*leaves, *idx)
        loss.backward()
        res.append((float(loss.detach()), leaves[4].grad.cpu()))
    (l_ref, g_ref), (l_dev, g_dev) = res
    _report(f"step criterion: default {l_ref:.8g} device distillation {l_dev:.8g}")
    assert abs(l_dev - l_ref) <= 1e-5 * abs(l_ref), (l_dev, l_ref)
    clip_logits, t_logits = outs[4].float().cpu(), outs[5].float().cpu()
    _, bi, si, tj = (t.cpu() for t in idx[4])
    Qc, C = clip_logits.shape[1:]
    rows = bi * Qc + si + model.static["lay"]["pad_size"]
    K = rows.numel()
    assert K > 0 and rows.unique().numel() == K
    w = torch.full((K,), 0.5 / K)
    r = restate_kl(clip_logits.reshape(-1, C), t_logits.reshape(-1, C), rows, tj, w)
    bound = UNITS * EPS32 * ((1 + r["R"]) * w.double() * (1.0 + 2.0 / math.log(C)))[:, None] * (r["p"] + r["t"])
    g = g_dev.reshape(-1, C)
    err = (g[rows].double() - r["grad_rows"]).abs()
    _report(f"step clip_logits gradient within {float((err / bound).max()) * UNITS:.2f} of {UNITS:.0f} units; "
            f"default composition {float(((g_ref.reshape(-1, C)[rows].double() - r['grad_rows']).abs() / bound).max()) * UNITS:.2f}")
    assert bool((err <= bound).all())
    rest = g.clone()
    rest[rows] = 0
    assert not bool(rest.any())


def test_graphed_step_with_device_distill_captures_and_matches_the_eager_step():
    """bench_step.run_graphed(device_distill=True): the row kernel and its total are captured with the rest of the criterion (a
    synchronising call inside the capture would fail it; no warning), and the first replay's loss is the eager step's on the same
    parameters, noise, two-stage selection and assignment within the 2e-3 that tests/test_gpu_step.py allows between the graphed and the
    eager bf16 step."""
    import bench_step
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = bench_step.run_graphed(2, torch.device(DEV, 0), steps=1, warmup=0, optimizer=False, noise_seed=3, return_grads=True,
                                     height=H, width=W_IMG, boxes_per_image=BOXES, seed=0, device_distill=True)
    noisy = [str(w.message)[:160] for w in caught if "AccumulateGrad" in str(w.message) or "sync" in str(w.message).lower()]
    assert not noisy, noisy
    model, images, mask, targets = _small_step(seed=0, device_distill=True)
    model.freeze_noise(3)
    for p in model.parameters():
        p.grad = None
    loss = model(images, mask, targets, res["indices"], res["topk"])
    gap = abs(res["loss"] - float(loss)) / abs(float(loss))
    _report(f"graphed step with device distillation: loss {res['loss']:.8g} eager {float(loss):.8g} relative gap {gap:.3g}")
    assert gap < 2e-3, (res["loss"], float(loss))
