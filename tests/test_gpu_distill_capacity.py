"""GPU (-m gpu): the distillation term over capacity buffers (richsem_amd/distill.py ``device_distill``; ``msda_distill_pairs``,
``msda_distill_scatter_f32`` / ``_bf16``, csrc/msda_distill_pairs.h) and the teacher's box targets over capacity buffers
(richsem_amd/modules/attnpool.py ``clip_box_targets_capacity``):

  * the pair kernel against its numpy restatement (tests/distill_capacity_ref.py), exactly, for every config of the fixture, both layer
    sets and objectives, ``pad_cap`` equal to and 9 above ``pad_size``; its status words;
  * loss and gradient against tests/golden/criterion_distill_capacity_reference.npz -- through the float64 restatement that
    tests/test_distill_capacity_host.py ties to the fixture --, with the bounds tests/test_gpu_distill.py holds the same row kernels to;
  * against the exact-size ``DistillLoss.stacked`` on the same pairs: the gradient bit for bit (float32 and bfloat16), the loss within
    2^-23 |loss| (the same float32 row losses, added in float64 in another order, rounded once on each side);
  * dead slots are never read; two runs give the same bits;
  * ``clip_box_targets_capacity`` against ``clip_box_targets`` in float64: at most 4 x the error of the existing float32 path, measured in
    the same test (the GEMM shapes differ between a capacity and an exact call: bits cannot be asked for);
  * ONE captured graph of teacher targets -> cost blocks -> assignment -> denoising meta -> distillation + backward, replayed on batches
    of other totals and per-image counts (in a process of its own).
"""
import math
import os

import numpy as np
import pytest
import torch

from distill_capacity_ref import CASES, LAYER_SETS, config, pairs_numpy
from richsem_amd.distill import DistillLoss, device_distill, device_distill_and_grads, distill_pairs
from richsem_amd.matcher import CostPlan, HungarianMatcher, TargetBuffers
from richsem_amd.modules.attnpool import AttentionPool2d, clip_box_targets, clip_box_targets_capacity
from test_distill_capacity_host import restated
from test_distill_host import EPS32

pytestmark = pytest.mark.gpu

DEV = "cuda"
CAPACITY = 16
UNITS = 16.0      # tests/test_gpu_distill.py


def _targets_of(counts, gen=None):
    gen = gen or torch.Generator().manual_seed(3)
    out = []
    for tb in counts:
        boxes = torch.cat((torch.rand(tb, 2, generator=gen) * 0.4 + 0.3, torch.rand(tb, 2, generator=gen) * 0.3 + 0.1), 1)
        out.append({"labels": torch.randint(0, 20, (tb,), generator=gen), "boxes": boxes})
    return out


def _device_case(ci, case, layers, slack, capacity=CAPACITY, bf16=False):
    """config ``ci`` of the fixture in the capacity layout on the device + its float64 restatement (on the float32 weights the device uses;
    with ``bf16`` on the bf16-rounded student)"""
    c = config(ci)
    pad_cap = c["pad"] + slack
    r = restated(c, case, layers, pad_cap, capacity, weights64=False)
    pred = torch.from_numpy(r["pred"]).float()
    if bf16:
        pred = pred.bfloat16()
    qot = torch.full((c["nl"] + 1, capacity), -1, dtype=torch.int64)
    qot[:, :c["total"]] = torch.from_numpy(c["qot"])
    return {"c": c, "r": r, "pad_cap": pad_cap, "layers": layers, "case": case,
            "pred": pred.to(DEV).requires_grad_(True), "teacher": torch.from_numpy(r["teacher"]).float().to(DEV),
            "bufs": TargetBuffers(c["N"], capacity, DEV).update_(_targets_of(c["counts"])), "qot": qot.to(DEV),
            "meta": torch.tensor([max(c["counts"]), c["groups"], c["pad"], c["total"], 0], dtype=torch.int64, device=DEV),
            "mask": None if r["mask"] is None else torch.from_numpy(r["mask"]).float().to(DEV)}


def _kw(d):
    kind, objective = d["case"].split("_")[0], d["case"].split("_")[1]
    return dict(pad_cap=d["pad_cap"], layers=d["layers"], distill_type="clip_logits" if kind == "kl" else "clip_l1", objective=objective,
                dynamic_weight=d["case"].endswith("dyn1"), class_mask=d["mask"])


def _run(d, **over):
    d["pred"].grad = None
    loss, status = device_distill(d["pred"], d["teacher"], d["bufs"], d["qot"], over.pop("meta", d["meta"]), **dict(_kw(d), **over))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), status, d["pred"].grad.clone()


# ---- the pair kernel ------------------------------------------------------------------------------------------------------------------------
def _pairs_on_device(bufs, qot, meta, nl, N, Q, pad_cap, layers, objective, num_boxes=None):
    cfg = (nl, N, Q, pad_cap, bufs.total, 1, sum(1 << l for l in layers), len(layers), True, ("gt", "pred").index(objective))
    return [t.cpu().numpy() for t in distill_pairs(bufs, qot, meta, num_boxes, cfg)]


def _assert_pairs_equal(got, want, what):
    for name, g, w in zip(("pred_row", "tgt_row", "row_weight", "row_group", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g, w.view(np.int32) if w.dtype == np.float32 else w), (what, name)


@pytest.mark.parametrize("ci", range(6))
@pytest.mark.parametrize("slack", [0, 9])
def test_pairs_kernel_is_exactly_its_restatement(ci, slack):
    c = config(ci)
    nl, N, Q, pad_cap = c["nl"], c["N"], c["Q"], c["pad"] + slack
    bufs = TargetBuffers(N, CAPACITY, DEV).update_(_targets_of(c["counts"]))
    qot = np.full((nl + 1, CAPACITY), -1, dtype=np.int64)
    qot[:, :c["total"]] = c["qot"]
    qot[:, c["total"]:] = 3      # (columns past the live targets: a valid-looking query that must not be read)
    meta = [max(c["counts"]), c["groups"], c["pad"], c["total"], 0]
    cum = np.concatenate(([0], np.cumsum(c["counts"])))
    for layers in LAYER_SETS + ((0,),):
        for objective in ("gt", "pred"):
            for use_meta in (True, False):
                got = _pairs_on_device(bufs, torch.from_numpy(qot).to(DEV), torch.tensor(meta, device=DEV) if use_meta else None, nl, N, Q, pad_cap,
                                       layers, objective)
                want = pairs_numpy(cum, qot, meta if use_meta else None, None, nl, N, Q, pad_cap, CAPACITY, layers, objective)
                _assert_pairs_equal(got, want, (ci, slack, layers, objective, use_meta))
                assert got[4].tolist() == [0, 0, 0, 0]
                assert int((got[0] >= 0).sum()) == len(layers) * (c["total"] + (c["groups"] * c["total"] if use_meta else 0))


def test_pairs_kernel_status_words_and_the_caller_s_num_boxes():
    c = config(1)      # counts (0, 5, 2), 20 groups, pad_size 200
    nl, N, Q, pad = c["nl"], c["N"], c["Q"], c["pad"]
    bufs = TargetBuffers(N, CAPACITY, DEV).update_(_targets_of(c["counts"]))
    qot = np.full((nl + 1, CAPACITY), -1, dtype=np.int64)
    qot[:, :7] = c["qot"]
    cum = np.array([0, 0, 5, 7])
    meta = [5, 20, 200, 7, 0]
    dev = lambda a: torch.as_tensor(np.asarray(a), device=DEV)
    # the denoising layout does not fit: the overflow flag, a pad_size above pad_cap, a pad_size that is no multiple of the groups
    for m, pad_cap in (([5, 20, 200, 7, 1], 200), (meta, 150), ([5, 20, 190, 7, 0], 200)):
        got = _pairs_on_device(bufs, dev(qot), dev(m), nl, N, Q, pad_cap, (0, 1), "gt")
        _assert_pairs_equal(got, pairs_numpy(cum, qot, m, None, nl, N, Q, pad_cap, CAPACITY, (0, 1), "gt"), m)
        assert got[4].tolist() == [1, 0, 0, 0] and int((got[0] >= 0).sum()) == 2 * 7 and not (got[0][2 * CAPACITY:] >= 0).any()
    # targets without a query: counted over the selected layers; in the last decoder output they also leave num_boxes (7 -> 5)
    q2 = qot.copy()
    q2[0, 3], q2[1, 1], q2[1, 6], q2[2, 0] = -1, Q, -5, -1      # (row 2 is the two-stage output: not looked at)
    for layers, n in (((0, 1), 3), ((1,), 2), ((0,), 1)):
        got = _pairs_on_device(bufs, dev(q2), dev(meta), nl, N, Q, pad, layers, "gt")
        _assert_pairs_equal(got, pairs_numpy(cum, q2, meta, None, nl, N, Q, pad, CAPACITY, layers, "gt"), layers)
        assert got[4].tolist() == [0, n, 0, 0]
        assert got[2].max() == np.float32(1.0 / 5.0)
    # the caller's num_boxes instead of the count
    nb = torch.tensor([3.5], device=DEV)
    got = _pairs_on_device(bufs, dev(q2), dev(meta), nl, N, Q, pad, (0, 1), "pred", num_boxes=nb)
    _assert_pairs_equal(got, pairs_numpy(cum, q2, meta, 3.5, nl, N, Q, pad, CAPACITY, (0, 1), "pred"), "num_boxes")
    assert sorted(set(got[2].tolist())) == [0.0, float(np.float32(1.0 / 70.0)), float(np.float32(1.0 / 3.5))]
    # a prefix that does not describe targets inside the capacity: every slot is dead, nothing is read through it
    for bad in ([1, 1, 5, 7], [0, 6, 5, 7], [0, 0, 5, 17]):
        with torch.no_grad():
            bufs.offsets_dev.copy_(dev(bad))
        got = _pairs_on_device(bufs, dev(qot), dev(meta), nl, N, Q, pad, (0, 1), "gt")
        _assert_pairs_equal(got, pairs_numpy(bad, qot, meta, None, nl, N, Q, pad, CAPACITY, (0, 1), "gt"), bad)
        assert got[4].tolist() == [0, 0, 0, 1] and not (got[0] >= 0).any() and not got[2].any()


# ---- loss and gradient ----------------------------------------------------------------------------------------------------------------------
def _check_against_restatement(d, loss, grad, what):
    """the bounds of tests/test_gpu_distill.py (check_kl / check_l1) on the live slots; exact zeros in every other row"""
    r, rr = d["r"], d["r"]["r"]
    pr, tr, w, grp, _ = r["pairs"]
    live = r["live"]
    want = r["loss"]
    loss = float(loss)
    print(f"{what}: loss {loss:.9g} float64 {want:.9g}")
    if want == 0.0:
        assert loss == 0.0, (what, loss)
    else:
        assert abs(loss - want) <= 1e-5 * abs(want), (what, loss, want)
    g = grad.detach().float().cpu().reshape(-1, grad.shape[-1])
    dead = torch.ones(g.shape[0], dtype=torch.bool)
    dead[torch.from_numpy(pr[live])] = False
    assert not g[dead].view(torch.int32).any(), what      # bit-zero where no pair points
    if not live.any():
        return
    wl = torch.from_numpy(w[live].astype(np.float64))
    if d["case"].startswith("kl"):
        C = g.shape[1]
        bound = UNITS * EPS32 * ((1 + rr["R"]) * wl * (rr["dw"] + 2.0 / math.log(max(C, 2))))[:, None] * (rr["p"] + rr["t"])
    else:
        bound = (UNITS * EPS32 * (wl * (1 + rr["u"].abs().sum(-1)) / rr["norm"]))[:, None]
    err = (g[torch.from_numpy(pr[live])].double() - rr["grad_rows"]).abs()
    worst = float((err / bound.clamp(min=1e-300)).max()) * UNITS
    print(f"{what}: gradient within {worst:.2f} of {UNITS:.0f} units")
    assert bool((err <= bound.expand_as(err)).all()), (what, worst)


@pytest.mark.parametrize("ci", range(6))
@pytest.mark.parametrize("slack", [0, 9])
def test_against_the_reference_loss_labels(ci, slack):
    for case in CASES:
        for layers in LAYER_SETS:
            d = _device_case(ci, case, layers, slack)
            loss, status, grad = _run(d)
            assert status.tolist() == [0, 0, 0, 0]
            _check_against_restatement(d, loss, grad, f"config {ci} slack {slack} {case} layers {layers}")


def _stacked(d, bf16=False):
    """the exact-size composition on the same pairs: ``DistillLoss.stacked`` with index tensors of the batch's live pairs"""
    r = d["r"]
    pr, tr, w, grp, _ = r["pairs"]
    live = r["live"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[live])).to(DEV)
    kind, objective = d["case"].split("_")[0], d["case"].split("_")[1]
    pred = d["pred"].detach().clone().requires_grad_(True)
    crit = DistillLoss("clip_logits" if kind == "kl" else "clip_l1", objective, d["case"].endswith("dyn1"), d["mask"] is not None)
    loss = crit.stacked(pred, d["teacher"], t(pr), t(tr), t(w), t(grp), d["mask"])
    loss.backward()
    return loss.detach(), pred.grad


@pytest.mark.parametrize("case,bf16", [(c, False) for c in CASES] + [("kl_gt_dyn1", True), ("kl_gt_fed", True), ("kl_pred", True)])
def test_against_the_exact_size_composition_bit_for_bit(case, bf16):
    """config 1 (counts (0, 5, 2), 20 denoising groups): 294 live pairs among 2 * (16 + 3 * 209) = 1286 slots"""
    d = _device_case(1, case, (0, 1), 9, bf16=bf16)
    loss, status, grad = _run(d)
    loss2, _, grad2 = _run(d)
    assert grad.dtype == d["pred"].dtype and status.tolist() == [0, 0, 0, 0]
    bits = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(bits(loss), bits(loss2)) and torch.equal(bits(grad), bits(grad2))      # two runs: the same bits
    want, want_grad = _stacked(d, bf16)
    assert torch.equal(bits(grad), bits(want_grad)), case
    assert abs(float(loss) - float(want)) <= 2.0 ** -23 * abs(float(want)), (case, float(loss), float(want))
    # the same launches without the autograd engine: the same bits
    loss3, status3, grad3 = device_distill_and_grads(d["pred"].detach(), d["teacher"], d["bufs"], d["qot"], d["meta"], **_kw(d))
    assert torch.equal(bits(loss3), bits(loss)) and torch.equal(bits(grad3), bits(grad)) and status3.tolist() == [0, 0, 0, 0]
    # d / d loss = 0.5 scales the gradient exactly
    _, _, half = device_distill_and_grads(d["pred"].detach(), d["teacher"], d["bufs"], d["qot"], d["meta"], grad_loss=torch.tensor(0.5, device=DEV), **_kw(d))
    assert torch.equal(half.float() * 2, grad.float()) or bf16


@pytest.mark.parametrize("case", ["kl_gt_dyn1", "kl_pred", "l1_gt"])
def test_dead_slots_are_exactly_dead(case):
    d = _device_case(0, case, (0, 1), 7)
    loss, status, grad = _run(d)
    c, pad, pad_cap = d["c"], d["c"]["pad"], d["pad_cap"]
    total = c["total"]
    with torch.no_grad():
        d["qot"][:, total:] = torch.tensor([1 << 40, -7, 3, 1 << 62, 0, 9, -1, 2, 5], device=DEV)[: CAPACITY - total]
        d["bufs"].tgt_boxes[total:] = float("nan")
        d["bufs"].tgt_ids[total:] = 10 ** 12
        if case.split("_")[1] == "gt":
            d["teacher"][total:] = float("nan")
        else:      # 'pred': the teacher's rows for the queries no pair names
            dead = torch.ones(d["teacher"].shape[:3], dtype=torch.bool, device=DEV).reshape(-1)
            dead[torch.from_numpy(d["r"]["pairs"][0][d["r"]["live"]]).to(DEV)] = False
            d["teacher"].reshape(-1, d["teacher"].shape[-1])[dead] = float("nan")
        d["pred"][:, :, pad:pad_cap] = float("nan")      # the student's rows past pad_size
    loss2, status2, grad2 = _run(d)
    assert status2.tolist() == [0, 0, 0, 0]
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int32), grad2.view(torch.int32))
    assert not grad2[:, :, pad:pad_cap].view(torch.int32).any()


def test_wrong_arguments_raise_before_any_launch():
    d = _device_case(2, "kl_gt_dyn0", (0, 1), 0)
    args = (d["pred"], d["teacher"], d["bufs"], d["qot"], d["meta"])
    kw = _kw(d)
    with pytest.raises(ValueError, match="DistillLoss"):
        device_distill(*args, **dict(kw, objective="pred_all"))
    with pytest.raises(TypeError):
        device_distill(d["pred"].double(), *args[1:], **kw)
    with pytest.raises(ValueError):
        device_distill(*args, **dict(kw, layers=(1,)))      # pred stacks two layers
    with pytest.raises(ValueError):
        device_distill(*args, **dict(kw, layers=(1, 2)))      # layer 2 of 2
    with pytest.raises(ValueError):
        device_distill(d["pred"], d["teacher"][:5], *args[2:], **kw)
    with pytest.raises(ValueError):
        device_distill(d["pred"], d["teacher"], d["bufs"], d["qot"][:, :5].contiguous(), d["meta"], **kw)
    with pytest.raises(ValueError):
        device_distill(*args, **dict(kw, class_mask=torch.ones(3, 301, device=DEV)))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        device_distill(d["pred"].detach().cpu(), *args[1:], **kw)


# ---- the teacher's box targets ----------------------------------------------------------------------------------------------------------------
def _teacher_setup(gen, N=3, C=32, H=7, W=11, classes=37, out_dim=16):
    torch.manual_seed(11)
    pool = AttentionPool2d(7, C, 4, out_dim).to(DEV)
    feats = torch.randn(N, C, H, W, generator=gen).to(DEV)
    text = torch.randn(classes, out_dim, generator=gen).to(DEV)
    return pool, feats, text, torch.tensor(math.log(30.0), device=DEV)


def _image_targets(counts, sizes, gen):
    out = _targets_of(counts, gen)
    for t, hw in zip(out, sizes):
        t["size"] = torch.tensor(hw)
    return [{k: v.to(DEV) for k, v in t.items()} for t in out]


def _check_teacher(prompt, logits, feats, targets, pool, text, scale, what):
    """live rows of the capacity path against clip_box_targets in float64: at most 4 x the error the existing float32 path shows here"""
    total = sum(len(t["labels"]) for t in targets)
    if total == 0:
        return
    p64, l64 = (torch.cat(v) for v in clip_box_targets(feats.double(), targets, pool, text, scale))
    p32, l32 = (torch.cat(v) for v in clip_box_targets(feats, targets, pool, text, scale))
    for name, got, f32, f64 in (("prompt", prompt[:total], p32, p64), ("logits", logits[:total], l32, l64)):
        base, err = float((f32.double() - f64).abs().max()), float((got.double() - f64).abs().max())
        print(f"{what} {name}: capacity path {err:.3e}, exact float32 path {base:.3e} against float64")
        assert err <= 4 * base, (what, name, err, base)


def test_clip_box_targets_capacity_against_the_exact_path_in_float64():
    gen = torch.Generator().manual_seed(21)
    pool, feats, text, scale = _teacher_setup(gen)
    sizes = [(211, 333), (197, 349), (220, 301)]
    targets = _image_targets((0, 5, 2), sizes, gen)
    s = torch.tensor(sizes, dtype=torch.int32, device=DEV)
    for capacity in (7, 16):
        bufs = TargetBuffers(3, capacity, DEV).update_(targets)
        prompt, logits = clip_box_targets_capacity(feats, bufs, s, pool, text, scale)
        assert prompt.shape == (capacity, 16) and logits.shape == (capacity, 37) and bool(torch.isfinite(logits).all())
        _check_teacher(prompt, logits, feats, targets, pool, text, scale, f"capacity {capacity}")


# ---- one graph, many batches ------------------------------------------------------------------------------------------------------------------
def test_one_graph_serves_many_batches():
    """clip_box_targets_capacity -> cost blocks -> msda_lsap -> denoising_queries (for its meta) -> device_distill_and_grads captured ONCE on
    capacity buffers; replays after ``update_`` on batches with totals 7, 16 (full), 0 and 7 with other per-image counts, each against the
    eager exact-size composition of THAT batch: ``_one_graph_job`` below, run in a process of its own, exactly as
    tests/test_gpu_criterion_capacity.py::test_one_graph_serves_many_batches is and for the reason its docstring gives:
    this test leaves the suite's process without a stream, a graph or a graph memory pool of its making."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_distill_capacity as t; t._one_graph_job(); print('one graph: ok')"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "one graph: ok" in r.stdout, (r.returncode, r.stderr[-2000:])


def _one_graph_job():
    """the body of test_one_graph_serves_many_batches (raises where it does not hold).  Per replay: the assignment is the one the batch's
    own exact plan gives; the teacher's live rows are within 4 x the existing float32 path's error of clip_box_targets in float64; and loss
    and gradient are those of the exact-size ``DistillLoss.stacked`` on host-built index tensors of that batch -- run on the graph's own
    teacher rows cut to the batch's size, so the gradient is compared bit for bit and the loss to 2^-23."""
    from richsem_amd.capture import capture, capture_stream
    from richsem_amd.dn import denoising_queries, dn_buffers, dn_capacity, dn_group_count
    nl, N, Q, C_det, C_clip, D, dn_number, max_per = 2, 2, 12, 23, 37, 8, 3, 8
    layers = (0, 1)
    pad_cap = dn_capacity(dn_number, max_per)
    gen = torch.Generator().manual_seed(9)
    batches = [[3, 4], [8, 8], [0, 0], [6, 1]]
    all_sizes = [[(211, 333), (197, 349)], [(224, 352), (180, 300)], [(200, 200), (210, 340)], [(190, 320), (222, 351)]]
    pool, feats0, text, scale = _teacher_setup(gen, N=N)
    feats_all = [torch.randn(N, 32, 7, 11, generator=gen) for _ in batches]
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=gen) * 0.6 + 0.2, torch.rand(*s, 2, generator=gen) * 0.4 + 0.03), -1)
    preds = [{"logits": torch.randn(nl, N, pad_cap + Q, C_det, generator=gen) * 3, "coords": rb(nl, N, pad_cap + Q),
              "il": torch.randn(N, Q, C_det, generator=gen) * 3, "ib": rb(N, Q), "clip": torch.randn(nl, N, pad_cap + Q, C_clip, generator=gen) * 4}
             for _ in batches]
    data = [_image_targets(counts, sizes, gen) for counts, sizes in zip(batches, all_sizes)]
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    table = torch.randn(C_det + 1, D, generator=gen).to(DEV)
    kw = dict(num_queries=Q, num_classes=C_det, dn_number=dn_number, label_noise_ratio=0.5, box_noise_scale=1.0)
    dkw = dict(pad_cap=pad_cap, layers=layers, distill_type="clip_logits", objective="gt", dynamic_weight=True)

    def outputs(L):
        return [{"pred_logits": L["logits"][l][:, pad_cap:], "pred_boxes": L["coords"][l][:, pad_cap:]} for l in range(nl)] + \
            [{"pred_logits": L["il"], "pred_boxes": L["ib"]}]

    with capture_stream() as side:
        bufs = TargetBuffers(N, CAPACITY, DEV, max_per_image=max_per)
        L = {k: v.to(DEV) for k, v in preds[0].items()}
        feats = feats_all[0].to(DEV)
        sizes = torch.tensor(all_sizes[0], dtype=torch.int32, device=DEV)
        uni = torch.rand((N, pad_cap, 10), generator=gen).to(DEV)
        dn_out = dn_buffers(N, pad_cap, Q, D, DEV)

        def step():
            prompt, teacher = clip_box_targets_capacity(feats, bufs, sizes, pool, text, scale)
            qot, st = matcher.match_many_device(outputs(L), bufs)
            meta = denoising_queries(bufs.offsets_dev, bufs.tgt_ids, bufs.tgt_boxes, table, uni, pad_cap=pad_cap, out=dn_out, **kw)[4]
            # (forward and backward launched from this thread: the capture holds no work of the autograd engine's threads)
            loss, status, grad = device_distill_and_grads(L["clip"], teacher, bufs, qot, meta, **dkw)
            return loss, grad, qot, st, meta, status, prompt, teacher

        bufs.update_(data[0])
        step()      # eager once, on the capture stream
        torch.cuda.synchronize()
        graph, (loss, grad, qot, st, meta, status, prompt, teacher) = capture(step, side)
        for i in (1, 2, 3, 0):
            counts, targets = batches[i], data[i]
            bufs.update_(targets)
            with torch.no_grad():
                for k in L:
                    L[k].copy_(preds[i][k])
                feats.copy_(feats_all[i])
                sizes.copy_(torch.tensor(all_sizes[i], dtype=torch.int32))
            graph.replay()
            torch.cuda.synchronize()
            total, groups = sum(counts), dn_group_count(dn_number, counts)
            pad = 2 * max(counts) * groups
            assert meta.tolist() == [max(counts), groups, pad, total, 0] and status.tolist() == [0, 0, 0, 0] and not st.any()
            if total:      # the same assignment from the batch's own exact plan
                q_ex, _ = matcher.match_many_device(outputs(L), CostPlan(targets, DEV, torch.float32))
                assert torch.equal(qot[:, :total], q_ex)
            _check_teacher(prompt, teacher, feats, targets, pool, text, scale, f"replay {counts}")
            # the exact-size composition: index tensors built on the host for this batch, the teacher's rows of this batch
            cum = np.concatenate(([0], np.cumsum(counts)))
            pr, tr, w, grp, _ = pairs_numpy(cum, qot.cpu().numpy(), meta.tolist(), None, nl, N, Q, pad_cap, CAPACITY, layers, "gt")
            live = pr >= 0
            assert int(live.sum()) == len(layers) * total * (1 + groups)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a[live])).to(DEV)
            student = L["clip"].detach().clone().requires_grad_(True)
            want = DistillLoss("clip_logits", "gt", True).stacked(student, teacher[:total].clone(), t(pr), t(tr), t(w))
            want.backward()
            want = want.detach()
            print(f"replay {counts}: loss {float(loss):.9g} composition {float(want):.9g}")
            assert torch.equal(grad.view(torch.int32), student.grad.view(torch.int32)), counts
            assert abs(float(loss) - float(want)) <= 2.0 ** -23 * abs(float(want)), (counts, float(loss), float(want))
            assert (float(loss) > 0) == (total > 0)
