"""GPU: the on-device PostProcess (richsem_amd/postprocess.py; kernels csrc/msda_postproc.h) against the committed fixture of the
reference's class, against ``torch.topk`` / a stable host sort at the LVIS size and on every kind of tie, its NMS against the plain-torch
restatement (tests/postprocess_ref.py), and both inside one captured graph."""
import numpy as np
import pytest
import torch

from richsem_amd.capture import capture
from richsem_amd.postprocess import PostProcess, nms_padded, select

import postprocess_ref as R
from test_postprocess_abi import fixture_cases

pytestmark = pytest.mark.gpu

DEV = "cuda"
Q_FULL, C_FULL = 900, 1203      # the LVIS configuration: 1 082 700 scores per image


def _boxes(B, Q, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.rand(B, Q, 2, generator=g) * 0.6 + 0.2, torch.rand(B, Q, 2, generator=g) * 0.3 + 0.02), -1)


def _sizes(B):
    return torch.tensor([[480.0 + 37 * b, 640.0 - 21 * b] for b in range(B)])


def _check_indices(logits, k, want_flat, boxes=None, sizes=None, box_mode=1):
    """select() on (B, Q, C) logits: flat indices equal to want_flat (B, k), labels / query indices consistent, scores the sigmoid of the
    selected logits within 1e-6, boxes bit-equal to the torch composition"""
    B, Q, C = logits.shape
    boxes = _boxes(B, Q) if boxes is None else boxes
    sizes = _sizes(B) if sizes is None else sizes
    lg, bx, sz = logits.to(DEV), boxes.to(DEV), sizes.to(DEV)
    scores, labels, out_boxes, qidx = select(lg, bx, sz, k, box_mode)
    want = torch.as_tensor(want_flat, dtype=torch.int64, device=DEV)
    got = qidx * C + labels
    assert got.shape == (B, k) and labels.dtype == torch.int64 and qidx.dtype == torch.int64
    assert torch.equal(got, want), f"{int((got != want).sum())} of {want.numel()} indices differ"
    assert int(labels.min()) >= 0 and int(labels.max()) < C and int(qidx.min()) >= 0 and int(qidx.max()) < Q
    ref_scores = torch.sigmoid(lg.flatten(1).float().gather(1, want))
    err = float((scores - ref_scores).abs().nan_to_num(0.0).max())
    print(f"select B={B} Q={Q} C={C} k={k} {logits.dtype}: max |score - sigmoid| = {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(out_boxes, R.decode_boxes(bx, qidx, sz, box_mode))
    return scores, labels, out_boxes, qidx


# ---- the fixture of the reference's class ----------------------------------------------------------------------------------------------
def test_fixture_parity():
    cases, z = fixture_cases()
    assert len(cases) == 7
    for name, ctor, fwd, with_masks in cases:
        outputs = {"pred_logits": torch.from_numpy(z["logits"]).to(DEV), "pred_boxes": torch.from_numpy(z["boxes"]).to(DEV)}
        if with_masks:
            outputs["pred_masks"] = torch.from_numpy(z["masks"]).to(DEV)
        pp = PostProcess(**ctor)
        results = pp(outputs, torch.from_numpy(z["sizes"]).to(DEV), **fwd)
        assert len(results) == 2
        for b, r in enumerate(results):
            assert np.array_equal(r["labels"].cpu().numpy(), z[f"{name}.labels.{b}"]), (name, b)
            assert np.array_equal(r["boxes"].cpu().numpy(), z[f"{name}.boxes.{b}"]), (name, b)            # bit-equal
            err = float(np.abs(r["scores"].cpu().numpy() - z[f"{name}.scores.{b}"]).max())
            print(f"fixture {name}[{b}]: {len(r['scores'])} detections, max |score - reference| = {err:.3e}")
            assert err <= 1e-6, (name, b)
        if ctor["use_opt"]:
            for b, i in enumerate(outputs["item_indices"]):
                assert i.dtype == torch.int64 and np.array_equal(i.cpu().numpy(), z[f"{name}.item_indices.{b}"]), (name, b)
        else:
            assert "item_indices" not in outputs
        if with_masks:
            assert np.array_equal(outputs["pred_masks"].cpu().numpy(), z[f"{name}.pred_masks"])
        # the device-only forms on the same inputs: query indices, and the NMS positions for the cases that have them
        mode = 0 if fwd["not_to_xyxy"] else (2 if fwd["test"] else 1)
        s, l, bx, q = pp.select(torch.from_numpy(z["logits"]).to(DEV), torch.from_numpy(z["boxes"]).to(DEV),
                                torch.from_numpy(z["sizes"]).to(DEV), mode)
        assert np.array_equal(q.cpu().numpy(), z["query_idx"]), name
        if ctor["use_opt"] or ctor["nms_iou_threshold"] > 0:
            keep, kept_idx, n_kept = pp.nms_padded(bx, l if ctor["use_opt"] else None, 0.7 if ctor["use_opt"] else ctor["nms_iou_threshold"])
            for b in range(2):
                want = z[f"{name}.item_indices.{b}"]
                assert int(n_kept[b]) == len(want) and np.array_equal(kept_idx[b, :len(want)].cpu().numpy(), want), (name, b)
                assert bool((kept_idx[b, len(want):] == -1).all()) and int(keep[b].sum()) == len(want)


def test_target_sizes_of_an_integer_type():
    _, z = fixture_cases()
    outputs = {"pred_logits": torch.from_numpy(z["logits"]).to(DEV), "pred_boxes": torch.from_numpy(z["boxes"]).to(DEV)}
    for dtype in (torch.int64, torch.int32, torch.float64):
        results = PostProcess(num_select=100)(outputs, torch.from_numpy(z["sizes"]).to(DEV).to(dtype))
        for b, r in enumerate(results):
            assert np.array_equal(r["boxes"].cpu().numpy(), z[f"plain.boxes.{b}"])


# ---- the LVIS size --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [300, 1000])
def test_full_size_f32(k):
    B, n = 2, Q_FULL * C_FULL
    logits = R.shuffled_linspace(-12, 2, B, n, seed=11).view(B, Q_FULL, C_FULL)
    flat = logits.to(DEV).flatten(1)
    want = torch.topk(flat, k, dim=1)[1]
    # the input is decidable, a property of the input taken on the host: the top k + 1 float32 probabilities lie 21 ulp or more apart
    # (no sigmoid that is good to a few ulp can reorder them) and are ordered as the logits
    pv, pi = torch.topk(logits.flatten(1).sigmoid(), k + 1, dim=1)
    ulp = torch.nextafter(pv[:, :-1], torch.full_like(pv[:, :-1], 2.0)) - pv[:, :-1]
    margin = float(((pv[:, :-1] - pv[:, 1:]) / ulp).min())
    print(f"full size k={k}: smallest gap of the top k + 1 probabilities = {margin:.1f} ulp")
    # (the figure is 21.0 with no slack: it belongs to this fixed input and to the float32 sigmoid of the CPU build of torch that runs
    # the test; a build whose CPU sigmoid rounds otherwise would move it by an ulp or two and fail here, not in the kernels)
    assert margin >= 21.0
    assert torch.equal(pi[:, :k].to(DEV), want)
    assert torch.equal(torch.topk(flat.sigmoid(), k, dim=1)[1], want)      # ... and so does the device's own sigmoid order them
    for mode in (0, 1, 2):
        _check_indices(logits, k, want, box_mode=mode)


def test_full_size_bf16_ties():
    """bf16 logits have at most 65536 distinct values: ties everywhere, the k-th largest value shared by many"""
    B, k = 2, 300
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(B, Q_FULL, C_FULL, generator=g) * 3 - 4).to(torch.bfloat16)
    x = logits.float().flatten(1).numpy()
    want = R.stable_topk(x, k)
    assert all(len(np.unique(x[b][want[b]])) < k for b in range(B))      # ties inside the top k
    _check_indices(logits, k, want)


def _tie_cases():
    g = torch.Generator().manual_seed(17)
    Q, C = 64, 333
    n = Q * C
    yield "all equal", torch.full((2, Q, C), 0.25), 300
    x = torch.full((2, n), -1.5)                               # exactly k - 1 above a value shared by thousands
    for b in range(2):
        x[b, torch.randperm(n, generator=g)[:299]] = torch.rand(299, generator=g) + 1
    yield "k - 1 above a plateau", x.view(2, Q, C), 300
    x = torch.full((2, n), -2.0)                               # fewer than k above the plateau, which is +-0.0 mixed
    zero = torch.where(torch.rand(2, n, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    plateau = torch.rand(2, n, generator=g) < 0.3
    x[plateau] = zero[plateau]
    for b in range(2):
        x[b, torch.randperm(n, generator=g)[:50]] = torch.rand(50, generator=g) + 0.5
    yield "+-0.0 mixed", x.view(2, Q, C), 300
    x = torch.randn(2, n, generator=g)
    for b in range(2):
        p = torch.randperm(n, generator=g)
        x[b, p[:40]] = float("inf")
        x[b, p[40:90]] = float("-inf")
    yield "+inf and -inf", x.view(2, Q, C), 300
    yield "-inf inside the top k", torch.where(torch.rand(1, 8, 40, generator=g) < 0.9, torch.tensor(float("-inf")), torch.randn(1, 8, 40, generator=g)), 200
    yield "k = 1", torch.randn(2, Q, C, generator=g), 1
    yield "k = 1, all equal", torch.zeros(2, Q, C), 1
    yield "k = Q * C", torch.randn(2, 25, 40, generator=g).round(decimals=1), 1000
    yield "C = 1", torch.randn(2, 5000, 1, generator=g), 300
    yield "odd Q * C", torch.randn(3, 77, 131, generator=g).round(decimals=2), 300      # (rows 1 and 2 start off the 16-byte grid)
    yield "B = 7", torch.randn(7, 33, 1203, generator=g).round(decimals=2), 123
    yield "one chunk and a bit", torch.randn(2, 1, 8195, generator=g).round(decimals=1), 1024


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ties_and_tie_order(dtype):
    for name, logits, k in _tie_cases():
        logits = logits.to(dtype)
        want = R.stable_topk(logits.float().flatten(1).numpy(), k)
        print(name, end=": ")
        _check_indices(logits, k, want)


def test_nan_sorts_above_inf():
    g = torch.Generator().manual_seed(23)
    x = torch.randn(2, 50, 200, generator=g)
    x[0, 3, 7] = float("nan")
    x[0, 20, 0] = float("inf")
    x[1, 49, 199] = -float("nan")
    lg = x.to(DEV)
    scores, labels, _, qidx = select(lg, _boxes(2, 50).to(DEV), _sizes(2).to(DEV), 10)
    flat = (qidx * 200 + labels).cpu()
    assert flat[0, 0] == 3 * 200 + 7 and flat[0, 1] == 20 * 200 and flat[1, 0] == 49 * 200 + 199
    assert torch.isnan(scores[0, 0]) and float(scores[0, 1]) == 1.0
    assert torch.equal(flat[0, 2:], torch.topk(x[0].flatten().nan_to_num(-9.0, posinf=-9.0), 8)[1])


# ---- NMS ------------------------------------------------------------------------------------------------------------------------------
def _check_nms(boxes, labels, thr):
    """nms_padded on (B, K, 4) boxes in descending score order against the restatement"""
    B, K = boxes.shape[:2]
    keep, kept_idx, n_kept = nms_padded(boxes.to(DEV), None if labels is None else labels.to(DEV), thr)
    assert keep.dtype == torch.bool and kept_idx.dtype == torch.int64 and n_kept.dtype == torch.int32
    scores = torch.arange(K, 0, -1, dtype=torch.float32)
    counts = []
    for b in range(B):
        want = R.nms(boxes[b], scores, thr) if labels is None else R.batched_nms(boxes[b], scores, labels[b], thr)
        n = int(n_kept[b])
        assert n == len(want), (b, n, len(want))
        assert torch.equal(kept_idx[b, :n].cpu(), want) and bool((kept_idx[b, n:] == -1).all())
        mask = torch.zeros(K, dtype=torch.bool)
        mask[want] = True
        assert torch.equal(keep[b].cpu(), mask)
        counts.append(n)
    return counts


@pytest.mark.parametrize("K", [300, 1024])
def test_nms_clustered(K):
    boxes = torch.stack([R.decidable_clustered_boxes(K, 40 + K + b, (0.5, 0.7)) for b in range(2)])
    g = torch.Generator().manual_seed(K)
    labels = torch.randint(0, 4, (2, K), generator=g)
    for thr in (0.5, 0.7):
        for b in range(2):      # decidable: no pair's IoU within 1e-5 of the threshold
            margin = R.iou_margin(boxes[b], (thr,))
            print(f"nms K={K} thr={thr} image {b}: smallest |IoU - thr| = {margin:.3e}")
            assert margin > 1e-5
        for lab in (None, labels):
            counts = _check_nms(boxes, lab, thr)
            print(f"nms K={K} thr={thr} {'per label' if lab is not None else 'class-agnostic'}: kept {counts}")
            assert all(0 < c < K for c in counts)      # the reference suppresses something and keeps something


def test_nms_corner_cases():
    assert _check_nms(torch.tensor([[[10.0, 10.0, 20.0, 30.0]]]), None, 0.5) == [1]                          # K = 1
    same = torch.tensor([10.0, 20.0, 110.0, 220.0]).repeat(2, 130, 1)
    assert _check_nms(same, None, 0.5) == [1, 1]                                                             # all identical: one kept
    labels = (torch.arange(130) % 3).repeat(2, 1)
    assert _check_nms(same, labels, 0.7) == [3, 3]                                                           # ... one per label
    degenerate = torch.tensor([[5.0, 5.0, 5.0, 5.0], [5.0, 5.0, 5.0, 9.0], [5.0, 5.0, 5.0, 5.0], [0.0, 0.0, 10.0, 10.0],
                               [1.0, 1.0, 9.0, 9.0]]).unsqueeze(0)
    assert _check_nms(degenerate, None, 0.5) == [4]                                                          # 0 / 0 is NaN: nothing suppressed by it
    disjoint = torch.stack([torch.tensor([20.0 * i, 0.0, 20.0 * i + 10, 10.0]) for i in range(70)]).unsqueeze(0)
    assert _check_nms(disjoint, None, 0.5) == [70]
    chain = R.decidable_clustered_boxes(130, 9, (0.8,), clusters=1).unsqueeze(0)                             # suppression across word boundaries
    assert R.iou_margin(chain[0], (0.8,)) > 1e-5
    assert 1 < _check_nms(chain, None, 0.8)[0] < 130


# ---- capture and the workspace cache -----------------------------------------------------------------------------------------------------
def test_graph_replays_equal_eager():
    B, Q, C, k = 2, 300, 1203, 300
    g = torch.Generator().manual_seed(31)
    boxes = torch.stack([R.clustered_boxes(Q, seed=60 + b, size=1.0) for b in range(B)])
    boxes = torch.cat(((boxes[..., :2] + boxes[..., 2:]) / 2, boxes[..., 2:] - boxes[..., :2]), -1).to(DEV)      # as cxcywh
    sizes = _sizes(B).to(DEV)
    inputs = [(torch.randn(B, Q, C, generator=g) * 2).round(decimals=2) for _ in range(3)] + [torch.zeros(B, Q, C)]      # ties in all of them
    static = inputs[0].to(DEV).clone()

    def run(lg):
        s, l, bx, q = select(lg, boxes, sizes, k)
        return (s, l, bx, q) + nms_padded(bx, l, 0.7)

    run(static)                                  # (the workspace exists before the capture)
    torch.cuda.synchronize()
    graph, captured = capture(lambda: run(static))      # (torch's own capture stream)
    for x in inputs:
        static.copy_(x.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        want = run(x.to(DEV))
        idx = R.stable_topk(x.flatten(1).numpy(), k)
        assert np.array_equal((got[3] * C + got[1]).cpu().numpy(), idx)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert all(0 < int(n) <= k for n in got[6])


def test_capture_without_rehearsal_owns_its_workspace():
    """a shape first seen under capture: the graph's call takes its workspace from the graph's pool and leaves the cache alone, so nothing
    cached dies with the graph; eager calls of that shape afterwards allocate and cache their own"""
    from richsem_amd import postprocess
    B, Q, C, k = 2, 41, 203, 77      # (no other test uses this shape)
    g = torch.Generator().manual_seed(37)
    x = torch.randn(B, Q, C, generator=g).round(decimals=1)
    want = R.stable_topk(x.flatten(1).numpy(), k)
    lg, boxes, sizes = x.to(DEV), _boxes(B, Q).to(DEV), _sizes(B).to(DEV)
    key = (lg.device, B, Q, C, k)
    select(lg[:1], boxes[:1], sizes[:1], k)      # (the kernels have run once, on another shape)
    assert key not in postprocess._workspaces
    torch.cuda.synchronize()
    graph, captured = capture(lambda: select(lg, boxes, sizes, k))
    assert key not in postprocess._workspaces
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal((captured[3] * C + captured[1]).cpu().numpy(), want)
    del graph, captured
    _check_indices(x, k, want)
    assert key in postprocess._workspaces
    postprocess.release_workspaces()
    assert not postprocess._workspaces
    _check_indices(x, k, want)


def test_two_shapes_in_one_process():
    g = torch.Generator().manual_seed(41)
    for _ in range(2):
        for B, Q, C, k in ((2, 30, 57, 100), (3, 100, 91, 300), (2, 30, 57, 50), (1, Q_FULL, C_FULL, 300)):
            logits = torch.randn(B, Q, C, generator=g).round(decimals=2)
            _check_indices(logits, k, R.stable_topk(logits.flatten(1).numpy(), k))
