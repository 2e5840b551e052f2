"""GPU (-m gpu): the denoising queries from the counts on the device (richsem_amd/dn.py ``denoising_queries``, csrc/msda_dn_noise.h) against
what the reference's own ``prepare_for_cdn`` computed (tests/golden/dn_noise_reference.npz) and against the numpy restatement
tests/dn_noise_ref.py (which tests/test_dn_queries_host.py ties to that fixture): labels, noised boxes, embedded rows and mask BIT-EQUAL,
``q_bbox`` within |got - y64| <= 2^-24 + k ulp32(|y64|) of the float64 inverse_sigmoid of the (bit-equal) noised box, k = 2
(dn_noise_ref.LOGF_ULPS: no statement of logf's accuracy was found with the toolkit's documents, so 2).  Every call writes into buffers
pre-filled with NaN / 0xff, so an element the kernel leaves out shows."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import dn_noise_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ["add_gt", "edge", "empty", "no_cdn", "one_group", "ragged", "small_dn"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dn_noise_reference.npz"))


def _poisoned(N, pad_cap, nq, D):
    from richsem_amd.dn import dn_buffers
    out = dn_buffers(N, pad_cap, nq, D, DEV)
    for k, t in out.items():
        t.fill_(float("nan")) if t.is_floating_point() else t.view(torch.uint8).fill_(0xff)
    return out


def _device_inputs(counts, labels, boxes, cap=None):
    counts = [int(c) for c in counts]
    cap = sum(counts) if cap is None else cap
    cum = torch.tensor(np.concatenate(([0], np.cumsum(counts))), dtype=torch.int64, device=DEV)
    lab = torch.zeros(cap, dtype=torch.int64, device=DEV)
    box = torch.zeros((cap, 4), dtype=torch.float32, device=DEV)
    lab[:sum(counts)] = torch.as_tensor(np.asarray(labels, dtype=np.int64), device=DEV)
    box[:sum(counts)] = torch.as_tensor(np.asarray(boxes, dtype=np.float32).reshape(-1, 4), device=DEV)
    return cum, lab, box


def _run(counts, labels, boxes, uniform, table, cap=None, **kw):
    from richsem_amd.dn import denoising_queries
    cum, lab, box = _device_inputs(counts, labels, boxes, cap)
    out = _poisoned(len(counts), kw["pad_cap"], kw["num_queries"], table.shape[1])
    q_label, q_bbox, mask, noised_label, meta = denoising_queries(cum, lab, box, torch.as_tensor(table, device=DEV),
                                                                  torch.as_tensor(uniform, device=DEV), out=out, **kw)
    torch.cuda.synchronize()
    assert mask.dtype == torch.bool and q_label.data_ptr() == out["q_label"].data_ptr()
    got = {"q_label": q_label, "q_bbox": q_bbox, "attn_mask": mask.view(torch.uint8), "noised_label": noised_label, "meta": meta,
           "noised_box": out["noised_box"]}
    return {k: v.cpu().numpy() for k, v in got.items()}


def _check(got, want):
    """bit equality with the restatement for everything but q_bbox; q_bbox within the bound; nothing left unwritten"""
    assert got["meta"].tolist() == want["meta"].tolist()
    assert np.array_equal(got["noised_label"], want["noised_label"])
    assert got["attn_mask"].max(initial=0) <= 1 and np.array_equal(got["attn_mask"].astype(bool), want["attn_mask"])
    assert got["noised_box"].tobytes() == want["noised_box"].tobytes()
    assert got["q_label"].tobytes() == want["q_label"].tobytes()
    y64, bound = R.q_bbox_bound(want["noised_box"])
    filled = want["noised_label"] >= 0
    assert not np.isnan(got["q_bbox"]).any() and not got["q_bbox"][~filled].any()
    err = np.abs(got["q_bbox"].astype(np.float64) - y64)
    assert (err[filled] <= bound[filled]).all(), float((err / bound)[filled].max())


def _golden_case(golden, name):
    z = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + ".")}
    hidden, nq, ncls = (int(v) for v in golden["dims"])
    dn_number, use_cdn, add_gt = (int(v) for v in z["args"])
    ratio, scale = (float(v) for v in z["noise"])
    kw = dict(num_queries=nq, num_classes=ncls, dn_number=dn_number, label_noise_ratio=ratio, box_noise_scale=scale, use_cdn=bool(use_cdn),
              add_gt=bool(add_gt))
    return z, kw, ncls


@pytest.mark.parametrize("name", CASES)
def test_every_fixture_case_at_the_exact_layout(golden, name):
    z, kw, ncls = _golden_case(golden, name)
    pad = int(z["meta"][0])
    u = R.uniform_from_draws(z["counts"], z["p"], z["new_label"], z["sign01"], z["rand"], ncls, pad, kw["use_cdn"])
    got = _run(z["counts"], z["labels"], z["boxes"], u, golden["table"], pad_cap=pad, **kw)
    # the reference's own outputs ...
    assert got["meta"][2] == z["meta"][0] and got["meta"][1] == z["meta"][1] and got["meta"][4] == 0
    assert got["q_label"].shape == z["input_query_label"].shape and got["q_label"].tobytes() == z["input_query_label"].tobytes()
    assert np.array_equal(got["attn_mask"].astype(bool), z["attn_mask"])
    groups2 = len(z["p"]) // max(len(z["labels"]), 1)
    rows = R.rows_from_slots(z["counts"], got["noised_box"], groups2, kw["use_cdn"])
    kept = ~np.isnan(rows[:, 0])
    assert rows[kept].tobytes() == z["noised_box_rows"][kept].tobytes()
    # ... and the restatement, element by element
    _check(got, R.denoising_queries_ref(z["counts"], z["labels"], z["boxes"], u, golden["table"], pad_cap=pad, **kw))


def _random_case(counts, D=16, V=8, seed=0, edge=False):
    rng = np.random.default_rng(seed)
    n = sum(counts)
    cxcy = rng.uniform(0.0, 1.0, (n, 2)) if edge else rng.uniform(0.2, 0.8, (n, 2))
    boxes = np.concatenate((cxcy, rng.uniform(0.05, 0.5, (n, 2))), 1).astype(np.float32)
    return rng.integers(0, V - 1, n), boxes, rng.standard_normal((V, D)).astype(np.float32), rng      # (class V - 1 is never a target)


KW = dict(num_queries=30, num_classes=7, dn_number=100, label_noise_ratio=0.5, box_noise_scale=1.0)


@pytest.mark.parametrize("counts,pad_cap,D", [((3, 7), 196, 16), ((3, 0, 7), 196, 16), ((12, 12), 200, 16), ((60, 60), 240, 16), ((0, 0), 0, 16),
                                              ((0, 0), 24, 16), ((12, 12), 200, 256), ((1,), 200, 24)])
def test_random_uniforms_against_the_restatement(counts, pad_cap, D):
    """uniforms drawn as the caller draws them (any value in [0, 1), not the fixture's four encodings); D = 256 once; D = 24: a row that is
    not a multiple of a wave's 16-byte pieces; more than one workgroup of rows and of mask bytes everywhere"""
    labels, boxes, table, rng = _random_case(counts, D=D, seed=len(counts) + pad_cap, edge=True)
    u = rng.random((len(counts), pad_cap, 10), dtype=np.float32)
    got = _run(counts, labels, boxes, u, table, pad_cap=pad_cap, **KW)
    want = R.denoising_queries_ref(counts, labels, boxes, u, table, pad_cap=pad_cap, **KW)
    assert want["meta"][4] == 0
    _check(got, want)


@pytest.mark.parametrize("pad_cap", [40, 64])
def test_capacity_form(pad_cap):
    counts, kw = (3, 7), dict(KW, dn_number=1)      # dn_number * 2 = 2 < 100: 2 groups, pad_size 28
    labels, boxes, table, rng = _random_case(counts, seed=5)
    pad = R.layout(counts, 1)[2]
    assert pad == 28 < pad_cap
    u = rng.random((2, pad_cap, 10), dtype=np.float32)
    exact = _run(counts, labels, boxes, u[:, :pad].copy(), table, pad_cap=pad, **kw)
    got = _run(counts, labels, boxes, u, table, pad_cap=pad_cap, cap=16, **kw)      # (target buffers with room to spare as well)
    _check(got, R.denoising_queries_ref(counts, labels, boxes, u, table, pad_cap=pad_cap, **kw))
    assert got["meta"].tolist() == exact["meta"].tolist() == [7, 2, 28, 10, 0]
    for k in ("q_label", "q_bbox", "noised_box", "noised_label"):
        assert got[k][:, :pad].tobytes() == exact[k].tobytes(), k
        assert not got[k][:, pad:].any() if k != "noised_label" else (got[k][:, pad:] == -1).all(), k
    m, nq = got["attn_mask"].astype(bool), kw["num_queries"]
    keep = np.r_[0:pad, pad_cap:pad_cap + nq]
    assert np.array_equal(m[np.ix_(keep, keep)], exact["attn_mask"].astype(bool))      # the reference's mask as a sub-matrix
    assert m[:, pad:pad_cap].all()                                                     # nobody sees a tail slot
    assert m[pad:pad_cap, :pad_cap].all() and not m[pad:pad_cap, pad_cap:].any()       # a tail row sees the matching queries only
    assert not m.all(axis=1).any()                                                     # no row is fully masked
    empty = np.ones((2, pad_cap), bool)
    for b, c in enumerate(counts):
        for g2 in range(4):
            empty[b, g2 * 7:g2 * 7 + c] = False
    assert np.array_equal(got["noised_label"] == -1, empty)


def test_overflow_is_reported_and_leaves_every_slot_empty():
    from richsem_amd.dn import dn_capacity
    counts = (30, 2)
    labels, boxes, table, rng = _random_case(counts, seed=9)
    for pad_cap, overflow in ((40, 1), (dn_capacity(100, 30), 0)):
        u = rng.random((2, pad_cap, 10), dtype=np.float32)
        got = _run(counts, labels, boxes, u, table, pad_cap=pad_cap, **KW)
        want = R.denoising_queries_ref(counts, labels, boxes, u, table, pad_cap=pad_cap, **KW)
        _check(got, want)
        assert got["meta"][4] == overflow and got["meta"][2] == (0 if overflow else 180)
        if overflow:
            assert (got["noised_label"] == -1).all() and not got["q_label"].any() and not got["q_bbox"].any()
            m = got["attn_mask"].astype(bool)
            assert m[:, :pad_cap].all() and not m[:, pad_cap:].any()
    # targets that do not fit the caller's label / box buffers: the same answer, and nothing is read past them
    u = rng.random((2, 200, 10), dtype=np.float32)
    from richsem_amd.dn import denoising_queries
    cum, lab, box = _device_inputs(counts, labels, boxes)
    out = _poisoned(2, 200, 30, 16)
    res = denoising_queries(cum, lab[:20].contiguous(), box[:20].contiguous(), torch.as_tensor(table, device=DEV), torch.as_tensor(u, device=DEV),
                            pad_cap=200, out=out, **KW)
    assert res[4].tolist() == [30, 3, 0, 32, 1] and (res[3] == -1).all() and not res[0].any()


def test_a_captured_call_follows_the_counts():
    from richsem_amd.capture import capture, capture_stream
    from richsem_amd.dn import denoising_queries, dn_buffers
    pad_cap, cap, kw = 96, 16, dict(KW, dn_number=2)      # 4 groups: pad_size 56 for (3, 7), 96 for (12, 0), 8 for (1, 1)
    batches = [(3, 7), (12, 0), (1, 1), (3, 7)]
    data = {}
    for i, counts in enumerate(batches):
        labels, boxes, table, rng = _random_case(counts, seed=20 + i % 3)
        data[i] = (counts, labels, boxes, rng.random((2, pad_cap, 10), dtype=np.float32))
    table = torch.as_tensor(table, device=DEV)

    def eager(i):
        counts, labels, boxes, u = data[i]
        cum, lab, box = _device_inputs(counts, labels, boxes, cap)
        res = denoising_queries(cum, lab, box, table, torch.as_tensor(u, device=DEV), pad_cap=pad_cap, **kw)
        torch.cuda.synchronize()
        return [t.clone() for t in res]

    with capture_stream() as side:
        cum, lab, box = _device_inputs(*data[0][:3], cap)
        uni = torch.as_tensor(data[0][3], device=DEV)
        out = dn_buffers(2, pad_cap, kw["num_queries"], 16, DEV)
        first = denoising_queries(cum, lab, box, table, uni, pad_cap=pad_cap, out=out, **kw)      # eager once; its buffers are the graph's outputs
        torch.cuda.synchronize()
        graph, res = capture(lambda: denoising_queries(cum, lab, box, table, uni, pad_cap=pad_cap, out=out, **kw), side)
        assert [t.data_ptr() for t in res] == [t.data_ptr() for t in first]
        for i in (1, 2, 3):
            c2, l2, b2 = _device_inputs(*data[i][:3], cap)
            cum.copy_(c2), lab.copy_(l2), box.copy_(b2), uni.copy_(torch.as_tensor(data[i][3], device=DEV))
            graph.replay()
            torch.cuda.synchronize()
            want = eager(i)
            for a, b in zip(res, want):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
            assert res[4].tolist() == [max(data[i][0]), 4, 8 * max(data[i][0]), sum(data[i][0]), 0]


def test_backward_is_the_embedding_gradient_in_a_fixed_order():
    from richsem_amd.dn import denoising_queries, _dn_backward
    counts, V, D, pad_cap = (12, 9), 8, 16, 200
    labels, boxes, table, rng = _random_case(counts, D=D, V=V, seed=31)
    u = rng.random((2, pad_cap, 10), dtype=np.float32)
    cum, lab, box = _device_inputs(counts, labels, boxes)
    tab = torch.as_tensor(table, device=DEV).requires_grad_(True)
    kw = dict(KW, num_classes=V - 1)      # classes 0 .. 6 are drawn and are targets: row 7 of the table is never looked up
    q_label, _, _, noised_label, meta = denoising_queries(cum, lab, box, tab, torch.as_tensor(u, device=DEV), pad_cap=pad_cap, **kw)
    assert meta.tolist() == [12, 8, 192, 21, 0]
    g = torch.randn(q_label.shape, device=DEV)
    grad, = torch.autograd.grad(q_label, tab, g)
    torch.cuda.synchronize()
    nl = noised_label.flatten()
    hits = torch.bincount(nl[nl >= 0], minlength=V)
    assert hits[:V - 1].min() > 10 and hits[V - 1] == 0
    t64 = torch.as_tensor(table, device=DEV).double().requires_grad_(True)
    torch.nn.functional.embedding(nl.clamp(min=0), t64).mul((nl >= 0)[:, None]).backward(g.reshape(-1, D).double())
    abs_sum = torch.zeros(V, D, device=DEV, dtype=torch.float64).index_add_(0, nl.clamp(min=0), (g.reshape(-1, D).double().abs() * (nl >= 0)[:, None]))
    bound = (hits - 1).clamp(min=0)[:, None].double() * 2.0 ** -24 * abs_sum
    assert ((grad.double() - t64.grad).abs() <= bound).all()
    assert not grad[V - 1].any() and not torch.isnan(grad).any()
    # the raw call into a NaN-filled buffer is not what is tested above (the wrapper allocates), so: twice more, bit-identical
    again = [_dn_backward(g, noised_label, V) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(again[0].view(torch.int32), grad.view(torch.int32)) and torch.equal(again[1].view(torch.int32), grad.view(torch.int32))


def test_backward_writes_every_row_of_a_poisoned_table_gradient():
    from richsem_amd import _lib
    V, D, rows = 11, 24, 130      # more rows than a ballot takes at once; D / 4 = 6 lanes of a wave
    rng = np.random.default_rng(3)
    nl = torch.as_tensor(rng.integers(-1, V - 1, rows), device=DEV)
    g = torch.randn(rows, D, device=DEV)
    grad = torch.full((V, D), float("nan"), device=DEV)
    _lib.check(_lib.load().msda_dn_queries_backward_f32(g.data_ptr(), nl.data_ptr(), rows, D, V, grad.data_ptr(), _lib.raw_stream(g.device)))
    torch.cuda.synchronize()
    ok = (nl >= 0)[:, None]
    want = torch.zeros(V, D, device=DEV, dtype=torch.float64).index_add_(0, nl.clamp(min=0), g.double() * ok)
    abs_sum = torch.zeros(V, D, device=DEV, dtype=torch.float64).index_add_(0, nl.clamp(min=0), g.double().abs() * ok)
    hits = torch.bincount(nl[nl >= 0], minlength=V)
    assert not torch.isnan(grad).any() and not grad[V - 1].any() and hits.max() > 2
    assert ((grad.double() - want).abs() <= (hits - 1).clamp(min=0)[:, None].double() * 2.0 ** -24 * abs_sum).all()
