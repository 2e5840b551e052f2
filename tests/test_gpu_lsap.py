"""GPU (-m gpu): the on-device Hungarian solver (msda_lsap_*, csrc/msda_lsap.h) against scipy.optimize.linear_sum_assignment on the same
cost values cast to float64.  Gates: validity (every target of a block with T <= Q has a query in [0, Q), no query twice; with T > Q
exactly Q targets matched), optimality (float64 total equal to scipy's to 1e-9 * max(1, |total|): rounding of a few hundred float64
additions, orders of magnitude below the gap to a second-best assignment), and index equality only where the optimum is unique."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from richsem_amd.capture import capture  # noqa: E402
from tests.test_oracle_matcher import make_case  # noqa: E402

pytestmark = pytest.mark.gpu

W = dict(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
SHAPES = [(1, 1), (40, 0), (40, 5), (40, 57), (120, 12), (900, 12), (900, 100), (900, 300), (900, 900), (1100, 250), (4096, 64)]


def dummy_plan(sizes, dtype=torch.float32):
    from richsem_amd.matcher import CostPlan
    targets = [{"labels": torch.zeros(s, dtype=torch.int64), "boxes": torch.zeros(s, 4)} for s in sizes]
    return CostPlan(targets, torch.device("cuda"), dtype)


def solve(blocks, target_major, dtype):
    """blocks[o][b]: (Q, T_b) numpy arrays -> (query_of_target (n_out, Ttot), status (n_out, B)) as numpy, through msda_lsap_*"""
    from richsem_amd.matcher import solve_blocks
    Q = blocks[0][0].shape[0]
    sizes = [blk.shape[1] for blk in blocks[0]]
    flat = np.concatenate([(blk.T if target_major else blk).reshape(-1) for out in blocks for blk in out]) if sum(sizes) * Q else np.zeros(0)
    plan = dummy_plan(sizes)
    cost = torch.from_numpy(flat.astype(dtype)).cuda()
    qot, status = solve_blocks(cost, plan, len(blocks), Q, target_major)
    torch.cuda.synchronize()
    return qot.cpu().numpy(), status.cpu().numpy()


def check_block(block, q, tag="", equal=False):
    """validity + optimality of one block's answer ``q`` (query per target) against scipy on the float64 block"""
    block = np.asarray(block, dtype=np.float64)
    Q, T = block.shape
    matched = np.nonzero(q >= 0)[0]
    assert len(matched) == min(Q, T), (tag, len(matched), Q, T)
    assert ((q[matched] >= 0) & (q[matched] < Q)).all(), tag
    assert len(set(q[matched].tolist())) == len(matched), tag
    if T == 0:
        return
    i, j = linear_sum_assignment(block)
    want, got = block[i, j].sum(), block[q[matched], matched].sum()
    print(f"{tag}: total {got!r} scipy {want!r} diff {abs(got - want):.3e}")
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (tag, got, want)
    if equal:
        order = np.argsort(q[matched])
        assert q[matched][order].tolist() == i.tolist() and matched[order].tolist() == j.tolist(), tag


def check_all(blocks, qot, status, tag="", equal=False):
    assert (status == 0).all(), (tag, status)
    for o, out in enumerate(blocks):
        t0 = 0
        for b, blk in enumerate(out):
            check_block(blk, qot[o, t0:t0 + blk.shape[1]], f"{tag} o{o} b{b} {blk.shape}", equal)
            t0 += blk.shape[1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("target_major", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_blocks(shape, target_major, dtype):
    Q, T = shape
    rng = np.random.default_rng(Q * 10007 + T)
    blocks = [[rng.normal(size=(Q, T)).astype(dtype)]]
    qot, status = solve(blocks, target_major, dtype)
    check_all(blocks, qot, status, f"random tm={target_major} {dtype.__name__}", equal=True)      # (continuous random costs: unique optimum)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_out", [1, 7])
@pytest.mark.parametrize("sizes", [(5, 0, 57, 1, 12), (100, 300), (250, 40, 900, 0)], ids=str)
def test_ragged_batches_one_launch(sizes, n_out, dtype):
    Q = {(5, 0, 57, 1, 12): 40, (100, 300): 900, (250, 40, 900, 0): 900}[sizes]
    rng = np.random.default_rng(len(sizes) * 31 + n_out)
    blocks = [[rng.normal(size=(Q, t)).astype(dtype) for t in sizes] for _ in range(n_out)]
    for tm in (False, True):
        qot, status = solve(blocks, tm, dtype)
        check_all(blocks, qot, status, f"ragged tm={tm}", equal=True)


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
@pytest.mark.parametrize("n_out,nq,sizes", [(1, 40, (5, 57)), (7, 900, (12, 12)), (7, 900, (100, 37, 0)), (1, 1100, (250,)), (1, 120, (12, 1))])
def test_costs_from_the_cost_kernel(n_out, nq, sizes, tdt):
    """the project's cost kernel on random logits / boxes (as tests/test_gpu_matcher.py draws them), both layouts, through
    match_many_device; expected: scipy on the query-major blocks the host path would have copied"""
    from richsem_amd.matcher import CostPlan, HungarianMatcher, cost_blocks
    ndt = np.float32 if tdt == torch.float32 else np.float64
    _, _, labels, tboxes = make_case(1, bs=len(sizes), nq=1, C=80, sizes=sizes, dtype=ndt)
    targets = [{"labels": torch.from_numpy(l).cuda(), "boxes": torch.from_numpy(b).cuda().to(tdt)} for l, b in zip(labels, tboxes)]
    plan = CostPlan(targets, torch.device("cuda"), tdt)
    outs = []
    for o in range(n_out):
        logits, boxes, _, _ = make_case(50 + o, bs=len(sizes), nq=nq, C=80, sizes=sizes, dtype=ndt)
        outs.append({"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(boxes).cuda()})
    m = HungarianMatcher(**W, solver="device")
    blocks = []
    for o in outs:
        flat = cost_blocks(o["pred_logits"], o["pred_boxes"], plan, W["cost_class"], W["cost_bbox"], W["cost_giou"], 0.25).cpu().numpy()
        blocks.append([flat[nq * plan.offsets[b]: nq * plan.offsets[b + 1]].reshape(nq, s) for b, s in enumerate(plan.sizes)])
    for tm in (True, False):
        qot, status = m.match_many_device(outs, plan, target_major=tm)
        assert qot.shape == (n_out, plan.total) and qot.dtype == torch.int64 and status.shape == (n_out, len(sizes)) and status.dtype == torch.int32
        check_all(blocks, qot.cpu().numpy(), status.cpu().numpy(), f"kernel costs tm={tm}")
    # the list format: sorted by query, int64, equal to the host solver's pair set in total cost
    lists = m.match_many(outs, targets)
    host = HungarianMatcher(**W).match_many(outs, targets)
    for o in range(n_out):
        for b, ((gi, gj), (hi, hj)) in enumerate(zip(lists[o], host[o])):
            assert gi.dtype == torch.int64 and gj.dtype == torch.int64 and len(gi) == len(hi)
            assert gi.tolist() == sorted(gi.tolist())
            blk = blocks[o][b].astype(np.float64)
            got, want = blk[gi.numpy(), gj.numpy()].sum(), blk[hi.numpy(), hj.numpy()].sum()
            assert abs(got - want) <= 1e-9 * max(1.0, abs(want))


def test_outputs_with_different_query_counts():
    from richsem_amd.matcher import HungarianMatcher
    sizes = (7, 0, 9)
    _, _, labels, tboxes = make_case(0, bs=3, nq=1, C=80, sizes=sizes, dtype=np.float32)
    targets = [{"labels": torch.from_numpy(l).cuda(), "boxes": torch.from_numpy(b).cuda()} for l, b in zip(labels, tboxes)]
    outs = []
    for o, nq in enumerate([300, 300, 200]):
        logits, boxes, _, _ = make_case(100 + o, bs=3, nq=nq, C=80, sizes=sizes, dtype=np.float32)
        outs.append({"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(boxes).cuda()})
    got = HungarianMatcher(**W, solver="device").match_many(outs, targets)
    want = HungarianMatcher(**W).match_many(outs, targets)
    for g, w in zip(got, want):
        for (gi, gj), (wi, wj) in zip(g, w):
            assert gi.tolist() == wi.tolist() and gj.tolist() == wj.tolist()


def test_long_augmenting_paths_product_costs():
    """cost[t][q] = (t + 1) * (q + 1) at 200 x 200: unique optimum by the rearrangement inequality (target t <-> query 199 - t), long paths"""
    n = 200
    block = np.outer(np.arange(1, n + 1), np.arange(1, n + 1)).astype(np.float64)      # (Q, T), symmetric
    for dtype in (np.float32, np.float64):
        for tm in (False, True):
            qot, status = solve([[block]], tm, dtype)
            check_all([[block]], qot, status, "product", equal=True)
            assert qot[0].tolist() == list(range(n - 1, -1, -1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties_and_scales(dtype):
    rng = np.random.default_rng(5)
    cases = {
        "small integers": rng.integers(0, 4, size=(60, 45)).astype(np.float64),
        "small integers T > Q": rng.integers(0, 3, size=(30, 50)).astype(np.float64),
        "all equal": np.full((50, 20), 0.75),
        "all zero square": np.zeros((33, 33)),
        "mixed sign": rng.normal(size=(128, 64)) * 3.0 - 1.0,
        "1e6": rng.normal(size=(100, 70)) * 1e6,
        "1e-6": rng.normal(size=(100, 70)) * 1e-6,
    }
    dup = rng.normal(size=(90, 20))
    dup[:, 10:] = dup[:, :10]                      # duplicated target columns (duplicate ground-truth boxes with one label)
    cases["duplicated targets"] = dup
    for name, block in cases.items():
        block = block.astype(dtype)
        for tm in (False, True):
            qot, status = solve([[block]], tm, dtype)
            check_all([[block]], qot, status, name)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_blocks_are_reported_and_the_rest_solved(bad):
    from richsem_amd.matcher import HungarianMatcher
    rng = np.random.default_rng(9)
    blocks = [[rng.normal(size=(64, t)).astype(np.float32) for t in (9, 20, 70)] for _ in range(3)]
    blocks[1][1][17, 3] = bad
    blocks[2][2][0, 69] = bad
    for tm in (False, True):
        qot, status = solve(blocks, tm, np.float32)
        want = np.zeros((3, 3), dtype=np.int32)
        want[1, 1] = want[2, 2] = 1
        assert (status == want).all(), status
        assert (qot[1, 9:29] == -1).all() and (qot[2, 29:] == -1).all()
        for o in range(3):
            t0 = 0
            for b, blk in enumerate(blocks[o]):
                if want[o, b] == 0:
                    check_block(blk, qot[o, t0:t0 + blk.shape[1]], f"beside non-finite o{o} b{b}", equal=True)
                t0 += blk.shape[1]
    # the list form raises as scipy does
    logits, boxes, labels, tboxes = make_case(5, nq=37, C=50, sizes=(5, 3), dtype=np.float32)
    logits[1, 4, :] = bad if not np.isinf(bad) else np.nan      # (an infinite logit gives a finite cost; NaN poisons it)
    targets = [{"labels": torch.from_numpy(l).cuda(), "boxes": torch.from_numpy(b).cuda()} for l, b in zip(labels, tboxes)]
    out = {"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(boxes).cuda()}
    with pytest.raises(ValueError, match="invalid numeric entries"):
        HungarianMatcher(**W, solver="device")(out, targets)


def test_too_large_is_refused_before_any_launch():
    import ctypes
    from richsem_amd import _lib
    from richsem_amd.matcher import LSAP_MAX_DIM, lsap_supported, solve_blocks
    L = _lib.load()
    n = ctypes.c_int64(-1)
    assert L.msda_lsap_workspace_bytes(7, 2, LSAP_MAX_DIM, LSAP_MAX_DIM, ctypes.byref(n)) == 0 and n.value >= 0
    assert L.msda_lsap_workspace_bytes(7, 2, LSAP_MAX_DIM + 1, 10, ctypes.byref(n)) == -4
    assert L.msda_lsap_workspace_bytes(7, 2, 900, LSAP_MAX_DIM + 1, ctypes.byref(n)) == -4
    # fake pointers: a launch would fault, the refusal comes first
    assert L.msda_lsap_f32(0x1000, 0, 0x1000, 1, 1, LSAP_MAX_DIM + 1, 10, 0x1000, 0x1000, None, None) == -4
    assert "msda_lsap" in _lib.last_error() or "lsap_impl" in _lib.last_error()
    assert L.msda_lsap_f64(0x1000, 1, 0x1000, 1, 1, 900, LSAP_MAX_DIM + 1, 0x1000, 0x1000, None, None) == -4
    assert L.msda_lsap_f32(0x1000, 0, None, 1, 1, 10, 10, 0x1000, 0x1000, None, None) == -1
    assert L.msda_lsap_f32(0x1000, 0, 0x1000, 0, 1, 10, 10, 0x1000, 0x1000, None, None) == -2
    assert lsap_supported(LSAP_MAX_DIM, LSAP_MAX_DIM) and not lsap_supported(LSAP_MAX_DIM + 1, 1) and not lsap_supported(1, LSAP_MAX_DIM + 1)
    plan = dummy_plan([3])
    with pytest.raises(RuntimeError, match="MSDA_ERR_TOO_LARGE"):
        solve_blocks(torch.zeros(3 * (LSAP_MAX_DIM + 1), device="cuda"), plan, 1, LSAP_MAX_DIM + 1)
    torch.cuda.synchronize()


def test_the_largest_supported_problem():
    """Q = 4096 against 4096 targets in one image: the 148 KB of LDS state"""
    rng = np.random.default_rng(4096)
    block = rng.normal(size=(4096, 4096)).astype(np.float32)
    qot, status = solve([[block]], True, np.float32)
    check_all([[block]], qot, status, "4096 x 4096", equal=True)


def test_device_solver_equals_the_reference_matcher_fixture():
    """tests/golden/matcher_hungarian.npz: the indices the reference's HungarianMatcher.forward returned, f32 and f64, including the image
    without targets (each non-empty block's optimum is unique)"""
    from richsem_amd.matcher import HungarianMatcher
    from tests.test_oracle_matcher import _fixture_cases
    n = 0
    for tag, tol, logits, boxes, labels, tboxes, offs, blocks, idx in _fixture_cases():
        tdt = torch.float64 if tag == "f64" else torch.float32
        targets = [{"labels": torch.from_numpy(l).cuda(), "boxes": torch.from_numpy(b).cuda().to(tdt)} for l, b in zip(labels, tboxes)]
        res = HungarianMatcher(**W, focal_alpha=0.25, solver="device")({"pred_logits": torch.from_numpy(logits).cuda(),
                                                                        "pred_boxes": torch.from_numpy(boxes).cuda()}, targets)
        assert len(res) == len(idx)
        for (gi, gj), (wi, wj) in zip(res, idx):
            assert gi.dtype == torch.int64 and gj.dtype == torch.int64
            assert gi.tolist() == wi.tolist() and gj.tolist() == wj.tolist(), tag
            n += 1
    assert n >= 4


def test_match_many_device_is_graph_safe():
    """captured into a graph after a warm-up; replayed on new logits / boxes written into the static inputs and on new per-image
    counts under the same total (CostPlan.update_); every replay equals a fresh eager solve.  No host synchronisation inside the call."""
    from richsem_amd.matcher import CostPlan, HungarianMatcher
    nq, C, n_out = 300, 80, 3
    m = HungarianMatcher(**W, solver="device")

    def draw(seed, sizes):
        _, _, labels, tboxes = make_case(seed, bs=len(sizes), nq=1, C=C, sizes=sizes, dtype=np.float32)
        targets = [{"labels": torch.from_numpy(l).cuda(), "boxes": torch.from_numpy(b).cuda()} for l, b in zip(labels, tboxes)]
        outs = []
        for o in range(n_out):
            logits, boxes, _, _ = make_case(seed * 10 + o, bs=len(sizes), nq=nq, C=C, sizes=sizes, dtype=np.float32)
            outs.append({"pred_logits": torch.from_numpy(logits).cuda(), "pred_boxes": torch.from_numpy(boxes).cuda()})
        return outs, targets

    outs, targets = draw(1, (20, 30))
    plan = CostPlan(targets, torch.device("cuda"), torch.float32)
    static = [{k: v.clone() for k, v in o.items()} for o in outs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.match_many_device(static, plan)                 # eager warm-up
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")           # (a synchronising torch call inside would raise)
        try:
            m.match_many_device(static, plan)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        g, (qot, status) = capture(lambda: m.match_many_device(static, plan), side)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for seed, sizes in ((1, (20, 30)), (2, (20, 30)), (3, (41, 9)), (4, (0, 50))):
        outs, targets = draw(seed, sizes)
        for s, o in zip(static, outs):
            s["pred_logits"].copy_(o["pred_logits"])
            s["pred_boxes"].copy_(o["pred_boxes"])
        plan.update_(targets)
        g.replay()
        torch.cuda.synchronize()
        fresh_q, fresh_s = m.match_many_device(outs, CostPlan(targets, torch.device("cuda"), torch.float32))
        assert torch.equal(qot, fresh_q) and torch.equal(status, fresh_s) and int(status.abs().sum()) == 0
        want = HungarianMatcher(**W).match_many(outs, targets)
        for o in range(n_out):
            for b, (wi, wj) in enumerate(want[o]):
                assert qot[o, plan.offsets[b] + wj].cpu().tolist() == wi.tolist()
        seen.append(qot.cpu().clone())
    assert not torch.equal(seen[0], seen[1])
    with pytest.raises(ValueError):
        plan.update_(draw(5, (20, 31))[1])
    with pytest.raises(ValueError):
        plan.update_(draw(5, (20, 20, 10))[1])
