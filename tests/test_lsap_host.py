"""CPU: the host-side pieces around the on-device Hungarian solver (richsem_amd/matcher.py): the ``solver`` keyword, the unchanged host
path on the committed fixture, ``pairs_from_query_of_target`` against a hand-built case and against ``Step.pack_indices``' layout,
``CostPlan.update_`` and the late status read.  No kernel is launched here."""
import types

import numpy as np
import pytest
import torch

from richsem_amd import matcher as M

from test_oracle_matcher import _fixture_cases


def _targets(sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"labels": torch.randint(0, 50, (s,), generator=g), "boxes": torch.rand(s, 4, generator=g)} for s in sizes]


def test_solver_keyword():
    assert M.HungarianMatcher().solver == "host"
    assert M.HungarianMatcher(2.0, 5.0, 2.0, solver="device").solver == "device"
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="solver"):
            M.HungarianMatcher(solver=bad)
    with pytest.raises(AssertionError):
        M.HungarianMatcher(0, 0, 0, solver="device")
    # CPU tensors are refused by both forms, as before
    out = {"pred_logits": torch.zeros(1, 4, 5), "pred_boxes": torch.rand(1, 4, 4)}
    for solver in ("host", "device"):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            M.HungarianMatcher(solver=solver)(out, _targets([2]))


def test_host_assignment_on_the_reference_fixture_is_unchanged():
    """the host path's solve (scipy on the copied blocks) returns the indices the reference's HungarianMatcher returned"""
    n = 0
    for tag, tol, logits, boxes, labels, tboxes, offs, blocks, idx in _fixture_cases():
        dt = torch.float64 if tag == "f64" else torch.float32
        targets = [{"labels": torch.from_numpy(l), "boxes": torch.from_numpy(b)} for l, b in zip(labels, tboxes)]
        plan = M.CostPlan(targets, "cpu", dt)
        nq = logits.shape[1]
        flat = torch.cat([torch.from_numpy(np.ascontiguousarray(b)).reshape(-1) for b in blocks])
        res = M._assign(flat, nq, plan)
        for (gi, gj), (wi, wj) in zip(res, idx):
            assert gi.tolist() == wi.tolist() and gj.tolist() == wj.tolist()
            n += 1
    assert n >= 4


def test_pairs_from_query_of_target_hand_built():
    plan = M.CostPlan(_targets([2, 0, 3]), "cpu", torch.float32)
    qot = torch.tensor([[5, 1, 7, 0, 2],        # decoder output 0
                        [4, 4, 1, 2, 3],        # decoder output 1 (the last decoder layer)
                        [9, 8, 0, 6, 5]])       # the two-stage output
    dec, inter, dis = M.pairs_from_query_of_target(qot, plan, num_queries=10)
    assert dec.dtype == torch.int64 and dec.shape == (4, 10) and inter.shape == (4, 5) and dis.shape == (4, 5)
    assert dec.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 2, 2, 2, 0, 0, 2, 2, 2], [5, 1, 7, 0, 2, 4, 4, 1, 2, 3], [0, 1, 2, 3, 4, 0, 1, 2, 3, 4]]
    assert inter.tolist() == [[0] * 5, [0, 0, 2, 2, 2], [9, 8, 0, 6, 5], [0, 1, 2, 3, 4]]
    assert dis.tolist() == [[0] * 5, [0, 0, 2, 2, 2], [4, 4, 1, 2, 3], [0, 1, 2, 3, 4]]
    # a block that was not solved: -1 is clamped (the status reports it), never an index
    qot[0, 3] = -1
    assert int(M.pairs_from_query_of_target(qot, plan, num_queries=10)[0].min()) == 0
    # the image index follows update_ (device offsets), not the lists the plan was built from
    plan.update_(_targets([1, 4, 0]))
    assert M.pairs_from_query_of_target(qot, plan, num_queries=10)[1][1].tolist() == [0, 1, 1, 1, 1]


def test_pairs_equal_pack_indices_layout():
    """the same pair SET as Step.pack_indices builds from the host matcher's lists, in target order instead of query order"""
    import bench_step
    sizes, nq, n_out = [4, 0, 6], 11, 4
    targets = _targets(sizes, seed=3)
    plan = M.CostPlan(targets, "cpu", torch.float32)
    g = torch.Generator().manual_seed(1)
    qot = torch.stack([torch.cat([torch.randperm(nq, generator=g)[:s] for s in sizes]) for _ in range(n_out)])
    lists = M.HungarianMatcher._lists_from_device(qot, torch.zeros(n_out, len(sizes), dtype=torch.int32), plan)
    for per_output in lists:
        for (i, j), s in zip(per_output, sizes):
            assert len(i) == s and i.tolist() == sorted(i.tolist()) and i.dtype == torch.int64 and j.dtype == torch.int64
    fake_step = types.SimpleNamespace(level_embed=torch.zeros(1))
    labels, boxes, dec, inter, dis = bench_step.Step.pack_indices(fake_step, lists, targets)
    got = M.pairs_from_query_of_target(qot, plan, num_queries=nq)
    for a, b in zip(got, (dec, inter, dis)):
        assert a.shape == b.shape
        assert sorted(map(tuple, a.t().tolist())) == sorted(map(tuple, b.t().tolist()))
    assert torch.equal(labels, plan.tgt_ids) and torch.equal(boxes, plan.tgt_boxes)


def test_more_targets_than_queries_is_rejected():
    plan = M.CostPlan(_targets([3, 8]), "cpu", torch.float32)
    qot = torch.zeros(3, 11, dtype=torch.int64)
    with pytest.raises(ValueError, match="8 targets against 5 queries"):
        M.pairs_from_query_of_target(qot, plan, num_queries=5)
    plan.num_queries = 7                      # (what match_many_device records)
    with pytest.raises(ValueError, match="8 targets against 7 queries"):
        M.pairs_from_query_of_target(qot, plan)
    M.pairs_from_query_of_target(qot, plan, num_queries=8)
    # the list form still serves T > Q: exactly Q targets matched, the rest skipped
    q = torch.tensor([[2, -1, 0, 1, -1]])
    (i, j), = M.HungarianMatcher._lists_from_device(q, torch.zeros(1, 1, dtype=torch.int32), M.CostPlan(_targets([5]), "cpu", torch.float32))[0]
    assert i.tolist() == [0, 1, 2] and j.tolist() == [2, 3, 0]
    with pytest.raises(ValueError, match="invalid numeric entries"):
        M.HungarianMatcher._lists_from_device(q, torch.ones(1, 1, dtype=torch.int32), M.CostPlan(_targets([5]), "cpu", torch.float32))


def test_cost_plan_update():
    t0, t1 = _targets([3, 2], seed=1), _targets([1, 4], seed=2)
    plan = M.CostPlan(t0, "cpu", torch.float64)
    ptrs = (plan.offsets_dev.data_ptr(), plan.tgt_ids.data_ptr(), plan.tgt_boxes.data_ptr())
    assert plan.update_(t1) is plan
    assert ptrs == (plan.offsets_dev.data_ptr(), plan.tgt_ids.data_ptr(), plan.tgt_boxes.data_ptr())      # the buffers a capture recorded
    assert plan.sizes == [1, 4] and plan.offsets == [0, 1, 5] and plan.offsets_dev.tolist() == [0, 1, 5] and plan.total == 5
    assert torch.equal(plan.tgt_ids, torch.cat([t["labels"] for t in t1]))
    assert torch.equal(plan.tgt_boxes, torch.cat([t["boxes"] for t in t1]).double())
    with pytest.raises(ValueError, match="6 targets"):
        plan.update_(_targets([2, 4]))
    with pytest.raises(ValueError, match="3 images"):
        plan.update_(_targets([1, 2, 2]))
    assert plan.sizes == [1, 4]               # a refused update changes nothing


def test_late_status_raises_one_step_late():
    late = M.LateStatus()
    ok, bad = torch.zeros(7, 2, dtype=torch.int32), torch.zeros(7, 2, dtype=torch.int32)
    bad[3, 1] = 1
    late.push(ok)
    late.push(bad)                            # checks `ok`
    with pytest.raises(ValueError, match="output 3, image 1"):
        late.push(ok)                         # checks `bad`
    late.flush()
    late.push(bad)
    with pytest.raises(ValueError, match="invalid numeric entries"):
        late.flush()
    late.flush()                              # nothing pending


def test_supported_sizes():
    assert M.lsap_supported(900, 600) and M.lsap_supported(M.LSAP_MAX_DIM, M.LSAP_MAX_DIM)
    assert not M.lsap_supported(M.LSAP_MAX_DIM + 1, 10) and not M.lsap_supported(900, M.LSAP_MAX_DIM + 1)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """msda_lsap_*: sizes beyond the limits, null pointers and bad dimensions are refused before any launch (fake pointers, no GPU)"""
    import ctypes
    from richsem_amd import _lib
    L = _lib.load()
    n = ctypes.c_int64(-1)
    assert L.msda_lsap_workspace_bytes(7, 2, 900, 600, ctypes.byref(n)) == 0 and n.value == 0
    assert L.msda_lsap_workspace_bytes(7, 2, M.LSAP_MAX_DIM + 1, 10, ctypes.byref(n)) == -4
    assert L.msda_lsap_workspace_bytes(7, 2, 900, M.LSAP_MAX_DIM + 1, ctypes.byref(n)) == -4
    assert L.msda_lsap_workspace_bytes(0, 2, 900, 10, ctypes.byref(n)) == -2
    assert L.msda_lsap_workspace_bytes(7, 2, 900, 10, None) == -1
    p = 0x1000
    for fn in (L.msda_lsap_f32, L.msda_lsap_f64):
        assert fn(p, 0, p, 1, 1, M.LSAP_MAX_DIM + 1, 10, p, p, None, None) == -4
        assert fn(p, 1, p, 1, 1, 900, M.LSAP_MAX_DIM + 1, p, p, None, None) == -4
        assert fn(p, 0, None, 1, 1, 10, 10, p, p, None, None) == -1
        assert fn(p, 0, p, 1, 1, 10, 10, None, p, None, None) == -1
        assert fn(None, 0, p, 1, 1, 10, 10, p, p, None, None) == -1
        assert fn(p, 0, p, 1, 0, 10, 10, p, p, None, None) == -2
        assert fn(p, 0, p, 1, 1, -1, 10, p, p, None, None) == -2
    with pytest.raises(RuntimeError, match="MSDA_ERR_TOO_LARGE"):
        _lib.check(L.msda_lsap_f32(p, 0, p, 1, 1, M.LSAP_MAX_DIM + 1, 10, p, p, None, None))
