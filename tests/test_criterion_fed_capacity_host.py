"""Host side of the criterion over capacity buffers with the federated loss and class-agnostic two-stage targets: the fixture
tests/golden/criterion_fed_capacity_reference.npz against the numpy restatement of the appeared classes (tests/criterion_fed_capacity_ref.py),
the two new entry points in header / binding / library, their refusals before any launch, ``device_set_criterion`` without a CPU path, and
``TargetBuffers.class_agnostic`` on CPU buffers.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from criterion_fed_capacity_ref import FIXTURE, appeared_sets, case, fixture, n_chosen_of
from richsem_amd import _build, _lib
from richsem_amd.criterion import device_criterion, device_set_criterion
from richsem_amd.distill import distill_class_mask
from richsem_amd.fed_loss import FedClassSampler
from richsem_amd.matcher import TargetBuffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msda_criterion_pairs_ex_f32", "msda_fed_class_mask_slots_f32")


def test_fixture_against_the_numpy_restatement():
    z = fixture()
    nl, N, Q, C, Qi = (int(v) for v in z["dims"])
    assert (nl, N, Q, C, Qi) == (2, 3, 10, 70, 13) and int(z["num_sample_cats"]) == 50
    want_cases = [(c + (d, a)) for c in ((0, 5, 2), (1, 0, 0), (0, 0, 0)) for d in (3, 100) for a in (0, 1)]
    assert [tuple(int(v) for v in row) for row in z["cases"]] == want_cases
    w = z["class_weight"]
    assert w.shape == (C,) and w[0] == 0 and w[17] == 0 and int((w > 0).sum()) == C - 2
    assert os.path.getsize(FIXTURE) < (1 << 20)
    seen_zero_weight = False
    for ci, row in enumerate(z["cases"]):
        c = case(ci)
        counts, total = [int(v) for v in row[:3]], int(sum(row[:3]))
        pad, groups = int(c["pad_size"]), int(c["groups"])
        assert list(c["keys"]) == ["_0", "", "_dn_0", "_dn", "_interm"] and c["per_call"].shape == (2 * nl + 1, 3)
        want = float((c["per_call"] * z["weights"]).sum())
        assert abs(want - float(c["loss"])) <= 1e-12 * abs(want)
        cum = np.concatenate(([0], np.cumsum(counts)))
        meta = (max(counts), groups, pad, total, 0)
        mine = appeared_sets(cum, c["labels"], c["qot"].reshape(nl + 1, total), meta, nl, Q, Qi, C, max(total, 1), flags=c["agn"])
        for g in range(2 * nl + 1):
            made = not (nl <= g < 2 * nl and pad == 0)      # (the reference makes no denoising call for a batch without targets)
            rec = c["appeared"][g]
            rec = rec[rec >= 0]
            ids = c["fed_ids"][g]
            if not made:
                assert (ids == -1).all() and rec.size == 0 and mine[g].size == 0
                continue
            assert np.array_equal(mine[g], rec), (ci, g, mine[g], rec)
            assert len(ids) == 50 and len(set(ids.tolist())) == 50 and ids.min() >= 0 and ids.max() < C
            assert set(rec.tolist()) <= set(ids.tolist())
            assert n_chosen_of(rec, w, 50) == 50
            for zc in (0, 17):      # a zero-weight class is in the subset iff it appeared
                assert (zc in ids) == (zc in rec)
                seen_zero_weight |= zc in rec
        if c["agn"] and total:
            assert c["appeared"][2 * nl][:2].tolist() == [0, -1]
        for k in ("logits", "coords", "dn_logits", "dn_coords", "il", "ib"):
            assert c["grad_" + k].shape == c[k].shape and np.isfinite(c["grad_" + k]).all()
        # the logit gradient is 0 off the recorded subset, call by call
        off = lambda g: np.setdiff1d(np.arange(C), c["fed_ids"][g])
        for l in range(nl):
            assert not c["grad_logits"][l][..., off(l)].any()
            if pad:
                assert not c["grad_dn_logits"][l][..., off(nl + l)].any()
        assert not c["grad_il"][..., off(2 * nl)].any()
    assert seen_zero_weight


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert re.search(r"#define\s+RICHSEM_MSDA_ABI_VERSION\s+13\b", header)
    assert _lib.ABI_VERSION == 13
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.msda_abi_version() == 13
    raw = ctypes.CDLL(_build.LIB_PATH)
    for name in NEW:
        assert ctypes.cast(getattr(raw, name), ctypes.c_void_p).value, name
        assert getattr(lib, name).argtypes is not None


def test_entry_points_check_their_arguments_on_the_host():
    """refusals come before any launch: no GPU is needed to see them"""
    lib = _lib.load()
    p = 0x1000
    # cum, tgt_ids, query_of_target, dn_meta, class_weight, uniform, nl, N, Q, Qi, C, capacity, num_sample_cats, flags, mask, n_chosen, stream
    args = [p, p, p, None, p, p, 2, 3, 10, 13, 70, 16, 50, 0, p, p, None]
    for i in (0, 1, 2, 4, 5, 14, 15):
        bad = list(args)
        bad[i] = None
        assert lib.msda_fed_class_mask_slots_f32(*bad) == -1 and "msda_fed_class_mask_slots_f32" in _lib.last_error(), i
    for i, v in ((10, 0), (10, 4097), (7, 1025), (6, 0), (11, 0), (12, -1)):      # C, C, N, nl, capacity, num_sample_cats
        bad = list(args)
        bad[i] = v
        assert lib.msda_fed_class_mask_slots_f32(*bad) == -2, (i, v)
    for i, v in ((11, 1 << 24), (6, 1 << 20)):      # capacity, nl
        bad = list(args)
        bad[i] = v
        assert lib.msda_fed_class_mask_slots_f32(*bad) == -4, (i, v)
    bad = list(args)
    bad[13] = 2
    assert lib.msda_fed_class_mask_slots_f32(*bad) == -7
    bad = list(args)
    bad[2] = p + 4      # query_of_target: int64
    assert lib.msda_fed_class_mask_slots_f32(*bad) == -5
    # the pair entry with options: the checks of msda_criterion_pairs_f32, under its own name, plus the flags
    args = [p] * 8 + [None, None, 2, 3, 10, 13, 37, 16, 60, 0.25, 1.0, 5.0, 2.0, 1, p, p, p, p, p, p, p, None]
    bad = list(args)
    bad[0] = None
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -1 and "msda_criterion_pairs_ex_f32" in _lib.last_error()
    bad = list(args)
    bad[14] = 0      # C
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -2
    bad = list(args)
    bad[1] = p + 4      # coords: 16-byte rows
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -5
    bad = list(args)
    bad[24] = p + 2      # row_group: int32
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -5
    bad = list(args)
    bad[21] = 4      # flags
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -7
    bad = list(args)
    bad[28] = None      # workspace
    assert lib.msda_criterion_pairs_ex_f32(*bad) == -1
    # the old entry still names itself
    old = [p] * 8 + [None, None, 2, 3, 10, 13, 37, 16, 60, 0.25, 1.0, 5.0, 2.0] + [p] * 6 + [None]
    old[0] = None
    assert lib.msda_criterion_pairs_f32(*old) == -1 and _lib.last_error().startswith("msda_criterion_pairs_f32:")


def _targets(counts, first_label=0):
    out, at = [], first_label
    for tb in counts:
        out.append({"labels": torch.arange(at, at + tb), "boxes": torch.full((tb, 4), 0.25) + 0.01 * torch.arange(at, at + tb)[:, None]})
        at += tb
    return out


def test_device_set_criterion_has_no_cpu_path():
    bufs = TargetBuffers(2, 4, "cpu").update_(_targets([1, 2]))
    logits, coords, il, ib = torch.zeros(2, 2, 7, 5), torch.zeros(2, 2, 7, 4), torch.zeros(2, 3, 5), torch.zeros(2, 3, 4)
    qot = torch.zeros(3, 4, dtype=torch.int64)
    sampler = FedClassSampler(3, num_classes=5)
    for kw in ({}, {"fed": sampler}, {"enc_cls_agn": True}, {"fed": torch.ones(5, 5)}, {"fed": sampler, "enc_cls_agn": True}):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            device_set_criterion(logits, coords, il, ib, bufs, qot, None, pad_cap=2, **kw)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        sampler.sample_slots(bufs, qot, None, nl=2, Q=5, Qi=3)
    for k in ("fed_loss", "enc_cls_agn", "distill"):      # the pinned refusals of device_criterion stay
        with pytest.raises(NotImplementedError):
            device_criterion(logits, coords, il, ib, bufs, qot, None, pad_cap=2, **{k: True})
    with pytest.raises(NotImplementedError, match="device_set_criterion"):
        device_criterion(logits, coords, il, ib, bufs, qot, None, pad_cap=2, fed_loss=True)


def test_class_agnostic_targets_share_storage_and_follow_update():
    bufs = TargetBuffers(3, 8, "cpu", max_per_image=5).update_(_targets([0, 5, 2], first_label=3))
    agn = bufs.class_agnostic()
    assert agn.offsets_dev is bufs.offsets_dev and agn.tgt_boxes is bufs.tgt_boxes
    assert agn.tgt_ids.data_ptr() != bufs.tgt_ids.data_ptr() and agn.tgt_ids.dtype == torch.int64 and agn.tgt_ids.tolist() == [0] * 8
    assert agn.total == agn.capacity == 8 and agn.sizes == [0, 5, 2] and agn.offsets == [0, 0, 5, 7] and agn.live == 7
    bufs.update_(_targets([1, 0, 0], first_label=9))
    assert agn.sizes == [1, 0, 0] and agn.offsets == [0, 1, 1, 1] and agn.live == 1 and agn.offsets_dev.tolist() == [0, 1, 1, 1]
    assert bufs.tgt_ids.tolist() == [9] + [0] * 7 and agn.tgt_ids.tolist() == [0] * 8
    assert torch.equal(agn.tgt_boxes, bufs.tgt_boxes)
    assert agn.update_(_targets([2, 2, 2], first_label=4)) is agn      # through the view: the labels go to the parent only
    assert bufs.sizes == [2, 2, 2] and bufs.tgt_ids[:6].tolist() == [4, 5, 6, 7, 8, 9] and agn.tgt_ids.tolist() == [0] * 8
    with pytest.raises(ValueError):
        agn.update_(_targets([6, 0, 0]))


def test_distill_class_mask_selects_the_calls_of_the_distilled_layers():
    nl, C = 4, 6
    mask = torch.arange((2 * nl + 1) * C, dtype=torch.float32).reshape(2 * nl + 1, C)
    got = distill_class_mask(mask, [3, 1], nl)
    assert torch.equal(got, mask[[1, 3, nl + 1, nl + 3]])
    assert torch.equal(distill_class_mask(mask, range(nl), nl), mask[: 2 * nl])
    with pytest.raises(ValueError):
        distill_class_mask(mask, [4], nl)
    with pytest.raises(ValueError):
        distill_class_mask(mask[:-1], [0], nl)
