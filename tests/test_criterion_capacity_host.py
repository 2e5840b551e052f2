"""Host side of the criterion over capacity buffers: ``TargetBuffers`` bookkeeping, argument refusals of ``device_criterion``, the new
entry points in header / binding / library, and the self-consistency of tests/golden/criterion_capacity_reference.npz.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from richsem_amd import _build, _lib
from richsem_amd.criterion import STATUS, device_criterion
from richsem_amd.matcher import TargetBuffers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msda_criterion_workspace_bytes", "msda_criterion_pairs_f32", "msda_criterion_pairs_backward_f32")


def _targets(counts, first_label=0):
    out, at = [], first_label
    for tb in counts:
        out.append({"labels": torch.arange(at, at + tb), "boxes": torch.full((tb, 4), 0.25) + 0.01 * torch.arange(at, at + tb)[:, None]})
        at += tb
    return out


def test_target_buffers_write_offsets_and_leave_the_tail_at_its_filler():
    bufs = TargetBuffers(3, 8, "cpu", max_per_image=5)
    assert bufs.total == bufs.capacity == 8 and bufs.offsets_dev.tolist() == [0, 0, 0, 0]
    assert bufs.tgt_ids.dtype == torch.int64 and tuple(bufs.tgt_boxes.shape) == (8, 4) and bufs.offsets_dev.dtype == torch.int64
    assert bufs.update_(_targets([0, 5, 2])) is bufs
    assert bufs.offsets_dev.tolist() == [0, 0, 5, 7] and bufs.offsets == [0, 0, 5, 7] and bufs.sizes == [0, 5, 2] and bufs.live == 7
    assert bufs.tgt_ids.tolist() == [0, 1, 2, 3, 4, 5, 6, 0] and bufs.tgt_boxes[7].tolist() == [0.5, 0.5, 1.0, 1.0]
    assert torch.equal(bufs.tgt_boxes[:7], torch.cat([t["boxes"] for t in _targets([0, 5, 2])]))
    bufs.update_(_targets([1, 0, 0], first_label=9))      # a smaller batch: the rows it no longer uses go back to the filler
    assert bufs.offsets_dev.tolist() == [0, 1, 1, 1] and bufs.tgt_ids.tolist() == [9] + [0] * 7
    assert bufs.tgt_boxes[1:].tolist() == [[0.5, 0.5, 1.0, 1.0]] * 7
    bufs.update_(_targets([0, 0, 0]))
    assert bufs.offsets_dev.tolist() == [0, 0, 0, 0] and bufs.live == 0
    bufs.update_(_targets([3, 5, 0]))      # exactly full
    assert bufs.offsets_dev.tolist() == [0, 3, 8, 8]


def test_target_buffers_refuse_what_does_not_fit():
    bufs = TargetBuffers(3, 8, "cpu", max_per_image=5).update_(_targets([1, 2, 3]))
    before = (bufs.offsets_dev.clone(), bufs.tgt_ids.clone(), bufs.tgt_boxes.clone())
    with pytest.raises(ValueError, match="images"):
        bufs.update_(_targets([1, 2]))
    with pytest.raises(ValueError, match="capacity"):
        bufs.update_(_targets([4, 4, 1]))
    with pytest.raises(ValueError, match="at most 5"):
        bufs.update_(_targets([6, 0, 0]))
    for a, b in zip(before, (bufs.offsets_dev, bufs.tgt_ids, bufs.tgt_boxes)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError):
        TargetBuffers(0, 8, "cpu")
    with pytest.raises(ValueError):
        TargetBuffers(2, 0, "cpu")


def test_device_criterion_has_no_cpu_path():
    bufs = TargetBuffers(2, 4, "cpu").update_(_targets([1, 2]))
    logits, coords, il, ib = torch.zeros(2, 2, 7, 5), torch.zeros(2, 2, 7, 4), torch.zeros(2, 3, 5), torch.zeros(2, 3, 4)
    qot = torch.zeros(3, 4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        device_criterion(logits, coords, il, ib, bufs, qot, None, pad_cap=2)
    for k in ("fed_loss", "enc_cls_agn", "distill"):      # what is out of scope says so, whatever the tensors
        with pytest.raises(NotImplementedError):
            device_criterion(logits, coords, il, ib, bufs, qot, None, pad_cap=2, **{k: True})
    assert len(STATUS) == 4


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert re.search(r"#define\s+RICHSEM_MSDA_ABI_VERSION\s+13\b", header)
    assert _lib.ABI_VERSION == 13
    for name in NEW:
        assert re.search(r"^int " + name + r"\(", header, re.M), name
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.msda_abi_version() == 13
    raw = ctypes.CDLL(_build.LIB_PATH)      # (a handle without the binding table: a symbol it resolves is one the library exports)
    for name in NEW:
        assert ctypes.cast(getattr(raw, name), ctypes.c_void_p).value, name
        assert getattr(lib, name).argtypes is not None


def test_entry_points_check_their_arguments_on_the_host():
    """refusals come before any launch: no GPU is needed to see them"""
    lib = _lib.load()
    n = ctypes.c_int64(0)
    assert lib.msda_criterion_workspace_bytes(2, 3, 10, 13, 16, 60, ctypes.byref(n)) == 0
    # 48 matched slots + 360 denoising slots of 28 bytes, 5 workgroups of partials and status words, rounded up to 16
    slots, groups = 3 * 16 + 2 * 3 * 60, 3 * 1 + 2 * 1
    assert n.value == (slots * 28 + groups * (24 + 16) + 15) // 16 * 16
    assert lib.msda_criterion_workspace_bytes(2, 3, 10, 13, 16, 60, None) == -1
    assert lib.msda_criterion_workspace_bytes(0, 3, 10, 13, 16, 60, ctypes.byref(n)) == -2
    assert lib.msda_criterion_workspace_bytes(2, 2000, 10, 13, 16, 60, ctypes.byref(n)) == -2      # N > 1024: cum is kept in LDS
    assert lib.msda_criterion_workspace_bytes(2, 3, 10, 13, 1 << 24, 60, ctypes.byref(n)) == -4
    p = 0x1000
    args = [p] * 8 + [None, None, 2, 3, 10, 13, 37, 16, 60, 0.25, 1.0, 5.0, 2.0] + [p] * 6 + [None]
    bad = list(args)
    bad[0] = None
    assert lib.msda_criterion_pairs_f32(*bad) == -1 and "msda_criterion_pairs_f32" in _lib.last_error()
    bad = list(args)
    bad[14] = 0      # C
    assert lib.msda_criterion_pairs_f32(*bad) == -2
    bad = list(args)
    bad[1] = p + 4      # coords: 16-byte rows
    assert lib.msda_criterion_pairs_f32(*bad) == -5
    back = [p, p, p, 2, 3, 10, 13, 37, 16, 60, p, p, p, p, None]
    bad = list(back)
    bad[2] = None
    assert lib.msda_criterion_pairs_backward_f32(*bad) == -1 and "msda_criterion_pairs_backward_f32" in _lib.last_error()
    bad = list(back)
    bad[12] = p + 8
    assert lib.msda_criterion_pairs_backward_f32(*bad) == -5


def test_fixture_is_self_consistent():
    z = np.load(os.path.join(ROOT, "tests", "golden", "criterion_capacity_reference.npz"))
    nl, N, Q, C, Qi = (int(v) for v in z["dims"])
    assert (nl, N, Q, C, Qi) == (2, 3, 10, 37, 13)
    assert [tuple(int(v) for v in row) for row in z["cases"]] == [(0, 5, 2, 3), (0, 5, 2, 100), (1, 0, 0, 3), (1, 0, 0, 100), (0, 0, 0, 3), (0, 0, 0, 100)]
    from richsem_amd.dn import dn_group_count
    for ci, row in enumerate(z["cases"]):
        p = f"c{ci}."
        counts, dn_number = [int(v) for v in row[:3]], int(row[3])
        total = sum(counts)
        per_call = z[p + "per_call"]
        assert per_call.shape == (2 * nl + 1, 3) and len(z[p + "keys"]) == 2 * nl + 1
        assert list(z[p + "keys"]) == ["_0", "", "_dn_0", "_dn", "_interm"]
        want = float((per_call * z["weights"]).sum())
        assert abs(want - float(z[p + "loss"])) <= 1e-12 * abs(want)
        groups = dn_group_count(dn_number, counts)
        assert int(z[p + "groups"]) == groups and int(z[p + "pad_size"]) == 2 * max(counts) * groups
        assert float(z[p + "num_boxes"]) == max(total, 1)
        pad = int(z[p + "pad_size"])
        assert z[p + "logits"].shape == (nl, N, Q, C) and z[p + "dn_logits"].shape == (nl, N, pad, C) and z[p + "il"].shape == (N, Qi, C)
        assert z[p + "qot"].shape == (nl + 1, total) and z[p + "labels"].shape == (total,) and z[p + "boxes"].shape == (total, 4)
        qot = z[p + "qot"]
        at = 0
        for tb in counts:      # every target matched once per output, to distinct queries of its image
            for o in range(nl + 1):
                q = qot[o, at: at + tb]
                assert len(set(q.tolist())) == tb and (q >= 0).all() and (q < (Qi if o == nl else Q)).all()
            at += tb
        for k in ("logits", "coords", "dn_logits", "dn_coords", "il", "ib"):
            assert z[p + "grad_" + k].shape == z[p + k].shape and np.isfinite(z[p + "grad_" + k]).all()
        # no prediction box equals a target box (the subgradient at the kink would be the implementation's own)
        for k in ("coords", "dn_coords", "ib"):
            flat = z[p + k].reshape(-1, 4)
            assert not any((flat == b).all(1).any() for b in z[p + "boxes"])
        if pad == 0:
            assert not per_call[nl: 2 * nl].any()
        # box gradients live only where a pair points: rows of images without targets get none
        for b, tb in enumerate(counts):
            if tb == 0:
                assert not z[p + "grad_coords"][:, b].any() and not z[p + "grad_ib"][b].any() and not z[p + "grad_dn_coords"][:, b].any()
