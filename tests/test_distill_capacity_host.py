"""Host side of the distillation term over capacity buffers: the new entry points in header / binding / library and their refusals, the
refusals of ``roi_align_targets`` / ``clip_box_targets_capacity`` / ``device_distill``, and the self-consistency of
tests/golden/criterion_distill_capacity_reference.npz -- the pairs the fixture's gradients sit on are the ones the numpy restatement of
``msda_distill_pairs`` names (tests/distill_capacity_ref.py), and the float64 restatement of the row formulas (tests/test_distill_host.py) on
those pairs gives the reference's losses and gradients.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from distill_capacity_ref import CASES, LAYER_SETS, calls_of, checksums, config, fixture, pairs_numpy
from richsem_amd import _build, _lib
from richsem_amd.distill import device_distill, device_distill_and_grads
from richsem_amd.matcher import TargetBuffers
from richsem_amd.modules.attnpool import clip_box_targets_capacity
from richsem_amd.roi import roi_align_targets
from test_distill_host import restate_kl, restate_l1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msda_roi_align_targets_f32", "msda_distill_pairs", "msda_distill_scatter_f32", "msda_distill_scatter_bf16")


def test_new_entry_points_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert re.search(r"#define\s+RICHSEM_MSDA_ABI_VERSION\s+13\b", header)
    assert _lib.ABI_VERSION == 13
    assert "distill_api.hip" in _build.SOURCES and "rows_api.hip" in _build.SOURCES
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
    p = 0x1000
    # input, cum, tgt_boxes, sizes, N, C, H, W, capacity, ph, pw, scale, sampling_ratio, output, status, stream
    roi = [p, p, p, p, 3, 5, 7, 11, 16, 7, 7, 1.0 / 32, 0, p, p, None]
    for i in (0, 1, 2, 3, 13, 14):
        bad = list(roi)
        bad[i] = None
        assert lib.msda_roi_align_targets_f32(*bad) == -1 and "msda_roi_align_targets_f32" in _lib.last_error()
    for i in (4, 5, 6, 7, 8, 9, 10):
        bad = list(roi)
        bad[i] = 0
        assert lib.msda_roi_align_targets_f32(*bad) == -2, i
    bad = list(roi)
    bad[4] = 1025      # N > 1024: cum is kept in LDS
    assert lib.msda_roi_align_targets_f32(*bad) == -2
    bad = list(roi)
    bad[8] = 1 << 24
    assert lib.msda_roi_align_targets_f32(*bad) == -4
    bad = list(roi)
    bad[2] = p + 8      # tgt_boxes: 16-byte rows
    assert lib.msda_roi_align_targets_f32(*bad) == -5
    bad = list(roi)
    bad[1] = p + 4      # cum: int64
    assert lib.msda_roi_align_targets_f32(*bad) == -5
    # cum, qot, meta, num_boxes, nl, N, Q, pad_cap, capacity, layer_mask, objective, pred_row, tgt_row, weight, group, status, stream
    pairs = [p, p, None, None, 2, 3, 10, 60, 16, 0b10, 0, p, p, p, p, p, None]
    for i in (0, 1, 11, 12, 13, 14, 15):
        bad = list(pairs)
        bad[i] = None
        assert lib.msda_distill_pairs(*bad) == -1 and "msda_distill_pairs" in _lib.last_error()
    for i, v in ((4, 0), (5, 0), (6, 0), (7, -1), (8, 0), (9, 0), (9, 0b100), (5, 1025)):      # (a layer outside 0..nl-1; N > 1024)
        bad = list(pairs)
        bad[i] = v
        assert lib.msda_distill_pairs(*bad) == -2, (i, v)
    bad = list(pairs)
    bad[10] = 2      # 'pred_all' has no slot space
    assert lib.msda_distill_pairs(*bad) == -7
    bad = list(pairs)
    bad[8] = 1 << 24
    assert lib.msda_distill_pairs(*bad) == -4
    bad = list(pairs)
    bad[11] = p + 4
    assert lib.msda_distill_pairs(*bad) == -5
    # grad_rows, pred_row, cum, gscale, n_d, N, Q, pad_cap, capacity, C, grad_pred, stream
    scat = [p, p, p, p, 2, 3, 10, 60, 16, 301, p, None]
    for name in ("msda_distill_scatter_f32", "msda_distill_scatter_bf16"):
        fn = getattr(lib, name)
        for i in (0, 1, 2, 3, 10):
            bad = list(scat)
            bad[i] = None
            assert fn(*bad) == -1 and name in _lib.last_error()
        for i in (4, 5, 6, 8, 9):
            bad = list(scat)
            bad[i] = 0
            assert fn(*bad) == -2, (name, i)
        bad = list(scat)
        bad[8] = 1 << 24
        assert fn(*bad) == -4
        bad = list(scat)
        bad[1] = p + 4
        assert fn(*bad) == -5
    bad = list(scat)
    bad[10] = p + 2      # a float32 gradient on a 2-byte boundary (fine for bf16)
    assert lib.msda_distill_scatter_f32(*bad) == -5


def _cpu_case(dtype=torch.float32):
    bufs = TargetBuffers(3, 16, "cpu")
    pred, teacher = torch.zeros(1, 3, 70, 301, dtype=dtype), torch.zeros(16, 301)
    qot = torch.zeros(3, 16, dtype=torch.int64)
    return pred, teacher, bufs, qot


def test_python_entry_points_refuse_before_any_launch():
    pred, teacher, bufs, qot = _cpu_case()
    kw = dict(pad_cap=60, layers=(1,), distill_type="clip_logits", objective="gt")
    for fn in (device_distill, device_distill_and_grads):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn(pred, teacher, bufs, qot, None, **kw)
        with pytest.raises(ValueError, match="DistillLoss"):
            fn(pred, teacher, bufs, qot, None, **dict(kw, objective="pred_all"))
        with pytest.raises(TypeError):
            fn(pred.double(), teacher, bufs, qot, None, **kw)
        with pytest.raises(TypeError):      # the L1 form takes no bf16 student
            fn(pred.bfloat16(), teacher, bufs, qot, None, **dict(kw, distill_type="clip_l1"))
        with pytest.raises(TypeError):
            fn(pred, teacher, bufs, qot.int(), None, **kw)
        with pytest.raises(NotImplementedError):
            fn(pred, teacher, bufs, qot, None, **dict(kw, distill_type="clip_cosine"))
    feat, sizes = torch.zeros(3, 5, 7, 11), torch.tensor([[200, 300]] * 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        roi_align_targets(feat, bufs, sizes, 7, 1.0 / 32)
    with pytest.raises(TypeError):
        roi_align_targets(feat.double(), bufs, sizes, 7, 1.0 / 32)
    with pytest.raises(TypeError):
        roi_align_targets(feat, bufs, sizes.long(), 7, 1.0 / 32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        clip_box_targets_capacity(feat, bufs, sizes, None, torch.zeros(4, 8), 0.0)


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
def restated(c, case, layers, pad_cap=None, cap=None, weights64=True):
    """config ``c``, case and layer set -> the float64 restatement on the pairs ``pairs_numpy`` names, in the capacity layout (``pad_cap``
    denoising rows, ``cap`` target slots; default: the batch's own sizes): dict with pred (n_d, N, pad_cap + Q, .) float64 (zeros in the rows
    past pad_size), teacher, pairs (pred_row, tgt_row, weight, group, status), live (K) bool, loss, per_call (2 n_d), grad (rows, .) float64, and
    the restatement's own dict ``r`` over the live slots"""
    nl, N, Q, pad = c["nl"], c["N"], c["Q"], c["pad"]
    pad_cap = pad if pad_cap is None else pad_cap
    cap = max(c["total"], 1) if cap is None else cap
    kind, objective = case.split("_")[0], case.split("_")[1]
    src = c[kind][list(layers)]
    n_d, ch = len(layers), src.shape[-1]
    pred = np.zeros((n_d, N, pad_cap + Q, ch))
    pred[:, :, :pad], pred[:, :, pad_cap:] = src[:, :, :pad], src[:, :, pad:]
    cum = np.concatenate(([0], np.cumsum(c["counts"])))
    qot = np.full((nl + 1, cap), -1, dtype=np.int64)
    qot[:, :c["total"]] = c["qot"]
    meta = [max(c["counts"]), c["groups"], pad, c["total"], 0]
    pr, tr, w, grp, status = pairs_numpy(cum, qot, meta, None, nl, N, Q, pad_cap, cap, layers, objective)
    if objective == "gt":
        teacher = np.zeros((cap, ch))
        teacher[:c["total"]] = c["teacher_gt"] if kind == "kl" else c["prompt_gt"]
    else:      # the student's tensor with the two layers swapped
        other = c[kind][::-1][list(layers)]
        teacher = np.zeros_like(pred)
        teacher[:, :, :pad], teacher[:, :, pad_cap:] = other[:, :, :pad], other[:, :, pad:]
    live = pr >= 0
    nb = float(c["num_boxes"])
    w64 = np.where(grp < n_d, 1.0 / nb, 1.0 / (nb * c["groups"]))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = (t(pred.reshape(-1, ch)), t(teacher.reshape(-1, ch)), t(pr[live]), t(tr[live]), t(w64[live] if weights64 else w[live].astype(np.float64)))
    mask = None
    if kind == "kl":
        subset = None
        if case.endswith("fed"):
            mask = c[case + ".masks"][calls_of(layers, nl)]
            subset = t(mask[grp[live]] != 0)
        r = restate_kl(*args, subset=subset, dynamic=case.endswith("dyn1"))
    else:
        r = restate_l1(*args, normalize_target=False)
    grad = np.zeros((n_d * N * (pad_cap + Q), ch))
    grad[pr[live]] = r["grad_rows"].numpy()
    per_call = np.zeros(2 * n_d)
    np.add.at(per_call, grp[live], r["row_loss"].numpy())
    return {"pred": pred, "teacher": teacher, "pairs": (pr, tr, w, grp, status), "live": live, "loss": float(r["loss"]), "per_call": per_call,
            "grad": grad, "r": r, "mask": mask}


def test_fixture_is_self_consistent():
    z = fixture()
    assert [int(v) for v in z["dims"]] == [2, 3, 10, 301, 130]
    assert [tuple(int(v) for v in row) for row in z["cfgs"]] == [(0, 5, 2, 3), (0, 5, 2, 100), (1, 0, 0, 3), (1, 0, 0, 100), (0, 0, 0, 3), (0, 0, 0, 100)]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "criterion_distill_capacity_reference.npz")) < (1 << 20)
    from richsem_amd.dn import dn_group_count
    for ci in range(6):
        c = config(ci)
        nl, N, Q, pad, counts, total = c["nl"], c["N"], c["Q"], c["pad"], c["counts"], c["total"]
        assert c["groups"] == dn_group_count(c["dn_number"], counts) and pad == 2 * max(counts) * c["groups"] and float(c["num_boxes"]) == max(total, 1)
        assert c["qot"].shape == (nl + 1, total)
        at = 0
        for tb in counts:      # one-to-one: every target matched once per output, to distinct queries of its image
            for o in range(nl + 1):
                q = c["qot"][o, at: at + tb]
                assert len(set(q.tolist())) == tb and (q >= 0).all() and (q < Q).all()
            at += tb
        for v in (c["kl"], c["teacher_gt"]):      # the generator's conditions hold for what expand() returns here
            if v.size:
                assert float((v.max(-1) - v.min(-1)).max()) <= 80.0
        for case in CASES:
            per_call, sums, sel, grad_sel = c[case + ".per_call"], c[case + ".grad_sums"], c["sel_rows"], c[case + ".grad_sel"]
            ch = c["C"] if case.startswith("kl") else c["D"]
            assert per_call.shape == (2 * nl,) and sums.shape == (nl * N * (pad + Q), 3) and grad_sel.shape == (len(sel), ch)
            full = restated(c, case, (0, 1))
            live_rows = np.zeros(sums.shape[0], dtype=bool)
            live_rows[full["pairs"][0][full["live"]]] = True
            assert len(set(full["pairs"][0][full["live"]].tolist())) == int(full["live"].sum())      # no student row is named twice
            assert not sums[~live_rows].any() and (sums[live_rows, 1] > 0).all()      # gradient rows: zero outside the live pairs, and only there
            if total == 0:
                assert not per_call.any() and not sums.any()      # an empty batch: loss 0
            if pad == 0:
                assert not per_call[nl:].any()
            assert set(sel.tolist()) <= set(np.nonzero(live_rows)[0].tolist())
            # the float64 restatement on the restated pairs IS the reference's result, for both layer sets
            for layers in LAYER_SETS:
                got = full if layers == (0, 1) else restated(c, case, layers)
                calls = calls_of(layers, nl)
                want = per_call[calls]
                assert np.all(np.abs(got["per_call"] - want) <= 1e-11 * np.abs(want)), (ci, case, layers, got["per_call"], want)
                first = 0 if layers == (0, 1) else N * (pad + Q)      # the rows of layer 1 in the stored gradient
                want_sums = sums[first:]
                err = np.abs(checksums(got["grad"]) - want_sums)
                assert np.all(err <= 1e-11 * np.maximum(want_sums[:, 1:2], 1e-300)), (ci, case, layers, float(err.max()))
                keep = sel >= first
                err = np.abs(got["grad"][sel[keep] - first] - grad_sel[keep].astype(np.float64))
                assert np.all(err <= 2.0 ** -23 * np.abs(grad_sel[keep]) + 1e-300), (ci, case, layers)
