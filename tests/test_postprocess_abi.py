"""CPU: the PostProcess entry points (ABI v11: ``msda_postprocess_workspace_bytes``, ``msda_postprocess_select``, ``msda_nms_f32``) are
declared, bound and exported and refuse bad arguments on the host; the committed fixture of the reference's ``PostProcess`` loads and
agrees with the plain-torch restatement the GPU tests compare against (tests/postprocess_ref.py).  No kernel is launched here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from richsem_amd import _build, _lib

import postprocess_ref as R
from conftest import ROOT

NAMES = ("msda_postprocess_workspace_bytes", "msda_postprocess_select", "msda_nms_f32")
FIXTURE = os.path.join(ROOT, "tests", "golden", "postprocess", "postprocess_reference.npz")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    for name in NAMES:
        assert name + "(" in header
        assert name in _lib.SYMBOLS
        assert f" T {name}\n" in exported
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int
    assert _lib.ABI_VERSION >= 11 and lib.msda_abi_version() == _lib.ABI_VERSION


def test_package_exports_the_module():
    import richsem_amd
    from richsem_amd import postprocess
    assert richsem_amd.PostProcess is postprocess.PostProcess
    pp = richsem_amd.PostProcess()
    assert (pp.num_select, pp.nms_iou_threshold, pp.use_opt) == (100, -1, False)
    out = {"pred_logits": torch.zeros(1, 4, 5), "pred_boxes": torch.rand(1, 4, 4)}
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        pp(out, torch.tensor([[480, 640]]))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        pp.select(out["pred_logits"], out["pred_boxes"], torch.tensor([[480, 640]]))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        pp.nms_padded(torch.rand(1, 4, 4))
    with pytest.raises(AssertionError):
        pp(out, torch.tensor([[480, 640], [1, 1]]))               # one size per image
    with pytest.raises(AssertionError):
        pp(out, torch.tensor([[480, 640, 3]]))


def _select(lib, logits=0x1000, boxes=0x1000, sizes=0x1000, B=2, Q=900, C=1203, k=300, mode=1, outs=(0x1000,) * 4, ws=0x1000, bf16=0):
    return lib.msda_postprocess_select(logits, bf16, boxes, sizes, B, Q, C, k, mode, outs[0], outs[1], outs[2], outs[3], ws, None)


def test_select_refuses_bad_arguments_on_the_host(lib):
    """fake pointers: every refusal comes before any launch"""
    p = 0x1000
    for kw in ({"logits": None}, {"boxes": None}, {"sizes": None}, {"ws": None}, {"outs": (None, p, p, p)}, {"outs": (p, None, p, p)},
               {"outs": (p, p, None, p)}, {"outs": (p, p, p, None)}):
        assert _select(lib, **kw) == -1, kw
    assert "msda_postprocess_select: null pointer" in _lib.last_error()
    for kw in ({"k": 0}, {"k": 1025}, {"k": 21, "Q": 4, "C": 5}, {"B": 0}, {"Q": 0}, {"C": 0}, {"mode": 3}, {"mode": -1}):
        assert _select(lib, **kw) == -2, kw
    with pytest.raises(RuntimeError, match="msda_postprocess_select.*dimension"):
        _lib.check(_select(lib, k=1025))
    assert _select(lib, Q=1 << 16, C=1 << 15) == -4                       # Q * C = 2^31
    with pytest.raises(RuntimeError, match="msda_postprocess_select.*too large.*MSDA_ERR_TOO_LARGE"):
        _lib.check(_select(lib, Q=1 << 16, C=1 << 15))
    for bf16 in (0, 1):
        for kw in ({"logits": p + 4}, {"logits": p + 2}, {"boxes": p + 4}, {"outs": (p, p, p + 8, p)}, {"ws": p + 4}):
            assert _select(lib, bf16=bf16, **kw) == -5, kw
    with pytest.raises(RuntimeError, match="msda_postprocess_select.*align.*MSDA_ERR_MISALIGNED"):
        _lib.check(_select(lib, logits=p + 4))


def test_nms_refuses_bad_arguments_on_the_host(lib):
    p = 0x1000
    assert lib.msda_nms_f32(None, None, 1, 10, 0.5, p, p, p, None) == -1
    assert lib.msda_nms_f32(p, None, 1, 10, 0.5, None, p, p, None) == -1
    assert lib.msda_nms_f32(p, None, 1, 10, 0.5, p, None, p, None) == -1
    assert lib.msda_nms_f32(p, None, 1, 10, 0.5, p, p, None, None) == -1
    assert "msda_nms_f32: null pointer" in _lib.last_error()
    assert lib.msda_nms_f32(p, p, 1, 1025, 0.5, p, p, p, None) == -2
    assert lib.msda_nms_f32(p, p, 1, 0, 0.5, p, p, p, None) == -2
    assert lib.msda_nms_f32(p, p, 0, 10, 0.5, p, p, p, None) == -2
    with pytest.raises(RuntimeError, match="msda_nms_f32.*dimension"):
        _lib.check(lib.msda_nms_f32(p, p, 1, 1025, 0.5, p, p, p, None))
    assert lib.msda_nms_f32(p + 4, p, 1, 10, 0.5, p, p, p, None) == -5


def test_workspace_bytes(lib):
    n = ctypes.c_int64(-1)
    prev = 0
    for B in (1, 2, 3, 7, 64):
        assert lib.msda_postprocess_workspace_bytes(B, 900, 1203, 300, ctypes.byref(n)) == 0
        assert n.value > 0 and n.value % 16 == 0 and n.value > prev
        prev = n.value
    assert lib.msda_postprocess_workspace_bytes(1, 1, 1, 1, ctypes.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert lib.msda_postprocess_workspace_bytes(2, 900, 1203, 300, None) == -1
    assert lib.msda_postprocess_workspace_bytes(2, 900, 1203, 0, ctypes.byref(n)) == -2
    assert lib.msda_postprocess_workspace_bytes(2, 900, 1203, 1025, ctypes.byref(n)) == -2
    assert lib.msda_postprocess_workspace_bytes(2, 4, 5, 21, ctypes.byref(n)) == -2
    assert lib.msda_postprocess_workspace_bytes(2, 1 << 16, 1 << 15, 300, ctypes.byref(n)) == -4
    assert "msda_postprocess_workspace_bytes: " in _lib.last_error()


def fixture_cases():
    """[(name, constructor kwargs, forward kwargs, with masks)] and the arrays of the committed fixture"""
    z = np.load(FIXTURE)
    cases = []
    for name, row in zip(z["case_names"], z["case_table"]):
        num_select, thr, use_opt, not_to_xyxy, test, with_masks = row
        cases.append((str(name), {"num_select": int(num_select), "nms_iou_threshold": float(thr), "use_opt": bool(use_opt)},
                      {"not_to_xyxy": bool(not_to_xyxy), "test": bool(test)}, bool(with_masks)))
    return cases, z


def test_fixture_is_self_consistent():
    cases, z = fixture_cases()
    assert [c[0] for c in cases] == ["plain", "not_to_xyxy", "test", "nms05", "nms07", "use_opt", "masks"]
    logits, boxes, sizes = (torch.from_numpy(z[k]) for k in ("logits", "boxes", "sizes"))
    B, Q, C = logits.shape
    assert (B, Q, C) == (2, 30, 57) and boxes.shape == (B, Q, 4) and not torch.equal(sizes[0], sizes[1])
    for b in range(B):      # the logits: a permutation of linspace(-8, 6, Q * C)
        assert torch.equal(logits[b].flatten().sort()[0], torch.linspace(-8, 6, Q * C))
    for name, ctor, fwd, with_masks in cases:
        k = ctor["num_select"]
        results, query_idx, items = R.postprocess(logits, boxes, sizes, k, ctor["nms_iou_threshold"], ctor["use_opt"], **fwd)
        assert np.array_equal(query_idx.numpy(), z["query_idx"])
        for b, r in enumerate(results):
            assert np.array_equal(r["labels"].numpy(), z[f"{name}.labels.{b}"]), name
            assert np.array_equal(r["boxes"].numpy(), z[f"{name}.boxes.{b}"]), name            # the same float32 operations: bit-equal
            assert np.array_equal(r["scores"].numpy(), z[f"{name}.scores.{b}"]), name
            if items is not None:
                assert np.array_equal(items[b].numpy(), z[f"{name}.item_indices.{b}"]), name
                assert 0 < len(items[b]) < k
            else:
                assert len(r["scores"]) == k
        if with_masks:
            masks = torch.from_numpy(z["masks"])
            want = torch.gather(masks, 1, query_idx.view(B, k, 1, 1, 1).expand(-1, -1, -1, *masks.shape[-2:]))
            assert np.array_equal(want.numpy(), z[f"{name}.pred_masks"])
    # what makes it decidable: top k + 1 probabilities >= 2e-5 apart and ordered as the logits; no IoU within 1e-5 of a threshold in use
    flat = logits.view(B, -1)
    pv, pi = torch.topk(flat.sigmoid(), 101, dim=1)
    assert float((pv[:, :-1] - pv[:, 1:]).min()) >= 2e-5 and torch.equal(pi, torch.topk(flat, 101, dim=1)[1])
    assert np.array_equal(R.stable_topk(flat.numpy(), 100) // C, z["query_idx"])
    for b in range(B):
        assert R.iou_margin(torch.from_numpy(z[f"plain.boxes.{b}"]), (0.5, 0.7)) > 1e-5
