"""No GPU: the host side of the class-head entry points (msda_cls_head_*, csrc/cls_head_mfma.hip).  Every argument check comes before any
launch -- the pointers below are fake and never dereferenced --, a refusal leaves "<entry point>: <class of error>" behind
msda_last_error(), and the Python layer marshals each entry point in exactly one place ("The Python host layer")."""
import ctypes
import glob
import os
import re

import pytest

from richsem_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL_POINTER, BAD_DIMS, MISALIGNED = -1, -2, -5
P = 0x10000      # a 16-byte aligned fake device pointer


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def _calls(lib):
    """entry point -> (function of a dict of overrides, the names of its pointer arguments, those that must be 16-byte aligned)"""
    n = ctypes.c_int64(0)

    def forward(a):
        return lib.msda_cls_head_forward(a["x"], a["bf16"], a["packed"], a["tokens"], a["d"], a["classes"], 14.0, a["parts"], a["logits"], a["n2"], None)

    def rows(a):
        return lib.msda_cls_head_backward_rows(a["g"], a["logits"], a["n2"], a["x"], a["bf16"], a["packed"], a["tokens"], a["d"], a["classes"], 14.0,
                                               a["parts"], a["dx"], a["beta"], None)

    def weights(a):
        return lib.msda_cls_head_backward_weights(a["g"], a["n2"], a["beta"], a["x"], a["bf16"], a["tokens"], a["d"], a["classes"], 14.0, a["parts"],
                                                  a["workspace"], a["dGA"], None)

    def pack(a):
        return lib.msda_cls_head_pack(a["G"], a["classes"], a["A"], a["d"], a["packed"], None)

    return {
        "msda_cls_head_forward": (forward, ("x", "packed", "logits", "n2"), ("x", "packed")),
        "msda_cls_head_backward_rows": (rows, ("g", "logits", "n2", "x", "packed", "dx", "beta"), ("x", "packed", "dx")),
        "msda_cls_head_backward_weights": (weights, ("g", "n2", "beta", "x", "workspace", "dGA"), ("x", "workspace", "dGA")),
        "msda_cls_head_pack": (pack, ("G", "A", "packed"), ()),
    }, n


def _good():
    a = {k: P for k in ("x", "packed", "logits", "n2", "g", "dx", "beta", "workspace", "dGA", "G", "A")}
    a.update(bf16=0, tokens=5, d=256, classes=33, parts=2)
    return a


def _refused(lib, name, call, code, what, **over):
    a = _good()
    a.update(over)
    assert call(a) == code, (name, over)
    text = _lib.last_error()
    assert text.startswith(name + ":") and what in text, (name, over, text)


def test_every_entry_point_refuses_bad_arguments_and_names_itself(lib):
    calls, n = _calls(lib)
    for name, (call, pointers, aligned16) in calls.items():
        for ptr in pointers:
            _refused(lib, name, call, NULL_POINTER, "null pointer", **{ptr: None})
        _refused(lib, name, call, BAD_DIMS, "dimension", d=128)
        for classes in (0, 8193, -1):
            _refused(lib, name, call, BAD_DIMS, "dimension", classes=classes)
        if name != "msda_cls_head_pack":
            for tokens in (0, -3):
                _refused(lib, name, call, BAD_DIMS, "dimension", tokens=tokens)
            for parts in (0, 3):
                _refused(lib, name, call, BAD_DIMS, "dimension", parts=parts)
        for ptr in aligned16:
            _refused(lib, name, call, MISALIGNED, "align", **{ptr: P + 8})
        for ptr in set(pointers) - set(aligned16) - {"G", "A", "packed"}:      # fp32 buffers: element alignment
            _refused(lib, name, call, MISALIGNED, "align", **{ptr: P + 2})
    # the two queries
    assert lib.msda_cls_head_packed_elems(33, None) == NULL_POINTER and _lib.last_error().startswith("msda_cls_head_packed_elems:")
    for classes in (0, 8193):
        assert lib.msda_cls_head_packed_elems(classes, ctypes.byref(n)) == BAD_DIMS and _lib.last_error().startswith("msda_cls_head_packed_elems:")
    assert lib.msda_cls_head_workspace_bytes(5, 33, None) == NULL_POINTER and _lib.last_error().startswith("msda_cls_head_workspace_bytes:")
    for tokens, classes in ((0, 33), (5, 0), (5, 8193)):
        assert lib.msda_cls_head_workspace_bytes(tokens, classes, ctypes.byref(n)) == BAD_DIMS
        assert _lib.last_error().startswith("msda_cls_head_workspace_bytes:")
    with pytest.raises(RuntimeError, match="msda_cls_head_forward.*dimension"):
        _lib.check(calls["msda_cls_head_forward"][0](dict(_good(), d=512)))


def test_the_queries_count_what_the_kernels_use(lib):
    n = ctypes.c_int64(0)
    for classes in (1, 16, 17, 33, 1204, 8192):
        assert lib.msda_cls_head_packed_elems(classes, ctypes.byref(n)) == 0
        tiles, steps = 16 + (classes + 15) // 16, (classes + 31) // 32
        assert n.value == tiles * 2 * 8 * 512 + steps * 2 * 16 * 512, classes      # [A; G] tiles, then G^T by steps of 32 classes; hi + lo
        assert n.value % 8 == 0
    for tokens, splits in ((1, 1), (511, 1), (512, 1), (513, 2), (13104, 26)):
        assert lib.msda_cls_head_workspace_bytes(tokens, 1204, ctypes.byref(n)) == 0
        assert n.value == splits * (1204 + 256) * 256 * 4, tokens


def test_each_entry_point_has_one_call_site():
    """as tests/test_loss_host_layer.py: one marshalling function per entry point, all in class_head.py"""
    for sym in ("msda_cls_head_packed_elems", "msda_cls_head_pack", "msda_cls_head_forward", "msda_cls_head_backward_rows",
                "msda_cls_head_workspace_bytes", "msda_cls_head_backward_weights"):
        hits = []
        for path in sorted(glob.glob(os.path.join(ROOT, "richsem_amd", "*.py"))):
            if os.path.basename(path) != "_lib.py":
                hits += [os.path.basename(path)] * len(re.findall(r"\.%s\(" % sym, open(path, encoding="utf-8").read()))
        assert hits == ["class_head.py"], (sym, hits)


def test_the_class_head_has_no_cpu_path():
    import torch
    from richsem_amd.class_head import ClassHead
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ClassHead().prepare(torch.zeros(8, 256), torch.zeros(3, 8), torch.tensor(0.0))
