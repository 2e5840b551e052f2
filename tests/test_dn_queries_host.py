"""CPU: the denoising queries from the counts on the device (``msda_dn_queries_f32`` / ``msda_dn_queries_backward_f32``, csrc/msda_dn_noise.h,
richsem_amd/dn.py) -- what can be said without a GPU: the two symbols are declared, bound and exported under an unchanged ABI version; every
host refusal names its entry point; the Python layer has no CPU fallback and one call site per entry point; ``dn_capacity`` is the
brute-force maximum; and the numpy restatement tests/dn_noise_ref.py, which the GPU tests compare the kernel with, reproduces what the
reference's own ``prepare_for_cdn`` computed (tests/golden/dn_noise_reference.npz, written by tests/golden/make_golden_dn_noise.py)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from richsem_amd import _build, _lib

from conftest import GOLDEN, ROOT
import dn_noise_ref as R

NULL_POINTER, BAD_DIMS, TOO_LARGE, MISALIGNED = -1, -2, -4, -5
FWD_PTRS = ("cum", "labels", "boxes", "uniform", "table", "q_label", "q_bbox", "noised_label", "noised_box", "attn_mask", "meta")
BWD_PTRS = ("grad_q_label", "noised_label", "grad_table")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "dn_noise_reference.npz"))


def _fwd(lib, target_cap=10, N=2, pad_cap=40, D=16, V=8, num_classes=7, num_queries=30, dn_number=100, ratio=0.5, scale=1.0, use_cdn=1, add_gt=0,
         **ptrs):
    """the forward entry with fake (never dereferenced) device pointers, 0x1000 unless given by name: every call here is refused on the host"""
    p = {k: 0x1000 for k in FWD_PTRS}
    p.update(ptrs)
    return lib.msda_dn_queries_f32(p["cum"], p["labels"], p["boxes"], target_cap, p["uniform"], p["table"], N, pad_cap, D, V, num_classes,
                                   num_queries, dn_number, ratio, scale, use_cdn, add_gt, p["q_label"], p["q_bbox"], p["noised_label"],
                                   p["noised_box"], p["attn_mask"], p["meta"], None)


def _bwd(lib, rows=80, D=16, V=8, **ptrs):
    p = {k: 0x1000 for k in BWD_PTRS}
    p.update(ptrs)
    return lib.msda_dn_queries_backward_f32(p["grad_q_label"], p["noised_label"], rows, D, V, p["grad_table"], None)


def _refused(lib, call, name, code, **kw):
    seed = lib.msda_sine_embed_bf16(None, 4, 1, 4, 128, 10000.0, None, None)      # another call's text is in place ...
    assert seed < 0 and "msda_sine_embed_bf16" in _lib.last_error()
    assert call(lib, **kw) == code, kw
    text = _lib.last_error()                                                      # ... and this call's own replaces it
    assert text.startswith(name + ": "), text
    return text


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays(lib):
    header = open(os.path.join(ROOT, "include", "richsem_msda.h")).read()
    assert int(re.search(r"#define RICHSEM_MSDA_ABI_VERSION (\d+)", header).group(1)) == 13
    assert lib.msda_abi_version() == 13 and _lib.ABI_VERSION == 13
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    for sym in ("msda_dn_queries_f32", "msda_dn_queries_backward_f32"):
        assert sym in _lib.SYMBOLS and re.search(r"\bint %s\(" % sym, header), sym
        assert re.search(r"\bT %s$" % sym, exported, re.M), sym
        assert getattr(lib, sym).argtypes is not None and getattr(lib, sym).restype is not None
    blob = open(_lib.lib_path(), "rb").read()
    assert b"dn_queries_kernel" in blob and b"dn_queries_backward_kernel" in blob


@pytest.mark.parametrize("name", ["cum", "labels", "boxes", "uniform", "table", "q_label", "q_bbox", "noised_label", "attn_mask", "meta"])
def test_forward_refuses_a_null_pointer(lib, name):
    assert "null pointer" in _refused(lib, _fwd, "msda_dn_queries_f32", NULL_POINTER, **{name: None})


def test_forward_takes_null_for_buffers_without_elements(lib):
    """(noised_box is optional; with no slots and no targets the buffers of size 0 may be null: the next check -- a bad dimension -- answers)"""
    assert "dimension" in _refused(lib, _fwd, "msda_dn_queries_f32", BAD_DIMS, noised_box=None, V=0)
    assert "dimension" in _refused(lib, _fwd, "msda_dn_queries_f32", BAD_DIMS, pad_cap=0, target_cap=0, labels=None, boxes=None, uniform=None,
                                   q_label=None, q_bbox=None, noised_label=None, V=0)


@pytest.mark.parametrize("kw", [dict(N=0), dict(pad_cap=-1), dict(D=0), dict(D=18), dict(D=2), dict(V=0), dict(num_classes=0), dict(num_queries=-1),
                                dict(dn_number=-1), dict(target_cap=-1), dict(use_cdn=2), dict(add_gt=-1), dict(ratio=-0.5), dict(scale=-1.0),
                                dict(ratio=float("nan"))], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_forward_refuses_bad_dimensions(lib, kw):
    assert "dimension" in _refused(lib, _fwd, "msda_dn_queries_f32", BAD_DIMS, **kw)


def test_forward_refuses_misaligned_and_oversized_calls(lib):
    for name, addr in (("boxes", 0x1008), ("table", 0x1004), ("q_label", 0x1008), ("q_bbox", 0x1004), ("noised_box", 0x1008), ("attn_mask", 0x1001),
                       ("cum", 0x1004), ("labels", 0x1004), ("noised_label", 0x1004), ("meta", 0x1004), ("uniform", 0x1002)):
        assert "aligned" in _refused(lib, _fwd, "msda_dn_queries_f32", MISALIGNED, **{name: addr}), name
    assert "too large" in _refused(lib, _fwd, "msda_dn_queries_f32", TOO_LARGE, N=1 << 16, pad_cap=1 << 16)      # N * pad_cap >= 2^31


def test_backward_refuses_bad_arguments(lib):
    for name in BWD_PTRS:
        assert "null pointer" in _refused(lib, _bwd, "msda_dn_queries_backward_f32", NULL_POINTER, **{name: None})
    for kw in (dict(rows=-1), dict(D=0), dict(D=6), dict(V=0)):
        assert "dimension" in _refused(lib, _bwd, "msda_dn_queries_backward_f32", BAD_DIMS, **kw)
    for name, addr in (("grad_q_label", 0x1008), ("grad_table", 0x1004), ("noised_label", 0x1004)):
        assert "aligned" in _refused(lib, _bwd, "msda_dn_queries_backward_f32", MISALIGNED, **{name: addr}), name
    assert "too large" in _refused(lib, _bwd, "msda_dn_queries_backward_f32", TOO_LARGE, rows=1 << 34, D=256)


def test_python_layer_has_no_cpu_fallback_and_checks_its_arguments():
    import richsem_amd
    from richsem_amd import dn
    assert richsem_amd.denoising_queries is dn.denoising_queries and richsem_amd.dn_capacity is dn.dn_capacity
    assert richsem_amd.DenoisingQueriesFunction is dn.DenoisingQueriesFunction
    cum, labels, boxes = torch.tensor([0, 1, 3]), torch.tensor([4, 5, 6]), torch.rand(3, 4)
    kw = dict(pad_cap=8, num_queries=5, num_classes=7, dn_number=100, label_noise_ratio=0.5, box_noise_scale=1.0)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        dn.denoising_queries(cum, labels, boxes, torch.rand(8, 16), torch.rand(2, 8, 10), **kw)
    with pytest.raises(NotImplementedError, match="check_pos_dn"):
        dn.denoising_queries(cum, labels, boxes, torch.rand(8, 16), torch.rand(2, 8, 10), check_pos_dn=True, **kw)


def test_each_entry_point_has_one_call_site():
    """the host-layer rule: a library entry point is called from one place in the Python package"""
    for sym in ("msda_dn_queries_f32", "msda_dn_queries_backward_f32"):
        hits = []
        for d, _, files in os.walk(os.path.join(ROOT, "richsem_amd")):
            for f in files:
                if f.endswith(".py") and f != "_lib.py":
                    text = open(os.path.join(d, f), encoding="utf-8").read()
                    hits += [f] * len(re.findall(r"\.%s\(" % sym, text))
        assert hits == ["dn.py"], (sym, hits)


@pytest.mark.parametrize("add_gt", [False, True])
@pytest.mark.parametrize("use_cdn", [True, False])
def test_dn_capacity_is_the_brute_force_maximum(use_cdn, add_gt):
    from richsem_amd.dn import dn_capacity, dn_group_count
    for dn_number in (0, 1, 3, 49, 50, 100, 300):
        for max_targets in (0, 1, 2, 7, 49, 50, 51, 99, 100, 101, 150, 333):
            want = 0
            for m in range(max_targets + 1):      # every possible largest count; the other images only add empty slots
                pad = m * 2 * dn_group_count(dn_number, [m, max(m - 1, 0)], add_gt)
                want = max(want, pad if use_cdn else pad // 2)
            assert dn_capacity(dn_number, max_targets, add_gt, use_cdn) == want, (dn_number, max_targets)
    for m in (0, 1, 30, 100, 101, 250):
        assert dn_capacity(100, m) == max(200, 2 * m) if m else dn_capacity(100, m) == 0


def test_the_uniform_encoding_of_a_class_floors_back_to_it():
    for C in (1, 2, 7, 80, 91, 1203, 1204, 4096):
        k = np.arange(C)
        u = ((k + 0.5).astype(np.float32) / np.float32(C)).astype(np.float32)
        assert (u < 1).all() and np.array_equal(np.floor(u * np.float32(C)).astype(np.int64), k), C


def _case(golden, name):
    z = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + ".")}
    hidden, nq, ncls = (int(v) for v in golden["dims"])
    dn_number, use_cdn, add_gt = (int(v) for v in z["args"])
    ratio, scale = (float(v) for v in z["noise"])
    pad_size = int(z["meta"][0])
    u = R.uniform_from_draws(z["counts"], z["p"], z["new_label"], z["sign01"], z["rand"], ncls, pad_size, bool(use_cdn))
    kw = dict(pad_cap=pad_size, num_queries=nq, num_classes=ncls, dn_number=dn_number, label_noise_ratio=ratio, box_noise_scale=scale,
              use_cdn=bool(use_cdn), add_gt=bool(add_gt))
    return z, u, kw


def _reference_labels(z, use_cdn):
    """what the reference embedded, in its row order: the drawn class where one was drawn, else the target's"""
    n, total = len(z["p"]), len(z["labels"])
    lab = np.tile(z["labels"], n // total if total else 0)
    return np.where(z["new_label"] >= 0, z["new_label"], lab)


def test_fixture_has_the_cases_and_clamps_at_both_ends(golden):
    assert sorted(golden["cases"].tolist()) == ["add_gt", "edge", "empty", "no_cdn", "one_group", "ragged", "small_dn"]
    z, u, kw = _case(golden, "edge")
    pre = R.denoising_queries_ref(z["counts"], z["labels"], z["boxes"], u, golden["table"], return_preclamp=True, **kw)["preclamp"]
    assert (pre < 0).any() and (pre > 1).any()
    assert 0 in _case(golden, "ragged")[0]["counts"] and not _case(golden, "no_cdn")[2]["use_cdn"] and _case(golden, "add_gt")[2]["add_gt"]
    assert _case(golden, "one_group")[0]["meta"][1] == 1 and 2 * _case(golden, "one_group")[0]["counts"].max() > 200
    assert os.path.getsize(os.path.join(GOLDEN, "dn_noise_reference.npz")) < 512 * 1024


@pytest.mark.parametrize("name", ["add_gt", "edge", "empty", "no_cdn", "one_group", "ragged", "small_dn"])
def test_restatement_reproduces_the_reference(golden, name):
    z, u, kw = _case(golden, name)
    got = R.denoising_queries_ref(z["counts"], z["labels"], z["boxes"], u, golden["table"], **kw)
    single = int(z["counts"].max())
    assert got["meta"].tolist() == [single, int(z["meta"][1]), int(z["meta"][0]), int(z["counts"].sum()), 0]
    assert np.array_equal(got["attn_mask"], z["attn_mask"])
    assert got["q_label"].shape == z["input_query_label"].shape and got["q_label"].tobytes() == z["input_query_label"].tobytes()
    groups2 = len(z["p"]) // max(len(z["labels"]), 1)
    rows = R.rows_from_slots(z["counts"], got["noised_box"], groups2, kw["use_cdn"])
    kept = ~np.isnan(rows[:, 0])
    assert kept.sum() == (got["noised_label"] >= 0).sum()
    assert rows[kept].tobytes() == z["noised_box_rows"][kept].tobytes()      # the noised boxes, bit for bit
    lab_rows = R.rows_from_slots(z["counts"], got["noised_label"].astype(np.float64), groups2, kw["use_cdn"])
    assert np.array_equal(lab_rows[kept], _reference_labels(z, kw["use_cdn"])[kept].astype(np.float64))
    filled = got["noised_label"] >= 0
    assert np.array_equal(filled, np.abs(z["input_query_bbox"]).sum(-1) != 0)
    # q_bbox: the restatement runs the reference's float32 chain with numpy's logarithm, the reference with torch's -- within the bound
    _, bound = R.q_bbox_bound(got["noised_box"])
    err = np.abs(got["q_bbox"].astype(np.float64) - z["input_query_bbox"].astype(np.float64))
    assert (err[filled] <= bound[filled]).all() and not got["q_bbox"][~filled].any()


def test_reference_float32_q_bbox_against_the_float64_value(golden):
    """How far the reference's own float32 ``input_query_bbox`` is from y64, the float64 inverse_sigmoid of the same noised box -- the value the
    GPU test holds the kernel to, within 2^-24 + k ulp32(|y64|).  A float32 chain in the reference's order cannot promise that bound: it rounds
    1 - x and x1 / x2 in front of the logarithm, up to 2^-24 relative each, so up to 2^-23 in the result (dn_noise_ref.q_bbox_bound_float32_chain),
    and near x = 0.5, where the result is small, that is many of its ulps.  Asserted here: the reference is within 2^-23 + k ulp32(|y64|).
    Measured on the fixture (torch CPU float32, k = 2): 20 of 5352 filled elements are further than 2^-24 + k ulp32(|y64|) from y64, the worst at
    1.291 x that (case add_gt: x = 0.49535546, y64 = -0.0185787061, reference -0.018578624), all with x in 0.46 .. 0.50 -- which is why the kernel
    takes the quotient and the logarithm in float64 (csrc/msda_dn_noise.h: dn_inverse_sigmoid)."""
    worst, outside, n = 0.0, 0, 0
    for name in golden["cases"].tolist():
        z, u, kw = _case(golden, name)
        got = R.denoising_queries_ref(z["counts"], z["labels"], z["boxes"], u, golden["table"], **kw)
        filled = got["noised_label"] >= 0
        y64, chain = R.q_bbox_bound_float32_chain(got["noised_box"])
        err = np.abs(z["input_query_bbox"].astype(np.float64) - y64)
        assert (err[filled] <= chain[filled]).all(), name
        ratio = (err / R.q_bbox_bound(got["noised_box"])[1])[filled]
        if ratio.size:
            worst, outside, n = max(worst, float(ratio.max())), outside + int((ratio > 1).sum()), n + ratio.size
    print(f"reference float32 q_bbox against 2^-24 + k ulp: worst {worst:.3f} x, {outside} of {n} elements outside")
    assert n == 5352
