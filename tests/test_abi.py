"""CPU: the C-ABI library builds for gfx950, loads, exports every symbol include/richsem_msda.h declares,
and rejects bad arguments on the host (no kernel is launched in this file)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from richsem_amd import _build, _lib

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "richsem_msda.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(msda_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.SYMBOLS)


def test_library_exports_every_declared_symbol(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for sym in declared_symbols():
        assert sym in exported, sym
        assert getattr(lib, sym) is not None


def test_library_contains_gfx950_code_object():
    blob = open(_lib.lib_path(), "rb").read()
    assert b"gfx950" in blob and b"fwd_direct_kernel" in blob and b"bwd_direct_kernel" in blob


def test_abi_version(lib):
    assert lib.msda_abi_version() == _lib.ABI_VERSION
    m = re.search(r"#define RICHSEM_MSDA_ABI_VERSION (\d+)", open(HEADER).read())
    assert int(m.group(1)) == _lib.ABI_VERSION


def test_options_roundtrip(lib):
    for key in ("fwd_variant", "bwd_variant", "bwd_split", "profile_filter"):
        old = _lib.get_option(key)
        _lib.set_option(key, 1)
        assert _lib.get_option(key) == 1
        _lib.set_option(key, old)
    with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION"):
        _lib.set_option("profile_filter", 48)
    with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION"):
        _lib.set_option("fwd_variant", 4)
    assert _lib.get_option("locality_monitor") == 1          # on by default
    _lib.set_option("locality_monitor", 0)
    assert _lib.get_option("locality_monitor") == 0
    _lib.set_option("locality_monitor", 1)
    assert _lib.get_option("locality_share_ppm") == -1       # nothing measured (and nothing can be, without a GPU)
    with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION"):
        _lib.set_option("locality_share_ppm", 5)             # read-only
    for key in ("no_such_option", "tile_debug"):
        with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION") as ei:
            _lib.set_option(key, 1)
        assert f"unknown option or value: {key}=1" in str(ei.value)
    with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION"):
        _lib.set_option("fwd_variant", 99)
    _walk_every_option(lib)


# every key msda_set_option accepts, with its lowest and highest accepted value and the values inside that range it rejects
_SETTABLE = {
    "fwd_variant": (0, 3, ()), "fwd_prep_fused": (0, 2, ()), "bwd_variant": (0, 5, (2, 3)), "band_lds_kb": (16, 150, ()),
    "band_hits": (32, 65536, ()), "rps_tile": (4, 16, ()), "rps_max_chunks": (1, 4096, ()), "rps_route_wgs": (1, 64, ()),
    "rps_seg_shift": (3, 11, ()), "rps_order": (0, 1, ()), "bwd_direct_cpl": (0, 4, (3,)), "tile_region": (4, 64, ()),
    "tile_margin": (0, 32, ()), "tile_persist": (0, 65536, ()), "bwd_levelsum": (0, 1, ()),
    "bwd_split": (0, 1, ()), "profile_filter": (0, 47, ()), "levelsum_lds_kb": (8, 150, ()), "tile_grow": (0, 1, ()),
    "locality_monitor": (0, 1, ()),
}
_READ_ONLY = ("locality_share_ppm",)


def _walk_every_option(lib):
    for key, (lo, hi, holes) in _SETTABLE.items():
        old = _lib.get_option(key)
        try:
            for v in (lo, hi):
                _lib.set_option(key, v)
                assert _lib.get_option(key) == v, (key, v)
            for v in (lo - 1, hi + 1) + tuple(holes):
                with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION") as ei:
                    _lib.set_option(key, v)
                assert f"unknown option or value: {key}={v}" in str(ei.value)
                assert _lib.get_option(key) == hi, (key, v)      # a rejected value changes nothing
        finally:
            _lib.set_option(key, old)
        assert _lib.get_option(key) == old
    for key in _READ_ONLY:
        _lib.get_option(key)
        for v in (-1, 0, 1):
            with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION") as ei:
                _lib.set_option(key, v)
            assert f"unknown option or value: {key}={v}" in str(ei.value)
    for key in ("no_such_option", "tile_debug"):
        with pytest.raises(RuntimeError, match="MSDA_ERR_BAD_OPTION") as ei:
            _lib.get_option(key)
        assert f"unknown option: {key}" in str(ei.value)
    assert lib.msda_set_option(None, 0) == -7 and "unknown option or value: (null)=0" in _lib.last_error()
    v = ctypes.c_int(0)
    assert lib.msda_get_option(None, ctypes.byref(v)) == -7 and "unknown option: (null)" in _lib.last_error()
    assert lib.msda_get_option(b"fwd_variant", None) == -1      # MSDA_ERR_NULL_POINTER



def _call_forward(lib, dims, shapes, lsi, im2col_step=64, null=None, ptr=0x1000):
    """Forward entry with fake (never dereferenced) device pointers: every check below fails on the host,
    before anything touches a device."""
    N, S, M, D, L, Lq, P = dims
    sh = np.asarray(shapes, dtype=np.int64)
    ls = np.asarray(lsi, dtype=np.int64)
    p = [ptr] * 5
    if null is not None:
        p[null] = None
    return lib.msda_forward_f32(p[0], p[1], p[2], p[3], p[4], N, S, M, D, L, Lq, P, im2col_step, ptr,
                                sh.ctypes.data, ls.ctypes.data, None)


def test_argument_errors_are_reported_not_printed(lib):
    good = (2, 30, 2, 4, 2, 5, 2)
    shapes, lsi = [[6, 4], [3, 2]], [0, 24]
    assert _call_forward(lib, good, shapes, lsi, null=0) == -1                      # MSDA_ERR_NULL_POINTER
    assert _call_forward(lib, (2, 30, 2, 0, 2, 5, 2), shapes, lsi) == -2            # non-positive D
    assert _call_forward(lib, (2, 31, 2, 4, 2, 5, 2), shapes, lsi) == -2            # sum H*W != S
    assert "!= S" in _lib.last_error()
    assert _call_forward(lib, good, shapes, [0, 25]) == -2                          # level runs past S
    assert _call_forward(lib, good, [[6, 4], [0, 2]], lsi) == -2                    # empty level
    assert _call_forward(lib, (3, 30, 2, 4, 2, 5, 2), shapes, lsi, im2col_step=2) == -3   # 3 % min(3,2) != 0
    assert "must divide im2col_step" in _lib.last_error()
    assert _call_forward(lib, good, shapes, lsi, im2col_step=0) == -3
    assert _call_forward(lib, (4, 1 << 20, 8, 64, 1, 5, 2), [[1024, 1024]], [0]) == -4   # >= 2^31 elements
    assert _call_forward(lib, good, shapes, lsi, ptr=0x1002) == -5                  # misaligned pointers
    with pytest.raises(RuntimeError, match="MSDA_ERR_MISALIGNED"):
        _lib.check(-5)


# element sizes of (value / out / grad_out / grad_value, sampling_loc / attn_weight and their gradients) per entry-point suffix
_ELEM = {"f32": (4, 4), "f64": (8, 8), "bf16": (2, 4)}


def _call_with_pointers(lib, sfx, backward, bad):
    """msda_forward_<sfx> / msda_backward_<sfx> with fake device pointers, all 0x1000 except those in ``bad`` (argument name -> address), and
    the host mirrors given: a call the alignment check refuses never dereferences any of them."""
    N, S, M, D, L, Lq, P = 2, 30, 2, 4, 2, 5, 2
    sh = np.asarray([[6, 4], [3, 2]], dtype=np.int64)
    ls = np.asarray([0, 24], dtype=np.int64)
    names = ["value", "shapes", "lsi", "loc", "aw"] + (["grad_out"] if backward else [])
    outs = ["grad_value", "grad_loc", "grad_aw"] if backward else ["out"]
    assert set(bad) <= set(names + outs)
    p = lambda k: bad.get(k, 0x1000)
    fn = getattr(lib, ("msda_backward_" if backward else "msda_forward_") + sfx)
    return fn(*[p(k) for k in names], N, S, M, D, L, Lq, P, 64, *[p(k) for k in outs], sh.ctypes.data, ls.ctypes.data, None)


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_every_entry_point_refuses_pointers_below_element_alignment(lib, sfx):
    """Row "pointer alignment demanded" of the dispatch table (msda_api.hip, above too_many_levels): sizeof(TV) for value / out / grad_out /
    grad_value, sizeof(T) for attn_weight and its gradient, 2*sizeof(T) for sampling_loc and its gradient -- for bf16 storage 2, 4 and
    8 bytes -- in all six entry points.  Each call has ONE pointer the library refuses; none is ever dereferenced.  Row "error texts":
    the bf16 message names "8 bytes", the others "2*sizeof(T)"."""
    ev, et = _ELEM[sfx]
    need = "8 bytes" if sfx == "bf16" else "2*sizeof(T)"
    cases = [(False, k, 0x1000 + ev // 2) for k in ("value", "out")]
    cases += [(True, k, 0x1000 + ev // 2) for k in ("value", "grad_out", "grad_value")]
    for backward in (False, True):
        cases += [(backward, "loc", 0x1000 + et), (backward, "aw", 0x1000 + et // 2)]      # loc: an element boundary, not a pair boundary
    cases += [(True, "grad_loc", 0x1000 + et), (True, "grad_aw", 0x1000 + et // 2)]
    for backward, name, addr in cases:
        assert _call_with_pointers(lib, sfx, backward, {name: addr}) == -5, (sfx, backward, name, hex(addr))      # MSDA_ERR_MISALIGNED
        text = _lib.last_error()
        assert "misaligned pointer" in text and need in text, (sfx, backward, name, text)
        assert ("grad_sampling_loc" in text) == backward, text
    assert (0x1004, 0x1008)[sfx == "f64"] == 0x1000 + et      # (the addresses the loc cases use: 0x1004 for f32 / bf16, 0x1008 for f64)


def test_host_variants_are_declared_and_not_implemented_as_in_the_reference(lib):
    """msda_forward_cpu / msda_backward_cpu (SURVEY.md section 8b "host (_cpu) variants of both"): the reference's bodies are
    AT_ERROR("Not implement on cpu") (src/cpu/ms_deform_attn_cpu.cpp:17-41); these return MSDA_ERR_NOT_ON_CPU with that text, touch no
    argument and launch nothing (called here with null pointers, on a machine without a GPU)."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.msda_forward_cpu.argtypes = [vp] * 5 + [ci] * 8 + [vp]
    lib.msda_forward_cpu.restype = ci
    lib.msda_backward_cpu.argtypes = [vp] * 6 + [ci] * 8 + [vp] * 3
    lib.msda_backward_cpu.restype = ci
    assert lib.msda_forward_cpu(*([None] * 5), 1, 1, 1, 1, 1, 1, 1, 64, None) == -8
    assert _lib.last_error() == "Not implement on cpu"
    assert lib.msda_backward_cpu(*([None] * 6), 1, 1, 1, 1, 1, 1, 1, 64, None, None, None) == -8
    assert _lib.last_error() == "Not implement on cpu"


def test_im2col_step_contract_matches_reference(lib):
    """reference ms_deform_attn_cuda.cu:48-52: step' = min(N, step); N % step' must be 0."""
    shapes, lsi = [[6, 4], [3, 2]], [0, 24]
    for N, step in [(6, 4), (5, 2), (7, 3), (64 * 3 + 1, 64)]:
        assert _call_forward(lib, (N, 30, 2, 4, 2, 5, 2), shapes, lsi, im2col_step=step) == -3
        assert f"batch({N}) must divide im2col_step({min(N, step)})" in _lib.last_error()


def test_error_notes_of_the_other_translation_units_name_the_call():
    """A failed argument check in the conv / lin256 / ffn / cls / attn / rows entry points leaves "<entry point>: <class of error>" in
    msda_last_error() (no GPU needed: the checks come before any launch)."""
    from richsem_amd import _lib
    L = _lib.load()
    n = ctypes.c_int64(0)
    rc = L.msda_conv_wgrad_workspace_bytes(1, 8, 8, 100, 128, 1, 1, 1, 0, ctypes.byref(n))        # C_in not a multiple of 128
    assert rc != 0
    with pytest.raises(RuntimeError, match="msda_conv_wgrad_workspace_bytes.*dimension"):
        _lib.check(rc)
    rc = L.msda_sine_embed_bf16(None, 4, 1, 4, 128, 10000.0, None, None)
    with pytest.raises(RuntimeError, match="msda_sine_embed_bf16.*null pointer"):
        _lib.check(rc)
    # the codes that used to come out as "<entry point>: error": a bad option value, and (on a machine without a GPU) no device
    assert L.msda_conv_set_ring(5) == -7
    assert re.fullmatch(r"msda_conv_set_ring: option value .*", _lib.last_error())
    import torch
    if not torch.cuda.is_available():
        buf = (ctypes.c_char * 1024)()
        p = (ctypes.addressof(buf) + 255) & ~255
        rc = L.msda_ffn_forward_bf16(p, p, p, p, p, p, p, 1e-5, 4, 256, 2048, p, None)
        assert rc == -6 and re.fullmatch(r"msda_ffn_forward\w*_bf16: no device.*", _lib.last_error()), _lib.last_error()      # MSDA_ERR_NO_DEVICE


def test_a_failed_launch_names_its_own_entry_point():
    """Without a device every launch fails (hipErrorNoDevice): the call returns the positive hipError_t and msda_last_error() is
    "<entry point>...: <hipGetErrorString> (hipError N)" of THIS call, not the text an earlier failed call left behind.  One entry point
    per translation unit.  With a GPU the host pointers below must never reach a launch: skipped before any library call."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU: the launches below are meant to fail")
    L = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    n = ctypes.c_int64(0)
    seeds = {      # a failed argument check of a DIFFERENT entry point
        "msda_sine_embed_bf16": lambda: L.msda_sine_embed_bf16(None, 4, 1, 4, 128, 10000.0, None, None),
        "msda_cls_packed_elems": lambda: L.msda_cls_packed_elems(0, ctypes.byref(n)),
    }
    calls = [
        ("msda_mask_rows_f32", lambda: L.msda_mask_rows_f32(p, p, 4, 8, None)),                                      # rows_api (moved there)
        ("msda_sine_embed_bf16", lambda: L.msda_sine_embed_bf16(p, 4, 1, 4, 128, 1e4, p, None)),                     # rows_api
        ("msda_lin256_pack_bf16", lambda: L.msda_lin256_pack_bf16(p, 64, 256, p, None)),                             # lin256_mfma
        ("msda_ffn_pack_w2_bf16", lambda: L.msda_ffn_pack_w2_bf16(p, 256, 32, p, None)),                             # ffn_mfma
        ("msda_cls_pack", lambda: L.msda_cls_pack(p, 16, p, 256, p, None)),                                          # cls_mfma
        ("msda_conv_pack_weight", lambda: L.msda_conv_pack_weight(p, 32, 32, 1, 1, p, None)),                        # conv_mfma
        ("msda_attn_forward_bf16", lambda: L.msda_attn_forward_bf16(p, 256, p, 256, p, 256, None, 32, 1, 0, 8, p, p, p, None)),   # attn_mfma
        ("msda_conv_wgrad_bf16", lambda: L.msda_conv_wgrad_bf16(p, p, 1, 4, 4, 128, 128, 1, 1, 1, 0, p, None, None, 0, p, None)),  # conv_wgrad
    ]
    for name, call in calls:
        seed = "msda_cls_packed_elems" if name == "msda_sine_embed_bf16" else "msda_sine_embed_bf16"
        assert seeds[seed]() < 0 and seed in _lib.last_error()
        rc = call()
        text = _lib.last_error()
        assert rc > 0, (name, rc)
        assert name in text and "hipError" in text, (name, text)
        assert seed not in text, (name, text)


def test_round4_entry_points_check_their_arguments_on_the_host():
    """ABI v7's additions (convolution rings / fused input gradient / grouped weight gradients, box refinement with the reference's gradient,
    the criterion's pair kernels): null pointers, bad dimensions, misalignment and bad option values are refused before any launch"""
    L = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15
    for bad in (2, 5, 7, -2):
        assert L.msda_conv_set_ring(bad) != 0
    with pytest.raises(RuntimeError, match="msda_conv_set_ring.*BAD_OPTION"):
        _lib.check(L.msda_conv_set_ring(5))
    for ok in (-1, 3, 4, 6, 0):
        assert L.msda_conv_set_ring(ok) == 0
    assert L.msda_conv_set_wgrad_ring(2) != 0 and L.msda_conv_set_wgrad_ring(1) == 0
    # fused input gradient: nulls, C_out not a multiple of 32, an output size that does not match, a misaligned `add`
    args = lambda dy, w, dx, add=None, mask=None, Cout=64, Ho=4: (dy, w, 1, Ho, 4, Cout, 64, 1, 1, 1, 0, 4, 4, add, mask, dx, None, None)
    assert L.msda_conv_dgrad_fused_bf16(*args(None, p16, p16)) == -1
    assert L.msda_conv_dgrad_fused_bf16(*args(p16, p16, p16, Cout=48)) == -2
    assert L.msda_conv_dgrad_fused_bf16(*args(p16, p16, p16, Ho=5)) == -2
    with pytest.raises(RuntimeError, match="msda_conv_dgrad_fused_bf16.*align"):
        _lib.check(L.msda_conv_dgrad_fused_bf16(*args(p16, p16, p16, add=p16 + 2)))
    # grouped weight gradients: no problems, too many, a channel count the kernel does not take, a missing workspace
    n = ctypes.c_int64(0)
    arr = (_lib.WgradProblem * 9)()
    for j in range(9):
        arr[j] = _lib.WgradProblem(p16, p16, p16, None, None, 1, 64, 64, 128, 128, 1, 1, 1, 0)
    assert L.msda_conv_wgrad_group_workspace_bytes(arr, 0, ctypes.byref(n)) == -2
    assert L.msda_conv_wgrad_group_workspace_bytes(arr, 9, ctypes.byref(n)) == -2
    assert L.msda_conv_wgrad_group_workspace_bytes(arr, 3, None) == -1
    assert L.msda_conv_wgrad_group_workspace_bytes(arr, 3, ctypes.byref(n)) == 0 and n.value > 0 and n.value % 4 == 0
    assert L.msda_conv_wgrad_group_bf16(arr, 3, None, None) == -1                     # the split needs its workspace
    arr[1].Cin = 100
    with pytest.raises(RuntimeError, match="msda_conv_wgrad_group_workspace_bytes.*dimension"):
        _lib.check(L.msda_conv_wgrad_group_workspace_bytes(arr, 3, ctypes.byref(n)))
    # box refinement / pair losses
    assert L.msda_box_refine_backward_ref(p, p, 8, p, 0, None, 1e-3, p, None) == -1        # grad_ref without ref
    assert L.msda_box_refine_backward_ref(p, p, 0, p, 0, p, 1e-3, p, None) == -2
    assert L.msda_box_pair_loss_f32(p16, p16, p, 0, 5.0, 2.0, p, p16, None) == -2
    assert L.msda_box_pair_loss_f32(p16, None, p, 4, 5.0, 2.0, p, p16, None) == -1
    with pytest.raises(RuntimeError, match="msda_box_pair_loss_f32.*align"):
        _lib.check(L.msda_box_pair_loss_f32(p16 + 4, p16, p, 4, 5.0, 2.0, p, p16, None))
    assert L.msda_focal_pos_sum_f32(p, p, 0, 0.25, p, p, None) == -2
    assert L.msda_focal_pos_sum_f32(None, p, 4, 0.25, p, p, None) == -1
