"""The host layer of the operator's own translation unit (richsem_amd/csrc/msda_api.hip; DESIGN.md, "The host layer of the C ABI"); no GPU.

(a) What a refused call answers: the literal (return code, msda_last_error() text) of bad argument sets of msda_forward_*, msda_backward_*
    and msda_forward_prep_*, among them pairs of simultaneous faults -- which of two competing checks fires first is part of the ABI's
    behaviour.  Fake, suitably aligned pointers and the host mirrors of the level tables, as tests/test_abi.py::_call_forward: every case is
    refused by a host-side check before anything touches a device.
(b) The shape of that code, as source scans in the manner of tests/test_loss_host_layer.py: no thread-local state but the error text, one
    call site of check_problem, one function that allocates workspaces."""
import glob
import os
import re

import numpy as np
import pytest

from richsem_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "richsem_amd", "csrc")

NULL, DIMS, STEP, LARGE, ALIGN = -1, -2, -3, -4, -5      # MSDA_ERR_NULL_POINTER, _BAD_DIMS, _IM2COL_STEP, _TOO_LARGE, _MISALIGNED
P0 = 0x1000
GOOD = dict(dims=(2, 30, 2, 4, 2, 5, 2), shapes=[[6, 4], [3, 2]], lsi=[0, 24])      # decoder-shaped: Lq = 5 != S = 30, L * P = 4
# encoder-shaped (Lq == S) with L = 17, P = 4 -- L > kPrepMaxL = 16 and L * P > 64 -- whose 17 one-pixel levels do not sum to S = 18
ENC17 = dict(dims=(1, 18, 1, 4, 17, 18, 4), shapes=[[1, 1]] * 17, lsi=list(range(17)))
ENC17_CHECK = "sum of H*W over levels (17) != S (18)"
ENC17_PREP = "L (17) > 16 or L*P (68) > 64"
NEED = {"f32": "2*sizeof(T)", "f64": "2*sizeof(T)", "bf16": "8 bytes"}


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def _options(lib):
    saved = {k: _lib.get_option(k) for k in ("fwd_variant", "fwd_prep_fused")}
    yield
    for k, v in saved.items():
        _lib.set_option(k, v)


def _tables(shapes, lsi):
    return np.asarray(shapes, dtype=np.int64), np.asarray(lsi, dtype=np.int64)


def call(lib, entry, sfx, dims=GOOD["dims"], shapes=GOOD["shapes"], lsi=GOOD["lsi"], step=64, ptrs=None, ref_dim=2, strides=None):
    """entry: "forward", "backward" or "forward_prep".  ptrs: argument name -> address (None: a null pointer); every other pointer is P0,
    never dereferenced.  strides: (off_stride, log_stride) of forward_prep, a whole row each unless given."""
    N, S, M, D, L, Lq, P = dims
    sh, ls = _tables(shapes, lsi)
    p = lambda k: (ptrs or {}).get(k, P0)
    fn = getattr(lib, "msda_%s_%s" % (entry, sfx))
    if entry == "forward":
        rc = fn(*[p(k) for k in ("value", "shapes", "lsi", "loc", "aw")], N, S, M, D, L, Lq, P, step, p("out"), sh.ctypes.data, ls.ctypes.data, None)
    elif entry == "backward":
        rc = fn(*[p(k) for k in ("value", "shapes", "lsi", "loc", "aw", "grad_out")], N, S, M, D, L, Lq, P, step,
                *[p(k) for k in ("grad_value", "grad_loc", "grad_aw")], sh.ctypes.data, ls.ctypes.data, None)
    else:
        off_stride, log_stride = strides or (M * L * P * 2, M * L * P)
        rc = fn(p("value"), p("shapes"), p("lsi"), p("offsets"), off_stride, p("logits"), log_stride, p("ref"), ref_dim, N, S, M, D, L, Lq, P,
                step, p("out"), p("loc"), p("aw"), sh.ctypes.data, ls.ctypes.data, None)
    return rc, _lib.last_error()


def _with(dims=GOOD["dims"], **kw):
    """GOOD with single dimensions replaced by name"""
    names = ("N", "S", "M", "D", "L", "Lq", "P")
    return tuple(kw.get(n, v) for n, v in zip(names, dims))


NON_POSITIVE_D = "non-positive dimension (N=2 S=30 M=2 D=0 L=2 Lq=5 P=2)"
# what check_problem refuses, in the order of its checks: (arguments, return code, text) -- the same for every entry point that reaches it
CHECK_PROBLEM = [
    (dict(dims=_with(D=0)), DIMS, NON_POSITIVE_D),
    (dict(dims=_with(D=0), step=0), DIMS, NON_POSITIVE_D),                                                   # dimensions before im2col_step
    (dict(step=0), STEP, "im2col_step(0) must be positive"),
    (dict(dims=_with(S=31), step=0), STEP, "im2col_step(0) must be positive"),                               # im2col_step before the level tables
    (dict(dims=_with(N=3), step=2), STEP, "batch(3) must divide im2col_step(2)"),
    (dict(dims=(4, 1 << 20, 8, 64, 1, 5, 2), shapes=[[1024, 1024]], lsi=[0]), LARGE,
     "tensor with >= 2^31 elements (value 2147483648, out 10240, loc 640)"),
    (dict(shapes=[[6, 4], [0, 2]]), DIMS, "level 1: bad spatial shape (0, 2)"),
    (dict(lsi=[0, 25]), DIMS, "level 1: level_start_index 25 + 3*2 exceeds S=30"),
    (dict(dims=_with(S=31)), DIMS, "sum of H*W over levels (30) != S (31)"),
]


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_forward_and_backward_refusals(lib, sfx):
    """null pointer, then check_problem in its own order, then alignment -- in msda_forward_* and msda_backward_* of every type"""
    elem = {"f32": 4, "f64": 8, "bf16": 4}[sfx]      # of sampling_loc: one element past a pair boundary is misaligned
    texts = {"forward": "misaligned pointer (sampling_loc needs %s)" % NEED[sfx],
             "backward": "misaligned pointer (sampling_loc / grad_sampling_loc need %s)" % NEED[sfx]}
    for entry, last in (("forward", "out"), ("backward", "grad_aw")):
        for kw, rc, text in CHECK_PROBLEM:
            assert call(lib, entry, sfx, **kw) == (rc, text), (entry, kw)
            # ... which a misaligned pointer does not overtake, and a null pointer does
            assert call(lib, entry, sfx, ptrs={"loc": P0 + elem}, **kw) == (rc, text), (entry, kw)
            assert call(lib, entry, sfx, ptrs={last: None}, **kw) == (NULL, "null pointer argument"), (entry, kw)
        assert call(lib, entry, sfx, ptrs={"value": None, "loc": P0 + elem}) == (NULL, "null pointer argument")
        assert call(lib, entry, sfx, ptrs={"loc": P0 + elem}) == (ALIGN, texts[entry])
        assert call(lib, entry, sfx, ptrs={"shapes": P0 + 4}) == (ALIGN, texts[entry])
    assert call(lib, "backward", sfx, ptrs={"grad_loc": P0 + elem}) == (ALIGN, texts["backward"])
    assert call(lib, "backward", sfx, ptrs={"grad_out": None}) == (NULL, "null pointer argument")


def test_bf16_forward_misaligned_and_non_positive_d(lib):
    """bf16 forward, both misaligned (value on an odd address) and D = 0: the dimension check fires"""
    assert call(lib, "forward", "bf16", dims=_with(D=0), ptrs={"value": P0 + 1}) == (DIMS, NON_POSITIVE_D)
    assert call(lib, "forward", "bf16", ptrs={"value": P0 + 1}) == (ALIGN, "misaligned pointer (sampling_loc needs 8 bytes)")


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("fused", [0, 1, 2])
def test_forward_prep_own_checks_come_first(lib, sfx, fused):
    """msda_forward_prep_*: null pointer, reference width, row strides -- in that order, before anything about the problem, whatever
    fwd_prep_fused says"""
    _lib.set_option("fwd_prep_fused", fused)
    ref_text = "reference points must have 2 or 4 components, got 3"
    assert call(lib, "forward_prep", sfx, ptrs={"offsets": None}, ref_dim=3) == (NULL, "null pointer argument")
    assert call(lib, "forward_prep", sfx, ptrs={"loc": None}, dims=_with(D=0)) == (NULL, "null pointer argument")
    assert call(lib, "forward_prep", sfx, ref_dim=3, dims=_with(D=0)) == (DIMS, ref_text)
    assert call(lib, "forward_prep", sfx, ref_dim=3, strides=(1, 1)) == (DIMS, ref_text)
    assert call(lib, "forward_prep", sfx, strides=(7, 4), dims=_with(D=0)) == (DIMS, "row stride smaller than a row (offsets 7, logits 4)")
    assert call(lib, "forward_prep", sfx, strides=(8, 3), step=0) == (DIMS, "row stride smaller than a row (offsets 8, logits 3)")


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_forward_prep_decoder_shaped_fused(lib, sfx):
    """Decoder-shaped call under fwd_prep_fused = 1 (one kernel): check_problem, then the alignment of the fused call -- bad im2col_step and
    a misaligned sampling_loc together give the im2col_step text.  The misalignment text names 2*sizeof(T) for every type here."""
    _lib.set_option("fwd_prep_fused", 1)
    elem = {"f32": 4, "f64": 8, "bf16": 4}[sfx]
    for kw, rc, text in CHECK_PROBLEM:
        assert call(lib, "forward_prep", sfx, **kw) == (rc, text), kw
        assert call(lib, "forward_prep", sfx, ptrs={"loc": P0 + elem}, **kw) == (rc, text), kw
    assert call(lib, "forward_prep", sfx, step=0, ptrs={"loc": P0 + elem}) == (STEP, "im2col_step(0) must be positive")
    text = "misaligned pointer (sampling_loc needs 2*sizeof(T))"
    assert call(lib, "forward_prep", sfx, ptrs={"loc": P0 + elem}) == (ALIGN, text)
    assert call(lib, "forward_prep", sfx, ptrs={"ref": P0 + elem // 2}) == (ALIGN, text)
    assert call(lib, "forward_prep", sfx, ptrs={"offsets": P0 + 1}) == (ALIGN, text)
    assert call(lib, "forward_prep", sfx, ptrs={"lsi": P0 + 4}) == (ALIGN, text)


def test_forward_prep_encoder_shaped_order_follows_the_option(lib):
    """Encoder-shaped call with L = 17, P = 4 and level shapes that do not sum to S: two faults at once.  Under fwd_prep_fused = 2 an
    fp32-compute call with P = 4 and fwd_variant != 1 has its problem checked first (the window kernel would read the raw projection):
    check_problem's text.  Otherwise the location / softmax kernel's own checks come first: its text.  f64 never takes the first form."""
    for fused, variant, sfx, text in ((2, 0, "f32", ENC17_CHECK), (2, 2, "f32", ENC17_CHECK), (2, 3, "f32", ENC17_CHECK),
                                      (2, 0, "bf16", ENC17_CHECK), (2, 1, "f32", ENC17_PREP), (2, 0, "f64", ENC17_PREP),
                                      (1, 0, "f32", ENC17_PREP), (0, 0, "f32", ENC17_PREP), (0, 0, "bf16", ENC17_PREP), (0, 0, "f64", ENC17_PREP)):
        _lib.set_option("fwd_prep_fused", fused)
        _lib.set_option("fwd_variant", variant)
        assert call(lib, "forward_prep", sfx, **ENC17) == (DIMS, text), (fused, variant, sfx)
        assert _lib.get_option("fwd_variant") == variant


# ---- (b) the shape of the code --------------------------------------------------------------------------------------------------------------
def _host_files():
    """msda_api.hip and the host-only headers it alone includes"""
    api = os.path.join(CSRC, "msda_api.hip")
    text = open(api, encoding="utf-8").read()
    others = "".join(open(p, encoding="utf-8").read() for p in glob.glob(os.path.join(CSRC, "*.hip")) if p != api)
    own = [h for h in re.findall(r'#include "(msda_\w+\.h)"', text) if ('"%s"' % h) not in others and "__global__" not in
           open(os.path.join(CSRC, h), encoding="utf-8").read()]
    return {"msda_api.hip": text, **{h: open(os.path.join(CSRC, h), encoding="utf-8").read() for h in own}}


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def _function_of(text, pos):
    """name of the function whose body holds text[pos]: the last definition at column 0 before it"""
    heads = [m for m in re.finditer(r"^\w[\w:<>\*&, ]*[ \*&](\w+)\([^;{}]*\)\n\{", text[:pos], re.M)]
    return heads[-1].group(1)


def test_no_thread_local_state_but_the_error_text():
    for name, text in _host_files().items():
        lines = [l.strip() for l in _code(text).splitlines() if "thread_local" in l]
        assert lines == (['thread_local char g_err[512] = "";'] if name == "msda_api.hip" else []), (name, lines)


def test_check_problem_has_one_call_site():
    calls = [(name, m.start()) for name, text in _host_files().items() for m in re.finditer(r"(?<!int )\bcheck_problem\(", _code(text))]
    assert len(calls) == 1, calls


def test_workspaces_are_allocated_by_one_function():
    """every hipMalloc of the operator's host code sits in the one grower, the locality monitor's own counters aside"""
    where = []
    for name, text in _host_files().items():
        code = _code(text)
        where += [_function_of(code, m.start()) for m in re.finditer(r"\bhipMalloc\(", code)]
    assert sorted(where) == ["grow_buffer", "monitor_choose_fwd"], where
