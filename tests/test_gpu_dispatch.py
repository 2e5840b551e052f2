"""GPU (-m gpu): every row of the dispatch table of msda_forward_* / msda_backward_* (richsem_amd/csrc/msda_api.hip, the comment block above
``too_many_levels``) against the oracle -- which kernel a call gets, and that the kernel it gets is right.

The C ABI promises ELEMENT alignment only (2*sizeof(T) for sampling_loc and its gradient); freshly allocated torch tensors are 256-byte
aligned, so the branches the dispatch takes for less (narrower channels per lane, no window / split forward, no routed / band backward,
the scalar tail of the bf16 rounding pass, the two-kernel form of msda_forward_prep_*) run here on contiguous views with a storage offset,
through the C ABI with caller-allocated, NaN-poisoned outputs between sentinel guards, and through the Python shim.

References (computed once per (shape, dtype), module scope): f64 -- the oracle in f64; f32 -- the oracle in f32 on the same inputs; bf16 -- the
f32 oracle on the bf16-rounded inputs, as test_gpu_bf16.run_bf16 does.  Tolerances are the project's own: test_gpu_parity.tols for f32 / f64,
test_gpu_bf16.check (4e-3 + one bf16 ulp almost everywhere) for bf16.

Rows of the table and where they are held:
  pointer alignment demanded      tests/test_abi.py::test_every_entry_point_refuses_pointers_below_element_alignment (no GPU needed)
  window forward eligible         expected_fwd + test_alignment_matrix, test_preconditions
  channels per lane               test_alignment_matrix (value / out / grad_out offsets; ODD: D = 30 and D = 7)
  split forward / backward        expected_fwd + test_alignment_matrix, test_bf16_split_forward_against_oracle
  "too many levels"               test_level_table_limit
  routed / band backward entered  expected_bwd + test_alignment_matrix, test_preconditions
  ... a launch error there        not reachable without making a launch fail on purpose; the REFUSED attempt (hipErrorNotSupported) gives its
                                  record back in both instances: expected_bwd + test_alignment_matrix
  level-sum backward              test_alignment_matrix (all levels), test_levelsum_takes_a_subset_of_levels (f32: a subset; bf16: none)
  bwd_direct_cpl option           test_bwd_direct_cpl
  direct backward adds grad_value test_bwd_direct_cpl (into grad_value / the fp32 scratch), test_alignment_matrix (null: level-sum took everything)
  no scratch during capture       test_bf16_scratch_and_stream_capture
  error texts                     test_level_table_limit, test_bf16_scratch_and_stream_capture, tests/test_abi.py ("8 bytes")
"""
import numpy as np
import pytest
import torch

from oracle import msda_oracle as O
from richsem_amd import _lib, workload as W
from richsem_amd import MultiScaleDeformableAttention as MSDA
from richsem_amd.capture import capture
from richsem_amd.functions import MSDeformAttnFunction, MSDeformAttnFusedFunction

import test_gpu_bf16 as B
from test_gpu_parity import _profiled_variants, dev, rel_err, tols

pytestmark = pytest.mark.gpu

TORCH = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
WORK = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.float32}      # sampling_loc / attn_weight and their gradients
SENTINEL = 1536.0      # (exact in every storage type)
GUARD = 8              # guard elements at least, before and after a payload
_OPTIONS = ("fwd_variant", "bwd_variant", "bwd_levelsum", "bwd_direct_cpl", "bwd_split", "fwd_prep_fused", "locality_monitor")


@pytest.fixture(autouse=True)
def _options():
    """locality_monitor = 0 for every record assertion: the automatic forward of an encoder-shaped call is then the window kernel whatever
    earlier tests left in the monitor's table; every option a test may touch is put back afterwards"""
    saved = {k: _lib.get_option(k) for k in _OPTIONS}
    _lib.set_option("locality_monitor", 0)
    yield
    for k, v in saved.items():
        _lib.set_option(k, v)


# ---- shapes: the smallest that still take each path ------------------------------------------------------------------------------------------
def _shapes():
    odd = dict(N=1, M=2, P=3, shapes=[(9, 7), (3, 2)], Lq=40)
    return {
        "ENC": W.shrunk(W.call_E(2), 4),       # Lq == S, D = 32, L = P = 4: window forward, routed backward
        "DEC": W.shrunk(W.call_Dd(2), 4),      # decoder-shaped, split-eligible, every level goes to the level-sum kernel
        "ODD": W.Call("odd", odd["N"], odd["M"], 30, odd["P"], odd["shapes"], odd["Lq"], False),      # two channels per lane at most
        "ODD7": W.Call("odd7", odd["N"], odd["M"], 7, odd["P"], odd["shapes"], odd["Lq"], False),     # one channel per lane
    }


SHAPES = _shapes()
_inputs, _oracle, _device = {}, {}, {}


def host_inputs(name, call=None):
    """f32 inputs of a shape: the "init" pattern with the first few queries moved by loc * 3 - 1 (dropped samples, border corners)"""
    if name not in _inputs:
        t = W.make_inputs(call or SHAPES[name], "init", seed=41)
        t["loc"][0, :7] = t["loc"][0, :7] * 3.0 - 1.0
        _inputs[name] = {k: v.numpy() for k, v in t.items()}
    return _inputs[name]


def typed_inputs(name, sfx, call=None):
    """the inputs as the entry points of `sfx` take them (numpy; bf16 values as float32 arrays holding bf16-representable numbers)"""
    z = dict(host_inputs(name, call))
    if sfx == "f64":
        for k in ("value", "loc", "aw", "grad_out"):
            z[k] = z[k].astype(np.float64)
    elif sfx == "bf16":
        for k in ("value", "grad_out"):
            z[k] = torch.from_numpy(z[k]).to(torch.bfloat16).float().numpy()
    return z


def oracle(name, sfx, call=None):
    """(out, grad_value, grad_loc, grad_aw) of the oracle, as float64 arrays; computed once per (shape, dtype)"""
    if (name, sfx) not in _oracle:
        z = typed_inputs(name, sfx, call)
        oo = O.forward(z["value"], z["shapes"], z["lsi"], z["loc"], z["aw"])
        og = O.backward(z["value"], z["shapes"], z["lsi"], z["loc"], z["aw"], z["grad_out"])
        assert oo.dtype == (np.float64 if sfx == "f64" else np.float32)
        _oracle[(name, sfx)] = tuple(a.astype(np.float64) for a in (oo,) + tuple(og))
    return _oracle[(name, sfx)]


def device_inputs(name, sfx, call=None):
    """aligned device tensors of the typed inputs (never written to)"""
    if (name, sfx) not in _device:
        z = typed_inputs(name, sfx, call)
        t = {k: dev(z[k]) for k in ("shapes", "lsi", "loc", "aw")}
        t["value"], t["grad_out"] = dev(z["value"]).to(TORCH[sfx]), dev(z["grad_out"]).to(TORCH[sfx])
        t["host"] = (np.ascontiguousarray(z["shapes"]), np.ascontiguousarray(z["lsi"]))
        _device[(name, sfx)] = t
    return _device[(name, sfx)]


def assert_matches(got, name, sfx, note="", call=None):
    """got: dict with "out" and / or "grad_value", "grad_loc", "grad_aw" (device tensors).  bf16: test_gpu_bf16.check, unchanged -- a call
    that ran only its forward or only its backward hands check the correctly rounded oracle value for the half it did not compute."""
    want = oracle(name, sfx, call)
    oo, ogv, ogl, oga = want
    if sfx == "bf16":
        assert "out" in got or "grad_value" in got
        rounded = lambda a: torch.from_numpy(a).float().to(torch.bfloat16)
        try:
            B.check((got["out"] if "out" in got else rounded(oo), got["grad_value"] if "grad_value" in got else rounded(ogv),
                     got["grad_loc"] if "grad_loc" in got else torch.from_numpy(ogl), got["grad_aw"] if "grad_aw" in got else torch.from_numpy(oga)),
                    want)
        except AssertionError as e:
            raise AssertionError(f"{note}: {e}") from e
        return
    tf, tg = tols(TORCH[sfx])
    if "out" in got:
        assert rel_err(got["out"], oo) < tf, (note, rel_err(got["out"], oo))
    if "grad_value" in got:
        e = [rel_err(got["grad_value"], ogv), rel_err(got["grad_loc"], ogl), rel_err(got["grad_aw"], oga)]
        assert max(e) < tg, (note, e)


# ---- offset views and the ctypes caller ---------------------------------------------------------------------------------------------------
def offset_view(t, k):
    """A contiguous tensor equal to ``t`` whose data_ptr() lies ``k`` elements past a 256-byte boundary: a slice of one flat allocation, with
    at least GUARD sentinel elements before and after the payload (see guards_intact)."""
    per = 256 // t.element_size()
    assert 0 <= k < per and per >= GUARD
    start, n = per + k, t.numel()
    flat = torch.full((start + n + per,), SENTINEL, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 256 == 0
    v = flat[start:start + n].view(t.shape)
    v.copy_(t)
    v.guard = (flat, start, n)
    assert v.is_contiguous() and v.data_ptr() == flat.data_ptr() + start * t.element_size()
    return v


def guards_intact(v):
    flat, start, n = v.guard
    return bool((flat[:start] == SENTINEL).all()) and bool((flat[start + n:] == SENTINEL).all())


def poisoned(shape, dtype, k):
    return offset_view(torch.full(shape, float("nan"), dtype=dtype, device="cuda"), k)


def call_abi(name, sfx, offs=None, fwd=True, bwd=True, stream=None, tensors=None, call=None):
    """msda_forward_<sfx> / msda_backward_<sfx> through ctypes.  offs: argument name -> offset in elements of that tensor past a 256-byte
    boundary (inputs AND outputs; 0 where absent).  Outputs are caller-allocated offset views, poisoned with NaN.  Returns
    (return codes, outputs); ``tensors`` carries outputs over to a later call (a graph replay writes the captured addresses)."""
    offs = offs or {}
    call = call or SHAPES[name]
    t = device_inputs(name, sfx, call)
    N, S, M, D, L, Lq, P = call.N, call.S, call.M, call.D, call.L, call.Lq, call.P
    a = {k: (offset_view(t[k], offs[k]) if offs.get(k) else t[k]) for k in ("value", "loc", "aw", "grad_out")}
    out = tensors if tensors is not None else {}
    if not out:
        if fwd:
            out["out"] = poisoned((N, Lq, M * D), TORCH[sfx], offs.get("out", 0))
        if bwd:
            out["grad_value"] = poisoned((N, S, M, D), TORCH[sfx], offs.get("grad_value", 0))
            out["grad_loc"] = poisoned((N, Lq, M, L, P, 2), WORK[sfx], offs.get("grad_loc", 0))
            out["grad_aw"] = poisoned((N, Lq, M, L, P), WORK[sfx], offs.get("grad_aw", 0))
    out["_inputs"] = a      # (kept alive with the outputs: a captured graph holds their addresses)
    lib = _lib.load()
    sh, ls = t["host"]
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rcs = []
    if fwd:
        rcs.append(getattr(lib, "msda_forward_" + sfx)(
            a["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), a["loc"].data_ptr(), a["aw"].data_ptr(), N, S, M, D, L, Lq, P,
            64, out["out"].data_ptr(), sh.ctypes.data, ls.ctypes.data, s))
    if bwd:
        rcs.append(getattr(lib, "msda_backward_" + sfx)(
            a["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), a["loc"].data_ptr(), a["aw"].data_ptr(), a["grad_out"].data_ptr(),
            N, S, M, D, L, Lq, P, 64, out["grad_value"].data_ptr(), out["grad_loc"].data_ptr(), out["grad_aw"].data_ptr(), sh.ctypes.data,
            ls.ctypes.data, s))
    return rcs, out


def assert_written_inside(out, note=""):
    """every payload element finite, every guard element still the sentinel: catches a store wider than the chosen path allows (and the
    n4 overshoot of the bf16 rounding pass), and an element no kernel wrote"""
    for k, v in out.items():
        if k.startswith("_"):
            continue
        assert bool(torch.isfinite(v).all()), (note, k, "a payload element was not written")
        assert guards_intact(v), (note, k, "a guard element was overwritten")
    for k, v in out["_inputs"].items():
        if hasattr(v, "guard"):
            assert guards_intact(v), (note, k)


def run_checked(name, sfx, offs, fwd=True, bwd=True, note=""):
    """one forward and / or backward through the C ABI: return codes, profile records, guards, oracle.  Returns the records."""
    res = {}
    ran = _profiled_variants(lambda: res.update(zip(("rcs", "out"), call_abi(name, sfx, offs, fwd, bwd))))
    for rc in res["rcs"]:
        _lib.check(rc)
    assert_written_inside(res["out"], note)
    assert_matches(res["out"], name, sfx, note=note)
    return ran


# ---- the path the table fixes for a call -------------------------------------------------------------------------------------------------
def _row_aligned(sfx, offs, names):
    """are the tensors in `names` aligned to rows of four storage elements (16 B of f32, 8 B of bf16)?"""
    return all(offs.get(k, 0) % 4 == 0 for k in names)


def expected_fwd(name, sfx, offs):
    """rows "window forward eligible" and "split forward": fp32 compute only, value and out aligned to four storage elements, the plan ok
    (ENC; with the monitor off the automatic choice is the window kernel) / D = 32, four channels per lane, a small call (DEC)"""
    if sfx != "f64" and _row_aligned(sfx, offs, ("value", "out")):
        if name == "ENC":
            return [("fwd", 2)]
        if name == "DEC":
            return [("fwd", 3)]
    return [("fwd", 1)]


def expected_bwd(name, sfx, offs, variant=0):
    """rows "routed / band backward entered": fp32 compute only, bwd_variant 4 (or 0 with Lq == S; 5: band) and value / grad_out /
    grad_value aligned to four storage elements.  A refused attempt leaves NO record of its own: exactly one ("bwd", 1)."""
    asked = variant or (4 if name == "ENC" else 1)
    if sfx != "f64" and asked in (4, 5) and name in ("ENC", "DEC") and _row_aligned(sfx, offs, ("value", "grad_out", "grad_value")):
        return [("bwd", asked)]
    return [("bwd", 1)]


DATA_OFFSETS = {"f32": (1, 2), "bf16": (1, 2, 4), "f64": (1,)}      # elements; 0 is the aligned call every case list starts with
FWD_ARGS, BWD_ARGS = ("value", "loc", "aw", "out"), ("value", "loc", "aw", "grad_out", "grad_value", "grad_loc", "grad_aw")


def alone_cases(sfx):
    """each tensor alone at each of its offsets: data tensors at DATA_OFFSETS, loc / grad_loc by one (x, y) pair, aw / grad_aw by one element"""
    cases = [{}]
    for k in ("value", "grad_out", "out", "grad_value"):
        cases += [{k: o} for o in DATA_OFFSETS[sfx]]
    cases += [{"loc": 2}, {"grad_loc": 2}, {"aw": 1}, {"grad_aw": 1}]
    return cases


def together_cases(sfx):
    return [dict({k: o for k in ("value", "grad_out", "out", "grad_value")}, loc=2, grad_loc=2, aw=1, grad_aw=1) for o in DATA_OFFSETS[sfx]]


def test_preconditions():
    """With every pointer aligned the shapes take the paths the alignment cases are about to leave (f32 and bf16):
    ENC fwd_variant 2 -> window forward, bwd_variant 0 -> routed backward; DEC automatic -> split forward, direct (+ level-sum) backward;
    DEC bwd_variant 5 -> row-band backward."""
    for sfx in ("f32", "bf16"):
        _lib.set_option("fwd_variant", 2)
        _lib.set_option("bwd_variant", 0)
        assert run_checked("ENC", sfx, {}, bwd=False) == [("fwd", 2)], sfx
        assert run_checked("ENC", sfx, {}, fwd=False) == [("bwd", 4)], sfx
        _lib.set_option("fwd_variant", 0)
        assert run_checked("DEC", sfx, {}, bwd=False) == [("fwd", 3)], sfx
        assert run_checked("DEC", sfx, {}, fwd=False) == [("bwd", 1)], sfx
        _lib.set_option("bwd_variant", 5)
        assert run_checked("DEC", sfx, {}, fwd=False) == [("bwd", 5)], sfx
        _lib.set_option("bwd_variant", 0)
    for name in ("DEC", "ODD", "ODD7"):      # the level-sum kernel takes every level of these (the direct backward adds no grad_value)
        c = SHAPES[name]
        z = host_inputs(name)
        plan = _lib.levelsum_plan(c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, z["shapes"], z["lsi"])
        assert plan["levels_mask"] == (1 << c.L) - 1, (name, plan)


MATRIX = [(name, sfx, "auto") for name in ("ENC", "DEC", "ODD", "ODD7") for sfx in ("f32", "f64", "bf16")] + \
         [(name, sfx, "forced") for name in ("ENC", "DEC") for sfx in ("f32", "f64", "bf16")]


@pytest.mark.parametrize("name,sfx,mode", MATRIX)
def test_alignment_matrix(name, sfx, mode):
    """Each tensor alone at each of its offsets, then all together, through the C ABI: results against the oracle, guards intact, and the
    profile records the table fixes --
      * value or out below four storage elements: no window forward, no split forward, exactly one ("fwd", 1);
      * value, grad_out or grad_value below four storage elements (bf16: 8 bytes): no routed / band backward, exactly one ("bwd", 1) and no
        second record from the refused attempt;
      * loc / grad_loc at 8 bytes, aw / grad_aw at 4 bytes: the records of the aligned call (only the level-sum form changes);
      * the channels per lane follow D and the data pointers (ODD: D = 30 -> two at most, ODD7: D = 7 -> one; DEC / ENC: four, two, one).
    mode "forced": fwd_variant 2 + bwd_variant 4 on ENC; fwd_variant 3 on DEC, whose backward is asked for the row-band kernel (5)."""
    fv, bv = (0, 0) if mode == "auto" else {"ENC": (2, 4), "DEC": (3, 5)}[name]
    _lib.set_option("fwd_variant", fv)
    _lib.set_option("bwd_variant", bv)
    cases = alone_cases(sfx) + (together_cases(sfx) if mode == "auto" else [])
    for offs in cases:
        note = (name, sfx, mode, offs)
        if not offs or any(k in FWD_ARGS for k in offs):
            ran = run_checked(name, sfx, {k: o for k, o in offs.items() if k in FWD_ARGS}, bwd=False, note=note)
            assert ran == expected_fwd(name, sfx, offs), (note, ran)
        if not offs or any(k in BWD_ARGS for k in offs):
            ran = run_checked(name, sfx, {k: o for k, o in offs.items() if k in BWD_ARGS}, fwd=False, note=note)
            assert ran == expected_bwd(name, sfx, offs, bv), (note, ran)


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name", ["ENC", "DEC"])
def test_offset_views_through_the_python_shim(name, sfx):
    """MultiScaleDeformableAttention.py passes data_ptr() through unchanged: a contiguous view with a storage offset -- value, then
    sampling_loc by one (x, y) pair -- reaches the fallback branches straight through ms_deform_attn_forward / _backward, and (f32, bf16)
    through MSDeformAttnFunction.apply."""
    t = device_inputs(name, sfx)
    for offs in ({"value": 1}, {"loc": 2}):
        a = {k: (offset_view(t[k], offs[k]) if k in offs else t[k]) for k in ("value", "loc", "aw", "grad_out")}
        got = {}
        ran = _profiled_variants(lambda: got.update(out=MSDA.ms_deform_attn_forward(a["value"], t["shapes"], t["lsi"], a["loc"], a["aw"], 64)))
        assert ran == expected_fwd(name, sfx, offs), (offs, ran)
        ran = _profiled_variants(lambda: got.update(zip(("grad_value", "grad_loc", "grad_aw"), MSDA.ms_deform_attn_backward(
            a["value"], t["shapes"], t["lsi"], a["loc"], a["aw"], a["grad_out"], 64))))
        assert ran == expected_bwd(name, sfx, offs), (offs, ran)
        assert_matches(got, name, sfx, note=("shim", offs))
        assert all(guards_intact(v) for v in a.values() if hasattr(v, "guard"))
        if sfx == "f64":
            continue
        v, loc, aw = (a[k].detach().requires_grad_(True) for k in ("value", "loc", "aw"))
        assert v.data_ptr() == a["value"].data_ptr() and loc.data_ptr() == a["loc"].data_ptr()
        out = MSDeformAttnFunction.apply(v, t["shapes"], t["lsi"], loc, aw, 64)
        out.backward(t["grad_out"])
        assert_matches(dict(out=out.detach(), grad_value=v.grad, grad_loc=loc.grad, grad_aw=aw.grad), name, sfx, note=("apply", offs))


# ---- bf16 on the paths it takes in training ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ENC", "DEC"])
def test_bf16_automatic_mode_against_oracle(name):
    """fwd_variant 0 / bwd_variant 0 in bf16 storage -- the training configuration -- through the shim: ENC takes the window forward and the
    routed backward, DEC the split forward and the level-sum + split backward; test_gpu_bf16.check's one-ulp criterion against the oracle."""
    t = device_inputs(name, "bf16")
    got = {}
    ran = _profiled_variants(lambda: got.update(out=MSDA.ms_deform_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], 64)))
    assert ran == expected_fwd(name, "bf16", {}), ran
    ran = _profiled_variants(lambda: got.update(zip(("grad_value", "grad_loc", "grad_aw"), MSDA.ms_deform_attn_backward(
        t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 64))))
    assert ran == expected_bwd(name, "bf16", {}), ran
    assert got["out"].dtype == torch.bfloat16 and got["grad_value"].dtype == torch.bfloat16 and got["grad_loc"].dtype == torch.float32
    B.check((got["out"], got["grad_value"], got["grad_loc"], got["grad_aw"]), oracle(name, "bf16"))


def _split_call(L, P):
    """a decoder-shaped problem of test_split_kernels_against_oracle_and_the_eight_lane_kernels' kind: D = 32, L * P a multiple of four"""
    shapes = [(9, 7), (3, 2), (1, 1), (17, 5)][:L]
    return W.Call(f"split{L}x{P}", 2, 3, 32, P, shapes, 37, False)


@pytest.mark.parametrize("which", ["DEC", (2, 6), (4, 4)])
def test_bf16_split_forward_against_oracle(which):
    """The bf16 split forward -- the default decoder forward -- forced (fwd_variant 3) and compared with the ORACLE under the one-ulp criterion
    (elsewhere it is only compared with the 8-lane kernel, at 2e-2): DEC, (L, P) = (2, 6) for the run-time point count and (4, 4) for the
    PPG = 4 instance.  The backward of the same call (level-sum + split backward) rides along."""
    name, call = (which, None) if which == "DEC" else (f"split{which[0]}x{which[1]}", _split_call(*which))
    _lib.set_option("fwd_variant", 3)
    res = {}
    ran = _profiled_variants(lambda: res.update(zip(("rcs", "out"), call_abi(name, "bf16", {}, call=call))))
    assert res["rcs"] == [0, 0], _lib.last_error()
    assert ran == [("fwd", 3), ("bwd", 1)], ran
    assert_written_inside(res["out"])
    o = res["out"]
    want = oracle(name, "bf16", call)
    B.check((o["out"], o["grad_value"], o["grad_loc"], o["grad_aw"]), want)
    assert B.ulp_share(o["out"], want[0]) < 1e-3


def test_levelsum_takes_a_subset_of_levels():
    """Row "level-sum backward": a level too large for the LDS windows stays with the direct kernel's atomics.  f32: the level-sum kernel
    takes the other level (a subset), the rest is added into the zero-filled grad_value; bf16: all levels or none -- here none: fp32
    scratch + zero-fill + direct kernel + one rounding pass.  Poisoned outputs, guards, oracle."""
    call = W.Call("part", 1, 1, 32, 4, [(300, 300), (9, 9)], 64, False)
    z = host_inputs("part", call)
    plan = _lib.levelsum_plan(call.N, call.S, call.M, call.D, call.L, call.Lq, call.P, z["shapes"], z["lsi"])
    assert plan["levels_mask"] == 2, plan
    # (grad_value one element past the boundary: in bf16 the rounding pass then has no 8-byte rows and rounds element by element)
    for sfx, offs in (("f32", {}), ("bf16", {}), ("f32", {"grad_value": 1}), ("bf16", {"grad_value": 1})):
        res = {}
        ran = _profiled_variants(lambda: res.update(zip(("rcs", "out"), call_abi("part", sfx, offs, fwd=False, call=call))))
        assert res["rcs"] == [0], _lib.last_error()
        assert ran == [("bwd", 1)], ran
        assert_written_inside(res["out"], (sfx, offs))
        assert_matches(res["out"], "part", sfx, note=(sfx, offs), call=call)


# ---- level-table limit ------------------------------------------------------------------------------------------------------------------
def _levels_call(L):
    return W.Call(f"L{L}", 1, 1, 32, 1, [(1, 1)] * L, 9, False)


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_level_table_limit(sfx):
    """Row '"too many levels"': the level table (16 bytes per level) and the point records of a block share 64 KB of LDS.  512 one-pixel
    levels work and match the oracle (no other test has a level table of hundreds of entries in LDS); 4096 levels are refused by both entry
    points with MSDA_ERR_BAD_DIMS and "too many levels (L=4096)".  The text is the same for all three storage types: the " (bf16)" tag of the
    table's "error texts" row goes on the runtime's (HIP) errors, not on this argument refusal -- and whether the forward looks at the
    limit before or after it considers the split kernel cannot be told apart from outside (a call the split kernel takes has L <= 32)."""
    name, call = "L512", _levels_call(512)
    res = {}
    ran = _profiled_variants(lambda: res.update(zip(("rcs", "out"), call_abi(name, sfx, {}, call=call))))
    assert res["rcs"] == [0, 0], _lib.last_error()
    assert ran == [("fwd", 1), ("bwd", 1)], ran
    assert_written_inside(res["out"])
    assert_matches(res["out"], name, sfx, call=call)
    # 4096 levels: refused before any kernel is launched (the inputs need no oracle: nothing is computed)
    call = _levels_call(4096)
    t = W.make_inputs(call, "uniform", seed=1)
    _device[(call.name, sfx)] = dict(
        {k: dev(t[k].numpy()) for k in ("shapes", "lsi")}, value=t["value"].to(TORCH[sfx]).cuda(), grad_out=t["grad_out"].to(TORCH[sfx]).cuda(),
        loc=t["loc"].to(WORK[sfx]).cuda(), aw=t["aw"].to(WORK[sfx]).cuda(), host=(t["shapes"].numpy(), t["lsi"].numpy()))
    try:
        for fwd in (True, False):
            rcs, _ = call_abi(call.name, sfx, {}, fwd=fwd, bwd=not fwd, call=call)
            assert rcs == [-2], (fwd, rcs)      # MSDA_ERR_BAD_DIMS
            assert _lib.last_error() == "too many levels (L=4096) for the level table in LDS", _lib.last_error()
        torch.cuda.synchronize()
    finally:
        del _device[(call.name, sfx)]


# ---- bf16 scratch and stream capture ----------------------------------------------------------------------------------------------------
def test_bf16_scratch_and_stream_capture():
    """Row "no scratch during stream capture" (and "level-sum backward", bf16): the fp32 scratch image of grad_value is kept per (device,
    stream) and never allocated while the stream is being captured.  On a stream that has run nothing (a high-priority stream: no other
    test of the suite is handed one from that pool), single stream, no parallel branches:
      0. ODD with the default options needs no scratch -- the level-sum kernel takes every level --: its capture succeeds at once;
      1. with bwd_levelsum = 0 the direct kernel adds into the scratch: the captured call is refused with MSDA_ERR_BAD_DIMS and
         "... outside the capture" (through ctypes: the return code is recorded and the capture ended normally);
      2. the same call run eagerly on that stream matches the oracle (and allocates the scratch);
      3. captured again it succeeds, and a replay matches the oracle."""
    name, sfx = "ODD", "bf16"
    rcs, out = call_abi(name, sfx, {}, fwd=False)      # default stream: the kernels' LDS limits are granted outside any capture
    assert rcs == [0], _lib.last_error()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(priority=-1)
    marker = torch.zeros(4, device="cuda")

    def captured(tensors):
        def body():
            marker.add_(1.0)      # (the graph is never empty, whatever the library call does)
            rcs, _ = call_abi(name, sfx, {}, fwd=False, stream=side.cuda_stream, tensors=tensors)
            return rcs, _lib.last_error()
        graph, (rcs, text) = capture(body, side)
        return graph, rcs, text

    def fresh():
        return call_abi_outputs_only(name, sfx)

    def replay_matches(graph, tensors, note):
        for k in ("grad_value", "grad_loc", "grad_aw"):
            tensors[k].fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_written_inside(tensors, note)
        assert_matches(tensors, name, sfx, note=note)

    # 0. default options: no scratch needed
    t0 = fresh()
    graph, rcs, text = captured(t0)
    assert rcs == [0], text
    replay_matches(graph, t0, "default options, captured on a fresh stream")
    # 1. the direct kernel has to add grad_value: refused during the capture
    _lib.set_option("bwd_levelsum", 0)
    t1 = fresh()
    graph1, rcs, text = captured(t1)
    assert rcs == [-2], (rcs, text)      # MSDA_ERR_BAD_DIMS
    assert "needs an fp32 scratch buffer" in text and "outside the capture" in text, text
    # 2. eagerly on that stream
    t2 = fresh()
    with torch.cuda.stream(side):
        rcs, _ = call_abi(name, sfx, {}, fwd=False, stream=side.cuda_stream, tensors=t2)
    side.synchronize()
    assert rcs == [0], _lib.last_error()
    assert_written_inside(t2, "eager")
    assert_matches(t2, name, sfx, note="eager on the side stream")
    # 3. captured again
    t3 = fresh()
    graph3, rcs, text = captured(t3)
    assert rcs == [0], text
    replay_matches(graph3, t3, "captured after the eager call")
    del graph, graph1, graph3


def call_abi_outputs_only(name, sfx):
    """poisoned, guarded backward outputs for a later call_abi(..., tensors=...)"""
    c = SHAPES[name]
    return dict(grad_value=poisoned((c.N, c.S, c.M, c.D), TORCH[sfx], 0), grad_loc=poisoned((c.N, c.Lq, c.M, c.L, c.P, 2), WORK[sfx], 0),
                grad_aw=poisoned((c.N, c.Lq, c.M, c.L, c.P), WORK[sfx], 0))


# ---- bwd_direct_cpl ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sfx", [("DEC", "f32"), ("ODD", "f32"), ("DEC", "bf16")])
def test_bwd_direct_cpl(name, sfx):
    """Rows "bwd_direct_cpl option" and "direct backward adds grad_value": with bwd_variant 1 and bwd_levelsum 0 the direct kernel adds
    grad_value itself (f32: into the zero-filled grad_value; bf16: into the fp32 scratch, rounded once).  f32 honours 1, 2 and 4 channels per
    lane (ODD, D = 30: 4 is clamped to the 2 that D allows); bf16 ignores the option.  Every value against the oracle."""
    _lib.set_option("bwd_variant", 1)
    _lib.set_option("bwd_levelsum", 0)
    for cpl in (1, 2, 4):
        _lib.set_option("bwd_direct_cpl", cpl)
        assert run_checked(name, sfx, {}, fwd=False, note=(name, sfx, cpl)) == [("bwd", 1)]
    # the option takes whatever the pointers allow, too: grad_value is added element by element at any alignment
    _lib.set_option("bwd_direct_cpl", 4)
    off = {"grad_value": 1, "grad_out": 1}
    assert run_checked(name, sfx, off, fwd=False, note=(name, sfx, "cpl 4, offset")) == [("bwd", 1)]


# ---- fused prep entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Lq", [273, 380])
def test_fused_prep_entry_with_offset_views(dtype, Lq):
    """msda_forward_prep_* (case (ref_dim = 4, L = 4, P = 4) of test_fused_prep_gather_equals_the_two_kernel_form) with value, and separately
    the raw projection (offsets), one element past a 256-byte boundary, against the two-kernel form on aligned copies with that test's
    tolerance.  Lq = 273, decoder-shaped (fwd_prep_fused 1): one kernel, ("fwd", 5), narrower channels per lane for the offset value.
    Lq = 380 = S, encoder-shaped (fwd_prep_fused 2): the fused window kernel ("fwd", 6) wants rows of four for value / out and (x, y) pairs
    for the offsets (rows_ok); either view sends the call to the two-kernel form -- location / softmax kernel, then msda_forward_*, which for
    the offset value is the direct kernel ("fwd", 1) and for the offset projection still the window kernel ("fwd", 2)."""
    N, M, D, L, P, ref_dim = 2, 8, 32, 4, 4, 4
    shapes = torch.tensor([(13, 21), (7, 11), (4, 6), (2, 3)], dtype=torch.int64, device="cuda")
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    S = int(shapes.prod(1).sum())
    g = torch.Generator(device="cuda").manual_seed(100 * L + 10 * P + ref_dim)
    value = torch.randn(N, S, M, D, device="cuda", generator=g).to(dtype)
    qproj = (torch.randn(N, Lq, M * L * P * 3, device="cuda", generator=g) * 1.5).to(dtype)
    ref = torch.rand(N, Lq, L, ref_dim, device="cuda", generator=g) * 0.8 + 0.1
    encoder = Lq == S
    fused_mode = 2 if encoder else 1

    def run(v, q, mode):
        _lib.set_option("fwd_prep_fused", mode)
        got = []
        ran = _profiled_variants(lambda: got.append(MSDeformAttnFusedFunction.apply(v, shapes, lsi, q, ref, M, L, P, 64)))
        return got[0].double(), ran

    base, ran = run(value, qproj, 0)
    assert ran == [("fwd", 2 if encoder else 3)], ran      # the two-kernel form: location / softmax kernel + window / split forward
    fused, ran = run(value, qproj, fused_mode)
    assert ran == [("fwd", 6 if encoder else 5)], ran
    tol = {torch.float32: 2e-6, torch.bfloat16: 1e-2}[dtype]
    scale = float(base.abs().max()) + 1e-30
    assert float((fused - base).abs().max()) <= tol * scale
    v1, q1 = offset_view(value, 1), offset_view(qproj, 1)
    for v, q, want in ((v1, qproj, ("fwd", 1 if encoder else 5)), (value, q1, ("fwd", 2 if encoder else 5))):
        out, ran = run(v, q, fused_mode)
        assert ran == [want], ran
        assert float((out - base).abs().max()) <= tol * scale, float((out - base).abs().max()) / scale
    assert guards_intact(v1) and guards_intact(q1)
