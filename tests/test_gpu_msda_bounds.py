"""GPU (-m gpu): every MSDeformAttn kernel -- direct, LDS-window and split forward; direct backward with its level-sum and split helpers;
routed and row-band backward -- held ELEMENT BY ELEMENT to the float64 restatement of tests/msda_ref.py:

    |kernel - reference| / bound < 1        for every element of out, grad_value, grad_sampling_loc and grad_attn_weight

(f64: < 2, because the float64 reference itself rounds under the same bound; nothing else is multiplied), with the bound derived in
msda_ref's docstring from the roundings on the path to each element, the location error of each sampling point and, for bf16 storage, the
one rounding at the store.  Where the bound is zero -- dropped samples, pixels nobody touched -- exactly zero is asked for.  The
whole-tensor criteria of test_gpu_parity.py / test_gpu_bf16.py let an error of 1.6 % in a whole pyramid level pass (tests/test_msda_ref.py
holds that on the CPU); these bounds put it thousands of bounds outside.

Every call goes through MultiScaleDeformableAttention.ms_deform_attn_forward / _backward and its profile record is asserted: a silent
fallback to the direct kernel cannot pass for the row it replaced.  Inputs (msda_ref.make_inputs): level l scaled by 2^-4l, grad_out by
2^-k per query, dropped samples, border corners, points outside [0, 1]^2.  References once per (shape, dtype), shared with
tests/test_msda_ref.py.

Then the exact probes (msda_ref.exact_probe: every intermediate is a float32 number -- a bf16 one where bf16 is stored): all four outputs
BIT-EQUAL to the float64 reference on every row the probe shape meets the preconditions of, at every quarter-pixel position from -1.25 to
H + 0.25 -- the drop test at exactly -1 and H, the inside test of each corner at 0 and H - 1, grad_loc's convention on a pixel boundary.
And the committed golden cases' inputs through the same element-wise check.

Measured worst ratios per row: profiles/r23_msda_bounds.md."""
import os

import numpy as np
import pytest
import torch

from richsem_amd import _lib
from richsem_amd import MultiScaleDeformableAttention as MSDA

import msda_ref as R
from conftest import GOLDEN
from test_gpu_dispatch import TORCH, WORK
from test_gpu_parity import _profiled_variants, dev
from test_msda_ref import CALLS, PROBES, case

pytestmark = pytest.mark.gpu

LIMIT = {"f32": 1.0, "bf16": 1.0, "f64": 2.0}      # f64: the float64 reference rounds under the same bound as the kernel
_OPTIONS = ("fwd_variant", "bwd_variant", "bwd_levelsum", "bwd_direct_cpl", "bwd_split", "locality_monitor", "tile_margin", "tile_grow",
            "rps_tile", "rps_max_chunks", "rps_seg_shift", "band_hits")
BWD = ("grad_value", "grad_loc", "grad_aw")


@pytest.fixture(autouse=True)
def _options():
    """locality_monitor = 0: the forward asked for is the forward that runs, whatever earlier tests left in the monitor's table; every
    option a test touches is put back"""
    saved = {k: _lib.get_option(k) for k in _OPTIONS}
    _lib.set_option("locality_monitor", 0)
    yield
    for k, v in saved.items():
        _lib.set_option(k, v)


_device = {}


def tensors(key, t, sfx):
    """device tensors of typed inputs (float64 numpy copies of what the kernel is given), once per key"""
    if (key, sfx) not in _device:
        d = {k: dev(t[k]) for k in ("shapes", "lsi")}
        d["value"], d["grad_out"] = dev(t["value"]).to(TORCH[sfx]), dev(t["grad_out"]).to(TORCH[sfx])
        d["loc"], d["aw"] = dev(t["loc"]).to(WORK[sfx]), dev(t["aw"]).to(WORK[sfx])
        for k in ("value", "grad_out", "loc", "aw"):      # the conversion is exact: the reference saw the same numbers
            assert np.array_equal(d[k].double().cpu().numpy(), t[k]), k
        _device[(key, sfx)] = d
    return _device[(key, sfx)]


def forward(d, opts, record):
    for k, v in opts.items():
        _lib.set_option(k, v)
    got = {}
    ran = _profiled_variants(lambda: got.update(out=MSDA.ms_deform_attn_forward(d["value"], d["shapes"], d["lsi"], d["loc"], d["aw"], 64)))
    assert ran == [("fwd", record)], (opts, ran)
    return got


def backward(d, opts, record):
    for k, v in opts.items():
        _lib.set_option(k, v)
    got = {}
    ran = _profiled_variants(lambda: got.update(zip(BWD, MSDA.ms_deform_attn_backward(
        d["value"], d["shapes"], d["lsi"], d["loc"], d["aw"], d["grad_out"], 64))))
    if record is not None:
        assert ran == [("bwd", record)], (opts, ran)
    return got


def inside(got, ref, bnd, sfx, note):
    w = R.worst(got, ref, bnd)
    print("ratio", note, sfx, {k: f"{v:.3f}" for k, v in w.items()})
    bad = {k: (v, np.unravel_index(R.ratios(got[k], ref[k], bnd[k])[1], ref[k].shape)) for k, v in w.items() if not v < LIMIT[sfx]}
    assert not bad, (note, sfx, bad)
    if sfx == "bf16":      # the stored number lies between the bf16 roundings of ref -+ the bound of the fp32 sum (msda_ref.stored_interval)
        for k in ("out", "grad_value"):
            if k in got:
                assert R.outside_interval(got[k], ref[k], bnd[k + "_sum"]) == 0, (note, k)


def bit_equal(got, ref, note):
    for k, a in got.items():
        a = a.double().cpu().numpy().reshape(ref[k].shape)      # (bf16: the one exact conversion)
        ne = a != ref[k]
        assert not ne.any(), (note, k, int(ne.sum()), np.argwhere(ne)[:4].tolist())


def plan_of(name):
    c = CALLS[name]
    z = case(name, "f32")[0]
    return c, (c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, z["shapes"], z["lsi"])


# ---- forward rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name", list(CALLS))
def test_direct_forward(name, sfx):
    t, ref, bnd = case(name, sfx)
    inside(forward(tensors(name, t, sfx), {"fwd_variant": 1}, 1), ref, bnd, sfx, ("direct forward", name))


# tile_margin 1 with tile_grow 0: every window is its region's footprint + 1 pixel (default: 6, grown into spare LDS), while the init
# pattern puts point k of a head k = 1..4 pixels from its query (+ 1 px of jitter) and an eighth of the points anywhere in
# [-0.15, 1.15]^2: most points of k >= 2 miss their window and take the kernel's global path.  (msda_tiled_plan reports the margin.)
WINDOW_OPTS = [{}, {"tile_margin": 1, "tile_grow": 0}]


@pytest.mark.parametrize("opts", WINDOW_OPTS, ids=["default", "margin1"])
@pytest.mark.parametrize("sfx", ["f32", "bf16"])
def test_window_forward(sfx, opts):
    t, ref, bnd = case("ENC", sfx)
    for k, v in opts.items():
        _lib.set_option(k, v)
    plan = _lib.tiled_plan(*plan_of("ENC")[1])
    assert plan["applicable"] == 1 and plan["margin"] == opts.get("tile_margin", 6), plan
    inside(forward(tensors("ENC", t, sfx), dict(opts, fwd_variant=2), 2), ref, bnd, sfx, ("window forward", tuple(opts.items())))


@pytest.mark.parametrize("sfx", ["f32", "bf16"])
def test_split_forward(sfx):
    t, ref, bnd = case("DEC", sfx)
    inside(forward(tensors("DEC", t, sfx), {"fwd_variant": 3}, 3), ref, bnd, sfx, ("split forward", "DEC"))


# ---- backward rows ------------------------------------------------------------------------------------------------------------------
def direct_backward_options(name, sfx):
    """bwd_variant 1 with: the level-sum kernel on (it takes every level of ENC / DEC / ODD / ODD7 and none of SCR: msda_levelsum_plan) and
    the split kernel for grad_loc / grad_aw on or off (D = 32 only; elsewhere the 8-lane kernel either way); the level-sum kernel off:
    the direct kernel adds grad_value itself (bf16: into the fp32 scratch) with 1, 2, 4 channels per lane where D and the type allow
    (f64: 16 bytes = 2 channels; bf16 ignores the option)"""
    o = [{"bwd_levelsum": 1, "bwd_split": 1}, {"bwd_levelsum": 1, "bwd_split": 0}]
    if sfx == "bf16":
        return o + [{"bwd_levelsum": 0}]
    D = CALLS[name].D
    cpls = [c for c in (1, 2, 4) if D % c == 0 and c * (8 if sfx == "f64" else 4) <= 16]
    return o + [{"bwd_levelsum": 0, "bwd_direct_cpl": c} for c in cpls]


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name", list(CALLS))
def test_direct_backward(name, sfx):
    t, ref, bnd = case(name, sfx)
    c, args = plan_of(name)
    assert _lib.levelsum_plan(*args)["levels_mask"] == (0 if name == "SCR" else (1 << c.L) - 1)
    d = tensors(name, t, sfx)
    for opts in direct_backward_options(name, sfx):
        inside(backward(d, dict(opts, bwd_variant=1), 1), ref, bnd, sfx, ("direct backward", name, tuple(opts.items())))
        _lib.set_option("bwd_direct_cpl", 0)


# rps_tile 4: tiles of at most 3 x 3 pixels (plan_rps: tmax = tile - 1) -- 126 + 28 + 8 + 2 tiles per (image, head) of ENC, nearly every
# point's corners cross a tile edge (the apron sums, flushed with row atomics onto the neighbours' first row / column).
# rps_max_chunks 1: a tile expected to fill more than one chunk of 1536 points is dealt over slabs -- level 3 (3 x 5): 1377 * 4 / 15 points
# per pixel * 9 pixels * 1.05 / 1536 -> 3 chunks -> 3 slabs, three workgroups adding their rows with atomics into the pre-zeroed level.
# rps_seg_shift 3: a pixel's list is walked in units of 8 points (the smallest; level 3 has ~370 points per pixel: ~46 units per list).
# 126 + 28 + 8 + 2 * 3 = 168 work items <= kRpsMaxUnits: the plan applies -- the record says so.
ROUTED_OPTS = [{}, {"rps_tile": 4, "rps_max_chunks": 1, "rps_seg_shift": 3}]


@pytest.mark.parametrize("opts", ROUTED_OPTS, ids=["default", "tile4"])
@pytest.mark.parametrize("sfx", ["f32", "bf16"])
def test_routed_backward(sfx, opts):
    t, ref, bnd = case("ENC", sfx)
    inside(backward(tensors("ENC", t, sfx), dict(opts, bwd_variant=4), 4), ref, bnd, sfx, ("routed backward", tuple(opts.items())))


# band_hits 32 (the smallest): DEC has 68 * 4 = 272 points per (image, head); plan_band expects 272 * (rows + 1) / (H + 1) hits per band
# -- 63 on level 0 (5 bands of 5 rows), 146 on level 1, 272 on levels 2 and 3 -- and deals a band over ceil(hits / 32) = 2, 5, 9, 9 query
# slabs: every level is then pre-zeroed and added to with row atomics (bf16: through the fp32 scratch).  Default 400: no slabs at all.
BAND_OPTS = [{}, {"band_hits": 32}]


@pytest.mark.parametrize("opts", BAND_OPTS, ids=["default", "hits32"])
@pytest.mark.parametrize("sfx", ["f32", "bf16"])
def test_band_backward(sfx, opts):
    t, ref, bnd = case("DEC", sfx)
    inside(backward(tensors("DEC", t, sfx), dict(opts, bwd_variant=5), 5), ref, bnd, sfx, ("row-band backward", tuple(opts.items())))


# ---- exact probes -------------------------------------------------------------------------------------------------------------------
_probe = {}


def probe(which, sfx):
    """inputs and float64 reference of an exact probe; bf16: the variant whose results are bf16 numbers (tests/test_msda_ref.py)"""
    key = (which, sfx == "bf16")
    if key not in _probe:
        z = R.exact_probe(per_query_go=sfx != "bf16", **PROBES[which])
        t = R.typed(z, "f32")
        _probe[key] = (t, R.evaluate(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"]))
    return _probe[key]


# encoder-shaped probe (Lq == S, D = 32): direct, window and split forward; direct (level-sum + split, level-sum + 8-lane, atomics at
# every width) and routed backward (defaults, and 3 x 3 tiles with slabs).  Decoder-shaped: direct and split forward; direct and row-band
# backward (defaults, and every band slabbed).  f64: the direct rows.
PROBE_FWD = {
    "enc": [({"fwd_variant": 1}, 1), ({"fwd_variant": 2}, 2), ({"fwd_variant": 2, "tile_margin": 0, "tile_grow": 0}, 2), ({"fwd_variant": 3}, 3)],
    "dec": [({"fwd_variant": 1}, 1), ({"fwd_variant": 3}, 3)],
}
_DIRECT = [{"bwd_levelsum": 1, "bwd_split": 1}, {"bwd_levelsum": 1, "bwd_split": 0}, {"bwd_levelsum": 0, "bwd_direct_cpl": 1},
           {"bwd_levelsum": 0, "bwd_direct_cpl": 2}, {"bwd_levelsum": 0, "bwd_direct_cpl": 4}]
PROBE_BWD = {
    "enc": [(dict(o, bwd_variant=1), 1) for o in _DIRECT] + [(dict(o, bwd_variant=4), 4) for o in ROUTED_OPTS],
    "dec": [(dict(o, bwd_variant=1), 1) for o in _DIRECT] + [(dict(o, bwd_variant=5), 5) for o in BAND_OPTS],
}


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("which", list(PROBES))
def test_exact_probe_bit_equal(which, sfx):
    t, ref = probe(which, sfx)
    d = tensors(("probe", which, sfx == "bf16"), t, sfx)
    for opts, record in PROBE_FWD[which]:
        if sfx == "f64" and record != 1:
            continue
        bit_equal(forward(d, opts, record), ref, (which, sfx, opts))
    for opts, record in PROBE_BWD[which]:
        if sfx == "f64" and (record != 1 or opts.get("bwd_direct_cpl") == 4):
            continue
        bit_equal(backward(d, opts, record), ref, (which, sfx, opts))
        _lib.set_option("bwd_direct_cpl", 0)


# ---- the committed golden cases' inputs -------------------------------------------------------------------------------------------------
GOLDEN_CASES = ["pyramid_encoder_f32", "decoder_n2m8_f64", "ref_test_grad_D32", "ref_test_grad_D30", "border_bands_grad"]
_golden = {}


def golden(name, sfx):
    if (name, sfx) not in _golden:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        if sfx != "f64":
            for k in ("value", "loc", "aw", "grad_out"):
                z[k] = z[k].astype(np.float32)
        t = R.typed(z, sfx) if sfx != "f64" else {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in z.items()}
        # the first-order location term needs floor() to decide alike in the kernel and in float64: these inputs are not nudged, so hold
        # their distance from a pixel boundary (d_h <= 3 u x 21 pixels < 2^-18 at these sizes) instead
        assert R.boundary_distance(t["loc"], t["shapes"]) > 2.0 ** -17
        _golden[(name, sfx)] = (t,) + R.reference(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], sfx)
    return _golden[(name, sfx)]


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_golden_inputs(name, sfx):
    """inputs only (the golden OUTPUTS are test_gpu_parity's business): variants as test_gpu_bf16.test_bf16_golden_inputs -- direct;
    window forward + routed backward; direct forward + routed backward -- each where the case's shape allows it, else what the dispatch
    falls back to (no record is asserted here: the rows above do that).  Exact-border samples follow the kernel convention, which the
    restatement shares with the oracle."""
    t, ref, bnd = golden(name, sfx)
    d = tensors(("golden", name), t, sfx)
    for fv, bv in ((1, 1),) if sfx == "f64" else ((1, 1), (2, 4), (1, 4)):
        _lib.set_option("fwd_variant", fv)
        _lib.set_option("bwd_variant", bv)
        got = {"out": MSDA.ms_deform_attn_forward(d["value"], d["shapes"], d["lsi"], d["loc"], d["aw"], 64)}
        got.update(backward(d, {}, None))
        inside(got, ref, bnd, sfx, ("golden", name, fv, bv))
