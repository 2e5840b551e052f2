"""CPU: the comparator of tests/test_gpu_msda_bounds.py (tests/msda_ref.py) is right, tight and sharp --
  * the float32 evaluation of the restatement and the float32 C oracle stay inside the element-wise bounds on all four outputs, at the
    shapes the GPU tests use (worst ratio < 1; bf16: after one rounding of out / grad_value; f64: the oracle in f64 within 2 x the bound,
    because the float64 reference itself rounds under the same bound);
  * every wrong variant (msda_ref.MUTANTS) lands more than 10 bounds outside on at least one output, and at least three of them PASS the
    suite's older whole-tensor criteria (test_gpu_parity.rel_err / tols, test_gpu_bf16.check) on every output: the record that those
    criteria are blind to an error in a whole pyramid level;
  * on the exact probes float32 equals float64 bit for bit (restatement and C oracle), and the bf16 probe's results are bf16 numbers;
  * the input recipe leaves no sampling position within 2^-10 of a pixel boundary;
  * the bounds are not trivial: the median of bound / |reference| is below 1e-3 (f32) on every output."""
import numpy as np
import pytest
import torch

from oracle import msda_oracle as O
from richsem_amd import workload as W

import msda_ref as R

SEED = 41


def calls():
    """the shapes of tests/test_gpu_msda_bounds.py: test_gpu_dispatch.SHAPES and the fp32-scratch shape of
    test_gpu_bf16.test_bf16_odd_shapes (one level larger than the LDS windows, D = 3)"""
    from test_gpu_dispatch import SHAPES
    return dict(SHAPES, SCR=W.Call("scr", 1, 1, 3, 2, [(301, 301)], 50, False))


CALLS = calls()
_cache = {}


def case(name, sfx):
    """(typed inputs, reference values, bounds), once per (shape, storage type)"""
    if (name, sfx) not in _cache:
        if ("z", name) not in _cache:
            _cache[("z", name)] = R.make_inputs(CALLS[name], SEED)
        t = R.typed(_cache[("z", name)], sfx)
        ref, bnd = R.reference(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], sfx)
        _cache[(name, sfx)] = (t, ref, bnd)
    return _cache[(name, sfx)]


def _args(t):
    return t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"]


def _oracle(t, dtype):
    a = [np.asarray(x, dtype=dtype) for x in (t["value"], t["loc"], t["aw"], t["grad_out"])]
    out = O.forward(a[0], t["shapes"], t["lsi"], a[1], a[2])
    gv, gl, ga = O.backward(a[0], t["shapes"], t["lsi"], a[1], a[2], a[3])
    return dict(out=out, grad_value=gv, grad_loc=gl, grad_aw=ga)


def _stored_bf16(res):
    """out / grad_value rounded to bf16 once, as the bf16 kernels store them"""
    r = dict(res)
    for k in ("out", "grad_value"):
        r[k] = torch.from_numpy(np.ascontiguousarray(res[k])).float().to(torch.bfloat16).double().numpy()
    return r


def test_unit_roundoff_of_a_bf16_store():
    """why the storage term is 2^-8 and not 2^-9: a correctly rounded bf16 store is off by up to 2^-8 / (1 + 2^-8) of the number"""
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=torch.float64)
    err = float((x.float().to(torch.bfloat16).double() - x).abs() / x)
    assert 2.0 ** -9 < err < R.U_BF16


@pytest.mark.parametrize("sfx", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CALLS))
def test_float32_evaluation_and_oracle_stay_inside_the_bounds(name, sfx):
    t, ref, bnd = case(name, sfx)
    store = _stored_bf16 if sfx == "bf16" else (lambda r: r)
    f32 = store(R.evaluate(*_args(t), dtype=torch.float32))
    w = R.worst(f32, ref, bnd)
    print(name, sfx, "float32 restatement", w)
    assert max(w.values()) < 1, w
    orc = store(_oracle(t, np.float32))
    w = R.worst(orc, ref, bnd)
    print(name, sfx, "float32 oracle", w)
    assert max(w.values()) < 1, w
    if sfx == "bf16":      # the sharper form of the storage term: between the roundings of ref -+ the fp32 sum's bound
        for k in ("out", "grad_value"):
            assert R.outside_interval(f32[k], ref[k], bnd[k + "_sum"]) == 0, k
            assert R.outside_interval(orc[k], ref[k], bnd[k + "_sum"]) == 0, k
            # ... which the forward's coarsest-level error does not survive, small as it is beside one bf16 rounding
        bad = store(R.evaluate(*_args(t), dtype=torch.float64, mutant="fwd_aw_coarse"))
        assert R.outside_interval(bad["out"], ref["out"], bnd["out_sum"]) > 0 or name == "SCR"


@pytest.mark.parametrize("name", list(CALLS))
def test_float64_oracle_stays_inside_twice_the_bounds(name):
    """2 x: the float64 reference rounds under the same bound as the float64 code under test.  Nothing else is multiplied."""
    t, ref, bnd = case(name, "f64")
    w = R.worst(_oracle(t, np.float64), ref, bnd)
    print(name, "float64 oracle", w)
    assert max(w.values()) < 2, w


def _old_metric_passes(name, sfx, got, ref):
    """today's whole-tensor criteria, unchanged: test_gpu_parity.rel_err / tols (f32), test_gpu_bf16.check (bf16)"""
    import test_gpu_bf16 as B
    from test_gpu_parity import rel_err, tols
    if sfx == "bf16":
        tt = lambda k, dt: torch.from_numpy(np.ascontiguousarray(got[k])).float().to(dt)
        try:
            B.check((tt("out", torch.bfloat16), tt("grad_value", torch.bfloat16), tt("grad_loc", torch.float32), tt("grad_aw", torch.float32)),
                    tuple(ref[k] for k in R.OUTPUTS))
        except AssertionError:
            return False
        return True
    tf, tg = tols(np.float32)
    return rel_err(got["out"], ref["out"]) < tf and all(rel_err(got[k], ref[k]) < tg for k in ("grad_value", "grad_loc", "grad_aw"))


@pytest.mark.parametrize("name", ["ENC", "DEC"])
def test_mutants_are_far_outside_the_bounds_and_the_old_metric_is_blind_to_three(name):
    blind = []
    for mutant in R.MUTANTS:
        sfx = "bf16" if mutant == "bf16_sum" else "f32"
        t, ref, bnd = case(name, sfx)
        got = R.evaluate(*_args(t), dtype=torch.float64, mutant=mutant)
        if sfx == "bf16":
            got = _stored_bf16(got)
        w = R.worst(got, ref, bnd)
        passes_old = _old_metric_passes(name, sfx, got, ref)
        print(name, mutant, "worst ratios", {k: f"{v:.3g}" for k, v in w.items()}, "old metric passes:", passes_old)
        assert max(w.values()) > 10, (mutant, w)
        if passes_old:
            blind.append(mutant)
    # the unmutated float64 evaluation passes the old criteria, of course
    t, ref, bnd = case(name, "f32")
    assert _old_metric_passes(name, "f32", ref, ref)
    assert len(blind) >= 3, blind


PROBES = {
    # encoder-shaped: Lq == S = 36, the walk of 23 x 39 + 15 x 15 = 1122 positions over 32 images; decoder-shaped: one image
    "enc": dict(shapes=[(4, 8), (2, 2)], N=32, Lq=36),
    "dec": dict(shapes=[(4, 8), (2, 2)], N=1, Lq=1124),
}


@pytest.mark.parametrize("per_query_go", [True, False])
@pytest.mark.parametrize("which", list(PROBES))
def test_exact_probe_is_exact(which, per_query_go):
    z = R.exact_probe(per_query_go=per_query_go, **PROBES[which])
    t = R.typed(z, "f32")
    ref = R.evaluate(*_args(t), dtype=torch.float64)
    f32 = R.evaluate(*_args(t), dtype=torch.float32)
    orc = _oracle(t, np.float32)
    for k in R.OUTPUTS:
        assert f32[k].dtype == np.float32 and orc[k].dtype == np.float32
        assert np.array_equal(f32[k].astype(np.float64), ref[k]), k
        assert np.array_equal(orc[k].astype(np.float64).reshape(ref[k].shape), ref[k]), k
        assert np.abs(ref[k]).max() > 0
    # every border position is there: h_im = -1 and H (dropped), 0 and H - 1 (one row of corners), w alike
    H, Wd = PROBES[which]["shapes"][0]
    h_im = z["loc"][..., 0, :, 1].astype(np.float64) * H - 0.5
    w_im = z["loc"][..., 0, :, 0].astype(np.float64) * Wd - 0.5
    live = z["aw"][..., 0, :] != 0
    for v in (-1.25, -1.0, -0.75, 0.0, H - 1.0, H - 0.75, float(H), H + 0.25):
        assert (live & (h_im == v)).any(), v
    for v in (-1.25, -1.0, 0.0, Wd - 1.0, float(Wd), Wd + 0.25):
        assert (live & (w_im == v)).any(), v
    if not per_query_go:      # the bf16 probe: inputs and stored results are bf16 numbers
        for k in ("value", "grad_out"):
            assert np.array_equal(R.typed(z, "bf16")[k], t[k]), k
        st = _stored_bf16(ref)
        for k in ("out", "grad_value"):
            assert np.array_equal(st[k], ref[k]), k


@pytest.mark.parametrize("name", list(CALLS))
def test_no_sampling_position_near_a_pixel_boundary(name):
    case(name, "f32")
    z = _cache[("z", name)]
    assert R.near_boundary(z["loc"], z["shapes"]) == 0
    # ... and the recipe did produce what it is for: dropped samples, corners outside the map, several grad_out scales
    H, Wd = CALLS[name].shapes[0]
    h_im = z["loc"][:, :, :, 0, :, 1] * H - 0.5
    if name != "SCR":      # (301 x 301 and 100 points: no sample lands in the half pixel above the map)
        assert (h_im <= -1).any() and ((h_im > -1) & (h_im < 0)).any() and (h_im > H - 1).any()
    assert len(np.unique(np.abs(z["grad_out"]).max(-1))) > 8
    # and the nudge has something to do where it is handed positions on a boundary
    loc = torch.full((1, 1, 1, 1, 1, 2), 0.375)      # h_im = 1 exactly
    assert R.near_boundary(loc.numpy(), [(4, 4)]) > 0
    assert R.near_boundary(R._nudge(loc, [(4, 4)]).numpy(), [(4, 4)]) == 0


@pytest.mark.parametrize("name", list(CALLS))
def test_bounds_are_not_trivial(name):
    t, ref, bnd = case(name, "f32")
    for k in R.OUTPUTS:
        nz = ref[k] != 0
        med = float(np.median(bnd[k][nz] / np.abs(ref[k][nz])))
        print(name, k, "median bound / |ref|", f"{med:.3g}")
        assert med < 1e-3, (k, med)
        assert (bnd[k][nz] > 0).all(), k
