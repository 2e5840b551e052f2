"""CPU: the comparators of tests/test_gpu_conv_bounds.py checked without a GPU (tests/conv_ref.py).
  * every exact probe meets its conditions for 100 % of its elements, and is not vacuous (more than half of the outputs non-zero);
  * two correct fp32 implementations (torch's fp32 convolutions, and the same with the contraction summed in shuffled chunks) stay
    inside every element-wise bound over four seeds -- the bounds can be met;
  * eight deliberate defects of the REFERENCE are caught by the exact probe on every case they apply to, and by the element-wise bound
    on the real-valued inputs -- the comparators bite.
Worst ratios and the numbers of failing elements are printed (pytest -s)."""
import pytest
import torch

import conv_ref as R

BF = torch.bfloat16


def _fwd_params():
    return [(c, e) for c in R.ALL_FWD_CASES for e in R.EPILOGUES]


def test_the_host_rule_for_forced_tiles():
    assert [R.valid_tiles(c) for c in R.PIXEL_EDGE_COUT] == [[1], [2], [4], [4, 8], [4, 8, 16]]
    assert not R.forced_tile_is_taken(256, 1) and not R.forced_tile_is_taken(256, 2) and not R.forced_tile_is_taken(64, 2)
    assert R.forced_tile_is_taken(48, 1) and R.forced_tile_is_taken(96, 2) and not R.forced_tile_is_taken(96, 4)
    for cout, ct, _ in R.RING_TILES:
        assert R.forced_tile_is_taken(cout, ct) and ct >= 2


def test_mask_probe_bit_patterns():
    v = R.mask_probe_values()
    assert (v > 0).tolist() == [False, False, True, False, True, False, True, False, True, False, True, False]
    assert ((v.view(torch.int16) > 0) == (v > 0)).all()      # the kernel's rule and the float comparison agree on every non-NaN class


@pytest.mark.parametrize("case,epilogue", _fwd_params(), ids=str)
def test_forward_probe_conditions(case, epilogue):
    ok, nonzero, smax = R.probe_conditions("forward", R.make_forward(case, epilogue, 0, probe=True))
    print(f"[probe] forward {case} {epilogue} nonzero={nonzero:.3f} max_sum={smax:.0f}")
    assert ok and nonzero > 0.5


@pytest.mark.parametrize("case", R.ALL_DGRAD_CASES, ids=str)
def test_dgrad_probe_conditions(case):
    for add, mask in R.DGRAD_VARIANTS:
        p = R.make_dgrad(case, add, mask, 0, probe=True)
        ok, nonzero, smax = R.probe_conditions("dgrad", p)
        assert ok, (case, add, mask)
        if case[6] == 1:      # (a strided gradient has classes no tap reaches: those are zeros by definition)
            assert nonzero > 0.5, nonzero
        else:
            assert nonzero > 0.5 / case[6] ** 2 or case[5] == 1, nonzero


@pytest.mark.parametrize("case", R.ALL_WGRAD_CASES, ids=str)
def test_wgrad_probe_conditions(case):
    for seed in range(8):      # (the grouped test uses a problem's index as its seed)
        ok, nonzero, _ = R.probe_conditions("wgrad", R.make_wgrad(case, seed, probe=True))
        assert ok and nonzero > 0.5


def _worst(tag, worst):
    print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("case,epilogue", _fwd_params(), ids=str)
def test_forward_two_fp32_implementations_inside_the_bound(case, epilogue):
    worst = {"plain": 0.0, "shuffled": 0.0}
    for seed in range(4):
        p = R.make_forward(case, epilogue, seed)
        y, b = R.forward_reference(p)
        worst["plain"] = max(worst["plain"], R.ratio(R.fp32_forward(p), y, b))
        worst["shuffled"] = max(worst["shuffled"], R.ratio(R.fp32_forward(p, torch.Generator().manual_seed(seed)), y, b))
    _worst(f"forward {case} {epilogue}", worst)
    assert max(worst.values()) <= 1.0, worst
    p = R.make_forward(case, epilogue, 0, probe=True)
    assert torch.equal(R.fp32_forward(p, torch.Generator().manual_seed(1)), R.forward_reference(p)[0].to(BF))


@pytest.mark.parametrize("case", R.ALL_DGRAD_CASES, ids=str)
def test_dgrad_two_fp32_implementations_inside_the_bound(case):
    worst = {"plain": 0.0, "shuffled": 0.0}
    for seed in range(4):
        for add, mask in R.DGRAD_VARIANTS:
            p = R.make_dgrad(case, add, mask, seed)
            y, b, z = R.dgrad_reference(p)
            worst["plain"] = max(worst["plain"], R.ratio(R.fp32_dgrad(p), y, b, z))
            worst["shuffled"] = max(worst["shuffled"], R.ratio(R.fp32_dgrad(p, torch.Generator().manual_seed(seed)), y, b, z))
    _worst(f"dgrad {case}", worst)
    assert max(worst.values()) <= 1.0, worst
    p = R.make_dgrad(case, True, True, 0, probe=True)
    assert torch.equal(R.fp32_dgrad(p, torch.Generator().manual_seed(1)), R.dgrad_reference(p)[0].to(BF))


@pytest.mark.parametrize("case", R.ALL_WGRAD_CASES, ids=str)
def test_wgrad_two_fp32_implementations_inside_the_bound(case):
    worst = {"dw": 0.0, "dbias": 0.0, "dw_shuffled": 0.0, "dbias_shuffled": 0.0}
    for seed in range(4):
        p = R.make_wgrad(case, seed)
        val, b = R.wgrad_reference(p)
        for tag, got in (("", R.fp32_wgrad(p)), ("_shuffled", R.fp32_wgrad(p, torch.Generator().manual_seed(seed)))):
            for n in ("dw", "dbias"):
                worst[n + tag] = max(worst[n + tag], R.ratio(got[n], val[n], b[n]))
    _worst(f"wgrad {case}", worst)
    assert max(worst.values()) <= 1.0, worst
    p = R.make_wgrad(case, 0, probe=True)
    got, (val, _) = R.fp32_wgrad(p, torch.Generator().manual_seed(1)), R.wgrad_reference(p)
    assert torch.equal(got["dw"].double(), val["dw"]) and torch.equal(got["dbias"].double(), val["dbias"])


# ---- the comparators catch errors -------------------------------------------------------------------------------------------------------
def _bites(tag, probe_pair, real_triple, dtype=BF):
    """the mutated reference, rounded to the kernel's output type, differs from the probe's; and leaves the real-valued bound"""
    (pm, pr), (ym, y, b) = probe_pair, real_triple
    n_probe = int((pm.to(dtype) != pr.to(dtype)).sum())
    n_real = int((((ym - y).abs() / b) > 1.0).sum())
    print(f"[mutation] {tag}: probe elements differing {n_probe} of {pr.numel()}, real-valued elements outside the bound {n_real} of {y.numel()}")
    assert n_probe > 0, tag
    assert n_real > 0, tag


@pytest.mark.parametrize("mutation", R.FWD_MUTATIONS)
def test_forward_comparators_catch(mutation):
    """on every case of the GPU file the defect applies to; the failing elements are added up over the three epilogues the GPU test runs on
    that case (a ReLU can hide two swapped channels of a single pixel)"""
    seen = 0
    for case in R.ALL_FWD_CASES:
        if not R.mutation_applies("forward", mutation, case):
            continue
        seen += 1
        pm, pr, ym, y, b = [], [], [], [], []
        for epilogue in R.EPILOGUES:
            pp, q = R.make_forward(case, epilogue, 0, probe=True), R.make_forward(case, epilogue, 0)
            pm.append(R.forward_reference(pp, mutate=mutation)[0])
            pr.append(R.forward_reference(pp)[0])
            ym.append(R.forward_reference(q, mutate=mutation)[0])
            ref = R.forward_reference(q)
            y.append(ref[0])
            b.append(ref[1])
        _bites(f"forward {mutation} {case}", (torch.stack(pm), torch.stack(pr)), (torch.stack(ym), torch.stack(y), torch.stack(b)))
    assert seen >= 2, seen


@pytest.mark.parametrize("mutation", R.DGRAD_MUTATIONS)
def test_dgrad_comparators_catch(mutation):
    seen = 0
    for case in R.ALL_DGRAD_CASES:
        if not R.mutation_applies("dgrad", mutation, case):
            continue
        seen += 1
        pp, pr = R.make_dgrad(case, True, True, 0, probe=True), R.make_dgrad(case, True, True, 0)
        y, b, _ = R.dgrad_reference(pr)
        _bites(f"dgrad {mutation} {case}", (R.dgrad_reference(pp, mutate=mutation)[0], R.dgrad_reference(pp)[0]),
               (R.dgrad_reference(pr, mutate=mutation)[0], y, b))
    assert seen >= 2


@pytest.mark.parametrize("mutation", R.WGRAD_MUTATIONS)
def test_wgrad_comparators_catch(mutation):
    for case in R.ALL_WGRAD_CASES:
        if not R.mutation_applies("wgrad", mutation, case):
            continue
        pp, pr = R.make_wgrad(case, 0, probe=True), R.make_wgrad(case, 0)
        val, b = R.wgrad_reference(pr)
        _bites(f"wgrad {mutation} {case}", (R.wgrad_reference(pp, mutate=mutation)[0]["dw"], R.wgrad_reference(pp)[0]["dw"]),
               (R.wgrad_reference(pr, mutate=mutation)[0]["dw"], val["dw"], b["dw"]), torch.float32)
        if mutation == "tail":
            vm = R.wgrad_reference(pr, mutate=mutation)[0]
            assert int((((vm["dbias"] - val["dbias"]).abs() / b["dbias"]) > 1.0).sum()) > 0
