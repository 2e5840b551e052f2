"""No GPU: tests/swin_block_ref.py against itself -- the fp32 emulation of the kernels' roundings stays inside the element-wise bounds, and
every wrong variant leaves them in at least one element.  RICHSEM_REPORT=1 prints the worst ratios (profiles/r32_swin_block.md)."""
import os

import pytest
import torch

import swin_block_ref as R

REPORT = bool(os.environ.get("RICHSEM_REPORT"))
LINEAR_SHAPES = [(1, 32, 32), (17, 96, 384), (200, 384, 96), (129, 160, 224), (17, 2112, 32), (70, 96, 96), (33, 6144, 32)]
LN_SHAPES = [(1, 32), (70, 96), (200, 1536), (70, 4096)]


def _report(tag, res):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)


@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
@pytest.mark.parametrize("T, K, N", LINEAR_SHAPES)
def test_linear_emulation_is_inside_the_bounds(T, K, N, epilogue):
    gen = torch.Generator().manual_seed(1000 * epilogue + T + K + N)
    x, w, bias, aux = R.linear_inputs(T, K, N, epilogue, gen)
    val, bound = R.linear_reference(x, w, bias, aux, epilogue)
    res = R.ratios(R.linear_emulate(x, w, bias, aux, epilogue), val, bound)
    _report(f"linear epilogue {epilogue} {(T, K, N)}", res)
    assert sorted(res) == sorted(val) and all(r <= 1.0 for r in res.values()), res


def test_gelu_backward_from_the_stored_preactivation_is_inside_the_moved_bound():
    """epilogue 3 fed the ROUNDED u of an epilogue 1, against the definition on the exact pre-activation: the `moved` term"""
    gen = torch.Generator().manual_seed(7)
    x, w1, b1, _ = R.linear_inputs(70, 96, 384, 1, gen)
    dy, w2t, _, _ = R.linear_inputs(70, 96, 384, 0, gen)
    fwd, fwd_bound = R.linear_reference(x, w1, b1, None, 1)
    u_stored = R.linear_emulate(x, w1, b1, None, 1)["out2"].to(R.BF)
    val, bound = R.linear_reference(dy, w2t, None, fwd["out2"], 3, moved=fwd_bound["out2"])
    plain = R.linear_reference(dy, w2t, None, fwd["out2"], 3)[1]
    got = R.linear_emulate(dy, w2t, None, u_stored, 3)
    res = R.ratios({"out": got["out"]}, {"out": val["out"]}, bound)
    _report("gelu backward, moved u", res)
    assert res["out"] <= 1.0
    assert R.ratios({"out": got["out"]}, {"out": val["out"]}, plain)["out"] > 1.0      # (and the term is needed)


@pytest.mark.parametrize("epilogue, wrong", [(e, v) for e, vs in R.LINEAR_WRONG.items() for v in vs])
def test_wrong_linear_variants_leave_the_bounds(epilogue, wrong):
    gen = torch.Generator().manual_seed(11 + epilogue)
    x, w, bias, aux = R.linear_inputs(40, 96, 96, epilogue, gen)
    val, bound = R.linear_reference(x, w, bias, aux, epilogue)
    bad = R.linear_reference(x, w, bias, aux, epilogue, wrong=wrong)[0]
    assert max(R.ratios(bad, val, bound).values()) > 1.0


@pytest.mark.parametrize("T, C", LN_SHAPES)
def test_layernorm_emulation_is_inside_the_bounds(T, C):
    gen = torch.Generator().manual_seed(T + C)
    x, dy, add, gamma, beta = R.layernorm_inputs(T, C, gen)
    val, bound = R.layernorm_reference(x, gamma, beta, 1e-5)
    res = R.ratios(R.layernorm_emulate(x, gamma, beta, 1e-5), val, bound)
    _report(f"layernorm {(T, C)}", res)
    assert sorted(res) == ["mean", "out", "rstd"] and all(r <= 1.0 for r in res.values()), res
    for a in (add, None):
        val, bound = R.layernorm_backward_reference(dy, x, gamma, a, 1e-5)
        res = R.ratios(R.layernorm_backward_emulate(dy, x, gamma, a, 1e-5), val, bound)
        _report(f"layernorm backward {(T, C)} add={a is not None}", res)
        assert sorted(res) == ["dbeta", "dgamma", "dx"] and all(r <= 1.0 for r in res.values()), res


@pytest.mark.parametrize("wrong", R.LN_WRONG)
def test_wrong_layernorm_variants_leave_the_bounds(wrong):
    x, _, _, gamma, beta = R.layernorm_inputs(40, 96, torch.Generator().manual_seed(3))
    val, bound = R.layernorm_reference(x, gamma, beta, 1e-5)
    assert max(R.ratios(R.layernorm_reference(x, gamma, beta, 1e-5, wrong=wrong)[0], val, bound).values()) > 1.0


@pytest.mark.parametrize("wrong", R.LN_BWD_WRONG)
def test_wrong_layernorm_backward_variants_leave_the_bounds(wrong):
    x, dy, add, gamma, _ = R.layernorm_inputs(40, 96, torch.Generator().manual_seed(4))
    val, bound = R.layernorm_backward_reference(dy, x, gamma, add, 1e-5)
    assert max(R.ratios(R.layernorm_backward_reference(dy, x, gamma, add, 1e-5, wrong=wrong)[0], val, bound).values()) > 1.0


def test_erf_and_tanh_gelu_are_closer_than_the_bounds_can_see():
    """what the docstring of swin_block_ref states: the two forms differ by less than 5e-4"""
    x = torch.linspace(-8, 8, 160001, dtype=torch.float64)
    tanh_form = 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    assert float((R.gelu(x) - tanh_form).abs().max()) < 5e-4
    assert float(R.gelu_grad(x).abs().max()) <= R.LIP and abs(float(R.gelu_grad(torch.zeros(1, dtype=torch.float64))) - 0.5) < 1e-15
