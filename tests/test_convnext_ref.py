"""No GPU: the bounds of tests/convnext_ref.py are wide enough for an fp32 implementation with the kernels' roundings (the emulation stays
inside every bound on every shape the GPU tests use) and narrow enough to catch the mistakes a depthwise-convolution or layer-scale kernel
can make (each wrong variant leaves its bound on those same shapes).  RICHSEM_REPORT=1 prints the worst ratios (recorded in
profiles/r34_convnext.md)."""
import os

import pytest
import torch

import convnext_ref as R

REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _gen(shape):
    return torch.Generator().manual_seed(1000 + sum(shape))


def _report(what, shape, r):
    if REPORT:
        print(f"[measured] {what} {shape}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()), flush=True)


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("flip", [0, 1])
def test_convolution_emulation_is_inside_and_wrong_variants_outside(shape, flip):
    for with_bias, with_add in ((True, True), (False, False), (True, False), (False, True)):
        x, w, bias, add = R.dwconv_inputs(shape, _gen(shape), with_bias, with_add)
        val, bound = R.dwconv_reference(x, w, bias, add, flip)
        r = R.ratios(R.dwconv_emulate(x, w, bias, add, flip), val, bound)
        _report(f"dwconv flip={flip} bias={with_bias} add={with_add}", shape, r)
        assert r["out"] <= 1.0, (shape, flip, with_bias, with_add, r)
    x, w, bias, add = R.dwconv_inputs(shape, _gen(shape))
    val, bound = R.dwconv_reference(x, w, bias, add, flip)
    for wrong in R.CONV_WRONG:      # "taps_flipped" is the forward with flipped taps for flip = 0 and the input gradient without the flip for flip = 1
        r = R.ratios(R.dwconv_reference(x, w, bias, add, flip, wrong=wrong)[0], val, bound)
        _report(f"dwconv flip={flip} wrong={wrong}", shape, r)
        assert (r["out"] == 0.0) if R.same_function(wrong, shape) else (r["out"] > 1.0), (shape, flip, wrong, r)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_torch_bf16_convolution_is_outside_the_bound(shape):
    """what the bound is for: a convolution that rounds more than once (F.conv2d in bf16, then bias and add in bf16) does not pass"""
    x, w, bias, add = R.dwconv_inputs(shape, _gen(shape))
    val, bound = R.dwconv_reference(x, w, bias, add, 0)
    C = shape[-1]
    w16 = w.t().reshape(C, 1, 7, 7).to(R.BF)
    out = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), w16, bias.to(R.BF), padding=3, groups=C).permute(0, 2, 3, 1) + add
    r = R.ratios({"out": out}, val, bound)
    _report("torch bf16 conv2d", shape, r)
    assert r["out"] > 1.0, (shape, r)


@pytest.mark.parametrize("shape", R.WGRAD_SHAPES)
def test_weight_gradient_emulation_is_inside_and_wrong_variants_outside(shape):
    gen = _gen(shape)
    x, dy = torch.randn(*shape, generator=gen).to(R.BF), torch.randn(*shape, generator=gen).to(R.BF)
    val, bound = R.wgrad_reference(dy, x)
    r = R.ratios(R.wgrad_emulate(dy, x), val, bound)
    _report("wgrad", shape, r)
    assert r["dw"] <= 1.0 and r["dbias"] <= 1.0, (shape, r)
    for wrong in R.WGRAD_WRONG:
        r = R.ratios(R.wgrad_reference(dy, x, wrong=wrong)[0], val, bound)
        _report(f"wgrad wrong={wrong}", shape, r)
        assert (r["dw"] == 0.0) if R.same_function(wrong, shape) else (r["dw"] > 1.0), (shape, wrong, r)


@pytest.mark.parametrize("tokens, C", R.SCALE_SHAPES)
def test_layer_scale_emulation_is_inside_and_wrong_variants_outside(tokens, C):
    z, gamma, res, dout = R.scale_inputs(tokens, C, _gen((tokens, C)))
    val, bound = R.scale_reference(z, gamma, res)
    r = R.ratios(R.scale_emulate(z, gamma, res), val, bound)
    _report("layer_scale", (tokens, C), r)
    assert r["out"] <= 1.0, r
    for wrong in R.SCALE_WRONG:
        assert R.ratios(R.scale_reference(z, gamma, res, wrong=wrong)[0], val, bound)["out"] > 1.0, wrong
    val, bound = R.scale_backward_reference(dout, z, gamma, res)
    r = R.ratios(R.scale_backward_emulate(dout, z, gamma, res), val, bound)
    _report("layer_scale backward", (tokens, C), r)
    assert r["dz"] <= 1.0 and r["dgamma"] <= 1.0, r
    for wrong in R.SCALE_BWD_WRONG:
        assert R.ratios(R.scale_backward_reference(dout, z, gamma, res, wrong=wrong)[0], val, bound)["dgamma"] > 1.0, wrong


def test_the_definition_is_torch_conv2d():
    """the tap-major formula of the helper against F.conv2d(groups=C) and its autograd in float64: forward, input gradient (flip = 1 with the
    cotangent as the map), weight and bias gradients"""
    gen = torch.Generator().manual_seed(7)
    for shape in ((2, 3, 5, 32), (1, 9, 8, 32)):
        x, w, bias, _ = R.dwconv_inputs(shape, gen)
        C = shape[-1]
        xd = x.double().requires_grad_(True)
        wd = w.double().t().reshape(C, 1, 7, 7).clone().requires_grad_(True)
        bd = bias.double().requires_grad_(True)
        out = torch.nn.functional.conv2d(xd.permute(0, 3, 1, 2), wd, bd, padding=3, groups=C).permute(0, 2, 3, 1)
        g = torch.randn(*shape, generator=gen).to(R.BF)
        (out * g.double()).sum().backward()
        torch.testing.assert_close(R.dwconv_reference(x, w, bias, None, 0)[0]["out"], out.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(R.dwconv_reference(g, w, None, None, 1)[0]["out"], xd.grad, rtol=1e-12, atol=1e-12)
        val, _ = R.wgrad_reference(g, x)
        torch.testing.assert_close(val["dw"], wd.grad.reshape(C, 49).t(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(val["dbias"], bd.grad, rtol=1e-12, atol=1e-12)
