"""No GPU: the bounds of tests/focalnet_ref.py are wide enough for an fp32 implementation with the kernels' roundings (the emulation stays
inside every bound on every shape and configuration the GPU tests use) and narrow enough to catch the mistakes a context-aggregation kernel
can make (each wrong variant leaves the bound of every tensor it changes on those same shapes).  RICHSEM_REPORT=1 prints the worst ratios
(recorded in profiles/r35_focalnet.md)."""
import os

import pytest
import torch
import torch.nn.functional as F

import focalnet_ref as R

REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _gen(shape, L):
    return torch.Generator().manual_seed(3000 + sum(shape) + L)


def _report(what, shape, r):
    if REPORT:
        print(f"[measured] {what} {shape}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items()), flush=True)


@pytest.fixture(scope="module")
def runs():
    """the emulated forward and backward of every (shape, configuration), computed once"""
    cache = {}

    def get(shape, cfg):
        if (shape, cfg) not in cache:
            L, window, normalize = cfg
            ctx0, gates, ws, dA = R.make_inputs(shape, L, window, _gen(shape, L))
            fwd = R.forward_emulate(ctx0, gates, ws, L, window, normalize)
            bwd = R.backward_emulate(dA, ctx0, gates, ws, L, window, normalize, fwd)
            cache[(shape, cfg)] = (ctx0, gates, ws, dA, fwd, {**fwd, **bwd})
        return cache[(shape, cfg)]
    return get


@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_forward_emulation_is_inside_and_wrong_variants_outside(shape, cfg, runs):
    L, window, normalize = cfg
    ctx0, gates, ws, _, fwd, _ = runs(shape, cfg)
    val, bound = R.forward_reference(ctx0, gates, ws, L, window, normalize, fwd)
    r = R.ratios(fwd, val, bound)
    _report(f"forward {cfg}", shape, r)
    assert set(r) == {f"u{l}" for l in range(L)} | {"m", "g", "A"} and all(v <= 1.0 for v in r.values()), (shape, cfg, r)
    for wrong in R.FORWARD_WRONG:
        r = R.ratios(R.forward_reference(ctx0, gates, ws, L, window, normalize, fwd, wrong=wrong)[0], val, bound)
        _report(f"forward {cfg} wrong={wrong}", shape, r)
        for k in R.affected(wrong, L):
            if k in r:
                assert (r[k] == 0.0) if R.same_function(wrong, shape, normalize) else (r[k] > 1.0), (shape, cfg, wrong, k, r)


@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_backward_emulation_is_inside_and_wrong_variants_outside(shape, cfg, runs):
    L, window, normalize = cfg
    ctx0, gates, ws, dA, _, both = runs(shape, cfg)
    val, bound = R.backward_reference(dA, ctx0, gates, ws, L, window, normalize, both)
    r = R.ratios(both, val, bound)
    _report(f"backward {cfg}", shape, r)
    assert set(r) == {f"du{l}" for l in range(L)} | {f"dw{l}" for l in range(L)} | {"dgates", "dctx0"}
    assert all(v <= 1.0 for v in r.values()), (shape, cfg, r)
    for wrong in R.BACKWARD_WRONG:
        r = R.ratios(R.backward_reference(dA, ctx0, gates, ws, L, window, normalize, both, wrong=wrong)[0], val, bound)
        _report(f"backward {cfg} wrong={wrong}", shape, r)
        for k in R.affected(wrong, L):
            if k in r:
                assert (r[k] == 0.0) if R.same_function(wrong, shape, normalize) else (r[k] > 1.0), (shape, cfg, wrong, k, r)


def test_modulation_product_emulation_is_inside():
    gen = torch.Generator().manual_seed(5)
    q, mod, dout = (torch.randn(65, 96, generator=gen).to(R.BF) for _ in range(3))
    val, bound = R.modulate_reference(q, mod, dout)
    r = R.ratios(R.modulate_emulate(q, mod, dout), val, bound)
    assert all(v <= 1.0 for v in r.values()), r
    assert R.ratios({"out": (q * mod) * 1.01}, val, bound)["out"] > 1.0


def test_torch_bf16_composition_is_outside_the_bounds():
    """what the bounds are for: a composition that rounds every intermediate to bf16 does not pass as the kernel"""
    shape, (L, window, normalize) = (2, 13, 9, 96), R.CONFIGS[0]
    ctx0, gates, ws, _ = R.make_inputs(shape, L, window, _gen(shape, L))
    fwd = R.forward_emulate(ctx0, gates, ws, L, window, normalize)
    val, bound = R.forward_reference(ctx0, gates, ws, L, window, normalize, fwd)
    C = shape[-1]
    ctx, acc = ctx0.permute(0, 3, 1, 2), 0
    for l, K in enumerate(R.sizes(L, window)):
        ctx = F.gelu(F.conv2d(ctx, ws[l].t().reshape(C, 1, K, K).to(R.BF), None, padding=K // 2, groups=C))
        acc = acc + ctx * gates[..., l].unsqueeze(1)
    acc = acc + F.gelu(ctx.mean((2, 3), keepdim=True)) * gates[..., L].unsqueeze(1)
    assert R.ratios({"A": acc.permute(0, 2, 3, 1)}, val, bound)["A"] > 1.0


def test_the_definition_is_torch_autograd():
    """the helper's formulas, chained in float64 without any stored intermediate, against torch's conv2d / gelu and their autograd"""
    gen = torch.Generator().manual_seed(7)
    for shape, (L, window, normalize) in (((2, 3, 5, 32), R.CONFIGS[0]), ((1, 9, 8, 32), R.CONFIGS[1])):
        ctx0, gates, ws, dA = R.make_inputs(shape, L, window, gen)
        C, ks = shape[-1], R.sizes(L, window)
        x = ctx0.double().requires_grad_(True)
        gt = gates.double().requires_grad_(True)
        wp = [w.double().t().reshape(C, 1, K, K).clone().requires_grad_(True) for w, K in zip(ws, ks)]
        ctx, acc, us = x.permute(0, 3, 1, 2), 0, []
        for l, K in enumerate(ks):
            us.append(F.conv2d(ctx, wp[l], None, padding=K // 2, groups=C))
            ctx = F.gelu(us[-1])
            acc = acc + ctx * gt[..., l].unsqueeze(1)
        m = ctx.mean((2, 3))
        acc = acc + F.gelu(m)[:, :, None, None] * gt[..., L].unsqueeze(1)
        A = (acc / (L + 1) if normalize else acc).permute(0, 2, 3, 1)
        dus = torch.autograd.grad((A * dA.double()).sum(), us, retain_graph=True)
        (A * dA.double()).sum().backward()
        stored = {f"u{l}": us[l].detach().permute(0, 2, 3, 1) for l in range(L)}
        stored.update({f"du{l}": dus[l].permute(0, 2, 3, 1) for l in range(L)})
        stored["m"], stored["g"] = m.detach(), F.gelu(m).detach()
        val, _ = R.forward_reference(ctx0, gates, ws, L, window, normalize, stored)
        close = dict(rtol=1e-10, atol=1e-12)
        for l in range(L):
            torch.testing.assert_close(val[f"u{l}"], stored[f"u{l}"], **close)
        torch.testing.assert_close(val["A"], A.detach(), **close)
        val, _ = R.backward_reference(dA, ctx0, gates, ws, L, window, normalize, stored)
        for l in range(L):
            torch.testing.assert_close(val[f"du{l}"], stored[f"du{l}"], **close)
            torch.testing.assert_close(val[f"dw{l}"], wp[l].grad.reshape(C, -1).t(), **close)
        torch.testing.assert_close(val["dctx0"], x.grad, **close)
        torch.testing.assert_close(val["dgates"], gt.grad, **close)
