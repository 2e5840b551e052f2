"""GPU (-m gpu): the kernels of csrc/convnext_dw.hip -- depthwise 7 x 7 convolution (both tap orders), its weight gradient, layer scale
forward and backward -- against the element-wise bounds of tests/convnext_ref.py, exact probes checked bit for bit, NaN-poisoned result
buffers with guard rows, and reproducibility of the reductions.

The shapes are those of tests/convnext_ref.py, on which tests/test_convnext_ref.py shows every wrong variant leaving the bounds: a map
smaller than the kernel, one pixel, an odd map of width 96, maps just past a 16 x 16 tile and at T - 1 / T + 1 in either direction, a wide
strip; for the weight gradient also (3, 17, 17, 4096), where a part of three (image, tile) pairs crosses from one image into the next.
Capture into a HIP graph is NOT tested here."""
import os

import pytest
import torch

import convnext_ref as R
from test_gpu_swin_block import Poisoned

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(*ts):
    return [t.cuda().contiguous() if t is not None else None for t in ts]


def _p(t):
    return t.data_ptr() if t is not None else None


def _inside(tag, got, val, bound):
    res = R.ratios(got, val, bound)
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)
    assert res and all(r <= 1.0 for r in res.values()), (tag, res)


def _gen(shape):
    return torch.Generator().manual_seed(2000 + sum(shape))


# ---- raw calls into poisoned buffers ---------------------------------------------------------------------------------------------------
def call_dwconv(x, w, bias, add, flip):
    from richsem_amd import _lib
    B, H, W, C = x.shape
    out = Poisoned(B * H * W, C, BF)
    _lib.check(_lib.load().msda_dwconv7_bf16(x.data_ptr(), w.data_ptr(), _p(bias), _p(add), flip, B, H, W, C, out.ptr(), _lib.raw_stream(x.device)))
    return {"out": out.result(f"dwconv out (flip {flip})").view(B, H, W, C)}


def call_wgrad(dy, x, want_bias=True):
    from richsem_amd import _lib, convnext
    B, H, W, C = x.shape
    dw, db = Poisoned(49, C, torch.float32), (Poisoned(C, 1, torch.float32) if want_bias else None)
    ws = torch.full((convnext.dwconv7_workspace_bytes(B, H, W, C) // 4,), float("nan"), device="cuda")
    _lib.check(_lib.load().msda_dwconv7_wgrad_bf16(dy.data_ptr(), x.data_ptr(), B, H, W, C, dw.ptr(), db.ptr() if db else None, ws.data_ptr(),
                                                   _lib.raw_stream(x.device)))
    res = {"dw": dw.result("dw")}
    if want_bias:
        res["dbias"] = db.result("dbias")[:, 0]
    return res


def call_scale(z, gamma, res):
    from richsem_amd import _lib
    T, C = z.shape
    out = Poisoned(T, C, BF)
    _lib.check(_lib.load().msda_layer_scale_forward_bf16(z.data_ptr(), gamma.data_ptr(), res.data_ptr(), T, C, out.ptr(), _lib.raw_stream(z.device)))
    return {"out": out.result("layer scale out")}


def call_scale_backward(dout, z, gamma, want_gamma=True):
    from richsem_amd import _lib, swin
    T, C = dout.shape
    dz, dg = Poisoned(T, C, BF), (Poisoned(C, 1, torch.float32) if want_gamma else None)
    ws = torch.full((swin.layernorm_workspace_bytes(T, C) // 4,), float("nan"), device="cuda") if want_gamma else None
    _lib.check(_lib.load().msda_layer_scale_backward_bf16(dout.data_ptr(), _p(z) if want_gamma else None, gamma.data_ptr(), T, C, dz.ptr(),
                                                          dg.ptr() if dg else None, _p(ws), _lib.raw_stream(dout.device)))
    res = {"dz": dz.result("dz")}
    if want_gamma:
        res["dgamma"] = dg.result("dgamma")[:, 0]
    return res


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES)
def test_convolution_inside_its_bound(shape):
    for flip in (0, 1):
        for with_bias, with_add in ((True, True), (False, False), (True, False), (False, True)):
            x, w, bias, add = R.dwconv_inputs(shape, _gen(shape), with_bias, with_add)
            val, bound = R.dwconv_reference(x, w, bias, add, flip)
            _inside(f"dwconv {shape} flip={flip} bias={with_bias} add={with_add}", call_dwconv(*_dev(x, w, bias, add), flip), val, bound)


@pytest.mark.parametrize("shape", R.WGRAD_SHAPES)
def test_weight_gradient_inside_its_bound_and_reproducible(shape):
    gen = _gen(shape)
    x, dy = torch.randn(*shape, generator=gen).to(BF), torch.randn(*shape, generator=gen).to(BF)
    val, bound = R.wgrad_reference(dy, x)
    dyd, xd = _dev(dy, x)
    first = call_wgrad(dyd, xd)
    _inside(f"wgrad {shape}", first, val, bound)
    again = call_wgrad(dyd, xd)
    assert _same(first["dw"], again["dw"]) and _same(first["dbias"], again["dbias"])
    alone = call_wgrad(dyd, xd, want_bias=False)
    assert _same(first["dw"], alone["dw"])


@pytest.mark.parametrize("tokens, C", R.SCALE_SHAPES)
def test_layer_scale_inside_its_bounds_and_reproducible(tokens, C):
    z, gamma, res, dout = R.scale_inputs(tokens, C, _gen((tokens, C)))
    zd, gd, rd, dd = _dev(z, gamma, res, dout)
    val, bound = R.scale_reference(z, gamma, res)
    _inside(f"layer scale {(tokens, C)}", call_scale(zd, gd, rd), val, bound)
    val, bound = R.scale_backward_reference(dout, z, gamma, res)
    first = call_scale_backward(dd, zd, gd)
    _inside(f"layer scale backward {(tokens, C)}", first, val, bound)
    again = call_scale_backward(dd, zd, gd)
    assert _same(first["dgamma"], again["dgamma"]) and _same(first["dz"], again["dz"])
    assert _same(first["dz"], call_scale_backward(dd, None, gd, want_gamma=False)["dz"])


# ---- exact probes ------------------------------------------------------------------------------------------------------------------------
PROBE = (2, 13, 20, 64)      # two tiles along x: the probe at (6, 14) spreads over the tile edge


def _dyadic(shape, gen):
    """multiples of 2^-6 below 2: exact in bf16, and so is the sum of two of them"""
    return torch.randint(-127, 128, shape, generator=gen).float() / 64


@pytest.mark.parametrize("y0, x0", [(6, 14), (0, 0), (12, 19)])
def test_one_hot_input_places_the_taps(y0, x0):
    B, H, W, C = PROBE
    c0 = 37
    gen = torch.Generator().manual_seed(11)
    w, bias = _dyadic((49, C), gen), _dyadic((C,), gen)
    x = torch.zeros(PROBE, dtype=BF)
    x[0, y0, x0, c0] = 1.0
    expect = torch.zeros(PROBE)
    for ky in range(7):
        for kx in range(7):
            y, xx = y0 + 3 - ky, x0 + 3 - kx
            if 0 <= y < H and 0 <= xx < W:
                expect[0, y, xx, c0] = w[7 * ky + kx, c0]
    xd, wd, bd = _dev(x, w, bias)
    got = call_dwconv(xd, wd, None, None, 0)["out"].cpu()
    assert _same(got, expect.to(BF))      # channels other than c0 and all of image 1: exact (positive) zeros
    got = call_dwconv(xd, wd, bd, None, 0)["out"].cpu()
    assert _same(got, (expect + bias).to(BF)) and _same(got[1], bias.to(BF).expand(H, W, C))      # image 1 is exactly the bias
    # the other tap order: the definition in float64 is exact on these operands
    val, _ = R.dwconv_reference(x, w, bias, None, 1)
    assert _same(call_dwconv(xd, wd, bd, None, 1)["out"].cpu(), val["out"].to(BF))
    assert not _same(val["out"].to(BF), (expect + bias).to(BF))


@pytest.mark.parametrize("b0, y0, x0", [(1, 6, 14), (0, 0, 0), (1, 12, 19)])
def test_one_hot_cotangent_reads_the_shifted_input(b0, y0, x0):
    B, H, W, C = PROBE
    c0 = 37
    x = torch.randn(PROBE, generator=torch.Generator().manual_seed(12)).to(BF)
    dy = torch.zeros(PROBE, dtype=BF)
    dy[b0, y0, x0, c0] = 1.0
    expect = torch.zeros(49, C)
    for ky in range(7):
        for kx in range(7):
            y, xx = y0 + ky - 3, x0 + kx - 3
            if 0 <= y < H and 0 <= xx < W:
                expect[7 * ky + kx, c0] = x[b0, y, xx, c0].float()
    got = call_wgrad(*_dev(dy, x))
    assert _same(got["dw"].cpu(), expect)
    onehot = torch.zeros(C)
    onehot[c0] = 1.0
    assert _same(got["dbias"].cpu(), onehot)


def test_zero_cotangent_gives_exact_zeros():
    x = torch.randn(PROBE, generator=torch.Generator().manual_seed(13)).to(BF)
    got = call_wgrad(*_dev(torch.zeros(PROBE, dtype=BF), x))
    assert _same(got["dw"].cpu(), torch.zeros(49, PROBE[3])) and _same(got["dbias"].cpu(), torch.zeros(PROBE[3]))


# ---- the autograd functions ----------------------------------------------------------------------------------------------------------------
def test_autograd_functions_return_the_kernels_results_in_the_parameters_dtypes():
    from richsem_amd import convnext
    shape = (2, 13, 9, 96)
    gen = _gen(shape)
    x, w, bias, _ = R.dwconv_inputs(shape, gen)
    g = torch.randn(*shape, generator=gen).to(BF)
    C = shape[-1]
    weight = w.t().reshape(C, 1, 7, 7).contiguous().cuda().requires_grad_(True)      # an fp32 parameter
    bd = bias.cuda().requires_grad_(True)
    xd = x.cuda().requires_grad_(True)
    out = convnext.dwconv7(xd, weight, bd)
    out.backward(g.cuda())
    val, bound = R.dwconv_reference(x, w, bias, None, 0)
    _inside("dwconv7()", {"out": out.detach()}, val, bound)
    val, bound = R.dwconv_reference(g, w, None, None, 1)
    _inside("dwconv7() input gradient", {"out": xd.grad}, val, bound)
    val, bound = R.wgrad_reference(g, x)
    assert weight.grad.dtype == torch.float32 and weight.grad.shape == weight.shape and bd.grad.dtype == torch.float32
    _inside("dwconv7() weight gradient", {"dw": weight.grad.reshape(C, 49).t(), "dbias": bd.grad}, val, bound)

    z, gamma, res, dout = R.scale_inputs(65, 96, gen)
    zd, rd = z.cuda().requires_grad_(True), res.cuda().requires_grad_(True)
    gd = gamma.to(BF).cuda().requires_grad_(True)      # a bf16 parameter: the kernel reads its fp32 copy
    out = convnext.layer_scale(zd, gd, rd)
    out.backward(dout.cuda())
    g32 = gamma.to(BF).float()
    val, bound = R.scale_reference(z, g32, res)
    _inside("layer_scale()", {"out": out.detach()}, val, bound)
    val, bound = R.scale_backward_reference(dout, z, g32, res)
    _inside("layer_scale() backward", {"dz": zd.grad}, val, bound)
    assert gd.grad.dtype == BF and _same(rd.grad.cpu(), dout)
    assert float(((gd.grad.double().cpu() - val["dgamma"]).abs() / (bound["dgamma"] + R.U * val["dgamma"].abs())).max()) <= 1.0
