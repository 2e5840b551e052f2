"""GPU (-m gpu): the weight-gradient rule of richsem_amd/functions/linear.py (linear_wgrad) at its boundary, for the autograd functions that
need the device -- which path ran is counted by wrappers around the real kernel call (linear_wgrad_bf16) and around WgradGroup.add, the
gradients are compared with fp32 autograd on the same bf16 operands (bound: 1e-2 * max|ref|, as tests/test_gpu_ffn.py holds
linear_bf16 to) -- and ConvAffineFunction against the stand-alone calls it now shares its launches with.

The smallest shapes these functions take: 256-wide inputs, 128-wide layers; T = 1024 is the first token count on the kernel, 1023 the
last on the transposed GEMM."""
import pytest
import torch
import torch.nn.functional as F

from richsem_amd.functions import linear as lin
from richsem_amd.functions.ffn import FFNSmallFunction
from richsem_amd.functions.linear import Lin256Function, StackedValueProjFunction, WgradGroup, lin256_pack, pack_linear256, wgrad_boundary

pytestmark = pytest.mark.gpu


@pytest.fixture
def counts(monkeypatch):
    n = {"kernel": 0, "deferred": 0}
    kernel, add = lin.linear_wgrad_bf16, WgradGroup.add

    def counted_kernel(*a, **k):
        n["kernel"] += 1
        return kernel(*a, **k)

    def counted_add(self, *a, **k):
        n["deferred"] += 1
        return add(self, *a, **k)

    monkeypatch.setattr(lin, "linear_wgrad_bf16", counted_kernel)
    monkeypatch.setattr(WgradGroup, "add", counted_add)
    return n


def rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * scale


def layers(widths, seed):
    ws = [rand(n, 256, seed=seed + i, scale=1 / 16).requires_grad_(True) for i, n in enumerate(widths)]
    bs_ = [rand(n, seed=seed + 10 + i, scale=0.1).requires_grad_(True) for i, n in enumerate(widths)]
    return ws, bs_


def close(got, ref, what):
    assert got.dtype == torch.float32 and got.shape == ref.shape
    err, top = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max|err| / max|ref| = {err / top:.2e}")
    assert err <= 1e-2 * top, what


def check_linear(x, dys, ws, bs_):
    """the parameters' gradients against fp32 autograd of x W^T + b on the bf16-rounded weights, one output gradient per layer"""
    refs = [(w.detach().to(torch.bfloat16).float().requires_grad_(True), b.detach().clone().requires_grad_(True)) for w, b in zip(ws, bs_)]
    for (wr, br), dy in zip(refs, dys):
        F.linear(x.float(), wr, br).backward(dy.float())
    for i, ((wr, br), w, b) in enumerate(zip(refs, ws, bs_)):
        close(w.grad, wr.grad, f"dW[{i}]")
        close(b.grad, br.grad, f"db[{i}]")


@pytest.mark.parametrize("widths", [(128,), (128, 128)], ids=["one_layer", "two_stacked"])
@pytest.mark.parametrize("T", [1023, 1024])
def test_lin256_function(counts, T, widths):
    x = rand(T, 256, seed=T).to(torch.bfloat16)
    ws, bs_ = layers(widths, seed=3)
    dy = rand(T, sum(widths), seed=7).to(torch.bfloat16)
    Lin256Function.apply(x, pack_linear256(ws, bs_), None, False, *ws, *bs_).backward(dy)
    assert counts == {"kernel": int(T == 1024), "deferred": 0}
    check_linear(x, dy.split(list(widths), 1), ws, bs_)


@pytest.mark.parametrize("T", [1023, 1024])
def test_stacked_value_projection(counts, T):
    x = rand(T, 256, seed=T + 1).to(torch.bfloat16)
    ws, bs_ = layers((256, 256), seed=5)
    dys = [rand(T, 256, seed=8 + i).to(torch.bfloat16) for i in range(2)]
    outs = StackedValueProjFunction.apply(x, pack_linear256(ws, bs_), None, *ws, *bs_)
    torch.autograd.backward(outs, dys)
    assert counts == {"kernel": int(T == 1024), "deferred": 0}
    check_linear(x, dys, ws, bs_)


@pytest.mark.parametrize("grouped", [False, True], ids=["alone", "in_group"])
@pytest.mark.parametrize("T", [1023, 1024])
def test_ffn_small_function(counts, T, grouped):
    """both weight gradients of the block: deferred to the layer's group when there is one and the rule picks the kernel, else computed
    on the spot by the kernel (T = 1024) or the transposed GEMM (T = 1023, group or not)"""
    x = rand(T, 256, seed=T + 2).to(torch.bfloat16)
    w1, b1 = rand(128, 256, seed=1, scale=1 / 16).requires_grad_(True), rand(128, seed=2, scale=0.1).requires_grad_(True)
    w2, b2 = rand(256, 128, seed=3, scale=128 ** -0.5).requires_grad_(True), rand(256, seed=4, scale=0.1).requires_grad_(True)
    gw, gb = (1 + rand(256, seed=5, scale=0.1)).requires_grad_(True), rand(256, seed=6, scale=0.1).requires_grad_(True)
    go = rand(T, 256, seed=9).to(torch.bfloat16)
    w2_16 = w2.detach().to(torch.bfloat16).contiguous()
    args = (x, pack_linear256([w1], [b1]), w2_16, lin256_pack(w2_16.t().contiguous()), 1e-5)
    if grouped:
        group = WgradGroup()
        a1, ab1, a2 = wgrad_boundary(group, w1, b1, w2)
        with group:
            out = FFNSmallFunction.apply(*args, a1, ab1, a2, b2, gw, gb)
    else:
        out = FFNSmallFunction.apply(*args, w1, b1, w2, b2, gw, gb)
    out.backward(go)
    on_kernel = 2 * int(T == 1024)
    assert counts == ({"kernel": 0, "deferred": on_kernel} if grouped else {"kernel": on_kernel, "deferred": 0})
    refs = [t.detach().to(torch.bfloat16).float().requires_grad_(True) if t.dim() == 2 else t.detach().clone().requires_grad_(True)
            for t in (w1, b1, w2, b2, gw, gb)]
    xf = x.float()
    F.layer_norm(xf + F.linear(torch.relu(F.linear(xf, refs[0], refs[1])), refs[2], refs[3]), (256,), refs[4], refs[5], 1e-5).backward(go.float())
    for t, r, name in zip((w1, b1, w2, b2, gw, gb), refs, ("dW1", "db1", "dW2", "db2", "d ln_w", "d ln_b")):
        close(t.grad, r.grad, name)


def test_conv_affine_function_runs_the_stand_alone_calls():
    """ConvAffineFunction's forward and weight gradient are conv_forward's and conv_wgrad's launches, its input gradient the entry point
    conv_dgrad's forwards to with no epilogue: equal bits (no k-split at this shape, and the weight gradient's chunk sums go through
    plain stores and a second kernel, so no sum's order depends on the run)"""
    from richsem_amd.conv import ConvAffine, ConvAffineFunction, _pack_form, conv_dgrad, conv_wgrad
    x = rand(1, 9, 7, 128, seed=1).to(torch.bfloat16).requires_grad_(True)
    w = rand(128, 128, 3, 3, seed=2, scale=(128 * 9) ** -0.5).requires_grad_(True)
    scale, shift = 1 + rand(128, seed=3, scale=0.3), rand(128, seed=4, scale=0.5)
    dy = rand(1, 9, 7, 128, seed=5).to(torch.bfloat16)
    y = ConvAffineFunction.apply(x, w, scale, shift, None, 1, 1, True)
    y.backward(dy)
    want = ConvAffine(w, scale, shift, stride=1, padding=1, relu=True)(x.detach())
    assert torch.equal(y, want) and float(want.float().abs().max()) > 0
    dz = torch.ops.aten.threshold_backward(dy, want, 0)
    assert torch.equal(w.grad, conv_wgrad(dz, x.detach(), 128, 3, 3, 1, 1, scale))
    assert torch.equal(x.grad, conv_dgrad(dz, _pack_form(w, scale, True), (1, 9, 7, 128), 128, 3, 3, 1, 1))
