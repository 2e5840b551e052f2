"""GPU (-m gpu): the kernels of csrc/swin_block_mfma.hip against the element-wise bounds of tests/swin_block_ref.py, exact probes checked bit
for bit, NaN-poisoned result buffers with guard rows, reproducibility and saved memory of ``swin_mlp``, and the float64 fixture of the
reference's classes with ``set_fused(True)`` under the rule of tests/test_gpu_swin.py (err(fused path) <= 2 err(torch composition)).

The shapes are the smallest at which the kernels can go wrong: one token, a partial 16-token tile, more than one workgroup (a row tile is
128 tokens: 129), K with a half-filled last 64-block (32, 96, 160) and with many blocks (2112 = 33 x 64), N with a half-filled last
64-channel tile (32, 96, 224), and one shape that takes the 128-channel tiles (N a multiple of 128 and at least 128 workgroups of them).
K is never split across workgroups, so there is no split-K case.  Capture of the new functions into a HIP graph is NOT tested here
("Class head": a capture test in a new file made an unrelated graphed-step test fault in whole-suite runs)."""
import os

import pytest
import torch

import swin_attn_ref as A
import swin_block_ref as R
from test_gpu_swin import NET, _backward, _compare, _results, comp_layer, comp_net

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
GUARD = 3            # guard rows (elements for the vectors) before and after every result
TOKENS = (1, 17, 200, 129)
KN = [(32, 32), (96, 384), (384, 96), (160, 224), (2112, 32)]


# ---- raw calls into poisoned buffers ---------------------------------------------------------------------------------------------------
class Poisoned:
    """a result buffer of `rows` rows of `width` with GUARD rows of NaN on either side, NaN inside too"""

    def __init__(self, rows, width, dtype):
        self.full = torch.full((rows + 2 * GUARD, width), float("nan"), dtype=dtype, device="cuda")
        self.view = self.full[GUARD:GUARD + rows]
        self.bits = torch.int16 if dtype == BF else torch.int32
        self.poison = self.full[0, 0].view(self.bits).item()

    def ptr(self):
        return self.view.data_ptr()

    def result(self, what):
        g = torch.cat([self.full[:GUARD], self.full[GUARD + self.view.shape[0]:]]).view(self.bits)
        assert bool((g == self.poison).all()), f"{what}: a guard row was written"
        assert not bool(torch.isnan(self.view).any()), f"{what}: an element was not written"
        return self.view


def call_linear(x, w, bias, aux, epilogue, want_out2):
    from richsem_amd import _lib
    T, K = x.shape
    N = w.shape[0]
    out, out2 = Poisoned(T, N, BF), (Poisoned(T, N, BF) if want_out2 else None)
    _lib.check(_lib.load().msda_swin_linear_bf16(x.data_ptr(), w.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                 aux.data_ptr() if aux is not None else None, epilogue, T, K, N, out.ptr(),
                                                 out2.ptr() if out2 else None, _lib.raw_stream(x.device)))
    res = {"out": out.result(f"out (epilogue {epilogue})")}
    if out2:
        res["out2"] = out2.result(f"out2 (epilogue {epilogue})")
    return res


def call_layernorm(x, gamma, beta, eps=1e-5, stats=True):
    from richsem_amd import _lib
    T, C = x.shape
    out, mean, rstd = Poisoned(T, C, BF), Poisoned(T, 1, torch.float32), Poisoned(T, 1, torch.float32)
    _lib.check(_lib.load().msda_swin_layernorm_forward_bf16(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, T, C, out.ptr(),
                                                            mean.ptr() if stats else None, rstd.ptr() if stats else None, _lib.raw_stream(x.device)))
    res = {"out": out.result("layernorm out")}
    if stats:
        res.update(mean=mean.result("mean")[:, 0], rstd=rstd.result("rstd")[:, 0])
    return res


def call_layernorm_backward(dy, x, mean, rstd, gamma, add, want_gamma=True, want_beta=True):
    from richsem_amd import _lib, swin
    T, C = x.shape
    dx, dg, db = Poisoned(T, C, BF), Poisoned(C, 1, torch.float32), Poisoned(C, 1, torch.float32)
    ws = torch.full((swin.layernorm_workspace_bytes(T, C) // 4,), float("nan"), device="cuda") if want_gamma or want_beta else None
    _lib.check(_lib.load().msda_swin_layernorm_backward_bf16(dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                             add.data_ptr() if add is not None else None, T, C, dx.ptr(),
                                                             dg.ptr() if want_gamma else None, db.ptr() if want_beta else None,
                                                             ws.data_ptr() if ws is not None else None, _lib.raw_stream(x.device)))
    res = {"dx": dx.result("dx")}
    if want_gamma:
        res["dgamma"] = dg.result("dgamma")[:, 0]
    if want_beta:
        res["dbeta"] = db.result("dbeta")[:, 0]
    return res


def _dev(*ts):
    return [t.cuda().contiguous() if t is not None else None for t in ts]


def _inside(tag, got, val, bound):
    res = R.ratios(got, val, bound)
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)
    assert res and all(r <= 1.0 for r in res.values()), (tag, res)
    return res


# ---- linear ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
@pytest.mark.parametrize("K, N", KN)
def test_linear_is_inside_the_bounds(K, N, epilogue):
    for T in TOKENS:
        gen = torch.Generator().manual_seed(100 * epilogue + T + K + N)
        x, w, bias, aux = R.linear_inputs(T, K, N, epilogue, gen)
        if epilogue == 3:
            bias = None
        val, bound = R.linear_reference(x, w, bias, aux, epilogue)
        got = call_linear(*_dev(x, w, bias, aux), epilogue, want_out2=epilogue in (1, 3))
        assert sorted(got) == sorted(val)
        _inside(f"linear epilogue {epilogue} {(T, K, N)}", got, val, bound)


@pytest.mark.parametrize("epilogue", [0, 1, 2, 3])
def test_linear_wide_tiles_are_inside_the_bounds(epilogue):
    """N % 128 == 0 and ceil(400 / 128) * 8192 / 128 = 256 >= 128 workgroups: the 128-channel tiles (every shape above takes the 64-channel ones)"""
    T, K, N = 400, 96, 8192
    gen = torch.Generator().manual_seed(50 + epilogue)
    x, w, bias, aux = R.linear_inputs(T, K, N, epilogue, gen)
    val, bound = R.linear_reference(x, w, bias, aux, epilogue)
    got = call_linear(*_dev(x, w, bias, aux), epilogue, want_out2=epilogue in (1, 3))
    _inside(f"linear wide epilogue {epilogue} {(T, K, N)}", got, val, bound)


def test_linear_without_bias_and_without_out2():
    gen = torch.Generator().manual_seed(9)
    x, w, _, _ = R.linear_inputs(17, 96, 96, 1, gen)
    val, bound = R.linear_reference(x, w, None, None, 1)
    got = call_linear(*_dev(x, w, None, None), 1, want_out2=False)
    assert sorted(got) == ["out"]
    _inside("linear epilogue 1, no bias, out2 NULL", got, val, bound)


def test_gelu_backward_from_the_stored_preactivation():
    """the chain fc1 -> (u stored) -> epilogue 3 against the float64 chain on the exact pre-activation: the `moved` term of the bound"""
    gen = torch.Generator().manual_seed(7)
    x, w1, b1, _ = R.linear_inputs(70, 96, 384, 1, gen)
    dy, w2t, _, _ = R.linear_inputs(70, 96, 384, 0, gen)
    fwd, fwd_bound = R.linear_reference(x, w1, b1, None, 1)
    xd, w1d, b1d, dyd, w2d = _dev(x, w1, b1, dy, w2t)
    u = call_linear(xd, w1d, b1d, None, 1, want_out2=True)["out2"].contiguous()
    val, bound = R.linear_reference(dy, w2t, None, fwd["out2"], 3, moved=fwd_bound["out2"])
    got = call_linear(dyd, w2d, None, u, 3, want_out2=False)
    _inside("gelu backward from the stored u", got, {"out": val["out"]}, bound)


# ---- exact probes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K, N", [(96, 384), (2112, 32), (160, 8192)])
def test_one_hot_rows_return_the_weight_columns_bit_for_bit(K, N):
    """x[t] = e_k with k = (5 t + 3) mod K, T >= K tokens (for (160, 8192): 400 tokens, the 128-channel tiles): out[t, n] = rnd(w[n, k] + bias[n])
    in fp32 -- pins the fragment and index maps of both operands, the k blocks and the channel permutation of the store"""
    T = max(K, 400 if N == 8192 else 0)
    gen = torch.Generator().manual_seed(K + N)
    _, w, bias, _ = R.linear_inputs(1, K, N, 0, gen)
    k = (5 * torch.arange(T) + 3) % K
    x = torch.zeros(T, K, dtype=BF)
    x[torch.arange(T), k] = 1
    got = call_linear(*_dev(x, w, bias, None), 0, want_out2=False)["out"]
    want = (w.float()[:, k].t() + bias[None]).to(BF)
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_zero_weight_residual_returns_aux_bit_for_bit():
    gen = torch.Generator().manual_seed(2)
    x, w, bias, aux = R.linear_inputs(129, 160, 224, 2, gen)
    got = call_linear(*_dev(x, torch.zeros_like(w), torch.zeros_like(bias), aux), 2, want_out2=False)["out"]
    assert torch.equal(got.cpu().view(torch.int16), aux.view(torch.int16))


def test_constant_rows_through_the_layernorm_return_beta():
    gen = torch.Generator().manual_seed(3)
    for C in (96, 1536):
        x = (torch.randn(70, 1, generator=gen) * 3).to(BF).expand(70, C).contiguous()
        gamma, beta = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
        got = call_layernorm(*_dev(x, gamma, beta))
        assert torch.equal(got["out"].cpu().view(torch.int16), beta.to(BF).expand(70, C).contiguous().view(torch.int16))
        assert torch.equal(got["mean"].cpu(), x[:, 0].float())


def test_gelu_backward_regenerates_the_forward_activation_bit_for_bit():
    gen = torch.Generator().manual_seed(4)
    x, w, bias, _ = R.linear_inputs(129, 96, 384, 1, gen)
    xd, wd, bd = _dev(x, w, bias)
    fwd = call_linear(xd, wd, bd, None, 1, want_out2=True)
    dy, w2, _, _ = R.linear_inputs(129, 96, 384, 0, gen)
    bwd = call_linear(*_dev(dy, w2), None, fwd["out2"].contiguous(), 3, want_out2=True)
    assert torch.equal(bwd["out2"].view(torch.int16), fwd["out"].view(torch.int16))


def test_zero_gradient_gives_exact_zeros_and_passes_add_through():
    gen = torch.Generator().manual_seed(5)
    x, _, add, gamma, beta = R.layernorm_inputs(200, 96, gen)
    xd, addd, gd, bd = _dev(x, add, gamma, beta)
    st = call_layernorm(xd, gd, bd)
    zero = torch.zeros_like(xd)
    got = call_layernorm_backward(zero, xd, st["mean"].contiguous(), st["rstd"].contiguous(), gd, addd)
    assert torch.equal(got["dx"], addd) and not bool(got["dgamma"].any()) and not bool(got["dbeta"].any())
    got = call_layernorm_backward(zero, xd, st["mean"].contiguous(), st["rstd"].contiguous(), gd, None)
    assert not bool(got["dx"].any())


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 96, 1536, 4096])
def test_layernorm_forward_and_backward_are_inside_the_bounds(C):
    """200 tokens: four 64-token partial rows reach the fixed-order sum of dgamma / dbeta (1 and 70: one and two)"""
    for T in (1, 70, 200):
        gen = torch.Generator().manual_seed(T + C)
        x, dy, add, gamma, beta = R.layernorm_inputs(T, C, gen)
        xd, dyd, addd, gd, bd = _dev(x, dy, add, gamma, beta)
        val, bound = R.layernorm_reference(x, gamma, beta, 1e-5)
        got = call_layernorm(xd, gd, bd)
        _inside(f"layernorm {(T, C)}", got, val, bound)
        alone = call_layernorm(xd, gd, bd, stats=False)
        assert sorted(alone) == ["out"] and torch.equal(alone["out"].view(torch.int16), got["out"].view(torch.int16))
        mean, rstd = got["mean"].contiguous(), got["rstd"].contiguous()
        for a, ad in ((add, addd), (None, None)):
            val, bound = R.layernorm_backward_reference(dy, x, gamma, a, 1e-5)
            full = call_layernorm_backward(dyd, xd, mean, rstd, gd, ad)
            assert sorted(full) == ["dbeta", "dgamma", "dx"]
            _inside(f"layernorm backward {(T, C)} add={a is not None}", full, val, bound)
            for wg, wb in ((False, False), (True, False), (False, True)):
                part = call_layernorm_backward(dyd, xd, mean, rstd, gd, ad, want_gamma=wg, want_beta=wb)
                assert sorted(part) == sorted(["dx"] + ["dgamma"] * wg + ["dbeta"] * wb)
                for k, v in part.items():      # (the same kernels: the same bits)
                    assert torch.equal(v.view(torch.int32 if v.dtype == torch.float32 else torch.int16),
                                       full[k].view(torch.int32 if v.dtype == torch.float32 else torch.int16)), k


# ---- swin_mlp --------------------------------------------------------------------------------------------------------------------------
def _mlp_modules(C, hidden, seed):
    torch.manual_seed(seed)
    norm, fc1, fc2 = torch.nn.LayerNorm(C), torch.nn.Linear(C, hidden), torch.nn.Linear(hidden, C)
    with torch.no_grad():
        norm.weight.add_(0.3 * torch.randn(C))
        norm.bias.add_(0.3 * torch.randn(C))
    return norm.cuda(), fc1.cuda(), fc2.cuda()


def _mlp_run(x, dout, mods):
    from richsem_amd import swin
    for m in mods:
        m.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    out = swin.swin_mlp(xr, *mods)
    out.backward(dout)
    return [out.detach(), xr.grad] + [p.grad for m in mods for p in m.parameters()]


@pytest.mark.parametrize("T, C, hidden", [(1100, 128, 512), (70, 96, 384)])
def test_swin_mlp_is_reproducible_and_matches_the_torch_composition(T, C, hidden):
    """two calls, the same bits in the output and in every gradient ((1100, 128, 512) takes the library's weight-gradient kernel, the other the
    transposed GEMM); and the function against autograd through the torch ops in float32 on the same bf16-rounded parameters"""
    mods = _mlp_modules(C, hidden, T)
    gen = torch.Generator().manual_seed(T)
    x, dout = torch.randn(2, T // 2, C, generator=gen).to(BF).cuda(), torch.randn(2, T // 2, C, generator=gen).to(BF).cuda()
    first, second = _mlp_run(x, dout, mods), _mlp_run(x, dout, mods)
    assert len(first) == 8
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and torch.equal(a.view(-1).view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                                  b.view(-1).view(torch.int32 if b.dtype == torch.float32 else torch.int16))
    norm, fc1, fc2 = mods
    w = [p.detach().to(BF).float().requires_grad_(True) if p.dim() == 2 else p.detach().clone().requires_grad_(True)
         for p in (norm.weight, norm.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias)]
    xr = x.float().requires_grad_(True)
    h = torch.nn.functional.layer_norm(xr, (C,), w[0], w[1], norm.eps)
    ref = xr + torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(h, w[2], w[3])), w[4], w[5])
    ref.backward(dout.float())
    for name, got, want in zip(("out", "dx", "dgamma", "dbeta", "dw1", "db1", "dw2", "db2"), first, [ref.detach(), xr.grad] + [t.grad for t in w]):
        assert got.dtype == (BF if name in ("out", "dx") else torch.float32), name
        err = float((got.float() - want).pow(2).mean().sqrt()) / float(want.pow(2).mean().sqrt())
        if REPORT:
            print(f"[measured] swin_mlp {(T, C, hidden)} {name} relative rms error {err:.2e}", flush=True)
        assert err < 2.0 ** -7, (name, err)      # (rms over the tensor of a few bf16 roundings, each <= 2^-8 relative)


def test_swin_mlp_saves_one_hidden_wide_tensor_and_nothing_under_no_grad():
    from richsem_amd import swin
    C, hidden = 96, 384
    mods = _mlp_modules(C, hidden, 1)
    x = torch.randn(70, C).to(BF).cuda().requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        out = swin.swin_mlp(x, *mods)
    assert sum(1 for s in saved if s[-1] == hidden) == 1, saved
    assert sorted(saved) == sorted([(70, C), (70, C), (70,), (70,), (70, hidden), (C,)]), saved      # x, norm(x), mean, rstd, u, gamma
    saved.clear()
    with torch.no_grad(), torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        quiet = swin.swin_mlp(x, *mods)
    assert saved == [] and quiet.grad_fn is None
    assert torch.equal(quiet.view(torch.int16), out.detach().view(torch.int16))


def test_fused_block_raises_on_widths_outside_the_limits_instead_of_falling_back():
    from richsem_amd import swin
    blk = swin.SwinTransformerBlock(32, 1, window_size=4, mlp_ratio=1.5).to(BF).cuda()      # hidden 48: not a multiple of 32
    blk.fused, blk.H, blk.W = True, 4, 4
    with pytest.raises(RuntimeError, match="msda_swin_linear_bf16"):
        blk(torch.zeros(1, 16, 32, dtype=BF, device="cuda"))
    blk = swin.SwinTransformerBlock(32, 1, window_size=4, drop_path=0.25).to(BF).cuda()
    blk.fused, blk.H, blk.W = True, 4, 4
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        blk(torch.zeros(1, 16, 32, dtype=BF, device="cuda"))
    blk.eval()
    assert blk(torch.zeros(1, 16, 32, dtype=BF, device="cuda")).shape == (1, 16, 32)


# ---- the fixture with the fused blocks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2])
def test_basic_layer_fused_path_against_the_fixture(n):
    from richsem_amd import swin
    tag = f"layer{n}"
    H, W, w, nH = (int(v) for v in A.fixture()[f"{tag}.cfg"])
    sd = A.fixture_state_dict(tag, BF)
    layer = swin.BasicLayer(dim=32 * nH, depth=2, num_heads=nH, window_size=w, mlp_ratio=1., downsample=swin.PatchMerging).to(BF)
    layer.load_state_dict(sd, strict=True)
    layer.cuda().set_fused(True)
    x = A.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    x_out, _, _, x_down, _, _ = layer(x, H, W)
    _backward(tag, (x_out, x_down))
    kernel = _results(tag, (x_out, x_down), x, {k: p.grad for k, p in layer.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    xc = A.fixture_exact(f"{tag}.x", BF).cuda().requires_grad_(True)
    outs = comp_layer(P, "", xc, H, W, w, nH, True)
    _backward(tag, outs)
    _compare(tag, kernel, _results(tag, outs, xc, {k: p.grad for k, p in P.items()}))


def test_toy_backbone_fused_path_against_the_fixture():
    from richsem_amd import swin
    sd = A.fixture_state_dict("net", BF)
    net = swin.SwinTransformer(**NET).to(BF)
    net.load_state_dict(sd, strict=True)
    net.cuda().set_fused(True)
    img = A.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    feats = net.forward_raw(img)
    _backward("net", feats)
    kernel = _results("net", feats, img, {k: p.grad for k, p in net.named_parameters()})

    P = {k: v.cuda().requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point}
    imgc = A.fixture_exact("net.x", BF).cuda().requires_grad_(True)
    outs = comp_net(P, imgc)
    _backward("net", outs)
    _compare("net", kernel, _results("net", outs, imgc, {k: p.grad for k, p in P.items()}))
