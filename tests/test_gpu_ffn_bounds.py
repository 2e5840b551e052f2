"""GPU (-m gpu): the feed-forward family (richsem_amd/csrc/ffn_mfma.hip, lin256_mfma.hip) through the C ABI and richsem_amd.functions
against the float64 references and ELEMENT-WISE bounds of tests/ffn_ref.py (derived there, rounding by rounding), at the kernels' own
tile edges: 48 tokens per wave and 192 per workgroup, the three-slot weight ring wrapping, uneven splits of lin256's 64-channel blocks
over its workgroup rows, the first turn of the grid-stride loops of add_layernorm (16384 tokens) and ffn_ln_backward (2048).  The fused
forward is also held against a rounding-exact emulation by the count of differing bf16 bits (ffn_ref.CAP_*), exact probes pin
constant rows, every position class of the W2 permutation and the relu-mask comparison, and the three autograd functions are compared
with fp32 autograd and with themselves under subsets of requires_grad.  RICHSEM_REPORT=1 prints the worst |err| / bound per tensor and
case and the three shares (profiles/r17_ffn_bounds.md).

Inputs are built on the CPU by the functions tests/test_ffn_ref.py uses; the emulation of the fused forward runs on the CPU as there."""
import os

import pytest
import torch
import torch.nn.functional as F

import ffn_ref as R
from richsem_amd import _lib
from richsem_amd.functions import AddLayerNormFunction, FusedFFNFunction, pack_w2_bf16
from richsem_amd.functions import ffn as FFN_MOD
from richsem_amd.functions.ffn import FFNSmallFunction, FusedFFNCachedFunction, pack_ffn
from richsem_amd.functions.linear import lin256, lin256_f32, lin256_f32_pack, lin256_pack, pack_linear256

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
POISON = 7.0            # bf16 / fp32 values no case here computes: rows past `tokens` must keep them
PAD = 5
REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(p):
    return {k: v.cuda() for k, v in p.items()}


def _say(tag, **kv):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()), flush=True)


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ---- fused forward ------------------------------------------------------------------------------------------------------------------------
def _ffn_launch(p, eps=R.EPS):
    """msda_ffn_forward_train_bf16 on CPU inputs `p` into buffers PAD rows too long -> CPU {"out", "yhat", "rstd"}; the tail keeps its poison"""
    d = _cuda(p)
    T, Fh = d["x"].shape[0], d["w1"].shape[0]
    out = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF)
    yhat = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF)
    rstd = torch.full((T + PAD,), POISON, device="cuda", dtype=torch.float32)
    w2p = pack_w2_bf16(d["w2"].contiguous())
    _lib.check(_lib.load().msda_ffn_forward_train_bf16(
        d["x"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(), w2p.data_ptr(), d["b2"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
        eps, T, 256, Fh, out.data_ptr(), rstd.data_ptr(), yhat.data_ptr(), _stream()))
    torch.cuda.synchronize()
    for t in (out, yhat, rstd):
        assert bool((t[T:] == POISON).all()), "rows past `tokens` were written"
    out2 = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF)      # the inference entry point: the same kernel without rstd / yhat
    _lib.check(_lib.load().msda_ffn_forward_bf16(
        d["x"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(), w2p.data_ptr(), d["b2"].data_ptr(), d["gamma"].data_ptr(), d["beta"].data_ptr(),
        eps, T, 256, Fh, out2.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    return {"out": out[:T].cpu(), "yhat": yhat[:T].cpu(), "rstd": rstd[:T].cpu()}


def _ffn_check(tag, p):
    """(a) every element inside the worst-case bound; (b)-(d) bits against the emulation within the caps"""
    T = p["x"].shape[0]
    got = _ffn_launch(p)
    val, bound = R.ffn_reference(**p)
    emu = R.emulate_ffn(**p)
    r = {n: R.ratio(got[n], val[n], bound[n]) for n in ("out", "yhat", "rstd")}
    s = {n: R.mismatch_shares(got[n], emu[n]) for n in ("out", "yhat")}
    if REPORT:
        e = {n: R.ratio(emu[n], val[n], bound[n]) for n in r}
        print(f"[measured] {tag} " + " ".join(f"{n}={r[n]:.3f}/{e[n]:.3f}" for n in r) +
              " " + " ".join(f"{n}_shares={s[n][0]:.5f},{s[n][1]},{s[n][2]}" for n in s), flush=True)
    for n in r:
        assert r[n] <= 1.0, (tag, n, r[n])
    for n in s:
        assert s[n][0] <= R.CAP_SHARE, (tag, n, "share of all elements", s[n])
        assert s[n][1] <= R.CAP_TOKEN, (tag, n, "channels of one token", s[n])
        assert s[n][2] <= R.cap_channel(T), (tag, n, "tokens of one channel", s[n])
    return got


@pytest.mark.parametrize("T,Fh,regime", R.FFN_CASES)
def test_fused_forward_elementwise_and_against_the_emulation(T, Fh, regime):
    _ffn_check(f"ffn T={T} F={Fh} {regime}", R.make_ffn(T, Fh, 0, regime))


def test_fused_forward_constant_rows_are_exact():
    """w2 = 0, b2 = 0, every token one bf16 value: yhat == 0, out == bf16(beta), rstd = eps^-1/2 within its bound"""
    p = R.make_ffn(193, 160, 1)
    vals = torch.tensor([0.0, 1.0, -3.5, 1e4, 2.0 ** -20, 448.0, -0.0078125], dtype=torch.float32).to(BF)
    p["x"] = vals[torch.arange(193) % len(vals)][:, None].expand(193, 256).contiguous()
    p["w2"], p["b2"] = torch.zeros_like(p["w2"]), torch.zeros_like(p["b2"])
    got = _ffn_launch(p)
    assert bool((got["yhat"] == 0).all())
    assert torch.equal(got["out"], p["beta"].to(BF).expand(193, 256))
    val, bound = R.ffn_reference(**p)
    assert float((val["rstd"] - R.EPS32 ** -0.5).abs().max()) < 1e-9
    r = R.ratio(got["rstd"], val["rstd"], bound["rstd"])
    _say("ffn constant rows", rstd=r)
    assert r <= 1.0


@pytest.mark.parametrize("j", R.LIVE_UNITS)
def test_fused_forward_one_live_hidden_unit(j):
    """y = x + b2 + w2[:, j] relu(x_k): one product per channel, so hidden unit j of the packed W2 and its ring slot are pinned"""
    k = (7 * j + 3) % 256
    p = R.make_live_unit(49, 160, j, k, 0)
    got = _ffn_check(f"ffn live unit j={j}", p)
    # and directly: the one-product y through a float64 LayerNorm, against which a neighbouring column of W2 is far off
    x, w2 = p["x"].double(), p["w2"].double()
    y = x + p["b2"].double() + w2[:, j][None, :] * torch.relu(x[:, k])[:, None]
    want = F.layer_norm(y, (256,), p["gamma"].double(), p["beta"].double(), R.EPS)
    assert float((got["out"].double() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())


# ---- add_layernorm ------------------------------------------------------------------------------------------------------------------------
def _aln_launch(a, b, gamma, beta, T, want_rstd=True, want_yhat=True, eps=R.EPS):
    out = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF)
    yhat = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF) if want_yhat else None
    rstd = torch.full((T + PAD,), POISON, device="cuda", dtype=torch.float32) if want_rstd else None
    _lib.check(_lib.load().msda_add_layernorm_forward_bf16(a.data_ptr(), _ptr(b), gamma.data_ptr(), beta.data_ptr(), eps, T, 256, out.data_ptr(),
                                                           _ptr(rstd), _ptr(yhat), _stream()))
    torch.cuda.synchronize()
    for t in (out, yhat, rstd):
        assert t is None or bool((t[T:] == POISON).all()), "rows past `tokens` were written"
    return {"out": out[:T], "yhat": yhat[:T] if want_yhat else None, "rstd": rstd[:T] if want_rstd else None}


@pytest.mark.parametrize("T", R.ALN_T)
def test_add_layernorm_elementwise(T):
    for regime in R.REGIMES:
        p = _cuda(R.make_aln(T, 0, regime))
        for b in (p["b"], None):      # (b == NULL: LayerNorm(a))
            got = _aln_launch(p["a"], b, p["gamma"], p["beta"], T)
            val, bound = R.add_layernorm_reference(p["a"], b, p["gamma"], p["beta"])
            r = {n: R.ratio(got[n], val[n], bound[n]) for n in ("out", "yhat", "rstd")}
            _say(f"aln T={T} {regime} b={'yes' if b is not None else 'NULL'}", **r)
            for n in r:
                assert r[n] <= 1.0, (T, regime, b is None, n, r[n])
        if regime == "plain":      # without rstd and / or yhat: the other outputs unchanged
            for wr, wy in ((False, True), (True, False), (False, False)):
                part = _aln_launch(p["a"], None, p["gamma"], p["beta"], T, wr, wy)
                for n in ("out", "yhat", "rstd"):
                    assert part[n] is None or torch.equal(part[n], got[n]), (T, wr, wy, n)


@pytest.mark.parametrize("T", (5, 16389))
def test_add_layernorm_constant_rows_are_exact(T):
    vals = torch.tensor([0.0, 1.0, -3.5, 1e4, 2.0 ** -20, 448.0, -0.0078125], dtype=torch.float32).to(BF)
    a = vals[torch.arange(T) % len(vals)][:, None].expand(T, 256).contiguous().cuda()
    g = torch.Generator().manual_seed(T)
    gamma, beta = R.signed_gamma(g).cuda(), torch.randn(256, generator=g).cuda()
    for b in (None, torch.zeros_like(a)):
        got = _aln_launch(a, b, gamma, beta, T)
        assert bool((got["yhat"] == 0).all()) and torch.equal(got["out"], beta.to(BF).expand(T, 256))
        val, bound = R.add_layernorm_reference(a, b, gamma, beta)
        assert R.ratio(got["rstd"], val["rstd"], bound["rstd"]) <= 1.0


# ---- ffn_ln_backward ----------------------------------------------------------------------------------------------------------------------
def _lnb_launch(dy, yhat, rstd, gamma, T):
    dz = torch.full((T + PAD, 256), POISON, device="cuda", dtype=BF)
    sums = torch.full((3, 256), 1e6, device="cuda", dtype=torch.float32)      # poisoned: overwritten, not added to
    _lib.check(_lib.load().msda_ffn_ln_backward_bf16(dy.data_ptr(), yhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), T, 256, dz.data_ptr(),
                                                     sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert bool((dz[T:] == POISON).all())
    return {"dz": dz[:T], "dgamma": sums[0], "dbeta": sums[1], "db2": sums[2]}


@pytest.mark.parametrize("T", R.LNB_T)
def test_ln_backward_elementwise(T):
    p = _cuda(R.make_lnb(T, 0))
    a = _cuda(R.make_aln(T, 0))
    fwd = _aln_launch(a["a"], a["b"], p["gamma"], a["beta"], T)      # (the yhat and rstd the backward really gets)
    for kind, q in (("synthetic", p), ("from add_layernorm", dict(p, yhat=fwd["yhat"].contiguous(), rstd=fwd["rstd"].contiguous()))):
        got = _lnb_launch(q["dy"], q["yhat"], q["rstd"], q["gamma"], T)
        val, bound = R.ln_backward_reference(**q)
        r = {n: R.ratio(got[n], val[n], bound[n]) for n in val}
        _say(f"lnb T={T} {kind}", **r)
        for n in r:
            assert r[n] <= 1.0, (T, kind, n, r[n])
        assert all(bool(torch.isfinite(got[n].float()).all()) for n in got)


# ---- lin256 -------------------------------------------------------------------------------------------------------------------------------
def _lin_configs(p, N):
    h = R.emulate_lin256(p["x"], p["w"], p["b"], 1)      # a ReLU output as the mask, as the backward has it ...
    h[0] = R.mask_probe_row(N).to(h.device)               # ... and one row of the edge values
    return ((0, p["b"], None), (0, None, None), (1, p["b"], None), (1, None, None), (2, None, h), (3, p["b"], p["row_mask"]),
            (3, None, p["row_mask"]))


@pytest.mark.parametrize("T,N", R.LIN_CASES)
def test_lin256_every_epilogue_elementwise(T, N):
    p = _cuda(R.make_lin(T, N, 0))
    wp = lin256_pack(p["w"])
    base = R.lin256_base(p["x"], p["w"])
    for epi, b, mask in _lin_configs(p, N):
        got = lin256(p["x"], wp, b, relu=epi == 1, relu_mask=mask if epi == 2 else None, row_mask=mask if epi == 3 else None)
        want, bound, zero = R.lin256_reference(p["x"], p["w"], b, epi, mask, base=base)
        assert got.dtype == BF and tuple(got.shape) == (T, N)
        assert bool((got[zero] == 0).all()), (T, N, epi, "masked elements are not exactly zero")
        r = R.ratio(got, want, bound, zero)
        _say(f"lin256 T={T} N={N} epi={epi} bias={'yes' if b is not None else 'no'}", ratio=r)
        assert r <= 1.0, (T, N, epi, b is not None, r)


@pytest.mark.parametrize("T,N", R.LIN_STACKED)
def test_lin256_stacked_layout(T, N):
    p = _cuda(R.make_lin(T, N, 1))
    wp = lin256_pack(p["w"])
    base = R.lin256_base(p["x"], p["w"])
    nl = N // 256
    for row_mask in (None, p["row_mask"]):
        out = torch.full((nl * T * 256 + 256,), POISON, device="cuda", dtype=BF)
        m8 = row_mask.contiguous().view(torch.uint8) if row_mask is not None else None
        _lib.check(_lib.load().msda_lin256_forward_stacked_bf16(p["x"].data_ptr(), wp.data_ptr(), p["b"].data_ptr(), _ptr(m8), T, 256, N,
                                                                out.data_ptr(), _stream()))
        torch.cuda.synchronize()
        assert bool((out[nl * T * 256:] == POISON).all())
        got = out[:nl * T * 256].view(nl, T, 256).permute(1, 0, 2).reshape(T, N)      # layer l's (T, 256) matrix = columns 256 l ..
        want, bound, zero = R.lin256_reference(p["x"], p["w"], p["b"], 3 if row_mask is not None else 0, row_mask, base=base)
        assert bool((got[zero] == 0).all())
        r = R.ratio(got, want, bound, zero)
        _say(f"lin256 stacked T={T} N={N} row_mask={'yes' if row_mask is not None else 'no'}", ratio=r)
        assert r <= 1.0, (T, N, r)


def test_relu_mask_is_mask_greater_than_zero():
    """epilogue 2 on +0, -0, the bf16 subnormals, NaN, the infinities and 1: non-zero exactly where torch's `mask > 0` is true on the CPU; the
    op-by-op branch of FusedFFNFunction's backward computes the same"""
    T, N = 50, 192
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(T, 256, generator=g) + 0.5).to(BF)      # positive operands: every unmasked product is > 0
    w = ((torch.rand(N, 256, generator=g) + 0.5) / 16).to(BF)
    probe = R.mask_probe_row(N + T)
    mask = torch.stack([probe[t:t + N] for t in range(T)]).contiguous()      # every column meets every value
    keep = mask > 0                                                          # on the CPU
    assert 0.3 < float(keep.float().mean()) < 0.45 and bool(torch.isnan(mask.float()).any())
    got = lin256(x.cuda(), lin256_pack(w.cuda()), relu_mask=mask.cuda()).cpu()
    assert torch.equal(got != 0, keep)
    assert bool(torch.isfinite(got.float()).all())
    plain = lin256(x.cuda(), lin256_pack(w.cuda())).cpu()
    assert torch.equal(got[keep], plain[keep])
    op_by_op = FFN_MOD.relu_input_grad(x.cuda() @ w.cuda().t(), mask.cuda()).cpu()
    assert torch.equal(op_by_op != 0, keep) and bool(torch.isfinite(op_by_op.float()).all())


# ---- lin256_f32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N", R.F32_CASES)
def test_lin256_f32_elementwise(T, N):
    for mixed in (False, True):
        p = _cuda(R.make_f32(T, N, 0, mixed))
        wp = lin256_f32_pack(p["w"])
        for b in (p["b"], None):
            got = lin256_f32(p["x"], wp, N, b)
            want, bound = R.lin256_f32_reference(p["x"], p["w"], b)
            r = R.ratio(got, want, bound)
            _say(f"lin256_f32 T={T} N={N} mixed={int(mixed)} bias={'yes' if b is not None else 'no'}", ratio=r)
            assert got.dtype == torch.float32 and r <= 1.0, (T, N, mixed, r)
    p = _cuda(R.exact_f32_probe(T, N, 0))      # every product and partial sum exact in fp32: the result is the float64 one
    want, _ = R.lin256_f32_reference(**p)
    got = lin256_f32(p["x"], lin256_f32_pack(p["w"]), N, p["b"])
    assert torch.equal(got.double(), want), (T, N, float((got.double() - want).abs().max()))


# ---- the autograd functions -----------------------------------------------------------------------------------------------------------------
NAMES = ("x", "w1", "b1", "w2", "b2", "ln_w", "ln_b")


def _ref_grads(p, go):
    refl = [p[k].cuda().float().clone().requires_grad_(True) for k in ("x", "w1", "b1", "w2", "b2", "gamma", "beta")]
    x, w1, b1, w2, b2, gw, gb = refl
    F.layer_norm(x + F.linear(torch.relu(F.linear(x, w1, b1)), w2, b2), (256,), gw, gb, R.EPS).backward(go.float())
    return [t.grad for t in refl]


def _compare_with_fp32_autograd(grads, ref, tag):
    """the tolerances of test_gpu_ffn.py::test_function_gradients_match_fp32_autograd"""
    for a, b, name in zip(grads, ref, NAMES):
        err = (a.float() - b).abs()
        mx, mean = float(err.max()) / (float(b.abs().max()) + 1e-12), float(err.mean()) / (float(b.abs().mean()) + 1e-12)
        _say(f"{tag} grad {name}", max=mx, mean=mean)
        assert mx < 0.15, (tag, name, mx)
        assert mean < 2e-2, (tag, name, mean)


def _small_apply(p):
    """-> (run, leaves): FFNSmallFunction on bf16 x and float32 master parameters, packs from pack_linear256 and lin256_pack"""
    d = _cuda(p)
    leaves = [d["x"].clone()] + [d[k].float().clone() for k in ("w1", "b1", "w2", "b2", "gamma", "beta")]
    pk1 = pack_linear256([leaves[1]], [leaves[2]])
    w2_16 = leaves[3].to(BF).contiguous()
    w2t = lin256_pack(w2_16.t().contiguous())
    return (lambda: FFNSmallFunction.apply(leaves[0], pk1, w2_16, w2t, R.EPS, *leaves[1:])), leaves


def _cached_apply(p):
    d = _cuda(p)
    leaves = [d["x"].clone()] + [d[k].float().clone() for k in ("w1", "b1", "w2", "b2", "gamma", "beta")]
    pk = pack_ffn(leaves[1], leaves[2], leaves[3])
    return (lambda: FusedFFNCachedFunction.apply(leaves[0], pk, R.EPS, *leaves[1:])), leaves


def _fused_apply(p):
    d = _cuda(p)
    leaves = [d[k].clone() for k in ("x", "w1", "b1", "w2", "b2", "gamma", "beta")]
    return (lambda: FusedFFNFunction.apply(*leaves, R.EPS)), leaves


def _grads(make, p, go, wanted):
    run, leaves = make(p)
    for i, t in enumerate(leaves):
        t.requires_grad_(i in wanted)
    run().backward(go)
    torch.cuda.synchronize()
    return [t.grad for t in leaves]


def _go(T, seed=9):
    return torch.randn(T, 256, generator=torch.Generator().manual_seed(seed)).to(BF).cuda()


@pytest.mark.parametrize("T,Fh", [(193, 256), (47, 2048)])
def test_small_function_gradients_match_fp32_autograd(T, Fh):
    p, go = R.make_ffn(T, Fh, 3), _go(T)
    _compare_with_fp32_autograd(_grads(_small_apply, p, go, range(7)), _ref_grads(p, go), f"FFNSmallFunction T={T} F={Fh}")


def test_cached_function_gradients_match_fp32_autograd():
    p, go = R.make_ffn(193, 128, 3), _go(193)
    _compare_with_fp32_autograd(_grads(_cached_apply, p, go, range(7)), _ref_grads(p, go), "FusedFFNCachedFunction T=193 F=128")


@pytest.mark.parametrize("name,make,T,Fh", [("fused", _fused_apply, 193, 128), ("fused_op_by_op", _fused_apply, 193, 96),
                                            ("cached", _cached_apply, 193, 128), ("small", _small_apply, 193, 256)])
def test_gradients_under_subsets_of_requires_grad(name, make, T, Fh):
    """input only, and weights frozen: the gradients still wanted equal the full run's bit for bit -- except the three token sums
    (ln_w, ln_b, b2), which ffn_ln_backward adds up with atomics in an order that is not fixed (ffn_ref: B_sum): two runs are each
    within B_sum of the exact sum, so within 2 B_sum of each other (B_sum from the float64 forward; 1.05 for the difference between
    its yhat and the kernel's bf16 copy)"""
    p, go = R.make_ffn(T, Fh, 4), _go(T, 10)
    full = _grads(make, p, go, range(7))
    val, _ = R.ffn_reference(**p)
    _, bound = R.ln_backward_reference(go.cpu(), val["yhat"], val["rstd"], p["gamma"])
    sums = {4: bound["db2"], 5: bound["dgamma"], 6: bound["dbeta"]}
    for wanted in ((0,), (0, 2, 4, 5, 6)):
        got = _grads(make, p, go, wanted)
        for i, n in enumerate(NAMES):
            if i not in wanted:
                assert got[i] is None, (name, wanted, n)
            elif i in sums:
                diff = (got[i].double() - full[i].double()).abs().cpu()
                _say(f"subset {name} {wanted} {n}", bit_equal=bool(torch.equal(got[i], full[i])), ratio=float((diff / (2.1 * sums[i])).max()))
                assert bool((diff <= 2.1 * sums[i]).all()), (name, wanted, n)
            else:
                assert torch.equal(got[i], full[i]), (name, wanted, n)


def test_add_layernorm_function_with_frozen_parameters():
    """AddLayerNormFunction with only the inputs wanting gradients: the same dz, bit for bit"""
    a = _cuda(R.make_aln(193, 2))
    go = _go(193, 11)
    res = []
    for params in (True, False):
        a1, b1 = a["a"].clone().requires_grad_(True), a["b"].clone().requires_grad_(True)
        w, bi = a["gamma"].clone().requires_grad_(params), a["beta"].clone().requires_grad_(params)
        AddLayerNormFunction.apply(a1, b1, w, bi, R.EPS).backward(go)
        res.append((a1.grad, b1.grad, w.grad, bi.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[1][2] is None and res[1][3] is None
