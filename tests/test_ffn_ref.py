"""CPU: the feed-forward comparator itself (tests/ffn_ref.py).  Every emulation -- torch ops with the kernels' rounding points -- must stay
inside its element-wise bound on the inputs the GPU tests use (built by the same functions, at reduced token counts where the GPU case
is large only to turn a grid-stride loop over): the check that a correct kernel can meet the bounds of tests/test_gpu_ffn_bounds.py.
For the fused forward, three correct implementations (fp32, fp32 with every sum in a shuffled order, float64 arithmetic) must agree
with each other within the caps the GPU test holds the kernel to."""
import pytest
import torch

import ffn_ref as R

SEEDS = range(4)


def _small(T):
    return T if T <= 400 else 193 + T % 7


def _worst(worst, name, r, tag):
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, (tag, name, r)


@pytest.mark.parametrize("seed", SEEDS)
def test_fused_forward_emulations_stay_inside_the_bound_and_agree_within_the_caps(seed):
    worst, shares = {}, [0.0, 0, 0.0]
    cases = [(R.make_ffn(T, Fh, seed, regime), (T, Fh, regime)) for T, Fh, regime in R.FFN_CASES]
    cases += [(R.make_live_unit(49, 160, j, (7 * j + 3) % 256, seed), ("live", j)) for j in R.LIVE_UNITS]
    for p, tag in cases:
        T = p["x"].shape[0]
        val, bound = R.ffn_reference(**p)
        emus = [R.emulate_ffn(**p), R.emulate_ffn(**p, permute=torch.Generator().manual_seed(seed)), R.emulate_ffn(**p, dtype=torch.float64)]
        for e in emus:
            for n in ("out", "yhat", "rstd"):
                _worst(worst, n, R.ratio(e[n], val[n], bound[n]), tag)
        for i, j in ((0, 1), (0, 2), (1, 2)):
            for n in ("out", "yhat"):
                s = R.mismatch_shares(emus[i][n], emus[j][n])
                assert R.within_caps(s, T), (tag, n, i, j, s)
                shares = [max(shares[0], s[0]), max(shares[1], s[1]), max(shares[2], s[2] / max(T, 1))]
    print("[ffn emulation] worst |err| / bound:", {n: round(x, 3) for n, x in worst.items()},
          "worst shares (elements, channels of a token, tokens of a channel / T):", shares)


@pytest.mark.parametrize("T", (193, 1000))
def test_fused_forward_spread_between_correct_implementations(T):
    """The spread between three correct implementations on a wider grid than the GPU cases: d_ffn = 32 .. 4096, the four input regimes.
    The share of all elements and the tokens of a channel stay inside their caps with room (worst here: 0.33 % of 1 %, 12 of 20 at
    T = 1000).  The channels of ONE token do not at small d_ffn with large hidden activations: a single flipped h there has an ulp of
    2^-3 .. 2^-2 against the output's 2^-7 and moves up to 100 channels of its token (T = 1000: d_ffn = 96 at scale 30: 100, d_ffn = 32
    with offset 8: 94), so that figure is printed, not asserted -- cap (c) is a property of the GPU test's cases (asserted for their inputs
    above, worst 55 of 96), not of every input."""
    worst = [0.0, 0, 0]
    for Fh in (32, 96, 160, 256, 1024, 2048, 4096):
        for regime in R.REGIMES:
            p = R.make_ffn(T, Fh, 11, regime)
            emus = [R.emulate_ffn(**p), R.emulate_ffn(**p, permute=torch.Generator().manual_seed(T + Fh)), R.emulate_ffn(**p, dtype=torch.float64)]
            for i, j in ((0, 1), (0, 2), (1, 2)):
                for n in ("out", "yhat"):
                    s = R.mismatch_shares(emus[i][n], emus[j][n])
                    assert s[0] <= R.CAP_SHARE and s[2] <= R.cap_channel(T), (Fh, regime, n, s)
                    worst = [max(a, b) for a, b in zip(worst, s)]
    print(f"[ffn spread T={T}] share {worst[0]:.5f}, channels of a token {worst[1]}, tokens of a channel {worst[2]}")


@pytest.mark.parametrize("seed", SEEDS)
def test_add_layernorm_and_backward_emulations_stay_inside_their_bounds(seed):
    worst = {}
    for T in R.ALN_T:
        for regime in R.REGIMES:
            p = R.make_aln(_small(T), seed, regime)
            for b in (p["b"], None):
                val, bound = R.add_layernorm_reference(p["a"], b, p["gamma"], p["beta"])
                e = R.emulate_add_layernorm(p["a"], b, p["gamma"], p["beta"])
                for n in ("out", "yhat", "rstd"):
                    _worst(worst, "aln_" + n, R.ratio(e[n], val[n], bound[n]), (T, regime))
    for T in R.LNB_T:
        p = R.make_lnb(T, seed)
        a = R.make_aln(T, seed)
        fwd = R.emulate_add_layernorm(a["a"], a["b"], p["gamma"], a["beta"])
        for q in (p, dict(p, yhat=fwd["yhat"], rstd=fwd["rstd"])):
            val, bound = R.ln_backward_reference(**q)
            e = R.emulate_ln_backward(**q)
            for n in val:
                _worst(worst, "lnb_" + n, R.ratio(e[n], val[n], bound[n]), T)
    print("[ln emulation] worst |err| / bound:", {n: round(x, 3) for n, x in worst.items()})


@pytest.mark.parametrize("seed", SEEDS)
def test_lin256_emulations_stay_inside_their_bounds(seed):
    worst = {}
    for T, N in R.LIN_CASES + R.LIN_STACKED:
        p = R.make_lin(_small(T), N, seed)
        h = R.emulate_lin256(p["x"], p["w"], p["b"], 1)
        h[0] = R.mask_probe_row(N)
        for epi, b, mask in ((0, p["b"], None), (0, None, None), (1, p["b"], None), (1, None, None), (2, None, h), (3, p["b"], p["row_mask"]),
                             (3, None, p["row_mask"])):
            want, bound, zero = R.lin256_reference(p["x"], p["w"], b, epi, mask)
            _worst(worst, f"epi{epi}", R.ratio(R.emulate_lin256(p["x"], p["w"], b, epi, mask), want, bound, zero), (T, N, epi))
    for T, N in R.F32_CASES:
        for mixed in (False, True):
            p = R.make_f32(T, N, seed, mixed)
            for b in (p["b"], None):
                want, bound = R.lin256_f32_reference(p["x"], p["w"], b)
                _worst(worst, "f32_mixed" if mixed else "f32", R.ratio(R.emulate_lin256_f32(p["x"], p["w"], b), want, bound), (T, N))
        p = R.exact_f32_probe(T, N, seed)
        want, _ = R.lin256_f32_reference(**p)
        assert torch.equal(R.emulate_lin256_f32(**p).double(), want)
    print("[lin256 emulation] worst |err| / bound:", {n: round(x, 4) for n, x in worst.items()})


def test_references_are_the_torch_definitions():
    import torch.nn.functional as F
    p = R.make_ffn(70, 96, 3)
    d = {k: v.double() for k, v in p.items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in d.items()}
    y = leaves["x"] + F.linear(torch.relu(F.linear(leaves["x"], leaves["w1"], leaves["b1"])), leaves["w2"], leaves["b2"])
    y.retain_grad()
    out = F.layer_norm(y, (256,), leaves["gamma"], leaves["beta"], R.EPS)
    val, _ = R.ffn_reference(**p)
    assert float((val["out"] - out.detach()).abs().max()) < 1e-12
    dy = torch.randn(70, 256, generator=torch.Generator().manual_seed(1)).to(R.BF)
    out.backward(dy.double())
    bval, _ = R.ln_backward_reference(dy, val["yhat"], val["rstd"], p["gamma"])      # (float64 yhat / rstd: the definition, not the kernel's copy)
    for n, w in (("dz", y.grad), ("dgamma", leaves["gamma"].grad), ("dbeta", leaves["beta"].grad), ("db2", leaves["b2"].grad)):
        assert float((bval[n] - w).abs().max()) < 1e-11 * (1 + float(w.abs().max())), n
    a = R.make_aln(9, 1)
    aval, _ = R.add_layernorm_reference(**a)
    want = F.layer_norm(a["a"].double() + a["b"].double(), (256,), a["gamma"].double(), a["beta"].double(), R.EPS)
    assert float((aval["out"] - want).abs().max()) < 1e-12


def test_constant_rows_and_the_mask_probe_are_exact_in_the_emulation():
    a = torch.tensor([0.0, 1.0, -3.5, 1e4, 2.0 ** -20, 448.0], dtype=torch.float32).to(R.BF)[:, None].expand(6, 256).contiguous()
    g = torch.Generator().manual_seed(0)
    gamma, beta = R.signed_gamma(g), torch.randn(256, generator=g)
    e = R.emulate_add_layernorm(a, None, gamma, beta)
    assert bool((e["yhat"] == 0).all()) and torch.equal(e["out"], beta.to(R.BF).expand(6, 256))
    val, bound = R.add_layernorm_reference(a, None, gamma, beta)
    assert R.ratio(e["rstd"], val["rstd"], bound["rstd"]) <= 1.0 and float((val["rstd"] - R.EPS32 ** -0.5).abs().max()) < 1e-9
    row = R.mask_probe_row(8)
    assert (row > 0).tolist() == [False, False, True, False, False, True, False, True]


def test_bounds_reject_the_mutations_of_the_profile_note():
    """value-only changes of the emulations, each far outside its bound (or, for the forward, outside the caps): the CPU side of the mutation
    table in profiles/r17_ffn_bounds.md"""
    p = R.make_ffn(193, 256, 0)
    emu = R.emulate_ffn(**p)
    x, w1, b1, w2, b2 = (p[k].float() for k in ("x", "w1", "b1", "w2", "b2"))
    hf = torch.relu(x @ w1.t() + b1)
    y = R._r16(hf) @ w2.t() + (b2 + x)
    d = y - y.mean(-1, keepdim=True)
    # variance divided by 255
    r255 = torch.rsqrt((d * d).sum(-1, keepdim=True) / 255 + R.EPS)
    m = (d * r255).to(R.BF)
    assert not R.within_caps(R.mismatch_shares(m, emu["yhat"]), 193)
    # h truncated
    ht = (hf.view(torch.int32) & -65536).view(torch.float32)
    mt = R._ln_emulate(ht @ w2.t() + (b2 + x), p["gamma"], p["beta"], R.EPS)
    assert not R.within_caps(R.mismatch_shares(mt["out"], emu["out"]), 193)
    # LayerNorm backward without the mean_c(g) term; db2 as the sum of g
    q = R.make_lnb(193, 0)
    val, bound = R.ln_backward_reference(**q)
    dy, yh, r, ga = q["dy"].float(), q["yhat"].float(), q["rstd"][:, None], q["gamma"]
    g_ = dy * ga
    assert R.ratio((r * (g_ - yh * (g_ * yh).mean(-1, keepdim=True))).to(R.BF), val["dz"], bound["dz"]) > 1.0
    assert R.ratio(g_.sum(0), val["db2"], bound["db2"]) > 1.0
