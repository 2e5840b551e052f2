"""Float64 definitions of what csrc/swin_block_mfma.hip writes (richsem_amd.swin: linear_kernel, layernorm_kernel, layernorm_backward_kernel)
with an ELEMENT-WISE error bound per tensor, an fp32 emulation of the kernels' roundings and wrong variants that must leave the bounds.
Test helper only: the package never imports it.

Inputs are the stored values (bf16 activations and weights, fp32 bias / gamma / beta), so their float64 copies are exact.

    linear      acc = x (T, K) . w (N, K)^T
       epilogue 0   out = acc + bias                                   2   out = acc + bias + aux
       epilogue 1   u = acc + bias (out2),  out = gelu(u)              3   out = acc gelu'(aux),  out2 = gelu(aux)
       gelu(x) = x Phi(x),  gelu'(x) = Phi(x) + x phi(x)   (the erf form of nn.GELU())
    layernorm   mean, var = biased moments over C,  rstd = (var + eps)^-1/2,  xhat = (x - mean) rstd,  out = xhat gamma + beta
    backward    g = dy gamma,  dx = add + rstd (g - mean_c(g) - xhat mean_c(g xhat)),  dgamma = sum_t dy xhat,  dbeta = sum_t dy
                (mean, rstd here are the float64 moments of x: the kernel is handed fp32 statistics, which moves its xhat)

The bounds.  u = 2^-8 is the unit round-off of bf16, e = 2^-24 that of fp32; every stored bf16 element is rounded ONCE, at its store.

  linear    an fp32 accumulation of K products in any order, followed by the epilogue's additions, is off by at most
                E_lin = (K + 2) e (|x| |w|^T + |bias| + |aux|)
            (K reaches 6144 in a Swin-L MLP: K e is 2^-11.4 there, so a constant in place of K would not carry over from the attention's
            bounds), and the store rounds:          B_0 = B_2 = B_u = u |value| + (1 + u) E_lin
  epilogue 1   out = rnd(gelu(u_stored)): the operand MOVED by B_u, |gelu'| <= 1.13 = L; erfc and the product in fp32 cost a few ulp, 2^-20
            = 16 e is taken:                        B_1 = L B_u + (u + 2^-20) (|gelu(u)| + L B_u)
  epilogue 3   aux is an input here (exact).  gelu' in fp32 (erfc, exp, two products, one sum, each term <= 1): 2^-20 absolute.
                                                    B_3 = u |value| + (1 + u) ((K + 2) e (|x| |w|^T) |gelu'(aux)| + 2^-20 |acc|)  [+ |acc| M d]
            where the bracket applies when aux is the STORED u of an epilogue 1 and the definition uses the exact pre-activation: the
            operand moved by d = B_u and |gelu''| <= 0.8 = M (`moved=`).           B_3' (out2) = (u + 2^-20) |gelu(aux)|
  layernorm    fp32 sums over C in any order:  B_mean = (C + 1) e mean_c|x|;  the variance from the moved mean (which adds exactly
            (mean' - mean)^2) and C three-rounding terms:  B_var = (C + 4) e var + B_mean^2;  rstd = 1 / sqrt(var + eps), three more
            roundings:  B_rstd = rstd (B_var / (2 (var + eps)) + 3 e);  then
                D_xhat = rstd B_mean + |x - mean| B_rstd + 2 e |xhat|
                B_out  = u |out| + (1 + u) (|gamma| D_xhat + 2 e (|xhat gamma| + |beta|))
  backward     the kernel's xhat comes from fp32 statistics: moved by D_xhat (its rstd by B_rstd).  The two row reductions:
                e_1 = (C + 2) e mean_c|g|,   e_2 = (C + 3) e mean_c|g xhat| + mean_c(|g| D_xhat)
                D_in = e_1 + D_xhat |m_2| + |xhat| e_2 + 4 e (|g| + |m_1| + |xhat m_2|)           (m_1, m_2 the two means)
                B_dx = u |dx| + (1 + u) (rstd D_in + B_rstd |inner| + 2 e (|add| + |rstd inner|))
            and the token sums, n terms in fp32 in a fixed (but here: any) order:
                B_dgamma = sum_t |dy| D_xhat + (n + 2) e sum_t |dy xhat|,    B_dbeta = n e sum_t |dy|

1e-30 is added to every bound so that exact zeros compare.

What the bounds cannot see: erf-GELU and its tanh approximation differ by less than 5e-4 absolute, below u |gelu(x)| + L u |x| wherever
|x| > 0.07 and comparable to it below -- a kernel that used the tanh form would pass most elements.  Reading the kernel (erfcf, not tanhf)
has to catch that; the tests do not claim to.

The fp32 emulation (torch on the CPU, the same roundings) stays inside the bounds; its worst error / bound ratios over the cases of
tests/test_swin_block_ref.py are recorded in profiles/r32_swin_block.md (the largest is 0.99, on bf16 tensors: one rounding to nearest
alone reaches u |value| just above a power of two; the fp32 tensors stay below 0.04).
"""
import math

import torch

U = 2.0 ** -8
E = 2.0 ** -24
G = 2.0 ** -20          # fp32 evaluation of gelu / gelu'
LIP = 1.13              # max |gelu'|  (1.1289 at x = 1.41)
CURV = 0.8              # max |gelu''| (2 phi(0) = 0.7979 at x = 0)
TINY = 1e-30
BF = torch.bfloat16

LINEAR_WRONG = {0: ("bias_dropped", "last_k_block_dropped", "w_transposed"), 1: ("silu_gate", "bias_dropped"),
                2: ("residual_dropped",), 3: ("gelu_ratio", "last_k_block_dropped")}
LN_WRONG = ("unbiased_variance", "beta_dropped")
LN_BWD_WRONG = ("no_mean_terms", "add_dropped", "dgamma_unnormalised", "dbeta_last_row_dropped")


def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def ident(t):
    return t


def phi(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def cdf(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0))


def gelu(x):
    return x * cdf(x)


def gelu_grad(x):
    return cdf(x) + x * phi(x)


# ---- linear ----------------------------------------------------------------------------------------------------------------------------
def _linear(x, w, bias, aux, epilogue, dtype, rnd, wrong=None):
    x, w = x.to(dtype), w.to(dtype)
    if wrong == "last_k_block_dropped":
        x = x.clone()
        x[:, -32:] = 0
    if wrong == "w_transposed":
        assert w.shape[0] == w.shape[1]
        w = w.t()
    acc = x @ w.t()
    b = bias.to(dtype) if bias is not None and wrong != "bias_dropped" else torch.zeros((), dtype=dtype)
    a = aux.to(dtype) if aux is not None else None
    if epilogue == 0:
        return {"out": rnd(acc + b)}
    if epilogue == 1:
        u = rnd(acc + b)
        if wrong == "silu_gate":      # x sigmoid(x) in place of x Phi(x): off by up to 0.2
            return {"out": rnd(u * torch.sigmoid(u)), "out2": u}
        return {"out": rnd(gelu(u)), "out2": u}
    if epilogue == 2:
        return {"out": rnd(acc + b + (0 if wrong == "residual_dropped" else a))}
    factor = gelu(a) / a.where(a != 0, torch.ones_like(a)) if wrong == "gelu_ratio" else gelu_grad(a)
    return {"out": rnd(acc * factor), "out2": rnd(gelu(a))}


def linear_reference(x, w, bias, aux, epilogue, wrong=None, moved=None):
    """-> (values, bounds), dicts of float64 tensors with the keys "out" (and "out2" for epilogues 1 and 3).  `moved` (epilogue 3): the
    bound d of |aux - exact pre-activation| when aux is an epilogue 1's stored u and the caller's definition uses the exact one."""
    val = _linear(x, w, bias, aux, epilogue, torch.float64, ident, wrong)
    K = x.shape[1]
    mag = x.double().abs() @ w.double().abs().t()
    if epilogue == 3:
        a = aux.double()
        acc = x.double() @ w.double().t()
        b_out = U * val["out"].abs() + (1 + U) * ((K + 2) * E * mag * gelu_grad(a).abs() + G * acc.abs())
        if moved is not None:
            b_out = b_out + acc.abs() * CURV * moved
        bound = {"out": b_out, "out2": (U + G) * gelu(a).abs()}
    else:
        extra = (bias.double().abs() if bias is not None else 0) + (aux.double().abs() if epilogue == 2 else 0)
        e_lin = (K + 2) * E * (mag + extra)
        key = "out2" if epilogue == 1 else "out"
        bound = {key: U * val[key].abs() + (1 + U) * e_lin}
        if epilogue == 1:
            bound["out"] = LIP * bound["out2"] + (U + G) * (val["out"].abs() + LIP * bound["out2"])
    return val, {k: b + TINY for k, b in bound.items()}


def linear_emulate(x, w, bias, aux, epilogue):
    return _linear(x, w, bias, aux, epilogue, torch.float32, rnd_bf16)


def linear_inputs(T, K, N, epilogue, gen):
    """bf16 x, w (scaled so that the pre-activations are O(1): both signs and both tails of the GELU are hit), fp32 bias, bf16 aux"""
    x = torch.randn(T, K, generator=gen).to(BF)
    w = (torch.randn(N, K, generator=gen) * (1.5 / math.sqrt(K))).to(BF)
    bias = torch.randn(N, generator=gen) * 0.5
    aux = (torch.randn(T, N, generator=gen) * 1.5).to(BF) if epilogue >= 2 else None
    return x, w, bias, aux


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------
def _moments(x, eps, wrong=None):
    C = x.shape[1]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).sum(1, keepdim=True) / (C - 1 if wrong == "unbiased_variance" else C)
    return mean, var, 1.0 / torch.sqrt(var + eps)


def _layernorm(x, gamma, beta, eps, dtype, rnd, wrong=None):
    x = x.to(dtype)
    mean, _, rstd = _moments(x, eps, wrong)
    out = (x - mean) * rstd * gamma.to(dtype) + (0 if wrong == "beta_dropped" else beta.to(dtype))
    return {"out": rnd(out), "mean": mean[:, 0], "rstd": rstd[:, 0]}


def _stat_bounds(x, eps):
    """(mean, var, rstd, xhat, B_mean, B_rstd, D_xhat) in float64, the statistics as (T, 1)"""
    xd = x.double()
    C = xd.shape[1]
    mean, var, rstd = _moments(xd, eps)
    b_mean = (C + 1) * E * xd.abs().mean(1, keepdim=True)
    b_var = (C + 4) * E * var + b_mean ** 2
    b_rstd = rstd * (b_var / (2 * (var + eps)) + 3 * E)
    xhat = (xd - mean) * rstd
    d_xhat = rstd * b_mean + (xd - mean).abs() * b_rstd + 2 * E * xhat.abs()
    return mean, var, rstd, xhat, b_mean, b_rstd, d_xhat


def layernorm_reference(x, gamma, beta, eps, wrong=None):
    val = _layernorm(x, gamma, beta, eps, torch.float64, ident, wrong)
    _, _, _, xhat, b_mean, b_rstd, d_xhat = _stat_bounds(x, eps)
    g, b = gamma.double(), beta.double()
    bound = {"out": U * val["out"].abs() + (1 + U) * (g.abs() * d_xhat + 2 * E * ((xhat * g).abs() + b.abs())),
             "mean": b_mean[:, 0], "rstd": b_rstd[:, 0]}
    return val, {k: v + TINY for k, v in bound.items()}


def layernorm_emulate(x, gamma, beta, eps):
    return _layernorm(x, gamma, beta, eps, torch.float32, rnd_bf16)


def _layernorm_backward(dy, x, mean, rstd, gamma, add, dtype, rnd, wrong=None):
    """mean, rstd (T,) in `dtype`"""
    dy, x, gamma = dy.to(dtype), x.to(dtype), gamma.to(dtype)
    xc = x - mean[:, None]
    xhat = xc * rstd[:, None]
    g = dy * gamma
    inner = g if wrong == "no_mean_terms" else g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True)
    dx = rstd[:, None] * inner
    if add is not None and wrong != "add_dropped":
        dx = add.to(dtype) + dx
    dbeta = (dy[:-1] if wrong == "dbeta_last_row_dropped" else dy).sum(0)
    return {"dx": rnd(dx), "dgamma": (dy * (xc if wrong == "dgamma_unnormalised" else xhat)).sum(0), "dbeta": dbeta}


def layernorm_backward_reference(dy, x, gamma, add, eps, wrong=None):
    """the statistics are the float64 moments of x"""
    mean, _, rstd, xhat, _, b_rstd, d_xhat = _stat_bounds(x, eps)
    val = _layernorm_backward(dy, x, mean[:, 0], rstd[:, 0], gamma, add, torch.float64, ident, wrong)
    dyd, gd = dy.double(), gamma.double()
    n, C = dyd.shape
    g = dyd * gd
    m1, m2 = g.mean(1, keepdim=True), (g * xhat).mean(1, keepdim=True)
    e1 = (C + 2) * E * g.abs().mean(1, keepdim=True)
    e2 = (C + 3) * E * (g * xhat).abs().mean(1, keepdim=True) + (g.abs() * d_xhat).mean(1, keepdim=True)
    d_in = e1 + d_xhat * m2.abs() + xhat.abs() * e2 + 4 * E * (g.abs() + m1.abs() + (xhat * m2).abs())
    inner = g - m1 - xhat * m2
    addm = add.double().abs() if add is not None else 0
    bound = {"dx": U * val["dx"].abs() + (1 + U) * (rstd * d_in + b_rstd * inner.abs() + 2 * E * (addm + (rstd * inner).abs())),
             "dgamma": (dyd.abs() * d_xhat).sum(0) + (n + 2) * E * (dyd * xhat).abs().sum(0), "dbeta": n * E * dyd.abs().sum(0)}
    return val, {k: v + TINY for k, v in bound.items()}


def layernorm_backward_emulate(dy, x, gamma, add, eps):
    """fp32, with the fp32 statistics of the fp32 forward emulation"""
    mean, _, rstd = _moments(x.float(), eps)
    return _layernorm_backward(dy, x, mean[:, 0], rstd[:, 0], gamma, add, torch.float32, rnd_bf16)


def layernorm_inputs(T, C, gen, with_add=True):
    """bf16 x (rows of different offsets and spreads), dy, add; fp32 gamma, beta"""
    x = (torch.randn(T, C, generator=gen) * (0.5 + 2 * torch.rand(T, 1, generator=gen)) + torch.randn(T, 1, generator=gen)).to(BF)
    dy = torch.randn(T, C, generator=gen).to(BF)
    add = torch.randn(T, C, generator=gen).to(BF) if with_add else None
    return x, dy, add, 1 + 0.5 * torch.randn(C, generator=gen), 0.5 * torch.randn(C, generator=gen)


def ratios(got, val, bound):
    """worst |got - want| / bound per tensor of `val` that `got` holds (inf for a NaN)"""
    res = {}
    for n in val:
        if got.get(n) is None:
            continue
        r = (got[n].double().cpu() - val[n]).abs() / bound[n]
        res[n] = float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())
    return res
