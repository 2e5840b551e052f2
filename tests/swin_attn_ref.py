"""Float64 restatement of the Swin window attention (csrc/swin_attn_mfma.hip, richsem_amd.swin.window_attention) with an ELEMENT-WISE
error bound for every tensor the kernels write, an fp32 emulation of the kernels' roundings, wrong variants that must leave the bounds,
the expectation of the exact probe, and the reader of tests/golden/layer_swin_reference.npz.  Test helper only: the package never imports it.

Operands in map layout: qkv (B, Hp, Wp, 3 * 32 * nH) ordered (3, nH, 32), table ((2w-1)^2, nH), dout (B, Hp, Wp, 32 * nH); the inputs are the
bf16 values (and the fp32 table), so their float64 copies are exact.  Written the reference's way -- roll by -s, cut into windows, merge,
roll back -- and not the package's (pixel indices): the two meet only in the numbers.

Per (image, window, head), with c = 1 / sqrt(32), bias[t, t'] = table[(i - i' + w - 1)(2w - 1) + (j - j' + w - 1), h] and, for s > 0,
mask[t, t'] = -100 where the region ids differ (region = 3 r(py, Hp) + r(px, Wp) on rolled coordinates, r(c, n) = [c >= n - w] + [c >= n - s]):

    S = c q k^T + bias + mask      P = softmax(S)       out = P v
    dP = dout v^T                  delta = rowsum(dout * out)
    dS = P * (dP - delta)          dq = c dS k          dk = c dS^T q       dv = P^T dout      dtable[r, h] = sum of dS over the pairs of index r

The bounds.  u = 2^-8 is the unit round-off of bf16 (round to nearest even); f = 2^-13 bounds the relative error of an fp32 accumulation
over fewer than 2^11 terms and, with room, the few-ulp errors of exp2f / logf / the reciprocal and of fp32 scores of magnitude <= 128 (the
-100 of the mask included: 2^7 * 2^-24 = 2^-17 absolute in the exponent).  Every rounding on the kernels' path, and where it is counted:

  out     the unnormalised probability tile is rounded to bf16 before V^T . P^T (u); fp32 accumulation over the keys, the row sum, 1 / l
          (f); the output is rounded to bf16 (u):                     B_out = (2 u + f) * (P |v|)
  dv      P recomputed in fp32 from the saved log-sum-exp (inside f), rounded to bf16 (u), accumulated in fp32 (f), rounded (u):
                                                                      B_dv  = (2 u + f) * (P^T |dout|)
  dq      delta is formed from the ROUNDED out:  |delta_got - delta| <= E[t] = sum_d |dout[t, d]| B_out[t, d], which moves dS by P E;
          dS is rounded to bf16 (u), accumulated in fp32 (f), scaled and rounded to bf16 (u):
                                                                      B_dq  = c ((2 u + f) |dS| |k| + E * (P |k|))
  dk      the same with the rows exchanged:                           B_dk  = c ((2 u + f) |dS|^T |q| + (P * E)^T |q|)
  dtable  the fp32 dS (NOT rounded to bf16) of n_r pairs are added in fp32.  A term P (dP - delta) carries the relative error of P and
          of the 32-term products (f, against the magnitudes |dout| |v|^T and sum_d |dout out|) and the moved delta (P E); adding n_r
          terms in fp32, in any order, costs at most n_r 2^-24 sum |dS|:
                                                                      B_dt  = sum_r [ f P (|dout| |v|^T + sum_d |dout out|) + P E ] + n_r 2^-24 sum_r |dS|

1e-30 is added to every bound so that exact zeros compare.
"""
import math
import os

import numpy as np
import torch

U = 2.0 ** -8
F = 2.0 ** -13
C = 1.0 / math.sqrt(32.0)
TINY = 1e-30
TENSORS = ("out", "dqkv", "dtable")
WRONG = ("no_mask", "roll_reversed", "bias_transposed", "scaled_bias", "pad_keys_unmasked")


# ---- windows the reference's way -------------------------------------------------------------------------------------------------------
def partition(x, w, s, sign=-1):
    """x (B, Hp, Wp, ...) -> (B, windows, w * w, ...) after rolling by sign * s"""
    if s:
        x = torch.roll(x, shifts=(sign * s, sign * s), dims=(1, 2))
    B, Hp, Wp = x.shape[:3]
    rest = tuple(x.shape[3:])
    x = x.reshape(B, Hp // w, w, Wp // w, w, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest)))
    return x.reshape(B, (Hp // w) * (Wp // w), w * w, *rest)


def merge(xw, Hp, Wp, w, s, sign=-1):
    B = xw.shape[0]
    rest = tuple(xw.shape[3:])
    x = xw.reshape(B, Hp // w, Wp // w, w, w, *rest).permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(B, Hp, Wp, *rest)
    if s:
        x = torch.roll(x, shifts=(-sign * s, -sign * s), dims=(1, 2))
    return x


def regions(Hp, Wp, w, s):
    """(windows, w * w) int64 region ids of the rolled map (zero for s = 0)"""
    ids = torch.zeros(Hp, Wp, dtype=torch.int64)
    if s:
        py, px = torch.arange(Hp), torch.arange(Wp)
        ry = (py >= Hp - w).long() + (py >= Hp - s).long()
        rx = (px >= Wp - w).long() + (px >= Wp - s).long()
        ids = 3 * ry[:, None] + rx[None, :]
    return partition(ids[None], w, 0)[0]


def bias_pairs(w, transposed=False):
    t = torch.arange(w * w)
    i, j = t // w, t % w
    di, dj = i[:, None] - i[None, :], j[:, None] - j[None, :]
    if transposed:
        di, dj = -di, -dj
    return (di + w - 1) * (2 * w - 1) + dj + w - 1


def _core(qkv, table, dout, nH, w, s, dtype, rnd, wrong=None):
    """the computation in `dtype`; rnd(x) is the bf16 rounding of the kernels' path (identity for the float64 definition)"""
    B, Hp, Wp, _ = qkv.shape
    N, R = w * w, (2 * w - 1) ** 2
    sign = 1 if wrong == "roll_reversed" else -1
    parts = partition(qkv.to(dtype).reshape(B, Hp, Wp, 3, nH, 32), w, s, sign).permute(3, 0, 1, 4, 2, 5)      # (3, B, nW, nH, N, 32)
    q, k, v = parts[0], parts[1], parts[2]
    g = partition(dout.to(dtype).reshape(B, Hp, Wp, nH, 32), w, s, sign).permute(0, 1, 3, 2, 4)                # (B, nW, nH, N, 32)
    idx = bias_pairs(w, wrong == "bias_transposed")
    bias = table.to(dtype)[idx].permute(2, 0, 1)                                                              # (nH, N, N)
    qk = q @ k.transpose(-1, -2)
    score = (qk + bias) * C if wrong == "scaled_bias" else qk * C + bias
    if s and wrong != "no_mask":
        reg = regions(Hp, Wp, w, s)
        score = score + ((reg[:, :, None] != reg[:, None, :]).to(dtype) * -100.0)[None, :, None]
    m = score.amax(-1, keepdim=True)
    if wrong == "pad_keys_unmasked" and N % 16:
        m = m.clamp_min(0.0)
    e = torch.exp(score - m)
    l = e.sum(-1, keepdim=True)
    if wrong == "pad_keys_unmasked" and N % 16:      # (16 - N % 16) keys of zeros with score 0 take part in the softmax
        l = l + (16 - N % 16) * torch.exp(-m)
    p = e / l
    out = rnd((rnd(e) @ v) / l)
    lse = m + torch.log(l)
    p2 = torch.exp(score - lse)                       # the backward's probabilities, from the saved log-sum-exp
    dp = g @ v.transpose(-1, -2)
    delta = (g * out).sum(-1, keepdim=True)           # from the rounded out
    ds = p2 * (dp - delta)
    dq = rnd(C * (rnd(ds) @ k))
    dk = rnd(C * (rnd(ds).transpose(-1, -2) @ q))
    dv = rnd(rnd(p2).transpose(-1, -2) @ g)
    dtable = torch.zeros(R, nH, dtype=dtype).index_add_(0, idx.reshape(-1), ds.sum((0, 1)).permute(1, 2, 0).reshape(N * N, nH))

    def to_map(t):      # (B, nW, nH, N, 32) -> (B, Hp, Wp, nH * 32)
        return merge(t.permute(0, 1, 3, 2, 4).reshape(B, -1, N, nH * 32), Hp, Wp, w, s, sign)
    val = {"out": to_map(out), "dqkv": torch.cat([to_map(dq), to_map(dk), to_map(dv)], -1), "dtable": dtable}
    return val, dict(q=q, k=k, v=v, g=g, p=p, ds=ds, out=out, idx=idx, to_map=to_map)


def reference(qkv, table, dout, nH, w, s, wrong=None):
    """-> (values, bounds): dicts with the keys of TENSORS, float64.  `wrong` (one of WRONG) computes a wrong implementation's values:
    its bounds are meaningless."""
    val, t = _core(qkv, table, dout, nH, w, s, torch.float64, lambda x: x, wrong)
    q, k, v, g, p, ds, out, idx = (t[n] for n in ("q", "k", "v", "g", "p", "ds", "out", "idx"))
    r = 2 * U + F
    b_out = r * (p @ v.abs())
    e_delta = (g.abs() * b_out).sum(-1, keepdim=True)
    b_dq = C * (r * (ds.abs() @ k.abs()) + e_delta * (p @ k.abs()))
    b_dk = C * (r * (ds.abs().transpose(-1, -2) @ q.abs()) + (p * e_delta).transpose(-1, -2) @ q.abs())
    b_dv = r * (p.transpose(-1, -2) @ g.abs())
    term = F * p * (g.abs() @ v.abs().transpose(-1, -2) + (g * out).abs().sum(-1, keepdim=True)) + p * e_delta
    N, nH_ = p.shape[-1], p.shape[2]
    R = (2 * w - 1) ** 2

    def by_index(x):      # (B, nW, nH, N, N) -> (R, nH)
        return torch.zeros(R, nH_, dtype=torch.float64).index_add_(0, idx.reshape(-1), x.sum((0, 1)).permute(1, 2, 0).reshape(N * N, nH_))
    count = torch.bincount(idx.reshape(-1), minlength=R).double()[:, None] * (p.shape[0] * p.shape[1])
    b_dt = by_index(term) + count * 2.0 ** -24 * by_index(ds.abs())
    bound = {"out": t["to_map"](b_out), "dqkv": torch.cat([t["to_map"](b_dq), t["to_map"](b_dk), t["to_map"](b_dv)], -1), "dtable": b_dt}
    return val, {n: b + TINY for n, b in bound.items()}


def emulate(qkv, table, dout, nH, w, s):
    """the same computation in fp32 with exactly the kernels' bf16 roundings -> dict with the keys of TENSORS, float32"""
    return _core(qkv, table, dout, nH, w, s, torch.float32, lambda x: x.to(torch.bfloat16).float())[0]


def ratios(got, val, bound):
    """worst |got - want| / bound per tensor (inf for a NaN)"""
    res = {}
    for n in TENSORS:
        r = (got[n].double().cpu() - val[n]).abs() / bound[n]
        res[n] = float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())
    return res


def random_inputs(B, Hp, Wp, nH, w, gen, scale=1.5, table_std=0.5):
    """bf16 qkv and dout, fp32 table"""
    qkv = torch.randn(B, Hp, Wp, 3, nH, 32, generator=gen)
    qkv[:, :, :, :2] *= scale
    return (qkv.reshape(B, Hp, Wp, 3 * nH * 32).to(torch.bfloat16), torch.randn((2 * w - 1) ** 2, nH, generator=gen) * table_std,
            torch.randn(B, Hp, Wp, nH * 32, generator=gen).to(torch.bfloat16))


def probe_expectation(v_map, nH, w, s, head, di, dj):
    """The exact probe: q = k = 0 and table = +60 at the offset (di, dj) of `head` (index (di + w - 1)(2w - 1) + dj + w - 1).  A query
    (i, j) whose neighbour (i - di, j - dj) lies in its window and region puts all its weight there.  v_map (B, Hp, Wp, nH * 32) ->
    (valid (B, Hp, Wp) bool, rows (B, Hp, Wp, 32): the neighbour's v row of that head where valid)"""
    B, Hp, Wp, _ = v_map.shape
    vw = partition(v_map.reshape(B, Hp, Wp, nH, 32)[:, :, :, head], w, s)      # (B, nW, N, 32)
    reg = regions(Hp, Wp, w, s)
    t = torch.arange(w * w)
    i, j = t // w - di, t % w - dj
    inside = (i >= 0) & (i < w) & (j >= 0) & (j < w)
    nb = (i.clamp(0, w - 1) * w + j.clamp(0, w - 1))
    valid = inside[None, :] & (reg.gather(1, nb[None].expand_as(reg)) == reg)   # (nW, N)
    rows = vw[:, :, nb]
    valid_map = merge(valid[None, :, :, None].expand(B, -1, -1, 1).to(torch.uint8), Hp, Wp, w, s)[..., 0].bool()
    return valid_map, merge(rows, Hp, Wp, w, s)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_swin_reference.npz")) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def fixture_exact(name, dtype=torch.float64):
    """a tensor stored as int16 multiples of 2^-6"""
    return (torch.from_numpy(fixture()[name].astype(np.float64)) / 64).to(dtype)


def fixture_state_dict(tag, dtype=torch.float64):
    sd = {}
    for k, a in fixture().items():
        if k.startswith(tag + ".sd."):
            sd[k[len(tag) + 4:]] = fixture_exact(k, dtype) if a.dtype == np.int16 else torch.from_numpy(a)
    return sd


def fixture_compare(name, got):
    """-> (stored float64 values, the matching values of `got`): the whole tensor, or every stride-th element plus the sum of all"""
    fx = fixture()
    want = torch.from_numpy(np.atleast_1d(fx[name])).double().reshape(-1)
    flat = got.detach().double().cpu().reshape(-1)
    if name + ".stride" in fx:
        flat = torch.cat([flat[::int(fx[name + ".stride"])], flat.sum().reshape(1)])
        want = torch.cat([want, torch.tensor([float(fx[name + ".sum"])], dtype=torch.float64)])
    assert flat.shape == want.shape, (name, flat.shape, want.shape)
    return want, flat
