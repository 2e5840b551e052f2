"""Float64 restatement of the decoder's masked self-attention (csrc/attn_mfma.hip) with an ELEMENT-WISE error bound for every
tensor the kernels write, and an fp32 emulation of the kernels' roundings.  The comparator of tests/test_gpu_attention.py (the
kernels against the bounds) and of tests/test_attention_ref.py (the emulation against the bounds: the check that the bounds are
attainable by a correct implementation).  Test helper only: the package never imports it.

All tensors are per (image, head): q, k, v, dout (B, H, nq, 32); mask (nq, nq) bool, True = query (row) must not attend to key
(column), or None.  The inputs are the bf16 values, so the float64 copies are exact.

The operation, with c = 1 / sqrt(32):

    S = c q k^T (masked: -inf)      P = softmax(S)       out = P v         lse2 = log2 sum_k exp(S)     (the kernel saves log2 units)
    dP = dout v^T                   delta = rowsum(dout * out)
    dS = c P * (dP - delta)         dq = dS k            dk = dS^T q       dv = P^T dout

(dS is the gradient with respect to the UNSCALED product q k^T -- the tile the backward kernels round to bf16.)
A row with no allowed key is DEFINED as out = 0, lse2 = +inf and no contribution to any gradient (P = 0 on that row, so dq = 0 there):
that is what the kernels do (include/richsem_msda.h); torch's softmax gives NaN.

The bounds.  u = 2^-8 is the unit round-off of bf16 under round-to-nearest-even (pack_bf16); f = 2^-13 bounds the relative error of
an fp32 accumulation over nq < 2^11 terms (2^11 * 2^-24), and with it the few-ulp errors of exp2f / log2f / the reciprocal and of the
fp32 scores, which are far smaller.  Every rounding on the kernels' path, and where it is counted:

  out   (1) the unnormalised probability tile is rounded to bf16 before V^T . P^T       u * P |v|
        (2) the fp32 accumulation over the keys, the wave merge, the row sum l, 1 / l     f * P |v|
        (3) the output is rounded to bf16                                                 u * |out| <= u * P |v|
        B_out = (2 u + f) * (P |v|)

  dv    P is recomputed in fp32 from the saved lse2 (its error: (2), inside f), rounded to bf16 (u), accumulated over the queries in
        fp32 (f), the result rounded to bf16 (u):
        B_dv = (2 u + f) * (P^T |dout|)

  dq    dP is an fp32 product of bf16 inputs over 32 terms (inside f); delta is formed from the bf16 `out`, whose element error is
        B_out, so  |delta_got - delta| <= E_delta[q] = sum_d |dout[q, d]| * B_out[q, d]  and dS moves by at most c P E_delta;
        dS is rounded to bf16 (u), accumulated over the keys in fp32 (f), the result rounded to bf16 (u):
        B_dq = (2 u + f) * (|dS| |k|) + c * E_delta * (P |k|)
  dk    the same with the roles of the rows exchanged:
        B_dk = (2 u + f) * (|dS|^T |q|) + c * ((P * E_delta)^T |q|)

  lse2  = m + log2(l): the relative error of the fp32 row sum l (<= f) becomes f / ln 2 < 1.5 f through log2; the fp32 scores
        (a product over 32 terms, a multiplication by c log2 e) and the final addition are each rounded at the magnitude of lse2:
        |lse2_got - lse2| <= 1.5 f + 2^-21 |lse2|          (2^-21 = 8 fp32 round-offs)

1e-30 is added to every bound so that exact zeros compare.  A row with no allowed key must be exact: out = 0, lse2 = +inf, dq = 0.
"""
import math

import torch

U = 2.0 ** -8
F = 2.0 ** -13
C = 1.0 / math.sqrt(32.0)
LOG2E = 1.4426950408889634
TINY = 1e-30
TENSORS = ("out", "lse2", "dq", "dk", "dv")


def _scores(q, k, mask):
    s = (q @ k.transpose(-1, -2)) * C
    if mask is not None:
        s = s.masked_fill(mask[None, None].to(s.device), float("-inf"))
    return s


def reference(q, k, v, dout, mask):
    """-> (values, bounds): two dicts with the keys of TENSORS, float64; lse2 is (B, H, nq), the others (B, H, nq, 32)"""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    s = _scores(q, k, mask)
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)                                   # (B, H, nq, 1): rows with no allowed key
    e = torch.exp(s - torch.where(empty, torch.zeros_like(m), m))      # (empty rows: exp(-inf) = 0)
    l = e.sum(-1, keepdim=True)
    p = e / torch.where(empty, torch.ones_like(l), l)
    lse2 = torch.where(empty, torch.full_like(m, float("inf")), (m + torch.log(torch.where(empty, torch.ones_like(l), l))) * LOG2E)[..., 0]
    out = p @ v
    delta = (dout * out).sum(-1, keepdim=True)
    ds = C * p * (dout @ v.transpose(-1, -2) - delta)
    val = {"out": out, "lse2": lse2, "dq": ds @ k, "dk": ds.transpose(-1, -2) @ q, "dv": p.transpose(-1, -2) @ dout}
    r = 2 * U + F
    b_out = r * (p @ v.abs())
    e_delta = (dout.abs() * b_out).sum(-1, keepdim=True)
    bound = {
        "out": b_out,
        "dv": r * (p.transpose(-1, -2) @ dout.abs()),
        "dq": r * (ds.abs() @ k.abs()) + C * e_delta * (p @ k.abs()),
        "dk": r * (ds.abs().transpose(-1, -2) @ q.abs()) + C * ((p * e_delta).transpose(-1, -2) @ q.abs()),
        "lse2": torch.where(torch.isinf(lse2), torch.zeros_like(lse2), 1.5 * F + 2.0 ** -21 * lse2.abs()),
    }
    return val, {n: b + TINY for n, b in bound.items()}


def _bf16(x):
    return x.to(torch.bfloat16).float()


def emulate(q, k, v, dout, mask):
    """The same computation in fp32 with exactly the kernels' bf16 roundings -> dict with the keys of TENSORS, float32"""
    q, k, v, dout = (t.float() for t in (q, k, v, dout))
    s2 = _scores(q, k, mask) * LOG2E                                   # log2 units, as the kernel's scale2
    m = s2.amax(-1, keepdim=True)
    empty = torch.isinf(m) & (m < 0)
    mu = torch.where(empty, torch.zeros_like(m), m)
    e = torch.exp2(s2 - mu)
    l = e.sum(-1, keepdim=True)                                        # the row sum takes the UNROUNDED probabilities
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    out = _bf16((_bf16(e) @ v) * inv)                                  # P rounded before P . V; the output rounded
    lse2 = torch.where(l > 0, m + torch.log2(l), torch.full_like(m, float("inf")))
    p = torch.exp2(s2 - lse2)                                          # recomputed from the fp32 lse (+inf: 0)
    delta = (dout * out).sum(-1, keepdim=True)                         # from the rounded out
    ds = _bf16(p * (dout @ v.transpose(-1, -2) - delta) * C)           # rounded before both products
    return {"out": out, "lse2": lse2[..., 0], "dq": _bf16(ds @ k), "dk": _bf16(ds.transpose(-1, -2) @ q),
            "dv": _bf16(_bf16(p).transpose(-1, -2) @ dout)}


def ratios(got, val, bound):
    """worst |got - want| / bound per tensor (inf where a value that must be exact -- an empty row's lse2 -- is not)"""
    res = {}
    for n in TENSORS:
        g, w = got[n].double(), val[n]
        exact = torch.isinf(w)
        diff = torch.where(exact, torch.zeros_like(w), g - torch.where(exact, torch.zeros_like(w), w)).abs()
        r = diff / bound[n]
        r = torch.where(exact & (g != w), torch.full_like(r, float("inf")), r)
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        res[n] = float(r.max())
    return res


def existing_test_mask(nq, gen):
    """the mask of test_attention_kernels_against_the_definition: a denoising-style block plus 30 % random holes, diagonal kept"""
    mask = torch.rand(nq, nq, generator=gen) < 0.3
    mask[nq // 3:, : nq // 3] = True
    mask.fill_diagonal_(False)
    return mask


def structured_mask(kind, nq):
    """the masks of the structured cases; True = masked"""
    i = torch.arange(nq)[:, None]
    j = torch.arange(nq)[None, :]
    if kind == "causal":
        return j > i
    if kind == "own_block":                       # every query sees only its own 32-key block
        return (j // 32) != (i // 32)
    if kind.startswith("wave"):                   # only the key blocks of one wave: the other three end with m = -inf
        return ((j // 32) % 4 != int(kind[4:])).expand(nq, nq).clone()
    if kind == "last_key":                        # the lone key of the last partial block
        return (j != nq - 1).expand(nq, nq).clone()
    if kind == "first_block_masked":              # every wave's first block (0..3) fully masked: the running maximum starts at -inf
        return (j < 128).expand(nq, nq).clone()
    raise ValueError(kind)


def random_inputs(bs, heads, nq, gen, scale=1.5):
    """bf16 q, k, v, dout (bs, heads, nq, 32), different for every (image, head)"""
    mk = lambda s: (torch.randn(bs, heads, nq, 32, generator=gen) * s).to(torch.bfloat16)
    return mk(scale), mk(scale), mk(1.0), mk(1.0)


def mask_outlier_last_key(q, k, mask):
    """in place: the last key is masked for every other query and scores far above query 0's allowed maximum (k_last = 16 sign(q_0))"""
    nq = q.shape[2]
    mask[: nq - 1, nq - 1] = True
    k[:, :, nq - 1] = torch.where(q[:, :, 0] < 0, -16.0, 16.0).to(k.dtype)


def sparse_mask(nq, gen):
    """every query allows 1, 2, 4 or 8 keys (cycling), positions random; keys 31 and 32 (the sign bit of word 0, the first bit of
    word 1) are among the allowed keys of every seventh query where they exist.  Not symmetric.  -> (mask, counts)"""
    mask = torch.ones(nq, nq, dtype=torch.bool)
    counts = torch.zeros(nq, dtype=torch.int64)
    for i in range(nq):
        n = min((1, 2, 4, 8)[i % 4], nq)
        keys = torch.randperm(nq, generator=gen)[:n].tolist()
        if i % 7 == 3 and n >= 2 and nq > 32:
            rest = [x for x in keys if x not in (31, 32)]
            keys = [31, 32] + rest[: n - 2]
        mask[i, keys] = False
        counts[i] = n
    assert not torch.equal(mask, mask.t())
    return mask, counts
