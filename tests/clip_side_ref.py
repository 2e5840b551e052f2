"""Float64 restatements of the CLIP side of the model -- the two-stage class score (richsem_amd/csrc/cls_mfma.hip), ROIAlign
(csrc/msda_roi.h) and the attention-pool core (csrc/msda_attnpool.h) -- AS THE KERNELS DEFINE THE OPERATIONS, with an ELEMENT-WISE error
bound for every value the kernels write, EXACT PROBES whose results are one representable number whatever the summation order, the case
lists, and emulations with the kernels' rounding points.  The comparator of tests/test_gpu_clip_side_bounds.py (the kernels against the
bounds and the probes) and of tests/test_clip_side_ref.py (the emulations against the bounds: the check that a correct implementation
can meet them).  Test helper only: the package never imports it.

Notation as in tests/ffn_ref.py (the constants are imported from there): u = 2^-8 is the unit round-off of bf16 under round-to-nearest-
even, e = 2^-24 that of fp32 (e64 = 2^-53 that of fp64); an fp32 sum of n terms, in ANY order, errs by at most n e sum|term| (first order;
no bound relies on the order); TINY = 1e-30 is added to every bound so that exact zeros compare.  All inputs are bf16 / fp32 / fp64
values, so their float64 copies are exact.

CLASS SCORE   s = scale m / sqrt(n2),   m = max_c (G x)_c,   n2 = x . (A x)       (G (classes, 256), A (256, 256) fp32; x fp32 or bf16)
    A row w of [G; A] and the token x are split as in lin256_f32 (ffn_ref.py, the derivation of C_F32): w = wh + wl + rw, x = xh + xl + rx,
    |wl| <= u |w|, |rw| <= u^2 |w|, the same for x; the kernel sums wh xh + wl xh + wh xl, exact products, in fp32.  Missing from w . x,
    relative to S = sum_k |w_k| |x_k|:
        fp32 x, parts 2:  wl xl (u^2), rw x and w rx (2 u^2), 768 products summed (768 e, + 1 as in C_F32):    c = (3 u^2 + 769 e)(1 + 2 u) = C_F32
        bf16 x, parts 2:  x = xh exactly -- no lo_x term, no rx: rw x (u^2), 512 products:                      c = (u^2 + 513 e)(1 + 2 u)
        fp32 x, parts 1:  the weights are bf16(w) (u: the bound is at u level), xl kept, rx (u^2), 512 products:  c = (u + u^2 + 513 e)(1 + 2 u)
        bf16 x, parts 1:  u, 256 products:                                                                      c = (u + 257 e)(1 + 2 u)
    (cls_c).  Per class |(G x)_c got - exact| <= c S_c, S_c = sum_k |G_ck| |x_k|.  The maximum is 1-Lipschitz in the sup norm:
        B_m = max_c c S_c.
    n2: every (A x)_j carries c SA_j, SA_j = sum_k |A_jk| |x_k|; it is multiplied by x_j (the fp32 x, or the bf16 x as it is) and summed by
    256 fmaf -- exact products, one rounding each -- in four lane groups that two more additions fold: 258 roundings of partial sums bounded
    by sum_j |x_j| (|(A x)_j| + c SA_j) <= (1 + c) Q,   Q = sum_jk |x_j| |A_jk| |x_k|:
        B_n2 = (c + 258 e (1 + c)) Q.
    Q, not n2: the bound is cancellation-aware and loosens by itself when A = Wp^T Wp is ill-conditioned and x lies in a small singular
    direction (n2 << Q).  rho = B_n2 / n2.  For rho < 1 the mean-value bound of t^-1/2 on [1 - rho, 1 + rho] gives
        |n2_got^-1/2 / n2^-1/2 - 1| <= r = rho / 2 / (1 - rho)^3/2;
    for rho >= 1 the bound cannot exclude n2_got <= 0 and is infinite (it says nothing; the tests count such tokens).  The epilogue is three
    fp32 operations -- scale * m (e), sqrtf and the division (correctly rounded under hipcc's default; 2 ulp = 4 e each is taken) -- 9 e,
    written 10 e:
        B_s = |scale| n2^-1/2 (B_m (1 + r + 10 e) + |m| (r + 10 e)).
    Against the oracle from (Wp, text) (oracle/cls_oracle.py in float64) G and A are float64 products rounded ONCE to fp32: e S_c more per
    class, e Q more in n2, and the fp32 rounding of scale = exp(logit_scale), one more e: c -> c + e (1 + c), 10 e -> 11 e (`oracle=True`).
    x = 0 gives m = 0, n2 = 0 and 0 / 0 = NaN; the reference's f / |f| is NaN as well.  No bound: the tests assert the NaN.

ROIALIGN   (reasoning of tests/test_gpu_roi_targets.py, element by element)
    A sample position is start + ph bin + (i + 0.5) bin / grid with start = roi * scale - offset, bin = (end - start) / bins: at most 12
    roundings on quantities of magnitude <= P, P = max(|start|, |end|, 1) over both axes of THAT ROI (a box may stick out of the map: the
    positions are as large as the box, not as the map), so a position is off by at most 12 eps P per axis.  Bilinear interpolation of values
    bounded by M is 2 M-Lipschitz per axis (the clamping at the borders is continuous): a sample is off by 2 * 2 M * 12 eps P = 48 eps P M
    from its position; 64 leaves a quarter for the products that form the position.  The interpolation is 4 products of 3 factors and 3
    additions on values <= M: below 16 eps M.  The mean adds gh gw samples, (gh gw + 1) eps M with the division:
        B = (64 P + gh gw + 16) eps M[image, channel],      M = max |input| over that element's own image and channel, gh, gw that ROI's grid;
    eps = e for f32.  For f64 the float64 reference errs by as much as the kernel: eps = 2 * 2^-53 (a few 2^-53 of the same form).
    spatial_scale reaches the kernel as a double and is cast to T: the reference of an f32 call uses float32(scale) (kernel_scale).
    CONDITIONS (roi_conditions, asserted in float64 on the test's own boxes): the operator is discontinuous where roi / bins crosses an
    integer (the adaptive grid is its ceil) and where a sample crosses -1 or the map's size (outside it counts 0); every roi / bins is at
    least ROI_MARGIN = 1e-4 from an integer and every sample at least ROI_MARGIN from -1 and from H (W), and 12 e P < ROI_MARGIN / 2.
    Refusals (the kernel's definition, restated): a batch index outside [0, N), a box whose start or size is not finite, or an adaptive
    grid above ROI_MAX_GRID per axis -> exact zeros.

ATTENTION POOL CORE   per (ROI k, head h), row = h K + k (head_major) or k H + h; tokens 0 (the mean token) and 1 + t
    sf_t = u . f_t:  C products, one rounding each, summed by four waves (every fourth channel) and a 4-term fold:  e_f[t] = (C + 5) eps S_t,
        S_t = sum_c |u_c| |f_ct|;   score_{1+t} = sf_t + spos_{1+t}:  e_s[1 + t] = e_f[t] + eps (S_t + |spos_{1+t}|)
    score_0 = spos_0 + (sum_t sf_t) / Tn:  e_s[0] = mean_t e_f[t] + (Tn + 3) eps (mean_t S_t + |spos_0|)
    d_t = score_t - max score: both carry their error, the subtraction rounds: delta_t = e_s[t] + max_t' e_s[t'] + eps |d_t|  -- the "2 x the
        score error" of the weights.  w_t = exp(d_t): |w_got / w - 1| <= r_t = expm1(delta_t) + X eps (1 + expm1(delta_t)), X = 4: expf and exp
        are specified to 1 ulp in the HIP math API's accuracy table (HIP programming guide, "Math API", single and double precision exp);
        2 ulp = 4 eps is taken so that the figure does not depend on how the table measures an ulp.  A weight below the smallest normal
        number may be flushed to 0: an absolute 2^-126 (f32), 2^-1022 (f64) per weight (FLUSH).
    sum = sum_t w_t over Tn + 1 terms: relative error <= rs = max_t r_t + (Tn + 4) eps (with 1 / sum and the product w_t * inv);
        a_t = w_t / sum:  |a_got - a_t| <= ea_t = a_t ((r_t + rs) / (1 - rs) + 4 eps) + FLUSH
    z_c = a_0 m0_c + sum_t a_{1+t} (f_ct + pos_{1+t,c}),  m0_c = mean_t f_ct + pos_0c:
        fp_t = f + pos: eps |fp_t|;  m0: e_m0 = (Tn + 2) eps (mean_t |f_ct| + |pos_0c|);  a (Tn + 2)-term sum of rounded products:
        B_z = sum_t ea_{1+t} |fp_t| + ea_0 |m0| + a_0 e_m0 + (Tn + 4) eps (sum_t a_{1+t} |fp_t| + a_0 |m0|)
    eps = e for f32; for f64 eps = 2 * 2^-53 (the float64 reference's own error has the same form).

EXACT PROBES (conditions asserted where the probes are built: cls_probe_expected, attn_uniform_probe, attn_probe_values; tests/test_clip_side_ref.py)
    class score: at every k, the entries of [G; A] are multiples of 2^g and those of x multiples of 2^h with g + h >= -6, and sum |w| |x| <
        2^18 for every row of [G; A] -- every product is a multiple of 2^-6 and every partial sum needs under 24 bits: exact in fp32 in any order; at every k at most one of (row, token) has a lo part,
        so the dropped lo * lo product is exactly 0; A = a a^T with n2 = (a . x)^2 = 4^p; scale = 2^4.  The score is then one float.
    ROIAlign: spatial_scale a power of two, box coordinates multiples of 2^-3, bins and bin / grid dyadic (grids 1, 2, 4), integer map values:
        float32 and float64 agree bit for bit with the float64 restatement.
    attention pool: u = 0 makes every score exactly spos; spos = 0 -> uniform weights 1 / (Tn + 1) (a power of two); spos = -1000 but for one
        token -> exp underflows to exactly 0 in both precisions and the selected weight is exactly 1; feat and pos are multiples of 2^-2.
"""
import math

import numpy as np
import torch

from ffn_ref import BF, C_F32, E, TINY, U  # noqa: F401

E64 = 2.0 ** -53
D = 256
ROI_MAX_GRID = 4096          # kRoiTgtMaxGrid (csrc/msda_roi.h)
ROI_MARGIN = 1e-4
ATTN_MAX_T = 256             # kAttnPoolMaxT (csrc/msda_attnpool.h)
EXP_ULPS_E = 4.0             # 2 ulp of expf / exp, in units of eps (module docstring)

# ---- the cases (shared by the CPU and the GPU test) -------------------------------------------------------------------------------------
CLS_T_SWEEP = (1, 15, 16, 17, 47, 48, 49, 191, 192, 193, 385)
CLS_C_SWEEP = (1, 5, 15, 16, 17, 31, 32, 33, 1203)
CLS_MODES = (("f32", 2), ("f32", 1), ("bf16", 2), ("bf16", 1))
CLS_CASES = [(T, 33) for T in CLS_T_SWEEP] + [(193, c) for c in CLS_C_SWEEP if c != 33]
CLS_NEG_CLASSES = (1, 5, 17, 33)
CLS_PROBE_SHAPES = ((193, 41), (49, 64), (385, 33))      # 41: two full tiles and a partial one of 9 rows; 64: the last tile is full
CLS_SPREADS = (1, 10, 100)
CLS_PROBE_SCALE = 16.0

# (N, C, H, W, output size, spatial_scale, sampling_ratio, aligned): maps <= 13 x 9, C in (1, 3), N in (1, 3), sizes 2, 7, (3, 5)
ROI_CASES = [
    (1, 1, 9, 13, 2, 0.5, 0, True),
    (3, 3, 13, 9, 7, 0.25, 0, True),
    (3, 1, 13, 9, (3, 5), 0.25, 0, False),
    (1, 3, 8, 8, 2, 1.0, 3, True),
    (3, 3, 5, 7, 7, 1.0 / 32, 2, True),
    (1, 3, 7, 5, (3, 5), 1.0, 2, False),
    (3, 1, 8, 8, 2, 1.0, 0, False),
    (1, 1, 6, 11, 7, 0.5, 3, False),
]
ROI_STRIDE_CASE = dict(C=1024, H=2, W=2, out=2, repeats=100, distinct=41)      # n_out = 4100 * 1024 * 4 = 16 793 600 > 65536 * 256

# (Tn, H, C, K, head_major, dtype)
ATTN_CASES = [
    (1, 1, 1, 1, 0, "f32"), (2, 2, 3, 3, 1, "f32"), (49, 32, 64, 3, 1, "f32"), (63, 3, 4, 1, 1, "f64"), (64, 4, 5, 3, 0, "f32"),
    (65, 8, 257, 1, 0, "f64"), (255, 4, 260, 1, 1, "f64"), (256, 4, 3, 3, 1, "f32"), (256, 1, 64, 1, 0, "f64"), (65, 3, 260, 3, 1, "f32"),
    (256, 4, 64, 1, 0, "f64"),
]
ATTN_RN50 = [(49, 32, 2048, 2, 1, "f32"), (49, 32, 2048, 2, 1, "f64")]
ATTN_SPREAD = [(65, 4, 64, 3, 1, "f32"), (65, 4, 64, 3, 0, "f64"), (49, 3, 64, 3, 1, "f64"), (49, 3, 64, 3, 0, "f32")]
NP_DT = {"f32": np.float32, "f64": np.float64}
EPS_OF = {"f32": E, "f64": 2 * E64}
FLUSH_OF = {"f32": 2.0 ** -126, "f64": 2.0 ** -1022}


def ratio_np(got, want, bound):
    """worst |got - want| / bound over an array; inf for a NaN"""
    r = np.abs(np.asarray(got, np.float64) - want) / bound
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


# ===== class score ==========================================================================================================================
def cls_c(x_dtype, parts, oracle=False):
    ew = U if parts == 1 else U * U
    ex = U * U if x_dtype == "f32" else 0.0
    lolo = U * U if (parts == 2 and x_dtype == "f32") else 0.0
    nprod = D * (1 + (parts == 2) + (x_dtype == "f32"))
    c = (ew + ex + lolo + (nprod + 1) * E) * (1 + 2 * U)
    return c + E * (1 + c) if oracle else c


assert cls_c("f32", 2) == C_F32


def make_cls(T, classes, seed=0, x_dtype="f32", negative=False):
    """Gaussian operands: G (classes, 256), A = W^T W (256, 256) fp32, x (T, 256) fp32 or bf16 torch CPU tensors, scale.  negative: a common
    direction is added to every token and subtracted from every class so that every logit of every token is negative"""
    g = torch.Generator().manual_seed(7919 * seed + 13 * T + classes)
    x = torch.randn(T, D, generator=g)
    wp = torch.randn(64, D, generator=g).double() / 8
    text = torch.randn(classes, 64, generator=g).double()
    text = text / text.norm(dim=-1, keepdim=True)
    G = text @ wp
    if negative:      # every token gets +8 along the unit vector d, every class -8: the logits are near -64 (asserted by the tests)
        d = torch.ones(D, dtype=torch.float64) / 16
        x = (x.double() + 8.0 * d).float()
        G = G - 8.0 * d
    x = x.to(BF) if x_dtype == "bf16" else x.float()
    return {"G": G.float().contiguous(), "A": (wp.t() @ wp).float().contiguous(), "x": x.contiguous(), "scale": float(np.float32(1 / 0.07))}


def cls_reference(G, A, x, scale, x_dtype="f32", parts=2, oracle=False):
    """-> dict: s (T,) float64, bound (T,), logits (T, classes), m, n2, rho.  G, A fp32 (or float64 when `oracle`: the unrounded products)"""
    G, A, x = G.double(), A.double(), x.double()
    c = cls_c(x_dtype, parts, oracle)
    logits = x @ G.t()
    m = logits.max(dim=1).values
    Bm = c * (x.abs() @ G.abs().t()).max(dim=1).values
    Ax = x @ A.t()
    n2 = (x * Ax).sum(1)
    Q = (x.abs() * (x.abs() @ A.abs().t())).sum(1)
    Bn2 = (c + 258 * E * (1 + c)) * Q
    rho = Bn2 / n2
    ok = (rho < 1) & (n2 > 0)
    r = torch.where(ok, 0.5 * rho / (1 - rho.clamp(max=1 - 1e-12)) ** 1.5, torch.full_like(rho, float("inf")))
    k = (11 if oracle else 10) * E
    isq = n2.clamp(min=0) ** -0.5
    s = scale * m * isq
    bound = abs(scale) * isq * (Bm * (1 + r + k) + m.abs() * (r + k)) + TINY
    bound = torch.where(ok, bound, torch.full_like(bound, float("inf")))
    return {"s": s, "bound": bound, "logits": logits, "m": m, "n2": n2, "rho": rho}


def _split(t):
    hi = t.to(BF).float()
    return hi, (t - hi).to(BF).float()


def emulate_cls(G, A, x, scale, parts=2, permute=None):
    """the kernel's arithmetic in fp32 torch ops: split into hi + lo parts, the three (two, one) products, fmaf-like norm, fp32 epilogue.
    permute (a torch.Generator): the k sum, the class maximum and the norm's channel sum in a shuffled order"""
    W = torch.cat([G, A]).float()
    wh, wl = _split(W)
    xf32 = x.dtype == torch.float32
    xs = x.float()
    xh, xl = _split(xs) if xf32 else (xs, None)
    pk = torch.randperm(D, generator=permute) if permute is not None else torch.arange(D)
    acc = torch.zeros(x.shape[0], W.shape[0])
    if parts == 2:
        acc = acc + xh[:, pk] @ wl[:, pk].t()
    if xf32:
        acc = acc + xl[:, pk] @ wh[:, pk].t()
    acc = acc + xh[:, pk] @ wh[:, pk].t()
    classes = G.shape[0]
    m = acc[:, :classes].max(dim=1).values
    pj = torch.randperm(D, generator=permute) if permute is not None else torch.arange(D)
    n2 = (acc[:, classes:] * xs)[:, pj].sum(1)
    return torch.tensor(scale, dtype=torch.float32) * m / torch.sqrt(n2)


NORM_CH = np.arange(0, D, 4)                                   # channels that carry the norm (A = a a^T lives here)
LOGIT_CH = np.array([k for k in range(D) if k % 4])            # 192 channels: keys, the bias channel, the dense part


def cls_probe(T, classes, lo=None, negative=False, seed=0, x_dtype="f32"):
    """Exact probe (module docstring).  Token t: winner w(t) = t mod classes -- with T >= classes every row of every tile, the last
    partial tile and class classes - 1 win somewhere --, norm a . x_t = 2^p, p = t mod 5 - 2: neighbouring tokens, and the last token that
    rows past T are clamped to, differ in winner and norm.
      key channels: x_t[key(w)] = 1024, G_c[key(c)] = 1: the winner's logit is 1024 + noise, every other at most |noise| <= 214
      dense channels: G, x in {-1, 0, 1}; norm channels: G in {-1, 0, 1}, x two entries of magnitude <= 12
      negative: a bias channel with x = 1, G = -2048 for every class: every logit of every token is negative, the winner unchanged
      lo = "x": x_t[key(w)] = 1025 (hi 1024, lo 1) and the RIVAL class w ^ 1 gets the same dense / norm row and x_t[key(rival)] = 1024: the
                lo part of x alone decides (fp32 x only)
      lo = "G": G_c[key(c)] = 1 + 2^-10 on even classes (hi 1, lo 2^-10), winners are even, the rival w + 1 as above: G's lo part alone decides
    -> dict G, A, x, scale, winner (T,), rival (T,) or None"""
    assert classes + 2 <= len(LOGIT_CH) - 100 and lo in (None, "x", "G") and not (lo == "x" and x_dtype != "f32")
    rng = np.random.default_rng(1000 * seed + 3 * T + classes)
    key = LOGIT_CH[:classes]
    bias_ch = LOGIT_CH[classes]
    dense = LOGIT_CH[classes + 1:]
    G = np.zeros((classes, D))
    x = np.zeros((T, D))
    G[:, dense] = rng.integers(-1, 2, (classes, len(dense)))
    G[:, NORM_CH] = rng.integers(-1, 2, (classes, len(NORM_CH)))
    x[:, dense] = rng.integers(-1, 2, (T, len(dense)))
    G[np.arange(classes), key] = 1.0
    t = np.arange(T)
    if lo is None:
        winner, rival = t % classes, None
    else:
        assert classes >= 2
        winner = 2 * (t % (classes // 2))
        rival = winner + 1
        G[1::2] = np.where(np.isin(np.arange(D), key)[None], G[1::2], G[0:2 * (classes // 2):2])      # pairs share everything but the key
        if lo == "G":
            G[np.arange(0, classes, 2), key[0::2]] = 1.0 + 2.0 ** -10
    x[t, key[winner]] = 1025.0 if lo == "x" else 1024.0
    if rival is not None:
        x[t, key[rival]] = 1024.0
    if negative:
        G[:, bias_ch] = -2048.0
        x[:, bias_ch] = 1.0
    # the norm: a in {1, -2, 2, -1} on the norm channels, x_t = 3 * 2^p / a_j1 at j1, -2 * 2^p / a_j2 at j2:  a . x = 2^p
    a = np.zeros(D)
    a[NORM_CH] = np.tile([1.0, -2.0, 2.0, -1.0], len(NORM_CH) // 4)
    p = t % 5 - 2
    j1, j2 = NORM_CH[(5 * t + 1) % len(NORM_CH)], NORM_CH[(5 * t + 3) % len(NORM_CH)]
    x[t, j1] = 3.0 * 2.0 ** p / a[j1]
    x[t, j2] = -2.0 * 2.0 ** p / a[j2]
    xt = torch.from_numpy(x).float()
    return {"G": torch.from_numpy(G).float(), "A": torch.from_numpy(np.outer(a, a)).float(), "x": xt.to(BF) if x_dtype == "bf16" else xt,
            "scale": CLS_PROBE_SCALE, "winner": winner, "rival": rival, "p": p}


def _granularity(M):
    """per column k of M (rows, 256): the largest g in [-12, 12] with every M[:, k] a multiple of 2^g"""
    g = torch.full((M.shape[1],), -13, dtype=torch.int64)
    for e in range(-12, 13):
        v = M * 2.0 ** -e
        g = torch.where((v == v.round()).all(0) & (g == e - 1), torch.full_like(g, e), g)
    assert int(g.min()) >= -12
    return g


def cls_probe_expected(p):
    """-> (scores float32 (T,), argmax (T,)) from float64; asserts the probe's conditions"""
    G, A, x = p["G"].double(), p["A"].double(), p["x"].double()
    W = torch.cat([G, A])
    assert int((_granularity(W) + _granularity(x)).min()) >= -6, "a product that is no multiple of 2^-6"
    assert float((x.abs() @ W.abs().t()).max()) < 2.0 ** 18
    lo_w = (_split(W.float())[1] != 0).any(0)
    lo_x = (_split(x.float())[1] != 0).any(0) if p["x"].dtype == torch.float32 else torch.zeros(D, dtype=torch.bool)
    assert not (lo_w & lo_x).any(), "a lo * lo product"
    for t in (W, x):      # hi + lo is the value itself: nothing is lost in the split
        hi, lo = _split(t.float())
        assert torch.equal((hi + lo).double(), t)
    logits = x @ G.t()
    m, arg = logits.max(dim=1)
    n2 = (x * (x @ A.t())).sum(1)
    root = n2.sqrt()
    assert torch.equal(root, 2.0 ** torch.from_numpy(p["p"]).double()), "n2 is not the intended square"
    s = p["scale"] * m / root
    assert torch.equal(s.float().double(), s), "the expected score is not a float"
    assert np.array_equal(arg.numpy(), p["winner"])
    return s.float(), logits


def make_cls_conditioned(spread, T=193, classes=33, proj=256, seed=0):
    """Wp (proj, 256) = U diag(s) V^T with singular values spread geometrically over a factor `spread`, a text matrix, Gaussian tokens, and
    the tokens 0, 8, 16, ... aligned with the smallest singular direction (x = 16 v_min, + 1 % of a Gaussian on every second of them).
    -> float32 numpy wp, text, x and logit_scale"""
    rng = np.random.default_rng(100 * seed + spread)
    Uo, _ = np.linalg.qr(rng.standard_normal((proj, D)))
    Vo, _ = np.linalg.qr(rng.standard_normal((D, D)))
    sv = spread ** (-np.arange(D) / (D - 1.0))                       # 1 ... 1 / spread
    wp = (Uo * sv) @ Vo.T / 2
    x = rng.standard_normal((T, D))
    al = np.arange(0, T, 8)
    x[al] = 16 * Vo[:, -1]
    x[al[1::2]] += 0.16 * rng.standard_normal((len(al[1::2]), D))
    text = rng.standard_normal((classes, proj))
    return wp.astype(np.float32), text.astype(np.float32), x.astype(np.float32), np.float32(np.log(1 / 0.07)), al


def scorer_operands(wp, text):
    """what ClassScorer._pack forms: float64 products (G64, A64) and their fp32 roundings"""
    wp, te = torch.from_numpy(wp).double(), torch.from_numpy(text).double()
    te = te / te.norm(dim=-1, keepdim=True)
    G64, A64 = te @ wp, wp.t() @ wp
    return G64, A64, G64.float().contiguous(), A64.float().contiguous()


# ===== ROIAlign =============================================================================================================================
def kernel_scale(scale, dtype):
    """the spatial_scale the kernel computes with: the double, cast to T"""
    return float(np.float32(scale)) if dtype in ("f32", np.float32) else float(scale)


def _axis(pos, size, dt):
    valid = ~((pos < dt(-1)) | (pos > dt(size))) & np.isfinite(pos)
    p = np.where(valid & (pos > 0), pos, dt(0)).astype(dt)
    low = p.astype(np.int64)
    top = low >= size - 1
    low = np.where(top, size - 1, low)
    high = np.where(top, size - 1, low + 1)
    p = np.where(top, low.astype(dt), p)
    l = (p - low.astype(dt)).astype(dt)
    return valid, low, high, l, (dt(1) - l).astype(dt)


def roi_geometry(roi, out_size, scale, ratio, aligned, dt=np.float64):
    """one roi (5,) in dtype dt -> None (refused: zeros) or (start_h, start_w, bin_h, bin_w, gh, gw, roi_h, roi_w, P) as the kernel forms them"""
    PH, PW = (out_size, out_size) if isinstance(out_size, int) else out_size
    roi = np.asarray(roi, dt)
    sc, off = dt(scale), dt(0.5 if aligned else 0.0)
    with np.errstate(all="ignore"):
        sw, sh, ew, eh = roi[1] * sc - off, roi[2] * sc - off, roi[3] * sc - off, roi[4] * sc - off
        rw, rh = ew - sw, eh - sh
        if not aligned:
            rw, rh = (rw if rw > 1 else dt(1)), (rh if rh > 1 else dt(1))
        if not all(np.isfinite(v) for v in (sw, sh, rw, rh)):
            return None
        bh, bw = rh / dt(PH), rw / dt(PW)
        if ratio > 0:
            gh = gw = ratio
        else:
            fh, fw = np.ceil(rh / dt(PH)), np.ceil(rw / dt(PW))
            if fh > ROI_MAX_GRID or fw > ROI_MAX_GRID:
                return None
            gh, gw = max(int(fh), 0), max(int(fw), 0)
    P = max(abs(float(sw)), abs(float(sh)), abs(float(sw + rw)), abs(float(sh + rh)), abs(float(ew)), abs(float(eh)), 1.0)
    return sh, sw, bh, bw, gh, gw, rh, rw, P


def roi_align_ref(inp, rois, out_size, scale, ratio, aligned, dt=np.float64, reverse=False):
    """the kernel's definition, every operation in dtype dt (float64: the reference; float32: the emulation), vectorised over channels,
    bins and samples; reverse: the samples of a bin are added in the opposite order.  scale: see kernel_scale"""
    PH, PW = (out_size, out_size) if isinstance(out_size, int) else out_size
    inp, rois = np.asarray(inp).astype(dt), np.asarray(rois).astype(dt)
    N, C, H, W = inp.shape
    out = np.zeros((rois.shape[0], C, PH, PW), dt)
    for k, roi in enumerate(rois):
        b = roi[0]
        if not (np.isfinite(b) and 0 <= int(b) < N and b > -1):
            continue
        geo = roi_geometry(roi, out_size, scale, ratio, aligned, dt)
        if geo is None:
            continue
        sh, sw, bh, bw, gh, gw = geo[:6]
        if gh * gw == 0:
            continue
        ph, iy = np.arange(PH).astype(dt)[:, None], np.arange(gh).astype(dt)[None, :]
        pw, ix = np.arange(PW).astype(dt)[:, None], np.arange(gw).astype(dt)[None, :]
        y = (sh + ph * bh + (iy + dt(0.5)) * bh / dt(gh)).astype(dt)          # (PH, gh)
        x = (sw + pw * bw + (ix + dt(0.5)) * bw / dt(gw)).astype(dt)          # (PW, gw)
        vy, yl, yh, ly, hy = _axis(y, H, dt)
        vx, xl, xh, lx, hx = _axis(x, W, dt)
        plane = inp[int(b)]
        Y = lambda a: a[None, :, :, None, None]
        X = lambda a: a[None, None, None, :, :]
        g = lambda yi, xi: plane[:, yi[:, :, None, None], xi[None, None, :, :]]
        val = (Y(hy) * X(hx) * g(yl, xl) + Y(hy) * X(lx) * g(yl, xh) + Y(ly) * X(hx) * g(yh, xl) + Y(ly) * X(lx) * g(yh, xh)).astype(dt)
        val = np.where(Y(vy) & X(vx), val, dt(0))
        acc = np.zeros((C, PH, PW), dt)
        order = [(i, j) for i in range(gh) for j in range(gw)]
        for i, j in (reversed(order) if reverse else order):
            acc = (acc + val[:, :, i, :, j]).astype(dt)
        out[k] = acc / dt(gh * gw)
    return out


def roi_conditions(rois, out_size, scale, ratio, aligned, H, W):
    """float64 -> dict: int_dist (smallest distance of a roi / bins from an integer; inf with a fixed grid), edge_dist (smallest distance of
    a sample from -1 and from the map's size), gh, gw, P per ROI (refused ROIs: grid 0, P 1)"""
    PH, PW = (out_size, out_size) if isinstance(out_size, int) else out_size
    int_dist = edge_dist = float("inf")
    gh_a, gw_a, P_a = [], [], []
    for roi in np.asarray(rois, np.float64):
        geo = roi_geometry(roi, out_size, scale, ratio, aligned)
        if geo is None:
            gh_a.append(0), gw_a.append(0), P_a.append(1.0)
            continue
        sh, sw, bh, bw, gh, gw, rh, rw, P = geo
        gh_a.append(gh), gw_a.append(gw), P_a.append(P)
        for start, per_bin, bins, grid, size in ((sh, bh, PH, gh, H), (sw, bw, PW, gw, W)):
            if ratio <= 0:
                int_dist = min(int_dist, abs(per_bin - round(per_bin)))
            for pb in range(bins):
                for i in range(grid):
                    pos = start + pb * per_bin + (i + 0.5) * per_bin / grid
                    edge_dist = min(edge_dist, abs(pos + 1.0), abs(pos - size))
    return {"int_dist": int_dist, "edge_dist": edge_dist, "gh": np.array(gh_a), "gw": np.array(gw_a), "P": np.array(P_a)}


def roi_bound(inp, rois, cond, dtype):
    """(K, C, 1, 1): (64 P + gh gw + 16) eps M"""
    N = inp.shape[0]
    M = np.abs(np.asarray(inp, np.float64)).max((2, 3))                       # (N, C)
    b = np.clip(np.nan_to_num(np.asarray(rois, np.float64)[:, 0]), 0, N - 1).astype(int)
    k = 64 * cond["P"] + cond["gh"] * cond["gw"] + 16
    return (k[:, None] * M[b] * EPS_OF[dtype])[:, :, None, None] + TINY


def make_roi_case(case, seed=0):
    """-> (inp float32 (N, C, H, W), rois float32 (9, 5)): random boxes inside the map; 0 sticks out on the top left, 1 on the bottom right, 2
    is smaller than a bin (the boxes of tests/test_gpu_roi.py), the batch indices cover 0 .. N - 1"""
    N, C, H, W, out, scale, ratio, aligned = case
    rng = np.random.default_rng(1000 * seed + 97 * H + 7 * W + ratio + 3 * N)
    inp = rng.standard_normal((N, C, H, W)).astype(np.float32)
    K = 9
    cx, cy = rng.uniform(0.2, 0.8, K) * W, rng.uniform(0.2, 0.8, K) * H
    w, h = rng.uniform(0.05, 0.4, K) * W, rng.uniform(0.05, 0.4, K) * H
    box = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)      # in map pixels
    box[0] = [-1.5625, -0.9375, 1.25, 1.875]
    box[1] = [W - 0.625, H - 0.625, W + 2.8125, H + 2.1875]
    box[2] = [0.3125, 0.3125, 0.328125, 0.31875]
    idx = np.arange(K) % N
    idx[-1] = N - 1
    rois = np.concatenate([idx[:, None].astype(np.float64), box / scale], 1).astype(np.float32)
    return inp, rois


def make_roi_stride(s=None):
    """the grid-stride case: -> (inp float32 (1, C, H, W), the `distinct` rois float32 the call repeats `repeats` times)"""
    s = s or ROI_STRIDE_CASE
    rng = np.random.default_rng(77)
    inp = rng.standard_normal((1, s["C"], s["H"], s["W"])).astype(np.float32)
    x1, y1 = rng.uniform(-0.3, 1.0, s["distinct"]), rng.uniform(-0.3, 1.0, s["distinct"])
    box = np.stack([x1, y1, x1 + rng.uniform(0.2, 1.5, s["distinct"]), y1 + rng.uniform(0.2, 1.5, s["distinct"])], 1)
    return inp, np.concatenate([np.zeros((s["distinct"], 1)), box], 1).astype(np.float32)


def roi_probe_map(N, C, H, W, seed=0):
    """integer map values in [-8, 8], no two images or channels alike"""
    return np.random.default_rng(seed + 10 * H + W).integers(-8, 9, (N, C, H, W)).astype(np.float64)


def roi_probe_groups(H=5, W=6, N=3):
    """The dyadic probes at the discontinuities: a list of (name, out_size, spatial_scale, sampling_ratio, aligned, rois (K, 5) float64,
    notes), notes[i] a word on ROI i.  Every coordinate is a multiple of 2^-3 and spatial_scale = 1 unless said: start, bin, bin / grid
    are dyadic."""
    g = []
    # fixed grid 1, 2 x 2 bins of size 1: the two samples of an axis are start + 0.5 and start + 1.5, start = coordinate - 0.5
    g.append(("cutoffs", 2, 1.0, 1, True, np.array([
        [0, 1.0, -1.0, 3.0, 1.0],                        # y samples -1 (taken, clamped to row 0) and 0
        [1, -1.0, 1.0, 1.0, 3.0],                        # the same on x
        [0, 1.0, -1.125, 3.0, 0.875],                    # y samples -1 - 2^-3 (contributes 0) and -2^-3
        [2, -1.125, 1.0, 0.875, 3.0],                    # the same on x
        [0, 1.0, H - 1.0, 3.0, H + 1.0],                 # y samples H - 1 and exactly H (taken from the last row)
        [1, W - 1.0, 1.0, W + 1.0, 3.0],                 # x samples W - 1 and exactly W
        [2, 1.0, H - 0.875, 3.0, H + 1.125],             # y samples H - 1 + 2^-3 and H + 2^-3 (contributes 0)
        [0, W - 0.875, 1.0, W + 1.125, 3.0],             # the same on x
        [N - 1, 1.0, 1.0, 3.0, 3.0],                     # batch index N - 1
        [N, 1.0, 1.0, 3.0, 3.0],                         # batch index N: zeros
        [-1, 1.0, 1.0, 3.0, 3.0],                        # batch index -1: zeros
    ]), ("y=-1", "x=-1", "y=-1-1/8", "x=-1-1/8", "y=H", "x=W", "y=H+1/8", "x=W+1/8", "batch N-1", "batch N", "batch -1")))
    g.append(("cutoffs grid 2", 2, 1.0, 2, True, np.array([
        [0, 1.0, -1.5, 3.0, 2.5],                        # bin 2, samples start + 0.5, 1.5, 2.5, 3.5 = -1.5 (0), -0.5, 0.5, 1.5
        [1, 1.0, -1.0, 3.0, 3.0],                        # samples -1 (taken), 0, 1, 2
        [2, 1.0, H - 3.0, 3.0, H + 1.0],                 # samples H - 3, H - 2, H - 1, H (taken)
        [0, W - 3.0, 1.0, W + 1.0, 3.0],
    ]), ("y=-1.5", "y=-1", "y=H", "x=W")))
    g.append(("adaptive", 2, 1.0, 0, True, np.array([
        [0, 1.0, 1.0, 5.0, 5.0],                         # roi / bins = 2 exactly: grid 2, not 3
        [1, 0.5, 0.5, 2.5, 4.5],                         # roi_w / 2 = 1: grid 1; roi_h / 2 = 2: grid 2
        [2, 0.0, 0.0, 4.0, 8.0],                         # roi_h / 2 = 4: grid 4 (the lower samples fall past H: zeros)
        [0, 1.0, 1.0, 4.0, 4.0],                         # roi / bins = 1.5: grid 2
        [1, 2.0, 3.0, 2.0, 3.0],                         # zero-size box: grid 0, exact zeros
        [2, 3.0, 1.0, 1.0, 3.0],                         # inverted on x: exact zeros
        [0, 1.0, 3.0, 3.0, 1.0],                         # inverted on y
    ]), ("integer 2", "integer 1 and 2", "integer 4", "1.5", "zero size", "inverted x", "inverted y")))
    g.append(("adaptive scale 1/2", (2, 4), 0.5, 0, True, np.array([
        [1, 2.0, 2.0, 10.0, 10.0],                       # start 0.5, roi 4: bins 2 (grid 2) and 1 (grid 1)
        [N - 1, 3.0, 1.0, 11.0, 5.0],
    ]), ("scale 1/2", "scale 1/2")))
    g.append(("legacy", 2, 1.0, 0, False, np.array([
        [0, 1.0, 2.0, 1.25, 2.25],                       # size 0.25 -> clamped to 1: bin 0.5, grid 1, samples 1.25, 1.75 / 2.25, 2.75
        [1, 2.0, 1.0, 2.0, 1.0],                         # zero size -> 1 x 1
        [2, 3.0, 3.0, 1.0, 1.0],                         # inverted -> clamped to 1 x 1
        [0, 0.0, 0.0, 4.0, 2.0],                         # roi_w / 2 = 2 exactly, roi_h / 2 = 1 exactly
    ]), ("clamp to 1", "zero size", "inverted", "integer")))
    return g


def roi_cap_rois():
    """(rois float64 (8, 5) for output 2, scale 1, adaptive, aligned; refused (8,) bool): just over the cap on one axis, +inf, NaN, among
    ordinary boxes, and one box exactly AT the cap on y (4096 x 1 samples per bin, integer positions: not refused, exact)"""
    big = 2.0 * ROI_MAX_GRID
    rois = np.array([
        [0, 1.0, 1.0, 3.0, 3.0],
        [0, 1.0, 0.0, 1.5, big + 1.0],                   # roi_h / 2 = 4096.5 -> grid 4097 > cap
        [0, 1.5, 1.5, 3.5, 3.5],
        [0, 1.0, 1.0, float("inf"), 3.0],
        [0, 1.0, float("nan"), 3.0, 3.0],
        [0, 0.5, 0.5, 2.5, 2.5],
        [0, 0.0, 1.0, big + 0.5, 1.5],                   # roi_w / 2 = 4096.25 -> grid 4097 on x
        [0, 1.0, 1.0, 1.5, big + 1.0],                   # roi_h / 2 = 4096 exactly -> grid 4096: inside the cap
    ])
    return rois, np.array([False, True, False, True, True, False, True, False])


def linear_map(N, C, H, W, dyadic=True):
    """f(y, x) = a y + b x + c per (image, channel): -> (map float64, coefficients (N, C, 3))"""
    rng = np.random.default_rng(H * 100 + W)
    co = rng.integers(-8, 9, (N, C, 3)) / 4.0 if dyadic else rng.standard_normal((N, C, 3))
    co = co.astype(np.float32).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    m = co[..., 0, None, None] * yy + co[..., 1, None, None] * xx + co[..., 2, None, None]
    return m, co


def linear_closed_form(co, rois, out_size, scale, aligned):
    """bin (ph, pw) of a ROI whose samples all lie in [0, H - 1] x [0, W - 1] equals f at the bin's centre (independent of the oracle)"""
    PH, PW = (out_size, out_size) if isinstance(out_size, int) else out_size
    rois = np.asarray(rois, np.float64)
    off = 0.5 if aligned else 0.0
    sw, sh = rois[:, 1] * scale - off, rois[:, 2] * scale - off
    rw, rh = rois[:, 3] * scale - off - sw, rois[:, 4] * scale - off - sh
    if not aligned:
        rw, rh = np.maximum(rw, 1.0), np.maximum(rh, 1.0)
    cy = sh[:, None] + (np.arange(PH) + 0.5) * rh[:, None] / PH          # (K, PH)
    cx = sw[:, None] + (np.arange(PW) + 0.5) * rw[:, None] / PW
    c = co[rois[:, 0].astype(int)]                                       # (K, C, 3)
    return c[:, :, 0, None, None] * cy[:, None, :, None] + c[:, :, 1, None, None] * cx[:, None, None, :] + c[:, :, 2, None, None]


def linear_rois(H, W, N, scale, dyadic):
    """boxes whose samples stay inside [0, H - 1] x [0, W - 1] (map pixels [1, size - 2] at scale 1, aligned)"""
    if dyadic:      # sizes 2 and 4: bins and bin / grid dyadic for output 2
        box = np.array([[1.5, 1.5, 3.5, 3.5], [0.5, 1.0, 4.5, 3.0], [1.0, 0.5, 3.0, 2.5], [2.0, 1.5, 4.0, 3.5]])
    else:
        rng = np.random.default_rng(5)
        x1, y1 = rng.uniform(0.6, W / 2 - 1, 6), rng.uniform(0.6, H / 2 - 1, 6)
        box = np.stack([x1, y1, x1 + rng.uniform(0.7, W / 2 - 0.5, 6), y1 + rng.uniform(0.7, H / 2 - 0.5, 6)], 1)
    idx = (np.arange(len(box)) % N).astype(np.float64)
    return np.concatenate([idx[:, None], box / scale], 1).astype(np.float32).astype(np.float64)


# ===== attention pool core ====================================================================================================================
def attn_rows(K, H, head_major):
    """row of (k, h) in u, spos and z: (K, H) int array"""
    k, h = np.meshgrid(np.arange(K), np.arange(H), indexing="ij")
    return h * K + k if head_major else k * H + h


def make_attn(case, seed=0, spread=0.0):
    """-> dict u (K H, C), feat (K, C, Tn), pos (Tn + 1, C), spos (K H, Tn + 1) in the case's dtype (float64 copies are exact).  spread: spos
    is drawn uniformly from +-spread (scores of that size)"""
    Tn, H, C, K, hm, dtype = case
    rng = np.random.default_rng(1000 * seed + 31 * Tn + 7 * H + C + K)
    dt = NP_DT[dtype]
    u = rng.standard_normal((K * H, C)) * C ** -0.5
    feat = rng.standard_normal((K, C, Tn))
    pos = rng.standard_normal((Tn + 1, C)) * 0.5
    spos = rng.uniform(-spread, spread, (K * H, Tn + 1)) if spread else rng.standard_normal((K * H, Tn + 1))
    return {"u": u.astype(dt), "feat": feat.astype(dt), "pos": pos.astype(dt), "spos": spos.astype(dt)}


def attn_reference(p, case):
    """float64 -> dict z (K H, C), bound, a (K H, Tn + 1) (the weights), ea (their bound)"""
    Tn, H, C, K, hm, dtype = case
    eps, flush = EPS_OF[dtype], FLUSH_OF[dtype]
    u, feat, pos, spos = (np.asarray(p[n], np.float64) for n in ("u", "feat", "pos", "spos"))
    rows = attn_rows(K, H, hm)                                         # (K, H)
    ur = u[rows]                                                       # (K, H, C)
    sf = np.einsum("khc,kct->kht", ur, feat)
    S = np.einsum("khc,kct->kht", np.abs(ur), np.abs(feat))
    sp = spos[rows]                                                    # (K, H, Tn + 1)
    score = np.concatenate([sp[..., :1] + sf.mean(-1, keepdims=True), sf + sp[..., 1:]], -1)
    e_f = (C + 5) * eps * S
    e_s = np.concatenate([e_f.mean(-1, keepdims=True) + (Tn + 3) * eps * (S.mean(-1, keepdims=True) + np.abs(sp[..., :1])),
                          e_f + eps * (S + np.abs(sp[..., 1:]))], -1)
    d = score - score.max(-1, keepdims=True)
    w = np.exp(d)
    a = w / w.sum(-1, keepdims=True)
    delta = e_s + e_s.max(-1, keepdims=True) + eps * np.abs(d)
    r = np.expm1(delta)
    r = r + EXP_ULPS_E * eps * (1 + r)
    rs = r.max(-1, keepdims=True) + (Tn + 4) * eps
    assert float(rs.max()) < 0.5, "scores too inaccurate for a bound"
    ea = a * ((r + rs) / (1 - rs) + 4 * eps) + flush
    fp = feat.transpose(0, 2, 1) + pos[None, 1:]                       # (K, Tn, C)
    m0 = feat.mean(-1) + pos[0]                                        # (K, C)
    e_m0 = (Tn + 2) * eps * (np.abs(feat).mean(-1) + np.abs(pos[0]))
    z = a[..., :1] * m0[:, None] + np.einsum("kht,ktc->khc", a[..., 1:], fp)
    mag = a[..., :1] * np.abs(m0)[:, None] + np.einsum("kht,ktc->khc", a[..., 1:], np.abs(fp))
    bound = (np.einsum("kht,ktc->khc", ea[..., 1:], np.abs(fp)) + ea[..., :1] * np.abs(m0)[:, None] + a[..., :1] * e_m0[:, None]
             + (Tn + 4) * eps * mag + TINY)
    zr, br = np.zeros((K * H, C)), np.zeros((K * H, C))
    zr[rows], br[rows] = z, bound
    return {"z": zr, "bound": br, "a": a, "ea": ea}


def emulate_attn(p, case, permute=None):
    """the kernel's steps in the case's own dtype with numpy: four wave partial sums folded, scores, max subtraction, exp, 1 / sum, the
    (Tn + 2)-term z.  permute (a numpy Generator): channels and tokens in a shuffled order.  -> (z (K H, C), weights (K, H, Tn + 1))"""
    Tn, H, C, K, hm, dtype = case
    dt = NP_DT[dtype]
    u, feat, pos, spos = (np.asarray(p[n], dt) for n in ("u", "feat", "pos", "spos"))
    rows = attn_rows(K, H, hm)
    pc = permute.permutation(C) if permute is not None else np.arange(C)
    pt = permute.permutation(Tn) if permute is not None else np.arange(Tn)
    ur = u[rows]
    prod = (ur[:, :, pc, None] * feat[:, None, pc, :]).astype(dt)                       # (K, H, C, Tn)
    part = [prod[:, :, w::4].sum(2, dtype=dt) for w in range(4)]
    sf = dt(0)
    for q in part:
        sf = (sf + q).astype(dt)
    sp = spos[rows]
    s0 = (sp[..., 0] + sf[..., pt].sum(-1, dtype=dt) / dt(Tn)).astype(dt)
    st = (sf + sp[..., 1:]).astype(dt)
    mx = np.maximum(s0, st.max(-1))
    e = np.exp((st - mx[..., None]).astype(dt)).astype(dt)
    e0 = np.exp((s0 - mx).astype(dt)).astype(dt)
    inv = (dt(1) / (e[..., pt].sum(-1, dtype=dt) + e0)).astype(dt)
    a = np.concatenate([(e0 * inv)[..., None], e * inv[..., None]], -1).astype(dt)
    fp = (feat.transpose(0, 2, 1) + pos[None, 1:]).astype(dt)                            # (K, Tn, C)
    m0 = (feat[:, :, pt].sum(-1, dtype=dt) / dt(Tn) + pos[0]).astype(dt)
    terms = (a[..., 1:, None] * fp[:, None]).astype(dt)                                  # (K, H, Tn, C)
    z = ((a[..., :1] * m0[:, None]).astype(dt) + terms[:, :, pt].sum(2, dtype=dt)).astype(dt)
    zr = np.zeros((K * H, C), dt)
    zr[rows] = z
    return zr, a


def attn_probe_values(K, C, Tn):
    """dyadic feat (K, C, Tn) and pos (Tn + 1, C), multiples of 2^-2, no two ROIs / channels / tokens alike.  f[k, c, t] = base[k, c] + d[t]
    with sum_t d = 0: the sum over t is Tn base without rounding and its division by Tn gives base exactly, whatever Tn"""
    rng = np.random.default_rng(10000 * K + 100 * C + Tn)
    base = rng.integers(-64, 65, (K, C, 1)) / 4.0
    r = rng.integers(1, 9, (Tn + 1) // 2) / 4.0
    d = np.stack([r, -r], 1).reshape(-1)[:Tn].copy()                   # the pairs (2 i, 2 i + 1) cancel
    if Tn % 2:
        d[-1] = 0.0
    assert float(d.sum()) == 0.0
    feat = base + d[None, None, :]
    pos = rng.integers(-64, 65, (Tn + 1, C)) / 4.0
    return feat.astype(np.float64), pos.astype(np.float64)


def attn_uniform_probe(case):
    """u = 0, spos = 0, Tn + 1 a power of two: every weight is 1 / (Tn + 1) exactly, z = (mean_t f + pos_0 + sum_t (f_t + pos_{1+t})) / (Tn + 1):
    multiples of 2^-2 below 2^15 summed, then an exact scaling.  -> (operands, z (K H, C) float64)"""
    Tn, H, C, K, hm, dtype = case
    assert (Tn + 1) & Tn == 0
    feat, pos = attn_probe_values(K, C, Tn)
    dt = NP_DT[dtype]
    p = {"u": np.zeros((K * H, C), dt), "feat": feat.astype(dt), "pos": pos.astype(dt), "spos": np.zeros((K * H, Tn + 1), dt)}
    base = feat.mean(-1)
    assert np.array_equal(base * 4, np.round(base * 4)) and np.array_equal(feat.sum(-1), base * Tn)
    zk = (base + pos[0] + (feat.transpose(0, 2, 1) + pos[None, 1:]).sum(1)) / (Tn + 1)          # (K, C)
    assert float(np.abs(zk).max()) * (Tn + 1) < 2.0 ** 15
    z = np.zeros((K * H, C))
    z[attn_rows(K, H, hm)] = zk[:, None]
    return p, z


def attn_select_probe(case, shift=0):
    """u = 0, spos = -1000 but 0 at ONE token per (ROI, head): sel(k, h) = (k H + h + shift) mod (Tn + 1) -- every head of a group and every
    ROI another token, the mean token 0 among them (its mean is exact: attn_probe_values).
    z[row] = f[k, :, sel - 1] + pos[sel] (sel >= 1), mean_t f[k] + pos[0] (sel = 0), bit for bit.  -> (operands, z float64, sel (K, H))"""
    Tn, H, C, K, hm, dtype = case
    feat, pos = attn_probe_values(K, C, Tn)
    dt = NP_DT[dtype]
    rows = attn_rows(K, H, hm)
    k, h = np.meshgrid(np.arange(K), np.arange(H), indexing="ij")
    sel = (k * H + h + shift) % (Tn + 1)
    spos = np.full((K * H, Tn + 1), -1000.0)
    spos[rows, sel] = 0.0
    z = np.zeros((K * H, C))
    for kk in range(K):
        for hh in range(H):
            s = sel[kk, hh]
            z[rows[kk, hh]] = feat[kk].mean(-1) + pos[0] if s == 0 else feat[kk, :, s - 1] + pos[s]
    p = {"u": np.zeros((K * H, C), dt), "feat": feat.astype(dt), "pos": pos.astype(dt), "spos": spos.astype(dt)}
    return p, z, sel


ATTN_UNIFORM = [(1, 2, 5, 2, 0, "f32"), (63, 4, 5, 2, 1, "f32"), (255, 4, 260, 1, 0, "f64"), (63, 3, 257, 2, 1, "f64"), (255, 1, 3, 1, 0, "f32")]
# every token in turn: K H >= Tn + 1, so sel covers every token
ATTN_SELECT = [(2, 4, 5, 1, 1, "f32"), (2, 1, 3, 3, 0, "f64"), (65, 4, 5, 17, 1, "f32"), (65, 4, 5, 17, 0, "f64"), (65, 3, 6, 22, 1, "f64"),
               (65, 3, 6, 22, 0, "f32"), (64, 8, 4, 9, 0, "f32"), (64, 2, 4, 33, 1, "f64")]
