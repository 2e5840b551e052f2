"""Float64 restatements of the feed-forward family (richsem_amd/csrc/ffn_mfma.hip, lin256_mfma.hip) with an ELEMENT-WISE error bound for
every tensor the kernels write, and fp32 emulations with the kernels' rounding points.  The comparator of tests/test_gpu_ffn_bounds.py
(the kernels against the bounds) and of tests/test_ffn_ref.py (the emulations against the bounds: the check that a correct
implementation can meet them).  Test helper only: the package never imports it.

All inputs are bf16 or fp32 values, so their float64 copies are exact and the float64 results are the reference (their own error,
2^-53 relative per operation, is nine orders below every bound here).

Notation.  u = 2^-8 is the unit round-off of bf16 under round-to-nearest-even (pack_bf16), e = 2^-24 that of fp32.  An fp32 sum of n
terms, in ANY order, errs by at most (n - 1) e sum|term| to first order; the bounds below write n e (or (n + k) e where k further
roundings touch the same magnitude) and never rely on the order.  Means are sums times 2^-8, which is exact.  D = 256 channels.
1e-30 (TINY) is added to every bound so that exact zeros compare.

LayerNorm core (_ln), shared by add_layernorm and the fused forward.  z is the exact LayerNorm input, e_in[t, c] a bound on the error
of the fp32 value the kernel holds for it.  Exact:  m = mean_c z,  d = z - m,  var = mean_c d^2,  rstd = (var + eps)^-1/2,
yhat = d rstd,  out = yhat gamma + beta.  The kernels compute the statistics in two passes (sum, then sum of squared differences):
    m      e_m   = mean e_in + (D + 1) e mean(|z| + e_in)                    the input errors, the 256-term sum
    d      e_d   = e_in + e_m + e |d|                                        (+ the subtraction's rounding)
    var    e_var = mean(2 |d| e_d + e_d^2) + (D + 3) e var                   d^2, the 256-term sum, * 1/256, + eps
    rstd   rho = e_var / (var + eps);  |rstd_got / rstd - 1| <= r_rel = rho / 2 / (1 - rho)^3/2 + 6 e
           (the mean-value bound of x^-1/2 on [1 - rho, 1 + rho]; 6 e: rsqrtf within 2 ulp = 4 e, the roundings of var / 256 + eps
           2 e; rho is capped at 1/2; eps is the float the kernel is handed, EPS32)
    yhat   e_yh  = rstd e_d (1 + r_rel) + |yhat| r_rel + 2 e |yhat|          in fp32, then ONE bf16 rounding:
           B_yhat = e_yh + u (|yhat| + e_yh)
    out    e_o   = |gamma| e_yh + 2 e (|yhat gamma| + |out|),   B_out = e_o + u (|out| + e_o)
    B_rstd = rstd r_rel
To first order |yhat| r_rel = rstd |yhat| mean(|yhat| e_d), so e_yh is the cancellation-aware form
rstd (e_d + |yhat| mean(|yhat| e_d)) with the second-order factors (1 + r_rel), (1 - rho)^-3/2 kept.
A CONSTANT row of one bf16 value v (and b absent or zero) is exact: 4 v, then the doubling exchanges, give 256 v without rounding,
m = v, d = 0, var = 0: yhat = 0, out = bf16(beta), rstd = rsqrt(eps); the tests assert that separately.

add_layernorm(a, b):  z = a + b is rounded once to fp32 (the operands are bf16 of possibly distant exponents): e_in = e |z|.

ffn_ln_backward, GIVEN the dy, yhat (bf16), rstd, gamma (fp32) the kernel is handed:
    g = dy gamma,  A = mean_c g,  Bm = mean_c (g yhat),  dz = rstd (g - A - yhat Bm)
    fp32:  g: e |g|;  A: (D + 1) e mean|g|;  g yhat: 2 e;  Bm: (D + 2) e mean|g yhat|;  yhat Bm, the two subtractions, the product
    with rstd: each one rounding at the magnitude of its result, all <= |g| + |A| + |yhat Bm|:
        e_z = e rstd (4 |g| + (D + 4) mean|g| + (D + 5) |yhat| mean|g yhat| + 3 (|A| + |yhat| |Bm|))
    B_dz = e_z + u (|dz| + e_z)                       -- the bf16 rounding scales with |dz| itself, the fp32 terms with the operands
    dgamma = sum_t dy yhat,  dbeta = sum_t dy,  db2 = sum_t dz (the fp32 z, before its rounding); the order of the token sum is not
    fixed (registers per wave, LDS across waves, atomics across workgroups):
        B_sum = (T + 3) e sum_t |term|        (+ sum_t e_z for db2, whose terms carry their own fp32 error)

lin256 (epilogues 0: x W^T + b, 1: relu of it, 2: (x W^T) * (mask > 0), 3: rows with a set mask byte zeroed; and the stacked layout):
    256 exact products (bf16 x bf16 fits fp32) summed in fp32, the bias added, one bf16 rounding:
        B = u |out| + 257 e (sum_k |x_k| |w_nk| + |b_n|)
    (relu is 1-Lipschitz and keeps 0: the same bound).  Elements masked by epilogue 2 and rows masked by epilogue 3 must be exactly 0.

lin256_f32: x = xh + xl + rx with xh = bf16(x), xl = bf16(x - xh) (x - xh is exact in fp32), |xl| <= u |x|, |rx| <= u |x - xh| <= u^2 |x|;
    the same for w.  The kernel sums xh wh + xh wl + xl wh.  What is missing from x w:
        xl wl       <= u^2 |x| |w|           the dropped lo * lo product
        rx w, x rw  <= 2 u^2 |x| |w|         the bf16 rounding of the two lo parts          (products of these three: O(u^3))
    and the three products per k are exact in fp32, 768 of them summed: 768 e sum|products| <= 768 e (1 + 2 u) sum|x||w|; the bias
    is added once more (e at the magnitude of the result <= sum|x||w| + |b|):
        c = (3 u^2 + 769 e) (1 + 2 u) = 9.24e-5,      B = c (sum_k |x_k| |w_nk| + |b_n|)
    (Typical errors are far smaller -- lo parts rarely round by their worst case -- so an exact probe backs this bound up:
    exact_f32_probe builds operands whose three products and all partial sums are exact in fp32 in any order.)

Fused forward, out = LayerNorm(x + W2 relu(W1 x + b1) + b2):
    p = W1 x + b1 in fp32 (the bias is the accumulator's initial value):       e_p = (D + 2) e (sum_k |w1| |x| + |b1|)
    h = bf16(relu(p)):                                                         e_h = e_p + u (h + e_p)     (0 where p < -e_p)
    y = sum_j w2 h_j + (b2 + x): exact products, d_ffn terms, two more adds:   e_y = sum_j |w2_cj| e_h_j + (F + 3) e (sum_j |w2| (h + e_h) + |b2| + |x|)
    then the LayerNorm core with e_in = e_y.  This is a WORST-CASE bound: every h rounds against its channel.  At d_ffn = 2048 it is
    about 0.3 max(1, |out|) -- a net against wild values.  The sharp comparator is the emulation.

Emulation of the fused forward (emulate_ffn): torch ops in fp32 with the kernel's rounding points -- h to bf16 after bias and ReLU, out and
yhat to bf16, everything else fp32, acc + (b2 + x) as the kernel adds them, two-pass statistics, rsqrt.  Two correct implementations
differ from each other only where an fp32 summation order moves a value across a bf16 rounding tie (a flipped h also disturbs its
token's row a little), so the test counts elements whose bf16 bits differ (mismatch_shares) and caps the counts (CAPS).  The caps are
conditions: tests/test_ffn_ref.py checks that three correct implementations (fp32, fp32 with permuted summation order, float64
arithmetic) meet them pairwise.
"""
import torch

U = 2.0 ** -8
E = 2.0 ** -24
TINY = 1e-30
D = 256
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))      # what the kernels receive: eps is a float argument
C_F32 = (3 * U * U + 769 * E) * (1 + 2 * U)
BF = torch.bfloat16

# fused forward against its emulation: share of all elements, channels of one token, tokens of one channel
CAP_SHARE = 0.01
CAP_TOKEN = 96


def cap_channel(T):
    return max(8, int(0.02 * T))


# ---- the cases (shared by the CPU and the GPU test) -----------------------------------------------------------------------------------
FFN_T_SWEEP = (1, 47, 48, 49, 191, 192, 193, 385)
FFN_F_SWEEP = (32, 64, 96, 128, 160, 224, 2048, 4096)
REGIMES = ("plain", "offset", "tiny", "large")
FFN_CASES = [(T, Fh, "plain") for Fh in (96, 160) for T in FFN_T_SWEEP] + [(193, Fh, "plain") for Fh in FFN_F_SWEEP if Fh not in (96, 160)] + \
            [(193, 256, r) for r in REGIMES]
LIVE_UNITS = (0, 3, 4, 15, 16, 19, 20, 31, 37, 159)
ALN_T = (1, 3, 4, 5, 16383, 16384, 16385, 16389)
LNB_T = (1, 3, 4, 5, 2047, 2048, 2049, 2053)
LIN_CASES = [(T, N) for N in (64, 576) for T in (1, 47, 48, 49, 191, 192, 193)] + [(50, N) for N in (64, 128, 192, 320, 576, 704)] + \
            [(192 * 199 + 5, 192), (192 * 512 + 1, 128)]
LIN_STACKED = [(193, 512), (193, 768)]
F32_CASES = [(T, N) for T in (1, 49, 193) for N in (32, 96, 160)]


def _scale_rows(x, regime):
    if regime == "plain":
        return x
    if regime == "offset":
        return x + 8.0
    if regime == "tiny":
        return 0.01 * x
    if regime == "large":
        return 30.0 * x
    raise ValueError(regime)


def make_ffn(T, Fh, seed=0, regime="plain"):
    """CPU tensors: x (T, 256), w1 (Fh, 256), w2 (256, Fh) bf16; b1, b2, gamma, beta fp32"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + Fh)
    r = lambda *s: torch.randn(*s, generator=g)
    x = _scale_rows(r(T, D), regime).to(BF)
    w1 = (r(Fh, D) * D ** -0.5).to(BF)
    w2 = (r(D, Fh) * Fh ** -0.5).to(BF)
    return {"x": x, "w1": w1, "b1": 0.1 * r(Fh), "w2": w2, "b2": 0.1 * r(D), "gamma": 1 + 0.1 * r(D), "beta": 0.1 * r(D)}


def make_live_unit(T, Fh, j, k, seed=0):
    """one live hidden unit: w1 = 0 except w1[j, k] = 1, b1 = -1000 except b1[j] = 0  ->  y = x + b2 + w2[:, j] relu(x_k)"""
    p = make_ffn(T, Fh, seed)
    p["w1"] = torch.zeros_like(p["w1"])
    p["w1"][j, k] = 1.0
    p["b1"] = torch.full_like(p["b1"], -1000.0)
    p["b1"][j] = 0.0
    return p


def make_aln(T, seed=0, regime="plain"):
    g = torch.Generator().manual_seed(1000 * seed + T)
    r = lambda *s: torch.randn(*s, generator=g)
    a = _scale_rows(r(T, D), regime).to(BF)
    b = _scale_rows(0.5 * r(T, D), "plain" if regime == "offset" else regime).to(BF)
    return {"a": a, "b": b, "gamma": torch.rand(D, generator=g) + 0.5, "beta": r(D)}


def signed_gamma(g):
    """gamma with one zero and some negative entries"""
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    gamma[5] = 0.0
    gamma[[0, 17, 128, 255]] *= -1.0
    gamma[200] = -0.0
    return gamma


def make_lnb(T, seed=0):
    """synthetic inputs of ffn_ln_backward: dy, yhat bf16 (T, 256); rstd fp32 (T) over four decades; gamma fp32"""
    g = torch.Generator().manual_seed(1000 * seed + T)
    dy = torch.randn(T, D, generator=g).to(BF)
    yhat = torch.randn(T, D, generator=g).to(BF)
    rstd = torch.exp(2.3 * (2 * torch.rand(T, generator=g) - 1)) * torch.where(torch.rand(T, generator=g) < 0.1, 30.0, 1.0)
    return {"dy": dy, "yhat": yhat, "rstd": rstd.float(), "gamma": signed_gamma(g)}


def make_lin(T, N, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 3 * T + N)
    x = torch.randn(T, D, generator=g).to(BF)
    w = (torch.randn(N, D, generator=g) / 16).to(BF)
    b = torch.randn(N, generator=g)
    row_mask = torch.rand(T, generator=g) < 0.3
    return {"x": x, "w": w, "b": b, "row_mask": row_mask}


def make_f32(T, N, seed=0, mixed=False):
    g = torch.Generator().manual_seed(1000 * seed + 3 * T + N + (1 if mixed else 0))
    x = torch.randn(T, D, generator=g)
    w = torch.randn(N, D, generator=g) / 16
    if mixed:      # magnitudes 1e4 and 1e-4 inside every row
        x = x * torch.where(torch.rand(T, D, generator=g) < 0.5, 1e4, 1e-4)
        w = w * torch.where(torch.rand(N, D, generator=g) < 0.5, 1e2, 1e-2)
    return {"x": x.float(), "w": w.float(), "b": torch.randn(N, generator=g)}


def exact_f32_probe(T, N, seed=0):
    """operands of lin256_f32 whose result is exact in fp32 in any summation order: x = 1 + s 2^-10, w = (1 + t 2^-10) / 16 with s, t in
    {-1, 0, 1} and never both non-zero at the same (token or channel, k) position class (s lives on even k, t on odd k), so the lo * lo
    product the kernel drops is zero, every product is a multiple of 2^-14 below 2^-3 and every partial sum needs under 24 bits"""
    g = torch.Generator().manual_seed(seed + T + N)
    k = torch.arange(D)
    s = torch.randint(-1, 2, (T, D), generator=g) * (k % 2 == 0)
    t = torch.randint(-1, 2, (N, D), generator=g) * (k % 2 == 1)
    x = (1 + s.double() * 2.0 ** -10).float()
    w = ((1 + t.double() * 2.0 ** -10) / 16).float()
    return {"x": x, "w": w, "b": torch.randint(-4, 5, (N,), generator=g).float()}


MASK_PROBE = (0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), float("nan"), float("inf"), float("-inf"), 1.0)


def mask_probe_row(N):
    """one relu-mask row: +0, -0, the smallest positive and negative bf16 subnormals, NaN, +inf, -inf and 1, repeated over N channels"""
    row = torch.tensor(MASK_PROBE, dtype=torch.float32).to(BF)
    assert row[2].view(torch.int16).item() == 1 and row[3].view(torch.int16).item() == -32767
    return row.repeat((N + 7) // 8)[:N].contiguous()


# ---- float64 references with bounds -------------------------------------------------------------------------------------------------------
def _ln(z, e_in, gamma, beta, eps):
    gamma, beta = gamma.double(), beta.double()
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean = z.mean(-1, keepdim=True)
    d = z - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps) ** -0.5
    yhat = d * rstd
    out = yhat * gamma + beta
    e_m = e_in.mean(-1, keepdim=True) + (D + 1) * E * (z.abs() + e_in).mean(-1, keepdim=True)
    e_d = e_in + e_m + E * d.abs()
    e_var = (2 * d.abs() * e_d + e_d * e_d).mean(-1, keepdim=True) + (D + 3) * E * var
    rho = (e_var / (var + eps)).clamp(max=0.5)
    r_rel = 0.5 * rho / (1 - rho) ** 1.5 + 6 * E
    e_yh = rstd * e_d * (1 + r_rel) + yhat.abs() * r_rel + 2 * E * yhat.abs()
    e_o = gamma.abs() * e_yh + 2 * E * ((yhat * gamma).abs() + out.abs())
    val = {"out": out, "yhat": yhat, "rstd": rstd[..., 0]}
    bound = {"out": e_o + U * (out.abs() + e_o) + TINY, "yhat": e_yh + U * (yhat.abs() + e_yh) + TINY, "rstd": (rstd * r_rel)[..., 0] + TINY}
    return val, bound


def add_layernorm_reference(a, b, gamma, beta, eps=EPS):
    z = a.double() + (b.double() if b is not None else 0.0)
    return _ln(z, E * z.abs(), gamma, beta, eps)


def ffn_reference(x, w1, b1, w2, b2, gamma, beta, eps=EPS):
    x, w1, b1, w2, b2 = (t.double() for t in (x, w1, b1, w2, b2))
    Fh = w1.shape[0]
    p = x @ w1.t() + b1
    h = torch.relu(p)
    e_p = (D + 2) * E * (x.abs() @ w1.abs().t() + b1.abs())
    e_h = torch.where(p < -e_p, torch.zeros_like(p), e_p + U * (h + e_p))
    y = x + b2 + h @ w2.t()
    e_y = e_h @ w2.abs().t() + (Fh + 3) * E * ((h + e_h) @ w2.abs().t() + b2.abs() + x.abs())
    return _ln(y, e_y, gamma, beta, eps)


def ln_backward_reference(dy, yhat, rstd, gamma):
    dy, yhat, rstd, gamma = dy.double(), yhat.double(), rstd.double()[:, None], gamma.double()
    T = dy.shape[0]
    g = dy * gamma
    A = g.mean(-1, keepdim=True)
    Bm = (g * yhat).mean(-1, keepdim=True)
    dz = rstd * (g - A - yhat * Bm)
    e_z = E * rstd * (4 * g.abs() + (D + 4) * g.abs().mean(-1, keepdim=True) + (D + 5) * yhat.abs() * (g * yhat).abs().mean(-1, keepdim=True)
                      + 3 * (A.abs() + yhat.abs() * Bm.abs()))
    val = {"dz": dz, "dgamma": (dy * yhat).sum(0), "dbeta": dy.sum(0), "db2": dz.sum(0)}
    s = (T + 3) * E
    bound = {"dz": e_z + U * (dz.abs() + e_z) + TINY, "dgamma": s * (dy * yhat).abs().sum(0) + TINY, "dbeta": s * dy.abs().sum(0) + TINY,
             "db2": s * (dz.abs() + e_z).sum(0) + e_z.sum(0) + TINY}
    return val, bound


def lin256_base(x, w):
    """the two float64 products every epilogue's reference starts from: (x W^T, |x| |W|^T); never modified by lin256_reference"""
    x, w = x.double(), w.double()
    return x @ w.t(), x.abs() @ w.abs().t()


def lin256_reference(x, w, b=None, epilogue=0, mask=None, base=None):
    """-> (out float64, bound, must_be_zero bool); mask: the (T, N) bf16 relu mask of epilogue 2 or the (T,) bool row mask of epilogue 3;
    base: lin256_base(x, w), where several epilogues share it"""
    lin, mag = base if base is not None else lin256_base(x, w)
    if b is not None and epilogue != 2:
        lin = lin + b.double()
        mag = mag + b.double().abs()
    zero = torch.zeros_like(lin, dtype=torch.bool)
    if epilogue == 1:
        lin = torch.relu(lin)
    elif epilogue == 2:
        zero = ~(mask > 0)
    elif epilogue == 3:
        zero = mask[:, None].expand_as(lin).clone()
    lin = torch.where(zero, torch.zeros_like(lin), lin)
    return lin, U * lin.abs() + (D + 1) * E * mag + TINY, zero


def lin256_f32_reference(x, w, b=None):
    x, w = x.double(), w.double()
    out = x @ w.t()
    mag = x.abs() @ w.abs().t()
    if b is not None:
        out, mag = out + b.double(), mag + b.double().abs()
    return out, C_F32 * mag + TINY


def ratio(got, want, bound, zero=None):
    """worst |got - want| / bound; inf for a NaN, or for a non-zero value where `zero` says the element must be exactly 0"""
    r = (got.double() - want).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if zero is not None:
        r = torch.where(zero & (got.double() != 0), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


# ---- emulations: torch ops with the kernels' rounding points ----------------------------------------------------------------------------
def _r16(t):
    return t.float().to(BF).to(t.dtype)


def _ln_emulate(y, gamma, beta, eps, pc=None):
    s = y if pc is None else y[:, pc]
    mean = s.sum(-1, keepdim=True) * (1.0 / D)
    d = y - mean
    q = d * d
    var = (q if pc is None else q[:, pc]).sum(-1, keepdim=True) * (1.0 / D)
    r = torch.rsqrt(var + eps)
    yh = d * r
    out = yh * gamma.to(y.dtype) + beta.to(y.dtype)
    return {"out": out.float().to(BF), "yhat": yh.float().to(BF), "rstd": r[..., 0].float()}


def emulate_ffn(x, w1, b1, w2, b2, gamma, beta, eps=EPS, dtype=torch.float32, permute=None):
    """the fused forward with the kernel's rounding points in `dtype` arithmetic; `permute` (a torch.Generator): every sum in a shuffled
    order.  -> {"out", "yhat": bf16, "rstd": fp32}"""
    x, w1, b1, w2, b2 = (t.to(dtype) for t in (x, w1, b1, w2, b2))
    Fh = w1.shape[0]
    pk = pf = pc = None
    if permute is not None:
        pk, pf, pc = torch.randperm(D, generator=permute), torch.randperm(Fh, generator=permute), torch.randperm(D, generator=permute)
    p = (x @ w1.t() if pk is None else x[:, pk] @ w1[:, pk].t()) + b1
    h = _r16(torch.relu(p))
    acc = h @ w2.t() if pf is None else h[:, pf] @ w2[:, pf].t()
    y = acc + (b2 + x)
    return _ln_emulate(y, gamma, beta, eps, pc)


def emulate_add_layernorm(a, b, gamma, beta, eps=EPS):
    z = a.float() + b.float() if b is not None else a.float()
    return _ln_emulate(z, gamma, beta, eps)


def emulate_ln_backward(dy, yhat, rstd, gamma):
    dy, yhat, rstd, gamma = dy.float(), yhat.float(), rstd.float()[:, None], gamma.float()
    g = dy * gamma
    A = g.sum(-1, keepdim=True) * (1.0 / D)
    Bm = (g * yhat).sum(-1, keepdim=True) * (1.0 / D)
    z = rstd * (g - A - yhat * Bm)
    return {"dz": z.to(BF), "dgamma": (dy * yhat).sum(0), "dbeta": dy.sum(0), "db2": z.sum(0)}


def emulate_lin256(x, w, b=None, epilogue=0, mask=None):
    y = x.float() @ w.float().t()
    if b is not None and epilogue != 2:
        y = y + b.float()
    if epilogue == 1:
        y = torch.relu(y)
    elif epilogue == 2:
        y = torch.where(mask > 0, y, torch.zeros_like(y))
    elif epilogue == 3:
        y = torch.where(mask[:, None], torch.zeros_like(y), y)
    return y.to(BF)


def emulate_lin256_f32(x, w, b=None):
    xh, wh = x.to(BF).float(), w.to(BF).float()
    xl, wl = (x - xh).to(BF).float(), (w - wh).to(BF).float()
    y = xh @ wl.t() + xl @ wh.t() + xh @ wh.t()
    return y + b if b is not None else y


def mismatch_shares(a, b):
    """bf16 (T, 256) tensors -> (share of elements whose bits differ, most differing channels in one token, most differing tokens in one
    channel); +0 and -0 count as equal"""
    ne = (a.view(torch.int16) != b.view(torch.int16)) & ~((a == 0) & (b == 0))
    return float(ne.float().mean()), int(ne.sum(1).max()), int(ne.sum(0).max())


def within_caps(shares, T):
    return shares[0] <= CAP_SHARE and shares[1] <= CAP_TOKEN and shares[2] <= cap_channel(T)
