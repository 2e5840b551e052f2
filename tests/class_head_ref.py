"""Float64 restatement of the class head (richsem_amd/csrc/cls_head_mfma.hip), forward and backward IN THE COLLAPSED FORM, with an
ELEMENT-WISE error bound for every value the kernels write (logits, n2, dx, dG, dA; dWp for the Python layer), an emulation with the
kernels' rounding points, exact probes and the case lists.  The comparator of tests/test_class_head_ref.py (CPU: the restatement against
the reference fixture, the emulation and three wrong implementations against the bounds) and tests/test_gpu_class_head.py.  Test helper
only: the package never imports it.

Notation and constants as in tests/clip_side_ref.py: u = 2^-8 (bf16), e = 2^-24 (fp32), an fp32 sum of n terms in ANY order errs by at
most n e sum|term|; TINY is added to every bound.  s = scale = exp(logit_scale), g = dL/dlogits.

    n2 = x . (A x),  n = sqrt(n2),  l_c = s (G x)_c / n,  beta = sum_c g_c l_c
    dx = c1 P - c2 (A x),   P = G^T g,  c1 = s / n,  c2 = beta / n2
    [dG; dA] = Y^T x,   Y = [ c1 g | -(c2 / 2) x ];      dWp = T^^T dG + Wp (dA + dA^T)

PRODUCTS.  An MFMA contraction of length K of a and b, each one of `split` (fp32 as bf16 hi + lo: residual u^2), `hi` (rounded to bf16 once:
u) or `exact` (a bf16 value: 0), errs relative to sum_k |a_k| |b_k| by at most
    mm_c = (err_a + err_b + [both split] u^2 + (K * products + 1) e) (1 + 2 u),      products = 1 + [a split] + [b split]
-- the derivation of cls_c (clip_side_ref.py), which is mm_c at K = 256: the dropped lo * lo product, the residuals, the fp32 additions,
and (1 + 2 u) for the cross terms and |ah| |bh| <= (1 + u)^2 |a| |b|.  `oracle`: G, A (and T^) are float64 products rounded once to fp32,
e more per operand: mm_c -> mm_c + e (1 + mm_c).

FORWARD.  clip_side_ref's class-score derivation per class instead of for the maximum: c = cls_c(x, parts); B_n2 = (c + 258 e (1 + c)) Q,
rho = B_n2 / n2, r = rho / 2 / (1 - rho)^3/2 (infinite for rho >= 1: such rows are counted); the epilogue is sqrtf, one division and one
product, 9 e, written 10 e:
    B_l[c] = s n^-1 (c S_c (1 + r + 10 e) + |(G x)_c| (r + 10 e)),   S_c = sum_k |G_ck| |x_k|.

BACKWARD, ROWS.  The kernel reads the SAVED logits and n2: values within B_l, B_n2 of the true ones (zero when a test hands the kernel
its own fp32 inputs and takes them for the truth).
    P_j:     g against G^T over the classes: cP = mm_c(split, split, classes) under parts = 2, mm_c(hi, hi, classes) under parts = 1;
             B_P = cP sum_c |g_c| |G_cj|.
    (A x)_j: the forward's products: B_Ax = c SA_j.
    beta:    classes fmaf in four lane groups and two folds on the saved logits:
             B_beta = sum_c |g_c| B_l[c] + (classes + 3) e sum_c |g_c| (|l_c| + B_l[c]).
    c1:      s / sqrtf(n2): relative r1 = r + 10 e.      c2 = beta / n2:  r2 = rho / (1 - rho) on 1 / n2, one division (5 e with slack):
             B_c2 = ((B_beta (1 + r2) + |beta| r2) (1 + 5 e) + 5 e |beta|) / n2.
    dx_j = c1 P_j - c2 (A x)_j in fp32, three roundings at most (fewer when contracted):
             B_dx = c1 (r1 (|P| + B_P) + B_P) + B_c2 (|Ax| + B_Ax) + |c2| B_Ax + 3 e (c1 (1 + r1) (|P| + B_P) + (|c2| + B_c2) (|Ax| + B_Ax)),
             and u (|dx| + B_dx) more for a bf16 result.

BACKWARD, WEIGHTS.  y = fp32(c1 g): |y - Y| <= dY = (r1 + e (1 + r1)) |Y|; y = fp32(-(beta / (2 n2)) x): dY = (B_c2 / 2 + e (|c2| + B_c2) / 2) |x|.
    Contraction over the R rows, in splits whose partial sums are added in order (n_splits more additions): parts = 2: y split against x
    split (fp32) or exact (bf16); parts = 1: y hi against x hi or exact:  cw = mm_c(...) at K = R, + n_splits e.
             B[m, k] = sum_r dY[r, m] |x[r, k]| (1 + cw) + cw sum_r |Y[r, m]| |x[r, k]|.
    A row with rho >= 1 makes every element's bound infinite.

dWp (Python, two fp32 products of lengths classes and 256, one addition each side):
             B = |T^|^T B_dG + |Wp| (B_dA + B_dA^T) + (classes + 256 + 4) e (|T^|^T |dG| + |Wp| (|dA| + |dA|^T)) (1 + small), small = 1e-3
    (T^ in fp32 carries e, inside the factor).

EXACT PROBE (head_probe): dyadic G in {-1, 0, 1}, A = a a^T with a . x_t = 2^p (p = t mod 3 - 1), sparse dyadic x, one-hot g (a power of
two at class (classes - 1 - t) mod classes: the last class of the last, partial tile is hit by row 0, every row -- the last one too -- has
its own class), s = 16.  Every product is exact and every sum stays under 24 bits (head_probe_expected asserts it term by term), so each
logit, n2, dx, dG and dA is ONE float whatever the order; a bf16 dx is that float rounded once.  Where Y's second block needs more than
8 bits (`y_needs_lo`: the first probe shape does) dA is exact under parts = 2 only.
"""
import numpy as np
import torch

import clip_side_ref as C
from ffn_ref import BF, E, TINY, U

D = 256
SPLIT_ROWS = 512             # kSplitRows (csrc/cls_head_mfma.hip)
PROBE_SCALE = 16.0
MODES = C.CLS_MODES
# the kernels' tiles: forward 48 rows per wave / 192 per workgroup (16-class tiles, stored in pairs: 32); rows backward 16 / 64 rows, 32-class
# k-steps; weights backward 32-row steps, 64-column groups, 512-row splits.  Every tile size +- 1:
ROW_SWEEP = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 191, 192, 193, 385)
CLASS_SWEEP = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1204)
CASES = [(r, 33) for r in ROW_SWEEP] + [(193, c) for c in CLASS_SWEEP if c != 33]
SPLIT_CASES = [(SPLIT_ROWS - 1, 17), (SPLIT_ROWS, 17), (SPLIT_ROWS + 1, 17), (2 * SPLIT_ROWS, 17), (2 * SPLIT_ROWS + 1, 17)]
PROBE_SHAPES = ((193, 41), (49, 64), (385, 33))


def n_splits(rows):
    return (rows + SPLIT_ROWS - 1) // SPLIT_ROWS


def mm_c(a, b, K, oracle=False):
    err = {"split": U * U, "hi": U, "exact": 0.0}
    prods = 1 + (a == "split") + (b == "split")
    c = (err[a] + err[b] + (U * U if a == b == "split" else 0.0) + (K * prods + 1) * E) * (1 + 2 * U)
    return c + E * (1 + c) if oracle else c


for _m in MODES:
    assert abs(mm_c("split" if _m[1] == 2 else "hi", "split" if _m[0] == "f32" else "exact", D) - C.cls_c(*_m)) < 1e-18


def make_head(rows, classes, seed=0, x_dtype="f32"):
    """Gaussian operands of clip_side_ref.make_cls (Wp of spread 1: rho stays far below 1) and a Gaussian g"""
    p = C.make_cls(rows, classes, seed, x_dtype)
    gen = torch.Generator().manual_seed(31 * seed + 7 * rows + classes)
    p["g"] = torch.randn(rows, classes, generator=gen).float().contiguous()
    return p


def _r_of(rho):
    ok = rho < 1
    r = torch.where(ok, 0.5 * rho / (1 - rho.clamp(max=1 - 1e-12)) ** 1.5, torch.full_like(rho, float("inf")))
    r2 = torch.where(ok, rho / (1 - rho.clamp(max=1 - 1e-12)), torch.full_like(rho, float("inf")))
    return r, r2


def reference(G, A, x, g, scale, x_dtype="f32", parts=2, oracle=False, saved=None, drop_norm_term=False):
    """-> dict of float64 values and bounds: logits, n2, dx, dGA (= [dG; dA]) and B_<name>; rho (R,), excluded (rows with rho >= 1).
    G, A: fp32 tensors (float64 ones with `oracle`: the unrounded products).  saved = (logits, n2) fp32 tensors: the backward's truth is
    computed FROM them (a test that hands the kernels its own saved values) and they carry no error; otherwise the backward reads the
    forward kernel's results, within B_logits / B_n2.  drop_norm_term: the wrong dx without -(beta / n2) A x (CPU test)"""
    G, A, x, g = G.double(), A.double(), x.double(), g.double()
    R, classes = g.shape
    c = C.cls_c(x_dtype, parts, oracle)
    k10 = (11 if oracle else 10) * E
    Gx = x @ G.t()
    S = x.abs() @ G.abs().t()
    Ax = x @ A.t()
    SA = x.abs() @ A.abs().t()
    n2 = (x * Ax).sum(1)
    Q = (x.abs() * SA).sum(1)
    B_n2 = (c + 258 * E * (1 + c)) * Q
    rho = torch.where(n2 > 0, B_n2 / n2, torch.full_like(n2, float("inf")))
    r, _ = _r_of(rho)
    isq = n2.clamp(min=0) ** -0.5
    logits = scale * Gx * isq[:, None]
    B_l = abs(scale) * isq[:, None] * (c * S * (1 + r[:, None] + k10) + Gx.abs() * (r[:, None] + k10))
    out = {"logits": logits, "B_logits": B_l + TINY, "n2": n2, "B_n2": B_n2 + TINY, "rho": rho, "excluded": rho >= 1}
    # ---- backward
    if saved is not None:
        logits, n2 = saved[0].double(), saved[1].double()
        B_l, B_n2s = torch.zeros_like(logits), torch.zeros_like(n2)
        isq = n2 ** -0.5
    else:
        B_n2s = B_n2
    rho_b = torch.where(n2 > 0, B_n2s / n2, torch.full_like(n2, float("inf")))
    r, r2 = _r_of(rho_b)
    r1 = r + k10
    beta = (g * logits).sum(1)
    B_beta = (g.abs() * B_l).sum(1) + (classes + 3) * E * (g.abs() * (logits.abs() + B_l)).sum(1)
    c1, c2 = scale * isq, beta / n2
    B_c2 = ((B_beta * (1 + r2) + beta.abs() * r2) * (1 + 5 * E) + 5 * E * beta.abs()) / n2
    kind = "split" if parts == 2 else "hi"
    cP = mm_c(kind, kind, classes, oracle)
    P = g @ G
    B_P = cP * (g.abs() @ G.abs())
    B_Ax = c * SA
    dx = c1[:, None] * P - (0.0 if drop_norm_term else 1.0) * c2[:, None] * Ax
    c1a, c2a, Bc2 = c1.abs()[:, None], c2.abs()[:, None], B_c2[:, None]
    B_dx = (c1a * (r1[:, None] * (P.abs() + B_P) + B_P) + Bc2 * (Ax.abs() + B_Ax) + c2a * B_Ax
            + 3 * E * (c1a * (1 + r1[:, None]) * (P.abs() + B_P) + (c2a + Bc2) * (Ax.abs() + B_Ax)))
    if x_dtype == "bf16":
        B_dx = B_dx + U * (dx.abs() + B_dx)
    out.update({"dx": dx, "B_dx": B_dx + TINY, "beta": beta, "B_beta": B_beta + TINY})
    Y = torch.cat([c1[:, None] * g, -(c2 / 2)[:, None] * x], 1)
    dY = torch.cat([(r1 + E * (1 + r1))[:, None] * Y[:, :classes].abs(), ((B_c2 + E * (c2.abs() + B_c2)) / 2)[:, None] * x.abs()], 1)
    xk = "exact" if x_dtype == "bf16" else kind
    cw = mm_c(kind, xk, R, oracle) + n_splits(R) * E
    dGA = Y.t() @ x
    B_dGA = (dY.t() @ x.abs()) * (1 + cw) + cw * (Y.abs().t() @ x.abs())
    if bool((rho_b >= 1).any()):
        B_dGA = torch.full_like(B_dGA, float("inf"))
    out.update({"dGA": dGA, "B_dGA": B_dGA + TINY})
    return out


def dwp_reference(ref, wp, t_hat, classes, transpose=True):
    """dWp and its bound from a reference()'s dGA: wp (proj, 256), t_hat (classes, proj) float64.  transpose=False: the wrong
    Wp dA instead of Wp (dA + dA^T) (CPU test)"""
    dG, dA = ref["dGA"][:classes], ref["dGA"][classes:]
    BG, BA = ref["B_dGA"][:classes], ref["B_dGA"][classes:]
    sym = dA + dA.t() if transpose else dA
    dwp = t_hat.t() @ dG + wp @ sym
    mag = t_hat.abs().t() @ dG.abs() + wp.abs() @ (dA.abs() + dA.abs().t())
    bound = t_hat.abs().t() @ BG + wp.abs() @ (BA + BA.t()) + (classes + D + 4) * E * mag * (1 + 1e-3) + TINY
    return dwp, bound


def float64_autograd(wp, text, logit_scale, x, g):
    """the reference's formula (richsem.py:182-205) by float64 autograd, NOT collapsed -> logits, dx, dWp"""
    wp = wp.double().clone().requires_grad_(True)
    x = x.double().clone().requires_grad_(True)
    f = x @ wp.t()
    f = f / f.norm(dim=-1, keepdim=True)
    t = text.double()
    t = t / t.norm(dim=-1, keepdim=True)
    logits = float(np.exp(np.float64(logit_scale))) * f @ t.t()
    logits.backward(g.double())
    return logits.detach(), x.grad, wp.grad


def _split(t, parts_kind):
    """-> (hi, lo or None) fp32 tensors of an fp32 / bf16 tensor under `split`, `hi` or `exact`"""
    t = t.float()
    hi = t.to(BF).float()
    return hi, ((t - hi).to(BF).float() if parts_kind == "split" else None)


def _mm(a, ak, b, bk):
    """the kernels' products of a (M, K) against b (N, K) -> (M, N) fp32: lo_a . hi_b + hi_a . lo_b + hi_a . hi_b"""
    ah, al = _split(a, ak)
    bh, bl = _split(b, bk)
    acc = torch.zeros(a.shape[0], b.shape[0])
    if al is not None:
        acc = acc + al @ bh.t()
    if bl is not None:
        acc = acc + ah @ bl.t()
    return acc + ah @ bh.t()


def emulate(G, A, x, g, scale, parts=2, drop_lo=False, saved=None):
    """the three kernels' arithmetic in fp32 torch ops -> dict logits, n2, dx (x's dtype), dGA.  drop_lo: the wrong implementation that
    computes parts = 2 without any lo part (CPU test).  saved: as in reference()"""
    xf32 = x.dtype == torch.float32
    xs = x.float()
    wk = "split" if parts == 2 and not drop_lo else "hi"
    xfwd = ("split" if not drop_lo else "hi") if xf32 else "exact"       # the forward keeps x's lo part under either `parts`
    s32 = torch.tensor(scale, dtype=torch.float32)
    classes = G.shape[0]
    acc = _mm(xs, xfwd, torch.cat([G, A]).float(), wk)
    Ax = acc[:, classes:]
    n2 = (Ax * xs).sum(1)
    logits = acc[:, :classes] * (s32 / torch.sqrt(n2))[:, None]
    out = {"logits": logits, "n2": n2}
    if saved is not None:
        logits, n2 = saved
    beta = (g * logits).sum(1)
    P = _mm(g, wk, G.float().t().contiguous(), wk)
    c1, c2 = s32 / torch.sqrt(n2), beta / n2
    dx = c1[:, None] * P - c2[:, None] * Ax
    out["dx"] = dx.to(x.dtype)
    y = torch.cat([c1[:, None] * g, -(beta / (2 * n2))[:, None] * xs], 1)
    xw = "exact" if not xf32 else wk
    dGA = torch.zeros(classes + D, D)
    for r0 in range(0, x.shape[0], SPLIT_ROWS):      # the splits, added in order
        sl = slice(r0, r0 + SPLIT_ROWS)
        dGA = dGA + _mm(y[sl].t().contiguous(), wk, xs[sl].t().contiguous(), xw)
    out["dGA"] = dGA
    return out


def ratio(got, want, bound):
    """worst |got - want| / bound over the elements with a finite bound; inf for a NaN there"""
    r = (got.double() - want).abs() / bound
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    r = r[torch.isfinite(bound)]
    return float(r.max()) if r.numel() else 0.0


# ---- exact probe ---------------------------------------------------------------------------------------------------------------------------
def head_probe(T, classes, x_dtype="f32"):
    """module docstring -> dict G, A, x, g (torch), scale, p (T,)"""
    assert classes <= 150
    rng = np.random.default_rng(17 * T + classes)
    key, dense = C.LOGIT_CH[:classes], C.LOGIT_CH[classes:]
    G = np.zeros((classes, D))
    x = np.zeros((T, D))
    G[:, dense] = rng.integers(-1, 2, (classes, len(dense)))
    G[:, C.NORM_CH] = rng.integers(-1, 2, (classes, len(C.NORM_CH)))
    G[np.arange(classes), key] = 1.0
    t = np.arange(T)
    x[t, key[t % classes]] = 100.0
    for i in range(3):
        x[t, dense[(7 * t + 11 * i) % len(dense)]] = rng.choice([-1.0, 1.0], T)
    a = np.zeros(D)
    a[C.NORM_CH] = np.tile([1.0, -2.0, 2.0, -1.0], len(C.NORM_CH) // 4)
    p = t % 3 - 1
    j1, j2 = C.NORM_CH[(5 * t + 1) % len(C.NORM_CH)], C.NORM_CH[(5 * t + 3) % len(C.NORM_CH)]
    x[t, j1] = 3.0 * 2.0 ** p / a[j1]
    x[t, j2] = -2.0 * 2.0 ** p / a[j2]
    g = np.zeros((T, classes))
    g[t, (classes - 1 - t) % classes] = 2.0 ** (t % 2)
    xt = torch.from_numpy(x).float()
    return {"G": torch.from_numpy(G).float(), "A": torch.from_numpy(np.outer(a, a)).float(), "x": xt.to(BF) if x_dtype == "bf16" else xt,
            "g": torch.from_numpy(g).float(), "scale": PROBE_SCALE, "p": p}


def _granule(v):
    """the value of the lowest set bit of every float64 in v (inf for 0)"""
    m, ex = np.frexp(np.abs(v))
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = (mi & -mi).astype(np.float64)
    return np.where(v == 0, np.inf, np.ldexp(low, ex - 53))


def _assert_exact_sums(a, b):
    """sum_k a[m, k] b[n, k] in fp32 is exact in any order: every product is an fp32 value and, per (m, n), the sum of the magnitudes is
    below 2^24 times the finest granule among its terms"""
    a, b = a.numpy(), b.numpy()
    for m0 in range(0, a.shape[0], 32):
        terms = a[m0:m0 + 32, None, :] * b[None, :, :]
        gr = _granule(terms).min(-1)
        assert (np.abs(terms).sum(-1) < 2.0 ** 24 * np.where(np.isinf(gr), 1.0, gr)).all(), "a sum that needs more than 24 bits"
        assert np.array_equal(terms.astype(np.float32).astype(np.float64), terms)


def head_probe_expected(p, check_sums=True):
    """-> dict logits, n2, dx, dGA as float32 tensors (dx in x's dtype), from float64; asserts the probe's conditions"""
    G, A, x, g = p["G"].double(), p["A"].double(), p["x"].double(), p["g"].double()
    classes = G.shape[0]
    for t in (p["G"], p["A"], p["x"].float(), p["g"]):
        assert torch.equal(t.to(BF).float(), t), "an operand with a lo part"
    if check_sums:
        _assert_exact_sums(x, torch.cat([G, A]))
    Gx, Ax = x @ G.t(), x @ A.t()
    n2 = (x * Ax).sum(1)
    root = n2.sqrt()
    assert torch.equal(root, 2.0 ** torch.from_numpy(p["p"]).double())
    logits = p["scale"] * Gx / root[:, None]
    beta = (g * logits).sum(1)
    c1, c2 = p["scale"] / root, beta / n2
    dx = c1[:, None] * (g @ G) - c2[:, None] * Ax
    Y = torch.cat([c1[:, None] * g, -(c2 / 2)[:, None] * x], 1)
    hi = Y.float().to(BF).float()
    lo = (Y.float() - hi).to(BF).float()
    assert torch.equal((hi + lo).double(), Y), "Y does not fit hi + lo"
    if check_sums:
        _assert_exact_sums(Y.t().contiguous(), x.t().contiguous())
    dGA = Y.t() @ x
    for name, v in (("logits", logits), ("n2", n2), ("dx", dx), ("dGA", dGA), ("beta", beta), ("c2", c2)):
        assert torch.equal(v.float().double(), v), f"{name} is not a float"
    return {"logits": logits.float(), "n2": n2.float(), "dx": dx.float().to(p["x"].dtype), "dGA": dGA.float(),
            "y_needs_lo": bool((lo != 0).any())}
