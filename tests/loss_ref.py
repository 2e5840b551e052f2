"""Float64 restatement of the loss and matcher kernels with an ELEMENT-WISE error bound for every output, the input recipes, the exact
probes and the wrong variants of tests/test_loss_ref.py (CPU) and tests/test_gpu_loss_bounds.py (the kernels).  Test helper only.

Kernels restated, operation for operation, in the kernels' order:
    focal_neg_{sum,grad}[_masked]   csrc/rows_api.hip, csrc/msda_fed.h      (1 - alpha) p^2 softplus(x), its derivative; __expf
    focal_pos_sum                   csrc/rows_api.hip                       alpha (1 - q)^2 softplus(-x) - (1 - alpha) q^2 softplus(x); expf
    box_pair_loss                   csrc/rows_api.hip                       c_l1 L1 + c_giou (1 - GIoU), four tangents (Dual4)
    matcher_cost<T, TM>             csrc/msda_matcher.h                     class / bbox / GIoU cost, f32 and f64, both layouts
    criterion_pairs (+ backward)    csrc/msda_criterion.h                   slot logic, weights, records, per-call terms, four gradients

Three ways to evaluate the same text (``Mode``): F64 -- plain float64 with double constants and unrounded weights, the mathematical
reference the fixtures are pinned to; F32 -- float32 tensors, what a correct float32 implementation gives; B32 / B64 -- float64 values
that carry a bound (class ``B``), with the constants and weights the float32 (float64) kernel really uses.

The bounds.  u = 2^-24 (f32) or 2^-53 (f64).  They are COUNTED, not guessed: ``B`` is a running error analysis that follows the
restatement operation by operation, so every rounding of the kernel appears once, acting on the magnitude it acts on:
    a + b, a - b   e = e_a + e_b + u |a + b|             a cancellation keeps the operands' absolute errors: 1 - p, 1 - q and
                                                         1 - p + 1e-8 carry  p d_p  whatever is left of the difference
    a b            e = |a| e_b + |b| e_a + e_a e_b + u |a b|       (times a power of two: exact)
    a / b          e = (e_a + |a / b| e_b) / (|b| - e_b) + u |a / b|
    exp a          e = exp(a) (expm1(e_a) + E),  E = 4 u for expf (libm: 2 ulp allowed), E = (2 + 2 |a|) u for __expf: exp2(a log2e) --
                   the constant log2e and the product each round in the exponent, u |a log2e| ln 2 = u |a| each, and v_exp_f32 is
                   good to an ulp (2 u).  No allowance beyond this count was needed on the GPU (profiles/r25_loss_bounds.md).
    log a          e = e_a / (|a| - e_a) + 4 u |log a|   so half an ulp of p passes through log(1 - p + 1e-8) as u p / (1 - p + 1e-8):
                   the matcher's bound GROWS towards saturated logits, nothing is excluded.  Where e_a reaches a the first-order form
                   is replaced by the interval [max(a - e_a, 1e-8), a + e_a] carried through log as it stands -- p <= 1 in any
                   precision, so the kernel's argument is never below 1e-8 and the bound stays finite (1.6 at logit 16.6, where the
                   float32 cost really is 0.44 from the float64 one).
    log1p a        e = e_a / (1 + a - e_a) + 4 u |log1p a|
    max, min, relu, |.|   the value keeps the larger operand error.  Where the operands are closer than their errors the float32 code may
                   take the other branch: the tangents then get |d_a - d_b| added (and the value e_a + e_b).
    every result   + eta (2^-126 / 2^-1022): a result below the smallest normal may be flushed.
    exactness      (f32 only) an operation on error-free operands whose exact result is a float32 is exact: e = 0.  Boxes on a dyadic grid
                   therefore have error-free corners, every comparison resolves alike in both precisions, ties are ties, and
                   hull - uni = 0 of a nested or identical pair is an exact 0 that nothing divides by.
    sums           a float32 accumulation of depth n over terms t_k with bounds e_k:  sum e_k + n u sum |t_k|  (any order); the float64
                   partials add nothing visible; a final conversion to float32 adds u |sum|.
The same through 2 (1 - p) softplus(x): the half ulp of p arrives as 2 u softplus(x).  f64 instances use u = 2^-53 and are held to 2
bounds, since the CPU's and the GPU's libm may differ by an ulp.  A bound of 0 asks for the exact value.
"""
import functools
import math
import os

import numpy as np
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
ETA32, ETA64 = 2.0 ** -126, 2.0 ** -1022
LIBM = 4.0      # libm calls (expf, logf, log1pf and their f64 forms): 2 ulp = 4 u allowed
ALPHA = 0.25

# wrong restatements (name, kernel it sits in, what is wrong).  tests/test_loss_ref.py evaluates each in float64 through the restatement:
# it must leave its bound; OLD_CRITERION_PASSES records whether the kernel's older whole-tensor criterion lets it pass (asserted there).
# (e) and (f) were first proposed on the other side (x > 8, p < 2^-10), where the part they drop is below 1e-9 of the element -- under half
# an ulp of a float32 result, so the variant IS the right kernel to float32.  They are kept under *_as_first_proposed, where the test
# shows that they stay far inside the bounds, and the list holds both where the dropped part is the element.
MUTANTS = (
    ("neg_grad_scaled", "focal_neg", "(a) all-negative gradient times 1 + 2^-6 where x < -4"),
    ("neg_grad_term_dropped", "focal_neg", "(b) 2 (1 - p) softplus(x) dropped from the gradient where x < -8"),
    ("dn_weight_scaled", "criterion", "(c) denoising weight of the box-gradient records times 1 + 2^-12"),
    ("hull_quotient_scaled", "pair", "(d) (hull - uni) / (hull + 1e-6) times 1 + 2^-10 for disjoint pairs"),
    ("pos_part_dropped", "focal_pos", "(e) alpha (1 - q)^2 softplus(-x) dropped where x < -8 (where it is the element)"),
    ("matcher_neg_dropped", "matcher", "(f) the matcher's neg term dropped where 1 - p < 2^-10 (where it is the element)"),
    ("tie_to_first", "pair", "(g) a tie of max / min passed whole to the first operand"),
    ("relu_blocks_zero", "pair", "(h) clamp(min = 0) blocking the gradient at exactly 0"),
    ("two_stage_dn_weight", "criterion", "(i) the two-stage call weighted with the denoising weight"),
)
SUB_ULP_AS_FIRST_PROPOSED = (
    ("pos_part_dropped_as_first_proposed", "focal_pos", "(e) as first proposed: the same part dropped where x > 8 (below 4e-11 of the element)"),
    ("matcher_neg_dropped_as_first_proposed", "matcher", "(f) as first proposed: neg dropped where p < 2^-10 (below 5e-10 of the element)"),
)


OLD_CRITERION_PASSES = {
    "neg_grad_scaled": True, "neg_grad_term_dropped": True, "dn_weight_scaled": True,
    "hull_quotient_scaled": False,      # its loss passes (1.1e-5 of 2e-5); its gradient is 3.1e-4 of the largest against 2e-4
    "pos_part_dropped": False, "matcher_neg_dropped": False,
    "tie_to_first": True, "relu_blocks_zero": True,      # (the older test's boxes: its only ties are identical boxes, nothing touches)
    "two_stage_dn_weight": False,
    "pos_part_dropped_as_first_proposed": True, "matcher_neg_dropped_as_first_proposed": True,
}


class Mode:
    def __init__(self, name, u, eta, dtype, f32_consts, bounded, threshold=True):
        self.name, self.u, self.eta, self.dtype, self.f32_consts, self.bounded = name, u, eta, dtype, f32_consts, bounded
        self.threshold = threshold      # softplus(x) = x beyond 20 as the kernels (and torch) have it; F64 takes log1p(exp(x)) throughout

    def c(self, x):
        """a source constant as the kernel holds it"""
        return float(np.float32(x)) if self.f32_consts else float(x)

    def lift(self, t):
        t = torch.as_tensor(t)
        if self.bounded:
            return B(t.to(torch.float64), None, self)
        return t.to(self.dtype)


# ---- values that carry a bound ---------------------------------------------------------------------------------------------------------------
def _pow2(c):
    return c != 0 and math.frexp(abs(c))[0] == 0.5


class B:
    """float64 value ``v`` with an absolute error bound ``e`` for the kernel's result (the rules: the module docstring)"""
    __slots__ = ("v", "e", "m")

    def __init__(self, v, e, m):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e
        self.m = m

    def _rnd(self, v, ein):
        m = self.m
        r = m.u * v.abs() + m.eta
        if m.u == U32:
            rep = (v.float().double() == v) & ((v.abs() >= ETA32) | (v == 0))
            r = torch.where((ein == 0) & rep, torch.zeros_like(r), r)
        return r

    def _o(self, o):
        return o if isinstance(o, B) else B(torch.as_tensor(o, dtype=torch.float64), None, self.m)

    def __neg__(self):
        return B(-self.v, self.e, self.m)

    def __add__(self, o):
        o = self._o(o)
        v = self.v + o.v
        ein = self.e + o.e
        return B(v, ein + self._rnd(v, ein), self.m)

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-self._o(o))

    def __rsub__(self, o):
        return self._o(o) - self

    def __mul__(self, o):
        if isinstance(o, (int, float)):
            if o == 0:
                return B(torch.zeros_like(self.v), None, self.m)
            if _pow2(o):
                return B(self.v * o, self.e * abs(o), self.m)
        o = self._o(o)
        v = self.v * o.v
        ein = self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e
        return B(v, ein + self._rnd(v, ein), self.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._o(o)
        v = self.v / o.v
        ein = (self.e + v.abs() * o.e) / (o.v.abs() - o.e).clamp(min=1e-300)
        ein = torch.where((self.e == 0) & (o.e == 0), torch.zeros_like(ein), ein)
        return B(v, ein + self._rnd(v, ein), self.m)

    def __rtruediv__(self, o):
        return self._o(o) / self

    def __getitem__(self, i):
        return B(self.v[i], self.e[i], self.m)

    @property
    def shape(self):
        return self.v.shape


def _v(x):
    return x.v if isinstance(x, B) else x


def _exp(x, fast=False):
    if isinstance(x, B):
        v = torch.exp(x.v)
        E = (2.0 + 2.0 * x.v.abs()) * x.m.u if fast else LIBM * x.m.u
        e = v * (torch.expm1(x.e) + E) + x.m.eta
        return B(v, torch.where(torch.isfinite(e), e, torch.full_like(e, float("inf"))), x.m)
    return torch.exp(x)


def _log(x, floor=None):
    """``floor``: a number the KERNEL's argument cannot fall below (1 - p + 1e-8 >= 1e-8 since p <= 1 in any precision): the interval
    [max(a - e_a, floor), a + e_a] is carried through log as it stands, so the bound stays finite where e_a exceeds a"""
    if isinstance(x, B):
        v = torch.log(x.v)
        if floor is None:
            e = x.e / (x.v.abs() - x.e).clamp(min=1e-300)
        else:
            lo = torch.maximum(x.v - x.e, torch.full_like(x.v, floor))
            e = torch.maximum(torch.log(x.v + x.e) - v, v - torch.log(lo))
        return B(v, e + LIBM * x.m.u * (v.abs() + e) + x.m.eta, x.m)
    return torch.log(x)


def _log1p(x):
    if isinstance(x, B):
        v = torch.log1p(x.v)
        return B(v, x.e / (1.0 + x.v - x.e).clamp(min=1e-300) + LIBM * x.m.u * v.abs() + x.m.eta, x.m)
    return torch.log1p(x)


def _like(x, like):
    if isinstance(like, B):
        return like._o(x)
    return x if torch.is_tensor(x) else torch.as_tensor(x, dtype=like.dtype)


def _where(c, a, b):
    like = a if (isinstance(a, B) or torch.is_tensor(a)) else b
    a, b = _like(a, like), _like(b, like)
    if isinstance(like, B):
        return B(torch.where(c, a.v, b.v), torch.where(c, a.e, b.e), like.m)
    return torch.where(c, a, b)


def _close(a, b):
    """where a float32 comparison of a and b may resolve the other way (never for error-free operands)"""
    if isinstance(a, B) and isinstance(b, B):
        s = a.e + b.e
        return ((a.v - b.v).abs() <= s) & (s > 0)
    return None


def _bump(x, amb, extra):
    """x with ``extra`` added to its bound where ``amb``"""
    return B(x.v, x.e + torch.where(amb, extra, torch.zeros_like(extra)), x.m)


def _max(a, b):
    r = _where(_v(a) > _v(b), a, b)
    if isinstance(r, B):
        a, b = r._o(a), r._o(b)
        r = _bump(r, _close(a, b), a.e + b.e)
    return r


def _min(a, b):
    r = _where(_v(a) < _v(b), a, b)
    if isinstance(r, B):
        a, b = r._o(a), r._o(b)
        r = _bump(r, _close(a, b), a.e + b.e)
    return r


def _abs(a):
    return B(a.v.abs(), a.e, a.m) if isinstance(a, B) else a.abs()


def _sum_f32(x, dim, depth, mode):
    """a float32 accumulation over ``dim`` in an unspecified order, ``depth`` additions deep"""
    if isinstance(x, B):
        return B(x.v.sum(dim), x.e.sum(dim) + depth * mode.u * x.v.abs().sum(dim), mode)
    return x.sum(dim)


def _sum_f64(x, dim=None):
    """the float64 partials: nothing visible is added"""
    if isinstance(x, B):
        return B(x.v.sum(dim) if dim is not None else x.v.sum(), x.e.sum(dim) if dim is not None else x.e.sum(), x.m)
    return x.double().sum(dim) if dim is not None else x.double().sum()


def _to_f32(x, mode):
    """the final conversion of a float64 sum to float32"""
    if isinstance(x, B):
        return B(x.v, x.e + x.m.u * x.v.abs(), x.m) if x.m.u == U32 else x
    return x.float() if mode.name == "f32" else x


F64 = Mode("f64", 0.0, 0.0, torch.float64, False, False, threshold=False)
F32 = Mode("f32", U32, ETA32, torch.float32, True, False)
B32 = Mode("b32", U32, ETA32, torch.float64, True, True)
B64 = Mode("b64", U64, ETA64, torch.float64, False, True)
F64K = Mode("f64k", 0.0, 0.0, torch.float64, True, False)      # float64 arithmetic on the float32 kernel's constants and weights (mutants)


def ratio(got, ref):
    """worst |got - ref.v| / ref.e over the elements; a bound of 0 asks for the exact value (inf otherwise); NaN must meet NaN"""
    got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
    v, e = ref.v.reshape(-1), ref.e.expand_as(ref.v).reshape(-1)
    assert got.shape == v.shape, (got.shape, v.shape)
    nan = torch.isnan(v)
    if bool((torch.isnan(got) != nan).any()):
        return float("inf")
    err = (got - v).abs()[~nan]
    e = e[~nan]
    r = torch.where(err == 0, torch.zeros_like(err), err / e.clamp(min=1e-320))
    r = torch.where((e == 0) & (err > 0), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def tightness(ref):
    """median bound / |ref| over the non-zero elements: the bounds are not vacuous"""
    v, e = ref.v.reshape(-1), ref.e.expand_as(ref.v).reshape(-1)
    k = torch.isfinite(v) & (v != 0)
    return float((e[k] / v[k].abs()).median()) if bool(k.any()) else 0.0


def _softplus(x, mode, fast=False):
    """x > 20 ? x : log1p(exp(x)) (torch's threshold); without the threshold (F64): max(x, 0) + log1p(exp(-|x|)), the same number"""
    if mode.threshold:
        return _where(_v(x) > 20.0, x, _log1p(_exp(x, fast)))
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


# ---- the all-negative focal term ---------------------------------------------------------------------------------------------------------------
def focal_neg_term(x, mode, mutant=None):
    """rows_api.hip focal_neg: -> (p^2 softplus(x), its derivative)"""
    xv = _v(x)
    fast = mode is not B64
    p = 1.0 / (1.0 + _exp(-x, fast))
    sp = _softplus(x, mode, fast)
    pp = p * p
    inner = 2.0 * (1.0 - p) * sp
    if mutant == "neg_grad_term_dropped":
        inner = _where(xv < -8.0, 0.0, inner)
    d = pp * (inner + p)
    if mutant == "neg_grad_scaled":
        d = _where(xv < -4.0, d * (1.0 + 2.0 ** -6), d)
    return pp * sp, d


def _live(w, group, mask, groups, C):
    """which (row, class) entries count: row weight != 0, the row's group inside [0, groups), the class in the group's mask"""
    live = (w != 0)[:, None].expand(-1, C)
    if mask is not None:
        ok = (group >= 0) & (group < groups)
        live = live & ok[:, None] & (mask[group.clamp(0, groups - 1).long()] != 0)
    return live


def focal_neg(x, w, alpha, gscale, mode, group=None, mask=None, mutant=None):
    """focal_neg_sum_kernel + the wrappers' sum of the partials, focal_neg_grad_kernel (and the masked forms of msda_fed.h).  x (rows, C)
    float32-exact logits, w (rows) float32 weights, gscale the backward's factor, group (rows) int / mask (G, C) or None.
    -> (loss, grad (rows, C), loss before its conversion to float32)"""
    x, w = torch.as_tensor(x), torch.as_tensor(w)
    rows, C = x.shape
    live = _live(w, None if mask is None else torch.as_tensor(group), None if mask is None else torch.as_tensor(mask),
                 0 if mask is None else mask.shape[0], C)
    X, W = mode.lift(x), mode.lift(w)
    f, d = focal_neg_term(X, mode, mutant)
    f, d = _where(live, f, 0.0), _where(live, d, 0.0)
    # thread t of the row's workgroup adds classes t, t + 256, ... in order; s * w[row] in float32; float64 from there on
    n = (C + 255) // 256
    s = None
    for i in range(n):
        part = f[:, i * 256: (i + 1) * 256]
        if part.shape[1] < 256 and i > 0:
            pad = 256 - part.shape[1]
            z = torch.zeros((rows, pad), dtype=torch.float64 if mode.bounded else mode.dtype)
            part = B(torch.cat((part.v, z), 1), torch.cat((part.e, z), 1), mode) if mode.bounded else torch.cat((part, z), 1)
        s = part if s is None else s + part
    t = s * W[:, None]
    raw = _sum_f64(t) * (1.0 - alpha)
    g = gscale * (1.0 - alpha) if mode is F64 else _like(mode.c(gscale), W) * (1.0 - alpha)      # gscale[0] * one_m_alpha, both float32
    wr = W * g
    return _to_f32(raw, mode), d * wr[:, None], raw


# ---- the positive entries ----------------------------------------------------------------------------------------------------------------------
def focal_pos_term(v, alpha, mode, mutant=None):
    """focal_pos_sum_kernel / crit::focal_pos_term: -> (l, dl)"""
    vv = _v(v)
    q = 1.0 / (1.0 + _exp(-v))
    sp_pos, sp_neg = _softplus(v, mode), _softplus(-v, mode)
    omq = 1.0 - q
    oma = 1.0 - alpha
    a_part = alpha * omq * omq * sp_neg
    da_part = -2.0 * omq * q * omq * sp_neg
    if mutant in ("pos_part_dropped", "pos_part_dropped_as_first_proposed"):
        drop = vv < -8.0 if mutant == "pos_part_dropped" else vv > 8.0
        a_part, da_part = _where(drop, 0.0, a_part), _where(drop, 0.0, da_part)
    l = a_part - oma * q * q * sp_pos
    dl = alpha * (da_part - omq * omq * omq) - oma * (2.0 * q * q * omq * sp_pos + q * q * q)
    return l, dl


def _block_sum(t, mode, threads=1024):
    """acc += term over k = thread, thread + threads, ... in order, then block_sum_1024: 6 + 6 shuffle steps (pair kernels)"""
    K = t.shape[0]
    n = (K + threads - 1) // threads
    s = None
    for i in range(n):
        part = t[i * threads: (i + 1) * threads]
        if part.shape[0] < threads and i > 0:
            z = torch.zeros(threads - part.shape[0], dtype=torch.float64 if mode.bounded else mode.dtype)
            part = B(torch.cat((part.v, z)), torch.cat((part.e, z)), mode) if mode.bounded else torch.cat((part, z))
        s = part if s is None else s + part
    return _sum_f32(s, 0, 12, mode)


def focal_pos(x, w, alpha, mode, mutant=None):
    """msda_focal_pos_sum_f32: -> (loss, grad (K))"""
    X, W = mode.lift(x), mode.lift(w)
    l, dl = focal_pos_term(X, alpha, mode, mutant)
    return _block_sum(l * W, mode), dl * W


# ---- the box pair loss -------------------------------------------------------------------------------------------------------------------------
class D4:
    """value + four tangents (rows_api.hip Dual4)"""

    def __init__(self, v, d):
        self.v, self.d = v, d

    def __add__(self, o):
        return D4(self.v + o.v, [a + b for a, b in zip(self.d, o.d)])

    def __sub__(self, o):
        return D4(self.v - o.v, [a - b for a, b in zip(self.d, o.d)])

    def __mul__(self, o):
        return D4(self.v * o.v, [a * o.v + self.v * b for a, b in zip(self.d, o.d)])

    def __truediv__(self, o):
        q, ib = self.v / o.v, 1.0 / o.v
        return D4(q, [(a - q * b) * ib for a, b in zip(self.d, o.d)])

    def scale(self, s):
        return D4(self.v * s, [a * s for a in self.d])


def _d4_const(v):
    z = _where(torch.zeros(_v(v).shape, dtype=torch.bool), v, 0.0)      # an exact 0 of v's kind
    return D4(v, [z, z, z, z])


def _d4_var(v, i):
    r = _d4_const(v)
    r.d[i] = _like_full(v, 1.0)
    return r


def _d4_pick(first, second, a, b, mutant_tie=False):
    """first -> a, second -> b, neither -> (a + b) / 2; tangents get |d_a - d_b| where the comparison may resolve otherwise in float32"""
    mid = a if mutant_tie else (a + b).scale(0.5)
    amb = _close(a.v, b.v) if isinstance(a.v, B) else None

    def pick(x, y, m, tangent):
        r = _where(first, x, _where(second, y, m))
        if amb is not None:
            r = _bump(r, amb, (x.v - y.v).abs() if tangent else x.e + y.e)
        return r
    return D4(pick(a.v, b.v, mid.v, False), [pick(x, y, m, True) for x, y, m in zip(a.d, b.d, mid.d)])


def _d4_max(a, b, mutant=None):
    return _d4_pick(_v(a.v) > _v(b.v), _v(b.v) > _v(a.v), a, b, mutant == "tie_to_first")


def _d4_min(a, b, mutant=None):
    return _d4_pick(_v(a.v) < _v(b.v), _v(b.v) < _v(a.v), a, b, mutant == "tie_to_first")


def _d4_relu(a, mutant=None):
    keep = _v(a.v) > 0.0 if mutant == "relu_blocks_zero" else _v(a.v) >= 0.0
    z = _d4_const(a.v)
    r = D4(_where(keep, a.v, 0.0), [_where(keep, x, zz) for x, zz in zip(a.d, z.d)])
    if isinstance(a.v, B):
        amb = (a.v.v.abs() <= a.v.e) & (a.v.e > 0)
        r = D4(_bump(r.v, amb, a.v.e), [_bump(x, amb, y.v.abs()) for x, y in zip(r.d, a.d)])
    return r


def _d4_abs(a):
    pos, neg = _v(a.v) > 0.0, _v(a.v) < 0.0
    m = a.scale(-1.0)
    z = _d4_const(a.v)
    r = D4(_where(pos, a.v, _where(neg, m.v, 0.0)), [_where(pos, x, _where(neg, y, zz)) for x, y, zz in zip(a.d, m.d, z.d)])
    if isinstance(a.v, B):
        amb = (a.v.v.abs() <= a.v.e) & (a.v.e > 0)
        r = D4(r.v, [_bump(x, amb, 2.0 * y.v.abs()) for x, y in zip(r.d, a.d)])
    return r


def box_pair_terms(p, t, mode, mutant=None):
    """box_pair_loss_kernel's body / crit::box_pair_terms: p, t (K, 4) cxcywh -> (l1, giou) as D4 w.r.t. p"""
    P, T = mode.lift(p), mode.lift(t)
    cx, cy, pw, ph = (_d4_var(P[:, i], i) for i in range(4))
    tc = [_d4_const(T[:, i]) for i in range(4)]
    l1 = _d4_abs(cx - tc[0]) + _d4_abs(cy - tc[1]) + _d4_abs(pw - tc[2]) + _d4_abs(ph - tc[3])
    half = _d4_const(_like_full(P[:, 0], 0.5))
    ax0, ay0, ax1, ay1 = cx - half * pw, cy - half * ph, cx + half * pw, cy + half * ph
    bx0, by0 = _d4_const(T[:, 0] - 0.5 * T[:, 2]), _d4_const(T[:, 1] - 0.5 * T[:, 3])
    bx1, by1 = _d4_const(T[:, 0] + 0.5 * T[:, 2]), _d4_const(T[:, 1] + 0.5 * T[:, 3])
    area_a, area_b = (ax1 - ax0) * (ay1 - ay0), (bx1 - bx0) * (by1 - by0)
    iw = _d4_relu(_d4_min(ax1, bx1, mutant) - _d4_max(ax0, bx0, mutant), mutant)
    ih = _d4_relu(_d4_min(ay1, by1, mutant) - _d4_max(ay0, by0, mutant), mutant)
    inter = iw * ih
    uni = area_a + area_b - inter
    eps = _d4_const(_like_full(P[:, 0], mode.c(1e-6)))
    iou = inter / (uni + eps)
    hw = _d4_relu(_d4_max(ax1, bx1, mutant) - _d4_min(ax0, bx0, mutant), mutant)
    hh = _d4_relu(_d4_max(ay1, by1, mutant) - _d4_min(ay0, by0, mutant), mutant)
    hull = hw * hh
    quot = (hull - uni) / (hull + eps)
    if mutant == "hull_quotient_scaled":
        dis = (_v(inter.v) == 0) & (_v(hull.v) > _v(uni.v))
        s = D4(quot.v * (1.0 + 2.0 ** -10), [x * (1.0 + 2.0 ** -10) for x in quot.d])
        quot = D4(_where(dis, s.v, quot.v), [_where(dis, x, y) for x, y in zip(s.d, quot.d)])
    return l1, iou - quot


def _like_full(like, c):
    if isinstance(like, B):
        return B(torch.full_like(like.v, c), None, like.m)
    return torch.full_like(like, c)


def _scale_c(x, c, mode):
    """x * c for a kernel argument c (a float32 number)"""
    if isinstance(x, B):
        return x * c if (c == 0 or _pow2(c)) else x * x._o(c)
    return x * c


def box_pair_loss_of(l1, giou, c_l1, c_giou, mode):
    one = _d4_const(_like_full(giou.v, 1.0))
    a, b = l1, one - giou
    return D4(_scale_c(a.v, c_l1, mode), [_scale_c(x, c_l1, mode) for x in a.d]) + \
        D4(_scale_c(b.v, c_giou, mode), [_scale_c(x, c_giou, mode) for x in b.d])


def box_pair(p, t, w, c_l1, c_giou, mode, mutant=None):
    """msda_box_pair_loss_f32: -> (loss, grad (K, 4))"""
    l1, giou = box_pair_terms(p, t, mode, mutant)
    l = box_pair_loss_of(l1, giou, c_l1, c_giou, mode)
    W = mode.lift(w)
    g = [x * W for x in l.d]
    grad = B(torch.stack([x.v for x in g], 1), torch.stack([x.e for x in g], 1), mode) if mode.bounded else torch.stack(g, 1)
    return _block_sum(l.v * W, mode), grad


def box_pair_autograd(p, t, w, c_l1, c_giou):
    """torch's CPU float64 autograd of the reference's box_ops formulas on the diagonal (box_cxcywh_to_xyxy, box_iou,
    generalized_box_iou written with torch.max / torch.min / clamp(min=0) / abs as there): -> (loss, grad (K, 4))"""
    p = torch.as_tensor(p, dtype=torch.float64).clone().requires_grad_(True)
    t, w = torch.as_tensor(t, dtype=torch.float64), torch.as_tensor(w, dtype=torch.float64)

    def xyxy(b):
        cx, cy, bw, bh = b.unbind(-1)
        return torch.stack([cx - 0.5 * bw, cy - 0.5 * bh, cx + 0.5 * bw, cy + 0.5 * bh], -1)
    a, b = xyxy(p), xyxy(t)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area_a + area_b - inter
    iou = inter / (union + 1e-6)
    wh = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    area = wh[:, 0] * wh[:, 1]
    giou = iou - (area - union) / (area + 1e-6)
    loss = ((c_l1 * (p - t).abs().sum(-1) + c_giou * (1 - giou)) * w).sum()
    loss.backward()
    return loss.detach(), p.grad


# ---- the matcher's cost ------------------------------------------------------------------------------------------------------------------------
def matcher_class_cost(x, alpha, mode, mutant=None):
    """pos - neg of matcher_cost_kernel (before w_class)"""
    p = 1.0 / (1.0 + _exp(-x))
    neg = (1.0 - alpha) * (p * p) * (-_log(1.0 - p + mode.c(1e-8), mode.c(1e-8)))
    pos = alpha * ((1.0 - p) * (1.0 - p)) * (-_log(p + mode.c(1e-8), mode.c(1e-8)))
    if mutant == "matcher_neg_dropped":
        neg = _where(1.0 - _v(p) < 2.0 ** -10, 0.0, neg)
    if mutant == "matcher_neg_dropped_as_first_proposed":
        neg = _where(_v(p) < 2.0 ** -10, 0.0, neg)
    return pos - neg


def matcher_blocks(logits, boxes, tgt_ids, tgt_boxes, offsets, w_class, w_bbox, w_giou, alpha, mode, mutant=None):
    """matcher_cost_kernel: logits (Bn, Q, C), boxes (Bn, Q, 4), tgt_ids (T), tgt_boxes (T, 4), offsets (Bn + 1) -> a list over the images
    of (Q, T_b) blocks (row-major; the target-major layout stores the same entries transposed).  A label outside [0, C): NaN column."""
    logits, boxes, tgt_boxes = torch.as_tensor(logits), torch.as_tensor(boxes), torch.as_tensor(tgt_boxes)
    ids = np.asarray(tgt_ids, dtype=np.int64)
    Bn, Q, C = logits.shape
    out = []
    for b in range(Bn):
        t0, t1 = int(offsets[b]), int(offsets[b + 1])
        lab = ids[t0:t1]
        bad = (lab < 0) | (lab >= C)
        cc = matcher_class_cost(mode.lift(logits[b][:, torch.as_tensor(np.where(bad, 0, lab))]), alpha, mode, mutant)      # (Q, Tb)
        cc = _where(torch.as_tensor(bad)[None, :].expand(Q, -1), float("nan"), cc)
        o = [mode.lift(boxes[b][:, i])[:, None] for i in range(4)]
        t = [mode.lift(tgt_boxes[t0:t1, i])[None, :] for i in range(4)]
        cb = _abs(o[0] - t[0]) + _abs(o[1] - t[1]) + _abs(o[2] - t[2]) + _abs(o[3] - t[3])
        ox0, oy0, ox1, oy1 = o[0] - 0.5 * o[2], o[1] - 0.5 * o[3], o[0] + 0.5 * o[2], o[1] + 0.5 * o[3]
        tx0, ty0, tx1, ty1 = t[0] - 0.5 * t[2], t[1] - 0.5 * t[3], t[0] + 0.5 * t[2], t[1] + 0.5 * t[3]
        area_o, area_t = (ox1 - ox0) * (oy1 - oy0), (tx1 - tx0) * (ty1 - ty0)
        iw, ih = _max(_min(ox1, tx1) - _max(ox0, tx0), 0.0), _max(_min(oy1, ty1) - _max(oy0, ty0), 0.0)
        inter = iw * ih
        uni = area_o + area_t - inter
        iou = inter / (uni + mode.c(1e-6))
        hw, hh = _max(_max(ox1, tx1) - _min(ox0, tx0), 0.0), _max(_max(oy1, ty1) - _min(oy0, ty0), 0.0)
        hull = hw * hh
        giou = iou - (hull - uni) / (hull + mode.c(1e-6))
        out.append(_scale_c(cb, w_bbox, mode) + _scale_c(cc, w_class, mode) + _scale_c(-giou, w_giou, mode))
    return out


def flat_blocks(blocks, target_major=False):
    """the kernel's flat layout of the blocks' values (and bounds)"""
    parts = [(b.v, b.e.expand_as(b.v)) if isinstance(b, B) else (b, b) for b in blocks]
    f = lambda x: (x.t() if target_major else x).reshape(-1)
    v, e = torch.cat([f(a) for a, _ in parts]), torch.cat([f(c) for _, c in parts])
    return B(v, e, blocks[0].m) if isinstance(blocks[0], B) else v


# ---- the criterion over capacity buffers: slot logic, records, terms, gradients -----------------------------------------------------------
def criterion(logits, coords, il, ib, cum, tgt_ids, tgt_boxes, qot, meta, num_boxes, pad_cap, mode, alpha=ALPHA, c_cls=1.0, c_l1=5.0,
              c_giou=2.0, flags=0, class_mask=None, gscale=1.0, mutant=None):
    """criterion_pairs_kernel + criterion_reduce_kernel + the all-negative launches + criterion_pairs_backward_kernel as
    richsem_amd/criterion.py strings them together.  Arrays as the kernel takes them (cum (N + 1), tgt_ids (cap), tgt_boxes (cap, 4), qot
    (nl + 1, cap), meta None or int[5], num_boxes None or a float).  -> dict: slots (row, label, weight per slot, matched slots first),
    rec_gx / rec_gb, terms (2 nl + 1, 3), status [4], row_weight / row_weight_int (float32 numpy, exact), row_group / row_group_int,
    loss, grads (logits, coords, il, ib), neg_per_call (2 nl + 1)."""
    logits, coords, il, ib = (torch.as_tensor(a) for a in (logits, coords, il, ib))
    cum, ids, qot = np.asarray(cum, dtype=np.int64), np.asarray(tgt_ids, dtype=np.int64), np.asarray(qot, dtype=np.int64)
    tgt_boxes = torch.as_tensor(tgt_boxes)
    nl, N, QT, C = logits.shape
    Q, Qi, cap = QT - pad_cap, il.shape[1], qot.shape[1]
    cum_ok = bool(cum[0] == 0 and (np.diff(cum) >= 0).all() and (cum <= cap).all())
    total = int(cum[N]) if cum_ok else 0
    pad_size, groups, stride, overflow = 0, 1, 1, False
    if meta is not None:
        m_groups, m_pad, m_over = int(meta[1]), int(meta[2]), int(meta[4])
        if m_over != 0 or m_groups < 1 or m_pad < 0 or m_pad > pad_cap or m_pad % m_groups != 0:
            overflow = True
        else:
            pad_size, groups, stride = m_pad, m_groups, m_pad // m_groups
    if num_boxes is not None:
        nb = float(np.float32(num_boxes))
    else:
        q_last = qot[nl - 1, :total]
        nb = float(max(int(((q_last >= 0) & (q_last < Q)).sum()), 1))
    w_m64, w_d64 = 1.0 / nb, 1.0 / (nb * groups)
    rnd = (lambda v: float(np.float32(v))) if mode.f32_consts else (lambda v: v)      # formed in float64, rounded once
    w_m, w_d = rnd(w_m64), rnd(w_d64)
    # ---- the row weights (and groups) --------------------------------------------------------------------------------------------------
    s_idx = np.arange(QT)
    w_row = np.where(s_idx >= pad_cap, w_m, np.where((not overflow) & (s_idx < pad_size), w_d, 0.0))
    row_weight = np.broadcast_to(w_row, (nl, N, QT)).copy()
    row_group = np.broadcast_to(np.where(s_idx >= pad_cap, np.arange(nl)[:, None, None], nl + np.arange(nl)[:, None, None]), (nl, N, QT)).copy()
    row_weight_int, row_group_int = np.full((N, Qi), w_m), np.full((N, Qi), 2 * nl)
    # ---- the slots -----------------------------------------------------------------------------------------------------------------------
    rows, labels, ws, ts, two = [], [], [], [], []
    n_noquery = n_badlabel = 0
    for o in range(nl + 1):
        nq = Qi if o == nl else Q
        for tt in range(cap):
            row, t, w = -1, -1, 0.0
            if tt < total:
                q = int(qot[o, tt])
                if 0 <= q < nq:
                    b = int(np.searchsorted(cum[1:], tt, side="right"))
                    row, t = (b * Qi + q if o == nl else (o * N + b) * QT + pad_cap + q), tt
                    w = w_d if (o == nl and mutant == "two_stage_dn_weight") else w_m
                else:
                    n_noquery += 1
                if o == nl - 1:
                    n_badlabel += int(ids[tt] < 0 or ids[tt] >= C)
            rows.append(row), ts.append(t), ws.append(w), two.append(o == nl)
    for l in range(nl):
        for b in range(N):
            for s in range(pad_cap):
                row, t, w = -1, -1, 0.0
                if cum_ok and not overflow and s < pad_size:
                    j = s % stride
                    if j < cum[b + 1] - cum[b]:
                        row, t, w = (l * N + b) * QT + s, int(cum[b] + j), w_d
                rows.append(row), ts.append(t), ws.append(w), two.append(False)
    rows, ts, ws, two = np.array(rows), np.array(ts), np.array(ws), np.array(two)
    labels = np.zeros_like(rows)
    for i in np.nonzero(rows >= 0)[0]:
        lab = 0 if (two[i] and flags & 1) else int(ids[ts[i]])
        if lab < 0 or lab >= C:
            rows[i], ws[i] = -1, 0.0
        else:
            labels[i] = lab
    S = rows.size
    live = np.nonzero(rows >= 0)[0]
    xs_dec, xs_int = logits.reshape(-1, C), il.reshape(-1, C)
    ps_dec, ps_int = coords.reshape(-1, 4), ib.reshape(-1, 4)
    r_t, lab_t, two_t = torch.as_tensor(rows[live]), torch.as_tensor(labels[live]), torch.as_tensor(two[live])
    r_dec, r_int = r_t.clamp(max=xs_dec.shape[0] - 1), r_t.clamp(max=xs_int.shape[0] - 1)
    xv = torch.where(two_t, xs_int[r_int, lab_t].double(), xs_dec[r_dec, lab_t].double())
    pv = torch.where(two_t[:, None], ps_int[r_int].double(), ps_dec[r_dec].double())
    tv = tgt_boxes[torch.as_tensor(ts[live])].double()
    Wl = mode.lift(torch.as_tensor(ws[live]))
    w_grad = ws[live].copy()
    if mutant == "dn_weight_scaled":
        w_grad[live >= (nl + 1) * cap] *= 1.0 + 2.0 ** -12
    Wg = mode.lift(torch.as_tensor(w_grad))
    lc, dl = focal_pos_term(mode.lift(xv), alpha, mode)
    l1, giou = box_pair_terms(pv, tv, mode)
    lb = box_pair_loss_of(l1, giou, c_l1, c_giou, mode)
    v_cls, v_l1, v_giou = lc * Wl, l1.v * Wl, (1.0 - giou.v) * Wl
    gx = _scale_c(dl * Wl, c_cls, mode)
    gb = [x * Wg for x in lb.d]

    def spread(x):
        """a per-live-slot quantity laid out over all S slots (zeros, exact, elsewhere)"""
        idx = torch.as_tensor(live)
        if isinstance(x, B):
            v, e = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.float64)
            v[idx], e[idx] = x.v, x.e
            return B(v, e, mode)
        v = torch.zeros(S, dtype=x.dtype)
        v[idx] = x
        return v
    rec_gx = spread(gx)
    rec_gb = [spread(x) for x in gb]
    # ---- per-call terms: wave shuffles (6 float32 steps), float64 from there, one conversion ----------------------------------------------
    call_of = np.concatenate([np.repeat(np.r_[np.arange(nl), 2 * nl], cap), np.repeat(nl + np.arange(nl), N * pad_cap)])
    terms = []
    for call in range(2 * nl + 1):
        k = torch.as_tensor(call_of == call)
        terms.append([_to_f32(_sum_f32(spread(x)[k], 0, 6, mode), mode) for x in (v_cls, v_l1, v_giou)])
    status = [int(meta is not None and overflow), n_noquery, n_badlabel, int(not cum_ok)]
    # ---- the all-negative term and the backward -----------------------------------------------------------------------------------------------
    gs_cls = float(np.float32(gscale) * np.float32(c_cls)) if mode.f32_consts else gscale * c_cls
    flat_w = lambda a: torch.as_tensor(a.reshape(-1))
    kw_d = dict(group=torch.as_tensor(row_group.reshape(-1)), mask=class_mask) if class_mask is not None else {}
    kw_i = dict(group=torch.as_tensor(row_group_int.reshape(-1)), mask=class_mask) if class_mask is not None else {}
    _, g_logits, neg_d = focal_neg(xs_dec, flat_w(row_weight), alpha, gs_cls, mode, **kw_d)
    _, g_il, neg_i = focal_neg(xs_int, flat_w(row_weight_int), alpha, gs_cls, mode, **kw_i)
    neg_per_call = []
    if not mode.bounded:
        f, _ = focal_neg_term(mode.lift(xs_dec), mode)
        fi, _ = focal_neg_term(mode.lift(xs_int), mode)
        lv_d = _live(flat_w(row_weight), kw_d.get("group"), class_mask, 0 if class_mask is None else class_mask.shape[0], C)
        lv_i = _live(flat_w(row_weight_int), kw_i.get("group"), class_mask, 0 if class_mask is None else class_mask.shape[0], C)
        per_row = (torch.where(lv_d, f, torch.zeros_like(f)).double().sum(1) * flat_w(row_weight).double()) * (1.0 - alpha)
        for call in range(2 * nl):
            neg_per_call.append(float(per_row[torch.as_tensor(row_group.reshape(-1) == call)].sum()))
        neg_per_call.append(float((torch.where(lv_i, fi, torch.zeros_like(fi)).double().sum(1) * flat_w(row_weight_int).double()).sum() * (1.0 - alpha)))
    tsum = [_sum_f64_list([t[k] for t in terms]) for k in range(3)]
    loss = _to_f32((neg_d + neg_i + tsum[0]) * c_cls + tsum[1] * c_l1 + tsum[2] * c_giou, mode) if mode.bounded else \
        (neg_d.double() + neg_i.double() + tsum[0]) * c_cls + tsum[1] * c_l1 + tsum[2] * c_giou
    g = mode.c(gscale) if mode.f32_consts else gscale

    def scatter(dense, rec, idx_rows, col, sel):
        """dense[idx_rows, col] += rec * g for the selected live slots (one slot per entry)"""
        add = _scale_c(rec, g, mode)
        if isinstance(dense, B):
            cur = B(dense.v[idx_rows, col], dense.e[idx_rows, col], mode)
            new = cur + B(add.v[sel], add.e[sel], mode)
            dense.v[idx_rows, col], dense.e[idx_rows, col] = new.v, new.e
        else:
            dense[idx_rows, col] = dense[idx_rows, col] + add[sel]
    if isinstance(g_logits, B):
        g_logits = B(g_logits.v.clone(), g_logits.e.expand_as(g_logits.v).clone(), mode)
        g_il = B(g_il.v.clone(), g_il.e.expand_as(g_il.v).clone(), mode)
    sel_dec, sel_int = torch.as_tensor(live[~two[live]]), torch.as_tensor(live[two[live]])
    scatter(g_logits, rec_gx, torch.as_tensor(rows[sel_dec]), torch.as_tensor(labels[sel_dec]), sel_dec)
    scatter(g_il, rec_gx, torch.as_tensor(rows[sel_int]), torch.as_tensor(labels[sel_int]), sel_int)

    def box_grads(n_rows, sel):
        cols = []
        for x in rec_gb:
            add = _scale_c(x, g, mode)
            if isinstance(add, B):
                v, e = torch.zeros(n_rows, dtype=torch.float64), torch.zeros(n_rows, dtype=torch.float64)
                v[torch.as_tensor(rows[sel])], e[torch.as_tensor(rows[sel])] = add.v[sel], add.e[sel]
                cols.append(B(v, e, mode))
            else:
                v = torch.zeros(n_rows, dtype=add.dtype)
                v[torch.as_tensor(rows[sel])] = add[sel]
                cols.append(v)
        if isinstance(cols[0], B):
            return B(torch.stack([c.v for c in cols], 1), torch.stack([c.e for c in cols], 1), mode)
        return torch.stack(cols, 1)
    g_coords, g_ib = box_grads(nl * N * QT, sel_dec), box_grads(N * Qi, sel_int)
    stack = lambda tt: B(torch.stack([torch.stack([x.v for x in r]) for r in tt]), torch.stack([torch.stack([x.e for x in r]) for r in tt]), mode) \
        if mode.bounded else torch.stack([torch.stack([torch.as_tensor(x) for x in r]) for r in tt])
    return {"rows": rows, "labels": labels, "weights": ws, "rec_gx": rec_gx, "rec_gb": rec_gb, "terms": stack(terms), "status": status,
            "row_weight": row_weight.astype(np.float32), "row_weight_int": row_weight_int.astype(np.float32),
            "row_group": row_group.astype(np.int32), "row_group_int": row_group_int.astype(np.int32), "loss": loss,
            "grads": {"logits": g_logits, "coords": g_coords, "il": g_il, "ib": g_ib}, "neg_per_call": neg_per_call,
            "num_boxes": nb, "groups": groups, "pad_size": pad_size}


def _sum_f64_list(xs):
    if isinstance(xs[0], B):
        return B(sum(x.v for x in xs), sum(x.e for x in xs), xs[0].m)
    return sum(x.double() for x in xs)


# ---- the older whole-tensor criteria (what the kernels were held to before) ----------------------------------------------------------------
def _maxnorm_ok(got, want, rel):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    k = ~(torch.isnan(got) & torch.isnan(want))
    return want.numel() == 0 or float((got - want)[k].abs().max()) <= rel * float(want[k].abs().max())


def old_focal_neg(loss, grad, ref_loss, ref_grad):
    """tests/test_gpu_step.py::test_focal_negative_sum_kernel: loss 1e-5 relative, gradient 1e-5 of the largest gradient"""
    return abs(float(loss) - float(ref_loss)) < 1e-5 * abs(float(ref_loss)) and _maxnorm_ok(grad, ref_grad, 1e-5)


def old_pair(loss, grad, ref_loss, ref_grad, rel_grad):
    """tests/test_gpu_step.py::test_pair_loss_kernels_against_the_op_sequence: loss 2e-5 relative, gradient 2e-4 (boxes) / 2e-5 (focal)
    of the largest gradient"""
    return abs(float(loss) - float(ref_loss)) <= 2e-5 * abs(float(ref_loss)) + 1e-6 and _maxnorm_ok(grad, ref_grad, rel_grad)


def old_criterion(res, ref):
    """tests/test_gpu_criterion_capacity.py: loss 1e-5 relative, box terms 1e-5 relative per call, logit gradients 1e-5 and box gradients
    2e-4 of the largest reference gradient (``_close``)"""
    ok = abs(float(res["loss"]) - float(ref["loss"])) <= 1e-5 * abs(float(ref["loss"]))
    ok = ok and bool(((res["terms"][:, 1:] - ref["terms"][:, 1:]).abs() <= 1e-5 * ref["terms"][:, 1:].abs()).all())
    for k, rel in (("logits", 1e-5), ("il", 1e-5), ("coords", 2e-4), ("ib", 2e-4)):
        ok = ok and _maxnorm_ok(res["grads"][k], ref["grads"][k], rel)
    return ok


def old_matcher(got, want):
    """tests/test_gpu_matcher.py::test_cost_blocks_equal_oracle: 2e-5 max(|want|.max(), 1)"""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    k = ~torch.isnan(want)
    return float((got - want)[k].abs().max()) <= 2e-5 * max(float(want[k].abs().max()), 1.0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
_F32 = lambda v: float(np.float32(v))
EXPLICIT = [20.0, -20.0, float(np.nextafter(np.float32(20), np.float32(30))), float(np.nextafter(np.float32(20), np.float32(0))),
            16.6, -16.6, 30.0, -30.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 0.0, 2.0 ** -20, -2.0 ** -20]
EXPLICIT = [_F32(v) for v in EXPLICIT]
NEG_SHAPES = [(1, 3), (4096, 3), (4097, 3), (8192, 3), (8200, 3), (5, 1), (5, 255), (5, 256), (5, 257), (5, 1203)]
PAIR_K = [1, 63, 64, 65, 1023, 1024, 1025, 3001]
PAIR_COEF = [(5.0, 2.0), (1.0, 0.0), (0.0, 1.0)]
MATCHER_COUNTS = [(5, 3), (0, 4), (1, 0), (40, 7), (12, 0, 12)]


def neg_inputs(rows, C, seed=0):
    """logits N(0, 6), an eighth redrawn from U[-30, 30], the explicit values spread over the tensor; row weights 2^0 .. 2^-7, a tenth of
    them exactly 0; for the masked form 3 groups -- mask 0 empty, 1 full, 2 random -- and rows with group -1 and 3"""
    g = torch.Generator().manual_seed(1000 + 7 * rows + C + seed)
    x = torch.randn(rows, C, generator=g) * 6
    u = torch.rand(rows, C, generator=g) * 60 - 30
    x = torch.where(torch.rand(rows, C, generator=g) < 0.125, u, x)
    flat = x.reshape(-1)
    n = flat.numel()
    at = (torch.arange(len(EXPLICIT)) * max(n // len(EXPLICIT), 1)) % n
    if n >= len(EXPLICIT):
        flat[at] = torch.tensor(EXPLICIT)
    w = 2.0 ** -(torch.arange(rows) % 8).float()
    w[torch.rand(rows, generator=g) < 0.1] = 0.0
    if rows > 1:
        w[-1] = 1.0
    group = torch.randint(0, 3, (rows,), generator=g, dtype=torch.int32)
    if rows >= 5:
        group[1], group[3] = -1, 3
    mask = torch.stack((torch.zeros(C), torch.ones(C), (torch.rand(C, generator=g) < 0.5).float()))
    return x.contiguous(), w, group, mask


def kink_boxes():
    """pairs on the dyadic grid (centres on multiples of 2^-7, sizes on multiples of 2^-6: every corner is exact in float32 and float64,
    every comparison resolves alike): -> (names, pred (n, 4), target (n, 4))"""
    c, s = 2.0 ** -7, 2.0 ** -6
    T = (64 * c, 64 * c, 16 * s, 16 * s)      # centre 0.5, size 0.25: corners 0.375 .. 0.625
    cases = [
        ("identical", T),
        ("touching_x", (96 * c, 64 * c, 16 * s, 16 * s)),                  # left edge 0.625 = the target's right edge: iw == 0
        ("touching_y", (64 * c, 96 * c, 16 * s, 16 * s)),                  # ih == 0
        ("touching_x_unequal", (96 * c, 66 * c, 16 * s, 8 * s)),           # iw == 0 with ih != hh: GIoU has a kink here
        ("touching_y_unequal", (62 * c, 96 * c, 8 * s, 16 * s)),
        ("touching_corner", (96 * c, 96 * c, 16 * s, 16 * s)),
        ("one_shared_edge", (60 * c, 64 * c, 12 * s, 8 * s)),              # left edges coincide (0.375), inside otherwise
        ("two_shared_edges", (60 * c, 60 * c, 12 * s, 12 * s)),            # left and top
        ("three_shared_edges", (60 * c, 64 * c, 12 * s, 16 * s)),          # left, top and bottom
        ("nested", (64 * c, 66 * c, 8 * s, 4 * s)),
        ("nesting", (64 * c, 64 * c, 24 * s, 20 * s)),
        ("disjoint_x", (112 * c, 64 * c, 8 * s, 16 * s)),
        ("disjoint_xy", (16 * c, 112 * c, 4 * s, 8 * s)),
        ("zero_width", (64 * c, 64 * c, 0.0, 8 * s)),
        ("zero_height", (70 * c, 64 * c, 8 * s, 0.0)),
        ("zero_area_outside", (120 * c, 120 * c, 0.0, 0.0)),
        ("equal_cx", (64 * c, 70 * c, 12 * s, 20 * s)),
        ("equal_cy", (70 * c, 64 * c, 20 * s, 12 * s)),
        ("equal_w", (66 * c, 62 * c, 16 * s, 10 * s)),
        ("equal_h", (62 * c, 66 * c, 10 * s, 16 * s)),
        ("overlapping", (72 * c, 58 * c, 14 * s, 18 * s)),
    ]
    pred = torch.tensor([b for _, b in cases], dtype=torch.float32)
    tgt = torch.tensor([T] * len(cases), dtype=torch.float32)
    names = [n for n, _ in cases] + ["zero_area_target"]
    pred = torch.cat((pred, torch.tensor([[64 * c, 64 * c, 8 * s, 8 * s]])))
    tgt = torch.cat((tgt, torch.tensor([[64 * c, 64 * c, 0.0, 0.0]])))
    return names, pred, tgt


def pair_inputs(K, seed=11, old_test=False):
    """(``old_test``: the older test's own recipe -- no kink pairs, weights U[0, 1) with every 13th 0.)  The random boxes of tests/test_gpu_step.py::test_pair_loss_kernels_against_the_op_sequence followed by as many kink pairs as fit,
    weights 2^0 .. 2^-10 with every 13th exactly 0, logits N(0, 8) with the explicit values"""
    g = torch.Generator().manual_seed(seed + K)
    tb = torch.rand(K, 4, generator=g) * 0.5 + 0.2
    pb = (tb + 0.15 * torch.randn(K, 4, generator=g)).clamp(0.01, 0.99)
    if K >= 64:
        pb[:7] = tb[:7]
        pb[7:14, :2] = tb[7:14, :2] + 0.6
        pb[14:21, 2:] = tb[14:21, 2:] * 0.3
        pb[14:21, :2] = tb[14:21, :2]
    _, kp, kt = kink_boxes()
    n = min(K, kp.shape[0])
    if K >= 63 and not old_test:
        pb[K - n:], tb[K - n:] = kp[:n], kt[:n]
    w = torch.rand(K, generator=g) if old_test else 2.0 ** -(torch.arange(K) % 11).float()
    w[::13] = 0.0
    if K == 1:
        w[0] = 0.5
    x = torch.randn(K, generator=g) * 8
    n = min(K, len(EXPLICIT))
    x[:n] = torch.tensor(EXPLICIT[:n])
    return pb.contiguous(), tb.contiguous(), w, x


def matcher_inputs(counts, saturated, dtype=torch.float32, seed=3, Q=93, C=120):
    """Q = 93 queries, C = 120 classes, per-image target counts ``counts``; logits N(0, 2), or (saturated) 6 times that with explicit
    +-16.6, +-20, +-30 in the labels' columns; random boxes with the kink pairs among them; one label of the largest image out of range"""
    g = torch.Generator().manual_seed(seed + 17 * sum(counts) + len(counts) + (1 if saturated else 0))
    Bn, T = len(counts), sum(counts)
    logits = torch.randn(Bn, Q, C, generator=g, dtype=torch.float64) * 2
    rb = lambda n: torch.cat((torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.6 + 0.2, torch.rand(n, 2, generator=g, dtype=torch.float64) * 0.3 + 0.05), 1)
    boxes, tgt_boxes = rb(Bn * Q).reshape(Bn, Q, 4), rb(T)
    labels = torch.randint(0, C, (T,), generator=g)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    _, kp, kt = kink_boxes()
    for b in range(Bn):
        if counts[b]:
            tgt_boxes[offsets[b]] = kt[0].double()
            boxes[b, :kp.shape[0]] = kp.double()
    if saturated:
        logits = logits * 6
        vals = torch.tensor([16.6, -16.6, 20.0, -20.0, 30.0, -30.0], dtype=torch.float64)
        for b in range(Bn):
            for t in range(int(offsets[b]), int(offsets[b + 1])):
                logits[b, 20:26, labels[t]] = vals
    if max(counts) >= 7:
        b = int(np.argmax(counts))
        labels[offsets[b] + 2] = C + 3      # NaN in exactly that column
    if dtype == torch.float32:
        logits, boxes, tgt_boxes = logits.float(), boxes.float(), tgt_boxes.float()
    return logits.contiguous(), boxes.contiguous(), labels, tgt_boxes.contiguous(), offsets


def criterion_inputs(seed=5):
    """nl = 2, N = 3, counts [130, 0, 127] (an empty image; 257 targets: one past a 256-thread workgroup), capacity 300, Q = 140, Qi = 150,
    C = 7, 2 denoising groups, pad_cap = pad_size + 10; every target matched to a distinct query except two at -1, one label out of range"""
    nl, N, Q, Qi, C, groups, cap = 2, 3, 140, 150, 7, 2, 300
    counts = [130, 0, 127]
    g = torch.Generator().manual_seed(seed)
    total, single = sum(counts), max(counts)
    pad_size = 2 * single * groups
    pad_cap = pad_size + 10
    labels = torch.zeros(cap, dtype=torch.int64)
    labels[:total] = torch.randint(0, C, (total,), generator=g)
    labels[200] = C + 2
    rb = lambda *s: torch.cat((torch.rand(*s, 2, generator=g) * 0.6 + 0.2, torch.rand(*s, 2, generator=g) * 0.4 + 0.03), -1)
    tgt_boxes = torch.tensor([0.5, 0.5, 1.0, 1.0]).repeat(cap, 1)
    tgt_boxes[:total] = rb(total)
    _, kp, kt = kink_boxes()
    qot = torch.full((nl + 1, cap), -1, dtype=torch.int64)
    for o in range(nl + 1):
        at = 0
        for tb in counts:
            qot[o, at: at + tb] = torch.randperm(Qi if o == nl else Q, generator=g)[:tb]
            at += tb
    qot[0, 5], qot[nl, 140] = -1, -1
    logits = torch.randn(nl, N, pad_cap + Q, C, generator=g) * 3
    il = torch.randn(N, Qi, C, generator=g) * 3
    coords, ib = rb(nl, N, pad_cap + Q), rb(N, Qi)
    # kink pairs: targets 10 .. of image 0 take the kink targets, their matched predictions the kink predictions
    n = kp.shape[0]
    tgt_boxes[10: 10 + n] = kt
    for i in range(n):
        coords[1, 0, pad_cap + int(qot[1, 10 + i])] = kp[i]
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    meta = np.array([single, groups, pad_size, total, 0], dtype=np.int64)
    return {"logits": logits.contiguous(), "coords": coords.contiguous(), "il": il.contiguous(), "ib": ib.contiguous(), "cum": cum,
            "tgt_ids": labels, "tgt_boxes": tgt_boxes, "qot": qot, "meta": meta, "pad_cap": pad_cap, "counts": counts, "cap": cap,
            "dims": (nl, N, Q, Qi, C, groups)}


CRIT_VARIANTS = {
    "plain": {},
    "flags1": {"flags": 1},
    "num_boxes": {"num_boxes": 301.0},
    "no_meta": {"meta": None},
    "row_groups": {"mask": True},
    "row_groups_flags1": {"mask": True, "flags": 1},
}


def crit_args(variant):
    z = criterion_inputs()
    kw = dict(CRIT_VARIANTS[variant])
    meta = kw.pop("meta", z["meta"])
    nb = kw.pop("num_boxes", None)
    if kw.pop("mask", False):
        nl, C = z["dims"][0], z["dims"][4]
        g = torch.Generator().manual_seed(2)
        kw["class_mask"] = (torch.rand(2 * nl + 1, C, generator=g) < 0.6).float()
        kw["class_mask"][1] = 1.0
    return (z["logits"], z["coords"], z["il"], z["ib"], z["cum"], z["tgt_ids"], z["tgt_boxes"], z["qot"], meta, nb, z["pad_cap"]), kw, z


@functools.lru_cache(maxsize=None)
def crit_ref(variant, gscale=1.0):
    a, kw, _ = crit_args(variant)
    return criterion(*a, B32, gscale=gscale, **kw)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
