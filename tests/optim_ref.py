"""Float64 restatement of ONE step of the library optimizer (csrc/msda_optim.h: gradient clipping + AdamW + EMA) with an ELEMENT-WISE
error bound for everything the kernels write, and an fp32 emulation of the kernels' op order.  The comparator of tests/test_gpu_optim.py
(the kernels, and torch's own clip_grad_norm_ + fused AdamW, against the bounds) and of tests/test_optim_host.py (the definition against
torch.optim.AdamW in float64; the emulation against the bounds; wrong variants far outside them).  Test helper only.

All arguments are lists over the tensors: p, g (None: no gradient), m, v, ``step`` (the counters BEFORE the step), ``group_of`` (index
into ``groups``: dicts with lr, betas, eps, weight_decay), and optionally ema (None per tensor: no shadow) with ema_decay.  The inputs
are the float32 values, so their float64 copies are exact; float64 inputs are taken as they are.

The operation (torch.nn.utils.clip_grad_norm_, torch.optim.AdamW, reference util/utils.py:396-397), t = step + 1:

    total_norm = sqrt(sum g^2)        coef = min(1, max_norm / (total_norm + 1e-6))   (max_norm <= 0: 1)        g' = coef g
    p1 = p (1 - lr wd)                m' = b1 m + (1 - b1) g'                         v' = b2 v + (1 - b2) g'^2
    D = sqrt(v') / sqrt(1 - b2^t) + eps                                               p' = p1 - (lr / (1 - b1^t)) m' / D
    e' = d e + (1 - d) p'
A tensor without a gradient is untouched (bound 0) and contributes nothing to the norm.

The bounds.  u = 2^-24 is the unit round-off of fp32.  Each line counts the roundings of the kernel AND of torch's kernels (they order a few
operations differently; the larger count is taken), times the magnitude of the term each rounding acts on.

  total_norm   the kernel adds the squares in double (error far below u) and rounds sqrt once.  torch adds them in fp32: per thread a few
               sequential adds, a tree over the block, a second reduction over blocks, per-tensor norms squared and added again -- the
               depth of any of these at the sizes tested is below 128 additions, each a relative u on a sum of non-negative terms:
               relative error of the sum <= 128 u, of its square root half that, plus the roundings of the squares, of the root, of the
               second norm:        R_norm = (128 / 2 + 2) u = 66 u.
  coef         when clipping can be active (max_norm > 0 and max_norm / (total_norm + 1e-6) < 1 + 2 R_c):  R_c = R_norm + 3 u  (max_norm
               cast to fp32: 1, the addition of 1e-6: 1, the division: 1);  g' = coef g adds 1:  R_g = R_c + u.  Otherwise coef = 1 and
               g' = g exactly: R_g = 0.
  m'           A = max(b1, 1 - b1) |m|,  G = (1 - b1) |g'|.  kernel: cast of b1 (1) and product (1) on A, cast of 1 - b1 (1) and product
               (1) on G, the sum (1) on |m'|.  torch (lerp: m + (1 - b1)(g' - m)): difference (1), cast (1), product (1) on
               (1 - b1)|g' - m| <= G + A, the sum (1).    B_m = u (3 A + 3 G + |m'|) + G R_g
  v'           cast of b2 (1), product (1) on b2 v;  cast of 1 - b2 (1), g'^2 (1), product (1) on V = (1 - b2) g'^2;  the sum (1):
               B_v = u (2 b2 v + 3 V + v') + V (2 R_g + R_g^2)
  p1           wd = 0: exact.  Otherwise the factor (1) and the product (1) on |p1|; torch (p - (lr wd) p): cast (1), product (1) on
               |lr wd p|, difference (1) on |p1|:     B_p1 = u (2 |p1| + 2 |lr wd p|)
  D            s = sqrt(v'): its input error moves it by at most min(B_v / s, sqrt(B_v));  sqrt (2: not assumed correctly rounded),
               cast of sqrt(bc2) (1), division (2) on s / c2;  the sum (1) on D;  cast of eps (1) on eps:
               B_D = min(B_v / s, sqrt(B_v)) / c2 + u (5 s / c2 + D + eps)
  p'           U = step_size m' / D:  B_U = step_size (B_m / D_lo + |m'| B_D / (D D_lo)) + 4 u |U|   (cast of step_size 1, product 1,
               division 2), D_lo = D - B_D;   the difference (1) on |p'|:      B_p = B_p1 + B_U + u |p'|
  e'           cast (1), product (1) on |d e| and on |(1 - d) p'|, the sum (1) on |e'|, and the error of p':
               B_e = u (2 |d e| + 2 (1 - d) |p'| + |e'|) + (1 - d) B_p

TINY = 2^-126 is added to every bound: results below the normal range round with an absolute, not a relative, error; exact zeros compare.
"""
import math

import torch

U = 2.0 ** -24
R_NORM = 66 * U
TINY = 2.0 ** -126
TENSORS = ("p", "m", "v", "ema")
VARIANTS = ("l2_decay", "eps_in_sqrt", "no_clip", "step_off_by_one")      # wrong restatements: the bounds must tell them apart


def _norm_and_coef(g, max_norm):
    sq = [x.double().pow(2).sum() for x in g if x is not None]
    tn = torch.sqrt(torch.stack(sq).sum()) if sq else torch.zeros((), dtype=torch.float64)
    tn = tn.cpu()      # (the scalars stay on the host; the tensors may live anywhere)
    if max_norm > 0:
        q = max_norm / (tn + 1e-6)
        coef = torch.where(q > 1.0, torch.ones_like(q), q)      # (a NaN stays: torch.clamp(max=1.0))
    else:
        q, coef = None, torch.ones((), dtype=torch.float64)
    return tn, q, coef


def reference(p, g, m, v, step, groups, group_of, max_norm, ema=None, ema_decay=None, variant=None):
    """-> (values, bounds): dicts with "p", "m", "v", "ema" (lists of float64 tensors; ema entries None where there is no shadow),
    "total_norm" (a float64 scalar tensor) and, in values only, "step" (the counters after the step)"""
    assert variant in (None,) + VARIANTS
    n = len(p)
    ema = ema if ema is not None else [None] * n
    tn, q, coef = _norm_and_coef(g, max_norm)
    if variant == "no_clip":
        coef = torch.ones_like(coef)
    r_c = 0.0
    if max_norm > 0 and not bool(q >= 1.0 + 2 * (R_NORM + 3 * U)):
        r_c = R_NORM + 3 * U
    r_g = r_c + U if r_c else 0.0
    val = {k: [] for k in TENSORS + ("step",)}
    bnd = {k: [] for k in TENSORS}
    val["total_norm"], bnd["total_norm"] = tn, R_NORM * tn + TINY
    for i in range(n):
        pi, mi, vi = p[i].double(), m[i].double(), v[i].double()
        ei = None if ema[i] is None else ema[i].double()
        if g[i] is None:
            for k, x in (("p", pi), ("m", mi), ("v", vi), ("ema", ei)):
                val[k].append(x)
                bnd[k].append(None if x is None else torch.zeros_like(x))
            val["step"].append(step[i])
            continue
        G = groups[group_of[i]]
        lr, (b1, b2), eps, wd = G["lr"], G["betas"], G["eps"], G["weight_decay"]
        t = step[i] + 1
        val["step"].append(t)
        tb = t + 1 if variant == "step_off_by_one" else t
        gc = coef.to(pi.device) * g[i].double()
        if variant == "l2_decay":
            gc = gc + wd * pi
            p1 = pi
        else:
            p1 = pi * (1.0 - lr * wd)
        m1 = b1 * mi + (1.0 - b1) * gc
        v1 = b2 * vi + (1.0 - b2) * gc * gc
        c2 = math.sqrt(1.0 - b2 ** tb)
        step_size = lr / (1.0 - b1 ** tb)
        s = torch.sqrt(v1)
        D = torch.sqrt(v1 / c2 ** 2 + eps) if variant == "eps_in_sqrt" else s / c2 + eps
        upd = step_size * m1 / D
        p2 = p1 - upd
        # ---- bounds (module docstring) ----
        A, Gm = max(b1, 1.0 - b1) * mi.abs(), (1.0 - b1) * gc.abs()
        b_m = U * (3 * A + 3 * Gm + m1.abs()) + Gm * r_g
        V = (1.0 - b2) * gc * gc
        b_v = U * (2 * b2 * vi + 3 * V + v1) + V * (2 * r_g + r_g * r_g)
        b_p1 = U * (2 * p1.abs() + 2 * (lr * wd * pi).abs()) if wd != 0 else torch.zeros_like(p1)
        ds = torch.minimum(b_v / s.clamp_min(1e-300), torch.sqrt(b_v))
        b_D = ds / c2 + U * (5 * s / c2 + D + eps)
        D_lo = D - b_D
        assert bool((D_lo > 0).all()), "eps too small for the bound to hold"
        b_u = step_size * (b_m / D_lo + m1.abs() * b_D / (D * D_lo)) + 4 * U * upd.abs()
        b_p = b_p1 + b_u + U * p2.abs()
        val["p"].append(p2); bnd["p"].append(b_p + TINY)
        val["m"].append(m1); bnd["m"].append(b_m + TINY)
        val["v"].append(v1); bnd["v"].append(b_v + TINY)
        if ei is None:
            val["ema"].append(None); bnd["ema"].append(None)
        else:
            d = ema_decay
            e1 = d * ei + (1.0 - d) * p2
            val["ema"].append(e1)
            bnd["ema"].append(U * (2 * (d * ei).abs() + 2 * (1.0 - d) * p2.abs() + e1.abs()) + (1.0 - d) * b_p + TINY)
    return val, bnd


def emulate(p, g, m, v, step, groups, group_of, max_norm, ema=None, ema_decay=None):
    """The kernels' op order in fp32 on the CPU -> dict like reference()'s values, float32 (the squares are added in double and the
    per-workgroup constants formed in double, as the kernels do)"""
    f32 = lambda x: torch.tensor(x, dtype=torch.float64).float()
    n = len(p)
    ema = ema if ema is not None else [None] * n
    sq = [x.double().pow(2).sum() for x in g if x is not None]
    tn = torch.sqrt(torch.stack(sq).sum()).float().cpu() if sq else torch.zeros(())
    coef = torch.ones(())
    if max_norm > 0:
        q = f32(max_norm) / (tn + f32(1e-6))
        coef = torch.where(q > 1.0, torch.ones(()), q)
    out = {k: [] for k in TENSORS + ("step",)}
    out["total_norm"] = tn
    for i in range(n):
        if g[i] is None:
            for k, x in (("p", p[i]), ("m", m[i]), ("v", v[i]), ("ema", ema[i])):
                out[k].append(None if x is None else x.float())
            out["step"].append(step[i])
            continue
        G = groups[group_of[i]]
        lr, (b1, b2), eps, wd = G["lr"], G["betas"], G["eps"], G["weight_decay"]
        t = step[i] + 1
        out["step"].append(t)
        gc = coef.to(g[i].device) * g[i].float()
        p1 = p[i].float() * f32(1.0 - lr * wd)
        m1 = f32(b1) * m[i].float() + f32(1.0 - b1) * gc
        v1 = f32(b2) * v[i].float() + f32(1.0 - b2) * (gc * gc)
        D = torch.sqrt(v1) / f32(math.sqrt(1.0 - b2 ** t)) + f32(eps)
        p2 = p1 - f32(lr / (1.0 - b1 ** t)) * m1 / D
        out["p"].append(p2); out["m"].append(m1); out["v"].append(v1)
        out["ema"].append(None if ema[i] is None else f32(ema_decay) * ema[i].float() + f32(1.0 - ema_decay) * p2)
    return out


def ratios(got, val, bnd, keys=TENSORS + ("total_norm",)):
    """worst |got - want| / bound per output over all tensors (inf where a NaN / inf pattern differs or an untouched tensor moved)"""
    res = {}
    for k in keys:
        worst = 0.0
        pairs = [(got[k], val[k], bnd[k])] if k == "total_norm" else zip(got[k], val[k], bnd[k])
        for a, w, b in pairs:
            if w is None:
                continue
            a = a.detach().double().to(w.device).reshape(w.shape)
            diff = (a - w).abs()
            r = torch.where(diff == 0, torch.zeros_like(diff), diff / b)      # (bound 0: exact or inf)
            r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
            if r.numel():
                worst = max(worst, float(r.max()))
        res[k] = worst
    return res


def nan_pattern(xs):
    """where the tensors of a list hold NaN (the non-finite cases compare patterns, not values)"""
    return [torch.isnan(x.detach().cpu()) for x in xs]
