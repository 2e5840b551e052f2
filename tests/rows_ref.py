"""Float64 restatement of the prep, box-head, GroupNorm and pooling kernels with an ELEMENT-WISE error bound for every output, the input
recipes, the exact probes and the wrong variants of tests/test_rows_ref.py (CPU) and tests/test_gpu_rows_bounds.py (the kernels).  Test
helper only.  The machinery -- ``B`` (a value with a counted bound), ``Mode`` (F64 / F32 / B32 / B64), ``ratio``, ``tightness`` -- is
tests/loss_ref.py's, imported, and so are its counting rules (its docstring).

Kernels restated, operation for operation, in the kernels' order:
    prep_forward / prep_backward     csrc/msda_prep.h      softmax over the L P lanes of a (query, head), location arithmetic; their
                                                           gradients, grad_ref through the butterfly (f32, f64, bf16 projection)
    mask_rows                        csrc/msda_prep.h      exact: masked rows all-zero bits, everything else untouched
    box_refine / box_refine_grad     csrc/rows_api.hip     sigmoid(delta + inverse_sigmoid(ref)), grad_delta, grad_ref (clamp gradients)
    sine_embed                       csrc/rows_api.hip     sin | cos of coordinate 2 pi exp2(-log2(T) 2 k / pe_dim), bf16
    narrow_linear_dx / _dw           csrc/rows_api.hip     fma chains; dw / db: a workgroup's chain, then float32 atomics
    gn8_stats/apply/bwd_stats/bwd_apply, pool_nhwc         csrc/conv_mfma.hip

What this family adds to the rules:
    bf16 store       the float32 value v with bound e is rounded once: U_BF16 (|v| + e) on top of e, U_BF16 = 2^-8 -- bf16 keeps 8
                     significant bits, so half an ulp is up to 2^-8 |v| (at the bottom of a binade); this is tests/msda_ref.py's term (2^-9 |v|
                     would refuse correctly rounded stores).  Stores are also held to msda_ref's monotone interval
                     [rn_bf16(v - e), rn_bf16(v + e)] (``bf16_outside``).
    sinf, cosf, exp2f, rsqrtf, expf, logf     the LIBM allowance (4 u |result|); sin and cos carry the argument's absolute error unchanged.
    fmaf             one rounding: fl(a b + c) costs u |a b + c| (nothing where the exact result is a float32 and the operands are error-free).
    sums of known order (a thread's chain)    followed step by step.
    sums of unknown order (atomics, butterflies)   sum e_k + n u sum |t_k| with n the real depth.  Float64 accumulation adds nothing visible.
    GroupNorm        is bounded IN THE ORDER OF THE DEFINITION -- the mean, then the centred second moment -- and NOT in the kernel's order
                     (sums of x and x^2, variance as E[x^2] - mean^2).  This is the one place where the restatement deliberately does not follow
                     the kernel: a bound that followed E[x^2] - mean^2 in float32 partials would carry a term mean^2 / var and would accept the
                     loss of the variance it is there to find.  The depth of both sums is the kernel's partition: 4 additions per trip of a thread
                     over its strip (+ 1 inside the pair), 8 shuffle / tree levels, the strips.  The bound has n u |mean| / std (the float32 mean
                     the apply kernel subtracts is rounded; a float32 sum of the kernel's depth is admitted -- the kernel itself adds in fp64
                     and stays far inside) and nothing proportional to mean^2 / var.  F32 mode is the float32 two-pass evaluation in that partition.
                     A constant group whose partial sums are all float32 numbers has an exact mean, xhat = 0 exactly and out = beta exactly.
                     The parent kernel's order, in float32 partials, is wrong variant (l).
f64 instances use u = 2^-53 and are held to 2 bounds (loss_ref.py).  A bound of 0 asks for the exact value.
"""
import functools
import math

import numpy as np
import torch

from loss_ref import (B, B32, B64, ETA32, F32, F64, F64K, LIBM, U32, U64, Mode, _exp, _like, _like_full, _log, _max, _sum_f32, _to_f32,  # noqa: F401
                      _v, _where, ratio, tightness)
from msda_ref import U_BF16, outside_interval

EPS_BOX = float(np.float32(1e-3))

MUTANTS = (
    ("logit_dot_dropped", "prep_backward", "(a) - a * dot dropped from grad_logits where a < 2^-10"),
    ("ly_with_rw", "prep_forward", "(b) ly formed with rw instead of rh on the last level only"),
    ("ref_wh_last_head", "prep_backward", "(c) the w / h part of grad_ref missing the last head"),
    ("pad_lanes_in_sum", "prep_forward", "(d) the pad lanes of an odd L P contributing exp(0) to the softmax sum"),
    ("ref_grad_blocked_at_bounds", "box_refine", "(e) grad_ref blocked at exactly r = 0 and r = 1"),
    ("eps_strict", "box_refine", "(f) r >= eps taken as r > eps at r == eps"),
    ("y1my_as_y", "box_refine", "(g) y (1 - y) taken as y where y < 2^-12"),
    ("phase_scaled", "sine_embed", "(h) the phase of channels k >= 16 times 1 + 2^-9"),
    ("w_block_swapped", "sine_embed", "(i) sin and cos swapped in the w block only"),
    ("dw_last_token", "narrow_linear", "(j) the last token of a workgroup's chunk left out of dw when T % 8 == 1"),
    ("db_column0", "narrow_linear", "(k) db read at column 0 for every column"),
    ("ex2_f32_partials", "group_norm", "(l) the parent's E[x^2] - mean^2 in float32 partials"),
    ("dx_b_term_dropped", "group_norm", "(m) B / cnt * xhat dropped from dx where |xhat| < 2^-6"),
    ("avg_bf16_reciprocal", "avg_pool", "(n) the reciprocal 1 / (k k) rounded to bf16, k = 3 (as first proposed, k = 1, it is a no-op)"),
)
# whether the kernel's older whole-tensor criterion (the table in profiles/r26_row_bounds.md) lets the variant pass on the older test's own
# inputs; asserted in tests/test_rows_ref.py
OLD_CRITERION_PASSES = {
    "logit_dot_dropped": False,      # 5e-4 of the largest gradient against 2e-4 -- but only because M L P = 128 softmax rows are dense in small a
    "ly_with_rw": False, "ref_wh_last_head": False,
    "pad_lanes_in_sum": True,        # the module tests have L P = 16: no pad lane, the variant is the kernel there
    "ref_grad_blocked_at_bounds": False, "eps_strict": True, "y1my_as_y": True,
    "phase_scaled": True, "w_block_swapped": False,
    "dw_last_token": True,           # the older T (37, 2184, 44646) are 5, 0, 6 modulo 8: the branch is never taken
    "db_column0": False,
    "ex2_f32_partials": True, "dx_b_term_dropped": True, "avg_bf16_reciprocal": True,
}


# ---- small additions to loss_ref's operations ---------------------------------------------------------------------------------------------
def bf(t):
    """round to bf16 and back (the value a bf16 tensor holds), keeping the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def store_bf16(x):
    """the bf16 store of a float32 result: -> B with the storage term added (F32: the rounded tensor; F64: unchanged)"""
    if isinstance(x, B):
        return B(x.v, x.e + U_BF16 * (x.v.abs() + x.e), x.m)
    return bf(x) if x.dtype == torch.float32 else x


def bf16_outside(got, ref32):
    """how many stored bf16 elements lie outside [rn_bf16(v - e), rn_bf16(v + e)] of the float32 result ``ref32`` (a B before its store)"""
    return outside_interval(got.detach().float().cpu().reshape(ref32.v.shape), ref32.v.numpy(), ref32.e.expand_as(ref32.v).numpy())


def _fma(a, b, c):
    """fmaf(a, b, c) for error-free a, b (tensors) and an accumulated c: one rounding"""
    if isinstance(c, B):
        v = a * b + c.v
        return B(v, c.e + c._rnd(v, c.e), c.m)
    if c.dtype == torch.float32:
        return (a.double() * b.double() + c.double()).float()
    return a * b + c


def _libm(x, f, df_abs):
    """y = f(x) through a libm call: the argument's error times |f'| (first order, on the interval's worse end) + LIBM u |y|"""
    if isinstance(x, B):
        v = f(x.v)
        return B(v, x.e * df_abs(x) + LIBM * x.m.u * v.abs() + x.m.eta, x.m)
    return f(x)


def _sin(x):
    return _libm(x, torch.sin, lambda b: 1.0)


def _cos(x):
    return _libm(x, torch.cos, lambda b: 1.0)


def _exp2(x):
    return _libm(x, torch.exp2, lambda b: torch.exp2(b.v + b.e) * math.log(2.0))


def _rsqrt(x):
    return _libm(x, torch.rsqrt, lambda b: 0.5 * (b.v - b.e).clamp(min=1e-300) ** -1.5)


def _sum(x, dim, depth, mode):
    """an accumulation of ``depth`` additions in the compute type (f64 kernels too: u = 2^-53), in any order.  Exactness: error-free terms
    on a common dyadic grid (multiples of 2^-12) whose absolute sum stays below 2^24 grid steps have float32 partial sums in every order"""
    r = _sum_f32(x, dim, depth, mode)
    if isinstance(x, B):
        grid = x.v * 4096.0
        exact = ((x.e.expand_as(x.v) == 0) & (grid == grid.round())).all(dim) & (grid.abs().sum(dim) < 2.0 ** 24)
        r = B(r.v, torch.where(exact, torch.zeros_like(r.e), r.e), r.m)
    return r


def _cat(parts, dim):
    if isinstance(parts[0], B):
        return B(torch.cat([p.v for p in parts], dim), torch.cat([p.e.expand_as(p.v) for p in parts], dim), parts[0].m)
    return torch.cat(parts, dim)


def _stack(parts, dim):
    if isinstance(parts[0], B):
        return B(torch.stack([p.v for p in parts], dim), torch.stack([p.e.expand_as(p.v) for p in parts], dim), parts[0].m)
    return torch.stack(parts, dim)


def _reshape(x, *shape):
    return B(x.v.reshape(*shape), x.e.expand_as(x.v).reshape(*shape), x.m) if isinstance(x, B) else x.reshape(*shape)


def _zero_like(x):
    return B(torch.zeros_like(x.v), None, x.m) if isinstance(x, B) else torch.zeros_like(x)


def _f32(v):
    return float(np.float32(v))


# ---- prep forward / backward ---------------------------------------------------------------------------------------------------------------------
def lanes(L, P):
    G = 1
    while G < L * P:
        G *= 2
    return G


def prep_forward(offsets, logits, ref, shapes, mode, mutant=None, sum_depth=None):
    """prep_forward_kernel: offsets (N, Lq, M, L, P, 2), logits (N, Lq, M, L, P), ref (N, Lq, L, 2 | 4), shapes [(H, W)] -> (loc, aw).
    The softmax sum is a butterfly over G lanes (log2 G additions, the same number in every lane; pad lanes add an exact 0).
    ``sum_depth``: the depth of the same sum in the fused forms, which cut it differently (``fused_sum_depth``)."""
    N, Lq, M, L, P, _ = offsets.shape
    rd = ref.shape[-1]
    G = lanes(L, P)
    depth = int(math.log2(G)) if sum_depth is None else sum_depth
    X = mode.lift(logits.reshape(N, Lq, M, L * P))
    mx = _like(_v(X).max(-1, keepdim=True)[0], X)
    e = _exp(X - mx)
    s = _sum(e, -1, depth, mode)
    if mutant == "pad_lanes_in_sum" and (L * P) % 2 == 1:
        s = s + float(G - L * P)
    aw = _reshape(e / s[..., None], N, Lq, M, L, P)
    O, R = mode.lift(offsets), mode.lift(ref)
    ox, oy = O[..., 0], O[..., 1]
    rx, ry = R[:, :, None, :, None, 0], R[:, :, None, :, None, 1]
    if rd == 2:
        Wn = torch.tensor([float(w) for _, w in shapes], dtype=torch.float64)[None, None, None, :, None]
        Hn = torch.tensor([float(h) for h, _ in shapes], dtype=torch.float64)[None, None, None, :, None]
        lx, ly = rx + ox / _like(Wn.to(_v(ox).dtype), ox), ry + oy / _like(Hn.to(_v(oy).dtype), oy)
    else:
        rw, rh = R[:, :, None, :, None, 2], R[:, :, None, :, None, 3]
        lx = rx + ox / float(P) * rw * 0.5
        ly = ry + oy / float(P) * rh * 0.5
        if mutant == "ly_with_rw":
            last = torch.zeros(1, 1, 1, L, 1, dtype=torch.bool)
            last[..., L - 1, :] = True
            ly = _where(last.expand(_v(ly).shape), ry + oy / float(P) * rw * 0.5, ly)
    return _stack([lx, ly], -1), aw


def prep_backward(grad_loc, grad_aw, aw, offsets, ref, shapes, mode, want_ref=True, bf16_proj=False, mutant=None):
    """prep_backward_kernel -> (grad_offsets, grad_logits, grad_ref or None); with ``bf16_proj`` the two projection gradients are stored in
    bf16 (-> also their float32 forms before the store, for the interval check: (goff, glog, gref, goff32, glog32))"""
    N, Lq, M, L, P, _ = grad_loc.shape
    rd = ref.shape[-1]
    G = lanes(L, P)
    depth = int(math.log2(G))
    A, GA = mode.lift(aw.reshape(N, Lq, M, L * P)), mode.lift(grad_aw.reshape(N, Lq, M, L * P))
    dot = _sum(A * GA, -1, depth, mode)
    glog = A * (GA - dot[..., None])
    if mutant == "logit_dot_dropped":
        glog = _where(_v(A) < 2.0 ** -10, A * GA, glog)
    glog = _reshape(glog, N, Lq, M, L, P)
    GL, O, R = mode.lift(grad_loc), mode.lift(offsets), mode.lift(ref)
    gx, gy = GL[..., 0], GL[..., 1]
    gref = None
    if rd == 2:
        Wn = torch.tensor([float(w) for _, w in shapes], dtype=torch.float64)[None, None, None, :, None]
        Hn = torch.tensor([float(h) for h, _ in shapes], dtype=torch.float64)[None, None, None, :, None]
        dox, doy = gx / _like(Wn.to(_v(gx).dtype), gx), gy / _like(Hn.to(_v(gy).dtype), gy)
    else:
        rw, rh = R[:, :, None, :, None, 2], R[:, :, None, :, None, 3]
        dox, doy = gx / float(P) * rw * 0.5, gy / float(P) * rh * 0.5
    if want_ref:
        # a lane's chain over the heads (in order), then the butterfly over the lanes of its level
        def chain(t, heads):
            s = None
            for m in range(heads):
                s = t[:, :, m] if s is None else s + t[:, :, m]
            return _sum(s, -1, depth, mode)      # (N, Lq, L, P) -> (N, Lq, L)
        parts = [chain(gx, M), chain(gy, M)]
        if rd == 4:
            heads = M - 1 if mutant == "ref_wh_last_head" else M
            tw, th = gx * (O[..., 0] / float(P)) * 0.5, gy * (O[..., 1] / float(P)) * 0.5
            parts += [chain(tw, heads), chain(th, heads)] if heads > 0 else [_zero_like(parts[0]), _zero_like(parts[0])]
        gref = _stack(parts, -1)
    goff = _stack([dox, doy], -1)
    if bf16_proj:
        return store_bf16(goff), store_bf16(glog), gref, goff, glog
    return goff, glog, gref


def prep_torch_f64(offsets, logits, ref, shapes, grad_loc=None, grad_aw=None):
    """the module's softmax + location lines (ms_deform_attn.py:100-109) in torch float64 autograd: -> (loc, aw[, grad_offsets, grad_logits,
    grad_ref])"""
    N, Lq, M, L, P, _ = offsets.shape
    o, x, r = (t.double().clone().requires_grad_(True) for t in (offsets, logits, ref))
    aw = torch.softmax(x.reshape(N, Lq, M, L * P), -1).reshape(N, Lq, M, L, P)
    if ref.shape[-1] == 2:
        norm = torch.tensor([[float(w), float(h)] for h, w in shapes], dtype=torch.float64)
        loc = r[:, :, None, :, None, :] + o / norm[None, None, None, :, None, :]
    else:
        loc = r[:, :, None, :, None, :2] + o / P * r[:, :, None, :, None, 2:] * 0.5
    if grad_loc is None:
        return loc.detach(), aw.detach()
    torch.autograd.backward([loc, aw], [grad_loc.double(), grad_aw.double()])
    return loc.detach(), aw.detach(), o.grad, x.grad, r.grad


PREP_LP = [(4, 4), (3, 3), (2, 5), (1, 1), (4, 8), (4, 16), (4, 9)]
PREP_SHAPES = [(13, 21), (7, 11), (4, 6), (2, 3)]
PREP_SHAPES_POW2 = [(8, 16), (4, 8), (2, 4), (1, 2)]


def prep_inputs(L, P, M, rd, N=2, Lq=37, dtype=torch.float32, bf16_proj=False, seed=0, special=True):
    """offsets N(0, 2) (pixels for ref_dim 2, N(0, 1) units of a box for 4), logits N(0, 1.5) with the special rows -- a spread row of range
    80, an all-equal row, one 0 among -200s -- in the first three (query, head)s; reference points U(0.1, 0.9), box sides U(0.01, 0.5);
    gradients N(0, 1); for a bf16 projection offsets and logits are rounded to bf16 first"""
    g = torch.Generator().manual_seed(77 + 131 * L + 17 * P + 5 * M + rd + seed)
    LP = L * P
    off = torch.randn(N, Lq, M, L, P, 2, generator=g, dtype=torch.float64) * (2.0 if rd == 2 else 1.0)
    log = torch.randn(N, Lq, M, L, P, generator=g, dtype=torch.float64) * 1.5
    flat = log.reshape(N * Lq * M, LP)
    if special:
        flat[0] = torch.linspace(-40.0, 40.0, LP) if LP > 1 else 0.0
        flat[1] = 0.75
        flat[2] = -200.0
        flat[2, LP // 2] = 0.0
    ref = torch.rand(N, Lq, L, rd, generator=g, dtype=torch.float64) * 0.8 + 0.1
    if rd == 4:
        ref[..., 2:] = torch.rand(N, Lq, L, 2, generator=g, dtype=torch.float64) * 0.49 + 0.01
    gl = torch.randn(N, Lq, M, L, P, 2, generator=g, dtype=torch.float64)
    ga = torch.randn(N, Lq, M, L, P, generator=g, dtype=torch.float64)
    off, log, ref, gl, ga = (t.to(dtype) for t in (off, log, ref, gl, ga))
    if bf16_proj:
        off, log = bf(off), bf(log)
    return off.contiguous(), log.contiguous(), ref.contiguous(), gl.contiguous(), ga.contiguous()


def fused_sum_depth(fused, L, P, D=32, f64=False):
    """the softmax sum of msda_forward_prep_*: fwd_prep_fused 1 (fwd_direct_prep_kernel, msda_direct.h) -- a lane adds its points j, j + G, ...
    in order, then a butterfly over the G = max(8, D / channels per lane) lanes of the item; 2 (the window kernel, msda_tiled.h) -- a lane of
    the quad adds its point of every level in order, then two steps over the quad"""
    if fused == 2:
        return (L - 1) + 2
    G = max(8, lanes(1, D // (2 if f64 else 4)))
    return (-(-L * P // G) - 1) + int(math.log2(G))


def keep_off_pixel_boundaries(off, log, ref, shapes, bf16_proj=False, near=2.0 ** -10):
    """offsets whose sampling position (float32 or float64 evaluation) lies within 2^-10 pixel of an integer grow by 1 / 16 (+ 0.02) until none
    does: tests/msda_ref.py's bound of ``out`` needs floor() to decide alike in the kernel and in float64 (its boundary_distance)"""
    off = off.clone()
    for _ in range(40):
        bad = torch.zeros(off.shape, dtype=torch.bool)
        for mode in (F32, F64):
            loc = _v(prep_forward(off.to(mode.dtype), log.to(mode.dtype), ref.to(mode.dtype), shapes, mode)[0]).double()
            for l, (H, Wd) in enumerate(shapes):
                for c, size in ((0, Wd), (1, H)):
                    im = loc[:, :, :, l, :, c] * size - 0.5
                    bad[:, :, :, l, :, c] |= (im - im.round()).abs() < near
        if not bool(bad.any()):
            return off
        off = torch.where(bad, off * 1.0625 + torch.where(off < 0, -0.02, 0.02), off)      # (away from 0: visible in bf16 too)
        if bf16_proj:
            off = bf(off)
    raise AssertionError("sampling positions stay on pixel boundaries")


def prep_probe_inputs(rd, dtype, L=4, P=4, M=3, N=2, Lq=37):
    """the exact probes: offsets on multiples of 1/4, reference points on multiples of 1/64, box sides powers of two, the power-of-two level
    shapes; logits all equal in the even rows, one 0 among -200s (float64: -1000s, where exp underflows to 0 there too) in the odd rows;
    for the backward an aw that is uniform / one-hot in the same rows and gradients on multiples of 1/8"""
    g = torch.Generator().manual_seed(4 + rd)
    off = torch.randint(-32, 33, (N, Lq, M, L, P, 2), generator=g).to(dtype) / 4
    log = torch.full((N, Lq, M, L, P), 0.75, dtype=dtype)
    flat = log.reshape(-1, L * P)
    flat[1::2] = -1000.0 if dtype == torch.float64 else -200.0
    flat[1::2, 5] = 0.0
    ref = torch.randint(1, 64, (N, Lq, L, rd), generator=g).to(dtype) / 64
    if rd == 4:
        ref[..., 2:] = 2.0 ** -torch.randint(1, 6, (N, Lq, L, 2), generator=g).to(dtype)
    aw = torch.full((N * Lq * M, L * P), 1.0 / (L * P), dtype=dtype)
    aw[1::2] = 0.0
    aw[1::2, 5] = 1.0
    ga = torch.randint(-16, 17, (N, Lq, M, L, P), generator=g).to(dtype) / 8
    gl = torch.randint(-16, 17, (N, Lq, M, L, P, 2), generator=g).to(dtype) / 8
    return off, log, ref, aw.reshape(N, Lq, M, L, P), gl, ga


# ---- box refine ----------------------------------------------------------------------------------------------------------------------------------
def box_refine(delta, ref, eps, mode):
    """box_refine_kernel: y = 1 / (1 + expf(-(delta + logf(max(r, eps) / max(1 - r, eps))))), r = clamp(ref, 0, 1)"""
    D = mode.lift(delta)
    r = mode.lift(torch.as_tensor(ref).clamp(0.0, 1.0))
    epsc = mode.c(eps) if mode.f32_consts else eps
    u = D + _log(_max(r, epsc) / _max(1.0 - r, epsc))
    return 1.0 / (1.0 + _exp(-u))


def box_refine_grad(gy, y, ref, eps, mode, bf16_delta=False, mutant=None):
    """box_refine_grad_kernel on the kernel's own y: -> (grad_delta, grad_ref, grad_delta before a bf16 store)"""
    GY, Y = mode.lift(gy), mode.lift(y)
    v = GY * Y * (1.0 - Y)
    if mutant == "y1my_as_y":
        v = _where(_v(Y) < 2.0 ** -12, GY * Y, v)
    r0 = torch.as_tensor(ref)
    r = mode.lift(r0.clamp(0.0, 1.0))
    epsc = mode.c(eps) if mode.f32_consts else eps
    omr = 1.0 - r
    if isinstance(omr, B):
        assert not bool((((omr.v - epsc).abs() <= omr.e) & (omr.e > 0)).any()), "1 - r too close to eps for a float32 comparison"
    lo_ok = _v(r) > epsc if mutant == "eps_strict" else _v(r) >= epsc
    hi_ok = _v(omr) >= epsc
    dr = _where(lo_ok, 1.0 / _max(r, epsc), 0.0) + _where(hi_ok, 1.0 / _max(omr, epsc), 0.0)
    inside = (r0 >= 0.0) & (r0 <= 1.0)
    if mutant == "ref_grad_blocked_at_bounds":
        inside = (r0 > 0.0) & (r0 < 1.0)
    gref = _where(inside, v * dr, 0.0)
    return (store_bf16(v) if bf16_delta else v), gref, v


def box_torch_f64(delta, ref, eps, gy):
    """inverse_sigmoid + sigmoid under torch float64 autograd (clamp gradients included): -> (y, grad_delta, grad_ref)"""
    d, r = delta.double().clone().requires_grad_(True), ref.double().clone().requires_grad_(True)
    x = r.clamp(min=0, max=1)
    y = (d + torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))).sigmoid()
    y.backward(gy.double())
    return y.detach(), d.grad, r.grad


def _nbrs(v):
    v = np.float32(v)
    return [float(np.nextafter(v, np.float32(-10))), float(v), float(np.nextafter(v, np.float32(10)))]


BOX_EXPLICIT_REF = _nbrs(0.0) + _nbrs(1.0) + _nbrs(EPS_BOX) + _nbrs(np.float32(1) - np.float32(EPS_BOX)) + [_f32(1e-4), _f32(1 - 1e-4), _f32(-0.1),
                                                                                                        _f32(1.2), 0.5]
BOX_N = [1, 255, 256, 257, 2048 * 256 + 5]


def box_inputs(n, bf16_delta=False, seed=0):
    """ref U(0, 1) with the explicit values first; delta N(0, 1) with +-20 and +-90 at the end; gy N(0, 1)"""
    g = torch.Generator().manual_seed(9 + n + seed)
    ref = torch.rand(n, generator=g)
    k = min(n, len(BOX_EXPLICIT_REF))
    ref[:k] = torch.tensor(BOX_EXPLICIT_REF[:k])
    delta = torch.randn(n, generator=g)
    if n >= 64:
        delta[-4:] = torch.tensor([20.0, -20.0, 90.0, -90.0])
        delta[-8:-4] = torch.tensor([8.0, -8.5, 9.0, -9.5])      # y and 1 - y below 2^-12
    gy = torch.randn(n, generator=g)
    return (bf(delta) if bf16_delta else delta), ref, gy


# ---- sine embed ----------------------------------------------------------------------------------------------------------------------------------
def sine_embed(boxes, pe_dim, mode, temperature=10000.0, mutant=None):
    """sine_embed_kernel: boxes (tokens, dims) -> (tokens, dims * pe_dim) before (B32: also after) the bf16 store, blocks (y, x, w, h).
    log2f(temperature) is formed on the host (an ulp allowed)."""
    tokens, dims = boxes.shape
    half = pe_dim // 2
    k = torch.arange(half, dtype=torch.float64)
    if mode is F64:
        scale = torch.exp2(-math.log2(temperature) * (2.0 * k) / pe_dim)
        two_pi = 2.0 * math.pi
    else:
        l2t = mode.lift(torch.tensor(_f32(math.log2(temperature))))
        if isinstance(l2t, B):
            l2t = B(l2t.v, 2.0 * l2t.m.u * l2t.v.abs(), l2t.m)
        scale = _exp2(-l2t * mode.lift(2.0 * k) / float(pe_dim))
        two_pi = mode.c(6.283185307179586)
    X = mode.lift(boxes)
    out = []
    for part in range(dims):
        src = 1 - part if part < 2 else part
        p = (X[:, src] * two_pi)[:, None] * scale[None, :]
        if mutant == "phase_scaled":
            p = _where((k >= 16)[None, :].expand(_v(p).shape), p * (1.0 + 2.0 ** -9), p)
        s, c = _sin(p), _cos(p)
        if mutant == "w_block_swapped" and part == 2:
            s, c = c, s
        out.append(_reshape(_stack([s, c], -1), tokens, pe_dim))
    return _cat(out, 1)


def sine_torch_f64(boxes, pe_dim):
    """gen_sineembed_for_position's op sequence in float64"""
    dim_t = torch.arange(pe_dim, dtype=torch.float64)
    dim_t = 10000.0 ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / pe_dim)

    def emb(c):
        p = (c.double() * (2 * math.pi))[:, None] / dim_t
        return torch.stack((p[:, 0::2].sin(), p[:, 1::2].cos()), dim=2).flatten(1)
    parts = [emb(boxes[:, 1]), emb(boxes[:, 0])]
    if boxes.shape[1] == 4:
        parts += [emb(boxes[:, 2]), emb(boxes[:, 3])]
    return torch.cat(parts, 1)


def sine_inputs(tokens, dims, seed=0):
    g = torch.Generator().manual_seed(3 + tokens + dims + seed)
    b = torch.rand(tokens, dims, generator=g)
    special = [0.0, 1.0, 2.0 ** -20, 0.25]
    for i, v in enumerate(special[:tokens]):
        b[i] = v
    return b


# ---- narrow linear backward ------------------------------------------------------------------------------------------------------------------------
NARROW_T = [1, 7, 8, 9, 31, 32, 33, 8191, 8192, 65536 + 5]


def narrow_chunk(T):
    return 256 if T >= 65536 else (128 if T >= 8192 else 32)


def narrow_linear_backward(dy, x, w, mode, mutant=None):
    """narrow_linear_dx_kernel, narrow_linear_dw_kernel: dy (T, n), x (T, 256) bf16 values, w (n, 256) f32 -> (dx after its bf16 store, dw, db,
    dx before the store).  dx: an fma chain over j.  dw / db: a workgroup's chain over its chunk's tokens in order (fma / add), then the
    float32 atomics of the workgroups in an unknown order."""
    T, n = dy.shape
    dt = torch.float64 if mode.bounded or mode.dtype == torch.float64 else torch.float32
    DY, X, Wt = dy.to(dt), x.to(dt), w.to(dt)
    acc = mode.lift(torch.zeros(T, 256))
    for j in range(n):
        acc = _fma(DY[:, j:j + 1], Wt[j][None, :], acc)
    chunk = narrow_chunk(T)
    nw = (T + chunk - 1) // chunk
    pad = nw * chunk - T
    DYp = torch.cat((DY, torch.zeros(pad, n, dtype=dt))).reshape(nw, chunk, n)
    Xp = torch.cat((X, torch.zeros(pad, 256, dtype=dt))).reshape(nw, chunk, 256)
    if mutant == "dw_last_token" and T % 8 == 1:
        last = torch.full((nw,), chunk - 1)
        last[-1] = (T - 1) % chunk
        Xp = Xp.clone()
        Xp[torch.arange(nw), last] = 0.0
    aw, ab = mode.lift(torch.zeros(nw, n, 256)), mode.lift(torch.zeros(nw, n))
    for t in range(chunk):
        aw = _fma(DYp[:, t, :, None], Xp[:, t, None, :], aw)
        ab = ab + _like(DYp[:, t, :], ab)
    dw, db = _sum(aw, 0, nw - 1, mode), _sum(ab, 0, nw - 1, mode)      # (the first atomic adds to an exact 0)
    if mutant == "db_column0":
        db = _stack([db[0]] * n, 0)
    return store_bf16(acc), dw, db, acc


def narrow_inputs(T, n, seed=0):
    """x: bf16 ReLU outputs of N(0, 1) (the box head's hidden layer), dy bf16 N(0, 1), w N(0, 1) / 16"""
    g = torch.Generator().manual_seed(1000 + T + n + seed)
    x = bf(torch.randn(T, 256, generator=g).clamp(min=0))
    dy = bf(torch.randn(T, n, generator=g))
    w = torch.randn(n, 256, generator=g) / 16
    return dy, x, w


def narrow_exact_inputs(T, n, seed=0):
    """small integers in [-2, 2] and a dyadic weight (multiples of 1/4 in [-1, 1]): every product and every partial sum in any order is an
    exact float32 (|dw| <= 4 T < 2^24), every dx (n <= 8 terms of at most 2, multiples of 1/4: at most 64 steps, 7 bits) an exact bf16"""
    g = torch.Generator().manual_seed(2000 + T + n + seed)
    x = torch.randint(-2, 3, (T, 256), generator=g).float()
    dy = torch.randint(-2, 3, (T, n), generator=g).float()
    w = torch.randint(-4, 5, (n, 256), generator=g).float() / 4
    return dy, x, w


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(1, 1, 8), (3, 63, 64), (2, 2048, 8), (2, 2049, 8), (1, 131080, 8), (2, 1050, 256)]
GN_SETS = [(0.5, 2.0), (8.0, 1.0), (32.0, 1.0), (48.0, 1.0), "const"]
GN_SETS_CPU = GN_SETS + [(64.0, 1.0), (100.0, 0.5)]      # two more offset groups for wrong variant (l)
GN_EPS = 1e-5


def gn_partition(HW):
    """-> (strips, trips, depth of the forward sums, depth of the backward sums) as the launches cut the pixels"""
    strips = min((HW + 2047) // 2048, 64)
    trips = -(-HW // (strips * 256))
    return strips, trips, 4 * trips + 1 + 8 + strips, trips + 6


def gn_inputs(N, HW, C, mean_std, seed=0):
    """x (N, HW, C) bf16 values N(mean, std) per group (or the constant 3), gamma U(0.5, 1.5), beta N(0, 1), dy bf16 N(0, 1)"""
    g = torch.Generator().manual_seed(5 + HW + C + seed)
    if mean_std == "const":
        x = torch.full((N, HW, C), 3.0)
        if C > 8:
            x[:, :, 8:] = bf(torch.randn(N, HW, C - 8, generator=g) * 2 + 0.5)
    else:
        x = bf(torch.randn(N, HW, C, generator=g) * mean_std[1] + mean_std[0])
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dy = bf(torch.randn(N, HW, C, generator=g))
    return x, gamma, beta, dy


def _gn_partition_sum_f32(t, strips_level="f32"):
    """sum over the pixels and the 8 channels of t (N, HW, G, 8) float32 as gn8_stats_kernel partitions it: a thread's trips (four pair sums
    per trip, in order), the 8 tree levels; then the strips in float32 (F32 mode) or in float64 (the kernel's atomics): -> (N, G)"""
    N, HW, G, _ = t.shape
    strips, trips, _, _ = gn_partition(HW)
    S = strips * 256
    tp = torch.cat((t, torch.zeros(N, trips * S - HW, G, 8, dtype=t.dtype)), 1).reshape(N, trips, S, G, 8)
    s = torch.zeros(N, S, G, dtype=t.dtype)
    for k in range(trips):
        for e in range(4):
            s = s + (tp[:, k, :, :, 2 * e] + tp[:, k, :, :, 2 * e + 1])
    s = s.reshape(N, strips, 256, G)
    o = 128
    while o > 0:
        s = s[:, :, :o] + s[:, :, o:2 * o]
        o //= 2
    s = s[:, :, 0]
    if strips_level == "f64":
        return s.double().sum(1)
    r = s[:, 0]
    for i in range(1, strips):
        r = r + s[:, i]
    return r


def group_norm(x, gamma, beta, eps, mode, dy=None, mutant=None):
    """GroupNorm with 8 channels per group in the order of the definition: x (N, HW, C) bf16 values -> dict out (float32), out_bf16, and with
    dy: dx (after its bf16 store), dx32, dgamma, dbeta.  F32: the float32 two-pass evaluation with the kernel's partition of the sums."""
    N, HW, C = x.shape
    G = C // 8
    cnt = float(HW * 8)
    strips, trips, depth, depth_b = gn_partition(HW)
    x4 = x.reshape(N, HW, G, 8)
    if mode is F32:
        X = x4.float()
        mean = _gn_partition_sum_f32(X) / np.float32(cnt)
        d = X - mean[:, None, :, None]
        var = _gn_partition_sum_f32(d * d) / np.float32(cnt)
        rstd = torch.rsqrt(var + np.float32(eps))
        Gm, Bt = gamma.float().reshape(G, 8), beta.float().reshape(G, 8)
    elif not mode.bounded:
        X = x4.double()
        if mutant == "ex2_f32_partials":
            s1 = _gn_partition_sum_f32(x4.float(), "f64") / cnt
            var = (_gn_partition_sum_f32(x4.float() * x4.float(), "f64") / cnt - s1 * s1).clamp(min=0)
            mean = s1.float().double()
        else:
            mean = X.mean((1, 3))
            var = ((X - mean[:, None, :, None]) ** 2).mean((1, 3))
        d = X - mean[:, None, :, None]
        rstd = torch.rsqrt(var + (mode.c(eps) if mode.f32_consts else eps))
        Gm, Bt = gamma.double().reshape(G, 8), beta.double().reshape(G, 8)
    else:
        X = mode.lift(x4)
        u = mode.u
        mv = X.v.sum((1, 3)) / cnt
        e_mean = depth * u * X.v.abs().sum((1, 3)) / cnt + u * mv.abs()
        # a constant group whose partial sums c k (k <= cnt) are all float32 numbers: every sum is exact, so is the mean
        c0 = X.v[:, :1, :, :1]
        const = (X.v == c0).all(3).all(1)
        odd = c0[:, 0, :, 0].abs()
        odd = torch.where(odd > 0, odd / torch.exp2(torch.floor(torch.log2(odd.clamp(min=1e-300))) - 7.0), odd)      # an 8-bit integer ...
        for _ in range(8):                                                                                           # ... without its trailing zeros
            odd = torch.where((odd > 0) & (odd % 2 == 0), odd / 2, odd)
        e_mean = torch.where(const & (odd * cnt < 2.0 ** 24), torch.zeros_like(e_mean), e_mean)
        mean = B(mv, e_mean, mode)
        d = X - mean[:, None, :, None]
        var = _sum(d * d, (1, 3), depth, mode) / cnt
        rstd = _rsqrt(var + mode.c(eps))
        Gm, Bt = mode.lift(gamma.reshape(G, 8)), mode.lift(beta.reshape(G, 8))
    xhat = d * rstd[:, None, :, None]
    out = xhat * Gm[None, None] + Bt[None, None]
    res = {"out": _reshape(out, N, HW, C), "out_bf16": _reshape(store_bf16(out), N, HW, C)}
    if dy is None:
        return res
    DY = mode.lift(dy.reshape(N, HW, G, 8)) if mode.bounded else dy.reshape(N, HW, G, 8).to(_v(out).dtype)
    s_dy, s_dyx = _sum(DY, 1, depth_b, mode), _sum(DY * xhat, 1, depth_b, mode)      # (N, G, 8)
    if mode.bounded:      # A, B in float64: the products and sums add nothing visible
        A = B((Gm.v[None] * s_dy.v).sum(-1), (Gm.v.abs()[None] * s_dy.e).sum(-1), mode)
        Bq = B((Gm.v[None] * s_dyx.v).sum(-1), (Gm.v.abs()[None] * s_dyx.e).sum(-1), mode)
        a, b = _to_f32(B(A.v / cnt, A.e / cnt, mode), mode), _to_f32(B(Bq.v / cnt, Bq.e / cnt, mode), mode)
        dgamma = _to_f32(B(s_dyx.v.sum(0), s_dyx.e.sum(0), mode), mode)
        dbeta = _to_f32(B(s_dy.v.sum(0), s_dy.e.sum(0), mode), mode)
    else:
        a = ((Gm[None].double() * s_dy.double()).sum(-1) / cnt).to(s_dy.dtype)
        b = ((Gm[None].double() * s_dyx.double()).sum(-1) / cnt).to(s_dy.dtype)
        dgamma, dbeta = s_dyx.double().sum(0).to(s_dy.dtype), s_dy.double().sum(0).to(s_dy.dtype)
    bterm = xhat * b[:, None, :, None]
    if mutant == "dx_b_term_dropped":
        bterm = _where(_v(xhat).abs() < 2.0 ** -6, 0.0, bterm)
    dx = rstd[:, None, :, None] * (Gm[None, None] * DY - a[:, None, :, None] - bterm)
    res.update(dx=_reshape(store_bf16(dx), N, HW, C), dx32=_reshape(dx, N, HW, C), dgamma=_reshape(dgamma, C), dbeta=_reshape(dbeta, C))
    return res


def gn_torch_f64(x, gamma, beta, eps, dy):
    """F.group_norm in float64 with autograd: -> (out, dx, dgamma, dbeta), NHWC-flattened like the kernels' tensors"""
    N, HW, C = x.shape
    xr = x.double().clone().requires_grad_(True)
    g, b = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    out = torch.nn.functional.group_norm(xr.permute(0, 2, 1), C // 8, g, b, eps).permute(0, 2, 1)
    out.backward(dy.double())
    return out.detach(), xr.grad, g.grad, b.grad


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------------------
def avg_pool(x, k, mode, mutant=None):
    """pool_nhwc_kernel<false>: x (N, H, W, C) bf16 values, stride k, no padding: the k k taps added in order (kh, then kw) in float32, times
    the float32 reciprocal 1 / (k k), one bf16 store -> (stored, before the store)"""
    N, H, W, C = x.shape
    Ho, Wo = (H - k) // k + 1, (W - k) // k + 1
    X = mode.lift(x)
    acc = None
    for kh in range(k):
        for kw in range(k):
            t = X[:, kh:kh + (Ho - 1) * k + 1:k, kw:kw + (Wo - 1) * k + 1:k]
            acc = (t + 0.0) if acc is None else acc + t
    if mode is F64:
        r = acc / float(k * k)
    else:
        sc = _f32(1.0 / np.float32(k * k))
        if mutant == "avg_bf16_reciprocal":
            sc = float(bf(torch.tensor(sc)))
        r = acc * sc
    return store_bf16(r), r


def pool_inputs(N, H, W, C, seed=0, dyadic=False):
    g = torch.Generator().manual_seed(40 + H * 31 + W + C + seed)
    if dyadic:
        return torch.randint(-8, 9, (N, H, W, C), generator=g).float() / 4
    return bf(torch.randn(N, H, W, C, generator=g))


# ---- the older whole-tensor criteria (the table of the issue; profiles/r26_row_bounds.md) ---------------------------------------------------------
def _maxnorm(got, want, rel):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    return float((got - want).abs().max()) <= rel * float(want.abs().max())


def old_prep(got, want):
    """tests/test_gpu_module.py (f32): max-norm 2e-6 on the forward's tensors, 2e-4 on the gradients -- applied here to the prep kernels' own
    outputs, which that test sees only through the operator"""
    return all(_maxnorm(got[k], want[k], 2e-6 if k in ("loc", "aw") else 2e-4) for k in got)


def old_box(got, want):
    """tests/test_gpu_layers.py::test_refine_boxes_kernel_matches_the_op_sequence (f32): y 2e-6 absolute, grad_delta 2e-6 max(1, largest),
    grad_ref 2e-5 of its largest element"""
    ok = float((got["y"].double() - want["y"].double()).abs().max()) < 2e-6
    gd, wd = got["grad_delta"].double(), want["grad_delta"].double()
    ok = ok and float((gd - wd).abs().max()) <= 2e-6 * max(1.0, float(wd.abs().max()))
    return ok and _maxnorm(got["grad_ref"], want["grad_ref"], 2e-5)


def old_box_inputs():
    """that test's inputs (its recipe on the CPU generator)"""
    g = torch.Generator().manual_seed(9)
    ref = torch.rand(2, 300, 4, generator=g)
    ref[0, :5] = torch.tensor([0.0, 1.0, 1e-4, 1 - 1e-4])
    ref[1, 0] = torch.tensor([-0.1, 1.2, 0.5, 0.5])
    delta = torch.randn(2, 300, 4, generator=g)
    gy = torch.randn(2, 300, 4, generator=g)
    return delta.reshape(-1), ref.reshape(-1), gy.reshape(-1)


def old_sine(got, want):
    """tests/test_gpu_layers.py::test_sine_embed_kernel_matches_the_mirror: 2^-8 + 1e-5 absolute"""
    return float((torch.as_tensor(got).double() - torch.as_tensor(want).double()).abs().max()) <= 2.0 ** -8 + 1e-5


def old_narrow(got, want):
    """tests/test_gpu_layers.py::test_narrow_linear_function_matches_autograd: dx 2^-7, dw and db 1e-3 of the largest element"""
    return _maxnorm(got["dx"], want["dx"], 2.0 ** -7) and _maxnorm(got["dw"], want["dw"], 1e-3) and _maxnorm(got["db"], want["db"], 1e-3)


def old_gn(got, want):
    """tests/test_gpu_conv.py::test_group_norm_kernel and tests/test_gpu_backbone.py::test_group_norm8_function_matches_autograd: out_f32 2e-5,
    out_bf16 2^-8, dx 2^-7, dgamma / dbeta 2e-4 of the largest element"""
    tol = {"out": 2e-5, "out_bf16": 2.0 ** -8, "dx": 2.0 ** -7, "dgamma": 2e-4, "dbeta": 2e-4}
    return all(_maxnorm(got[k], want[k], tol[k]) for k in tol if k in got)


def old_pool(got, want):
    """tests/test_gpu_conv.py::test_pooling_kernels: 2^-8 of the largest element"""
    return _maxnorm(got, want, 2.0 ** -8)


def vals(x):
    """the values of a B or a tensor, float64"""
    return x.v if isinstance(x, B) else torch.as_tensor(x).double()


@functools.lru_cache(maxsize=None)
def gn_case(N, HW, C, set_index, mode_name="b32"):
    x, gamma, beta, dy = gn_inputs(N, HW, C, GN_SETS_CPU[set_index])
    return x, gamma, beta, dy, group_norm(x, gamma, beta, GN_EPS, {"b32": B32, "f32": F32, "f64": F64}[mode_name], dy=dy)
