"""tests/rows_ref.py on the CPU: (1) a float32 evaluation of every restatement stays inside its bound on every input set of
tests/test_gpu_rows_bounds.py, no element left out; (2) the bounds say something (median bound / |reference| below 1e-3 for float32
outputs); (3) the float64 restatement is the op sequence the library mirrors (torch float64, autograd for the gradients), to 1e-12;
(4) every wrong variant leaves its bound, and the older whole-tensor criterion gives the recorded verdict on the older test's own inputs.
``RICHSEM_REPORT=1`` prints the figures of profiles/r26_row_bounds.md."""
import os

import pytest
import torch
import torch.nn.functional as F

import rows_ref as R

REPORT = os.environ.get("RICHSEM_REPORT") == "1"


def _inside(name, got, ref, tight=True):
    r = R.ratio(got, ref)
    t = R.tightness(ref)
    if REPORT:
        print(f"[measured] cpu f32 {name}: ratio {r:.3g} median bound/|ref| {t:.3g}")
    assert r <= 1.0, (name, r)
    if tight:
        assert t < 1e-3, (name, t)
    return r


def _rel(name, a, b, rel=1e-12, scale=None):
    a, b = R.vals(a), R.vals(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    tol = rel * (b.abs() if scale is None else b.abs() + scale)
    assert bool(((a - b).abs() <= tol).all()), (name, float(((a - b).abs() - tol).max()))


# ---- prep ----------------------------------------------------------------------------------------------------------------------------------------
PREP_CASES = [(L, P, M, rd) for (L, P) in R.PREP_LP for M in (1, 3, 8) for rd in (2, 4)]


def _shapes(L, rd):
    return R.PREP_SHAPES[:L] if rd == 2 else [(1, 1)] * L


@pytest.mark.parametrize("L,P,M,rd", PREP_CASES)
@pytest.mark.parametrize("bf16_proj", [False, True])
def test_prep_float32_inside_the_bounds(L, P, M, rd, bf16_proj):
    off, log, ref, gl, ga = R.prep_inputs(L, P, M, rd, bf16_proj=bf16_proj)
    sh = _shapes(L, rd)
    loc_b, aw_b = R.prep_forward(off, log, ref, sh, R.B32)
    loc, aw = R.prep_forward(off, log, ref, sh, R.F32)
    tag = f"prep {'bf16' if bf16_proj else 'f32'} L{L} P{P} M{M} rd{rd}"
    _inside(tag + " loc", loc, loc_b)
    _inside(tag + " aw", aw, aw_b)
    got = R.prep_backward(gl, ga, aw, off, ref, sh, R.F32, bf16_proj=bf16_proj)
    want = R.prep_backward(gl, ga, aw, off, ref, sh, R.B32, bf16_proj=bf16_proj)
    _inside(tag + " grad_offsets", got[0], want[0], tight=not bf16_proj)
    _inside(tag + " grad_logits", got[1], want[1], tight=not bf16_proj)
    _inside(tag + " grad_ref", got[2], want[2])
    if bf16_proj:
        assert R.bf16_outside(got[0], want[3]) == 0 and R.bf16_outside(got[1], want[4]) == 0


@pytest.mark.parametrize("L,P,M,rd", [(4, 4, 8, 2), (3, 3, 3, 4), (4, 9, 1, 4), (1, 1, 3, 2)])
def test_prep_float64_is_the_module_op_sequence(L, P, M, rd):
    off, log, ref, gl, ga = R.prep_inputs(L, P, M, rd, dtype=torch.float64)
    sh = _shapes(L, rd)
    loc, aw = R.prep_forward(off, log, ref, sh, R.F64)
    t_loc, t_aw, t_go, t_gx, t_gr = R.prep_torch_f64(off, log, ref, sh, gl, ga)
    _rel("loc", loc, t_loc)
    _rel("aw", aw, t_aw)
    goff, glog, gref = R.prep_backward(gl, ga, aw, off, ref, sh, R.F64)
    _rel("grad_offsets", goff, t_go)
    _rel("grad_logits", glog, t_gx, scale=float(t_gx.abs().max()) * 1e-3)      # a (g - dot) cancels: conditioned by |a g| + |a dot|
    _rel("grad_ref", gref, t_gr, scale=float(gl.abs().max()))                  # a sum of M P terms of either sign


@pytest.mark.parametrize("rd", [2, 4])
@pytest.mark.parametrize("mode,dt", [(R.B32, torch.float32)])
def test_prep_probes_are_exact_by_the_count(rd, mode, dt):
    """the GPU file's bit-equal probes have bound 0 (the hot and the uniform lanes of aw are compared with their closed forms there)"""
    off, log, ref, aw, gl, ga = R.prep_probe_inputs(rd, dt)
    sh = R.PREP_SHAPES_POW2 if rd == 2 else [(1, 1)] * 4
    loc, _ = R.prep_forward(off, log, ref, sh, mode)
    assert float(loc.e.max()) == 0.0
    want = R.prep_backward(gl, ga, aw, off, ref, sh, mode)
    assert max(float(w.e.max()) for w in want) == 0.0
    assert torch.equal(want[1].v.reshape(-1, 16)[1::2, 5], torch.zeros(want[1].v.numel() // 32, dtype=torch.float64))


# ---- box refine ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.BOX_N)
@pytest.mark.parametrize("bf16_delta", [False, True])
def test_box_refine_float32_inside_the_bounds(n, bf16_delta):
    delta, ref, gy = R.box_inputs(n, bf16_delta)
    y_b = R.box_refine(delta, ref, R.EPS_BOX, R.B32)
    y = R.box_refine(delta, ref, R.EPS_BOX, R.F32)
    tag = f"box_refine n{n} {'bf16' if bf16_delta else 'f32'}"
    _inside(tag + " y", y, y_b)
    gd, gr, _ = R.box_refine_grad(gy, y, ref, R.EPS_BOX, R.F32, bf16_delta)
    gd_b, gr_b, gd32 = R.box_refine_grad(gy, y, ref, R.EPS_BOX, R.B32, bf16_delta)
    _inside(tag + " grad_delta", gd, gd_b, tight=not bf16_delta)
    _inside(tag + " grad_ref", gr, gr_b)
    if bf16_delta:
        assert R.bf16_outside(gd, gd32) == 0


def test_box_refine_float64_is_torch_autograd_with_its_clamp_gradients():
    delta, ref, gy = R.box_inputs(257)
    y = R.box_refine(delta.double(), ref.double(), R.EPS_BOX, R.F64)
    gd, gr, _ = R.box_refine_grad(gy.double(), y, ref.double(), R.EPS_BOX, R.F64)
    t_y, t_gd, t_gr = R.box_torch_f64(delta, ref, R.EPS_BOX, gy)
    _rel("y", y, t_y)
    _rel("grad_delta", gd, t_gd)
    _rel("grad_ref", gr, t_gr)
    k = len(R.BOX_EXPLICIT_REF)
    assert int((t_gr[:k] == 0).sum()) == 4      # below 0 (two values) and above 1 (two values): the explicit set reaches the blocked side


# ---- sine embed ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,dims,pe_dim", [(1, 2, 128), (137, 2, 128), (137, 4, 128), (4097, 4, 128), (137, 4, 2), (137, 2, 2)])
def test_sine_embed_float32_inside_the_bounds(tokens, dims, pe_dim):
    b = R.sine_inputs(tokens, dims)
    want = R.sine_embed(b, pe_dim, R.B32)
    got = R.sine_embed(b, pe_dim, R.F32)
    tag = f"sine_embed t{tokens} d{dims} pe{pe_dim}"
    _inside(tag + " f32", got, want)
    assert R.ratio(R.bf(got), R.store_bf16(want)) <= 1.0 and R.bf16_outside(R.bf(got), want) == 0
    _rel(tag, R.sine_embed(b.double(), pe_dim, R.F64), R.sine_torch_f64(b, pe_dim), scale=2 * torch.pi)      # |sin'| <= 1: conditioned by the phase


# ---- narrow linear -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n", [(33, 1), (33, 4), (33, 8), (8192, 4), (8192, 8)])
def test_narrow_linear_float32_inside_the_bounds(T, n):
    dy, x, w = R.narrow_inputs(T, n)
    want = R.narrow_linear_backward(dy, x, w, R.B32)
    got = R.narrow_linear_backward(dy, x, w, R.F32)
    tag = f"narrow_linear T{T} n{n}"
    _inside(tag + " dx", got[0], want[0], tight=False)
    assert R.bf16_outside(got[0], want[3]) == 0
    _inside(tag + " dx32", got[3], want[3])
    _inside(tag + " dw", got[1], want[1])
    _inside(tag + " db", got[2], want[2])
    f = R.narrow_linear_backward(dy.double(), x.double(), w.double(), R.F64)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), torch.zeros(n, dtype=torch.float64, requires_grad=True)
    F.linear(xr, wr, br).backward(dy.double())
    _rel("dx", f[3], xr.grad, scale=float(xr.grad.abs().max()) * 1e-3)
    _rel("dw", f[1], wr.grad, scale=float(wr.grad.abs().max()))
    _rel("db", f[2], br.grad, scale=float(br.grad.abs().max()))


@pytest.mark.parametrize("T", R.NARROW_T)
def test_narrow_linear_exact_inputs_have_bound_zero_results(T):
    """the whole-tensor exact probe of the GPU file is exact in float32 whatever the order: the restatement in float32 and in float64 agree
    bit for bit, dx is a bf16 number"""
    dy, x, w = R.narrow_exact_inputs(T, 4)
    a = R.narrow_linear_backward(dy, x, w, R.F32)
    b = R.narrow_linear_backward(dy.double(), x.double(), w.double(), R.F64)
    for i in (1, 2, 3):
        assert torch.equal(a[i].double(), b[i])
    assert torch.equal(R.bf(a[3]), a[3])


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GN_SHAPES)
@pytest.mark.parametrize("si", range(len(R.GN_SETS)))
def test_group_norm_float32_two_pass_inside_the_bounds(shape, si):
    x, gamma, beta, dy, want = R.gn_case(*shape, si)
    got = R.group_norm(x, gamma, beta, R.GN_EPS, R.F32, dy=dy)
    tag = f"group_norm {shape} set {R.GN_SETS[si]}"
    # (tightness is asserted on the (0.5, 2) set: the bound rightly grows with n u |mean| / std, 105 * 2^-24 * 48 = 3e-4 on the (48, 1) set)
    tight = si == 0 and shape[1] > 1
    _inside(tag + " out_f32", got["out"], want["out"], tight=tight)
    _inside(tag + " out_bf16", got["out_bf16"], want["out_bf16"], tight=False)
    assert R.bf16_outside(got["out_bf16"], want["out"]) == 0
    _inside(tag + " dx32", got["dx32"], want["dx32"], tight=tight)
    _inside(tag + " dx", got["dx"], want["dx"], tight=False)
    assert R.bf16_outside(got["dx"], want["dx32"]) == 0
    _inside(tag + " dgamma", got["dgamma"], want["dgamma"], tight=tight and shape[1] * shape[0] < 4096)
    _inside(tag + " dbeta", got["dbeta"], want["dbeta"], tight=tight and shape[1] * shape[0] < 4096)
    if R.GN_SETS[si] == "const":      # variance 0: xhat is exactly 0 and the result exactly beta, bound 0
        assert float(want["out"].e[:, :, :8].max()) == 0.0 and torch.equal(want["out"].v[:, :, :8], beta[:8].double().expand(shape[0], shape[1], 8))


def test_group_norm_bound_has_no_mean_squared_term():
    """the same group shifted by 8, 32, 48: the bound of out_f32 grows like |mean| / std, not like mean^2 / var"""
    e = []
    for si in (1, 2, 3):
        want = R.gn_case(2, 1050, 256, si)[4]
        e.append(float(want["out"].e.median()))
    assert e[1] / e[0] < 1.5 * 32 / 8 and e[2] / e[0] < 1.5 * 48 / 8, e


@pytest.mark.parametrize("shape,si", [((3, 63, 64), 0), ((2, 2049, 8), 2), ((1, 1, 8), 0), ((2, 1050, 256), 4)])
def test_group_norm_float64_is_torch_group_norm(shape, si):
    x, gamma, beta, dy = R.gn_inputs(*shape, R.GN_SETS[si])
    got = R.group_norm(x, gamma, beta, R.GN_EPS, R.F64, dy=dy)
    out, dx, dg, db = R.gn_torch_f64(x, gamma, beta, R.GN_EPS, dy)
    # xhat = (x - mean) rstd is conditioned by |x| + |mean|; the gradients' sums by their terms
    _rel("out", got["out"], out, scale=float(x.abs().max()))
    _rel("dx", got["dx32"], dx, scale=float(dx.abs().max()) + float(x.abs().max()))
    _rel("dgamma", got["dgamma"], dg, scale=float(dy.abs().sum(1).max()) * float(x.abs().max()))
    _rel("dbeta", got["dbeta"], db, scale=float(dy.abs().sum(1).max()))


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,H,W", [(2, 7, 9), (3, 7, 8), (7, 15, 20), (3, 3, 3)])
def test_avg_pool_float32_inside_the_bounds(k, H, W):
    x = R.pool_inputs(2, H, W, 16)
    want, want32 = R.avg_pool(x, k, R.B32)
    got, got32 = R.avg_pool(x, k, R.F32)
    _inside(f"avg_pool k{k} {H}x{W} f32", got32, want32)
    _inside(f"avg_pool k{k} {H}x{W} bf16", got, want, tight=False)
    assert R.bf16_outside(got, want32) == 0
    ref = F.avg_pool2d(x.double().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1)
    _rel("avg_pool", R.avg_pool(x.double(), k, R.F64)[1], ref, scale=float(x.abs().max()))


def test_avg_pool_of_two_on_dyadic_inputs_has_bound_zero():
    x = R.pool_inputs(1, 6, 6, 8, dyadic=True)
    want, want32 = R.avg_pool(x, 2, R.B32)
    assert float(want32.e.max()) == 0.0
    assert torch.equal(R.bf(want32.v.float()).double(), want32.v)      # ... and is a bf16 number: the store is exact


# ---- the wrong variants --------------------------------------------------------------------------------------------------------------------------
def _prep_mut(name):
    fwd = name in ("ly_with_rw", "pad_lanes_in_sum")
    L, P, M, rd = (3, 3, 3, 4)
    out = []
    for old in (False, True):
        if old:      # the module test's geometry: L = P = 4, M = 8, random rows only
            L, P, M = 4, 4, 8
        off, log, ref, gl, ga = R.prep_inputs(L, P, M, rd, special=not old)
        sh = _shapes(L, rd)
        loc_b, aw_b = R.prep_forward(off, log, ref, sh, R.B32)
        if fwd:
            loc, aw = R.prep_forward(off.double(), log.double(), ref.double(), sh, R.F64K, mutant=name)
            got, want = {"loc": loc, "aw": aw}, {"loc": loc_b, "aw": aw_b}
        else:
            aw = aw_b.v.float()
            w = R.prep_backward(gl, ga, aw, off, ref, sh, R.B32)
            g = R.prep_backward(gl.double(), ga.double(), aw.double(), off.double(), ref.double(), sh, R.F64K, mutant=name)
            got, want = dict(zip(("goff", "glog", "gref"), g)), dict(zip(("goff", "glog", "gref"), w))
        if old:
            out.append(R.old_prep(got, {k: v.v for k, v in want.items()}))
        else:
            out.append(max(R.ratio(got[k], want[k]) for k in got))
    return out


def _box_mut(name):
    out = []
    for old in (False, True):
        delta, ref, gy = R.old_box_inputs() if old else R.box_inputs(257)
        y = R.box_refine(delta, ref, R.EPS_BOX, R.B32)
        y32 = y.v.float()
        gd_b, gr_b, _ = R.box_refine_grad(gy, y32, ref, R.EPS_BOX, R.B32)
        gd, gr, _ = R.box_refine_grad(gy.double(), y32.double(), ref.double(), R.EPS_BOX, R.F64K, mutant=name)
        if old:
            out.append(R.old_box({"y": y.v, "grad_delta": gd, "grad_ref": gr}, {"y": y.v, "grad_delta": gd_b.v, "grad_ref": gr_b.v}))
        else:
            out.append(max(R.ratio(gd, gd_b), R.ratio(gr, gr_b)))
    return out


def _sine_mut(name):
    b = R.sine_inputs(137, 4)
    want = R.sine_embed(b, 128, R.B32)
    got = R.sine_embed(b.double(), 128, R.F64K, mutant=name)
    g = torch.Generator().manual_seed(3)      # the older test's boxes: U(0, 1) only
    bo = torch.rand(2 * 137, 4, generator=g)
    old = R.old_sine(R.bf(R.sine_embed(bo.double(), 128, R.F64K, mutant=name).float()), R.sine_embed(bo.double(), 128, R.F64K))
    return R.ratio(got, want), old      # (held to the float32 bound before the store: the mutant is a float64 evaluation)


def _narrow_mut(name):
    dy, x, w = R.narrow_inputs(33, 4)
    want = R.narrow_linear_backward(dy, x, w, R.B32)
    got = R.narrow_linear_backward(dy.double(), x.double(), w.double(), R.F64K, mutant=name)
    r = max(R.ratio(got[1], want[1]), R.ratio(got[2], want[2]))
    g = torch.Generator().manual_seed(37)      # the older test's smallest T, its recipe
    xo, wo, dyo = R.bf(torch.randn(37, 256, generator=g)), torch.randn(4, 256, generator=g) / 16, R.bf(torch.randn(37, 4, generator=g))
    a = R.narrow_linear_backward(dyo.double(), xo.double(), wo.double(), R.F64K, mutant=name)
    b = R.narrow_linear_backward(dyo.double(), xo.double(), wo.double(), R.F64K)
    return r, R.old_narrow({"dx": a[3], "dw": a[1], "db": a[2]}, {"dx": b[3], "dw": b[1], "db": b[2]})


def _gn_mut(name):
    keys = ("out", "dx32", "dgamma", "dbeta")
    worst = {}
    for si in (0, 2, 3, 5, 6):
        x, gamma, beta, dy, want = R.gn_case(2, 1050, 256, si)
        got = R.group_norm(x, gamma, beta, R.GN_EPS, R.F64K, dy=dy, mutant=name)
        worst[si] = max(R.ratio(got[k], want[k]) for k in keys)
    x, gamma, beta, dy = R.gn_inputs(2, 240, 256, (0.5, 2.0), seed=1)      # the older tests' distribution, (2, 12, 20, 256)
    a = R.group_norm(x, gamma, beta, R.GN_EPS, R.F64K, dy=dy, mutant=name)
    b = R.group_norm(x, gamma, beta, R.GN_EPS, R.F64K, dy=dy)
    old = R.old_gn({"out": a["out"], "out_bf16": R.bf(a["out"].float()), "dx": R.bf(a["dx32"].float()), "dgamma": a["dgamma"], "dbeta": a["dbeta"]},
                   {"out": b["out"], "out_bf16": b["out"], "dx": b["dx32"], "dgamma": b["dgamma"], "dbeta": b["dbeta"]})
    return worst, old


def _pool_mut(name):
    x = R.pool_inputs(2, 7, 8, 16)
    _, want32 = R.avg_pool(x, 3, R.B32)
    _, got32 = R.avg_pool(x.double(), 3, R.F64K, mutant=name)
    torch.manual_seed(3)
    xo = R.bf(torch.randn(2, 9, 9, 8))
    old = R.old_pool(R.bf(R.avg_pool(xo.double(), 3, R.F64K, mutant=name)[1].float()), R.avg_pool(xo.double(), 3, R.F64)[1])
    return R.ratio(got32, want32), old


def _run_mutant(name, kernel):
    if kernel.startswith("prep"):
        return _prep_mut(name)
    if kernel == "box_refine":
        return _box_mut(name)
    if kernel == "sine_embed":
        return _sine_mut(name)
    if kernel == "narrow_linear":
        return _narrow_mut(name)
    if kernel == "avg_pool":
        return _pool_mut(name)
    raise AssertionError(kernel)


@pytest.mark.parametrize("name,kernel,what", [m for m in R.MUTANTS if m[1] != "group_norm"])
def test_wrong_variant_leaves_its_bound(name, kernel, what):
    r, old = _run_mutant(name, kernel)
    if REPORT:
        print(f"[measured] mutant {name}: ratio {r:.3g} old criterion passes {old}   {what}")
    assert r > 1.0, (name, r)
    assert old == R.OLD_CRITERION_PASSES[name], (name, old)


def test_parent_variance_order_leaves_the_bound_on_offset_groups_only():
    """(l): E[x^2] - mean^2 with float32 partials -- inside on N(0.5, 2), the older tests' only input, outside on the (32, 1), (48, 1), (64, 1) and (100, 0.5) sets
    (1.02, 1.75, 2.3 and 6.5 bounds at HW = 1050: the bound admits a float32 mean of the kernel's depth, 30 u |mean| / std)"""
    worst, old = _gn_mut("ex2_f32_partials")
    if REPORT:
        print(f"[measured] mutant ex2_f32_partials: ratio by set {worst} old criterion passes {old}")
    assert worst[0] <= 1.0 and worst[2] > 1.0 and worst[3] > 1.0 and worst[5] > 1.0 and worst[6] > 1.0, worst
    assert old == R.OLD_CRITERION_PASSES["ex2_f32_partials"]


def test_dropped_b_term_leaves_the_bound():
    worst, old = _gn_mut("dx_b_term_dropped")
    if REPORT:
        print(f"[measured] mutant dx_b_term_dropped: ratio by set {worst} old criterion passes {old}")
    assert worst[0] > 1.0, worst
    assert old == R.OLD_CRITERION_PASSES["dx_b_term_dropped"]


def test_average_pool_variant_as_first_proposed_is_a_no_op():
    """(n) as first proposed: dividing by k instead of k k where k = 1 -- the same number; avg_pool_nhwc(x, 1) returns x itself"""
    x = R.pool_inputs(1, 3, 3, 8)
    want, want32 = R.avg_pool(x, 1, R.B32)
    assert float(want32.e.max()) == 0.0 and torch.equal(want32.v, x.double())


def test_the_list_is_long_enough():
    assert len(R.MUTANTS) >= 10 and sum(R.OLD_CRITERION_PASSES[m[0]] for m in R.MUTANTS) >= 4
    assert R.OLD_CRITERION_PASSES["ex2_f32_partials"]
