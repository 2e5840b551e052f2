"""The prep, mask_rows, box-refine, sine-embed, narrow-linear, GroupNorm and pooling kernels against the element-wise bounds and exact probes
of tests/rows_ref.py (derivation: its docstring), through their wrappers -- ``refine_boxes``, ``sine_embed_bf16``, ``Lin256NarrowFunction``,
``group_norm8_nhwc`` / ``GroupNorm8Function``, ``avg_pool_nhwc`` / ``max_pool_nhwc``, ``mask_rows_`` -- and through ctypes on the C ABI where
a wrapper hides an output or an argument (``msda_prep_forward_* / msda_prep_backward_*`` in both row layouts, ``msda_box_refine_backward``,
``msda_narrow_linear_backward_bf16`` with dx / db NULL, ``msda_groupnorm8_backward_nhwc_bf16`` with dgamma / dbeta NULL).  One ``ratio``
per output: worst |kernel - restatement| / bound, <= 1 for f32 and <= 2 for f64; bf16 stores also inside the monotone rounding interval;
probes compare bits.  tests/test_rows_ref.py shows on the CPU that a float32 evaluation meets the same bounds on the same inputs and
that the wrong variants do not.  Measured figures: profiles/r26_row_bounds.md."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from richsem_amd import _lib

import rows_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPORT = os.environ.get("RICHSEM_REPORT") == "1"
SFX_DT = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}


def _r(name, got, ref, limit=1.0):
    r = R.ratio(got, ref)
    if REPORT:
        print(f"[measured] rows {name}: ratio {r:.3g}", flush=True)
    assert r <= limit, (name, r)
    return r


def _stored(name, got, ref32):
    """a bf16 output: inside the bound with the storage term and inside the monotone rounding interval of the float32 result"""
    _r(name, got.float(), R.store_bf16(ref32))
    assert R.bf16_outside(got, ref32) == 0, name


def _bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _p(t):
    return t.data_ptr() if t is not None else None


def _call(name, *args):
    with _lib.on_device(torch.device(DEV)):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.raw_stream(torch.device(DEV))))


# ---- prep forward / backward -----------------------------------------------------------------------------------------------------------------
def _shapes(L, rd, pow2=False):
    return (R.PREP_SHAPES_POW2 if pow2 else R.PREP_SHAPES)[:L]


def _prep_forward(sfx, off, log, ref, shapes, gemm_layout):
    """msda_prep_forward_<sfx> on host tensors -> (loc, aw) on the host.  ``gemm_layout``: offsets and logits inside ONE (N, Lq, 3 M L P)
    tensor (row stride 3 M L P), else two contiguous tensors"""
    N, Lq, M, L, P, _ = off.shape
    pt, wt = SFX_DT[sfx], torch.float32 if sfx == "bf16" else SFX_DT[sfx]
    n_off, n_log = M * L * P * 2, M * L * P
    if gemm_layout:
        q = torch.cat((off.reshape(N, Lq, n_off), log.reshape(N, Lq, n_log)), -1).to(pt).to(DEV).contiguous()
        o_ptr, l_ptr, so, sl = q.data_ptr(), q.data_ptr() + n_off * q.element_size(), n_off + n_log, n_off + n_log
    else:
        o, lg = off.to(pt).to(DEV).contiguous(), log.to(pt).to(DEV).contiguous()
        o_ptr, l_ptr, so, sl = o.data_ptr(), lg.data_ptr(), n_off, n_log
    r = ref.to(wt).to(DEV).contiguous()
    loc = torch.full((N, Lq, M, L, P, 2), float("nan"), dtype=wt, device=DEV)
    aw = torch.full((N, Lq, M, L, P), float("nan"), dtype=wt, device=DEV)
    sh = np.ascontiguousarray(np.array(shapes, dtype=np.int64))
    _call("msda_prep_forward_" + sfx, o_ptr, so, l_ptr, sl, r.data_ptr(), ref.shape[-1], sh.ctypes.data, N, Lq, M, L, P, loc.data_ptr(),
          aw.data_ptr())
    torch.cuda.synchronize()
    return loc.cpu(), aw.cpu()


def _prep_backward(sfx, gl, ga, aw, off, ref, shapes, gemm_layout, want_ref=True):
    """msda_prep_backward_<sfx> -> (grad_offsets, grad_logits, grad_ref) on the host (the projection gradients in the projection's type)"""
    N, Lq, M, L, P, _ = off.shape
    pt, wt = SFX_DT[sfx], torch.float32 if sfx == "bf16" else SFX_DT[sfx]
    n_off, n_log = M * L * P * 2, M * L * P
    esz = torch.empty(0, dtype=pt).element_size()
    if gemm_layout:
        q = torch.cat((off.reshape(N, Lq, n_off), torch.zeros(N, Lq, n_log, dtype=off.dtype)), -1).to(pt).to(DEV).contiguous()
        gq = torch.full((N, Lq, n_off + n_log), float("nan"), dtype=pt, device=DEV)
        o_ptr, so = q.data_ptr(), n_off + n_log
        go_ptr, gl_ptr, sgo, sgl = gq.data_ptr(), gq.data_ptr() + n_off * esz, n_off + n_log, n_off + n_log
    else:
        q = off.to(pt).to(DEV).contiguous()
        go_t = torch.full((N, Lq, n_off), float("nan"), dtype=pt, device=DEV)
        gl_t = torch.full((N, Lq, n_log), float("nan"), dtype=pt, device=DEV)
        o_ptr, so = q.data_ptr(), n_off
        go_ptr, gl_ptr, sgo, sgl = go_t.data_ptr(), gl_t.data_ptr(), n_off, n_log
    d = [t.to(wt).to(DEV).contiguous() for t in (gl, ga, aw, ref)]
    gref = torch.full(ref.shape, float("nan"), dtype=wt, device=DEV) if want_ref else None
    sh = np.ascontiguousarray(np.array(shapes, dtype=np.int64))
    _call("msda_prep_backward_" + sfx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), o_ptr, so, d[3].data_ptr(), ref.shape[-1], sh.ctypes.data,
          N, Lq, M, L, P, go_ptr, sgo, gl_ptr, sgl, ctypes.c_void_p(gref.data_ptr()) if want_ref else None)
    torch.cuda.synchronize()
    if gemm_layout:
        g = gq.cpu()
        goff, glog = g[..., :n_off], g[..., n_off:]
    else:
        goff, glog = go_t.cpu(), gl_t.cpu()
    return goff.reshape(N, Lq, M, L, P, 2), glog.reshape(N, Lq, M, L, P), (gref.cpu() if want_ref else None)


def _prep_check(tag, sfx, off, log, ref, gl, ga, shapes, gemm_layout):
    mode, limit = (R.B64, 2.0) if sfx == "f64" else (R.B32, 1.0)
    loc_b, aw_b = R.prep_forward(off, log, ref, shapes, mode)
    loc, aw = _prep_forward(sfx, off, log, ref, shapes, gemm_layout)
    _r(tag + " loc", loc, loc_b, limit)
    _r(tag + " aw", aw, aw_b, limit)
    want = R.prep_backward(gl, ga, aw, off, ref, shapes, mode, bf16_proj=sfx == "bf16")      # on the kernel's own aw
    goff, glog, gref = _prep_backward(sfx, gl, ga, aw, off, ref, shapes, gemm_layout)
    if sfx == "bf16":
        _stored(tag + " grad_offsets", goff, want[3])
        _stored(tag + " grad_logits", glog, want[4])
    else:
        _r(tag + " grad_offsets", goff, want[0], limit)
        _r(tag + " grad_logits", glog, want[1], limit)
    _r(tag + " grad_ref", gref, want[2], limit)


@pytest.mark.parametrize("L,P", R.PREP_LP)
@pytest.mark.parametrize("rd", [2, 4])
def test_prep_kernels_inside_the_bounds(L, P, rd):
    """N = 2, Lq = 37 (the last wave holds fewer groups than fit), M in {1, 3, 8}, f32 / f64 / bf16 projection, both row layouts"""
    for M in (1, 3, 8):
        for sfx in ("f32", "f64", "bf16"):
            off, log, ref, gl, ga = R.prep_inputs(L, P, M, rd, dtype=torch.float64 if sfx == "f64" else torch.float32, bf16_proj=sfx == "bf16")
            for gemm_layout in (True, False):
                _prep_check(f"prep_{sfx} L{L} P{P} M{M} rd{rd} {'gemm' if gemm_layout else 'separate'}", sfx, off, log, ref, gl, ga,
                            _shapes(L, rd), gemm_layout)


def test_prep_forward_beyond_the_grid_cap():
    """G = 64: 4 items per workgroup, 8192 workgroups: 33600 (n, q, m) items take a second sweep"""
    off, log, ref, gl, ga = R.prep_inputs(4, 16, 8, 2, N=2, Lq=2100)
    loc_b, aw_b = R.prep_forward(off, log, ref, _shapes(4, 2), R.B32)
    loc, aw = _prep_forward("f32", off, log, ref, _shapes(4, 2), True)
    _r("prep_f32 forward 33600 items loc", loc, loc_b)
    _r("prep_f32 forward 33600 items aw", aw, aw_b)


def test_prep_backward_beyond_the_grid_cap():
    """G = 64: 4 (n, q) rows per workgroup: 32800 rows take a second sweep"""
    off, log, ref, gl, ga = R.prep_inputs(4, 16, 1, 4, N=2, Lq=16400)
    aw = R.prep_forward(off, log, ref, _shapes(4, 4), R.F32)[1]
    want = R.prep_backward(gl, ga, aw, off, ref, _shapes(4, 4), R.B32)
    got = _prep_backward("f32", gl, ga, aw, off, ref, _shapes(4, 4), False)
    for k, name in enumerate(("grad_offsets", "grad_logits", "grad_ref")):
        _r("prep_f32 backward 32800 rows " + name, got[k], want[k])


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_prep_exact_probes(sfx):
    """bit-equal: uniform rows give 1 / (L P), one-hot rows 1 and 0, dyadic offsets on power-of-two levels exact locations; backward: a
    one-hot aw gives grad_logits 0 in the hot lane, a uniform aw with dyadic grad_aw its closed form, dyadic grad_loc exact sums"""
    dt = torch.float64 if sfx == "f64" else torch.float32
    mode = R.B64 if sfx == "f64" else R.B32
    L, P = 4, 4
    for rd in (2, 4):
        shapes = _shapes(L, rd, pow2=True)
        off, log, ref, aw_p, gl, ga = R.prep_probe_inputs(rd, dt)
        loc_b, aw_b = R.prep_forward(off, log, ref, shapes, mode)
        assert mode is R.B64 or float(loc_b.e.max()) == 0.0      # the probe is exact by the count (float32; in float64 a fortiori)
        for gemm_layout in (True, False):
            loc, aw = _prep_forward(sfx, off, log, ref, shapes, gemm_layout)
            assert torch.equal(_bits(loc), _bits(loc_b.v.to(dt))), (sfx, rd)
            a = aw.reshape(-1, L * P)
            assert torch.equal(_bits(a[0::2]), _bits(torch.full_like(a[0::2], 1.0 / (L * P))))
            hot = torch.zeros_like(a[1::2])
            hot[:, 5] = 1.0
            assert torch.equal(_bits(a[1::2]), _bits(hot))
        # backward on an aw that is one-hot in the odd rows and uniform in the even rows
        aw = aw_p
        want = R.prep_backward(gl, ga, aw, off, ref, shapes, mode)
        assert mode is R.B64 or max(float(w.e.max()) for w in want) == 0.0
        for gemm_layout in (True, False):
            got = _prep_backward(sfx, gl, ga, aw, off, ref, shapes, gemm_layout)
            st = (lambda v: v.float().to(torch.bfloat16).double()) if sfx == "bf16" else (lambda v: v)      # (one rounding of the exact value)
            for k in range(3):
                assert torch.equal(got[k].double(), st(want[k].v) if k < 2 else want[k].v), (sfx, rd, k)
            glog = got[1].reshape(-1, L * P)
            assert torch.equal(_bits(glog[1::2, 5]), torch.zeros_like(_bits(glog[1::2, 5])))
            gaf = ga.reshape(-1, L * P)[0::2].double()
            assert torch.equal(glog[0::2].double(), st((gaf - gaf.mean(1, keepdim=True)) / (L * P)))
            assert torch.equal(got[2][..., :2].double(), gl.double().sum((2, 4)))


# ---- mask_rows -------------------------------------------------------------------------------------------------------------------------------
def _masks(rows, g):
    m = {"none": torch.zeros(rows, dtype=torch.bool), "all": torch.ones(rows, dtype=torch.bool)}
    m["first"] = m["none"].clone()
    m["first"][0] = True
    m["last"] = m["none"].clone()
    m["last"][-1] = True
    m["every64"] = m["none"].clone()
    m["every64"][::64] = True
    m["random"] = torch.rand(rows, generator=g) < 0.1
    return m


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
def test_mask_rows_is_exact_and_touches_nothing_else(sfx):
    from richsem_amd.functions.fused import mask_rows_
    g = torch.Generator().manual_seed(12)
    dt = SFX_DT[sfx]
    guard = 64
    cases = [(rows, re) for rows in (1, 63, 64, 65, 1000) for re in (1, 3, 64, 65, 256)] + [(1048576 + 77, 3)]      # (beyond the 4096-workgroup sweep)
    for rows, re in cases:
        n = rows * re
        fill = torch.randn(n + 2 * guard, generator=g) - 0.5
        fill[::7], fill[3::11], fill[5::13], fill[1::5] = float("nan"), float("inf"), float("-inf"), -0.0
        fill = fill.to(dt).to(DEV)
        for name, mask in _masks(rows, g).items():
            buf = fill.clone()
            body = buf[guard: guard + n]
            mask_rows_(body, mask.to(DEV))
            want = _bits(fill).clone()
            want[guard: guard + n].reshape(rows, re)[mask.to(DEV)] = 0
            assert torch.equal(_bits(buf), want), (sfx, rows, re, name)


# ---- box refine ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.BOX_N)
@pytest.mark.parametrize("bf16_delta", [False, True])
def test_box_refine_kernels_inside_the_bounds(n, bf16_delta):
    from richsem_amd.modules.decoder import refine_boxes
    delta, ref, gy = R.box_inputs(n, bf16_delta)
    tag = f"box_refine n{n} {'bf16' if bf16_delta else 'f32'}"
    d = delta.to(torch.bfloat16 if bf16_delta else torch.float32).to(DEV).requires_grad_(True)
    r = ref.to(DEV).requires_grad_(True)
    y = refine_boxes(d, r, R.EPS_BOX)
    assert y.dtype == torch.float32
    _r(tag + " y", y.detach().cpu(), R.box_refine(delta, ref, R.EPS_BOX, R.B32))
    y.backward(gy.to(DEV))
    yk = y.detach().cpu()
    gd_b, gr_b, gd32 = R.box_refine_grad(gy, yk, ref, R.EPS_BOX, R.B32, bf16_delta)      # on the kernel's own y
    if bf16_delta:
        _stored(tag + " grad_delta", d.grad.cpu(), gd32)
    else:
        _r(tag + " grad_delta", d.grad.cpu(), gd_b)
    _r(tag + " grad_ref", r.grad.cpu(), gr_b)
    outside = (ref < 0) | (ref > 1)
    assert torch.equal(_bits(r.grad.cpu())[outside], torch.zeros(int(outside.sum()), dtype=torch.int32))
    # gy -> 4 gy scales every gradient bit-exactly; a reference without a gradient and msda_box_refine_backward give the same grad_delta
    d4, r4 = d.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
    refine_boxes(d4, r4, R.EPS_BOX).backward(4 * gy.to(DEV))
    assert torch.equal(_bits(d4.grad.float()), _bits(4 * d.grad.float())) and torch.equal(_bits(r4.grad), _bits(4 * r.grad))
    d0 = d.detach().clone().requires_grad_(True)
    refine_boxes(d0, r.detach(), R.EPS_BOX).backward(gy.to(DEV))
    assert torch.equal(_bits(d0.grad), _bits(d.grad))
    gdc = torch.full((n,), float("nan"), dtype=d.dtype, device=DEV)
    gyd = gy.to(DEV)
    _call("msda_box_refine_backward", gyd.data_ptr(), y.detach().data_ptr(), n, gdc.data_ptr(), int(bf16_delta))
    torch.cuda.synchronize()
    assert torch.equal(_bits(gdc), _bits(d.grad))


@pytest.mark.parametrize("bf16_delta", [False, True])
def test_box_refine_exact_probe(bf16_delta):
    """ref = 0.5, delta = 0: y = 0.5, grad_delta = gy / 4, grad_ref = gy, bit-equal"""
    from richsem_amd.modules.decoder import refine_boxes
    n = 300
    gy = (torch.randint(-64, 65, (n,)).float() / 16).to(DEV)
    d = torch.zeros(n, dtype=torch.bfloat16 if bf16_delta else torch.float32, device=DEV).requires_grad_(True)
    r = torch.full((n,), 0.5, device=DEV).requires_grad_(True)
    y = refine_boxes(d, r, R.EPS_BOX)
    y.backward(gy)
    assert torch.equal(_bits(y), _bits(torch.full_like(y, 0.5)))
    assert torch.equal(_bits(d.grad.float()), _bits(gy / 4)) and torch.equal(_bits(r.grad), _bits(gy))


# ---- sine embed ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tokens,dims,pe_dim", [(1, 2, 128), (137, 2, 128), (137, 4, 128), (4097, 4, 128), (137, 4, 2), (137, 2, 2)])
def test_sine_embed_inside_the_bounds(tokens, dims, pe_dim):
    """4097 tokens of 4 x 64 pairs: beyond the 4096-workgroup grid; contiguous boxes and the level-0 slice (ld = L * dims)"""
    from richsem_amd.modules.decoder import sine_embed_bf16
    b = R.sine_inputs(tokens, dims)
    want = R.sine_embed(b, pe_dim, R.B32)
    full = torch.rand(tokens, 4, dims).to(DEV)
    full[:, 0] = b.to(DEV)
    for name, boxes in (("contiguous", b.to(DEV)), ("level-0 slice", full[:, 0, :])):
        got = sine_embed_bf16(boxes, pe_dim)
        assert got.dtype == torch.bfloat16 and got.shape == (tokens, dims * pe_dim)
        _stored(f"sine_embed t{tokens} d{dims} pe{pe_dim} {name}", got.cpu(), want)


def test_sine_embed_probes():
    """a box of 0: sin = +0, cos = 1 in every channel, bit-equal; the block order (y, x, w, h): one non-zero coordinate at a time"""
    from richsem_amd.modules.decoder import sine_embed_bf16
    pe = 128
    boxes = torch.zeros(5, 4)
    for i in range(4):
        boxes[1 + i, i] = 0.25
    got = sine_embed_bf16(boxes.to(DEV), pe).cpu()
    zero = torch.stack((torch.zeros(pe // 2), torch.ones(pe // 2)), -1).reshape(pe).to(torch.bfloat16)
    assert torch.equal(_bits(got[0]), _bits(zero.repeat(4)))
    want = R.sine_embed(boxes, pe, R.B32)
    for i, block in enumerate((1, 0, 2, 3)):      # coordinate i (x, y, w, h) lands in block (y, x, w, h)
        row = got[1 + i].reshape(4, pe)
        for blk in range(4):
            if blk == block:
                assert not torch.equal(_bits(row[blk]), _bits(zero))
                _stored(f"sine_embed coordinate {i} block {blk}", row[blk], want[1 + i, blk * pe:(blk + 1) * pe])
            else:
                assert torch.equal(_bits(row[blk]), _bits(zero)), (i, blk)


# ---- narrow linear backward ----------------------------------------------------------------------------------------------------------------------
def _narrow(dy, x, w, want_dx=True, want_db=True):
    T, n = dy.shape
    d, xx, ww = dy.to(torch.bfloat16).to(DEV).contiguous(), x.to(torch.bfloat16).to(DEV).contiguous(), w.float().to(DEV).contiguous()
    dx = torch.full((T, 256), float("nan"), dtype=torch.bfloat16, device=DEV) if want_dx else None
    dw = torch.full((n, 256), float("nan"), device=DEV)
    db = torch.full((n,), float("nan"), device=DEV) if want_db else None
    _call("msda_narrow_linear_backward_bf16", d.data_ptr(), xx.data_ptr(), ww.data_ptr(), T, n, _p(dx), dw.data_ptr(), _p(db))
    torch.cuda.synchronize()
    return (dx.cpu() if want_dx else None), dw.cpu(), (db.cpu() if want_db else None)


@pytest.mark.parametrize("T", R.NARROW_T)
def test_narrow_linear_whole_tensor_exact_probe(T):
    """small integers and a dyadic weight: dw, db exact integers whatever order the atomics take, dx exact -- bit for bit, n in {1, 4, 8};
    with dx = NULL and db = NULL the remaining outputs keep their bits"""
    for n in (1, 4, 8):
        dy, x, w = R.narrow_exact_inputs(T, n)
        dx, dw, db = _narrow(dy, x, w)
        # (+ 0.0: the kernels' sums start from +0, so a zero result is +0 whatever the signs of its zero products)
        assert torch.equal(_bits(dw), _bits(dy.t() @ x + 0.0)), (T, n)
        assert torch.equal(_bits(db), _bits(dy.sum(0) + 0.0)), (T, n)
        assert torch.equal(_bits(dx), _bits((dy @ w + 0.0).to(torch.bfloat16))), (T, n)
        _, dw2, _ = _narrow(dy, x, w, want_dx=False, want_db=False)
        assert torch.equal(_bits(dw2), _bits(dw))


@pytest.mark.parametrize("T", [33, 8192, 65536 + 5])
def test_narrow_linear_single_token_probe(T):
    """one non-zero dy[t*, j]: dw[j] is the row x[t*], every other row of dw is 0 -- t* at the trip, chunk and tensor edges"""
    n, chunk = 4, R.narrow_chunk(T)
    _, x, w = R.narrow_inputs(T, n)
    for j, ts in enumerate(sorted({0, 7, 8, chunk - 1, chunk, T - 1})):
        if ts >= T:
            continue
        dy = torch.zeros(T, n)
        dy[ts, j % n] = 1.0
        _, dw, db = _narrow(dy, x, w, want_dx=False)
        want = torch.zeros(n, 256)
        want[j % n] = x[ts]
        assert torch.equal(_bits(dw), _bits(want)), (T, ts)
        assert torch.equal(db, dy.sum(0))


@pytest.mark.parametrize("T", [33, 8192])
def test_narrow_linear_inside_the_bounds(T):
    for n in (1, 4, 8):
        dy, x, w = R.narrow_inputs(T, n)
        want = R.narrow_linear_backward(dy, x, w, R.B32)
        dx, dw, db = _narrow(dy, x, w)
        tag = f"narrow_linear T{T} n{n}"
        _stored(tag + " dx", dx, want[3])
        _r(tag + " dw", dw, want[1])
        _r(tag + " db", db, want[2])


def test_narrow_linear_function_backward_inside_the_bounds():
    from richsem_amd.functions.linear import Lin256NarrowFunction, pack_linear256_padded
    T, n = 33, 4
    dy, x, w = R.narrow_inputs(T, n)
    xd = x.to(torch.bfloat16).to(DEV).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), torch.zeros(n, device=DEV, requires_grad=True)
    y = Lin256NarrowFunction.apply(xd, pack_linear256_padded(wd, bd), wd, bd)
    y.backward(dy.to(torch.bfloat16).to(DEV))
    want = R.narrow_linear_backward(dy, x, w, R.B32)
    _stored("Lin256NarrowFunction dx", xd.grad.cpu(), want[3])
    _r("Lin256NarrowFunction dw", wd.grad.cpu(), want[1])
    _r("Lin256NarrowFunction db", bd.grad.cpu(), want[2])


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GN_SHAPES)
@pytest.mark.parametrize("si", range(len(R.GN_SETS)))
def test_group_norm_inside_the_bounds(shape, si):
    """strips 1, 2 and the cap of 64; one group; one pixel; groups N(0.5, 2), offset groups (8, 1), (32, 1), (48, 1) and a constant group;
    out_f32 only, out_bf16 only, both; backward with dgamma / dbeta present (GroupNorm8Function) and NULL (ctypes)"""
    from richsem_amd.conv import GroupNorm8Function, _group_norm8, group_norm8_nhwc
    N, HW, C = shape
    x, gamma, beta, dy, want = R.gn_case(N, HW, C, si)
    tag = f"group_norm {shape} set {R.GN_SETS[si]}"
    xd = x.to(torch.bfloat16).reshape(N, HW, 1, C).to(DEV)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    o32, o16 = group_norm8_nhwc(xd, gd, bd, R.GN_EPS)
    _r(tag + " out_f32", o32.cpu().reshape(N, HW, C), want["out"])
    _stored(tag + " out_bf16", o16.cpu().reshape(N, HW, C), want["out"])
    only32, none16 = group_norm8_nhwc(xd, gd, bd, R.GN_EPS, want_bf16=False)
    none32, only16 = group_norm8_nhwc(xd, gd, bd, R.GN_EPS, want_f32=False)
    assert none16 is None and none32 is None
    _r(tag + " out_f32 alone", only32.cpu().reshape(N, HW, C), want["out"])
    _stored(tag + " out_bf16 alone", only16.cpu().reshape(N, HW, C), want["out"])
    if R.GN_SETS[si] == "const":      # variance 0: rstd = eps^-1/2, xhat exactly 0, the result exactly beta
        assert torch.equal(_bits(o32.cpu().reshape(N, HW, C)[:, :, :8]), _bits(beta[:8].expand(N, HW, 8)))
    xg, gg, bg = xd.clone().requires_grad_(True), gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    dyd = dy.to(torch.bfloat16).reshape(N, HW, 1, C).to(DEV)
    GroupNorm8Function.apply(xg, gg, bg, R.GN_EPS).backward(dyd)
    _stored(tag + " dx", xg.grad.cpu().reshape(N, HW, C), want["dx32"])
    _r(tag + " dgamma", gg.grad.cpu(), want["dgamma"])
    _r(tag + " dbeta", bg.grad.cpu(), want["dbeta"])
    _, _, xc, g32, stats = _group_norm8(xd, gd, bd, R.GN_EPS, False, True)
    dx = torch.full_like(xc, float("nan"))
    bstats = torch.empty(N * (C // 8) * 16, dtype=torch.float64, device=DEV)
    _call("msda_groupnorm8_backward_nhwc_bf16", xc.data_ptr(), dyd.data_ptr(), g32.data_ptr(), R.GN_EPS, N, HW, C, stats.data_ptr(),
          bstats.data_ptr(), dx.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dx), _bits(xg.grad))


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (2, 2, 0)])
def test_max_pool_is_bit_equal_to_torch(k, stride, pad):
    from richsem_amd.conv import max_pool_nhwc
    g = torch.Generator().manual_seed(k)
    for H in (1, 2, 7, 8):
        for W in (1, 2, 7, 8):
            if (H + 2 * pad - k) // stride + 1 < 1 or (W + 2 * pad - k) // stride + 1 < 1 or H + 2 * pad < k or W + 2 * pad < k:
                continue
            for C in (8, 64):
                x = R.bf(torch.randn(2, H, W, C, generator=g))
                x[0, :, :, 0] = float("-inf")                       # a channel of -inf only: every window of it is -inf
                x[1, H // 2, W // 2, :] = float("-inf")
                got = max_pool_nhwc(x.to(torch.bfloat16).to(DEV), k, stride, pad).cpu()
                want = F.max_pool2d(x.permute(0, 3, 1, 2), k, stride, pad).permute(0, 2, 3, 1).to(torch.bfloat16)
                assert got.shape == want.shape and torch.equal(_bits(got), _bits(want.contiguous())), (H, W, C)


@pytest.mark.parametrize("k,H,W", [(2, 7, 9), (3, 7, 8), (7, 15, 20), (3, 3, 3)])
def test_avg_pool_inside_the_bounds(k, H, W):
    from richsem_amd.conv import avg_pool_nhwc
    x = R.pool_inputs(2, H, W, 16)
    _, want32 = R.avg_pool(x, k, R.B32)
    got = avg_pool_nhwc(x.to(torch.bfloat16).to(DEV), k).cpu()
    _stored(f"avg_pool k{k} {H}x{W}", got, want32)


def test_avg_pool_of_two_on_dyadic_inputs_is_bit_equal():
    from richsem_amd.conv import avg_pool_nhwc
    x = R.pool_inputs(2, 7, 9, 64, dyadic=True)
    _, want32 = R.avg_pool(x, 2, R.B32)
    assert float(want32.e.max()) == 0.0
    got = avg_pool_nhwc(x.to(torch.bfloat16).to(DEV), 2).cpu()
    assert torch.equal(_bits(got), _bits(want32.v.to(torch.bfloat16)))


# ---- the by-products of msda_forward_prep_* (fwd_prep_fused 1 and 2) -------------------------------------------------------------------------
_FUSED_OPTIONS = ("fwd_prep_fused", "fwd_variant", "locality_monitor")


def _fused_call(sfx, fused, shapes_l, off, log, ref, value, record):
    """MSDeformAttnFusedFunction on the one-GEMM layout with ``fwd_prep_fused = fused``: -> (out, loc, aw) on the host, loc / aw being the
    kernel's by-products (``out.grad_fn.saved_tensors``); asserts the profile record of the path that ran; the options are put back"""
    from richsem_amd.functions import MSDeformAttnFusedFunction
    from test_gpu_parity import _profiled_variants
    N, Lq, M, L, P, _ = off.shape
    pt, wt = SFX_DT[sfx], torch.float32 if sfx == "bf16" else SFX_DT[sfx]
    q = torch.cat((off.reshape(N, Lq, -1), log.reshape(N, Lq, -1)), -1).to(pt).to(DEV).contiguous().requires_grad_(True)
    shapes = torch.tensor(shapes_l, dtype=torch.int64, device=DEV)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    v, r = value.to(pt).to(DEV), ref.to(wt).to(DEV)
    saved = {k: _lib.get_option(k) for k in _FUSED_OPTIONS}
    got = []
    try:
        _lib.set_option("locality_monitor", 0)
        _lib.set_option("fwd_prep_fused", fused)
        if fused == 2:
            _lib.set_option("fwd_variant", 2)
        ran = _profiled_variants(lambda: got.append(MSDeformAttnFusedFunction.apply(v, shapes, lsi, q, r, M, L, P, 64)))
    finally:
        for k, val in saved.items():
            _lib.set_option(k, val)
    assert ran == [("fwd", record)], ran
    saved_t = got[0].grad_fn.saved_tensors
    return got[0].detach().cpu(), saved_t[3].cpu(), saved_t[4].cpu(), lsi.cpu()


def _fused_check(tag, sfx, fused, shapes_l, off, log, ref, value, record):
    import msda_ref as MR
    N, Lq, M, L, P, _ = off.shape
    D = value.shape[-1]
    mode, limit = (R.B64, 2.0) if sfx == "f64" else (R.B32, 1.0)
    out, loc, aw, lsi = _fused_call(sfx, fused, shapes_l, off, log, ref, value, record)
    depth = R.fused_sum_depth(fused, L, P, D, sfx == "f64")
    loc_b, aw_b = R.prep_forward(off, log, ref, shapes_l, mode, sum_depth=depth)
    _r(tag + " loc", loc, loc_b, limit)
    _r(tag + " aw", aw, aw_b, limit)
    # out: tests/msda_ref.py's bound at the kernel's own loc / aw
    sh = np.array(shapes_l, dtype=np.int64)
    assert MR.boundary_distance(loc.double().numpy(), sh) > 2.0 ** -17
    res, bnd = MR.reference(value.double().numpy(), sh, lsi.numpy(), loc.double().numpy(), aw.double().numpy(),
                            np.zeros((N, Lq, M * D)), sfx)
    ro = MR.ratios(out, res["out"], bnd["out"])[0]
    if REPORT:
        print(f"[measured] rows {tag} out: ratio {ro:.3g}", flush=True)
    assert ro <= limit, (tag, ro)
    if sfx == "bf16":
        assert MR.outside_interval(out, res["out"], bnd["out_sum"]) == 0, tag


@pytest.mark.parametrize("sfx", ["f32", "f64", "bf16"])
@pytest.mark.parametrize("rd,L,P,Lq", [(4, 4, 4, 273), (2, 3, 3, 50)])
def test_fused_prep_by_products_decoder_shaped(sfx, rd, L, P, Lq):
    """fwd_prep_fused = 1: fwd_direct_prep_kernel, record ("fwd", 5)"""
    N, M, D = 2, 8, 32
    dt = torch.float64 if sfx == "f64" else torch.float32
    shapes_l = R.PREP_SHAPES[:L]
    off, log, ref, _, _ = R.prep_inputs(L, P, M, rd, N=N, Lq=Lq, dtype=dt, bf16_proj=sfx == "bf16")
    off = R.keep_off_pixel_boundaries(off, log, ref, shapes_l, sfx == "bf16")
    g = torch.Generator().manual_seed(100 * L + 10 * P + rd)
    S = sum(h * w for h, w in shapes_l)
    value = torch.randn(N, S, M, D, generator=g, dtype=dt)
    value = R.bf(value) if sfx == "bf16" else value
    _fused_check(f"fused 1 {sfx} rd{rd} L{L} P{P} Lq{Lq}", sfx, 1, shapes_l, off, log, ref, value, 5)


@pytest.mark.parametrize("rd,spread", [(2, 1.5), (2, 40.0), (4, 1.5)])
def test_fused_prep_by_products_encoder_shaped(rd, spread):
    """fwd_prep_fused = 2 (f32, P = 4, Lq = S): the window kernel, record ("fwd", 6); offsets of 1.5 pixels stay in their windows, 40
    pixels send most points through the fix-up that recomputes the softmax from the raw row (the cases of
    test_fused_prep_window_gather_equals_the_two_kernel_form)"""
    from richsem_amd import workload as W
    from richsem_amd.modules import get_reference_points
    call = W.shrunk(W.call_E(2), 4)
    shapes_l = [tuple(int(v) for v in s) for s in W.level_tensors(call, "cpu")[0].tolist()]
    N, S, M, D, L, P = call.N, call.S, call.M, call.D, call.L, call.P
    g = torch.Generator().manual_seed(31 + rd)
    value = torch.randn(N, S, M, D, generator=g)
    off = torch.randn(N, S, M, L, P, 2, generator=g) * spread
    log = torch.randn(N, S, M, L, P, generator=g) * 2.0
    vr = torch.rand(N, L, 2, generator=g) * 0.2 + 0.8
    ref = get_reference_points(shapes_l, vr, "cpu").float()
    if rd == 4:
        ref = torch.cat((ref, torch.rand(N, S, L, 2, generator=g) * 0.2 + 0.02), -1).contiguous()
    off = R.keep_off_pixel_boundaries(off, log, ref, shapes_l)
    _fused_check(f"fused 2 f32 rd{rd} spread {spread}", "f32", 2, shapes_l, off, log, ref, value, 6)
