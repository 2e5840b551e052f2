"""GPU (-m gpu): the kernels of csrc/focalnet_ctx.hip -- the context aggregation forward and backward (msda_fmod_context_*) and the
modulation product (msda_fmod_modulate_*) -- against the element-wise bounds of tests/focalnet_ref.py, exact probes checked bit for bit,
NaN-poisoned result buffers with guard rows, and reproducibility of the reductions.

Every tensor a call writes is compared with the float64 definition formed from the STORED inputs of the kernel that wrote it (u_l from the
stored u_{l-1}, du_{l-1} from the stored du_l, ...), so each kernel is checked on its own.  ctx0, the gates and q are read IN PLACE from
wider rows (q | ctx0 | gates | NaN padding), dctx0, the gate gradients and dq are written in place into NaN-poisoned rows of that layout,
whose other columns must stay untouched.  The two configurations (L = 3, window 5) and (L = 4, window 3, normalised) run every K in
{3, 5, 7, 9}; the shapes are those of tests/focalnet_ref.py, on which tests/test_focalnet_ref.py shows every wrong variant leaving the
bounds.  Capture into a HIP graph is NOT tested here."""
import os

import pytest
import torch

import focalnet_ref as R
from test_gpu_swin_block import GUARD, Poisoned

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _bits(t):
    return t.contiguous().view(-1).view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _inside(tag, got, val, bound):
    res = R.ratios(got, val, bound)
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)
    assert sorted(res) == sorted(val) and all(r <= 1.0 for r in res.values()), (tag, res)


def _gen(shape, L):
    return torch.Generator().manual_seed(4000 + sum(shape) + L)


def _ld(C, L):
    return 2 * C + 8 * ((L + 1 + 7) // 8)


def _rows(ctx0, gates, q=None):
    """(B H W, ld) bf16 on the device: q | ctx0 | gates | NaN"""
    B, H, W, C = ctx0.shape
    L = gates.shape[-1] - 1
    rows = torch.full((B * H * W, _ld(C, L)), float("nan"), dtype=BF)
    rows[:, :C] = q.reshape(-1, C) if q is not None else 0
    rows[:, C:2 * C] = ctx0.reshape(-1, C)
    rows[:, 2 * C:2 * C + L + 1] = gates.reshape(-1, L + 1)
    return rows.cuda()


# ---- raw calls into poisoned buffers ---------------------------------------------------------------------------------------------------
def call_forward(rows, wform, shape, L, window, normalize):
    """-> {"u0".., "m", "g", "A"} and the raw u (L, B, H, W, C) and mg (2, B, C) for the backward"""
    from richsem_amd import _lib, focalnet
    B, H, W, C = shape
    n, ld = B * H * W, rows.shape[1]
    u, A, mg = Poisoned(L * n, C, BF), Poisoned(n, C, BF), Poisoned(2 * B, C, torch.float32)
    ws = torch.full((focalnet.workspace_bytes(B, H, W, C) // 4,), float("nan"), device="cuda")
    _lib.check(_lib.load().msda_fmod_context_forward_bf16(rows[:, C:].data_ptr(), ld, rows[:, 2 * C:].data_ptr(), ld, wform.data_ptr(), B, H, W, C,
                                                          L, window, int(normalize), u.ptr(), mg.ptr(), A.ptr(), ws.data_ptr(),
                                                          _lib.raw_stream(rows.device)))
    uu, mm = u.result("u").view(L, B, H, W, C), mg.result("mg").view(2, B, C)
    res = {f"u{l}": uu[l] for l in range(L)}
    res.update(m=mm[0], g=mm[1], A=A.result("A").view(B, H, W, C))
    return res, uu, mm


def call_backward(dA, rows, wform, u, mg, shape, L, window, normalize, want_weights=True):
    """-> {"dgates", "du0".., "dctx0", "dw0"..}; dctx0 and dgates are written in place into NaN rows of the layout of ``rows``"""
    from richsem_amd import _lib, focalnet
    B, H, W, C = shape
    n, ld = B * H * W, rows.shape[1]
    du, drows = Poisoned(L * n, C, BF), Poisoned(n, ld, BF)
    dw = Poisoned(wform.shape[0], C, torch.float32) if want_weights else None
    ws = torch.full((focalnet.workspace_bytes(B, H, W, C) // 4,), float("nan"), device="cuda")
    _lib.check(_lib.load().msda_fmod_context_backward_bf16(dA.data_ptr(), rows[:, C:].data_ptr(), ld, rows[:, 2 * C:].data_ptr(), ld, wform.data_ptr(),
                                                           u.data_ptr(), mg.data_ptr(), B, H, W, C, L, window, int(normalize), du.ptr(),
                                                           drows.view[:, C:].data_ptr(), ld, drows.view[:, 2 * C:].data_ptr(), ld,
                                                           dw.ptr() if dw else None, ws.data_ptr(), _lib.raw_stream(rows.device)))
    full = drows.full.view(torch.int16)
    assert bool((full[:GUARD] == drows.poison).all()) and bool((full[GUARD + n:] == drows.poison).all()), "gradient rows: a guard row was written"
    inner = drows.view.view(torch.int16)
    assert bool((inner[:, :C] == drows.poison).all()) and bool((inner[:, 2 * C + L + 1:] == drows.poison).all()), "gradient rows: a foreign column was written"
    dctx0, dgates = drows.view[:, C:2 * C], drows.view[:, 2 * C:2 * C + L + 1]
    assert not bool(torch.isnan(dctx0).any()) and not bool(torch.isnan(dgates).any()), "gradient rows: an element was not written"
    dd = du.result("du").view(L, B, H, W, C)
    res = {f"du{l}": dd[l] for l in range(L)}
    res.update(dctx0=dctx0.reshape(B, H, W, C), dgates=dgates.reshape(B, H, W, L + 1))
    if want_weights:
        dww, row = dw.result("dw"), 0
        for l, K in enumerate(R.sizes(L, window)):
            res[f"dw{l}"] = dww[row:row + K * K]
            row += K * K
    return res


def _run(shape, cfg, want_weights=True):
    L, window, normalize = cfg
    ctx0, gates, ws, dA = R.make_inputs(shape, L, window, _gen(shape, L))
    rows, wform, dAd = _rows(ctx0, gates), R.weight_form(ws).cuda(), dA.cuda()
    fwd, u, mg = call_forward(rows, wform, shape, L, window, normalize)
    bwd = call_backward(dAd, rows, wform, u, mg, shape, L, window, normalize, want_weights)
    return (ctx0, gates, ws, dA), (rows, wform, dAd, u, mg), fwd, bwd


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", R.CONFIGS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_every_kernel_inside_its_bound_and_reproducible(shape, cfg):
    L, window, normalize = cfg
    (ctx0, gates, ws, dA), (rows, wform, dAd, u, mg), fwd, bwd = _run(shape, cfg)
    stored = {k: v.cpu() for k, v in {**fwd, **bwd}.items()}
    val, bound = R.forward_reference(ctx0, gates, ws, L, window, normalize, stored)
    _inside(f"forward {shape} {cfg}", fwd, val, bound)
    val, bound = R.backward_reference(dA, ctx0, gates, ws, L, window, normalize, stored)
    _inside(f"backward {shape} {cfg}", bwd, val, bound)
    fwd2, u2, mg2 = call_forward(rows, wform, shape, L, window, normalize)
    assert all(_same(fwd[k], fwd2[k]) for k in fwd)
    bwd2 = call_backward(dAd, rows, wform, u2, mg2, shape, L, window, normalize)
    assert all(_same(bwd[k], bwd2[k]) for k in bwd)
    alone = call_backward(dAd, rows, wform, u, mg, shape, L, window, normalize, want_weights=False)
    assert all(_same(bwd[k], alone[k]) for k in alone) and not any(k.startswith("dw") for k in alone)


def test_weight_gradient_at_the_widest_map_inside_its_bound_and_reproducible():
    shape, cfg = R.WGRAD_SHAPE, R.CONFIGS[1]
    L, window, normalize = cfg
    (ctx0, gates, ws, dA), (rows, wform, dAd, u, mg), fwd, bwd = _run(shape, cfg)
    stored = {k: v.cpu() for k, v in {**fwd, **bwd}.items()}
    val, bound = R.backward_reference(dA, ctx0, gates, ws, L, window, normalize, stored, only="dw")
    _inside(f"weight gradient {shape}", {k: v for k, v in bwd.items() if k.startswith("dw")}, val, bound)
    again = call_backward(dAd, rows, wform, u, mg, shape, L, window, normalize)
    assert all(_same(bwd[k], again[k]) for k in bwd)


@pytest.mark.parametrize("tokens, C", [(1, 32), (65, 96), (130, 4096)])
def test_modulation_product_inside_its_bounds(tokens, C):
    from richsem_amd import _lib
    gen = torch.Generator().manual_seed(tokens + C)
    q, mod, dout = (torch.randn(tokens, C, generator=gen).to(BF) for _ in range(3))
    ld = 2 * C + 8
    rows = torch.full((tokens, ld), float("nan"), dtype=BF)
    rows[:, :C] = q
    rows, md, dd = rows.cuda(), mod.cuda(), dout.cuda()
    out, dmod, drows = Poisoned(tokens, C, BF), Poisoned(tokens, C, BF), Poisoned(tokens, ld, BF)
    lib, stream = _lib.load(), _lib.raw_stream(rows.device)
    _lib.check(lib.msda_fmod_modulate_forward_bf16(rows.data_ptr(), ld, md.data_ptr(), tokens, C, out.ptr(), stream))
    _lib.check(lib.msda_fmod_modulate_backward_bf16(dd.data_ptr(), rows.data_ptr(), ld, md.data_ptr(), tokens, C, drows.ptr(), ld, dmod.ptr(), stream))
    assert bool((drows.full.view(torch.int16)[:, C:] == drows.poison).all()), "dq: a foreign column was written"
    got = {"out": out.result("out"), "dmod": dmod.result("dmod"), "dq": drows.view[:, :C]}
    val, bound = R.modulate_reference(q, mod, dout)
    _inside(f"modulate {(tokens, C)}", got, val, bound)


# ---- exact probes ------------------------------------------------------------------------------------------------------------------------
PROBE = (2, 13, 20, 64)      # two tiles along x: the probe at (6, 14) spreads over the tile edge


def _dyadic(shape, gen, steps=127, unit=64):
    return torch.randint(-steps, steps + 1, shape, generator=gen).float() / unit


@pytest.mark.parametrize("K", [3, 5, 7, 9])
@pytest.mark.parametrize("y0, x0", [(6, 14), (0, 0), (12, 19)])
def test_one_hot_input_places_the_taps(K, y0, x0):
    """one level of window K: u_0 is the convolution itself"""
    B, H, W, C = PROBE
    c0, p = 37, K // 2
    w = _dyadic((K * K, C), torch.Generator().manual_seed(11 + K))
    ctx0 = torch.zeros(PROBE, dtype=BF)
    ctx0[0, y0, x0, c0] = 1.0
    expect = torch.zeros(PROBE)
    for ky in range(K):
        for kx in range(K):
            y, xx = y0 + p - ky, x0 + p - kx
            if 0 <= y < H and 0 <= xx < W:
                expect[0, y, xx, c0] = w[K * ky + kx, c0]
    rows = _rows(ctx0, torch.zeros(B, H, W, 2, dtype=BF))
    fwd, u, mg = call_forward(rows, w.cuda(), PROBE, 1, K, False)
    assert _same(fwd["u0"].cpu(), expect.to(BF))      # channels other than c0 and all of image 1: exact (positive) zeros
    # the backward's flipped taps: a one-hot du_0 (dA one-hot, gate_0 = 1, u_0 = 16 where GELU' is 1 in fp32) spreads the other way
    ctx0 = torch.zeros(PROBE, dtype=BF)
    gates = torch.zeros(B, H, W, 2, dtype=BF)
    gates[..., 0] = 1.0
    centre = torch.zeros(K * K, C)
    centre[K * p + p] = 1.0
    rows = _rows(torch.full(PROBE, 16.0, dtype=BF), gates)
    fwd, u, mg = call_forward(rows, centre.cuda(), PROBE, 1, K, False)
    assert _same(fwd["u0"].cpu(), torch.full(PROBE, 16.0, dtype=BF))
    dA = torch.zeros(PROBE, dtype=BF)
    dA[0, y0, x0, c0] = 1.0
    bwd = call_backward(dA.cuda(), rows, w.cuda(), u, mg, PROBE, 1, K, False)
    assert _same(bwd["du0"].cpu(), dA)
    flipped = torch.zeros(PROBE)
    for ky in range(K):
        for kx in range(K):
            y, xx = y0 + ky - p, x0 + kx - p
            if 0 <= y < H and 0 <= xx < W:
                flipped[0, y, xx, c0] = w[K * ky + kx, c0]
    assert _same(bwd["dctx0"].cpu(), flipped.to(BF))
    # ... and the weight gradient reads the shifted input: every pixel of ctx0 is 16, so tap (ky, kx) is 16 where the shifted pixel exists
    inside = torch.zeros(K * K, C)
    for ky in range(K):
        for kx in range(K):
            if 0 <= y0 + ky - p < H and 0 <= x0 + kx - p < W:
                inside[K * ky + kx, c0] = 16.0
    assert _same(bwd["dw0"].cpu(), inside)


def test_zero_cotangent_gives_exact_zeros():
    cfg = R.CONFIGS[1]
    L, window, normalize = cfg
    ctx0, gates, ws, _ = R.make_inputs(PROBE, L, window, torch.Generator().manual_seed(13))
    rows, wform = _rows(ctx0, gates), R.weight_form(ws).cuda()
    _, u, mg = call_forward(rows, wform, PROBE, L, window, normalize)
    bwd = call_backward(torch.zeros(PROBE, dtype=BF).cuda(), rows, wform, u, mg, PROBE, L, window, normalize)
    for k, v in bwd.items():
        assert bool((v == 0).all()), k


@pytest.mark.parametrize("normalize", [False, True])
def test_exact_maps_make_single_floats(normalize):
    """u in {0, 8, 16}, where erf-GELU is exact in fp32 (GELU(8) = 8, GELU(16) = 16), dyadic gates and cotangents: the means, g, A and the
    gate gradients are single floats whatever the order of the sums, and are compared bit for bit.  Centre-tap weights keep u_l = ctx0 at
    every level (L = 3, s = 1 or 1/4); channel c is 0, 8 or 16 everywhere, or 0 and 16 on alternating pixels (mean 8)."""
    L, window = 3, 3
    B, H, W, C = shape = (2, 4, 8, 32)
    gen = torch.Generator().manual_seed(17)
    kind = torch.arange(C) % 4
    alt = (torch.arange(H * W).reshape(H, W) % 2).float() * 16
    ctx0 = torch.zeros(shape)
    ctx0[..., kind == 1] = 8.0
    ctx0[..., kind == 2] = 16.0
    ctx0[..., kind == 3] = alt[None, :, :, None]
    ctx0[1] = ctx0[1].flip(-1)      # the images differ
    gates = _dyadic((B, H, W, L + 1), gen, steps=4, unit=4)
    dA = _dyadic(shape, gen, steps=2, unit=2)
    ws = []
    for K in R.sizes(L, window):
        w = torch.zeros(K * K, C)
        w[K * (K // 2) + K // 2] = 1.0
        ws.append(w)
    rows, wform = _rows(ctx0.to(BF), gates.to(BF)), R.weight_form(ws).cuda()
    fwd, u, mg = call_forward(rows, wform, shape, L, window, normalize)
    s = 1.0 / (L + 1) if normalize else 1.0
    m = ctx0.mean((1, 2))
    assert all(_same(fwd[f"u{l}"].cpu(), ctx0.to(BF)) for l in range(L))
    assert _same(fwd["m"].cpu(), m) and _same(fwd["g"].cpu(), m) and set(m.unique().tolist()) == {0.0, 8.0, 16.0}
    A = s * ((gates[..., :L].sum(-1, keepdim=True)) * ctx0 + gates[..., L:] * m[:, None, None, :]) + 0.0      # (+ 0.0: no negative zeros)
    assert torch.equal(A.to(BF).float(), A) and _same(fwd["A"].cpu(), A.to(BF))
    bwd = call_backward(dA.to(BF).cuda(), rows, wform, u, mg, shape, L, window, normalize, want_weights=False)
    dg = torch.stack([s * (dA * ctx0).sum(-1)] * L + [s * (dA * m[:, None, None, :]).sum(-1)], -1) + 0.0
    assert torch.equal(dg.to(BF).float(), dg) and _same(bwd["dgates"].cpu(), dg.to(BF))


# ---- the autograd functions ----------------------------------------------------------------------------------------------------------------
def test_autograd_functions_return_the_kernels_results_in_the_parameters_dtypes():
    from richsem_amd import focalnet
    shape, (L, window, normalize) = (2, 13, 9, 96), R.CONFIGS[0]
    B, H, W, C = shape
    ctx0, gates, ws, dA = R.make_inputs(shape, L, window, _gen(shape, L))
    params = [w.t().reshape(C, 1, K, K).contiguous().cuda().requires_grad_(True) for w, K in zip(ws, R.sizes(L, window))]      # fp32 parameters
    params[1] = params[1].detach().to(BF).requires_grad_(True)      # ... and a bf16 one: the kernel reads its fp32 copy
    forms = [w if i != 1 else w.to(BF).float() for i, w in enumerate(ws)]
    rows = _rows(ctx0, gates, torch.randn(B, H, W, C, generator=_gen(shape, L + 1)).to(BF)).view(B, H, W, -1).requires_grad_(True)
    q, c0, gt = torch.split(rows, (C, C, rows.shape[-1] - 2 * C), -1)
    A = focalnet.focal_context(c0, gt[..., :L + 1], params, normalize)      # strided views of wider rows: read in place
    A.backward(dA.cuda())
    wform = R.weight_form(forms).cuda()
    fwd, u, mg = call_forward(rows.detach().view(B * H * W, -1), wform, shape, L, window, normalize)
    bwd = call_backward(dA.cuda(), rows.detach().view(B * H * W, -1), wform, u, mg, shape, L, window, normalize)
    assert _same(A.detach(), fwd["A"])
    assert _same(rows.grad[..., C:2 * C], bwd["dctx0"]) and _same(rows.grad[..., 2 * C:2 * C + L + 1], bwd["dgates"])
    for l, (p, K) in enumerate(zip(params, R.sizes(L, window))):
        assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
        assert _same(p.grad, bwd[f"dw{l}"].t().reshape(C, 1, K, K).to(p.dtype))
    # a contiguous copy of the operands gives the same bits
    A2 = focalnet.focal_context(c0.detach().contiguous(), gt[..., :L + 1].detach().contiguous(), [p.detach() for p in params], normalize)
    assert _same(A2, fwd["A"])
    qd, md = q.detach().contiguous().requires_grad_(True), fwd["A"].clone().requires_grad_(True)
    out = focalnet.modulate(qd, md)
    out.backward(dA.cuda())
    val, bound = R.modulate_reference(qd.detach().cpu(), md.detach().cpu(), dA)
    _inside("modulate()", {"out": out.detach(), "dq": qd.grad, "dmod": md.grad}, val, bound)
