"""GPU (-m gpu): the convolution family (richsem_amd/csrc/conv_mfma.hip, conv_wgrad.hip) through richsem_amd.conv and the C ABI against
the float64 references of tests/conv_ref.py.  Every case runs twice:
  (a) the EXACT PROBE (small integers: every product and partial sum exact in fp32, so the result does not depend on the summation
      order) -- torch.equal with the reference, for the k split's atomics, the chunk reductions, the rings and every tile shape alike;
  (b) real-valued inputs (randn, weight scaled by K^-1/2) against the ELEMENT-WISE bound derived in conv_ref's docstring, no exclusions.
Shapes are the smallest that reach the edge named: pixel counts around the 16-pixel tiles, the 64-pixel workgroups and the 48-pixel
waves of pt = 3; every channel class; ring lengths around the slot count; uneven k slices; empty parity classes; pixel chunks of one
pixel.  Every test that forces a tile asserts conv_ref.forced_tile_is_taken, so no forced tile is silently the automatic one.
RICHSEM_REPORT=1 prints the worst |err| / bound per tensor (profiles/r18_conv_bounds.md)."""
import ctypes
import os

import pytest
import torch

import conv_ref as R
from richsem_amd import _lib
from richsem_amd.conv import ConvAffineFunction, _pack, _pack_form, conv_dgrad, conv_forward, set_ring, set_tiling

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
NAN = float("nan")


def _say(tag, **kv):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in kv.items()), flush=True)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def _dims(case):
    N, H, W, Cin, Cout, k, stride, pad = case
    return N, H, W, Cin, Cout, k, k, stride, pad


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
class _Forward:
    """one problem on the device: packed once, launched under any tile / ring setting"""

    def __init__(self, p, misalign=False):
        self.p = p
        self.Cout, _, self.k, _ = p["w"].shape
        self.packed = _pack(p["w"].cuda().contiguous())
        x = _nhwc(p["x"])
        if misalign:      # the few-channel kernel reads x element by element: a pointer that is only 2-byte aligned
            buf = torch.zeros(x.numel() + 1, dtype=BF, device="cuda")
            buf[1:] = x.reshape(-1)
            x = buf[1:].view(x.shape)
            assert x.data_ptr() % 4 == 2
        self.x = x
        self.scale = (p["scale"] if p["scale"] is not None else torch.ones(self.Cout)).cuda()
        self.shift = (p["shift"] if p["shift"] is not None else torch.zeros(self.Cout)).cuda()
        self.res = _nhwc(p["residual"]) if p["residual"] is not None else None

    def __call__(self):
        p = self.p
        return _nchw(conv_forward(self.x, self.packed, self.scale, self.shift, self.res, self.Cout, self.k, self.k, p["stride"], p["pad"], p["relu"]))


def _forward_pair(case, epilogue, **kw):
    """-> [(launcher, exact result or None, float64 reference, bound)] for the probe and the real-valued inputs"""
    pp, pr = R.make_forward(case, epilogue, 0, probe=True), R.make_forward(case, epilogue, 0)
    ok, nonzero, _ = R.probe_conditions("forward", pp)
    assert ok and nonzero > 0.5, (case, epilogue, nonzero)
    return pp, pr, _Forward(pp, **kw), _Forward(pr, **kw)


def _check_forward(tag, fp, fr, want_p, ref_r):
    got = fp()
    assert torch.equal(got, want_p), (tag, "exact probe", int((got != want_p).sum()), float((got.double() - want_p.double()).abs().max()))
    y, b = ref_r
    r = R.ratio(fr(), y, b)
    assert r <= 1.0, (tag, "real-valued", r)
    return r


def _forward_case(case, configs=((0, 0),), ring=None, ksplit=False, epilogues=R.EPILOGUES, **kw):
    """every epilogue under every (ct, pt) of `configs` ((0, 0): automatic); ring: the msda_conv_set_ring value, or None: untouched"""
    N, H, W, Cin, Cout, k, stride, pad = case
    worst = 0.0
    for epilogue in epilogues:
        pp, pr, fp, fr = _forward_pair(case, epilogue, **kw)
        want_p, ref_r = R.forward_reference(pp)[0].to(BF), R.forward_reference(pr, ksplit=ksplit)
        for ct, pt in configs:
            if ct:
                assert R.forced_tile_is_taken(Cout, ct), (Cout, ct)
            try:
                set_tiling(ct, pt)
                if ring is not None:
                    set_ring(ring)
                worst = max(worst, _check_forward((case, epilogue, ct, pt, ring), fp, fr, want_p, ref_r))
            finally:
                set_ring(0)
                set_tiling(0, 0)
    _say(f"forward {case} ring={ring}", y=worst)


def _edge_params():
    return [(cout, s) for cout in R.PIXEL_EDGE_COUT for s in R.pixel_edge_shapes(cout)]


@pytest.mark.parametrize("cout,case", _edge_params(), ids=str)
def test_forward_pixel_tile_edges_under_every_tile(cout, case):
    """P around 16 (a tile), 64 (a workgroup at pt = 1), 192 (at pt = 3); every forced tile the host takes for this C_out, pt 1 .. 3"""
    assert R.valid_tiles(cout)
    _forward_case(case, [(0, 0)] + [(ct, pt) for ct in R.valid_tiles(cout) for pt in (1, 2, 3)])


@pytest.mark.parametrize("case", R.CHANNEL_CASES, ids=str)
def test_forward_channel_classes(case):
    """C_in = 32, 96: one k-step per barrier; 64, 128, 192: pairs of k-steps (one and three pairs: odd)"""
    _forward_case(case, ring=-1)
    if case[3] % 64 == 0:
        _forward_case(case, [(R.valid_tiles(case[4])[0], 1)], ring=3)


@pytest.mark.parametrize("case", R.FEW_CASES, ids=str)
def test_forward_few_channel_path(case):
    """K = KH KW C_in up to the table's 512 entries (507 padded to 512; 512 exactly), C_in = 1 .. 48, stride 1 and 2, and an input pointer
    that is only 2-byte aligned"""
    assert case[3] % 32 != 0 and case[3] * case[5] ** 2 <= 512
    _forward_case(case)
    _forward_case(case, epilogues=("residual_relu",), misalign=True)


def test_few_channel_limit_is_refused():
    for cin, k in ((57, 3), (8, 9)):      # K = 513, 648
        with pytest.raises(RuntimeError, match="BAD_DIMS"):
            _pack(torch.zeros(32, cin, k, k, device="cuda"))


def _ring_params():
    return [(slots, S) for slots in R.RING_SLOTS for S in R.ring_lengths(slots)] + [(slots, 9) for slots in R.RING_SLOTS]


@pytest.mark.parametrize("slots,S", _ring_params(), ids=str)
def test_ring_forward_lengths_around_the_slot_count(slots, S):
    """conv_ring_kernel with R slots on k loops of S = 1, 2, R - 2 .. R + 1 iterations (and a 3 x 3's 9): the prologue's R - 1 requests, the
    repeated requests past the end and the slot wrap; 35 pixels (no multiple of 16 pt); against the reference AND the register-staged
    kernel under the same tile"""
    for cout, ct, pt in R.RING_TILES:
        case = R.ring_case(S, cout)
        assert R.forced_tile_is_taken(cout, ct) and ct >= 2 and pt <= 2 and case[3] % 64 == 0      # choose_ring's conditions under a forced tile
        _forward_case(case, [(ct, pt)], ring=slots)
        _, pr, _, fr = _forward_pair(case, "residual_relu")
        try:
            set_tiling(ct, pt)
            set_ring(-1)
            want = fr()
            set_ring(slots)
            got = fr()
        finally:
            set_ring(0)
            set_tiling(0, 0)
        assert torch.equal(got, want), (cout, ct, pt)


def _bytes(fn, *dims):
    nb = ctypes.c_int64(0)
    _lib.check(fn(*dims, ctypes.byref(nb)))
    return nb.value


@pytest.mark.parametrize("case", R.KSPLIT_FWD, ids=str)
def test_forward_k_split(case):
    """k slices that add their sums with fp32 atomics: S = 72 in 9 slices, S = 81 in 10 uneven ones; the probe makes them bit-comparable"""
    N, H, W, Cin, Cout, k, stride, pad = case
    assert _bytes(_lib.load().msda_conv_forward_workspace_bytes, *_dims(case)) == N * H * W * Cout * 4 > 0
    _forward_case(case, ksplit=True)


# ---- input gradient -------------------------------------------------------------------------------------------------------------------
def _dgrad_run(p, add=True, mask=True):
    Cout, Cin, k, _ = p["w"].shape
    N, _, H, W = p["x_shape"]
    packed_t = _pack_form(p["w"].cuda(), p["scale"].cuda(), True)
    return _nchw(conv_dgrad(_nhwc(p["dz"]), packed_t, (N, H, W, Cin), Cout, k, k, p["stride"], p["pad"],
                            add=_nhwc(p["add"]) if add and p["add"] is not None else None,
                            relu_out=_nhwc(p["relu_out"]) if mask and p["relu_out"] is not None else None))


def _variant(p, add, mask):
    q = dict(p)
    if not add:
        q["add"] = None
    if not mask:
        q["relu_out"] = None
    return q


def _dgrad_case(case, rings=(-1, 4), ksplit=False):
    pp, pr = R.make_dgrad(case, True, True, 0, probe=True), R.make_dgrad(case, True, True, 0)
    worst = 0.0
    for add, mask in R.DGRAD_VARIANTS:
        qp, qr = _variant(pp, add, mask), _variant(pr, add, mask)
        assert R.probe_conditions("dgrad", qp)[0]
        want_p = R.dgrad_reference(qp)[0].to(BF)
        y, b, zero = R.dgrad_reference(qr, ksplit=ksplit)
        for ring in rings:
            try:
                set_ring(ring)
                got_p, got_r = _dgrad_run(qp), _dgrad_run(qr)
            finally:
                set_ring(0)
            assert torch.equal(got_p, want_p), (case, add, mask, ring, "exact probe", int((got_p != want_p).sum()))
            r = R.ratio(got_r, y, b, zero)
            assert r <= 1.0, (case, add, mask, ring, "real-valued", r)
            worst = max(worst, r)
    _say(f"dgrad {case}", dx=worst)


@pytest.mark.parametrize("case", R.DGRAD_CASES, ids=str)
def test_input_gradient(case):
    """stride 2 with rows the forward never read (6 x 7, 7 x 6) and with EMPTY parity classes (height or width 1), stride 2 k 1 (three
    classes without taps), stride 3, k 5 at pad 0 / 2 / 4; C_out = 32, 96 (one k-step per barrier) and 64, 128 (pairs); both kernels;
    plain, + add, relu_out, both"""
    assert _bytes(_lib.load().msda_conv_dgrad_workspace_bytes, case[0], *R.out_hw(*case[1:3], *case[5:8]), case[4], case[3], case[5], case[5],
                  case[6], case[7], case[1], case[2]) == 0
    _dgrad_case(case)


def test_input_gradient_k_split():
    case = R.KSPLIT_DGRAD
    N, H, W, Cin, Cout, k, stride, pad = case
    assert _bytes(_lib.load().msda_conv_dgrad_workspace_bytes, N, H, W, Cout, Cin, k, k, stride, pad, H, W) == N * H * W * Cin * 4 > 0
    _dgrad_case(case, rings=(0,), ksplit=True)


@pytest.mark.parametrize("case", [R.DGRAD_CASES[0], R.DGRAD_CASES[2], R.DGRAD_CASES[-1], R.KSPLIT_DGRAD], ids=str)
def test_mask_rule_is_relu_out_greater_than_zero(case):
    """relu_out cycling over +-0, the +- smallest / largest subnormals, the +- smallest normal, +-1, +-inf in EVERY element position: the
    gradient is kept, bit for bit, iff relu_out > 0 (conv_epilogue and, for the k split, conv_ksum_finish_kernel)"""
    p = R.make_dgrad(case, True, True, 0, mask_probe=True)
    keep = p["relu_out"] > 0
    assert 0.4 < float(keep.float().mean()) < 0.6
    for ring in (-1, 4):
        try:
            set_ring(ring)
            masked, unmasked = _dgrad_run(p), _dgrad_run(p, mask=False)
        finally:
            set_ring(0)
        assert torch.equal(masked, torch.where(keep, unmasked, torch.zeros_like(unmasked))), ring
        assert bool((masked[~keep].view(torch.int16) == 0).all())      # +0, not -0
    y, b, zero = R.dgrad_reference(p, ksplit=case == R.KSPLIT_DGRAD)
    assert R.ratio(masked, y, b, zero) <= 1.0


def test_mask_rule_on_nan_is_the_sign_bit():
    """PINNED, not endorsed: the kernel compares the bf16's bits as int16 with 0, so a NaN activation keeps the gradient when its sign bit
    is clear and zeroes it when set; aten::threshold_backward keeps both.  The forward's fmaxf never produces a NaN activation."""
    case = R.DGRAD_CASES[0]
    p = R.make_dgrad(case, True, True, 0)
    bits = torch.tensor([0x7FC0, 0xFFC0 - 0x10000, 0x7F81, 0xFF81 - 0x10000], dtype=torch.int16)
    act = p["relu_out"].permute(0, 2, 3, 1).reshape(-1).clone()
    act[:] = bits.view(BF)[torch.arange(act.numel()) % 4]
    p["relu_out"] = act.view(case[0], case[1], case[2], case[3]).permute(0, 3, 1, 2).contiguous()
    assert bool(torch.isnan(p["relu_out"]).all())
    keep = p["relu_out"].view(torch.int16) > 0
    masked, unmasked = _dgrad_run(p), _dgrad_run(p, mask=False)
    assert torch.equal(masked, torch.where(keep, unmasked, torch.zeros_like(unmasked)))
    ref = torch.ops.aten.threshold_backward(unmasked, p["relu_out"], 0)
    assert torch.equal(ref, unmasked)      # (what the aten op does with NaN: keeps every element)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
def _wgrad_single(dz, x, case, torch_layout, scale, want_bias, ring):
    """msda_conv_wgrad_bf16 into NaN-poisoned result and workspace buffers -> (dw as (C_out, C_in, k, k), dbias or None) on the CPU"""
    N, H, W, Cin, Cout, k, stride, pad = case
    L = _lib.load()
    nb = _bytes(L.msda_conv_wgrad_workspace_bytes, *_dims(case))
    dw = torch.full((Cout, Cin, k, k) if torch_layout else (Cout, k, k, Cin), NAN, device="cuda")
    db = torch.full((Cout,), NAN, device="cuda") if want_bias else None
    ws = torch.full((max(nb // 4, 1),), NAN, device="cuda")
    try:
        _lib.check(L.msda_conv_set_wgrad_ring(ring))
        _lib.check(L.msda_conv_wgrad_bf16(dz.data_ptr(), x.data_ptr(), *_dims(case), dw.data_ptr(), db.data_ptr() if want_bias else None,
                                          scale.data_ptr() if scale is not None else None, torch_layout, ws.data_ptr(), _lib.raw_stream(x.device)))
        torch.cuda.synchronize()
    finally:
        _lib.check(L.msda_conv_set_wgrad_ring(1))
    return (dw if torch_layout else dw.permute(0, 3, 1, 2)).cpu(), db.cpu() if want_bias else None


@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=str)
def test_weight_gradient(case):
    """pixel counts around a ring stage (32), a stage (64) and a chunk (128: at 129 the second chunk holds ONE pixel); image boundaries
    inside a stage; 70 images of one output pixel; two channel blocks on either side; torch_layout x scale x dbias x ring"""
    worst = {"dw": 0.0, "dbias": 0.0}
    for probe in (True, False):
        p = R.make_wgrad(case, 0, probe=probe)
        if probe:
            ok, nonzero, _ = R.probe_conditions("wgrad", p)
            assert ok and nonzero > 0.5
        refs = {s: R.wgrad_reference(p, scaled=s) for s in (False, True)}
        dz, x, scale = _nhwc(p["dz"]), _nhwc(p["x"]), p["scale"].cuda()
        for torch_layout in (0, 1):
            for scaled in (False, True):
                for want_bias in (False, True):
                    for ring in (0, 1):
                        tag = (case, "probe" if probe else "real", torch_layout, scaled, want_bias, ring)
                        dw, db = _wgrad_single(dz, x, case, torch_layout, scale if scaled else None, want_bias, ring)
                        val, b = refs[scaled]
                        if probe:
                            assert torch.equal(dw.double(), val["dw"]), (tag, int((dw.double() != val["dw"]).sum()))
                            assert db is None or torch.equal(db.double(), val["dbias"]), tag
                        else:
                            got = {"dw": dw, "dbias": db}
                            for n in got:
                                if got[n] is not None:
                                    r = R.ratio(got[n], val[n], b[n])
                                    assert r <= 1.0, (tag, n, r)
                                    worst[n] = max(worst[n], r)
    _say(f"wgrad {case}", **worst)


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("ring", [0, 1])
def test_grouped_weight_gradient_against_the_reference(n, ring):
    """msda_conv_wgrad_group_bf16 through ctypes: problems of one chunk and of several in one group, dbias on some problems and NULL on others
    (conv_wgrad_group_kernel<true, true> with mixed bias pointers), scale on some; against the float64 reference, not the single launches"""
    L = _lib.load()
    cases = R.GROUP_POOL[:n]
    worst = {"dw": 0.0, "dbias": 0.0}
    for probe in (True, False):
        arr = (_lib.WgradProblem * n)()
        keep, outs = [], []
        for j, case in enumerate(cases):
            N, H, W, Cin, Cout, k, stride, pad = case
            p = R.make_wgrad(case, j, probe=probe)
            assert not probe or R.probe_conditions("wgrad", p)[0]
            dz, x, scale = _nhwc(p["dz"]), _nhwc(p["x"]), p["scale"].cuda() if j % 3 != 1 else None
            dw = torch.full((Cout, Cin, k, k), NAN, device="cuda")
            db = torch.full((Cout,), NAN, device="cuda") if j % 2 == 0 else None
            keep += [dz, x, scale]
            outs.append((p, dw, db, scale is not None))
            arr[j] = _lib.WgradProblem(dz.data_ptr(), x.data_ptr(), dw.data_ptr(), scale.data_ptr() if scale is not None else None,
                                       db.data_ptr() if db is not None else None, N, H, W, Cin, Cout, k, k, stride, pad)
        nb = _bytes(L.msda_conv_wgrad_group_workspace_bytes, arr, n)
        assert (nb > 0) == (n > 1)      # the first problem alone (33 pixels) is one chunk; the second (390 pixels) is split
        ws = torch.full((max(nb // 4, 1),), NAN, device="cuda")
        try:
            _lib.check(L.msda_conv_set_wgrad_ring(ring))
            _lib.check(L.msda_conv_wgrad_group_bf16(arr, n, ws.data_ptr(), _lib.raw_stream(ws.device)))
            torch.cuda.synchronize()
        finally:
            _lib.check(L.msda_conv_set_wgrad_ring(1))
        for j, (p, dw, db, scaled) in enumerate(outs):
            val, b = R.wgrad_reference(p, scaled=scaled)
            got = {"dw": dw.cpu(), "dbias": db.cpu() if db is not None else None}
            for name in got:
                if got[name] is None:
                    continue
                if probe:
                    assert torch.equal(got[name].double(), val[name]), (n, ring, j, name, int((got[name].double() != val[name]).sum()))
                else:
                    r = R.ratio(got[name], val[name], b[name])
                    assert r <= 1.0, (n, ring, j, name, r)
                    worst[name] = max(worst[name], r)
    _say(f"wgrad group n={n} ring={ring}", **worst)


# ---- module level -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.MODULE_CASES, ids=str)
def test_conv_affine_function_forward_and_gradients(case):
    """ConvAffineFunction: y, dx, dw and the residual's gradient against the bounds.  The ReLU mask of the backward is taken from the y the
    kernel returned (an exact element-wise op: the residual's gradient must equal it bit for bit).  128 -> 128 takes the library's weight
    gradient; 64 -> 96 takes MIOpen's on bf16 operands, whose bf16 result gets conv_ref.miopen_dw_bound."""
    N, H, W, Cin, Cout, k, stride, pad = case
    p = R.make_forward(case, "residual_relu", 0)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(N, Cout, *R.out_hw(H, W, k, stride, pad), generator=g).to(BF)
    xg = _nhwc(p["x"]).requires_grad_(True)
    wg = p["w"].cuda().requires_grad_(True)
    rg = _nhwc(p["residual"]).requires_grad_(True)
    y = ConvAffineFunction.apply(xg, wg, p["scale"].cuda(), p["shift"].cuda(), rg, stride, pad, True)
    y.backward(_nhwc(dy))
    y_got = _nchw(y.detach())
    yr, yb = R.forward_reference(p)
    r = {"y": R.ratio(y_got, yr, yb)}
    dz = torch.where(y_got > 0, dy, torch.zeros_like(dy))
    assert torch.equal(_nchw(rg.grad), dz)
    q = {"dz": dz, "w": p["w"], "scale": p["scale"], "add": None, "relu_out": None, "x_shape": (N, Cin, H, W), "stride": stride, "pad": pad}
    dxr, dxb, zero = R.dgrad_reference(q)
    r["dx"] = R.ratio(_nchw(xg.grad), dxr, dxb, zero)
    wp = {"dz": dz, "x": p["x"], "scale": p["scale"], "k": k, "stride": stride, "pad": pad}
    val, b = R.wgrad_reference(wp)
    own = Cout % 128 == 0 and Cin % 128 == 0
    r["dw"] = R.ratio(wg.grad.cpu(), val["dw"], b["dw"] if own else R.miopen_dw_bound(wp))
    _say(f"module {case} {'own' if own else 'miopen'} wgrad", **r)
    for n in r:
        assert r[n] <= 1.0, (n, r[n])
