"""GPU (-m gpu): the CLIP side of the model -- the class score (richsem_amd/csrc/cls_mfma.hip), ROIAlign (csrc/msda_roi.h) and the
attention-pool core (csrc/msda_attnpool.h) -- against the float64 restatements, the ELEMENT-WISE bounds and the EXACT PROBES of
tests/clip_side_ref.py (derivations in its docstring; tests/test_clip_side_ref.py shows that correct implementations meet them).
The class score and the attention pool go through the C ABI with ctypes, so that G, A, u, spos and the result buffers are the test's own;
one pass per family goes through ClassScorer, roi_align and AttentionPool2d.  Every result buffer is NaN-poisoned and longer than needed:
the tail holds a sentinel that must be untouched after the call.  An excess over a derived bound is a bug in the kernel or in the
derivation, not a reason to widen it.  RICHSEM_REPORT=1 prints the worst |err| / bound per case (profiles/r22_clip_side_bounds.md)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import clip_side_ref as R
from oracle import cls_oracle, roi_oracle
from richsem_amd import _lib

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
SENTINEL = -12345.0
TAIL = 64
TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
OK, NULL_POINTER, BAD_DIMS = 0, -1, -2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_align", "parent_kernel_r22.npz")


def _say(tag, **kv):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3g}" for k, v in kv.items()), flush=True)


def _poisoned(n, dtype):
    buf = torch.full((n + TAIL,), float("nan"), dtype=dtype, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _result(buf, n):
    """the first n elements on the CPU, after checking that the call wrote nothing past them"""
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENTINEL).all()), "stored past the end of the result"
    return buf[:n].cpu()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t.to(dtype) if dtype is not None else t).contiguous().cuda()


# ===== class score ==============================================================================================================================
class _Scorer:
    """[G; A] packed once on the device by msda_cls_pack; scores of any x under either `parts`"""

    def __init__(self, G, A):
        self.lib = _lib.load()
        self.classes = G.shape[0]
        n = ctypes.c_int64(0)
        _lib.check(self.lib.msda_cls_packed_elems(self.classes, ctypes.byref(n)))
        self.packed = torch.empty(n.value, dtype=torch.int16, device="cuda")
        self.G, self.A = _dev(G.float()), _dev(A.float())
        _lib.check(self.lib.msda_cls_pack(self.G.data_ptr(), self.classes, self.A.data_ptr(), 256, self.packed.data_ptr(), _lib.raw_stream()))

    def __call__(self, x, scale, parts):
        xd = _dev(x)
        assert xd.dtype in (torch.float32, BF) and xd.data_ptr() % 16 == 0
        T = xd.shape[0]
        out = _poisoned(T, torch.float32)
        _lib.check(self.lib.msda_cls_max_scores(xd.data_ptr(), int(xd.dtype == BF), self.packed.data_ptr(), T, 256, self.classes, scale, parts,
                                                out.data_ptr(), _lib.raw_stream()))
        return _result(out, T)


def _cls_ratio(got, ref):
    r = (got.double() - ref["s"]).abs() / ref["bound"]
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max())


@pytest.mark.parametrize("x_dtype,parts", R.CLS_MODES, ids=str)
def test_class_score_within_the_bound(x_dtype, parts):
    """every token of every case: T around 16 (a tile), 48 (a wave), 192 (a workgroup); classes around the 16-row tiles"""
    worst = 0.0
    for T, classes in R.CLS_CASES:
        p = R.make_cls(T, classes, 0, x_dtype)
        ref = R.cls_reference(p["G"], p["A"], p["x"], p["scale"], x_dtype, parts)
        assert torch.isfinite(ref["bound"]).all()
        r = _cls_ratio(_Scorer(p["G"], p["A"])(p["x"], p["scale"], parts), ref)
        assert r <= 1.0, (T, classes, r)
        worst = max(worst, r)
    _say(f"class score bound x={x_dtype} parts={parts}", ratio=worst)


@pytest.mark.parametrize("shape", R.CLS_PROBE_SHAPES, ids=str)
def test_class_score_exact_probes(shape):
    """bit equality: the winner visits every row of every tile, the last partial tile and class classes - 1; every token has another
    winner and norm than its neighbours; the lo part of x alone, then of G alone, decides the winner"""
    T, classes = shape
    for x_dtype in ("f32", "bf16"):
        for lo in (None, "x", "G"):
            if lo == "x" and x_dtype == "bf16":
                continue
            p = R.cls_probe(T, classes, lo, False, 0, x_dtype)
            want, _ = R.cls_probe_expected(p)
            sc = _Scorer(p["G"], p["A"])
            got = sc(p["x"], p["scale"], 2)
            assert torch.equal(got, want), (shape, x_dtype, lo, int((got != want).sum()), torch.nonzero(got != want)[:4].tolist())
            if lo != "G":      # G has no lo part: parts = 1 computes the same
                assert torch.equal(sc(p["x"], p["scale"], 1), want), (shape, x_dtype, lo, "parts=1")


@pytest.mark.parametrize("classes", R.CLS_NEG_CLASSES)
def test_class_score_all_logits_negative(classes):
    """a zero padding row of the last tile (or of the [G; 0; A] layout), or a row of A taken for a class, would win"""
    for x_dtype in ("f32", "bf16"):
        p = R.cls_probe(49, classes, None, True, 0, x_dtype)
        want, logits = R.cls_probe_expected(p)
        assert float(logits.max()) < 0
        got = _Scorer(p["G"], p["A"])(p["x"], p["scale"], 2)
        assert torch.equal(got, want) and bool((got < 0).all()), (classes, x_dtype)
    worst = 0.0
    for x_dtype, parts in R.CLS_MODES:
        p = R.make_cls(193, classes, 0, x_dtype, negative=True)
        ref = R.cls_reference(p["G"], p["A"], p["x"], p["scale"], x_dtype, parts)
        assert float(ref["logits"].max()) < 0 and torch.isfinite(ref["bound"]).all()
        got = _Scorer(p["G"], p["A"])(p["x"], p["scale"], parts)
        r = _cls_ratio(got, ref)
        assert r <= 1.0 and bool((got < 0).all()), (classes, x_dtype, parts, r)
        worst = max(worst, r)
    _say(f"class score all-negative classes={classes}", ratio=worst)


@pytest.mark.parametrize("spread", R.CLS_SPREADS)
def test_class_scorer_against_the_oracle_under_conditioning(spread):
    """ClassScorer (the public entry point) against oracle/cls_oracle.py in float64, Wp's singular values spread over `spread`, every
    eighth token in the smallest singular direction.  Asserted: the bound (which loosens by itself; tokens with rho >= 1 have none) and
    finiteness.  Recorded, not asserted: the error of the kernel and of the reference's own op chain in float32, both against float64"""
    from richsem_amd.two_stage import ClassScorer
    wp, text, x, ls, aligned = R.make_cls_conditioned(spread)
    G64, A64, _, _ = R.scorer_operands(wp, text)
    scale = float(np.exp(np.float64(ls)))
    ref = R.cls_reference(G64, A64, torch.from_numpy(x), scale, "f32", 2, oracle=True)
    want = cls_oracle.max_logits(x.astype(np.float64), wp.astype(np.float64), text.astype(np.float64), np.float64(ls))
    assert np.abs(ref["s"].numpy() - want).max() <= 1e-9 * np.abs(want).max()
    sc = ClassScorer(2).prepare(torch.from_numpy(wp).cuda(), torch.from_numpy(text).cuda(), torch.tensor(float(ls)))
    got = sc.max_logits(torch.from_numpy(x).cuda()).cpu()
    assert torch.isfinite(got).all()
    finite = torch.isfinite(ref["bound"])
    assert spread > 10 or finite.all()
    r = float(((got.double() - torch.from_numpy(want)).abs() / ref["bound"])[finite].max())
    assert r <= 1.0, (spread, r)
    ref32 = cls_oracle.max_logits(x, wp, text, ls)
    rel = lambda v, idx: float(np.abs(np.asarray(v, np.float64) - want)[idx].max() / np.abs(want).max())
    rest = np.setdiff1d(np.arange(len(want)), aligned)
    _say(f"class score conditioning spread={spread}", ratio=r, unbounded=float((~finite).sum()), kernel_aligned=rel(got.numpy(), aligned),
         chain32_aligned=rel(ref32, aligned), kernel_rest=rel(got.numpy(), rest), chain32_rest=rel(ref32, rest))
    assert "librichsem_msda.so" in open("/proc/self/maps").read()


def test_class_score_zero_row_is_nan_and_stays_alone():
    """x = 0: m = 0 and n2 = 0, the score is 0 / 0 = NaN (the reference's f / |f| is NaN as well); the other tokens do not change"""
    for x_dtype in ("f32", "bf16"):
        p = R.make_cls(50, 17, 1, x_dtype)
        sc = _Scorer(p["G"], p["A"])
        base = sc(p["x"], p["scale"], 2)
        x = p["x"].clone()
        zero = [0, 16, 47, 49]
        x[zero] = 0
        got = sc(x, p["scale"], 2)
        keep = torch.ones(50, dtype=torch.bool)
        keep[zero] = False
        assert torch.isnan(got[zero]).all() and torch.equal(got[keep], base[keep]) and torch.isfinite(base).all()


# ===== ROIAlign ===================================================================================================================================
def _roi_run(inp, rois, out_size, scale, ratio, aligned, dtype, N=None, expect=OK):
    """msda_roi_align_forward_* on the test's own buffers -> numpy (K, C, PH, PW)"""
    lib = _lib.load()
    PH, PW = (out_size, out_size) if isinstance(out_size, int) else out_size
    x, r = _dev(inp, TORCH_DT[dtype]), _dev(rois, TORCH_DT[dtype])
    Nn, C, H, W = x.shape
    K = r.shape[0]
    n = K * C * PH * PW
    out = _poisoned(n, TORCH_DT[dtype])
    rc = getattr(lib, "msda_roi_align_forward_" + dtype)(x.data_ptr(), r.data_ptr(), K, N or Nn, C, H, W, PH, PW, float(scale), ratio, int(aligned),
                                                          out.data_ptr(), _lib.raw_stream())
    assert rc == expect, (rc, _lib.last_error())
    return _result(out, n).view(K, C, PH, PW).numpy()


_ROI_REF = {}


def _roi_reference(case, dtype):
    key = (case, dtype)
    if key not in _ROI_REF:
        N, C, H, W, out, scale, ratio, aligned = case
        inp, rois = R.make_roi_case(case)
        sc = R.kernel_scale(scale, dtype)
        cond = R.roi_conditions(rois, out, sc, ratio, aligned, H, W)
        assert cond["int_dist"] >= R.ROI_MARGIN and cond["edge_dist"] >= R.ROI_MARGIN          # the two conditions: asserted, not assumed
        assert 12 * R.E * cond["P"].max() < R.ROI_MARGIN / 2 and cond["gh"].max() <= 8 and cond["gw"].max() <= 8
        want = roi_oracle.roi_align(inp, rois, out, sc, ratio, aligned)
        _ROI_REF[key] = (inp, rois, want, R.roi_bound(inp, rois, cond, dtype))
    return _ROI_REF[key]


@pytest.mark.parametrize("dtype", ("f32", "f64"))
@pytest.mark.parametrize("case", R.ROI_CASES, ids=str)
def test_roi_align_within_the_bound(case, dtype):
    """element-wise, against oracle/roi_oracle.py in float64; boxes that stick out on the top left and the bottom right and a sub-bin box"""
    N, C, H, W, out, scale, ratio, aligned = case
    inp, rois, want, bound = _roi_reference(case, dtype)
    r = R.ratio_np(_roi_run(inp, rois, out, scale, ratio, aligned, dtype), want, bound)
    assert r <= 1.0, (case, dtype, r)
    _say(f"roi bound {case} {dtype}", ratio=r)


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_roi_align_public_entry_point(dtype):
    from richsem_amd.roi import roi_align
    for case in (R.ROI_CASES[1], R.ROI_CASES[2]):
        N, C, H, W, out, scale, ratio, aligned = case
        inp, rois, want, bound = _roi_reference(case, dtype)
        got = roi_align(_dev(inp, TORCH_DT[dtype]), _dev(rois, TORCH_DT[dtype]), out, scale, ratio, aligned)
        assert got.dtype == TORCH_DT[dtype] and R.ratio_np(got.cpu().numpy(), want, bound) <= 1.0
        assert np.array_equal(got.cpu().numpy(), _roi_run(inp, rois, out, scale, ratio, aligned, dtype))
    assert "librichsem_msda.so" in open("/proc/self/maps").read()


def _roi_probe_results(dtype):
    """every dyadic probe group and the cap-free boxes of roi_cap_rois through the kernel: name -> array"""
    H, W, N = 5, 6, 3
    m = R.roi_probe_map(N, 2, H, W)
    res = {}
    for name, out, scale, ratio, aligned, rois, _ in R.roi_probe_groups(H, W, N):
        res[name] = _roi_run(m, rois, out, scale, ratio, aligned, dtype)
    return res


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_roi_align_exact_probes_at_the_discontinuities(dtype):
    """dyadic geometry, integer map: samples at exactly -1 and H (taken), 2^-3 beyond (zero), integer roi / bins (the grid equals it), zero-size
    and inverted boxes (zeros), the legacy clamp, batch indices N - 1, N and -1 -- float32 and float64 equal the float64 restatement bit
    for bit (tests/test_clip_side_ref.py holds the restatement to the oracle and to closed forms)"""
    H, W, N = 5, 6, 3
    m = R.roi_probe_map(N, 2, H, W)
    got = _roi_probe_results(dtype)
    for name, out, scale, ratio, aligned, rois, notes in R.roi_probe_groups(H, W, N):
        want = R.roi_align_ref(m, rois, out, scale, ratio, aligned)
        bad = [notes[i] for i in range(len(rois)) if not np.array_equal(got[name][i].astype(np.float64), want[i])]
        assert not bad, (name, dtype, bad)


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_roi_align_linear_map_closed_form(dtype):
    """f(y, x) = a y + b x + c: a bin whose samples lie inside the map equals f at its centre -- exactly with dyadic data, within the bound else"""
    N, C, H, W, out, scale = 3, 2, 9, 8, 2, 1.0
    for dyadic in (True, False):
        m, co = R.linear_map(N, C, H, W, dyadic)
        rois = R.linear_rois(H, W, N, scale, dyadic)
        want = R.linear_closed_form(co, rois, out, scale, True)
        got = _roi_run(m, rois, out, scale, 0, True, dtype)
        if dyadic:
            assert np.array_equal(got.astype(np.float64), want)
        else:
            cond = R.roi_conditions(rois, out, scale, 0, True, H, W)
            assert cond["int_dist"] >= R.ROI_MARGIN
            # (the kernel is given float32(map) in f32: every map value is off by e |value|, and so is an interpolation of them)
            r = R.ratio_np(got, want, R.roi_bound(m, rois, cond, dtype) + (R.E * np.abs(m).max() if dtype == "f32" else 0))
            assert r <= 1.0, (dtype, r)
            _say(f"roi linear map {dtype}", ratio=r)


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_roi_align_refuses_what_would_not_end(dtype):
    """a box whose adaptive grid is just over the cap on one axis, +inf and NaN coordinates: exact zeros, the other ROIs of the call
    unaffected; a fixed sampling_ratio above the cap is refused on the host"""
    m = R.roi_probe_map(1, 2, 5, 6)
    rois, refused = R.roi_cap_rois()
    got = _roi_run(m, rois, 2, 1.0, 0, True, dtype)
    want = R.roi_align_ref(m, rois, 2, 1.0, 0, True)
    assert not got[refused].any() and not np.isnan(got).any()
    assert np.array_equal(got[~refused].astype(np.float64), want[~refused]) and all(want[i].any() for i in np.flatnonzero(~refused))
    lib = _lib.load()
    x, r, o = _dev(m, TORCH_DT[dtype]), _dev(rois, TORCH_DT[dtype]), _poisoned(8, TORCH_DT[dtype])
    fn = getattr(lib, "msda_roi_align_forward_" + dtype)
    assert fn(x.data_ptr(), r.data_ptr(), 1, 1, 2, 5, 6, 2, 2, 1.0, R.ROI_MAX_GRID + 1, 1, o.data_ptr(), _lib.raw_stream()) == BAD_DIMS
    assert bool(torch.isnan(_result(o, 8)).all())


def test_roi_align_grid_stride_loop():
    """n_out > 65536 * 256: the launch is capped at 65536 workgroups and every thread walks more than one element.  4100 ROIs (41 distinct
    boxes, repeated) x 1024 channels x 2 x 2 bins of ONE sample on a 2 x 2 map; compared on the device"""
    s = R.ROI_STRIDE_CASE
    inp, rois = R.make_roi_stride(s)
    cond = R.roi_conditions(rois, s["out"], 1.0, 1, True, s["H"], s["W"])
    assert cond["edge_dist"] >= R.ROI_MARGIN
    want = torch.from_numpy(R.roi_align_ref(inp, rois, s["out"], 1.0, 1, True)).cuda()
    bound = torch.from_numpy(np.broadcast_to(R.roi_bound(inp, rois, cond, "f32"), want.shape).copy()).cuda()
    lib = _lib.load()
    x = _dev(inp)
    r = _dev(np.tile(rois, (s["repeats"], 1)))
    K = r.shape[0]
    n = K * s["C"] * s["out"] ** 2
    assert n > 65536 * 256
    out = _poisoned(n, torch.float32)
    _lib.check(lib.msda_roi_align_forward_f32(x.data_ptr(), r.data_ptr(), K, 1, s["C"], s["H"], s["W"], s["out"], s["out"], 1.0, 1, 1, out.data_ptr(),
                                              _lib.raw_stream()))
    torch.cuda.synchronize()
    assert bool((out[n:] == SENTINEL).all())
    got = out[:n].view(s["repeats"], s["distinct"], s["C"], s["out"], s["out"])
    ratio = ((got.double() - want[None]).abs() / bound[None])
    assert not bool(torch.isnan(got).any()) and float(ratio.max()) <= 1.0
    assert bool((got == got[:1]).all())      # every repeat of a box gives the same bits
    _say("roi grid stride", ratio=float(ratio.max()))


def roi_record():
    """what tests/golden/roi_align/parent_kernel_r22.npz holds: the kernel's results for the dyadic probes and for every Gaussian case of
    ROI_CASES, recorded on an MI355X from the commit BEFORE the grid cap went into roi_align_fwd_kernel"""
    rec = {}
    for dtype in ("f32", "f64"):
        for name, v in _roi_probe_results(dtype).items():
            rec[f"probe/{name}/{dtype}"] = v
        for i, case in enumerate(R.ROI_CASES):
            N, C, H, W, out, scale, ratio, aligned = case
            inp, rois = R.make_roi_case(case)
            rec[f"case/{i}/{dtype}"] = _roi_run(inp, rois, out, scale, ratio, aligned, dtype)
    return rec


def test_roi_align_is_bit_identical_to_the_kernel_before_the_grid_cap():
    """every box inside the cap: the same bits as the recorded results of the parent commit's kernel (same machine type)"""
    gold = np.load(GOLDEN)
    rec = roi_record()
    assert sorted(gold.files) == sorted(rec)
    for k, v in rec.items():
        assert v.dtype == gold[k].dtype and np.array_equal(v, gold[k]), k


# ===== attention pool core ==========================================================================================================================
def _attn_run(p, case, expect=OK):
    """msda_attnpool_core_* on the test's own buffers -> numpy z (K H, C)"""
    Tn, H, C, K, hm, dtype = case
    lib = _lib.load()
    dt = TORCH_DT[dtype]
    u, feat, pos, spos = (_dev(p[n], dt) for n in ("u", "feat", "pos", "spos"))
    assert u.shape == (K * H, C) and feat.shape == (K, C, Tn) and pos.shape == (Tn + 1, C) and spos.shape == (K * H, Tn + 1)
    z = _poisoned(K * H * C, dt)
    rc = getattr(lib, "msda_attnpool_core_" + dtype)(u.data_ptr(), feat.data_ptr(), pos.data_ptr(), spos.data_ptr(), K, H, C, Tn, hm, z.data_ptr(),
                                                     _lib.raw_stream())
    assert rc == expect, (rc, _lib.last_error())
    return _result(z, K * H * C).view(K * H, C).numpy()


@pytest.mark.parametrize("case", R.ATTN_CASES + R.ATTN_RN50, ids=str)
def test_attention_pool_within_the_bound(case):
    """both HG instantiations, both layouts, both precisions; Tn around the wave size and at the maximum; C < 4 (waves without a channel) and
    C > 256 (the channel loop's second pass); CLIP-RN50's own size"""
    p = R.make_attn(case)
    ref = R.attn_reference(p, case)
    r = R.ratio_np(_attn_run(p, case), ref["z"], ref["bound"])
    assert r <= 1.0, (case, r)
    _say(f"attnpool bound {case}", ratio=r)


@pytest.mark.parametrize("case", R.ATTN_UNIFORM, ids=str)
def test_attention_pool_uniform_weights_probe(case):
    p, want = R.attn_uniform_probe(case)
    got = _attn_run(p, case)
    assert np.array_equal(got.astype(np.float64), want), (case, int((got != want).sum()))


@pytest.mark.parametrize("case", R.ATTN_SELECT, ids=str)
def test_attention_pool_selects_every_token_in_turn(case):
    """spos = -1000 but for one token per (ROI, head): z = f_t + pos_{1 + t} (the mean token: mean_t f + pos_0) bit for bit -- the 1 + t
    offset, the head / ROI row arithmetic of both layouts and the fold over the waves"""
    for shift in (0, 1):
        p, want, sel = R.attn_select_probe(case, shift)
        got = _attn_run(p, case)
        bad = np.flatnonzero((got.astype(np.float64) != want).any(1))
        assert bad.size == 0, (case, shift, bad[:8].tolist())


@pytest.mark.parametrize("case", R.ATTN_SPREAD, ids=str)
def test_attention_pool_large_score_spread(case):
    """scores around +-80 (f32), +-700 (f64): no overflow, z within the bound, and -- with feat = 1, pos = 0, where z is the sum of the
    weights -- the weights sum to 1 within the bound"""
    Tn, H, C, K, hm, dtype = case
    p = R.make_attn(case, spread=80.0 if dtype == "f32" else 700.0)
    ref = R.attn_reference(p, case)
    got = _attn_run(p, case)
    r = R.ratio_np(got, ref["z"], ref["bound"])
    assert np.isfinite(got).all() and r <= 1.0, (case, r)
    ones = dict(p, feat=np.ones_like(p["feat"]), pos=np.zeros_like(p["pos"]), u=np.zeros_like(p["u"]))
    ref1 = R.attn_reference(ones, case)
    assert np.abs(ref1["z"] - 1).max() < 1e-12
    r1 = R.ratio_np(_attn_run(ones, case), ref1["z"], ref1["bound"])
    assert r1 <= 1.0, (case, r1)
    _say(f"attnpool spread {case}", ratio=r, weights_sum=r1)


@pytest.mark.parametrize("dtype", ("f32", "f64"))
def test_attention_pool_module_rests_on_the_bounded_core(dtype):
    """AttentionPool2d (the public entry point): the u, spos it forms go through the C ABI again, that z is within the bound, and the
    module's output is the same bits as its own last two products applied to that z"""
    from richsem_amd.modules import AttentionPool2d
    dt = TORCH_DT[dtype]
    sd, C, H, od, K = 7, 64, 4, 32, 3
    torch.manual_seed(3)
    m = AttentionPool2d(sd, C, H, od).to(dt).cuda().eval()
    x = torch.randn(K, C, sd, sd, dtype=dt, device="cuda")
    out = m(x)
    d = m._derived(dt)
    hd, T = C // H, sd * sd
    x0 = x.flatten(2).mean(dim=2) + d["pos"][0]
    q = torch.addmm(d["bq"], x0, d["wq_t"])
    u = torch.bmm(q.view(K, H, hd).transpose(0, 1), d["wk_h"])
    spos = torch.mm(u.view(H * K, C), d["pos_t"])
    case = (T, H, C, K, 1, dtype)
    p = {"u": u.view(H * K, C).cpu().numpy(), "feat": x.flatten(2).cpu().numpy(), "pos": d["pos"].cpu().numpy(), "spos": spos.cpu().numpy()}
    ref = R.attn_reference(p, case)
    z = _attn_run(p, case)
    r = R.ratio_np(z, ref["z"], ref["bound"])
    assert r <= 1.0, r
    zt = torch.from_numpy(z).cuda().view(H, K, C)
    o = torch.bmm(zt, d["wv_ht"]).transpose(0, 1).reshape(K, C)
    assert torch.equal(out, torch.addmm(d["bc"], o, d["wc_t"]))
    _say(f"attnpool module {dtype}", ratio=r)
    assert "librichsem_msda.so" in open("/proc/self/maps").read()


def test_attention_pool_refusals():
    lib = _lib.load()
    case = (R.ATTN_MAX_T + 1, 4, 4, 1, 1, "f32")
    _attn_run(R.make_attn(case), case, expect=BAD_DIMS)                                  # Tn = 257; the result buffer stays poisoned:
    for dtype in ("f32", "f64"):
        dt = TORCH_DT[dtype]
        fn = getattr(lib, "msda_attnpool_core_" + dtype)
        u, feat, pos, spos = (torch.zeros(64, dtype=dt, device="cuda") for _ in range(4))
        z = _poisoned(16, dt)
        args = [u.data_ptr(), feat.data_ptr(), pos.data_ptr(), spos.data_ptr()]
        assert fn(*args, 0, 4, 4, 3, 1, z.data_ptr(), _lib.raw_stream()) == OK            # K = 0: nothing is written
        assert fn(*args, 1, 4, 4, R.ATTN_MAX_T + 1, 1, z.data_ptr(), _lib.raw_stream()) == BAD_DIMS
        for i in range(4):
            a = list(args)
            a[i] = None
            assert fn(*a, 1, 4, 4, 3, 1, z.data_ptr(), _lib.raw_stream()) == NULL_POINTER
        assert fn(*args, 1, 4, 4, 3, 1, None, _lib.raw_stream()) == NULL_POINTER
        assert bool(torch.isnan(_result(z, 16)).all())
