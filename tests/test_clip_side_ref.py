"""CPU: the comparators of tests/test_gpu_clip_side_bounds.py checked without a GPU (tests/clip_side_ref.py).
  * fp32 (fp64) emulations of the class score, ROIAlign and the attention-pool core with the kernels' rounding points, and the same with
    every sum in a permuted order, stay inside every element-wise bound on every listed case -- the bounds can be met;
  * every exact probe meets its conditions and goes through the emulations bit for bit, in both orders;
  * the float64 restatement of ROIAlign equals oracle/roi_oracle.py, and the closed forms (linear map, the cut-offs) hold;
  * the case lists cover what they claim to cover.
Worst ratios are printed (pytest -s)."""
import numpy as np
import pytest
import torch

import clip_side_ref as R
from oracle import cls_oracle, roi_oracle


def _gen(seed=1):
    return torch.Generator().manual_seed(seed)


# ---- class score ------------------------------------------------------------------------------------------------------------------------------
def test_case_lists_cover_the_edges():
    assert {T for T, c in R.CLS_CASES if c == 33} == set(R.CLS_T_SWEEP) and {c for T, c in R.CLS_CASES if T == 193} == set(R.CLS_C_SWEEP)
    for axis, want in ((0, (1, 2, 49, 63, 64, 65, 255, 256)), (1, (1, 2, 3, 4, 8, 32)), (2, (1, 3, 4, 5, 64, 257, 260)), (3, (1, 3))):
        assert {c[axis] for c in R.ATTN_CASES} == set(want), axis
    assert {(c[1] % 4 == 0, c[4], c[5]) for c in R.ATTN_CASES} == {(g, hm, d) for g in (False, True) for hm in (0, 1) for d in ("f32", "f64")}
    assert all(c[0] <= R.ATTN_MAX_T for c in R.ATTN_CASES + R.ATTN_SELECT + R.ATTN_UNIFORM + R.ATTN_SPREAD)
    assert {c[1] for c in R.ROI_CASES} == {1, 3} and {c[0] for c in R.ROI_CASES} == {1, 3} and {c[6] for c in R.ROI_CASES} == {0, 2, 3}
    assert {c[4] for c in R.ROI_CASES} == {2, 7, (3, 5)} and {c[7] for c in R.ROI_CASES} == {True, False}
    assert all(c[2] * c[3] <= 13 * 9 and max(c[2], c[3]) <= 13 for c in R.ROI_CASES)
    s = R.ROI_STRIDE_CASE
    assert s["repeats"] * s["distinct"] * s["C"] * s["out"] ** 2 > 65536 * 256


@pytest.mark.parametrize("x_dtype,parts", R.CLS_MODES, ids=str)
def test_class_score_emulation_meets_the_bound(x_dtype, parts):
    worst = 0.0
    for T, classes in R.CLS_CASES:
        for negative in (False, True) if classes in R.CLS_NEG_CLASSES and T == 193 else (False,):
            p = R.make_cls(T, classes, 0, x_dtype, negative)
            ref = R.cls_reference(p["G"], p["A"], p["x"], p["scale"], x_dtype, parts)
            assert torch.isfinite(ref["bound"]).all() and float(ref["rho"].max()) < 0.5
            if negative:
                assert float(ref["logits"].max()) < 0
            for perm in (None, _gen(T)):
                got = R.emulate_cls(p["G"], p["A"], p["x"], p["scale"], parts, perm)
                r = float(((got.double() - ref["s"]).abs() / ref["bound"]).max())
                assert r <= 1.0, (T, classes, negative, perm is not None, r)
                worst = max(worst, r)
    print(f"[emulation] class score x={x_dtype} parts={parts} worst err/bound={worst:.3f}")


def test_class_score_bound_levels():
    """parts = 1 is at u level, the split product at fp32 level, bf16 x has no lo_x term"""
    assert R.cls_c("f32", 2) == R.C_F32 and R.cls_c("bf16", 2) < R.cls_c("f32", 2) < 1e-4
    assert R.U < R.cls_c("bf16", 1) < R.cls_c("f32", 1) < 1.1 * R.U + 1e-4


@pytest.mark.parametrize("shape", R.CLS_PROBE_SHAPES, ids=str)
def test_class_score_probes_are_exact_in_the_emulation(shape):
    T, classes = shape
    for x_dtype in ("f32", "bf16"):
        for lo in (None, "x", "G"):
            if lo == "x" and x_dtype == "bf16":
                continue
            for negative in (False, True):
                p = R.cls_probe(T, classes, lo, negative, 0, x_dtype)
                want, logits = R.cls_probe_expected(p)
                if negative:
                    assert float(logits.max()) < 0
                for perm in (None, _gen(3)):
                    assert torch.equal(R.emulate_cls(p["G"], p["A"], p["x"], p["scale"], 2, perm), want), (shape, x_dtype, lo, negative)
                if lo is not None:      # the lo part alone decides: without it the rival ties at the hi level and the value differs
                    hi_only = R.emulate_cls(p["G"], p["A"], p["x"], p["scale"], 1) if lo == "G" else \
                        R.emulate_cls(p["G"], p["A"], p["x"].to(R.BF).float(), p["scale"], 2)
                    assert not (hi_only == want).any()
    p = R.cls_probe(T, classes)
    if T >= classes:      # every row of every tile, the last partial tile and class classes - 1 win somewhere
        assert set(p["winner"].tolist()) == set(range(classes))
    w, n = p["winner"], p["p"]
    assert all((w[t] != w[t + 1] and n[t] != n[t + 1]) for t in range(T - 1))
    want = R.cls_probe_expected(p)[0]
    assert all(want[t] != want[t + 1] for t in range(T - 1)) and (T < 3 or want[T - 1] != want[T - 2])


def test_class_score_zero_row_is_nan_in_the_emulation_and_the_reference():
    p = R.make_cls(17, 5)
    p["x"][7] = 0
    got = R.emulate_cls(p["G"], p["A"], p["x"], p["scale"])
    assert torch.isnan(got[7]) and torch.isfinite(got[torch.arange(17) != 7]).all()
    with np.errstate(all="ignore"):
        ref = cls_oracle.max_logits(p["x"].numpy().astype(np.float64), np.eye(256), np.eye(5, 256), np.float64(0.0))
    assert np.isnan(ref[7]) and np.isfinite(np.delete(ref, 7)).all()


@pytest.mark.parametrize("spread", R.CLS_SPREADS)
def test_conditioning_against_the_oracle(spread):
    """the bound against the oracle from (Wp, text) loosens by itself; the emulation stays inside wherever the bound is finite"""
    wp, text, x, ls, aligned = R.make_cls_conditioned(spread)
    G64, A64, G, A = R.scorer_operands(wp, text)
    scale = float(np.exp(np.float64(ls)))
    ref = R.cls_reference(G64, A64, torch.from_numpy(x), scale, "f32", 2, oracle=True)
    want = cls_oracle.max_logits(x.astype(np.float64), wp.astype(np.float64), text.astype(np.float64), np.float64(ls))
    assert np.abs(ref["s"].numpy() - want).max() <= 1e-9 * np.abs(want).max()      # the collapsed form IS the oracle's value
    got = R.emulate_cls(G, A, torch.from_numpy(x), float(np.float32(scale)))
    finite = torch.isfinite(ref["bound"])
    r = float(((got.double() - ref["s"]).abs() / ref["bound"])[finite].max())
    print(f"[emulation] conditioning spread={spread} err/bound={r:.3f} unbounded tokens={int((~finite).sum())} rho max={float(ref['rho'].max()):.3g}")
    assert r <= 1.0 and torch.isfinite(got).all()
    if spread <= 10:
        assert finite.all()


# ---- ROIAlign -----------------------------------------------------------------------------------------------------------------------------------
def _roi_check_conditions(cond):
    assert cond["int_dist"] >= R.ROI_MARGIN and cond["edge_dist"] >= R.ROI_MARGIN, (cond["int_dist"], cond["edge_dist"])
    assert 12 * R.E * cond["P"].max() < R.ROI_MARGIN / 2 and cond["gh"].max() <= 8 and cond["gw"].max() <= 8


@pytest.mark.parametrize("case", R.ROI_CASES, ids=str)
def test_roi_restatement_equals_the_oracle_and_the_emulation_meets_the_bound(case):
    N, C, H, W, out, scale, ratio, aligned = case
    inp, rois = R.make_roi_case(case)
    for dtype in ("f32", "f64"):
        sc = R.kernel_scale(scale, dtype)
        cond = R.roi_conditions(rois, out, sc, ratio, aligned, H, W)
        _roi_check_conditions(cond)
        want = R.roi_align_ref(inp, rois, out, sc, ratio, aligned)
        assert np.array_equal(want, roi_oracle.roi_align(inp, rois, out, sc, ratio, aligned))
        bound = R.roi_bound(inp, rois, cond, dtype)
        for reverse in (False, True):
            got = R.roi_align_ref(inp, rois, out, sc, ratio, aligned, R.NP_DT[dtype], reverse)
            r = R.ratio_np(got, want, bound)
            assert r <= 1.0, (case, dtype, reverse, r)
        print(f"[emulation] roi {case} {dtype} err/bound={r:.4f}")


def test_roi_stride_case_conditions():
    s = R.ROI_STRIDE_CASE
    inp, rois = R.make_roi_stride(s)
    cond = R.roi_conditions(rois, s["out"], 1.0, 1, True, s["H"], s["W"])
    assert cond["edge_dist"] >= R.ROI_MARGIN and len(rois) == s["distinct"]
    got = R.roi_align_ref(inp, rois, s["out"], 1.0, 1, True, np.float32)
    assert R.ratio_np(got, R.roi_align_ref(inp, rois, s["out"], 1.0, 1, True), R.roi_bound(inp, rois, cond, "f32")) <= 1.0


def test_roi_probes_are_exact_and_say_what_they_claim():
    H, W, N = 5, 6, 3
    m = R.roi_probe_map(N, 2, H, W)
    for name, out, scale, ratio, aligned, rois, notes in R.roi_probe_groups(H, W, N):
        assert len(notes) == len(rois) and np.array_equal(rois * 8, np.round(rois * 8))
        want = R.roi_align_ref(m, rois, out, scale, ratio, aligned)
        assert np.array_equal(want, R.roi_align_ref(m, rois, out, scale, ratio, aligned, np.float32).astype(np.float64)), name
        assert np.array_equal(want, R.roi_align_ref(m, rois, out, scale, ratio, aligned, np.float32, True).astype(np.float64)), name
        inside = np.array([0 <= r[0] < N for r in rois])
        assert np.array_equal(want[inside], roi_oracle.roi_align(m, rois[inside], out, scale, ratio, aligned)), name
        assert not want[~inside].any()
        if name == "cutoffs":      # closed forms, independent of both restatements: bins are single samples at integer positions
            p = m[0, :, :, :]
            assert np.array_equal(want[0, :, 0, :], p[:, 0, [1, 2]]) and np.array_equal(want[0, :, 1, :], p[:, 0, [1, 2]])       # y = -1 -> row 0
            assert np.array_equal(want[1, :, :, 0], m[1][:, [1, 2], 0]) and np.array_equal(want[1, :, :, 1], m[1][:, [1, 2], 0])
            assert not want[2, :, 0, :].any() and np.array_equal(want[2, :, 1, :], p[:, 0, [1, 2]])                               # -1 - 1/8 -> 0
            assert not want[3, :, :, 0].any() and np.array_equal(want[3, :, :, 1], m[2][:, [1, 2], 0])
            assert np.array_equal(want[4, :, 0, :], p[:, H - 1, [1, 2]]) and np.array_equal(want[4, :, 1, :], p[:, H - 1, [1, 2]])  # y = H -> last row
            assert np.array_equal(want[5, :, :, 1], m[1][:, [1, 2], W - 1])
            assert np.array_equal(want[6, :, 0, :], m[2][:, H - 1, [1, 2]]) and not want[6, :, 1, :].any()                          # H + 1/8 -> 0
            assert np.array_equal(want[7, :, :, 0], p[:, [1, 2], W - 1]) and not want[7, :, :, 1].any()
            alone = R.roi_align_ref(m[N - 1:], np.array([[0, 1.0, 1.0, 3.0, 3.0]]), out, scale, ratio, aligned)[0]
            assert np.array_equal(want[8], alone) and np.array_equal(alone, m[N - 1][:, 1:3, 1:3])                                # batch N - 1: its own image
            assert not want[9].any() and not want[10].any()
        if name == "adaptive":
            geo = [R.roi_geometry(r, out, scale, ratio, aligned) for r in rois]
            assert [(g[4], g[5]) for g in geo] == [(2, 2), (2, 1), (4, 2), (2, 2), (0, 0), (1, 0), (0, 1)]
            assert not want[4:].any() and want[:4].any()
        if name == "legacy":
            geo = [R.roi_geometry(r, out, scale, ratio, aligned) for r in rois]
            assert [(g[4], g[5], float(g[6]), float(g[7])) for g in geo][:3] == [(1, 1, 1.0, 1.0)] * 3 and (geo[3][4], geo[3][5]) == (1, 2)
            assert want[:3].any()


def test_roi_grid_cap_restated():
    rois, refused = R.roi_cap_rois()
    m = R.roi_probe_map(1, 2, 5, 6)
    want = R.roi_align_ref(m, rois, 2, 1.0, 0, True)
    assert [R.roi_geometry(r, 2, 1.0, 0, True) is None for r in rois] == refused.tolist()
    assert not want[refused].any() and all(want[i].any() for i in np.flatnonzero(~refused))


@pytest.mark.parametrize("dyadic", (True, False))
def test_roi_linear_map_closed_form(dyadic):
    N, C, H, W, out, scale = 3, 2, 9, 8, 2, 1.0
    m, co = R.linear_map(N, C, H, W, dyadic)
    rois = R.linear_rois(H, W, N, scale, dyadic)
    cond = R.roi_conditions(rois, out, scale, 0, True, H, W)
    want = R.linear_closed_form(co, rois, out, scale, True)
    got64 = R.roi_align_ref(m, rois, out, scale, 0, True)
    got32 = R.roi_align_ref(m.astype(np.float32), rois, out, scale, 0, True, np.float32)
    if dyadic:
        assert np.array_equal(got64, want) and np.array_equal(got32.astype(np.float64), want)
    else:
        assert cond["int_dist"] >= R.ROI_MARGIN
        assert R.ratio_np(got64, want, R.roi_bound(m, rois, cond, "f64")) <= 1.0
        # (float32(map): every value is off by e |value|, and so is an interpolation of them)
        assert R.ratio_np(got32, want, R.roi_bound(m, rois, cond, "f32") + R.E * np.abs(m).max()) <= 1.0


# ---- attention pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ATTN_CASES + R.ATTN_RN50, ids=str)
def test_attention_pool_emulation_meets_the_bound(case):
    p = R.make_attn(case)
    ref = R.attn_reference(p, case)
    for perm in (None, np.random.default_rng(2)):
        z, a = R.emulate_attn(p, case, perm)
        r = R.ratio_np(z, ref["z"], ref["bound"])
        ra = R.ratio_np(a, ref["a"], ref["ea"])
        assert r <= 1.0 and ra <= 1.0, (case, r, ra)
    print(f"[emulation] attnpool {case} z err/bound={r:.3f} weights={ra:.3f}")


@pytest.mark.parametrize("case", R.ATTN_SPREAD, ids=str)
def test_attention_pool_score_spread(case):
    spread = 80.0 if case[5] == "f32" else 700.0
    p = R.make_attn(case, spread=spread)
    ref = R.attn_reference(p, case)
    z, a = R.emulate_attn(p, case)
    assert np.isfinite(z).all() and R.ratio_np(z, ref["z"], ref["bound"]) <= 1.0 and R.ratio_np(a, ref["a"], ref["ea"]) <= 1.0
    assert (np.abs(a.astype(np.float64).sum(-1) - 1) <= ref["ea"].sum(-1)).all()


@pytest.mark.parametrize("case", R.ATTN_UNIFORM, ids=str)
def test_attention_pool_uniform_probe_is_exact(case):
    p, want = R.attn_uniform_probe(case)
    for perm in (None, np.random.default_rng(4)):
        z, a = R.emulate_attn(p, case, perm)
        assert np.array_equal(z.astype(np.float64), want) and (a == 1.0 / (case[0] + 1)).all()


@pytest.mark.parametrize("case", R.ATTN_SELECT, ids=str)
def test_attention_pool_select_probe_is_exact(case):
    Tn, H, C, K, hm, dtype = case
    p, want, sel = R.attn_select_probe(case)
    assert set(sel.ravel().tolist()) == set(range(Tn + 1))                      # every token in turn, the mean token among them
    assert all(len(set(sel[k, g:g + 4].tolist())) == min(4, H - g, Tn + 1) for k in range(K) for g in range(0, H, 4))      # the heads of a group differ
    assert K == 1 or all((sel[k] != sel[k + 1]).all() for k in range(K - 1))
    for perm in (None, np.random.default_rng(5)):
        z, a = R.emulate_attn(p, case, perm)
        assert np.array_equal(z.astype(np.float64), want)
    assert len({tuple(r) for r in want.tolist()}) == len({(k, int(sel[k, h])) for k in range(K) for h in range(H)})      # a row misplaced is a row wrong
