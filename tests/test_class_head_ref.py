"""CPU: tests/class_head_ref.py checked against itself and against the reference fixture (tests/golden/cls_head_reference.npz, written by
the reference's own ``CLIPAlign.forward_hs`` and autograd): the float64 restatement in the collapsed form IS the reference's function, dWp
included; the emulation with the kernels' rounding points meets every bound; three wrong implementations do not; the exact probes'
conditions hold and the emulation reproduces them bit for bit.  No GPU."""
import os

import numpy as np
import pytest
import torch

import class_head_ref as H
import clip_side_ref as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cls_head_reference.npz")
CPU_CASES = [(49, 33), (193, 17), (65, 64), (H.SPLIT_ROWS + 1, 17)]


def load_fixture(tag):
    """-> dict of torch tensors: hs (rows, 256), g / logits on cls_idx, full-width g, the gradients"""
    z = np.load(GOLDEN)
    f = {k[len(tag) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(tag + ".")}
    classes = f["text_embed"].shape[0]
    f["x"] = f["hs"].reshape(-1, 256)
    f["x_grad"] = f["hs_grad"].reshape(-1, 256)
    g = torch.zeros(f["x"].shape[0], classes, dtype=f["g"].dtype)
    g[:, f["cls_idx"]] = f["g"].reshape(-1, len(f["cls_idx"]))
    f["g_full"] = g
    f["logits_slice"] = f["logits"].reshape(-1, len(f["cls_idx"]))
    return f


def collapsed(f):
    """float64 G, A, T^ of a fixture"""
    wp, te = f["proj_weight"].double(), f["text_embed"].double()
    te = te / te.norm(dim=-1, keepdim=True)
    return te @ wp, wp.t() @ wp, te


@pytest.mark.parametrize("tag,tol", [("f64", 1e-12), ("f32", 2e-5)])
def test_the_collapsed_restatement_is_the_references_function(tag, tol):
    """relative to the largest magnitude of each tensor: 1e-12 against the float64 fixture, a few fp32 roundings of 1024- and 1204-term sums
    against the float32 one"""
    f = load_fixture(tag)
    G, A, te = collapsed(f)
    scale = float(np.exp(np.float64(f["logit_scale"])))
    ref = H.reference(G, A, f["x"], f["g_full"], scale, oracle=True)
    classes = G.shape[0]
    dwp, _ = H.dwp_reference(ref, f["proj_weight"].double(), te, classes)
    for name, got, want in (("logits", ref["logits"][:, f["cls_idx"]], f["logits_slice"]), ("dx", ref["dx"], f["x_grad"]),
                            ("dWp", dwp, f["proj_weight_grad"])):
        err = float((got - want.double()).abs().max() / want.double().abs().max())
        assert err < tol, (tag, name, err)
    # and against float64 autograd of the un-collapsed formula on the same inputs
    lg, dx, dw = H.float64_autograd(f["proj_weight"], f["text_embed"], float(f["logit_scale"]), f["x"], f["g_full"])
    for name, got, want in (("logits", ref["logits"], lg), ("dx", ref["dx"], dx), ("dWp", dwp, dw)):
        assert float((got - want).abs().max() / want.abs().max()) < 1e-12, name


@pytest.mark.parametrize("x_dtype,parts", H.MODES, ids=str)
def test_the_emulation_meets_every_bound(x_dtype, parts):
    for rows, classes in CPU_CASES:
        p = H.make_head(rows, classes, 0, x_dtype)
        ref = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], x_dtype, parts)
        assert int(ref["excluded"].sum()) == 0 and float(ref["rho"].max()) < 0.5
        em = H.emulate(p["G"], p["A"], p["x"], p["g"], p["scale"], parts)
        for name in ("logits", "n2", "dx", "dGA"):
            assert torch.isfinite(ref["B_" + name]).all()
            r = H.ratio(em[name], ref[name], ref["B_" + name])
            assert r <= 1.0, (rows, classes, name, r)
        # the kernels handed saved values of the test's own
        saved = (ref["logits"].float(), ref["n2"].float())
        ref_s = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], x_dtype, parts, saved=saved)
        em_s = H.emulate(p["G"], p["A"], p["x"], p["g"], p["scale"], parts, saved=saved)
        for name in ("dx", "dGA"):
            r = H.ratio(em_s[name], ref_s[name], ref_s["B_" + name])
            assert r <= 1.0, (rows, classes, name, "saved", r)


def test_at_most_one_percent_of_the_rows_is_excluded():
    """rho >= 1 makes a row's bound infinite: on every case of the GPU test the float64 restatement excludes none (the cap is 1 %)"""
    for rows, classes in H.CASES + H.SPLIT_CASES:
        for x_dtype, parts in H.MODES:
            if classes == 1204 and (x_dtype, parts) != ("f32", 1):
                continue      # (rho depends on A and x, not on the classes: one mode is enough at the large shape)
            p = H.make_head(rows, classes, 0, x_dtype)
            c = C.cls_c(x_dtype, parts)
            x, A = p["x"].double(), p["A"].double()
            n2 = (x * (x @ A.t())).sum(1)
            Q = (x.abs() * (x.abs() @ A.abs().t())).sum(1)
            rho = (c + 258 * H.E * (1 + c)) * Q / n2
            assert float((rho >= 1).double().mean()) <= 0.01 and float(rho.max()) < 0.5, (rows, classes, x_dtype, parts)


def test_the_bounds_are_not_slack():
    """three wrong implementations, each outside the bounds on the test's own inputs"""
    rows, classes = 193, 33
    p = H.make_head(rows, classes, 0, "f32")
    ref = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], "f32", 2)
    # 1. the -(beta / n2) A x term dropped
    wrong = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], "f32", 2, drop_norm_term=True)
    assert H.ratio(wrong["dx"], ref["dx"], ref["B_dx"]) > 1.0
    # 2. the lo parts dropped under parts = 2: logits and dx leave their bounds (n2 need not: its bound is relative to
    #    Q = sum |x_j| |A_jk| |x_k|, some twenty times n2 on Gaussian operands, and 65 536 u-level errors of random sign stay inside);
    #    so do dx and [dG; dA] of the backward alone, on saved values of the test's own (their bounds then carry nothing of n2's)
    em = H.emulate(p["G"], p["A"], p["x"], p["g"], p["scale"], 2, drop_lo=True)
    for name in ("logits", "dx"):
        assert H.ratio(em[name], ref[name], ref["B_" + name]) > 1.0, name
    saved = (ref["logits"].float(), ref["n2"].float())
    ref_s = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], "f32", 2, saved=saved)
    em_s = H.emulate(p["G"], p["A"], p["x"], p["g"], p["scale"], 2, drop_lo=True, saved=saved)
    for name in ("dx", "dGA"):
        assert H.ratio(em_s[name], ref_s[name], ref_s["B_" + name]) > 1.0, name
    # 3. dA without its transpose in dWp
    gen = torch.Generator().manual_seed(3)
    wp = torch.randn(64, 256, generator=gen).double() / 8
    te = torch.randn(classes, 64, generator=gen).double()
    te = te / te.norm(dim=-1, keepdim=True)
    ref = H.reference(te @ wp, wp.t() @ wp, p["x"], p["g"], p["scale"], "f32", 2, oracle=True)
    dwp, bound = H.dwp_reference(ref, wp, te, classes)
    lg, dx, dw = H.float64_autograd(wp, te, float(np.log(p["scale"])), p["x"], p["g"])
    assert H.ratio(dwp, dw, bound) <= 1.0
    wrong, _ = H.dwp_reference(ref, wp, te, classes, transpose=False)
    assert H.ratio(wrong, dw, bound) > 1.0


@pytest.mark.parametrize("shape", H.PROBE_SHAPES, ids=str)
def test_the_exact_probes_are_exact(shape):
    """the conditions (asserted in head_probe_expected, term by term) and the emulation, in fp32 and in whatever order torch sums: equal bits"""
    T, classes = shape
    for x_dtype in ("f32", "bf16"):
        p = H.head_probe(T, classes, x_dtype)
        want = H.head_probe_expected(p)
        if shape == H.PROBE_SHAPES[0]:
            assert want["y_needs_lo"]      # (this probe exercises the lo part of Y: parts = 1 cannot give its dA)
        g = p["g"]
        assert int((g != 0).sum()) == T and bool((g[0, classes - 1] != 0)) and bool((g[T - 1] != 0).any())
        for parts in (2, 1):
            em = H.emulate(p["G"], p["A"], p["x"], g, p["scale"], parts)
            for name in ("logits", "n2", "dx"):
                assert torch.equal(em[name], want[name]), (shape, x_dtype, parts, name)
            assert torch.equal(em["dGA"][:classes], want["dGA"][:classes]), (shape, x_dtype, parts, "dG")
            if parts == 2 or not want["y_needs_lo"]:
                assert torch.equal(em["dGA"][classes:], want["dGA"][classes:]), (shape, x_dtype, "dA")
