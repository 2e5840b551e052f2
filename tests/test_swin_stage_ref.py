"""No GPU: tests/swin_stage_ref.py against itself, ON THE SHAPES OF tests/test_gpu_swin_stage.py -- the index helpers are what the formulas
say (and what PatchMerging.forward and a convolution compute), the fp32 emulations stay inside the element-wise bounds, and every wrong
variant leaves them on every shape on which it is a different function.  RICHSEM_REPORT=1 prints the worst ratios
(profiles/r33_swin_stages.md)."""
import os

import pytest
import torch
import torch.nn.functional as F

import swin_stage_ref as S

REPORT = bool(os.environ.get("RICHSEM_REPORT"))
EPS = 1e-5


def _report(tag, res):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3f}" for k, v in res.items()), flush=True)


def _gen(*shape):
    return torch.Generator().manual_seed(sum(shape) + 7 * len(shape))


# ---- the index helpers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, W, C", S.MERGE_SHAPES)
def test_merge_index_is_the_concatenation_order_of_patch_merging(B, H, W, C):
    from richsem_amd import swin
    x = torch.randn(B, H, W, C, generator=_gen(B, H, W, C), dtype=torch.float64)
    idx = S.merge_index(B, H, W, C)
    xp = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    want = torch.cat([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
    assert torch.equal(S.gather(x, idx), want)
    assert int((idx < 0).sum()) == 4 * C * idx.shape[0] - x.numel()
    assert torch.equal(S.scatter(S.gather(x, idx), idx, x.shape), x)      # (asserts the bijection)
    merge = swin.PatchMerging(C).double()
    with torch.no_grad():
        got = merge(x.view(B, H * W, C), H, W)
        assert torch.allclose(got, merge.reduction(merge.norm(want)).view(got.shape), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape, patch", S.PATCH_SHAPES)
def test_patch_rows_reference_is_the_convolution(shape, patch):
    ph, pw = patch
    B, Cin, H, W = shape
    gen = _gen(*shape)
    img = torch.randn(*shape, generator=gen, dtype=torch.float64)
    w, bias = torch.randn(8, Cin, ph, pw, generator=gen, dtype=torch.float64), torch.randn(8, generator=gen, dtype=torch.float64)
    rows = S.patch_rows_reference(img, ph, pw)
    K = Cin * ph * pw
    assert rows.shape[1] % 32 == 0 and rows.shape[1] - K < 32 and not bool(rows[:, K:].any())
    conv = F.conv2d(F.pad(img, (0, (pw - W % pw) % pw, 0, (ph - H % ph) % ph)), w, bias, stride=(ph, pw))
    assert torch.allclose((rows[:, :K] @ w.flatten(1).t() + bias).view(B, conv.shape[2], conv.shape[3], 8).permute(0, 3, 1, 2), conv,
                          rtol=1e-12, atol=1e-12)
    drows = torch.randn(rows.shape, generator=gen, dtype=torch.float64)
    leaf = img.clone().requires_grad_(True)
    (S.patch_rows_reference(leaf, ph, pw) * drows).sum().backward()
    assert torch.equal(S.patch_rows_backward_reference(drows, shape, ph, pw), leaf.grad)


# ---- merging norm ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, H, W, C", S.MERGE_SHAPES)
def test_merge_norm_emulation_is_inside_the_bounds(B, H, W, C):
    x, dy, gamma, beta = S.merge_inputs(B, H, W, C, _gen(B, H, W, C))
    val, bound = S.merge_norm_reference(x, gamma, beta, EPS)
    res = S.ratios(S.merge_norm_emulate(x, gamma, beta, EPS), val, bound)
    _report(f"merge norm {(B, H, W, C)}", res)
    assert sorted(res) == ["mean", "out", "rstd"] and all(r <= 1.0 for r in res.values()), res
    val, bound = S.merge_norm_backward_reference(dy, x, gamma, EPS)
    assert val["dx"].shape == x.shape and bound["dx"].shape == x.shape
    res = S.ratios(S.merge_norm_backward_emulate(dy, x, gamma, EPS), val, bound)
    _report(f"merge norm backward {(B, H, W, C)}", res)
    assert sorted(res) == ["dbeta", "dgamma", "dx"] and all(r <= 1.0 for r in res.values()), res


@pytest.mark.parametrize("wrong", S.MERGE_WRONG)
@pytest.mark.parametrize("B, H, W, C", S.MERGE_SHAPES)
def test_wrong_merge_norm_variants_leave_the_bounds(B, H, W, C, wrong):
    if not S.merge_wrong_applies(wrong, B, H, W, C):
        return      # (the same function on this shape: nothing to tell apart)
    x, _, gamma, beta = S.merge_inputs(B, H, W, C, _gen(B, H, W, C))
    val, bound = S.merge_norm_reference(x, gamma, beta, EPS)
    bad = S.merge_norm_reference(x, gamma, beta, EPS, wrong=wrong)[0]
    assert S.ratios(bad, val, bound)["out"] > 1.0


@pytest.mark.parametrize("wrong", S.MERGE_BWD_WRONG)
@pytest.mark.parametrize("B, H, W, C", S.MERGE_SHAPES)
def test_wrong_merge_norm_backward_variants_leave_the_bounds(B, H, W, C, wrong):
    if not S.merge_wrong_applies(wrong, B, H, W, C):
        return
    x, dy, gamma, _ = S.merge_inputs(B, H, W, C, _gen(B, H, W, C))
    val, bound = S.merge_norm_backward_reference(dy, x, gamma, EPS)
    res = S.ratios(S.merge_norm_backward_reference(dy, x, gamma, EPS, wrong=wrong)[0], val, bound)
    assert res["dgamma" if wrong == "pad_out_of_dgamma" else "dx"] > 1.0, res


def test_every_wrong_merge_variant_applies_to_some_gpu_shape_and_padding_to_most():
    for wrong in S.MERGE_WRONG + S.MERGE_BWD_WRONG:
        assert sum(S.merge_wrong_applies(wrong, *shape) for shape in S.MERGE_SHAPES) >= 4, wrong


# ---- output norm to NCHW ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, HW, C", S.NCHW_SHAPES)
def test_norm_nchw_emulation_is_inside_the_bounds(B, HW, C):
    x, dy, gamma, beta = S.nchw_inputs(B, HW, C, _gen(B, HW, C))
    val, bound = S.norm_nchw_reference(x, gamma, beta, EPS)
    assert val["out"].shape == (B, C, HW)
    assert torch.allclose(val["out"], F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), EPS).transpose(1, 2), rtol=1e-10, atol=1e-10)
    res = S.ratios(S.norm_nchw_emulate(x, gamma, beta, EPS), val, bound)
    _report(f"norm nchw {(B, HW, C)}", res)
    assert sorted(res) == ["mean", "out", "rstd"] and all(r <= 1.0 for r in res.values()), res
    val, bound = S.norm_nchw_backward_reference(dy, x, gamma, EPS)
    res = S.ratios(S.norm_nchw_backward_emulate(dy, x, gamma, EPS), val, bound)
    _report(f"norm nchw backward {(B, HW, C)}", res)
    assert sorted(res) == ["dbeta", "dgamma", "dx"] and all(r <= 1.0 for r in res.values()), res


def test_norm_nchw_backward_reference_is_autograd_through_the_transposed_layernorm():
    B, HW, C = 2, 35, 64
    x, dy, gamma, _ = S.nchw_inputs(B, HW, C, _gen(B, HW, C))
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xd, (C,), gd, bd, EPS).transpose(1, 2).backward(dy.double())
    val, _ = S.norm_nchw_backward_reference(dy, x, gamma, EPS)
    for got, want in ((val["dx"], xd.grad), (val["dgamma"], gd.grad), (val["dbeta"], bd.grad)):
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("wrong", S.NCHW_WRONG)
@pytest.mark.parametrize("B, HW, C", S.NCHW_SHAPES)
def test_wrong_norm_nchw_variants_leave_the_bounds(B, HW, C, wrong):
    if not S.nchw_wrong_applies(wrong, B, HW, C):
        return
    x, _, gamma, beta = S.nchw_inputs(B, HW, C, _gen(B, HW, C))
    val, bound = S.norm_nchw_reference(x, gamma, beta, EPS)
    assert S.ratios(S.norm_nchw_reference(x, gamma, beta, EPS, wrong=wrong)[0], val, bound)["out"] > 1.0


@pytest.mark.parametrize("wrong", S.NCHW_BWD_WRONG)
@pytest.mark.parametrize("B, HW, C", S.NCHW_SHAPES)
def test_wrong_norm_nchw_backward_variants_leave_the_bounds(B, HW, C, wrong):
    if not S.nchw_wrong_applies(wrong, B, HW, C):
        return
    x, dy, gamma, _ = S.nchw_inputs(B, HW, C, _gen(B, HW, C))
    val, bound = S.norm_nchw_backward_reference(dy, x, gamma, EPS)
    res = S.ratios(S.norm_nchw_backward_reference(dy, x, gamma, EPS, wrong=wrong)[0], val, bound)
    assert res["dbeta" if wrong == "dbeta_over_channels" else "dx"] > 1.0, res


# ---- the exact probe -------------------------------------------------------------------------------------------------------------------
def test_sign_probe_rows_have_mean_zero_and_variance_one_exactly():
    gen = torch.Generator().manual_seed(1)
    x = S.sign_probe((2, 4, 6, 32), gen)
    rows = S.gather(x.float(), S.merge_index(2, 4, 6, 32))
    assert not bool(rows.sum(1).any()) and bool((rows.pow(2).sum(1) == 128).all())
    emu = S.merge_norm_emulate(x, torch.full((128,), 1.5), torch.full((128,), 0.25), 0.0)
    assert torch.equal(emu["out"], (rows * 1.5 + 0.25).to(S.BF).float())
