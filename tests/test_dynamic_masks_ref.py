"""The float64 restatement of the dynamic mask head (tests/dynamic_masks_ref.py) against the reference's numbers
(tests/golden/dynamic_masks/dynamic_masks_reference.npz), its wrong variants against its own bounds, the ReLU margin of every test input, and the
closed form of ``aligned_bilinear`` against ``F.interpolate``.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dynamic_masks_ref as R

DYN, BRANCH = R.load_golden()
OUTPUTS = ("out", "g_feats", "g_params", "g_ref")


def synthetic_cases():
    """the GPU suite's synthetic shapes (tests/test_gpu_dynamic_masks.py builds the same ones from the same seeds)"""
    import test_gpu_dynamic_masks as G
    return G.SYNTHETIC


@pytest.mark.parametrize("name", list(DYN))
def test_restatement_matches_the_reference(name):
    case, mine = DYN[name], R.dynamic_masks(DYN[name])
    for k in OUTPUTS:
        assert np.abs(mine[k] - case[k]).max() <= 1e-12 * max(1.0, np.abs(case[k]).max()), k
    dead = case["inst"] < 0
    assert not mine["out"][dead].any() and not case["out"][dead].any()


def test_the_fixture_holds_the_cases_the_head_needs():
    assert {int(c["feats"].shape[1]) for c in DYN.values()} == {8, 16} and {int(c["rel"]) for c in DYN.values()} == {0, 1}
    assert {tuple(c["feats"].shape[-2:]) for c in DYN.values()} >= {(1, 1), (3, 4), (5, 7), (9, 13)}
    full = DYN["c8_rel_empty_and_full"]["inst"]
    assert (full[0] < 0).all() and sorted(full[1].tolist()) == [0, 1, 2]
    assert (DYN["c16_rel_no_instance"]["inst"] < 0).all() and not DYN["c16_rel_no_instance"]["out"].any()
    assert {int(c["params"].shape[-1]) for c in DYN.values()} == {153, 169, 217, 233}
    assert set(BRANCH) == {"branch_train", "branch_eval"}


@pytest.mark.parametrize("variant", R.WRONG)
def test_wrong_variants_leave_the_bounds(variant):
    """every wrong variant is outside the fp32 bound of the forward output on every case -- or the case is named in R.SAME, and there it is the
    same function"""
    told_apart = 0
    for name, case in DYN.items():
        right, wrong = R.dynamic_masks(case, grads=False), R.dynamic_masks(case, variant=variant, grads=False)
        if R.is_same(variant, case):
            assert np.abs(wrong["out"] - right["out"]).max() <= 1e-12 * max(1.0, np.abs(right["out"]).max()), (variant, name)
        else:
            assert (np.abs(wrong["out"] - right["out"]) > right["b_out"]).any(), (variant, name)
            bf = R.dynamic_masks(case, out_dtype="bf16", grads=False)
            assert (np.abs(wrong["out"] - right["out"]) > bf["b_out"]).any(), (variant, name, "bf16")
            told_apart += 1
    assert told_apart >= 2, variant


def test_the_bounds_are_tight_enough_to_mean_something():
    """the fp32 bound of an output is a few thousand round-offs of the largest magnitude at the most, never a tolerance in disguise"""
    for name, case in DYN.items():
        res = R.dynamic_masks(case)
        for k in OUTPUTS:
            if np.abs(res[k]).max() > 0:
                assert res["b_" + k].max() <= 4096 * R.E * max(np.abs(res[k]).max(), 1.0), (name, k, res["b_" + k].max())


def test_relu_margin_of_every_input():
    """every pre-activation of every live row and pixel of every case the GPU suite runs is further than MARGIN forward bounds from zero: a
    condition on the inputs, with no element left out (R.dynamic_masks takes the minimum over all of them)"""
    cases = dict(DYN, **synthetic_cases())
    assert len(cases) > len(DYN)
    for name, case in cases.items():
        assert R.dynamic_masks(case, grads=False)["margin"] > R.MARGIN, name


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (4, 1), (3, 4), (9, 13)])
def test_closed_form_of_aligned_bilinear(hw):
    """U t U^T against the reference's construction: replicate pad, bilinear interpolate with align_corners=True, replicate pad, crop"""
    t = torch.randn(2, 3, *hw, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    h, w = hw
    x = F.pad(t, pad=(0, 1, 0, 1), mode="replicate")
    x = F.interpolate(x, size=(2 * h + 1, 2 * w + 1), mode="bilinear", align_corners=True)
    x = F.pad(x, pad=(1, 0, 1, 0), mode="replicate")[:, :, :2 * h, :2 * w]
    mine = np.einsum("ah,nchw,bw->ncab", R.up_matrix(h, 2), t.numpy(), R.up_matrix(w, 2))
    assert np.abs(mine - x.numpy()).max() <= 1e-14 * max(1.0, float(t.abs().max()))
    from richsem_amd import cond_inst
    assert np.abs(cond_inst.aligned_bilinear(t, 2).numpy() - x.numpy()).max() <= 1e-14 * max(1.0, float(t.abs().max()))
    assert cond_inst.aligned_bilinear(t, 1) is t
