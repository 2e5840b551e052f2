"""The float64 restatement of the mask terms (tests/mask_terms_ref.py) against the reference's own numbers
(tests/golden/mask_terms/mask_terms_reference.npz), and every wrong variant against the bounds the GPU tests use, on the GPU tests' own shapes."""
import numpy as np
import pytest

import mask_terms_ref as R

LOSS, POST = R.load_golden()


@pytest.mark.parametrize("name", list(LOSS))
def test_restatement_equals_the_fixture(name):
    case = LOSS[name]
    r = R.mask_terms(case)
    assert abs(r["loss_mask"] - float(case["loss_mask"])) <= 1e-12 * max(1.0, abs(r["loss_mask"]))
    assert abs(r["loss_dice"] - float(case["loss_dice"])) <= 1e-12 * max(1.0, abs(r["loss_dice"]))
    assert np.abs(r["grad"] - case["grad"]).max() <= 1e-12 * max(1.0, np.abs(case["grad"]).max())
    assert tuple(case["canvas"]) == (R.round_up(case["mask_hw"][:, 0].max()), R.round_up(case["mask_hw"][:, 1].max()))


@pytest.mark.parametrize("name", list(POST))
def test_postprocess_restatement_equals_the_fixture_and_leaves_nothing_out(name):
    """on these logits no pixel lies so close to the threshold that float32 could decide it either way: the cap of the GPU test (0.1 %) is
    not used up by the reference itself"""
    case = POST[name]
    items = None
    if "items" in case:
        items = np.split(case["items"], np.cumsum(case["item_counts"])[:-1])
    res = R.postprocess(case["pred"], case["max_sizes"], case["orig_sizes"], float(case["threshold"]), items)
    for i, (mask, near) in enumerate(res):
        assert mask.shape == case[f"out{i}"].shape
        assert (mask == case[f"out{i}"]).all()
        assert not near.any()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("wrong", R.LOSS_WRONG)
def test_wrong_variants_leave_the_bounds(wrong, dtype):
    for name, case in LOSS.items():
        right = R.mask_terms(case, out_dtype=dtype)
        other = R.mask_terms(case, wrong=wrong)
        if name in R.SAME[wrong]:
            assert abs(other["loss_mask"] - right["loss_mask"]) <= 1e-12 and abs(other["loss_dice"] - right["loss_dice"]) <= 1e-12
            assert np.abs(other["grad"] - right["grad"]).max() <= 1e-12
        else:
            assert R.leaves_bounds(right, other), (wrong, name)


def test_the_right_function_stays_inside_its_bounds():
    for case in LOSS.values():
        right = R.mask_terms(case)
        assert not R.leaves_bounds(right, right)
        assert (right["b_grad"] > 0).all() and right["b_loss_mask"] > 0 and right["b_loss_dice"] > 0


def _post_all(case, wrong=None):
    items = np.split(case["items"], np.cumsum(case["item_counts"])[:-1]) if "items" in case else None
    return [m for m, _ in R.postprocess(case["pred"], case["max_sizes"], case["orig_sizes"], float(case["threshold"]), items, wrong)]


@pytest.mark.parametrize("wrong", ["round_to_nearest", "crop_after_resize"])
def test_wrong_postprocess_variants_differ_from_the_fixture(wrong):
    differ = 0
    for name, case in POST.items():
        for i, m in enumerate(_post_all(case, wrong)):
            differ += int((m != case[f"out{i}"]).sum())
    assert differ > 0
    case = POST["p9x13"]      # both rules differ on the case with a crop and a down-sized original
    assert any((m != case[f"out{i}"]).any() for i, m in enumerate(_post_all(case, wrong)))


def test_greater_equal_differs_on_the_threshold_itself():
    """sigmoid(0) is 0.5 exactly: ``>`` gives zeros, ``>=`` ones"""
    pred = np.zeros((1, 2, 3, 3))
    (right, _), = R.postprocess(pred, [(12, 12)], [(7, 9)], 0.5)
    (other, _), = R.postprocess(pred, [(12, 12)], [(7, 9)], 0.5, wrong="greater_equal")
    assert not right.any() and other.all()
