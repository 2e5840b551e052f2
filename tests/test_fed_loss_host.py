"""CPU: the federated loss's host side (richsem_amd/fed_loss.py; ABI v9) -- the three entry points refuse bad arguments before any launch,
and the class weights are the reference's ``SetCriterion.set_cats`` weights (richsem.py:930-936)."""
import ctypes

import pytest
import torch

from richsem_amd import _lib
from richsem_amd.fed_loss import FedClassSampler, class_weights_from_image_counts


def test_fed_entry_points_check_their_arguments_on_the_host():
    L = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    n = ctypes.c_int(0)

    def sampler(labels=p, n_labels=4, weight=p, uniform=p, groups=13, C=1204, k=50, mask=p, n_chosen=p):
        return L.msda_fed_class_mask_f32(labels, n_labels, weight, uniform, groups, C, k, mask, n_chosen, None)

    for kw in ({"labels": None}, {"weight": None}, {"uniform": None}, {"mask": None}, {"n_chosen": None}):
        assert sampler(**kw) == -1, kw                                                   # MSDA_ERR_NULL_POINTER
    for kw in ({"C": 0}, {"C": 4097}, {"groups": 0}, {"k": -1}, {"n_labels": -1}):
        assert sampler(**kw) == -2, kw                                                   # MSDA_ERR_BAD_DIMS
    with pytest.raises(RuntimeError, match="msda_fed_class_mask_f32.*BAD_DIMS"):
        _lib.check(sampler(C=5000))

    def neg_sum(logits=p, w=p, grp=p, mask=p, groups=13, rows=8, C=1204, partial=p, max_partial=4096, n_partial=ctypes.byref(n)):
        return L.msda_focal_neg_sum_masked_f32(logits, w, grp, mask, groups, rows, C, 0.25, partial, max_partial, n_partial, None)

    def neg_grad(logits=p, w=p, grp=p, mask=p, groups=13, rows=8, C=1204, gscale=p, gx=p):
        return L.msda_focal_neg_grad_masked_f32(logits, w, grp, mask, groups, rows, C, 0.25, gscale, gx, None)

    for kw in ({"logits": None}, {"w": None}, {"grp": None}, {"mask": None}, {"partial": None}, {"n_partial": None}):
        assert neg_sum(**kw) == -1, kw
    for kw in ({"rows": 0}, {"C": 0}, {"groups": 0}, {"max_partial": 0}):
        assert neg_sum(**kw) == -2, kw
    for kw in ({"logits": None}, {"w": None}, {"grp": None}, {"mask": None}, {"gscale": None}, {"gx": None}):
        assert neg_grad(**kw) == -1, kw
    for kw in ({"rows": 0}, {"C": 0}, {"groups": 0}):
        assert neg_grad(**kw) == -2, kw
    with pytest.raises(RuntimeError, match="msda_focal_neg_grad_masked_f32.*NULL_POINTER"):
        _lib.check(neg_grad(gx=None))


def test_class_weights_are_the_reference_set_cats_weights():
    # set_cats (richsem.py:930-936), by hand: cats = {1: 4 images, 3: 9, 4: 2} -> max_cid = 4 ->
    # fed_weight = [0, 4, 0, 9, 2] ** 0.5 = [0, 2, 0, 3, sqrt 2]: ids without a category weigh 0
    cats = {1: {"id": 1, "image_count": 4}, 3: {"id": 3, "image_count": 9}, 4: {"id": 4, "image_count": 2}}
    want = torch.tensor([0.0, 2.0, 0.0, 3.0, 2.0 ** 0.5, 0.0])
    for counts in (cats, {1: 4, 3: 9, 4: 2}, torch.tensor([0, 4, 0, 9, 2]), [0, 4, 0, 9, 2, 0]):
        w = class_weights_from_image_counts(counts, 6)
        assert w.dtype == torch.float32 and w.shape == (6,)
        assert torch.equal(w, want.float()), (counts, w)
    assert torch.equal(class_weights_from_image_counts({1: 16}, 3, power=0.25), torch.tensor([0.0, 2.0, 0.0]))
    with pytest.raises(ValueError):
        class_weights_from_image_counts({7: 1}, 6)
    with pytest.raises(ValueError):
        class_weights_from_image_counts(torch.ones(7), 6)


def test_sampler_refuses_what_the_kernel_cannot_take():
    with pytest.raises(ValueError):
        FedClassSampler(50)                                     # uniform weights need a class count
    with pytest.raises(ValueError):
        FedClassSampler(50, torch.ones(4097))
    with pytest.raises(ValueError):
        FedClassSampler(-1, torch.ones(8))
    s = FedClassSampler(50, num_classes=1204)
    assert s.num_classes == 1204 and torch.equal(s.class_weight, torch.ones(1204))
    with pytest.raises(RuntimeError, match="CPU"):
        s.sample(torch.tensor([1, 2]), 13)
