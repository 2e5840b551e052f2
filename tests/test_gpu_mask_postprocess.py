"""``PostProcessSegm`` on the GPU (msda_mask_postprocess_*, csrc/mask_terms.hip) against the reference's bytes
(tests/golden/mask_terms/mask_terms_reference.npz) and exact probes."""
import numpy as np
import pytest
import torch

import mask_terms_ref as R
from test_masks_host import POST
from richsem_amd import masks

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def run(pred, max_sizes, orig_sizes, threshold=0.5, items=None, five_dims=True):
    outputs = {"pred_masks": pred[:, :, None] if five_dims else pred}
    if items is not None:
        outputs["item_indices"] = [torch.as_tensor(i, dtype=torch.int64, device="cuda") for i in items]
    results = [{"scores": n} for n in range(pred.shape[0])]
    back = masks.PostProcessSegm(threshold)(results, outputs, torch.as_tensor(orig_sizes, device="cuda"), torch.as_tensor(max_sizes, device="cuda"))
    assert back is results and all(r["scores"] == n for n, r in enumerate(results))
    torch.cuda.synchronize()
    return [r["masks"] for r in results]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("value, want", [(1.0, 1), (-1.0, 0)])
def test_constant_logits(value, want, dtype):
    pred = torch.full((2, 3, 7, 10), value, dtype=DT[dtype], device="cuda")
    for m, (oh, ow) in zip(run(pred, [(28, 33), (40, 60)], [(56, 66), (17, 23)]), [(56, 66), (17, 23)]):
        assert m.dtype == torch.uint8 and m.is_cuda and tuple(m.shape) == (3, 1, oh, ow)
        assert bool((m == want).all())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_positive_source_pixel(dtype):
    """one +8 among -8: the footprint computed in float64 -- the resized logit is a multiple of 1/4 there (x4 weights are multiples of 1/8,
    their products of 1/64, times 16), exact in float32, and never 0 +- the margin"""
    pred = torch.full((1, 2, 9, 13), -8.0, dtype=DT[dtype], device="cuda")
    pred[0, 1, 4, 6] = 8.0
    pred[0, 0, 0, 12] = 8.0      # a corner: the clamps
    sizes = ([(36, 52)], [(75, 101)])
    got = run(pred, *sizes, five_dims=False)[0]
    (want, near), = R.postprocess(pred.double().cpu().numpy(), *sizes, 0.5)
    assert not near.any() and want.sum() > 0
    assert (got.cpu().numpy() == want).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(POST))
def test_fixture_byte_for_byte(name, dtype):
    """the reference's bytes, except where the float64 resized logit lies within 8 * 2^-24 * sum |weight * value| of the threshold's logit:
    those pixels are left out, at most 0.1 % of a case (the reference alone leaves out none on these logits: tests/test_mask_terms_ref.py)"""
    case = POST[name]
    items = np.split(case["items"], np.cumsum(case["item_counts"])[:-1]) if "items" in case else None
    pred = torch.from_numpy(case["pred"]).to("cuda", DT[dtype])      # (bf16-exact values)
    got = run(pred, case["max_sizes"], case["orig_sizes"], float(case["threshold"]), items)
    ref = R.postprocess(case["pred"], case["max_sizes"], case["orig_sizes"], float(case["threshold"]), items)
    left_out = total = 0
    for i, (m, (_, near)) in enumerate(zip(got, ref)):
        want = case[f"out{i}"]
        assert m.dtype == torch.uint8 and tuple(m.shape) == want.shape
        assert ((m.cpu().numpy() == want) | near).all(), (name, i)
        left_out, total = left_out + int(near.sum()), total + near.size
    assert left_out <= 0.001 * total
