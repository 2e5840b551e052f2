"""CPU: the attention comparator itself (tests/attention_ref.py) and the mask packing of richsem_amd/functions/attention.py.
The emulation -- fp32 with exactly the kernels' bf16 roundings -- must stay inside every element-wise bound on the shapes the GPU
tests use: that is the check that a correct kernel can meet the bounds of tests/test_gpu_attention.py."""
import math

import pytest
import torch

import attention_ref as R

NQ_SWEEP = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160)
STRUCTURED = [("causal", 129), ("own_block", 129), ("wave0", 129), ("wave1", 129), ("wave2", 129), ("wave3", 129), ("last_key", 129),
              ("first_block_masked", 129), ("first_block_masked", 257)]


def _cases(gen):
    """(name, nq, mask, score scale) of every GPU parity case that does not need the device to build its mask"""
    for nq in NQ_SWEEP:
        yield f"sweep{nq}", nq, None, 1.5
        yield f"sweep{nq}m", nq, R.existing_test_mask(nq, gen), 1.5
    for kind, nq in STRUCTURED:
        yield kind, nq, R.structured_mask(kind, nq), 1.5
    m = R.existing_test_mask(129, gen)
    m[[0, 128, 5, 77]] = True
    m[48:64] = True
    yield "empty_rows", 129, m, 1.5
    yield "large", 129, None, 8.0
    yield "large_m", 129, R.existing_test_mask(129, gen), 8.0
    yield "large_outlier", 129, R.existing_test_mask(129, gen), 8.0


@pytest.mark.parametrize("seed", range(6))
def test_emulation_stays_inside_every_bound(seed):
    gen = torch.Generator().manual_seed(seed)
    worst = {n: 0.0 for n in R.TENSORS}
    for name, nq, mask, scale in _cases(gen):
        q, k, v, do = R.random_inputs(1, 2, nq, gen, scale)
        if name == "large_outlier":
            R.mask_outlier_last_key(q, k, mask)
        val, bound = R.reference(q, k, v, do, mask)
        r = R.ratios(R.emulate(q, k, v, do, mask), val, bound)
        for n in R.TENSORS:
            worst[n] = max(worst[n], r[n])
            assert r[n] <= 1.0, (name, n, r[n])
    print("[emulation] worst |err| / bound:", {n: round(x, 3) for n, x in worst.items()})
    assert worst["out"] > 0.2 and worst["dv"] > 0.2          # (the bounds are not an order of magnitude loose either)


def test_reference_is_the_softmax_definition_where_torch_defines_it():
    gen = torch.Generator().manual_seed(3)
    nq = 70
    q, k, v, do = R.random_inputs(2, 3, nq, gen)
    mask = R.existing_test_mask(nq, gen)
    val, _ = R.reference(q, k, v, do, mask)
    a, b, c = (t.double().requires_grad_(True) for t in (q, k, v))
    s = (a @ b.transpose(-1, -2) / math.sqrt(32)).masked_fill(mask, float("-inf"))
    out = torch.softmax(s, -1) @ c
    out.backward(do.double())
    for n, w in (("out", out.detach()), ("dq", a.grad), ("dk", b.grad), ("dv", c.grad),
                 ("lse2", torch.logsumexp(s.detach(), -1) / math.log(2))):
        assert float((val[n] - w).abs().max()) < 1e-12 * (1 + float(w.abs().max())), n


def test_rows_without_an_allowed_key_are_zero_and_contribute_nothing():
    gen = torch.Generator().manual_seed(4)
    nq = 40
    q, k, v, do = R.random_inputs(1, 2, nq, gen)
    mask = R.existing_test_mask(nq, gen)
    rows = [0, 17, 39]
    mask[rows] = True
    for fn in (lambda *a: R.reference(*a)[0], R.emulate):
        val = fn(q, k, v, do, mask)
        assert all(bool(torch.isfinite(val[n]).all()) for n in ("out", "dq", "dk", "dv"))
        assert bool((val["out"][:, :, rows] == 0).all()) and bool((val["dq"][:, :, rows] == 0).all())
        assert bool((val["lse2"][:, :, rows] == float("inf")).all())
        keep = [i for i in range(nq) if i not in rows]
        assert bool(torch.isfinite(val["lse2"][:, :, keep]).all())
    # the same problem with those rows opened and their dout zeroed: they then contribute nothing to dk / dv by construction
    val = R.reference(q, k, v, do, mask)[0]
    mask2, do2 = mask.clone(), do.clone()
    mask2[rows] = False
    do2[:, :, rows] = 0
    val2 = R.reference(q, k, v, do2, mask2)[0]
    for n in ("dk", "dv"):
        assert float((val[n] - val2[n]).abs().max()) < 1e-13, n


def test_one_flipped_mask_bit_leaves_the_bounds():
    """the sparse masks of the exact probes: any single flipped bit moves `out` far outside its bound"""
    gen = torch.Generator().manual_seed(5)
    nq = 97
    mask, counts = R.sparse_mask(nq, gen)
    assert counts.tolist()[:4] == [1, 2, 4, 8] and not bool(mask[3, 31]) and not bool(mask[3, 32])
    z = torch.zeros(1, 1, nq, 32, dtype=torch.bfloat16)
    v = torch.randint(-8, 9, (1, 1, nq, 32), generator=gen).to(torch.bfloat16)
    do = torch.randint(-2, 3, (1, 1, nq, 32), generator=gen).to(torch.bfloat16)
    val, bound = R.reference(z, z, v, do, mask)
    assert R.ratios(R.emulate(z, z, v, do, mask), val, bound)["out"] == 0.0
    for _ in range(20):
        i, j = (int(x) for x in torch.randint(0, nq, (2,), generator=gen))
        m2 = mask.clone()
        m2[i, j] = ~m2[i, j]
        if bool(m2[i].all()):
            continue                      # (the query's only key: the row becomes empty, lse2 = +inf -- caught as well)
        assert R.ratios(R.emulate(z, z, v, do, m2), val, bound)["out"] > 1.0, (i, j)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 97])
def test_mask_bits_is_the_documented_packing(n):
    """bit j of word (q, kb) = mask[q, 32 kb + j], and the same of the transposed mask (include/richsem_msda.h); bits past n are 0"""
    from richsem_amd.functions import attention as A
    gen = torch.Generator().manual_seed(n)
    mask = torch.rand(n, n, generator=gen) < 0.5
    if n > 31:
        mask[:, 31] = True                # the sign bit of the int32 word
        mask[0, :] = False                # (not symmetric, so the transposed bits differ)
        mask[0, 31] = True
    A._MASK_CACHE.clear()
    bits, bits_t = A.mask_bits(mask)
    A._MASK_CACHE.clear()
    nkb = (n + 31) // 32
    for got, m in ((bits, mask), (bits_t, mask.t())):
        assert got.dtype == torch.int32 and tuple(got.shape) == (n, nkb) and got.is_contiguous()
        word = got.to(torch.int64) & 0xFFFFFFFF
        unpacked = ((word[:, :, None] >> torch.arange(32)) & 1).reshape(n, nkb * 32)
        assert torch.equal(unpacked[:, :n], m.to(torch.int64))
        assert int(unpacked[:, n:].sum()) == 0
    if n > 1:
        assert not torch.equal(bits, bits_t)
