"""No GPU: the bounds of tests/swin_attn_ref.py are attainable and have teeth.  The fp32 emulation of the kernels' roundings stays inside
them; each of five wrong implementations -- shift mask omitted, roll direction reversed, bias index transposed, scale applied to the
bias, padded key columns of a 49-token window left unmasked -- leaves them, on the padded maps of the fixture's layers."""
import pytest
import torch

import swin_attn_ref as R

# (B, Hp, Wp, nH, w): the fixture's layers (13 x 9, 14 x 21 at w = 7; 5 x 20 at w = 12) padded to multiples of the window
SHAPES = ((2, 14, 14, 1, 7), (2, 14, 21, 2, 7), (2, 12, 24, 2, 12))


def _inputs(shape, seed=0):
    B, Hp, Wp, nH, w = shape
    return R.random_inputs(B, Hp, Wp, nH, w, torch.Generator().manual_seed(100 + seed))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("shifted", [False, True])
def test_emulation_stays_inside_the_bounds(shape, shifted):
    B, Hp, Wp, nH, w = shape
    s = w // 2 if shifted else 0
    qkv, table, dout = _inputs(shape)
    val, bound = R.reference(qkv, table, dout, nH, w, s)
    r = R.ratios(R.emulate(qkv, table, dout, nH, w, s), val, bound)
    print(shape, s, r)
    assert all(v <= 1.0 for v in r.values()), r
    assert max(r.values()) > 0.01, "the bounds are orders of magnitude above a correct implementation's error"


def test_emulation_other_shifts_and_single_windows():
    for (B, Hp, Wp, nH, w, s) in ((1, 4, 4, 1, 4, 1), (2, 4, 12, 3, 4, 3), (1, 7, 7, 1, 7, 6), (1, 12, 12, 1, 12, 1), (1, 36, 24, 1, 12, 11)):
        qkv, table, dout = R.random_inputs(B, Hp, Wp, nH, w, torch.Generator().manual_seed(s))
        val, bound = R.reference(qkv, table, dout, nH, w, s)
        r = R.ratios(R.emulate(qkv, table, dout, nH, w, s), val, bound)
        assert all(v <= 1.0 for v in r.values()), ((B, Hp, Wp, nH, w, s), r)


@pytest.mark.parametrize("shape, wrong", [(sh, wr) for sh in SHAPES for wr in R.WRONG
                                          if wr != "pad_keys_unmasked" or (sh[4] * sh[4]) % 16])      # (144 tokens: no padded keys)
def test_wrong_implementations_leave_the_bounds(shape, wrong):
    B, Hp, Wp, nH, w = shape
    s = w // 2
    qkv, table, dout = _inputs(shape, 1)
    val, bound = R.reference(qkv, table, dout, nH, w, s)
    bad, _ = R.reference(qkv, table, dout, nH, w, s, wrong=wrong)
    r = R.ratios(bad, val, bound)
    assert all(v > 1.0 for v in r.values()), (wrong, r)


def test_region_mask_is_the_layers_mask():
    """the closed form of the regions against the slices of the reference's BasicLayer.forward (swin_transformer.py:353-369), restated"""
    for (Hp, Wp, w, s) in ((14, 21, 7, 3), (7, 7, 7, 3), (12, 24, 12, 6), (8, 4, 4, 1), (12, 12, 12, 11)):
        img = torch.zeros(Hp, Wp, dtype=torch.int64)
        cnt = 0
        for hs in (slice(0, -w), slice(-w, -s), slice(-s, None)):
            for ws in (slice(0, -w), slice(-w, -s), slice(-s, None)):
                img[hs, ws] = cnt
                cnt += 1
        assert torch.equal(R.partition(img[None], w, 0)[0], R.regions(Hp, Wp, w, s))


def test_probe_expectation_is_what_the_definition_gives():
    """q = k = 0, +60 at one offset: the float64 definition returns the neighbour's v row where the probe says it must"""
    B, Hp, Wp, nH, w, s = 1, 14, 7, 2, 7, 3
    qkv, _, dout = R.random_inputs(B, Hp, Wp, nH, w, torch.Generator().manual_seed(3))
    qkv = qkv.reshape(B, Hp, Wp, 3, nH * 32).clone()
    qkv[:, :, :, :2] = 0
    qkv = qkv.reshape(B, Hp, Wp, -1)
    for head, di, dj in ((0, 0, 0), (1, 2, -3), (0, -6, 0)):
        table = torch.zeros((2 * w - 1) ** 2, nH)
        table[(di + w - 1) * (2 * w - 1) + dj + w - 1, head] = 60.0
        val, _ = R.reference(qkv, table, dout, nH, w, s)
        valid, rows = R.probe_expectation(qkv[..., 2 * nH * 32:].double(), nH, w, s, head, di, dj)
        got = val["out"].reshape(B, Hp, Wp, nH, 32)[:, :, :, head]
        assert valid.any() and (di == 0 and dj == 0) == bool(valid.all())
        torch.testing.assert_close(got[valid], rows[valid], rtol=0, atol=1e-20)
