"""GPU (-m gpu): the Swin window-attention kernels (richsem_amd/csrc/swin_attn_mfma.hip) against the float64 restatement, the ELEMENT-WISE
bounds and the EXACT PROBE of tests/swin_attn_ref.py (derivations in its docstring; tests/test_swin_attn_ref.py shows that a correct
implementation meets them and five wrong ones do not).  The kernels go through the C ABI with ctypes on buffers of the test's own: every
result buffer is NaN-poisoned and has a sentinel in front of and behind it that must be untouched after the call -- a padded query row
(49 -> 64, 16 -> 16, 144 -> 144 tokens) has no place to appear.  An excess over a derived bound is a bug in the kernel or in the
derivation, not a reason to widen it.  RICHSEM_REPORT=1 prints the worst |err| / bound per case.

No test here captures a graph ("Swin window attention": capture is untested)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import swin_attn_ref as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
SENTINEL = -12345.0
GUARD = 64

WINDOWS = (4, 7, 12)                  # one exact 16-token tile; 49 -> 64 padding; nine tiles
MAPS = ((1, 1), (1, 3), (3, 2))       # windows per column, per row: a single window in a direction wraps the region ids


def _shifts(w):
    return sorted({0, 1, w // 2, w - 1})


def _poisoned(n, dtype):
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
    buf[:GUARD] = SENTINEL
    buf[GUARD + n:] = SENTINEL
    return buf


def _result(buf, shape):
    n = int(np.prod(shape))
    torch.cuda.synchronize()
    guard = torch.tensor(SENTINEL).to(buf.dtype)
    assert bool((buf[:GUARD] == guard).all()) and bool((buf[GUARD + n:] == guard).all()), "stored outside the result"
    return buf[GUARD:GUARD + n].view(*shape)


class _Kernels:
    def __init__(self):
        from richsem_amd import _lib
        self._lib, self.lib = _lib, _lib.load()

    def forward(self, qkv, table, nH, w, s):
        B, Hp, Wp, C3 = qkv.shape
        C = C3 // 3
        out, lse = _poisoned(B * Hp * Wp * C, BF), _poisoned(B * Hp * Wp * nH, torch.float32)
        self._lib.check(self.lib.msda_swin_attn_forward_bf16(qkv.data_ptr(), table.data_ptr(), B, Hp, Wp, C, nH, w, s, out[GUARD:].data_ptr(),
                                                             lse[GUARD:].data_ptr(), self._lib.raw_stream()))
        return _result(out, (B, Hp, Wp, C)), _result(lse, (B, Hp, Wp, nH))

    def backward(self, qkv, table, out, lse, dout, nH, w, s):
        B, Hp, Wp, C3 = qkv.shape
        C = C3 // 3
        n = ctypes.c_int64(0)
        self._lib.check(self.lib.msda_swin_attn_workspace_bytes(B, Hp, Wp, C, nH, w, ctypes.byref(n)))
        assert n.value == B * (Hp // w) * (Wp // w) * nH * (2 * w - 1) ** 2 * 4
        ws, dqkv, dtable = _poisoned(n.value // 4, torch.float32), _poisoned(qkv.numel(), BF), _poisoned(table.numel(), torch.float32)
        self._lib.check(self.lib.msda_swin_attn_backward_bf16(qkv.data_ptr(), table.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), B,
                                                              Hp, Wp, C, nH, w, s, dqkv[GUARD:].data_ptr(), dtable[GUARD:].data_ptr(),
                                                              ws[GUARD:].data_ptr(), self._lib.raw_stream()))
        _result(ws, (n.value // 4,))
        return _result(dqkv, tuple(qkv.shape)), _result(dtable, tuple(table.shape))

    def run(self, qkv, table, dout, nH, w, s):
        qkv, table, dout = qkv.cuda().contiguous(), table.float().cuda().contiguous(), dout.cuda().contiguous()
        out, lse = self.forward(qkv, table, nH, w, s)
        dqkv, dtable = self.backward(qkv, table, out.contiguous(), lse.contiguous(), dout, nH, w, s)
        return {"out": out, "dqkv": dqkv, "dtable": dtable, "lse": lse}


@pytest.fixture(scope="module")
def kern():
    return _Kernels()


@pytest.mark.parametrize("w", WINDOWS)
@pytest.mark.parametrize("wins", MAPS)
def test_kernels_stay_inside_the_elementwise_bounds(kern, w, wins):
    gen = torch.Generator().manual_seed(1000 * w + 10 * wins[0] + wins[1])
    Hp, Wp = wins[0] * w, wins[1] * w
    worst = {n: 0.0 for n in R.TENSORS}
    for s in _shifts(w):
        for nH in (1, 3):
            for B in (1, 2):
                qkv, table, dout = R.random_inputs(B, Hp, Wp, nH, w, gen)
                val, bound = R.reference(qkv, table, dout, nH, w, s)
                got = kern.run(qkv, table, dout, nH, w, s)
                r = R.ratios(got, val, bound)
                for n in R.TENSORS:
                    worst[n] = max(worst[n], r[n])
                assert all(v <= 1.0 for v in r.values()), ((B, Hp, Wp, nH, w, s), r)
                lse_want = torch.logsumexp(_scores(qkv, table, nH, w, s), -1)
                torch.testing.assert_close(got["lse"].double().cpu(), lse_want, rtol=2.0 ** -20, atol=1.5 * R.F)
    if REPORT:
        print(f"[measured] w={w} windows={wins} " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()), flush=True)


def _scores(qkv, table, nH, w, s):
    """the score rows in float64, merged back to (B, Hp, Wp, nH, N): what lse sums over"""
    B, Hp, Wp, _ = qkv.shape
    parts = R.partition(qkv.double().reshape(B, Hp, Wp, 3, nH, 32), w, s).permute(3, 0, 1, 4, 2, 5)
    score = parts[0] @ parts[1].transpose(-1, -2) * R.C + table.double()[R.bias_pairs(w)].permute(2, 0, 1)
    if s:
        reg = R.regions(Hp, Wp, w, s)
        score = score + ((reg[:, :, None] != reg[:, None, :]).double() * -100.0)[None, :, None]
    return R.merge(score.permute(0, 1, 3, 2, 4), Hp, Wp, w, s)      # (B, nW, N, nH, N) -> (B, Hp, Wp, nH, N)


@pytest.mark.parametrize("w, wins, s", [(4, (1, 1), 1), (4, (3, 2), 3), (7, (1, 3), 3), (7, (3, 2), 6), (12, (1, 1), 6), (12, (3, 2), 1), (7, (3, 2), 0)])
def test_exact_probe_pins_roll_partition_and_bias_index(kern, w, wins, s):
    """q = k = 0, table = +60 at one offset of one head: a query whose neighbour at that offset lies in its window and region returns
    that neighbour's v row bit for bit (every other key weighs e^-60: below half an ulp of the fp32 sum, v kept away from zero)"""
    gen = torch.Generator().manual_seed(7 * w + s)
    B, nH, Hp, Wp = 2, 3, wins[0] * w, wins[1] * w
    qkv, _, dout = R.random_inputs(B, Hp, Wp, nH, w, gen)
    qkv = qkv.reshape(B, Hp, Wp, 3, nH * 32).clone()
    qkv[:, :, :, :2] = 0
    v = qkv[:, :, :, 2].float()
    qkv[:, :, :, 2] = torch.where(v.abs() < 2.0 ** -6, torch.full_like(v, 2.0 ** -6), v).to(BF)
    qkv = qkv.reshape(B, Hp, Wp, -1)
    for head, di, dj in ((0, 0, 0), (1, w - 1, -(w - 1)), (2, -1, 0), (1, 0, 1), (0, -(w // 2), w // 2)):
        table = torch.zeros((2 * w - 1) ** 2, nH)
        table[(di + w - 1) * (2 * w - 1) + dj + w - 1, head] = 60.0
        out, _ = kern.forward(qkv.cuda(), table.cuda(), nH, w, s)
        valid, rows = R.probe_expectation(qkv[..., 2 * nH * 32:], nH, w, s, head, di, dj)
        got = out.cpu().reshape(B, Hp, Wp, nH, 32)[:, :, :, head]
        if (di, dj) == (0, 0):
            assert bool(valid.all())
        assert torch.equal(got[valid].view(torch.int16), rows[valid].view(torch.int16)), (head, di, dj, int(valid.sum()))


def test_zero_dout_gives_exactly_zero_gradients(kern):
    gen = torch.Generator().manual_seed(11)
    for (B, Hp, Wp, nH, w, s) in ((2, 14, 21, 3, 7, 3), (1, 12, 24, 1, 12, 6), (1, 4, 4, 1, 4, 0)):
        qkv, table, dout = R.random_inputs(B, Hp, Wp, nH, w, gen)
        got = kern.run(qkv, table, torch.zeros_like(dout), nH, w, s)
        assert int((got["dqkv"].view(torch.int16) & 0x7FFF).abs().max()) == 0 and int((got["dtable"].view(torch.int32) & 0x7FFFFFFF).max()) == 0


def test_backward_is_bitwise_reproducible(kern):
    gen = torch.Generator().manual_seed(12)
    for (B, Hp, Wp, nH, w, s) in ((2, 21, 14, 3, 7, 3), (2, 36, 24, 2, 12, 6)):
        qkv, table, dout = (t.cuda() for t in R.random_inputs(B, Hp, Wp, nH, w, gen))
        out, lse = kern.forward(qkv, table, nH, w, s)
        out, lse = out.contiguous(), lse.contiguous()
        first = kern.backward(qkv, table, out, lse, dout, nH, w, s)
        first = [t.clone() for t in first]
        for _ in range(3):
            again = kern.backward(qkv, table, out, lse, dout, nH, w, s)
            assert torch.equal(first[0].view(torch.int16), again[0].view(torch.int16))
            assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))


def test_autograd_function_returns_the_kernels_results(kern):
    from richsem_amd import swin
    gen = torch.Generator().manual_seed(13)
    B, Hp, Wp, nH, w, s = 2, 14, 21, 2, 7, 3
    qkv, table, dout = (t.cuda() for t in R.random_inputs(B, Hp, Wp, nH, w, gen))
    want = kern.run(qkv, table, dout, nH, w, s)
    q, t = qkv.clone().requires_grad_(True), table.clone().requires_grad_(True)
    out = swin.window_attention(q, t, nH, w, s)
    out.backward(dout)
    assert torch.equal(out.view(torch.int16), want["out"].view(torch.int16))
    assert torch.equal(q.grad.view(torch.int16), want["dqkv"].view(torch.int16)) and torch.equal(t.grad, want["dtable"])


def test_error_paths_through_the_abi():
    from richsem_amd import swin

    def call(Hp, Wp, C3, nH, w, s=0, dtype=BF, contiguous=True):
        qkv = torch.zeros(1, Hp, Wp, C3, dtype=dtype, device="cuda")
        if not contiguous:
            qkv = qkv.transpose(1, 2)
        return swin.window_attention(qkv, torch.zeros((2 * w - 1) ** 2, nH, device="cuda"), nH, w, s)

    with pytest.raises(RuntimeError, match="msda_swin_attn_forward_bf16: .*BAD_DIMS"):
        call(13, 13, 96, 1, 13)                      # w w > 144
    with pytest.raises(RuntimeError, match="msda_swin_attn_forward_bf16: .*BAD_DIMS"):
        call(15, 14, 96, 1, 7)                       # map not a multiple of the window
    with pytest.raises(RuntimeError, match="msda_swin_attn_forward_bf16: .*BAD_DIMS"):
        call(14, 14, 3 * 48, 1, 7)                   # C not a multiple of 32
    with pytest.raises(RuntimeError, match="msda_swin_attn_forward_bf16: .*BAD_DIMS"):
        call(14, 14, 96, 1, 7, s=7)
    with pytest.raises(RuntimeError, match="bfloat16"):
        call(14, 14, 96, 1, 7, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="contiguous"):
        call(14, 14, 96, 1, 7, contiguous=False)
    with pytest.raises(RuntimeError, match="table"):
        swin.window_attention(torch.zeros(1, 14, 14, 96, dtype=BF, device="cuda"), torch.zeros(100, 1, device="cuda"), 1, 7, 0)
