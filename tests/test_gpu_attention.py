"""GPU (-m gpu): the attention kernels (csrc/attn_mfma.hip) through the C ABI, EVERY element of out / lse / dq / dk / dv against the
float64 reference and the element-wise rounding bounds of tests/attention_ref.py (|err| / bound <= 1), at the shapes where the four
waves, the 32-key blocks and the 16-query workgroups change what the kernel does; exact probes of the mask bits; leading dimensions,
workspace size and untouched memory; bit-equal repeats.  RICHSEM_REPORT=1 prints the worst ratio of every case next to the
emulation's on the same data (profiles/r10_attention_bounds.md)."""
import os

import pytest
import torch

import attention_ref as R
from richsem_amd import _lib

pytestmark = pytest.mark.gpu

SENT16 = 0x7B5A          # the sentinels: a bf16 bit pattern, a float and a byte no kernel here writes
SENTF = -1234.5
SENT8 = 0xA5
GUARD_ROWS = 3


def _ceil32(n):
    return (n + 31) // 32 * 32


def _tokens(x, batch_first):
    """(B, H, nq, 32) -> the ABI's (rows, H * 32): token (i, b) at row i * bs + b, or b * nq + i with batch_first"""
    B, H, nq, _ = x.shape
    t = x.permute(0, 2, 1, 3) if batch_first else x.permute(2, 0, 1, 3)
    return t.reshape(B * nq, H * 32)


def _heads(rows, B, H, nq, batch_first):
    t = rows.reshape(B, nq, H, 32) if batch_first else rows.reshape(nq, B, H, 32)
    return t.permute(0, 2, 1, 3) if batch_first else t.permute(1, 2, 0, 3)


class _Buf:
    """a (rows + GUARD_ROWS, ld) bf16 buffer full of the sentinel; the tensor lives in columns [col, col + width) of the first rows"""

    def __init__(self, rows, ld, width, col=0, base=None):
        self.rows, self.ld, self.width, self.col = rows, ld, width, col
        self.raw = base if base is not None else torch.full((rows + GUARD_ROWS, ld), SENT16, dtype=torch.int16, device="cuda")

    def put(self, x):
        self.raw[: self.rows, self.col: self.col + self.width] = x.contiguous().view(torch.int16)
        return self

    def ptr(self):
        return self.raw.data_ptr() + 2 * self.col

    def get(self):
        return self.raw[: self.rows, self.col: self.col + self.width].contiguous().view(torch.bfloat16)


def _untouched(bufs):
    """every element of the raw buffers outside the tensors' columns, and every guard row, still holds the sentinel"""
    seen = {}
    for b in bufs:
        keep = seen.setdefault(id(b.raw), (b.raw, torch.ones_like(b.raw, dtype=torch.bool)))[1]
        keep[: b.rows, b.col: b.col + b.width] = False
    return all(bool((raw[keep] == SENT16).all()) for raw, keep in seen.values())


def run_abi(q, k, v, do, mask, batch_first=False, layout="stacked", check_memory=False):
    """q, k, v, do (B, H, nq, 32) bf16 on the GPU, mask (nq, nq) bool or None -> dict out / lse2 / dq / dk / dv per (image, head),
    plus `lse_pad` (B * H, ceil32(nq) - nq).  Layouts: "stacked" -- q and k interleaved in one (rows, 2 C) buffer as the stacked
    projection leaves them, dq / dk the same, v and dv (rows, C); "wide" -- q, k, v each in a wider buffer of its own; "wide_stacked"
    -- q and k interleaved in a wider buffer, v wider; both wide layouts with three different, wider lddq / lddk / lddv."""
    from richsem_amd.functions.attention import _MASK_CACHE, mask_bits
    lib = _lib.load()
    B, H, nq, _ = q.shape
    C, rows, nqp = H * 32, B * nq, _ceil32(nq)
    tq, tk, tv, tdo = (_tokens(x, batch_first) for x in (q, k, v, do))
    if layout == "stacked":
        qk = torch.full((rows + GUARD_ROWS, 2 * C), SENT16, dtype=torch.int16, device="cuda")
        bq, bk, bv = _Buf(rows, 2 * C, C, 0, qk).put(tq), _Buf(rows, 2 * C, C, C, qk).put(tk), _Buf(rows, C, C).put(tv)
        dqk = torch.full_like(qk, SENT16)
        bdq, bdk, bdv = _Buf(rows, 2 * C, C, 0, dqk), _Buf(rows, 2 * C, C, C, dqk), _Buf(rows, C, C)
    else:
        if layout == "wide":
            bq, bk = _Buf(rows, C + 8, C).put(tq), _Buf(rows, C + 16, C, 8).put(tk)
        else:
            qk = torch.full((rows + GUARD_ROWS, 2 * C + 8), SENT16, dtype=torch.int16, device="cuda")
            bq, bk = _Buf(rows, 2 * C + 8, C, 0, qk).put(tq), _Buf(rows, 2 * C + 8, C, C, qk).put(tk)
        bv = _Buf(rows, C + 8, C).put(tv)
        bdq, bdk, bdv = _Buf(rows, C + 8, C), _Buf(rows, C + 24, C, 8), _Buf(rows, C + 16, C)
    bout, bdo = _Buf(rows, C, C), _Buf(rows, C, C).put(tdo)
    lse = torch.full((B * H * nqp + 64,), SENTF, dtype=torch.float32, device="cuda")
    nws = lib.msda_attn_workspace_bytes(nq, B, H)
    ws_f, ws_b = (torch.full((nws + 256,), SENT8, dtype=torch.uint8, device="cuda") for _ in range(2))
    bits = (None, None)
    if mask is not None:
        _MASK_CACHE.clear()
        bits = mask_bits(mask.cuda())
        _MASK_CACHE.clear()
    mp = [b.data_ptr() if b is not None else None for b in bits]
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.msda_attn_forward_bf16(bq.ptr(), bq.ld, bk.ptr(), bk.ld, bv.ptr(), bv.ld, mp[0], nq, B, int(batch_first), H,
                                          bout.ptr(), lse.data_ptr(), ws_f.data_ptr(), st))
    _lib.check(lib.msda_attn_backward_bf16(bq.ptr(), bq.ld, bk.ptr(), bk.ld, bv.ptr(), bv.ld, bout.ptr(), bdo.ptr(), lse.data_ptr(),
                                           mp[0], mp[1], nq, B, int(batch_first), H, bdq.ptr(), bdq.ld, bdk.ptr(), bdk.ld,
                                           bdv.ptr(), bdv.ld, ws_b.data_ptr(), st))
    torch.cuda.synchronize()
    if check_memory:
        assert _untouched([bq, bk, bv, bdo]), "an input buffer was written"
        assert _untouched([bout, bdq, bdk, bdv]), "columns outside the heads or guard rows of an output were written"
        assert bool((lse[B * H * nqp:] == SENTF).all()), "floats past lse were written"
        for ws in (ws_f, ws_b):
            assert bool((ws[nws:] == SENT8).all()), "bytes past msda_attn_workspace_bytes were written"
    lse = lse[: B * H * nqp].view(B, H, nqp)
    res = {n: _heads(b.get(), B, H, nq, batch_first) for n, b in (("out", bout), ("dq", bdq), ("dk", bdk), ("dv", bdv))}
    res["lse2"], res["lse_pad"] = lse[:, :, :nq], lse[:, :, nq:]
    return res


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(bs, heads, nq, gen, scale=1.5):
    return tuple(t.cuda() for t in R.random_inputs(bs, heads, nq, gen, scale))


def _check(tag, got, q, k, v, do, mask):
    """every element of the five tensors inside its bound, the lse padding +inf, nothing else non-finite -> the ratios"""
    mask = None if mask is None else mask.cuda()
    val, bound = R.reference(q, k, v, do, mask)
    r = R.ratios(got, val, bound)
    if os.environ.get("RICHSEM_REPORT"):
        e = R.ratios(R.emulate(q, k, v, do, mask), val, bound)
        print(f"[measured] {tag} " + " ".join(f"{n}={r[n]:.3f}/{e[n]:.3f}" for n in R.TENSORS), flush=True)
    for n in R.TENSORS:
        assert r[n] <= 1.0, (tag, n, r[n])
    for n in ("out", "dq", "dk", "dv"):
        assert got[n].dtype == torch.bfloat16 and bool(torch.isfinite(got[n].float()).all()), (tag, n)
    assert bool((got["lse_pad"] == float("inf")).all()), (tag, "lse padding")
    assert bool((torch.isinf(got["lse2"]) == torch.isinf(val["lse2"])).all()), (tag, "lse")
    return r


# ---- element-wise parity at the edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160])
def test_every_element_is_inside_its_bound_across_the_block_boundaries(nq, masked):
    """nq around 16 (workgroup), 32 (key block), 128 (four waves x 32): 1-3 waves without any key block, one block per wave, a wave
    with two, workgroups wholly in the padding; every (image, head) has data of its own"""
    gen = _gen(1000 + 2 * nq + masked)
    mask = R.existing_test_mask(nq, gen) if masked else None
    for bs in (1, 2):
        for heads in (1, 3):
            for batch_first in (False, True):
                q, k, v, do = _inputs(bs, heads, nq, gen)
                got = run_abi(q, k, v, do, mask, batch_first)
                _check(f"sweep nq={nq} masked={int(masked)} bs={bs} heads={heads} bf={int(batch_first)}", got, q, k, v, do, mask)


@pytest.mark.parametrize("kind,nq", [("causal", 129), ("own_block", 129), ("wave0", 129), ("wave1", 129), ("wave2", 129), ("wave3", 129),
                                     ("last_key", 129), ("first_block_masked", 129), ("first_block_masked", 257)])
def test_structured_masks(kind, nq):
    """masks that leave whole waves without a key (the merge must ignore their m = -inf), a wave's first block dead and a later one
    alive (the running maximum starts at -inf; at nq = 257 that is every wave), only the lone key of the last partial block"""
    gen = _gen(len(kind) * 31 + nq)
    mask = R.structured_mask(kind, nq)
    q, k, v, do = _inputs(2, 3, nq, gen)
    _check(f"{kind} nq={nq}", run_abi(q, k, v, do, mask), q, k, v, do, mask)


def test_denoising_mask():
    from richsem_amd import dn
    mask = dn.prepare_dn_layout([3], dn_number=10, num_queries=20)["attn_mask"].clone()
    nq = mask.shape[0]
    assert bool(mask.any()) and not bool(mask.all(1).any())
    q, k, v, do = _inputs(2, 3, nq, _gen(7))
    _check(f"denoising nq={nq}", run_abi(q, k, v, do, mask, batch_first=True), q, k, v, do, mask)


def test_rows_without_an_allowed_key():
    """out = 0, lse = +inf and dq = 0 exactly on those rows, nothing from them in dk / dv, everything else inside its bound"""
    nq, gen = 129, _gen(21)
    mask = R.existing_test_mask(nq, gen)
    rows = [0, 5, 77, 128] + list(range(48, 64))          # the first and the last row, and all 16 rows of one workgroup
    mask[rows] = True
    for batch_first in (False, True):
        q, k, v, do = _inputs(2, 3, nq, gen)
        got = run_abi(q, k, v, do, mask, batch_first)
        _check(f"empty rows bf={int(batch_first)}", got, q, k, v, do, mask)      # (dk / dv: the reference leaves those rows out)
        assert bool((got["out"][:, :, rows].float() == 0).all()) and bool((got["dq"][:, :, rows].float() == 0).all())
        assert bool((got["lse2"][:, :, rows] == float("inf")).all())
        keep = [i for i in range(nq) if i not in rows]
        assert bool(torch.isfinite(got["lse2"][:, :, keep]).all())
    # all rows empty: every output is zero
    q, k, v, do = _inputs(1, 2, 33, gen)
    got = run_abi(q, k, v, do, torch.ones(33, 33, dtype=torch.bool))
    assert all(bool((got[n].float() == 0).all()) for n in ("out", "dq", "dk", "dv")) and bool((got["lse2"] == float("inf")).all())


@pytest.mark.parametrize("masked", [0, 1, 2])
def test_large_logits(masked):
    """scores beyond +-150 in log2 units: an exp2f that is not taken relative to the maximum overflows or flushes to zero.
    masked = 2: the last key -- the one the 31 padded keys of the last block are loaded from -- is masked for every other query and
    scores far above each row's allowed maximum: a dead key whose exp2f overflows must still contribute exactly nothing"""
    nq, gen = 129, _gen(31 + masked)
    mask = R.existing_test_mask(nq, gen) if masked else None
    q, k, v, do = _inputs(2, 3, nq, gen, scale=8.0)
    if masked == 2:
        R.mask_outlier_last_key(q, k, mask)
    s2 = (q.double() @ k.double().transpose(-1, -2)) * R.C * R.LOG2E
    assert float(s2.max()) > 150 and float(s2.min()) < -150
    if masked == 2:
        allowed_max = s2.masked_fill(mask.cuda(), float("-inf")).amax(-1)
        assert float((s2[:, :, 0, nq - 1] - allowed_max[:, :, 0]).min()) > 200
    _check(f"large logits masked={masked}", run_abi(q, k, v, do, mask), q, k, v, do, mask)


@pytest.mark.parametrize("layout", ["wide", "wide_stacked"])
@pytest.mark.parametrize("nq", [33, 64])
def test_leading_dimensions_and_untouched_memory(nq, layout):
    """inputs and gradients in wider buffers with different leading dimensions; columns outside the heads, guard rows after every
    output, guard floats after lse and 256 guard bytes after a workspace of exactly msda_attn_workspace_bytes keep their sentinel"""
    gen = _gen(nq + len(layout))
    mask = R.existing_test_mask(nq, gen)
    for bs, heads, batch_first in ((2, 3, False), (1, 1, True), (2, 1, True)):
        q, k, v, do = _inputs(bs, heads, nq, gen)
        got = run_abi(q, k, v, do, mask, batch_first, layout=layout, check_memory=True)
        _check(f"{layout} nq={nq} bs={bs} heads={heads} bf={int(batch_first)}", got, q, k, v, do, mask)
        same = run_abi(q, k, v, do, mask, batch_first, check_memory=True)          # the layout changes no bit of the result
        assert all(torch.equal(got[n], same[n]) for n in R.TENSORS)


def test_repeats_are_bit_equal():
    nq, gen = 129, _gen(41)
    mask = R.existing_test_mask(nq, gen)
    q, k, v, do = _inputs(2, 3, nq, gen)
    a, b = run_abi(q, k, v, do, mask), run_abi(q, k, v, do, mask)
    for n in R.TENSORS:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("batch_first", [False, True])
def test_autograd_wrapper_meets_the_same_bounds(batch_first):
    """masked_self_attention (stacked q | k projection, torch-allocated outputs) instead of the raw ABI"""
    from richsem_amd.functions.attention import masked_self_attention
    nq, bs, heads, gen = 129, 2, 3, _gen(51)
    mask = R.existing_test_mask(nq, gen).cuda()
    q, k, v, do = _inputs(bs, heads, nq, gen)
    qk = torch.cat([_tokens(q, batch_first), _tokens(k, batch_first)], 1)
    shape = (bs, nq) if batch_first else (nq, bs)
    qk = qk.reshape(*shape, 2 * heads * 32).clone().requires_grad_(True)
    vv = _tokens(v, batch_first).reshape(*shape, heads * 32).clone().requires_grad_(True)
    out = masked_self_attention(qk, vv, mask, heads, batch_first=batch_first)
    out.backward(_tokens(do, batch_first).reshape(*shape, heads * 32))
    C = heads * 32
    un = lambda t: _heads(t.reshape(bs * nq, C), bs, heads, nq, batch_first)
    val, bound = R.reference(q, k, v, do, mask)
    got = {"out": un(out.detach()), "dq": un(qk.grad[..., :C]), "dk": un(qk.grad[..., C:]), "dv": un(vv.grad), "lse2": val["lse2"]}
    r = R.ratios(got, val, bound)
    assert all(r[n] <= 1.0 for n in ("out", "dq", "dk", "dv")), r
    raw = run_abi(q, k, v, do, mask, batch_first)
    assert all(torch.equal(got[n], raw[n]) for n in ("out", "dq", "dk", "dv"))


# ---- exact probes of the mask bits -----------------------------------------------------------------------------------------------------
def _probe(nq, seed):
    gen = _gen(seed)
    mask, counts = R.sparse_mask(nq, gen)
    v = torch.randint(-8, 9, (2, 2, nq, 32), generator=gen).to(torch.bfloat16).cuda()
    do = torch.randint(-2, 3, (2, 2, nq, 32), generator=gen).to(torch.bfloat16).cuda()
    ints = torch.randint(-4, 5, (2, 2, nq, 32), generator=gen).to(torch.bfloat16).cuda()
    return mask, counts, v, do, ints, torch.zeros_like(v)


@pytest.mark.parametrize("nq", [33, 97])
def test_with_equal_scores_out_and_dv_are_exact_functions_of_the_mask(nq):
    """q = k = 0: every allowed key weighs 1 / count with count in {1, 2, 4, 8}, so out and dv are exact in bf16 -- one mask bit read
    wrong (keys 31 and 32 of a word among them) changes an element by a multiple of 1 / 8"""
    mask, counts, v, do, _, z = _probe(nq, 60 + nq)
    assert not bool(mask[3, 31]) and not bool(mask[3, 32])
    val, bound = R.reference(z, z, v, do, mask.cuda())
    for n in ("out", "dv"):          # the reference values are bf16 numbers: exact equality is a fair demand
        assert torch.equal(val[n].to(torch.bfloat16).double(), val[n]), n
    for batch_first in (False, True):
        got = run_abi(z, z, v, do, mask, batch_first)
        assert torch.equal(got["out"].double(), val["out"]) and torch.equal(got["dv"].double(), val["dv"])
        assert bool((got["dq"].float() == 0).all()) and bool((got["dk"].float() == 0).all())
        want_lse = torch.log2(counts.double()).cuda().expand(2, 2, nq)
        assert float((val["lse2"] - want_lse).abs().max()) < 1e-12
        assert bool(((got["lse2"].double() - want_lse).abs() <= bound["lse2"]).all())


@pytest.mark.parametrize("which", ["dq_through_mask_bits", "dk_through_maskt_bits"])
@pytest.mark.parametrize("nq", [33, 97])
def test_sparse_mask_gradients(nq, which):
    """q = 0 with integer k: dq = dS k is a function of mask_bits alone; k = 0 with integer q: dk = dS^T q of maskt_bits alone.  The
    mask is not symmetric, so a kernel that reads the mask where it needs the transpose cannot pass."""
    mask, _, v, do, ints, z = _probe(nq, 80 + nq)
    q, k = (z, ints) if which.startswith("dq") else (ints, z)
    got = run_abi(q, k, v, do, mask)
    r = _check(f"{which} nq={nq}", got, q, k, v, do, mask)
    val, bound = R.reference(q, k, v, do, mask.cuda())
    n = which[:2]
    assert float(val[n].abs().max()) > 0.5
    # the bound separates the mask from its transpose: the reference of the transposed mask is far outside it
    wrong = R.reference(q, k, v, do, mask.t().contiguous().cuda())[0]
    assert float(((wrong[n] - val[n]).abs() / bound[n]).max()) > 10 and r[n] <= 1.0
