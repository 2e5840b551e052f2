"""GPU (-m gpu): the grouped re-pack (csrc/msda_repack.h, richsem_amd/repack.py) writes, in one launch, exactly the bits the existing
builders write from the same masters -- int16 / int32 views compared with ``torch.equal`` (a NaN must stay a NaN; its payload is not
compared) -- and a recorded plan keeps every bound form on the current masters through optimizer steps, eager and captured."""
import copy

import numpy as np
import pytest
import torch

import layer_params as LP
from richsem_amd import _lib, conv, param_cache, repack
from richsem_amd.capture import capture, capture_stream, pin_grad_accumulators
from richsem_amd.functions.ffn import pack_ffn, pack_w2_bf16
from richsem_amd.functions.linear import lin256_pack, lin256_pack_transposed, pack_linear256, pack_linear256_padded
from richsem_amd.param_cache import VersionCache, cast_bf16
from richsem_amd.repack import RepackPlan

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
# +-0, the smallest and the largest denormal, a mid denormal, +-Inf, exact bf16 ties that round down / up to even (both signs), the
# largest finite fp32 (rounds to Inf), one ulp either side of a tie, a quiet and a signalling NaN
SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F800000, 0xFF800000, 0x3F808000, 0x3F818000, 0xBF808000,
                0xBF818000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F807FFF, 0x3F808001, 0x7FC00000, 0x7F800001]


def _rand(*shape, seed=0, scale=0.1):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).mul_(scale).to(DEV)


def _plant(t, seed=0):
    """the special values at scattered places of the fp32 tensor ``t`` (in place; as many as fit)"""
    flat = t.detach().view(-1).view(torch.int32)
    n = min(len(SPECIAL_BITS), flat.numel())
    pos = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(100 + seed))[:n].to(t.device)
    flat[pos] = torch.tensor(np.array(SPECIAL_BITS[:n], dtype=np.uint32).view(np.int32), device=t.device)


def _new_masters(params, seed):
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(_rand(*p.shape, seed=seed + i))
            _plant(p, seed + i)


def _same_bits(got, want):
    """bit equality of two tensors of one dtype and size; where ``want`` is a NaN, ``got`` must be one (payload not compared)"""
    if got.dtype != want.dtype or got.numel() != want.numel():
        return False
    g, w = got.reshape(-1), want.reshape(-1)
    fl = {torch.int16: BF, torch.bfloat16: BF, torch.float32: torch.float32}[w.dtype]
    gi, wi = (g.view(torch.int16), w.view(torch.int16)) if fl == BF else (g.view(torch.int32), w.view(torch.int32))
    gn, wn = torch.isnan(g.view(fl)), torch.isnan(w.view(fl))
    return bool(torch.equal(gn, wn)) and bool(torch.equal(gi[~wn], wi[~wn]))


def _leaves(v):
    return repack._leaves(v, [])


def _follows(params, build, seed):
    """record ``build`` (the existing builders on ``params``) in a cache of its own, give the masters new values with the special ones
    planted, and compare what ONE refresh wrote with the builders run fresh"""
    cache, plan = VersionCache(), RepackPlan()
    with plan.record():
        val = cache.get(params, build)
    assert cache._binding is not None, plan.unbound
    _new_masters(params, seed)
    got = cache.get(params, build)
    assert got is val and plan.launches == 1
    with torch.no_grad():
        want = build()
    gl, wl = _leaves(got), _leaves(want)
    assert len(gl) == len(wl) and len(gl) > 0
    for i, (a, b) in enumerate(zip(gl, wl)):
        assert a.data_ptr() != b.data_ptr() or a.dtype == torch.float32      # (an fp32 bias is the master itself)
        assert _same_bits(a, b), (i, a.dtype, tuple(a.shape))
    torch.cuda.synchronize()
    return plan


# ---- lin256 forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(64,), (128, 64), (256, 128), (64, 64, 64), (256,)], ids=lambda r: "+".join(map(str, r)))
def test_lin256_forms_of_stacked_layers(rows):
    """w16, packed, packed_t (a 256-row stack) and b32 of pack_linear256: one block, two and three segments, the MSDeformAttn query
    stack, and the 256 x 256 layer with its transposed form"""
    ws = [torch.nn.Parameter(_rand(r, 256, seed=i)) for i, r in enumerate(rows)]
    bs = [torch.nn.Parameter(_rand(r, seed=10 + i)) for i, r in enumerate(rows)]
    plan = _follows(ws + bs, lambda: pack_linear256(ws, bs), seed=20)
    kinds = sorted(j.kind for j in plan.jobs())
    assert kinds == sorted(["cast", "lin256"] + (["lin256_t"] if sum(rows) == 256 else []) + (["copy"] if len(rows) > 1 else []))


def test_lin256_forms_of_a_row_slice():
    """the decoder layer's value projection: rows 512.. of a (768, 256) in_proj_weight"""
    w, b = torch.nn.Parameter(_rand(768, 256, seed=1)), torch.nn.Parameter(_rand(768, seed=2))
    plan = _follows([w, b], lambda: {"qk": pack_linear256([w[:512]], [b[:512]]), "v": pack_linear256([w[512:]], [b[512:]])}, seed=30)
    assert any(j.segments[0].data_ptr() == w.data_ptr() + 512 * 256 * 4 for j in plan.jobs())


def test_lin256_forms_padded_from_four_rows():
    """the box heads' 256 -> 4: zero rows up to 64, a zero tail of the bias"""
    w, b = torch.nn.Parameter(_rand(4, 256, seed=3)), torch.nn.Parameter(_rand(4, seed=4))
    cache, plan = VersionCache(), RepackPlan()
    build = lambda: pack_linear256_padded(w, b)
    with plan.record():
        pk = cache.get([w, b], build)
    assert cache._binding is not None
    for t in (pk["w16"], pk["packed"], pk["b32"]):
        t.fill_(1.0)                                   # (the padding must be WRITTEN as zeros, not left over)
    _new_masters([w, b], 40)
    got = cache.get([w, b], build)
    want = build()
    for k in ("w16", "packed", "b32"):
        assert _same_bits(got[k], want[k]), k
    assert float(got["b32"][4:].abs().max()) == 0.0 and float(got["w16"][4:].float().abs().max()) == 0.0


def test_transposed_lin256_form_of_linear2():
    """lin256_pack of the transpose of a (256, d_ffn) linear2.weight, beside its bf16 cast (the decoder layer's forms)"""
    w2 = torch.nn.Parameter(_rand(256, 192, seed=5))
    _follows([w2], lambda: {"w2_16": cast_bf16(w2), "w2t": lin256_pack_transposed(w2)}, seed=50)


# ---- the feed-forward block ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d_ffn", [64, 192])
def test_ffn_forms(d_ffn):
    """pack_ffn at the smallest d_ffn its lin256 forms take and at a larger multiple that is no power of two"""
    w1, b1 = torch.nn.Parameter(_rand(d_ffn, 256, seed=6)), torch.nn.Parameter(_rand(d_ffn, seed=7))
    w2 = torch.nn.Parameter(_rand(256, d_ffn, seed=8))
    plan = _follows([w1, b1, w2], lambda: pack_ffn(w1, b1, w2), seed=60)
    assert sorted(j.kind for j in plan.jobs()) == ["cast", "ffn_w2", "lin256", "lin256_t"]


@pytest.mark.parametrize("d_ffn", [32, 96])
def test_ffn_w2_order_at_the_smallest_width(d_ffn):
    """the W2 order alone at the smallest d_ffn msda_ffn_forward_train_bf16 accepts (32: below lin256's 64 rows) and at 96"""
    w2 = torch.nn.Parameter(_rand(256, d_ffn, seed=9))

    def build():
        out = pack_w2_bf16(w2.detach().to(BF).contiguous())
        param_cache.note("ffn_w2", out, [w2])
        return out
    _follows([w2], build, seed=70)


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(16, 3, 7, 7), (32, 32, 3, 3), (64, 64, 1, 1), (48, 64, 3, 3), (128, 256, 1, 1)]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_packs(shape):
    """the forward pack (few-channel path with K = 147 padded to 160, groups of 2 / 4 / 1 row tiles, with and without k-step pairs) and,
    where the input gradient exists (Cout % 32 == 0, Cin % 16 == 0), its flipped / transposed pack with a non-trivial scale folded in"""
    Cout, Cin = shape[:2]
    w = torch.nn.Parameter(_rand(*shape, seed=11))
    scale = (torch.rand(Cout, generator=torch.Generator().manual_seed(12)) + 0.5).to(DEV)
    slots = [False] + ([True] if Cout % 32 == 0 and Cin % 16 == 0 else [])
    cache, plan = conv.PackCache(), RepackPlan()
    with plan.record():
        vals = {t: cache.get(w, scale, t) for t in slots}
    assert sorted(cache._bound) == slots and not plan.unbound
    _new_masters([w], 80)
    for t in slots:
        got = cache.get(w, scale, t)
        assert got is vals[t]
        assert _same_bits(got, conv._pack_form(w, scale, t)), (shape, t)
    assert plan.launches == 1


# ---- flat casts and copies ---------------------------------------------------------------------------------------------------------------
def test_flat_casts_and_copies():
    """1-D biases, a shape whose element count is no multiple of 8, the bf16 cast of two stacked tensors"""
    a, b, c = (torch.nn.Parameter(_rand(*s, seed=13 + i)) for i, s in enumerate([(300,), (7, 13), (5,)]))
    u, v = torch.nn.Parameter(_rand(128, 32, seed=16)), torch.nn.Parameter(_rand(64, 32, seed=17))

    def build():
        b32 = torch.cat([a.detach(), c.detach()]).float().contiguous()
        param_cache.note("copy", b32, [a, c])
        return {"a": cast_bf16(a), "b": cast_bf16(b), "c": cast_bf16(c), "uv": cast_bf16(u, v), "ac": cast_bf16(a, c), "b32": b32}
    _follows([a, b, c, u, v], build, seed=90)


# ---- one table, every kind, guard words ------------------------------------------------------------------------------------------------
def _guarded(n, dtype):
    item = torch.empty((), dtype=dtype).element_size()
    buf = torch.full((16 + n * item + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[16:16 + n * item].view(dtype)


def test_one_launch_writes_every_kind_and_nothing_else():
    """jobs of all seven kinds in one table; the first is no multiple of the chunk (nor of a 16-byte unit) and is followed by others; each
    destination sits between guard bytes that the launch must leave alone"""
    C = repack.CHUNK
    src = {k: _rand(*s, seed=30 + i) for i, (k, s) in enumerate({
        "cast_a": (C + 9,), "cast_b": (4,), "copy": (1001,), "l0": (20, 256), "l1": (40, 256), "lt": (256, 64), "w2": (256, 32),
        "cv": (16, 3, 7, 7), "ct": (32, 32, 3, 3)}.items())}
    for i, t in enumerate(src.values()):
        _plant(t, i)
    scale = (torch.rand(32, generator=torch.Generator().manual_seed(3)) + 0.5).to(DEV)
    wl = torch.zeros(64, 256, device=DEV)
    wl[:20], wl[20:60] = src["l0"], src["l1"]
    cast_want = torch.zeros(C + 13, dtype=BF, device=DEV)
    cast_want[:C + 9], cast_want[C + 9:] = src["cast_a"].to(BF), src["cast_b"].to(BF)
    copy_want = torch.zeros(1003, device=DEV)
    copy_want[:1001] = src["copy"]
    specs = [      # (kind, destination dtype, destination shape, segments, scale, what the existing builders give)
        ("cast", BF, (C + 13,), [src["cast_a"], src["cast_b"]], None, cast_want),
        ("copy", torch.float32, (1003,), [src["copy"]], None, copy_want),
        ("lin256", BF, (64, 256), [src["l0"], src["l1"]], None, lin256_pack(wl)),
        ("lin256_t", BF, (64, 256), [src["lt"]], None, lin256_pack(src["lt"].to(BF).t().contiguous())),
        ("ffn_w2", BF, (256, 32), [src["w2"]], None, pack_w2_bf16(src["w2"].to(BF).contiguous())),
        ("conv", torch.int16, (16 * 160,), [src["cv"]], None, conv._pack_form(src["cv"], None, False)),
        ("conv_t", torch.int16, (32 * 288,), [src["ct"]], scale, conv._pack_form(src["ct"], scale, True)),
    ]
    rows = np.zeros(len(specs), dtype=repack.JOB_DT)
    held = []
    for i, (kind, dt, shape, segs, sc, _) in enumerate(specs):
        buf, dst = _guarded(int(np.prod(shape)), dt)
        dst = dst.view(shape)
        held.append((buf, dst))
        rows[i] = repack.job_row(kind, dst, segs, sc)
    chunks = repack.plan_chunks(rows)
    assert [int(c["count"]) for c in chunks[:3]] == [C, 13, 1003] and int(chunks[2]["job"]) == 1
    table = torch.from_numpy(np.concatenate([rows.view(np.uint8), chunks.view(np.uint8)])).to(DEV)
    torch.cuda.synchronize()
    _lib.check(_lib.load().msda_repack(table.data_ptr(), table.data_ptr() + rows.nbytes, len(chunks), _lib.raw_stream(table.device)))
    torch.cuda.synchronize()
    for (kind, _, _, _, _, want), (buf, dst) in zip(specs, held):
        assert _same_bits(dst, want), kind
        assert bool((buf[:16] == 0xA5).all()) and bool((buf[-16:] == 0xA5).all()), kind


# ---- follows training ------------------------------------------------------------------------------------------------------------------
class _Small(torch.nn.Module):
    """a decoder MLP 256 -> 256 -> 4, an MSDeformAttn at d_model 256 and a ConvBNAct 64 -> 64 3 x 3"""

    def __init__(self):
        super().__init__()
        from richsem_amd.conv import ConvBNAct
        from richsem_amd.modules import MLP, MSDeformAttn
        self.mlp = LP.fill(MLP(256, 256, 4, 2), 300)
        self.attn = LP.fill(MSDeformAttn(256, 4, 8, 4), 500)
        self.conv = ConvBNAct(64, 64, 3, 1, 1)
        with torch.no_grad():
            self.conv.bn_weight.copy_(torch.rand(64, generator=torch.Generator().manual_seed(1)) + 0.5)


def _small_inputs():
    from richsem_amd import workload as W
    call = W.shrunk(W.call_Dd(2), 4)
    shapes, lsi = W.level_tensors(call, torch.device(DEV))
    g = torch.Generator().manual_seed(17)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return dict(xm=rnd(96, 256).to(BF), q=rnd(call.N, 50, 256).to(BF), rp=(torch.rand(call.N, 50, 4, 4, generator=g) * 0.4 + 0.2).to(DEV),
                xv=rnd(call.N, call.S, 256).to(BF), shapes=shapes, lsi=lsi, xc=rnd(2, 13, 17, 64).to(BF).requires_grad_(True))


def _loss(m, i):
    return (m.mlp(i["xm"]).float().sum() + m.attn(i["q"], i["rp"], i["xv"], i["shapes"], i["lsi"], None).float().pow(2).mean()
            + m.conv(i["xc"]).float().pow(2).mean())


def _work(m, i, opt):
    for p in m.parameters():
        p.grad = None
    i["xc"].grad = None
    _loss(m, i).backward()
    opt.step()


def _fresh_form(j):
    """the form of job ``j`` from the existing builders on the CURRENT masters"""
    segs = [s.detach() for s in j.segments]
    if j.kind in ("cast", "copy"):
        flat = torch.cat([s.reshape(-1) for s in segs])
        out = torch.zeros(j.dst.numel(), dtype=j.dst.dtype, device=flat.device)
        out[:flat.numel()] = flat.to(j.dst.dtype).contiguous()
        return out
    if j.kind == "lin256":
        w = torch.zeros(j.dst.shape[0], 256, device=segs[0].device)
        cat = torch.cat(segs, 0)
        w[:cat.shape[0]] = cat
        return lin256_pack(w)
    if j.kind == "lin256_t":
        return lin256_pack(torch.cat(segs, 0).to(BF).t().contiguous())
    if j.kind == "ffn_w2":
        return pack_w2_bf16(segs[0].to(BF).contiguous())
    return conv._pack_form(segs[0], j.scale, j.kind == "conv_t")


def _all_fresh(plan):
    torch.cuda.synchronize()
    jobs = plan.jobs()
    assert jobs
    return all(_same_bits(j.dst, _fresh_form(j)) for j in jobs)


def _recorded_small():
    torch.manual_seed(0)
    m = _Small().to(DEV)
    i = _small_inputs()
    plan = RepackPlan()
    return m, i, plan


def _check_bound(m, plan):
    assert m.mlp._packs._binding is not None and m.attn._packs._binding is not None and sorted(m.conv._pack_cache._bound) == [False, True]
    assert [u["cache"] for u in plan.unbound] == [m.conv._folded]      # the frozen affine's fold: no trained master, no job
    assert plan.n_jobs == 17 and plan.n_chunks >= plan.n_jobs
    kinds = {j.kind for j in plan.jobs()}
    assert kinds == {"cast", "copy", "lin256", "lin256_t", "conv", "conv_t"}


@pytest.mark.parametrize("optimizer", ["clip_adamw_attached", "torch_adamw_then_refresh"])
def test_bound_forms_follow_three_eager_steps(optimizer):
    from richsem_amd.optim import ClipAdamW
    m, i, plan = _recorded_small()
    with plan.record():
        _loss(m, i).backward()
    _check_bound(m, plan)
    assert _all_fresh(plan)
    params = list(m.parameters())
    if optimizer == "clip_adamw_attached":
        opt = ClipAdamW(params, lr=2e-2, max_norm=0.0)
        opt.attach_repack(plan)
    else:
        opt = torch.optim.AdamW(params, lr=2e-2, fused=True)
    for step in range(3):
        before = [j.dst.clone() for j in plan.jobs()]
        _work(m, i, opt)
        if optimizer != "clip_adamw_attached":
            plan.refresh()
        assert plan.launches == step + 1                       # the step's forward and backward found every form fresh
        assert _all_fresh(plan), (optimizer, step)
        moved = sum(not torch.equal(a, j.dst) for a, j in zip(before, plan.jobs()))
        assert moved == plan.n_jobs, (step, moved)             # (the control: every form did change with the step)
    with torch.no_grad():
        _loss(m, i)
    assert plan.launches == 3


def test_bound_forms_follow_three_replays_of_a_captured_step():
    """forward + backward + ClipAdamW.step() with the plan attached in ONE graph: the forms are compared, not the losses (the atomics of a
    backward cannot decide the test)"""
    from richsem_amd.optim import ClipAdamW
    m, i, plan = _recorded_small()
    params = list(m.parameters())
    opt = ClipAdamW(params, lr=2e-2, max_norm=0.0)
    with capture_stream() as side:
        pinned = pin_grad_accumulators(params + [i["xc"]])      # noqa: F841
        with plan.record():
            _loss(m, i).backward()
        _check_bound(m, plan)
        for p in params:
            p.grad = None
        i["xc"].grad = None
        opt.attach_repack(plan)
        opt.init_state()
        opt.sync()
        torch.cuda.synchronize()
        launches = plan.launches
        graph, _ = capture(lambda: _work(m, i, opt), side)
        assert plan.launches == launches + 1                   # the capture recorded ONE refresh and no other pack launch
        for step in range(3):
            before = [j.dst.clone() for j in plan.jobs()]
            graph.replay()
            assert _all_fresh(plan), step
            assert sum(not torch.equal(a, j.dst) for a, j in zip(before, plan.jobs())) == plan.n_jobs
        del graph


def test_load_state_dict_and_copy_make_the_next_get_refresh():
    m, i, plan = _recorded_small()
    with plan.record():
        _loss(m, i).backward()
    other = _Small().to(DEV)
    with torch.no_grad():
        for p in other.parameters():
            p.mul_(1.5)
    m.load_state_dict(other.state_dict())
    with torch.no_grad():
        m.mlp(i["xm"])
    assert plan.launches == 1 and _all_fresh(plan)
    with torch.no_grad():
        m.conv.weight.copy_(_rand(64, 64, 3, 3, seed=5))
        m.conv(i["xc"])
    assert plan.launches == 2 and _all_fresh(plan)
    with torch.no_grad():
        _loss(m, i)
    assert plan.launches == 2


def test_release_restores_rebuilding_and_a_deep_copy_is_unbound():
    m, i, plan = _recorded_small()
    with plan.record():
        _loss(m, i).backward()
    twin = copy.deepcopy(m)
    assert twin.mlp._packs._binding is None and twin.attn._packs._binding is None and not twin.conv._pack_cache._bound
    with torch.no_grad():
        for p in twin.parameters():
            p.mul_(0.5)
        _loss(twin, i)                                          # builds its own forms from its own parameters
    tw = twin.mlp._packs._val[0][1]
    assert _same_bits(tw["packed"], lin256_pack(twin.mlp.layers[0].weight)) and tw["packed"].data_ptr() != m.mlp._packs._binding.val[0][1]["packed"].data_ptr()
    assert plan.launches == 0 and _all_fresh(plan)
    plan.release()
    assert m.mlp._packs._binding is None and not m.conv._pack_cache._bound
    opt = torch.optim.AdamW(list(m.parameters()), lr=2e-2, fused=True)
    _work(m, i, opt)
    with torch.no_grad():
        _loss(m, i)
    assert plan.launches == 0
    assert _same_bits(m.mlp._packs._val[0][1]["packed"], lin256_pack(m.mlp.layers[0].weight))
    assert _same_bits(m.conv._pack_cache._slots[False][1], conv._pack_form(m.conv.weight, None, False))


def test_a_cache_with_an_unnoted_tensor_is_listed_and_follows_the_optimizer_the_old_way():
    w = torch.nn.Parameter(_rand(64, 256, seed=1))
    cache, plan = VersionCache(), RepackPlan()
    build = lambda: {"w16": cast_bf16(w), "wt": w.detach().t().contiguous()}
    with plan.record():
        cache.get([w], build)
    assert cache._binding is None and [u["cache"] for u in plan.unbound] == [cache] and plan.n_jobs == 0
    w.grad = _rand(64, 256, seed=2)
    torch.optim.AdamW([w], lr=2e-2, fused=True).step()
    got = cache.get([w], build)
    assert torch.equal(got["wt"], w.detach().t()) and torch.equal(got["w16"], w.detach().to(BF)) and plan.launches == 0
