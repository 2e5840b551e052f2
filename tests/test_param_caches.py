"""CPU: the invalidation contract of the caches of derived parameter forms (richsem_amd/param_cache.py: VersionCache; conv.PackCache).

After every write to a parameter that the library promises to notice -- a step of any torch.optim optimizer (fused, foreach or for-loop),
``load_state_dict``, ``copy_`` -- the next ``get`` must rebuild, and what it returns must equal a build on the current parameters; a
write through ``.data`` is noticed after ``clear()``.  While a graph is being captured, ``get`` must build on every call and keep nothing.
Fused optimizers do not bump autograd's version counter by themselves: without the library's optimizer step hook every cache here
would keep the step-0 weights for the rest of training."""
import pytest
import torch

from richsem_amd import conv
from richsem_amd.functions.linear import VersionCache

OPTIMIZERS = {
    "sgd_foreach": lambda ps: torch.optim.SGD(ps, lr=0.1, foreach=True),
    "sgd_fused": lambda ps: torch.optim.SGD(ps, lr=0.1, fused=True),
    "adam_fused": lambda ps: torch.optim.Adam(ps, lr=0.1, fused=True),
    "adamw_fused": lambda ps: torch.optim.AdamW(ps, lr=0.1, fused=True),
    "adamw_foreach": lambda ps: torch.optim.AdamW(ps, lr=0.1, foreach=True),
    "adamw_forloop": lambda ps: torch.optim.AdamW(ps, lr=0.1, foreach=False),
}


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(64, 32, generator=g) * 0.5), torch.nn.Parameter(torch.randn(64, generator=g) * 0.5)]


def _grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


def _bf16(params):
    """the derived form under test: the bf16 casts of the parameters, flattened into one vector (what the bf16 layers keep)"""
    return torch.cat([p.detach().reshape(-1) for p in params]).to(torch.bfloat16)


class _Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_version_cache_follows_an_optimizer_step(name):
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _bf16(params))
    v0 = cache.get(params, build)
    assert cache.get(params, build) is v0 and build.calls == 1          # a hit between writes
    opt = OPTIMIZERS[name](params)
    for step in range(2):
        _grads(params, seed=10 + step)
        before = _bf16(params)
        opt.step()
        after = _bf16(params)
        assert float((after != before).float().mean()) > 0.9, name      # the bf16-rounded weights did change
        got = cache.get(params, build)
        assert build.calls == 2 + step, (name, step, build.calls)
        assert torch.equal(got, after), (name, step)
        assert cache.get(params, build) is got and build.calls == 2 + step


@pytest.mark.parametrize("name", sorted(OPTIMIZERS))
def test_pack_cache_follows_an_optimizer_step(name, monkeypatch):
    """both slots of a conv.PackCache (the forward weight; the flipped / transposed / scale-folded weight of the input gradient), with a
    CPU stand-in for the pack kernel"""
    def stand_in(weight, scale, transposed):
        w = weight.detach().float()
        if transposed:
            w = (w * scale.view(-1, 1, 1, 1)).flip(2, 3).permute(1, 0, 2, 3)
        return w.contiguous().to(torch.bfloat16)

    pack = _Counting(stand_in)
    monkeypatch.setattr(conv, "_pack_form", pack)
    g = torch.Generator().manual_seed(1)
    w = torch.nn.Parameter(torch.randn(32, 16, 3, 3, generator=g) * 0.2)
    scale = torch.rand(32, generator=g) + 0.5
    cache = conv.PackCache()
    for t in (False, True):
        cache.get(w, scale, t)
        cache.get(w, scale, t)
    assert pack.calls == 2
    opt = OPTIMIZERS[name]([w])
    for step in range(2):
        _grads([w], seed=20 + step)
        before = w.detach().to(torch.bfloat16)
        opt.step()
        assert float((w.detach().to(torch.bfloat16) != before).float().mean()) > 0.9, name
        for t in (False, True):
            assert torch.equal(cache.get(w, scale, t), stand_in(w, scale, t)), (name, step, t)
        assert pack.calls == 4 + 2 * step, (name, step, pack.calls)
        for t in (False, True):
            cache.get(w, scale, t)
        assert pack.calls == 4 + 2 * step


def test_an_optimizer_step_leaves_parameters_without_a_gradient_cached():
    """the step hook bumps what the step may have written: parameters that had no gradient are not touched, their caches stay valid"""
    params, frozen = _params(0), _params(1)
    cache = VersionCache()
    build = _Counting(lambda: _bf16(frozen))
    cache.get(frozen, build)
    opt = torch.optim.AdamW(params + frozen, lr=0.1, fused=True)
    _grads(params, seed=3)
    opt.step()
    assert cache.get(frozen, build) is not None and build.calls == 1


def test_version_cache_follows_writes_outside_an_optimizer():
    """load_state_dict and copy_ are seen by the version counter; a write through ``.data`` is not, and clear() is the documented remedy"""
    lin = torch.nn.Linear(32, 64)
    params = [lin.weight, lin.bias]
    cache = VersionCache()
    build = _Counting(lambda: _bf16(params))
    cache.get(params, build)
    other = torch.nn.Linear(32, 64)
    lin.load_state_dict(other.state_dict())
    assert torch.equal(cache.get(params, build), _bf16(params)) and build.calls == 2
    with torch.no_grad():
        lin.weight.copy_(torch.randn(64, 32))
    assert torch.equal(cache.get(params, build), _bf16(params)) and build.calls == 3
    lin.weight.data.mul_(0.5)
    cache.clear()
    assert torch.equal(cache.get(params, build), _bf16(params)) and build.calls == 4
    assert cache.get(params, build) is not None and build.calls == 4


def test_pack_cache_follows_load_state_dict_copy_and_clear(monkeypatch):
    pack = _Counting(lambda weight, scale, transposed: weight.detach().to(torch.bfloat16).clone())
    monkeypatch.setattr(conv, "_pack_form", pack)
    m = torch.nn.Conv2d(16, 32, 3, bias=False)
    scale = torch.ones(32)
    cache = conv.PackCache()
    cache.get(m.weight, scale, False)
    m.load_state_dict(torch.nn.Conv2d(16, 32, 3, bias=False).state_dict())
    assert torch.equal(cache.get(m.weight, scale, False), m.weight.detach().to(torch.bfloat16)) and pack.calls == 2
    with torch.no_grad():
        m.weight.copy_(torch.randn_like(m.weight))
    assert torch.equal(cache.get(m.weight, scale, False), m.weight.detach().to(torch.bfloat16)) and pack.calls == 3
    m.weight.data.mul_(0.5)
    cache.clear()
    assert torch.equal(cache.get(m.weight, scale, False), m.weight.detach().to(torch.bfloat16)) and pack.calls == 4


def test_caches_build_and_keep_nothing_while_capturing(monkeypatch):
    """rule 2 of param_cache.py, with the capture state stood in: every get builds (its kernels would be recorded into the graph), and
    nothing built during the capture is handed out afterwards"""
    from richsem_amd import param_cache
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _bf16(params))
    eager = cache.get(params, build)
    pack = _Counting(lambda weight, scale, transposed: weight.detach().to(torch.bfloat16).clone())
    monkeypatch.setattr(conv, "_pack_form", pack)
    w = torch.nn.Parameter(torch.randn(32, 16, 3, 3))
    pcache = conv.PackCache()
    pk = pcache.get(w, torch.ones(32), False)
    for flag in (param_cache, conv):
        monkeypatch.setattr(flag, "capturing", lambda t: True)
    during = [cache.get(params, build) for _ in range(2)]
    pdur = [pcache.get(w, torch.ones(32), False) for _ in range(2)]
    assert build.calls == 3 and pack.calls == 3
    assert all(v is not eager and torch.equal(v, eager) for v in during)
    assert all(v is not pk and torch.equal(v, pk) for v in pdur)
    for flag in (param_cache, conv):
        monkeypatch.setattr(flag, "capturing", lambda t: False)
    assert cache.get(params, build) is eager and pcache.get(w, torch.ones(32), False) is pk
    assert build.calls == 3 and pack.calls == 3


def test_module_caches_follow_a_fused_optimizer_step():
    """the library's own caches that build on the CPU: MSDeformAttn's bf16 casts (widths other than 256), the attention pool's derived
    forms, ConvBNAct's folded affine (buffers: load_state_dict)"""
    from richsem_amd.modules import MSDeformAttn
    from richsem_amd.modules.attnpool import AttentionPool2d
    torch.manual_seed(0)
    m = MSDeformAttn(32, 2, 4, 2)
    ps = list(m.parameters())
    first = m._bf16_params()
    assert m._bf16_params() is first
    opt = torch.optim.AdamW(ps, lr=0.1, fused=True)
    _grads(ps, seed=5)
    opt.step()
    now = m._bf16_params()
    assert torch.equal(now["wq"], torch.cat((m.sampling_offsets.weight, m.attention_weights.weight)).detach().to(torch.bfloat16))
    assert torch.equal(now["wo"], m.output_proj.weight.detach().to(torch.bfloat16))
    assert not torch.equal(now["wo"], first["wo"])

    pool = AttentionPool2d(3, 32, 4, 16)
    d0 = pool._derived(torch.float32)
    assert pool._derived(torch.float32) is d0
    pps = list(pool.parameters())
    opt = torch.optim.Adam(pps, lr=0.1, fused=True)
    _grads(pps, seed=6)
    opt.step()
    d1 = pool._derived(torch.float32)
    assert torch.equal(d1["wc_t"], pool.c_proj.weight.detach().t().contiguous()) and not torch.equal(d1["wc_t"], d0["wc_t"])
    assert torch.equal(d1["pos"], pool.positional_embedding.detach())

    cb = conv.ConvBNAct(16, 32, 3, padding=1)
    s0, _ = cb.scale_shift()
    sd = cb.state_dict()
    sd["running_var"] = torch.full((32,), 4.0)
    cb.load_state_dict(sd)
    s1, b1 = cb.scale_shift()
    want = conv.fold_bn(cb.bn_weight, cb.bn_bias, cb.running_mean, cb.running_var, 1e-5)
    assert torch.equal(s1, want[0]) and torch.equal(b1, want[1]) and not torch.equal(s0, s1)
