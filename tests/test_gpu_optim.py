"""GPU (-m gpu): richsem_amd.optim -- gradient clipping + AdamW + EMA in two launches (csrc/msda_optim.h) against the float64 definition
with element-wise bounds (tests/optim_ref.py), against torch's own clip_grad_norm_ + fused AdamW (which must sit inside the same bounds),
exact probes, graph capture, checkpoints in both directions, the packed-weight caches and the composed step."""
import copy
import os

import pytest
import torch

import optim_ref as R
from richsem_amd import _lib
from richsem_amd.capture import capture, capture_stream, pin_grad_accumulators

pytestmark = pytest.mark.gpu

CHUNK = _lib.OPTIM_CHUNK
# 1, 3, 4, 5: below / at / above one float4; CHUNK +- 1 and 2 CHUNK + 3: chunk edges and a scalar tail; 300 one-element tensors: more
# partial sums than a workgroup has threads (256)
SIZES = [1, 3, 4, 5, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 3] + [1] * 300
NO_GRAD = 2                   # the 4-element tensor never has a gradient
VIEW = (3, 5)                 # parameters that are views one float into their storage (4-byte-only aligned), gradient and state aligned:
                              # the element-by-element path, over two chunks for the second
ALL_VIEWS = 6                 # parameter, gradient AND state one float in: scalar head (3), float4 body, scalar tail
GROUPS = [dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1),
          dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0),
          dict(lr=1e-3, betas=(0.95, 0.98), eps=1e-7, weight_decay=1e-4)]
GROUP_OF = [i % 3 for i in range(len(SIZES))]
DEV = "cuda"


def _view(t):
    """the same values one float into a fresh storage"""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:].copy_(t.flatten())
    return base[1:].view(t.shape)


def _params(seed=0, sizes=SIZES):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i, n in enumerate(sizes):
        t = torch.randn(n, generator=gen).to(DEV)
        out.append(torch.nn.Parameter(_view(t) if sizes is SIZES and i in VIEW + (ALL_VIEWS,) else t))
    return out


def _grads(seed, scale=1.0, sizes=SIZES):
    gen = torch.Generator().manual_seed(1000 + seed)
    return [None if sizes is SIZES and i == NO_GRAD else (torch.randn(n, generator=gen) * scale).to(DEV) for i, n in enumerate(sizes)]


def _set_grads(params, grads):
    for i, (p, g) in enumerate(zip(params, grads)):
        p.grad = None if g is None else (_view(g) if len(params) == len(SIZES) and i == ALL_VIEWS else g.clone())


def _optimizer(params, max_norm, groups=GROUPS, group_of=GROUP_OF, drop=()):
    from richsem_amd.optim import ClipAdamW
    opt = ClipAdamW([dict(params=[p for i, p in enumerate(params) if group_of[i] == gi and i not in drop], **G) for gi, G in enumerate(groups)],
                    max_norm=max_norm)
    if len(params) == len(SIZES) and ALL_VIEWS not in drop:
        p = params[ALL_VIEWS]
        opt.state[p] = {"step": torch.zeros((), device=DEV), "exp_avg": _view(torch.zeros_like(p)), "exp_avg_sq": _view(torch.zeros_like(p))}
    opt.init_state()
    return opt


def _torch_optimizer(params, groups=GROUPS, group_of=GROUP_OF):
    return torch.optim.AdamW([dict(params=[p for i, p in enumerate(params) if group_of[i] == gi], **G) for gi, G in enumerate(groups)], fused=True)


def _snap(opt, params):
    """p, m, v (clones) and step (ints) as the optimizer holds them now; zeros / 0 where a parameter has no state yet"""
    p = [x.detach().clone() for x in params]
    st = [opt.state.get(x, {}) for x in params]
    m = [s["exp_avg"].clone() if s else torch.zeros_like(x) for s, x in zip(st, params)]
    v = [s["exp_avg_sq"].clone() if s else torch.zeros_like(x) for s, x in zip(st, params)]
    step = [int(s["step"]) if s else 0 for s in st]
    return p, m, v, step


def _got(opt, params, norm):
    p, m, v, step = _snap(opt, params)
    return {"p": p, "m": m, "v": v, "step": step, "total_norm": norm.detach().clone()}


def _report(tag, ratio):
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] {tag}: worst |err| / bound " + " ".join(f"{k} {v:.3g}" for k, v in ratio.items()), flush=True)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", ["clipping", "not_clipping"])
def test_three_steps_inside_the_bounds_and_so_is_torch(case):
    """every element of p, m, v and total_norm of three steps inside the bound of the float64 definition, each step from the float32 state
    the step started from; the same for torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(fused=True) on the same gradients"""
    max_norm = 0.1 if case == "clipping" else 1e4      # the gradients' norm is ~ 550
    ours, theirs = _params(), _params()
    opt, ref_opt = _optimizer(ours, max_norm), _torch_optimizer(theirs)
    for k in range(3):
        grads = _grads(k, scale=2.0)
        for params, o, mine in ((ours, opt, True), (theirs, ref_opt, False)):
            p, m, v, step = _snap(o, params)
            val, bnd = R.reference(p, grads, m, v, step, GROUPS, GROUP_OF, max_norm)
            _set_grads(params, grads)
            if mine:
                o.step()
                norm = o.total_norm
                assert all(g is None or torch.equal(x.grad, g) for x, g in zip(params, grads))      # the gradient is read, never written
            else:
                norm = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
                o.step()
            got = _got(o, params, norm)
            ratio = R.ratios(got, val, bnd, keys=("p", "m", "v", "total_norm"))
            _report(f"{case} step {k + 1} {'library' if mine else 'torch'}", ratio)
            assert max(ratio.values()) <= 1.0, (case, k, "ours" if mine else "torch", ratio)
            assert got["step"] == val["step"] == [0 if i == NO_GRAD else k + 1 for i in range(len(SIZES))]
    assert (float(opt.total_norm) > max_norm) == (case == "clipping")


def _run(max_norm, grads_list, groups=GROUPS, seed=0, drop=(), sizes=SIZES, group_of=GROUP_OF):
    params = _params(seed, sizes)
    opt = _optimizer(params, max_norm, groups, group_of, drop)
    for grads in grads_list:
        _set_grads(params, grads)
        opt.step()
    return _got(opt, params, opt.total_norm), params, opt


def test_zero_gradients_without_decay_change_nothing():
    nowd = [dict(G, weight_decay=0.0) for G in GROUPS]
    zeros = [None if g is None else torch.zeros_like(g) for g in _grads(0)]
    got, params, _ = _run(0.1, [zeros, zeros], groups=nowd)
    assert _equal(got["p"], [x.detach() for x in _params()])
    assert all(float(x.abs().max()) == 0.0 for x in got["m"] + got["v"])
    assert float(got["total_norm"]) == 0.0
    assert got["step"] == [0 if i == NO_GRAD else 2 for i in range(len(SIZES))]


def test_a_norm_below_max_norm_is_no_clipping_bitwise():
    grads = [_grads(0, 1e-3), _grads(1, 1e-3)]      # norm ~ 0.27
    a, _, _ = _run(10.0, grads)
    assert 0.0 < float(a["total_norm"]) < 10.0
    for other in (0.0, 1e30):
        b, _, _ = _run(other, grads)
        assert all(_equal(a[k], b[k]) for k in ("p", "m", "v")) and torch.equal(a["total_norm"], b["total_norm"])


@pytest.mark.parametrize("k", [-20, 0, 7, 40])
def test_one_power_of_two_is_its_own_norm(k):
    grads = [None if g is None else torch.zeros_like(g) for g in _grads(0)]
    grads[5][CHUNK] = 2.0 ** k            # the second chunk of a tensor on the element-by-element path
    got, _, _ = _run(0.1, [grads])
    assert float(got["total_norm"]) == 2.0 ** k


def test_a_parameter_without_gradient_is_untouched_and_does_not_matter():
    grads = [_grads(0), _grads(1)]
    got, params, opt = _run(0.1, grads)
    fresh = _params()
    assert torch.equal(got["p"][NO_GRAD], fresh[NO_GRAD].detach())
    st = opt.state[params[NO_GRAD]]
    assert float(st["step"]) == 0.0 and float(st["exp_avg"].abs().max()) == 0.0 and float(st["exp_avg_sq"].abs().max()) == 0.0
    without, _, _ = _run(0.1, grads, drop=(NO_GRAD,))
    keep = [i for i in range(len(SIZES)) if i != NO_GRAD]
    for key in ("p", "m", "v"):
        assert _equal([got[key][i] for i in keep], [without[key][i] for i in keep])
    assert torch.equal(got["total_norm"], without["total_norm"])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradients_give_the_nans_torch_gives(bad):
    """an inf: coef = 0, NaN at that element and a zero-gradient update elsewhere; a NaN: NaN everywhere -- the patterns of clip_grad_norm_
    + fused AdamW, and equal values wherever both are finite up to the bounds' scale"""
    grads = _grads(0)
    grads[6][CHUNK + 7] = bad
    got, _, _ = _run(0.1, [grads])
    theirs = _params()
    ref_opt = _torch_optimizer(theirs)
    _set_grads(theirs, grads)
    norm = torch.nn.utils.clip_grad_norm_(theirs, 0.1, foreach=True)
    ref_opt.step()
    want = _got(ref_opt, theirs, norm)
    for key in ("p", "m", "v"):
        a, b = R.nan_pattern(got[key]), R.nan_pattern(want[key])
        assert _equal(a, b), key
        for x, y, nan in zip(got[key], want[key], a):
            assert torch.allclose(x[~nan.to(DEV)], y[~nan.to(DEV)], rtol=1e-5, atol=1e-12), key
    n_nan = sum(int(x.sum()) for x in R.nan_pattern(got["p"]))
    assert n_nan == (1 if bad == float("inf") else sum(SIZES) - SIZES[NO_GRAD])
    assert (torch.isnan(got["total_norm"]) and torch.isnan(want["total_norm"])) or torch.equal(got["total_norm"], want["total_norm"])


def test_two_runs_from_equal_state_are_bitwise_equal():
    grads = [_grads(0, 2.0), _grads(1, 2.0), _grads(2, 2.0)]
    a, _, _ = _run(0.1, grads)
    b, _, _ = _run(0.1, grads)
    assert all(_equal(a[k], b[k]) for k in ("p", "m", "v")) and torch.equal(a["total_norm"], b["total_norm"])


# ---- EMA ----------------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(37, 19)
        self.bn = torch.nn.BatchNorm1d(19)
        self.out = torch.nn.Linear(19, 3)


def _ema_bound(e, m, d):
    e, m = e.double(), m.double()
    want = d * e + (1.0 - d) * m
    return want, R.U * (2 * (d * e).abs() + 2 * (1.0 - d) * m.abs() + want.abs()) + R.TINY


def test_folded_ema_is_inside_its_bound_and_off_means_untouched():
    from richsem_amd.optim import ModelEma
    torch.manual_seed(0)
    model = _Net().to(DEV)
    ema = ModelEma(model, decay=0.97)
    with torch.no_grad():
        model.bn.running_mean.normal_()            # (after the copy: the model's buffers differ from the shadow's)
        model.bn.running_var.uniform_(0.5, 2.0)
        for e in ema.module.parameters():
            e.add_(torch.randn_like(e) * 0.1)      # a shadow that differs from the model
    names = [n for n, _ in model.named_parameters()]
    params = list(model.parameters())
    groups, group_of = GROUPS[:2], [i % 2 for i in range(len(params))]
    from richsem_amd.optim import ClipAdamW
    opt = ClipAdamW([dict(params=[p for i, p in enumerate(params) if group_of[i] == gi], **G) for gi, G in enumerate(groups)], max_norm=0.1)
    opt.attach_ema(ema)
    gen = torch.Generator().manual_seed(3)
    no_grad = names.index("bn.bias")
    shadows = [ema.shadow_of(p) for p in params]

    def one_step(k):
        grads = [None if i == no_grad else torch.randn(p.shape, generator=gen).to(DEV) for i, p in enumerate(params)]
        p, m, v, step = _snap(opt, params)
        before = [e.clone() for e in shadows]
        val, bnd = R.reference(p, grads, m, v, step, groups, group_of, 0.1, ema=before, ema_decay=0.97)
        for x, g in zip(params, grads):
            x.grad = g
        opt.step()
        return before, val, bnd

    before, val, bnd = one_step(0)                    # ema_on is False: the shadows are bitwise untouched, the step is the step
    assert _equal(shadows, before) and not opt.folded()
    got = dict(_got(opt, params, opt.total_norm), ema=before)
    assert max(R.ratios(got, val, bnd, keys=("p", "m", "v", "total_norm")).values()) <= 1.0
    opt.ema_on = True
    state_before = {k: t.clone() for k, t in ema.module.state_dict().items()}
    before, val, bnd = one_step(1)
    got = dict(_got(opt, params, opt.total_norm), ema=[e.clone() for e in shadows])
    ratio = R.ratios(got, val, bnd)
    _report("folded ema", ratio)
    assert max(ratio.values()) <= 1.0, ratio
    assert torch.equal(shadows[no_grad], before[no_grad])                      # no gradient: not folded ...
    assert opt.folded() == frozenset(id(p) for i, p in enumerate(params) if i != no_grad)
    # ... so update() covers it, with the buffers: every state_dict entry is the reference's formula of the model's state now
    model.bn.num_batches_tracked.fill_(11)
    ema.update(model)
    torch.cuda.synchronize()
    for (name, e), m in zip(ema.module.state_dict().items(), model.state_dict().values()):
        if not e.dtype.is_floating_point:
            assert torch.equal(e, (0.97 * state_before[name] + (1.0 - 0.97) * m).to(e.dtype)), name
            continue
        want, bound = _ema_bound(state_before[name], m, 0.97)
        assert float(((e.double() - want).abs() / bound).max()) <= 1.0, name
        assert not torch.equal(e, state_before[name]), name
    ema.set(model)
    assert all(torch.equal(e, m) for e, m in zip(ema.module.state_dict().values(), model.state_dict().values()))
    assert not ema.module.training and model.training


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def _two_layer(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(24, 40), torch.nn.Tanh(), torch.nn.Linear(40, 6)).to(DEV)


def test_captured_step_equals_eager_steps_bitwise_through_a_rebuild_and_a_schedule():
    """backward + opt.step() captured with the gradients allocated inside the capture: three replays = three eager steps; an eager step in
    between (new gradients: the table is rebuilt) does not change what the replay does; a new lr, max_norm and ema_on + sync() + replay = the
    eager schedule (the EMA's switch lives in the device table: flipping it needs no new capture)"""
    from richsem_amd.optim import ClipAdamW, ModelEma
    x = torch.randn(16, 24, generator=torch.Generator().manual_seed(1)).to(DEV)
    graphed, eager = _two_layer(), _two_layer()
    mk = lambda mod: ClipAdamW([dict(params=[mod[0].weight, mod[0].bias], lr=1e-2), dict(params=[mod[2].weight, mod[2].bias], weight_decay=0.0)],
                               lr=3e-3, weight_decay=0.05, max_norm=0.1)
    opt_g, opt_e = mk(graphed), mk(eager)
    ema_g, ema_e = ModelEma(graphed, 0.9), ModelEma(eager, 0.9)
    opt_g.attach_ema(ema_g)
    opt_e.attach_ema(ema_e)
    shadow0 = [e.detach().clone() for e in ema_g.module.parameters()]

    def work(mod, opt):
        for p in mod.parameters():
            p.grad = None
        mod(x).pow(2).sum().backward()
        opt.step()

    def same():
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(list(graphed.parameters()) + list(ema_g.module.parameters()),
                                                     list(eager.parameters()) + list(ema_e.module.parameters()))) \
            and torch.equal(opt_g.total_norm, opt_e.total_norm)

    with capture_stream() as side:
        pinned = pin_grad_accumulators(list(graphed.parameters()) + list(eager.parameters()))      # noqa: F841
        for mod in (graphed, eager):                       # eager warm-up of forward + backward on the capture stream (no step)
            mod(x).pow(2).sum().backward()
            for p in mod.parameters():
                p.grad = None
        opt_g.init_state()
        opt_g.sync()
        torch.cuda.synchronize()
        graph, _ = capture(lambda: work(graphed, opt_g), side)
        assert len(opt_g._captured) == 1
        for _ in range(3):
            graph.replay()
            work(eager, opt_e)
        assert same()
        assert all(float(opt_g.state[p]["step"]) == 3.0 for p in graphed.parameters())
        work(graphed, opt_g)                               # eager, on new gradients: the table is rebuilt
        work(eager, opt_e)
        assert same()
        graph.replay()
        work(eager, opt_e)
        assert same()
        assert all(torch.equal(a, b) for a, b in zip(shadow0, ema_g.module.parameters()))      # ema_on was off so far
        for opt in (opt_g, opt_e):                         # the schedule: lr drop in both groups, no clipping any more, the EMA starts
            for g in opt.param_groups:
                g["lr"] *= 0.1
            opt.max_norm = 0.0
            opt.ema_on = True
        opt_g.sync()
        graph.replay()
        work(eager, opt_e)
        assert same()
        assert not any(torch.equal(a, b) for a, b in zip(shadow0, ema_g.module.parameters()))
        before = [p.detach().clone() for p in graphed.parameters()]
        graph.replay()                                     # (and the replay does move the weights)
        torch.cuda.synchronize()
        assert not any(torch.equal(a, b) for a, b in zip(before, graphed.parameters()))
    del graph


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
def test_state_dict_moves_between_clip_adamw_and_torch_adamw():
    sizes = [5, CHUNK + 1, 33]
    group_of = [0, 1, 2]

    def check_one_step(a_params, a_opt, b_params, b_opt, grads):
        """both optimizers (same state) take one step on ``grads``: each result inside the bound of the definition from the state before"""
        for params, opt in ((a_params, a_opt), (b_params, b_opt)):
            p, m, v, step = _snap(opt, params)
            assert step == [2, 2, 2]
            val, bnd = R.reference(p, grads, m, v, step, GROUPS, group_of, 0.0)
            _set_grads(params, grads)
            opt.step()
            got = _got(opt, params, torch.zeros(()))
            ratio = R.ratios(got, val, bnd, keys=("p", "m", "v"))
            _report("after a checkpoint " + type(opt).__name__, ratio)
            assert max(ratio.values()) <= 1.0, ratio
            assert got["step"] == [3, 3, 3]

    # ours -> torch
    got, params, opt = _run(0.0, [_grads(0, sizes=sizes), _grads(1, sizes=sizes)], sizes=sizes, group_of=group_of)
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref_opt = _torch_optimizer(theirs, group_of=group_of)
    ref_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert ref_opt.param_groups[0]["fused"] is True
    check_one_step(params, opt, theirs, ref_opt, _grads(2, sizes=sizes))
    # torch -> ours
    theirs = _params(1, sizes)
    ref_opt = _torch_optimizer(theirs, group_of=group_of)
    for k in range(2):
        _set_grads(theirs, _grads(k, sizes=sizes))
        ref_opt.step()
    ours = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    opt = _optimizer(ours, 0.0, group_of=group_of)
    opt.load_state_dict(copy.deepcopy(ref_opt.state_dict()))
    check_one_step(ours, opt, theirs, ref_opt, _grads(2, sizes=sizes))


# ---- the packed-weight caches (tests/test_gpu_param_caches.py with this optimizer) -----------------------------------------------------
BF = torch.bfloat16
CACHE_LR, OUT_TOL = 2e-2, 1e-3


def _mrel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().mean()) / (float(b.abs().mean()) + 1e-30)


def _mlp():
    import layer_params as LP
    from richsem_amd.modules import MLP
    return LP.fill(MLP(256, 256, 4, 3), 420).cuda()


def _fresh_mlp(state):
    m = _mlp()
    m.load_state_dict(state)
    return m


@pytest.mark.parametrize("captured", [False, True])
def test_bf16_mlp_reads_the_weights_clip_adamw_wrote(captured):
    """the bf16 MLP keeps lin256-packed weights keyed on the parameters' versions: ClipAdamW is a torch.optim.Optimizer, so param_cache's
    global step hook fires -- after a step the module (eager, or its forward captured into a graph before the step) computes what a fresh
    module with the new weights computes, and not what one with the old weights does (the control)"""
    from richsem_amd.optim import ClipAdamW
    mod = _mlp()
    x = torch.randn(2, 60, 256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(17)).to(BF)
    params = list(mod.parameters())
    opt = ClipAdamW(params, lr=CACHE_LR, weight_decay=1e-4, max_norm=0.1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.no_grad():
            for _ in range(2):
                mod(x)                                     # the caches are warm
        torch.cuda.synchronize()
        if captured:
            with torch.no_grad():
                graph, static = capture(lambda: mod(x), side)
        state0 = copy.deepcopy(mod.state_dict())
        g = torch.Generator(device=DEV).manual_seed(5)
        for p in params:
            p.grad = torch.randn(p.shape, device=DEV, generator=g)
        before = [p.detach().to(BF) for p in params]
        opt.step()
        moved = sum(int((p.detach().to(BF) != b).sum()) for p, b in zip(params, before)) / sum(p.numel() for p in params)
        assert moved > 0.5, moved
        with torch.no_grad():
            if captured:
                graph.replay()
                got = static.float().clone()
            else:
                got = mod(x).float()
            want = _fresh_mlp(mod.state_dict())(x).float()
            stale = _fresh_mlp(state0)(x).float()
        torch.cuda.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    err, ctl = _mrel(got, want), _mrel(stale, want)
    assert ctl >= 10 * OUT_TOL, ctl
    assert err <= OUT_TOL, (captured, err, ctl)


# ---- the composed step --------------------------------------------------------------------------------------------------------------
def test_composed_step_with_the_library_optimizer():
    """bench_step.run_graphed(library=True) on the small Step of tests/test_gpu_step.py: ONE training step; with the gradients that step
    produced, every parameter is inside the bound of the definition from the initial state -- and so is what clip_grad_norm_ + fused AdamW
    make of the same gradients (one step: a comparison of the optimizers, not of chaos in training)"""
    import bench_step
    from richsem_amd.optim import ClipAdamW
    kw = dict(height=256, width=320, boxes_per_image=5, seed=0)
    res = bench_step.run_graphed(2, torch.device("cuda", 0), steps=1, warmup=0, optimizer=True, noise_seed=3, return_grads=True,
                                 return_model=True, library=True, **kw)
    assert res["optimizer"].startswith("ClipAdamW")
    model, grads = res.pop("model"), res["grads"]
    trained = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    del model, res["ga"], res["step"]
    init = bench_step.Step(n_img=2, dev=torch.device("cuda", 0), **kw)
    names = [n for n, p in init.named_parameters() if p.requires_grad]
    p0 = [dict(init.named_parameters())[n].detach().clone() for n in names]
    g = [grads.get(n) for n in names]
    assert sum(x is not None for x in g) > 0.9 * len(names)
    zeros = [torch.zeros_like(x) for x in p0]
    groups = [dict(lr=bench_step.LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)]
    val, bnd = R.reference(p0, g, zeros, zeros, [0] * len(names), groups, [0] * len(names), bench_step.CLIP_MAX_NORM)
    ratio = R.ratios({"p": [trained[n] for n in names]}, val, bnd, keys=("p",))
    _report("composed step library", ratio)
    assert ratio["p"] <= 1.0, ratio
    assert float(val["total_norm"]) > bench_step.CLIP_MAX_NORM      # (clipping was active)
    theirs = [torch.nn.Parameter(x.clone()) for x in p0]
    for x, gi in zip(theirs, g):
        x.grad = None if gi is None else gi.clone()
    opt = bench_step.make_optimizer(theirs, bench_step.LR)
    assert not isinstance(opt, ClipAdamW)                           # (the default stays torch's)
    bench_step.optimizer_step(opt, theirs)
    ratio = R.ratios({"p": [x.detach() for x in theirs]}, val, bnd, keys=("p",))
    _report("composed step torch", ratio)
    assert ratio["p"] <= 1.0, ratio
    moved = sum(int((a != b).sum()) for a, b in zip(p0, (trained[n] for n in names)))
    assert moved > 0.5 * sum(x.numel() for x in p0)
