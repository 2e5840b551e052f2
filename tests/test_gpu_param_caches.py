"""GPU (-m gpu): the bf16 layers read their CURRENT fp32 masters after an optimizer step -- eager, inside a captured graph, and in the
three training forms of bench_step.py.

Every bf16 layer keeps derived forms of its parameters (bf16 casts, lin256 / FFN fragment-packed weights, scale-folded convolution packs)
in caches keyed on the parameters' version counters (richsem_amd/param_cache.py).  Fused optimizers do not bump those counters by
themselves, and a graph captured after the caches were warm would read the warm-up buffers forever.  Each check below compares the module
after a step with a FRESH module loaded with the same state_dict (nothing cached), and carries a control: a fresh module loaded with the
weights from BEFORE the step must differ from it by at least ten times the tolerance, so that a stale cache cannot pass."""
import copy
import os

import pytest
import torch

import layer_params as LP
from richsem_amd.capture import capture, capture_stream, graphed_callables, pin_grad_accumulators

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LR = 2e-2        # per-element Adam steps of ~2e-2 against weights of ~0.06: far more than half a bf16 ulp (~1.2e-4 there)
OPTIMIZERS = {
    "sgd_foreach": lambda ps: torch.optim.SGD(ps, lr=LR, foreach=True),
    "sgd_fused": lambda ps: torch.optim.SGD(ps, lr=LR, fused=True),
    "adam_fused": lambda ps: torch.optim.Adam(ps, lr=LR, fused=True),
    "adamw_fused": lambda ps: torch.optim.AdamW(ps, lr=LR, fused=True),
    "adamw_foreach": lambda ps: torch.optim.AdamW(ps, lr=LR, foreach=True),
    "adamw_forloop": lambda ps: torch.optim.AdamW(ps, lr=LR, foreach=False),
}
# mean |got - want| / mean |want| of a module after the step against the fresh module (the same kernels on the same inputs and weights:
# 0 where the kernels are deterministic, atomics' order otherwise).  The controls (stale weights) measure 1e-1 and more.
OUT_TOL, DX_TOL = 1e-3, 1e-2
KINDS = ["msda", "msda_d128", "encoder", "decoder", "stack", "conv", "bottleneck"]


def _mrel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().mean()) / (float(b.abs().mean()) + 1e-30)


def _report(tag, err, ctl):
    if os.environ.get("RICHSEM_REPORT"):
        print(f"[measured] {tag}: error {err:.3g} control {ctl:.3g}", flush=True)


def _case(kind):
    """-> (make: () -> module on the GPU, fwd: (module, x) -> output tensor, x: the bf16 input that carries the input gradient)"""
    from richsem_amd import workload as W
    from richsem_amd.backbone import Bottleneck
    from richsem_amd.conv import ConvBNAct
    from richsem_amd.modules import (MLP, DeformableTransformerDecoderLayer, DeformableTransformerEncoderLayer, MSDeformAttn,
                                     TransformerDecoder, get_reference_points)
    g = torch.Generator(device="cuda").manual_seed(17)
    dev = "cuda"
    C, F, L, H, P = LP.D_MODEL, LP.D_FFN, LP.LEVELS, LP.HEADS, LP.POINTS
    shapes = torch.tensor(LP.SHAPES, dtype=torch.int64, device=dev)
    lsi = torch.cat((shapes.new_zeros(1), shapes.prod(1).cumsum(0)[:-1]))
    N, S, nq = 2, int(shapes.prod(1).sum()), 60
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    if kind in ("msda", "msda_d128"):
        d = 256 if kind == "msda" else 128           # 128: the bf16 casts of _bf16_params; 256: the lin256 packs
        call = W.shrunk(W.call_Dd(2), 4)
        shapes, lsi = W.level_tensors(call, dev)
        q, rp = rnd(call.N, 50, d).to(BF), torch.rand(call.N, 50, 4, 4, device=dev, generator=g) * 0.4 + 0.2
        x = rnd(call.N, call.S, d).to(BF)
        return (lambda: LP.fill(MSDeformAttn(d, 4, 8 if d == 256 else 4, 4), 500).cuda(),
                lambda m, x: m(q, rp, x, shapes, lsi, None), x)
    if kind == "encoder":
        pos = rnd(N, S, C).to(BF)
        ref = get_reference_points(LP.SHAPES, torch.rand(N, L, 2, device=dev, generator=g) * 0.2 + 0.8, dev)

        def make():
            m = LP.fill(DeformableTransformerEncoderLayer(C, F, dropout=0.0, n_levels=L, n_heads=H, n_points=P), 400).cuda()
            m.fused_min_tokens = 0                   # (256 tokens: the fused feed-forward kernel and its packed weights)
            return m
        return make, lambda m, x: m(x, pos, ref, shapes, lsi, None), rnd(N, S, C).to(BF)
    if kind == "decoder":
        qpos, mem = rnd(nq, N, C).to(BF), rnd(S, N, C).to(BF)
        refp = torch.rand(nq, N, L, 4, device=dev, generator=g) * 0.4 + 0.2
        return (lambda: LP.fill(DeformableTransformerDecoderLayer(C, F, dropout=0.0, n_levels=L, n_heads=H, n_points=P), 410).cuda(),
                lambda m, x: m(tgt=x, tgt_query_pos=qpos, tgt_reference_points=refp, memory=mem, memory_level_start_index=lsi,
                               memory_spatial_shapes=shapes),
                rnd(nq, N, C).to(BF))
    if kind == "stack":
        mem, refu = rnd(S, N, C).to(BF), rnd(nq, N, 4)
        vr = torch.rand(N, L, 2, device=dev, generator=g) * 0.2 + 0.8

        def make():
            layer = DeformableTransformerDecoderLayer(C, F, dropout=0.0, n_levels=L, n_heads=H, n_points=P)
            m = TransformerDecoder(layer, 2, torch.nn.LayerNorm(C), d_model=C, query_dim=4, num_feature_levels=L)
            m.bbox_embed = torch.nn.ModuleList([MLP(C, C, 4, 3) for _ in range(2)])
            return LP.fill(m, 420).cuda()

        def fwd(m, x):
            hs, refs = m(tgt=x, memory=mem, refpoints_unsigmoid=refu, level_start_index=lsi, spatial_shapes=shapes, valid_ratios=vr)
            return torch.cat([t.float().flatten() for t in list(hs) + list(refs[1:])])
        return make, fwd, rnd(nq, N, C).to(BF)

    def randomise_bn(m):
        with torch.no_grad():
            for name, b in m.named_buffers():
                b.copy_(torch.rand(b.shape, generator=torch.Generator().manual_seed(len(name))) * 0.5 + (0.75 if "var" in name or
                                                                                                        name.endswith("weight") else -0.25))
        return m
    if kind == "conv":
        return (lambda: randomise_bn(ConvBNAct(64, 128, 3, 1, 1)).cuda(), lambda m, x: m(x), rnd(2, 13, 17, 64).to(BF))
    assert kind == "bottleneck"
    return (lambda: randomise_bn(Bottleneck(128, 32, stride=1, downsample=True)).cuda(), lambda m, x: m(x), rnd(2, 9, 11, 128).to(BF))


def _normalise_grads(params):
    """every gradient scaled to RMS 1: an SGD step of LR then moves the weights by ~LR too (Adam is invariant to the scale)"""
    for p in params:
        if p.grad is not None and float(p.grad.norm()) > 0:
            p.grad.mul_(p.grad.numel() ** 0.5 / p.grad.norm())


def _bf16_changed(mod, before):
    """fraction of the bf16-rounded weights (of the parameters that had a gradient) that a step changed"""
    moved = total = 0
    for n, p in mod.named_parameters():
        if p.grad is not None:
            moved += int((p.detach().to(BF) != before[n]).sum())
            total += p.numel()
    return moved / total


def _fresh(make, state):
    m = make()
    m.load_state_dict(state)
    return m


def _out_and_dx(mod, fwd, x, go):
    xi = x.detach().clone().requires_grad_(True)
    out = fwd(mod, xi)
    (out.float() * go).sum().backward()
    return out.detach().float(), xi.grad.detach().float()


@pytest.mark.parametrize("opt_name", sorted(OPTIMIZERS))
@pytest.mark.parametrize("kind", KINDS)
def test_eager_module_follows_an_optimizer_step(kind, opt_name):
    """forward, backward, optimizer step, forward + backward again: output and input gradient equal a fresh module's with the new weights"""
    torch.manual_seed(3)
    make, fwd, x = _case(kind)
    mod = make()
    go = torch.randn(fwd(mod, x).shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    params = [p for p in mod.parameters() if p.requires_grad]
    opt = OPTIMIZERS[opt_name](params)
    _out_and_dx(mod, fwd, x, go)                       # fills the caches and the gradients
    _normalise_grads(params)
    state0 = copy.deepcopy(mod.state_dict())
    before = {n: p.detach().to(BF) for n, p in mod.named_parameters()}
    opt.step()
    changed = _bf16_changed(mod, before)
    assert changed > 0.5, (kind, opt_name, changed)
    out, dx = _out_and_dx(mod, fwd, x, go)
    want, want_dx = _out_and_dx(_fresh(make, mod.state_dict()), fwd, x, go)
    stale, stale_dx = _out_and_dx(_fresh(make, state0), fwd, x, go)
    err, ctl = _mrel(out, want), _mrel(stale, want)
    derr, dctl = _mrel(dx, want_dx), _mrel(stale_dx, want_dx)
    _report(f"eager {kind} {opt_name} out", err, ctl)
    _report(f"eager {kind} {opt_name} dx", derr, dctl)
    assert ctl >= 10 * OUT_TOL and dctl >= 10 * DX_TOL, (ctl, dctl)
    assert err <= OUT_TOL, (kind, opt_name, err, ctl)
    assert derr <= DX_TOL, (kind, opt_name, derr, dctl)


def _assigned_grads(params, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)


@pytest.mark.parametrize("kind", KINDS)
def test_captured_forward_follows_a_fused_adamw_step(kind):
    """the forward captured into a graph (on the stream it was warmed on) after the caches were warm; a fused AdamW step on assigned
    gradients; the replay must compute with the new weights (the pack kernels are in the graph) -- twice, so that the second step is not
    served by anything the first one left behind"""
    make, fwd, x = _case(kind)
    mod = make()
    params = [p for p in mod.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=LR, fused=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            fwd(mod, x)
        torch.cuda.synchronize()
        graph, static = capture(lambda: fwd(mod, x), side)
        graph.replay()
        torch.cuda.synchronize()
        assert _mrel(static.float(), fwd(_fresh(make, mod.state_dict()), x).float()) <= OUT_TOL
        for step in range(2):
            state0 = copy.deepcopy(mod.state_dict())
            _assigned_grads(params, seed=step)
            before = {n: p.detach().to(BF) for n, p in mod.named_parameters()}
            opt.step()
            assert _bf16_changed(mod, before) > 0.5
            graph.replay()
            torch.cuda.synchronize()
            got = static.detach().float().clone()
            want = fwd(_fresh(make, mod.state_dict()), x).float()
            stale = fwd(_fresh(make, state0), x).float()
            err, ctl = _mrel(got, want), _mrel(stale, want)
            _report(f"captured {kind} step {step}", err, ctl)
            assert ctl >= 10 * OUT_TOL, ctl
            assert err <= OUT_TOL, (kind, step, err, ctl)
    torch.cuda.current_stream().wait_stream(side)
    del graph


class _Bound(torch.nn.Module):
    """a module's forward with everything but the activation bound: what make_graphed_callables takes (tensors in, tensors out)"""

    def __init__(self, mod, fwd):
        super().__init__()
        self.mod, self.fwd = mod, fwd

    def forward(self, x):
        return self.fwd(self.mod, x)


@pytest.mark.parametrize("kind", ["encoder", "bottleneck"])
def test_graphed_callable_follows_a_fused_adamw_step(kind):
    """forward AND backward captured by richsem_amd.capture.graphed_callables (one side stream for the warm-up and the capture,
    AccumulateGrad nodes pinned on it); after a fused AdamW step the replayed output and input gradient (the transposed packs of the
    backward) must equal a fresh module's"""
    make, fwd, x = _case(kind)
    mod = make()
    bound = _Bound(mod, fwd)
    params = [p for p in mod.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=LR, fused=True)
    go = torch.randn(fwd(make(), x).shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    with capture_stream():
        pinned = pin_grad_accumulators(params)      # noqa: F841  (alive to the end: the graphs reuse these nodes)
        _out_and_dx(bound, lambda m, t: m(t), x, go)
        for p in params:
            p.grad = None
        torch.cuda.synchronize()
        gbound = graphed_callables(bound, (x.detach().clone().requires_grad_(True),))
        for step in range(2):
            for p in params:
                p.grad = None
            _out_and_dx(gbound, lambda m, t: m(t), x, go)      # real gradients from the replayed backward
            _normalise_grads(params)
            state0 = copy.deepcopy(mod.state_dict())
            before = {n: p.detach().to(BF) for n, p in mod.named_parameters()}
            opt.step()
            assert _bf16_changed(mod, before) > 0.5
            out, dx = _out_and_dx(gbound, lambda m, t: m(t), x, go)
            torch.cuda.synchronize()
            want, want_dx = _out_and_dx(_fresh(make, mod.state_dict()), fwd, x, go)
            stale, stale_dx = _out_and_dx(_fresh(make, state0), fwd, x, go)
            err, ctl, derr, dctl = _mrel(out, want), _mrel(stale, want), _mrel(dx, want_dx), _mrel(stale_dx, want_dx)
            _report(f"graphed callable {kind} step {step} out", err, ctl)
            _report(f"graphed callable {kind} step {step} dx", derr, dctl)
            assert ctl >= 10 * OUT_TOL and dctl >= 10 * DX_TOL, (ctl, dctl)
            assert err <= OUT_TOL and derr <= DX_TOL, (kind, step, err, derr)


# ---- the composed step (bench_step.py) in its three training forms ---------------------------------------------------------------
H_IMG, W_IMG, BOXES = 256, 320, 5
STEP_LR = 2e-3           # three AdamW steps move the weights by several per cent: the outputs by far more than STEP_TOL
# The step's forward is not bitwise reproducible (measured: 0 in one run, logits 4e-3 / boxes 0.25 in another), and its two-stage top-900
# selection is discrete: a near-tie flipped by that noise swaps proposals and moves the boxes of whole queries.  So the selection of the
# step under test is held fixed in the fresh steps (as tests/test_gpu_step.py holds top-k and assignment); what is left is continuous.
# Stale weights measure 0.5-1.4 (the controls).
STEP_TOL = 1e-2


def _step_outputs(model, images, mask, targets, topk=None):
    """the model part (no teacher) with the two-stage selection ``topk`` held fixed (None: the model's own)"""
    with torch.no_grad():
        return [t.detach().float().clone() for t in model.model_part(images, mask, targets, teacher=False, topk=topk)]


def _fresh_step(state=None, seed=0):
    import bench_step
    m = bench_step.Step(n_img=2, height=H_IMG, width=W_IMG, boxes_per_image=BOXES, seed=seed, dev=torch.device("cuda", 0))
    m.timing = False
    if state is not None:
        m.load_state_dict(state)
    images, mask, targets = m.batch()
    m.prepare(mask, targets)
    m.freeze_noise(3)
    return m, images, mask, targets


def check_trained_step(got, topk, state, seed=0, tag="", scorer_operand=None):
    """``got``: the model-part outputs of a trained step at two-stage selection ``topk``; they must equal a fresh Step's with the trained
    ``state`` (per output: mean relative difference below STEP_TOL) and differ from a fresh Step's with the initial weights by ten times
    that (the control).  ``scorer_operand``: the trained step's two-stage scorer operand, which must be the fresh one's"""
    fresh, images, mask, targets = _fresh_step(state, seed)
    want = _step_outputs(fresh, images, mask, targets, topk)
    if scorer_operand is not None:
        assert torch.equal(scorer_operand, fresh.scorer.packed)
    del fresh
    init, images, mask, targets = _fresh_step(None, seed)
    stale = _step_outputs(init, images, mask, targets, topk)
    del init
    errs = [_mrel(a, b) for a, b in zip(got, want)]
    ctls = [_mrel(a, b) for a, b in zip(stale, want)]
    _report(f"step {tag} outputs", max(errs), max(ctls))
    assert len(got) == len(want)
    assert max(ctls) >= 10 * STEP_TOL, ctls
    assert max(errs) <= STEP_TOL, (tag, errs, ctls)


def test_eager_training_step_reads_the_updated_weights():
    import bench_step
    res = bench_step.run(2, torch.device("cuda", 0), steps=3, warmup=0, graph=False, lr=STEP_LR, noise_seed=3, return_model=True,
                         height=H_IMG, width=W_IMG, boxes_per_image=BOXES, seed=0)
    model = res.pop("model")
    model.timing = False
    images, mask, targets = model.batch()
    got = _step_outputs(model, images, mask, targets)
    topk, operand = model.last_topk.clone(), model.scorer.packed.clone()
    state = copy.deepcopy(model.state_dict())
    del model
    check_trained_step(got, topk, state, tag="eager", scorer_operand=operand)


def test_graphed_training_step_reads_the_updated_weights():
    """bench_step.run_graphed with fused AdamW: the model part's graph (make_graphed_callables) replayed after three steps computes with
    the trained weights"""
    import bench_step
    res = bench_step.run_graphed(2, torch.device("cuda", 0), steps=3, warmup=0, optimizer=True, noise_seed=3, lr=STEP_LR, return_model=True,
                                 height=H_IMG, width=W_IMG, boxes_per_image=BOXES, seed=0)
    model, ga, images = res.pop("model"), res.pop("ga"), res.pop("images")
    got = [t.detach().float().clone() for t in ga(images)]      # (grad mode on: the graphed callable replays its captured forward)
    topk = model.last_topk.clone()                              # (the graph's own output tensor: the replay's selection)
    torch.cuda.synchronize()
    state = copy.deepcopy(model.state_dict())
    del model, ga
    check_trained_step(got, topk, state, tag="graphed")
