"""The dynamic mask head's kernels (csrc/dynamic_masks.hip behind richsem_amd.cond_inst) on the GPU against the reference's numbers
(tests/golden/dynamic_masks/dynamic_masks_reference.npz) and the float64 restatement with its element-wise bounds (tests/dynamic_masks_ref.py):
every output written exactly once into NaN-poisoned buffers with guard rows, exact zeros for rows without a query and queries without a row,
the same bits on every run, exact probes, the 2x rule against the torch composition on the same device, the chain into the mask terms, one
captured graph that serves a second batch, and the memory a call takes.

The figures of the 2x rule (worst over the fixture's cases, kernels / torch composition, relative to the largest reference magnitude;
measured on an MI355X): see profiles/r37_dynamic_masks.md."""
import numpy as np
import pytest
import torch

import dynamic_masks_ref as R
import test_gpu_swin_block as SB
from test_cond_inst_host import DYN, tensors_of
from richsem_amd import _lib, capture, cond_inst, masks

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def identity(N, Q, dead=()):
    inst = np.tile(np.arange(Q), (N, 1))
    for n, q in dead:
        inst[n, q] = -1
    return inst


# the tile dimensions of the kernels: a backward workgroup, and a forward one without up-sampling, takes 8 x 32 pixels; a forward workgroup of
# the x2 map owns 7 x 31 of them (the first row and column are the halo) -- one pixel below, at and above each of the four; a forward workgroup
# takes 16 output rows, four at a time -- 17 rows cross both
EDGES = {
    "h6_w30": R.synthetic(8, 6, 30, 3, [[2, 0], [1, -1]], seed=1),
    "h7_w31": R.synthetic(16, 7, 31, 2, [[1], [0]], seed=2),
    "h8_w32": R.synthetic(8, 8, 32, 2, [[0, 1]], seed=3),
    "h9_w33": R.synthetic(16, 9, 33, 2, [[1, 0], [-1, 1]], seed=4),
    "h9_w33_factor1": R.synthetic(8, 9, 33, 2, [[1, 0]], factor=1, seed=5),
    "h7_w31_factor1": R.synthetic(8, 7, 31, 2, [[0], [1]], factor=1, seed=6),
    "rows17": R.synthetic(8, 3, 4, 17, identity(2, 17, dead=[(0, 3), (1, 16)]), seed=7),
    "rows16_all_live": R.synthetic(16, 2, 3, 16, identity(1, 16), seed=8),
}
SHAPES = {
    "map1x1_q1": R.synthetic(16, 1, 1, 1, [[0], [0]], seed=9),
    "map2x1": R.synthetic(8, 2, 1, 2, [[1, 0]], seed=10),
    "c16_norel_factor1": R.synthetic(16, 5, 7, 3, [[2, 0], [1, -1]], rel=0, factor=1, seed=11),
    "c8_norel": R.synthetic(8, 4, 5, 2, [[0, 1]], rel=0, seed=12),
    "no_live_image": R.synthetic(8, 4, 5, 3, [[-1, -1, -1], [0, 1, 2]], seed=13),
    "one_query_twice": R.synthetic(8, 3, 4, 2, [[1, 1, 0]], seed=14),      # rows naming one query: added in ascending order
}
SYNTHETIC = dict(EDGES, **SHAPES)
CASES = dict(DYN, **SYNTHETIC)
OUTPUTS = ("out", "g_feats", "g_params", "g_ref")


def raw_call(case, dtype):
    """the C entry points on NaN-poisoned outputs with guard rows: -> dict(out, g_feats, g_params, g_ref) on the host"""
    feats, params, ref, sizes, inst, gout = tensors_of(case, "cuda", DT[dtype])
    rel, F = int(case["rel"]), int(case["factor"])
    N, C, H, W = feats.shape
    Q, R_ = params.shape[1], inst.shape[1]
    P = params.shape[2]
    ref2, inst32 = ref[..., :2].contiguous(), inst.to(torch.int32).contiguous()
    dims = (N, C, H, W, Q, R_, rel, F)
    ws = torch.empty(cond_inst.workspace_bytes(N, C, H, W, Q, R_), dtype=torch.uint8, device="cuda")
    out, gf = SB.Poisoned(N * R_ * F * H, F * W, DT[dtype]), SB.Poisoned(N * C * H, W, DT[dtype])
    gp, gr = SB.Poisoned(N * Q, P, DT[dtype]), SB.Poisoned(N * Q, 2, torch.float32)
    L, st = _lib.load(), _lib.raw_stream(feats.device)
    _lib.check(getattr(L, "msda_dynmask_forward_" + dtype)(feats.data_ptr(), params.data_ptr(), ref2.data_ptr(), sizes.data_ptr(),
                                                           inst32.data_ptr(), *dims, out.ptr(), st))
    _lib.check(getattr(L, "msda_dynmask_backward_" + dtype)(gout.data_ptr(), feats.data_ptr(), params.data_ptr(), ref2.data_ptr(), sizes.data_ptr(),
                                                            inst32.data_ptr(), *dims, gp.ptr(), gf.ptr(), gr.ptr(), ws.data_ptr(), st))
    torch.cuda.synchronize()
    return {"out": out.result("out").reshape(N, R_, F * H, F * W).cpu(), "g_feats": gf.result("grad_feat").reshape(N, C, H, W).cpu(),
            "g_params": gp.result("grad_params").reshape(N, Q, P).cpu(), "g_ref": gr.result("grad_ref").reshape(N, Q, 2).cpu()}


_REF = {}


def reference(name, dtype):
    """the restatement of a case, computed once"""
    if (name, dtype) not in _REF:
        _REF[name, dtype] = R.dynamic_masks(CASES[name], out_dtype=dtype)
    return _REF[name, dtype]


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_inside_the_bounds_zeros_exact_and_reproducible(name, dtype):
    case, ref = CASES[name], reference(name, dtype)
    got = raw_call(case, dtype)
    worst = {k: float((np.abs(got[k].double().numpy() - ref[k]) / ref["b_" + k]).max()) for k in OUTPUTS}
    print(f"{name} {dtype}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of the bound")
    for k in OUTPUTS:
        assert worst[k] <= 1.0, (k, worst[k])
    # rows without a query and queries without a row: exact zeros (+0.0: all bits clear)
    inst, Q = case["inst"], case["params"].shape[1]
    for n in range(inst.shape[0]):
        for r in range(inst.shape[1]):
            if not 0 <= inst[n, r] < Q:
                assert not bits(got["out"][n, r]).any(), (n, r)
        for q in range(Q):
            if q not in inst[n].tolist():
                assert not bits(got["g_params"][n, q]).any() and not bits(got["g_ref"][n, q]).any(), (n, q)
        if not (inst[n] >= 0).any():
            assert not bits(got["g_feats"][n]).any(), n
    again = raw_call(case, dtype)
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k


def one_hot_case(C, rel):
    """W0 rows one-hot, W1 = I, w2 one-hot, integer features, coordinates and biases: t = relu(relu(in[c] + b0) + b1) + b2 of one input
    channel c, an integer below 64 -- every output is a multiple of 1 / 4, exact in fp32 and in bf16.  Query q's hidden unit i reads input
    channel (q + i) mod Cin and its w2 takes hidden unit q mod 8: over the Cin queries every slot of W0 and every input channel is placed,
    and with them the coordinates' sign and the + 4."""
    rng = np.random.default_rng(5)
    cin, H, W = C + 2 * rel, 3, 4
    Q = cin
    params = np.zeros((1, Q, R.num_params(C, rel)))
    for q in range(Q):
        W0, W1 = np.zeros((8, cin)), np.eye(8)
        for i in range(8):
            W0[i, (q + i) % cin] = 1.0
        w2 = np.zeros(8)
        w2[q % 8] = 1.0
        params[0, q] = np.concatenate([W0.reshape(-1), W1.reshape(-1), w2, rng.integers(-2, 3, 8), rng.integers(-2, 3, 8), rng.integers(-2, 3, 1)])
    sizes = np.array([[32.0, 32.0]])      # (k / 32) * 32 = k: the coordinates are integers in fp32 too
    ref = np.concatenate([rng.integers(0, 33, (1, Q, 2)) / 32.0, np.full((1, Q, 2), 0.5)], axis=2)
    return {"feats": rng.integers(-3, 4, (1, C, H, W)).astype(np.float64), "params": params, "ref": ref, "sizes": sizes,
            "inst": identity(1, Q), "rel": np.int64(rel), "factor": np.int64(2), "gout": np.zeros((1, Q, 2 * H, 2 * W))}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("C,rel", [(8, 1), (16, 1), (8, 0), (16, 0)])
def test_one_hot_probe_is_exact(C, rel, dtype):
    case = one_hot_case(C, rel)
    want = R.dynamic_masks(case, grads=False)["out"]
    assert (want * 4 == np.round(want * 4)).all() and np.abs(want).max() < 64 and len(np.unique(want)) > 8
    got = raw_call(case, dtype)["out"].double().numpy()
    assert (got == want).all(), np.abs(got - want).max()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dead_hidden_layer_leaves_only_the_last_bias(dtype):
    """zero weights and an all-negative b0: every gradient except b2's is an exact zero, and b2's is the sum of the adjoint"""
    case = dict(CASES["c8_rel_9x13"])
    params = np.zeros_like(case["params"])
    params[..., -25:-17] = -1.0      # b0
    params[..., -1] = 0.5            # b2
    case["params"] = params
    got, ref = raw_call(case, dtype), R.dynamic_masks(case, out_dtype=dtype)
    assert (got["g_feats"] == 0).all() and (got["g_ref"] == 0).all() and (got["g_params"][..., :-1] == 0).all()
    live = case["inst"] >= 0
    assert (got["out"].double().numpy()[live] == 0.5).all()
    db2 = got["g_params"][..., -1].double().numpy()
    assert np.abs(db2).max() > 0 and (np.abs(db2 - ref["g_params"][..., -1]) <= ref["b_g_params"][..., -1]).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_hot_cotangent_places_the_adjoints_taps(dtype):
    """t = feats[2] + 8 through live ReLUs, so grad_feats[2] IS the adjoint of the up-sampling: a one-hot cotangent at an odd-odd, an odd-even,
    an even-even position, the F[0] corner and the last corner gives the taps 1, 1/2, 1/4 where the closed form has them -- exactly"""
    C, H, W = 8, 3, 4
    params = np.zeros((1, 1, 169))
    params[0, 0, 2 + 2] = 1.0          # W0[0, feature 2]
    params[0, 0, 80:144] = np.eye(8).reshape(-1)
    params[0, 0, 144] = 1.0            # w2[0]
    params[0, 0, 152] = 8.0            # b0[0]
    base = {"feats": np.random.default_rng(2).integers(-3, 4, (1, C, H, W)).astype(np.float64), "params": params,
            "ref": np.full((1, 1, 4), 0.5), "sizes": np.array([[24.0, 32.0]]), "inst": np.zeros((1, 1), dtype=np.int64), "rel": np.int64(1),
            "factor": np.int64(2)}
    expect = {(0, 0): {(0, 0): 1.0}, (3, 5): {(1, 2): 1.0}, (3, 4): {(1, 2): 0.5, (1, 1): 0.5}, (2, 4): {(1, 2): 0.25, (1, 1): 0.25, (0, 2): 0.25, (0, 1): 0.25},
              (0, 4): {(0, 2): 0.5, (0, 1): 0.5}, (2, 0): {(1, 0): 0.5, (0, 0): 0.5}, (5, 7): {(2, 3): 1.0}, (4, 6): {(2, 3): 0.25, (2, 2): 0.25, (1, 3): 0.25, (1, 2): 0.25}}
    for (oy, ox), taps in expect.items():
        gout = np.zeros((1, 1, 2 * H, 2 * W))
        gout[0, 0, oy, ox] = 1.0
        got = raw_call(dict(base, gout=gout), dtype)
        want = np.zeros((H, W))
        for (y, x), v in taps.items():
            want[y, x] = v
        assert (got["g_feats"][0, 2].double().numpy() == want).all(), (oy, ox)
        assert (got["g_feats"][0, [0, 1, 3, 4, 5, 6, 7]] == 0).all()
        assert (got["g_feats"].double().numpy() == R.dynamic_masks(dict(base, gout=gout))["g_feats"]).all()
        assert float(got["g_params"][0, 0, 168]) == sum(taps.values())      # b2: the sum of the adjoint


def run_api(fn, case, dtype):
    feats, params, ref, sizes, inst, gout = tensors_of(case, "cuda", DT[dtype])
    for t in (feats, params, ref):
        t.requires_grad_(True)
    out = fn(feats, params, ref, sizes, inst, rel_coord=bool(case["rel"]), mask_out_stride=8 // int(case["factor"]))
    (out * gout).sum().backward()
    g_ref = ref.grad[..., :2] if ref.grad is not None else torch.zeros_like(ref[..., :2])
    return {"out": out.detach(), "g_feats": feats.grad, "g_params": params.grad, "g_ref": g_ref}


def compose_with_table(feats, params, ref, sizes, inst, rel_coord=True, mask_out_stride=4):
    return cond_inst._compose(feats, params, ref, sizes, inst, rel_coord, 8 // mask_out_stride)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_x_rule_against_the_torch_composition(dtype):
    """the kernels' error against the reference's float64 numbers is at most twice that of the torch composition in the same type on the same
    device: per output the worst error over the fixture's cases, relative to the largest magnitude of the reference's output"""
    err = {k: [0.0, 0.0] for k in OUTPUTS}
    for name, case in DYN.items():
        if not (case["inst"] >= 0).any():
            continue
        for i, fn in enumerate((cond_inst._with_table, compose_with_table)):
            got = run_api(fn, case, dtype)
            for k in OUTPUTS:
                if np.abs(case[k]).max() > 0:
                    err[k][i] = max(err[k][i], float(np.abs(got[k].double().cpu().numpy() - case[k]).max() / np.abs(case[k]).max()))
    for k, (ours, theirs) in err.items():
        print(f"2x rule {dtype} {k}: kernels {ours:.3e} torch {theirs:.3e} ratio {ours / max(theirs, 1e-300):.3f}")
    for k, (ours, theirs) in err.items():
        assert ours <= 2 * theirs, (k, ours, theirs)


def test_tables_on_the_device_are_the_host_ones():
    mt = masks.MaskTargets(2, 6, (32, 32), "cuda").update_([{"masks": torch.ones(1, 8, 8, dtype=torch.bool)},
                                                            {"masks": torch.ones(3, 8, 8, dtype=torch.bool)}])
    qot = torch.tensor([2, 0, 7, -1, 3, 1], device="cuda")
    rows = torch.tensor([[2, 4, -1], [0, 0, 3]], device="cuda")
    dims = (2, 8, 3, 4, 4)
    for kw in ({}, {"mask_targets": mt, "query_of_target": qot}, {"rows": rows}):
        dev = cond_inst.table_device(dims, torch.device("cuda"), **kw)
        assert dev.dtype == torch.int32 and torch.equal(dev.long(), cond_inst.table_torch(2, 4, "cuda", **kw)), kw
    # the public forms reach the same rows as the table given
    case = CASES["c8_rel_9x13"]
    feats, params, ref, sizes, inst, _ = tensors_of(case, "cuda", torch.float32)
    with torch.no_grad():
        a = cond_inst.dynamic_masks(feats, params, ref, sizes, rows=inst)
        b = cond_inst._with_table(feats, params, ref, sizes, inst)
        every = cond_inst.dynamic_masks(feats, params, ref, sizes)
    assert torch.equal(a, b) and torch.equal(a[1, 1], every[1, 3]) and not a[0, 2].any()
    with pytest.raises(RuntimeError, match="rows= is forward-only"):
        cond_inst.dynamic_masks(feats.requires_grad_(True), params, ref, sizes, rows=inst)


def chain_buffers(case, device):
    """mask targets for the fixture case c8_rel_9x13 as a training batch: image 0 has targets for queries 2 and 0, image 1 for 1, 3 and 0"""
    gen = torch.Generator().manual_seed(11)
    counts = [int((r >= 0).sum()) for r in case["inst"]]
    tg = [{"masks": torch.rand(c, 60, 90, generator=gen) < 0.4} for c in counts]
    mt = masks.MaskTargets(len(counts), sum(counts) + 2, (64, 96), device).update_(tg)
    qot = torch.full((mt.capacity,), -1, dtype=torch.int64)
    qot[:sum(counts)] = torch.from_numpy(np.concatenate([r[r >= 0] for r in case["inst"]]))
    return mt, qot.to(device), float(sum(counts))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_end_to_end_into_the_mask_terms(dtype):
    """dynamic_masks -> mask_losses -> backward against the float64 composition of both: the 2x rule on the losses and on the three
    gradients, with the torch compositions of both in the same type on the same device as the comparator"""
    case = CASES["c8_rel_9x13"]

    def chain(head, loss, device, dt):
        feats, params, ref, sizes, _, _ = tensors_of(case, device, dt)
        mt, qot, nb = chain_buffers(case, device)
        for t in (feats, params, ref):
            t.requires_grad_(True)
        out = loss(head(feats, params, ref, sizes, mask_targets=mt, query_of_target=qot), mt, qot, nb)
        (0.75 * out["loss_mask"] + 1.5 * out["loss_dice"]).backward()
        return {"loss_mask": out["loss_mask"].detach(), "loss_dice": out["loss_dice"].detach(), "g_feats": feats.grad, "g_params": params.grad,
                "g_ref": ref.grad[..., :2]}

    want = {k: v.numpy() for k, v in chain(cond_inst.dynamic_masks_torch, masks.mask_losses_torch, "cpu", torch.float64).items()}
    ours = chain(cond_inst.dynamic_masks, masks.mask_losses, "cuda", DT[dtype])
    theirs = chain(cond_inst.dynamic_masks_torch, masks.mask_losses_torch, "cuda", DT[dtype])
    for k, w in want.items():
        e = [float(np.abs(g[k].double().cpu().numpy() - w).max() / np.abs(w).max()) for g in (ours, theirs)]
        print(f"end to end {dtype} {k}: kernels {e[0]:.3e} torch {e[1]:.3e}")
        assert e[0] <= 2 * e[1], (k, e)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_captured_graph_serves_a_second_batch(dtype):
    """forward + backward over the matched queries captured once; after update_ with a batch of other counts and another matching the
    replay equals the eager result bit for bit"""
    a = CASES["c8_rel_9x13"]
    b = R.synthetic(8, 9, 13, 4, identity(2, 4, dead=[(0, 0), (0, 1), (0, 3), (1, 2)]), seed=21)
    with capture.capture_stream() as side:
        feats, params, ref, sizes, _, _ = tensors_of(a, "cuda", DT[dtype])
        gout = torch.from_numpy(b["gout"]).to("cuda", DT[dtype])      # (N, Q, 2 H, 2 W): the same cotangent in both batches
        mt, qot, _ = chain_buffers(a, "cuda")
        run = lambda: cond_inst.dynamic_masks_and_grads(feats, params, ref, sizes, gout, mask_targets=mt, query_of_target=qot)      # noqa: E731
        eager_a = run()
        torch.cuda.synchronize()
        graph, out = capture.capture(run, side)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(out, eager_a):
            assert torch.equal(bits(x), bits(y))
        # the second batch: other counts (1 + 3 of capacity 7), another matching, other features, parameters and points
        gen = torch.Generator().manual_seed(12)
        mt.update_([{"masks": torch.rand(1, 50, 96, generator=gen) < 0.4}, {"masks": torch.rand(3, 64, 70, generator=gen) < 0.4}])
        qot.copy_(torch.tensor([2, 0, 3, 1, -1, -1, -1]))
        for dst, k in ((feats, "feats"), (params, "params"), (ref, "ref"), (sizes, "sizes")):
            dst.copy_(torch.from_numpy(b[k]).to(dst.dtype))
        graph.replay()
        torch.cuda.synchronize()
        replay = [t.clone() for t in out]
        eager_b = run()
        torch.cuda.synchronize()
    for x, y in zip(replay, eager_b):
        assert torch.equal(bits(x), bits(y))
    want = R.dynamic_masks(b, out_dtype=dtype)
    for got, k in zip(replay, OUTPUTS):
        assert (np.abs(got.double().cpu().numpy() - want[k]) <= want["b_" + k]).all(), k
    assert not replay[0][0, 0].any() and replay[0][0, 2].any()


def test_memory_is_outputs_gradients_and_workspace():
    """a forward + backward at Q = 64 on 25 x 42: the peak beyond the inputs stays below output + gradients + workspace + the table, the
    float32 copy of the points and 64 KiB -- far below the Q (C + 2) H W floats per image of the repeated input"""
    N, C, H, W, Q = 2, 16, 25, 42, 64
    gen = torch.Generator().manual_seed(6)
    feats, params = torch.randn(N, C, H, W, generator=gen).cuda(), (torch.randn(N, Q, 233, generator=gen) * 0.3).cuda()
    ref, sizes = torch.rand(N, Q, 4, generator=gen).cuda(), torch.tensor([[200.0, 336.0]] * N).cuda()
    gout = torch.randn(N, Q, 2 * H, 2 * W, generator=gen).cuda()
    cond_inst.dynamic_masks_and_grads(feats, params, ref, sizes, gout)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = cond_inst.dynamic_masks_and_grads(feats, params, ref, sizes, gout)
    torch.cuda.synchronize()
    outputs = sum(t.numel() * t.element_size() for t in res)
    extra = torch.cuda.max_memory_allocated() - base - outputs
    ws = cond_inst.workspace_bytes(N, C, H, W, Q, Q)
    print(f"peak beyond the outputs: {extra} bytes, workspace {ws}, repeated input {N * Q * (C + 2) * H * W * 4}")
    assert extra <= ws + N * Q * 4 + N * Q * 2 * 4 + (64 << 10)
    assert extra < N * Q * (C + 2) * H * W * 4
