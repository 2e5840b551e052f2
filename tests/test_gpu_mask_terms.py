"""The mask-loss kernels (csrc/mask_terms.hip behind richsem_amd.masks) on the GPU against the reference's numbers
(tests/golden/mask_terms/mask_terms_reference.npz) and the float64 restatement with its element-wise bounds (tests/mask_terms_ref.py): every output
written exactly once into NaN-poisoned buffers with guard rows, exact zeros where there is no pair, the same bits on every run, the 2x rule
against the torch composition on the same device, a closed-form probe, the tile edges, no float tensor of the canvas' size, and one captured
graph that serves a second batch.

The figures of the 2x rule on the fixture (worst over the cases, kernel / torch composition, relative to the largest reference magnitude; measured
on an MI355X, profiles/r36_mask_terms.md): see the profile."""
import math

import numpy as np
import pytest
import torch

import mask_terms_ref as R
import test_gpu_swin_block as SB
from test_masks_host import LOSS, buffers_of
from richsem_amd import _lib, capture, masks

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def synthetic(h, w, canvas, images, qot, Q=3, seed=0):
    """a case in the fixture's format (without results) from a seed: bf16-exact logits, random masks"""
    gen = torch.Generator().manual_seed(seed)
    N, total = len(images), sum(c for c, _ in images)
    pred = (torch.randn(N, Q, h, w, generator=gen) * 3).bfloat16().double().numpy()
    m = np.zeros((total,) + tuple(canvas), dtype=np.uint8)
    s = 0
    for c, (H, W) in images:
        m[s:s + c, :H, :W] = (torch.rand(c, H, W, generator=gen) < 0.4).numpy()
        s += c
    n_pairs = max(sum(1 for q in qot if q >= 0), 1)
    return {"pred": pred, "counts": np.array([c for c, _ in images]), "mask_hw": np.array([s for _, s in images]), "canvas": np.array(canvas),
            "masks": m, "qot": np.array(qot, dtype=np.int64), "num_boxes": np.float64(n_pairs), "g": np.array([0.75, 1.5])}


# the tile dimensions of the kernels: a forward workgroup sweeps 4096 canvas pixels (8 rows of 512) at a time; a backward workgroup holds
# 1024 source pixels (4 rows of 256; 3 rows from w = 257 on) and 4 canvas rows -- one 32-step below, at and above the sweep, and one source
# column below, at and above the row count's change
EDGES = {
    "w255_480": synthetic(5, 255, (32, 480), [(1, (30, 470)), (1, (32, 480))], [2, 0], seed=1),
    "w256_512": synthetic(5, 256, (32, 512), [(1, (30, 500)), (1, (32, 512))], [1, 2], seed=2),
    "w257_544": synthetic(5, 257, (32, 544), [(1, (20, 544)), (1, (32, 530))], [0, 1], seed=3),
    # down-sizing by 3: the canvas reads source index 3 d + 1 alone (weight 0 on 3 d + 2), two source rows and columns in three are untouched
    "down3": synthetic(96, 96, (32, 32), [(1, (32, 30)), (1, (20, 32))], [1, 0], Q=2, seed=4),
}
CASES = dict(LOSS, **EDGES)


def raw_call(case, dtype, extra=2):
    """the two C entry points on NaN-poisoned outputs with guard rows: -> dict(losses (2,), sums (cap, 4), grad (N, Q, h, w)) on the host"""
    mt, qot = buffers_of(case, "cuda", extra)
    pred = torch.from_numpy(case["pred"]).to("cuda", DT[dtype]).contiguous()
    N, Q, h, w = pred.shape
    dims = (N, Q, h, w) + mt.canvas + (mt.capacity,)
    nb = torch.tensor([float(case["num_boxes"])], dtype=torch.float32, device="cuda")
    g = torch.from_numpy(case["g"]).to("cuda", torch.float32)
    ws = torch.empty(masks.workspace_bytes(*dims), dtype=torch.uint8, device="cuda")
    losses, sums, grad = SB.Poisoned(1, 2, torch.float32), SB.Poisoned(mt.capacity, 4, torch.float32), SB.Poisoned(N * Q * h, w, DT[dtype])
    L, st = _lib.load(), _lib.raw_stream(pred.device)
    _lib.check(getattr(L, "msda_mask_loss_forward_" + dtype)(pred.data_ptr(), mt.masks.data_ptr(), mt.offsets_dev.data_ptr(), qot.data_ptr(),
                                                             nb.data_ptr(), *dims, R.ALPHA, losses.ptr(), sums.ptr(), ws.data_ptr(), st))
    _lib.check(getattr(L, "msda_mask_loss_backward_" + dtype)(pred.data_ptr(), mt.masks.data_ptr(), mt.offsets_dev.data_ptr(), qot.data_ptr(),
                                                              nb.data_ptr(), sums.ptr(), g.data_ptr(), *dims, R.ALPHA, grad.ptr(), ws.data_ptr(), st))
    torch.cuda.synchronize()
    return {"losses": losses.result("losses").reshape(2).cpu(), "sums": sums.result("pair sums").cpu(),
            "grad": grad.result("grad_pred").reshape(N, Q, h, w).cpu()}


_REF = {}


def reference(name, dtype):
    """the restatement of a case, computed once"""
    if (name, dtype) not in _REF:
        _REF[name, dtype] = R.mask_terms(CASES[name], out_dtype=dtype)
    return _REF[name, dtype]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_inside_the_bounds_zeros_exact_and_reproducible(name, dtype):
    case, ref = CASES[name], reference(name, dtype)
    got = raw_call(case, dtype)
    lm, ld, grad = float(got["losses"][0]), float(got["losses"][1]), got["grad"].double().numpy()
    worst = (np.abs(grad - ref["grad"]) / ref["b_grad"]).max()
    print(f"{name} {dtype}: loss_mask {abs(lm - ref['loss_mask']) / ref['b_loss_mask']:.3f} loss_dice "
          f"{abs(ld - ref['loss_dice']) / ref['b_loss_dice']:.3f} grad {worst:.3f} of the bound")
    assert abs(lm - ref["loss_mask"]) <= ref["b_loss_mask"] and abs(ld - ref["loss_dice"]) <= ref["b_loss_dice"]
    assert worst <= 1.0
    # queries without a pair, dead slots and slots without a query: exact zeros (+0.0: all bits clear)
    paired = {(b, q) for _, b, q in R.pairs_of(case)}
    bits = got["grad"].view(torch.int16 if dtype == "bf16" else torch.int32)
    for b in range(grad.shape[0]):
        for q in range(grad.shape[1]):
            if (b, q) not in paired:
                assert not bits[b, q].any(), (b, q)
    live = {s for s, _, _ in R.pairs_of(case)}
    for s in range(got["sums"].shape[0]):
        if s not in live:
            assert not got["sums"][s].view(torch.int32).any(), s
    if not paired:
        assert not got["losses"].view(torch.int32).any()
    again = raw_call(case, dtype)
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_down_sizing_writes_its_zeros(dtype):
    """source pixels no canvas pixel reads come back as written zeros (the poisoned buffer has no NaN left, checked by raw_call), and they are
    where the restatement has them.  At (40, 40) -> (32, 32) every source index is some canvas index's i0 or i1; at (96, 96) -> (32, 32)
    two in three are not."""
    for name in ("s40x40_down", "down3"):
        got = raw_call(CASES[name], dtype)["grad"].double().numpy()
        untouched = reference(name, dtype)["grad"] == 0
        assert (got[untouched] == 0).all()
    assert untouched[0, 1].mean() > 0.8 and untouched[0, 1, 0].all() and not untouched[0, 1, 1, 1]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_two_x_rule_against_the_torch_composition(dtype):
    """the kernels' error against the reference's float64 numbers is at most twice that of the torch composition in the same type on the same
    device: per output the worst error over the fixture's cases, relative to the largest magnitude of the reference's output"""
    err = {k: [0.0, 0.0] for k in ("loss_mask", "loss_dice", "grad")}
    for name, case in LOSS.items():
        if not R.pairs_of(case):
            continue
        mt, qot = buffers_of(case, "cuda")
        pred = torch.from_numpy(case["pred"]).to("cuda", DT[dtype])
        g = torch.from_numpy(case["g"]).to("cuda")
        for i, fn in enumerate((masks.mask_losses, masks.mask_losses_torch)):
            p = pred.clone().requires_grad_(True)
            out = fn(p, mt, qot, float(case["num_boxes"]))
            (g[0].to(out["loss_mask"].dtype) * out["loss_mask"] + g[1].to(out["loss_dice"].dtype) * out["loss_dice"]).backward()
            for k in ("loss_mask", "loss_dice"):
                err[k][i] = max(err[k][i], abs(float(out[k].detach()) - float(case[k])) / abs(float(case[k])))
            err["grad"][i] = max(err["grad"][i], float(np.abs(p.grad.double().cpu().numpy() - case["grad"]).max() / np.abs(case["grad"]).max()))
    for k, (ours, theirs) in err.items():
        print(f"2x rule {dtype} {k}: kernels {ours:.3e} torch {theirs:.3e} ratio {ours / max(theirs, 1e-300):.3f}")
    for k, (ours, theirs) in err.items():
        assert ours <= 2 * theirs, (k, ours, theirs)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_closed_form_probe(dtype):
    """all-zero logits on an all-zero target: 0.75 * 0.25 * ln 2 per pixel, and 1 - 1 / (Hp Wp / 2 + 1)"""
    Hp, Wp = 64, 96
    mt = masks.MaskTargets(2, 3, (Hp, Wp), "cuda").update_([{"masks": torch.zeros(2, 40, 52, dtype=torch.bool)},
                                                           {"masks": torch.zeros(1, 64, 90, dtype=torch.bool)}])
    qot = torch.tensor([0, 2, 1], device="cuda")
    out = masks.mask_losses(torch.zeros(2, 3, 9, 13, dtype=DT[dtype], device="cuda"), mt, qot, 3.0)
    assert abs(float(out["loss_mask"]) - 0.75 * 0.25 * math.log(2)) <= 4 * R.E
    assert abs(float(out["loss_dice"]) - (1 - 1 / (Hp * Wp / 2 + 1))) <= 4 * R.E


def test_no_float_tensor_of_the_canvas_size():
    """one call at 4 pairs on a 256 x 256 canvas: the peak beyond the call's outputs stays below 4 * 256 * 256 * 4 bytes, the size of the one
    float tensor that must not exist"""
    gen = torch.Generator().manual_seed(5)
    tg = [{"masks": torch.rand(2, 256, 256, generator=gen) < 0.4}, {"masks": torch.rand(2, 250, 256, generator=gen) < 0.4}]
    mt = masks.MaskTargets(2, 4, (256, 256), "cuda").update_(tg)
    qot = torch.tensor([1, 3, 0, 2], device="cuda")
    pred = torch.randn(2, 4, 32, 32, generator=gen).cuda()
    masks.mask_losses_and_grads(pred, mt, qot, 4.0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    losses, grad = masks.mask_losses_and_grads(pred, mt, qot, 4.0)
    torch.cuda.synchronize()
    outputs = grad.numel() * grad.element_size() + 2 * 4
    extra = torch.cuda.max_memory_allocated() - base - outputs
    print(f"peak beyond the outputs: {extra} bytes")
    assert extra < 4 * 256 * 256 * 4


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_captured_graph_serves_a_second_batch(dtype):
    """forward + backward captured once; after update_ with a batch of other counts the replay equals the eager result bit for bit"""
    a, b = LOSS["s9x13_inside"], synthetic(9, 13, (64, 96), [(1, (50, 96)), (3, (64, 70))], [1, 2, -1, 0], seed=7)
    with capture.capture_stream() as side:
        mt, qot_a = buffers_of(a, "cuda", extra=3)
        qot = qot_a.clone()
        pred = torch.from_numpy(a["pred"]).to("cuda", DT[dtype]).contiguous()
        nb = torch.tensor([float(a["num_boxes"])], dtype=torch.float32, device="cuda")
        g = torch.from_numpy(a["g"]).to("cuda", torch.float32)      # (the same weights in both batches)
        run = lambda: masks.mask_losses_and_grads(pred, mt, qot, nb, grad_losses=g)      # noqa: E731
        eager_a = run()
        torch.cuda.synchronize()
        graph, out = capture.capture(run, side)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[1].view(torch.uint8), eager_a[1].view(torch.uint8))
        # the second batch: other counts (1 + 3 of capacity 6), an unmatched target, other logits
        from test_masks_host import targets_of
        mt.update_(targets_of(b))
        qot_b = torch.full_like(qot, -1)
        qot_b[:4] = torch.from_numpy(b["qot"]).cuda()
        qot.copy_(qot_b)
        pred.copy_(torch.from_numpy(b["pred"]).to("cuda", DT[dtype]))
        nb.fill_(float(b["num_boxes"]))
        graph.replay()
        torch.cuda.synchronize()
        replay = [out[0]["loss_mask"].clone(), out[0]["loss_dice"].clone(), out[1].clone()]
        eager_b = run()
        torch.cuda.synchronize()
    for x, y in zip(replay, (eager_b[0]["loss_mask"], eager_b[0]["loss_dice"], eager_b[1])):
        assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))
    ref = R.mask_terms(b, out_dtype=dtype)
    assert abs(float(replay[0]) - ref["loss_mask"]) <= ref["b_loss_mask"] and abs(float(replay[1]) - ref["loss_dice"]) <= ref["b_loss_dice"]
    assert (np.abs(replay[2].double().cpu().numpy() - ref["grad"]) <= ref["b_grad"]).all()
