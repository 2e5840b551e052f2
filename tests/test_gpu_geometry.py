"""GPU: the batch-geometry tensors from the image sizes (richsem_amd/geometry.py, ``msda_batch_geometry_f32``) against

  * tests/golden/geometry/geometry_reference.npz -- the reference's own ``PositionEmbeddingSineHW``, ``gen_encoder_output_proposals``, ``get_valid_ratio``
    and ``get_reference_points`` run on the CPU on the level masks of the same sizes (tests/golden/make_golden_geometry.py), and
  * the torch composition the kernel replaces, on the GPU: ``Step.prepare``'s geometry lines (``F.interpolate``, ``bench_step.sine_position``,
    ``encoder_output_proposals``, ``get_reference_points``) on the image mask of the same sizes.

(One line of that composition is restated here: the valid ratios are divided by a tensor, not by a Python number -- see ``_torch_geometry``.)

Bounds (``_check``): ``mask_flat``, ``zeroed``, the positions of ``+inf`` and ``valid_ratios`` bit for bit; ``ref`` within 1 float32 ulp (its two
operations are correctly rounded and in the reference's order, so bit equality is what is expected: reported); ``pos_sine`` within 4e-6
absolute -- the arguments lie in [0, 2 pi], where an ulp is 4.8e-7: one rounding of the quotient, one ulp of ``dim_t`` and 2 ulp of sinf / cosf
on each side --; the finite ``proposals`` within 1e-6 absolute (a quotient in (0.0101, 99), logf to a few ulp).  ``RICHSEM_REPORT=1`` prints the
measured maxima (profiles/r15_geometry.md records them).

Then: every nullable output skipped without a byte written outside the others; sizes outside [1, canvas] behave as their clamped values; a
captured call follows the ``sizes`` tensor at replay; and the composed step with ``Step(device_geometry=True)``, eager and graphed.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from richsem_amd import workload as W
from richsem_amd.capture import capture, capture_stream
from richsem_amd.geometry import OUTPUTS, batch_geometry

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry", "geometry_reference.npz")
SMALL = [(64, 96), (72, 104)]      # pyramids 8x12, 4x6, 2x3, 1x2 (a 1-row level) and 9x13, 5x7, 3x4, 2x2 (ceil strides: vh differs from h / stride)
POS_BOUND, PROPOSAL_BOUND = 4e-6, 1e-6
REPORT = bool(os.environ.get("RICHSEM_REPORT"))


def _size_sets(H, Wd):
    return {"main": [(H, Wd), (H // 2 + 3, Wd // 3 + 5), (1, 1)], "edge": [(H, 17), (31, Wd)]}


def _dev():
    return torch.device("cuda", 0)


def _sizes(rows):
    return torch.tensor(rows, dtype=torch.int32).to(_dev())


_torch_cache = {}


def _torch_geometry(sizes, canvas):
    """``Step.prepare``'s geometry lines on the GPU, on the padding mask of images of ``sizes`` in ``canvas``: computed once per case, shared"""
    key = (tuple(map(tuple, sizes)), tuple(canvas))
    if key not in _torch_cache:
        import bench_step
        from richsem_amd.modules import get_reference_points
        dev = _dev()
        mask = torch.ones((len(sizes),) + tuple(canvas), dtype=torch.bool, device=dev)
        for n, (h, w) in enumerate(sizes):
            mask[n, :h, :w] = False
        shapes = list(W.pyramid_shapes(*canvas))
        masks = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in shapes]
        # valid ratios: float(count) / float(extent) as an IEEE division, i.e. by a TENSOR.  ``Step.prepare`` (and the reference's
        # get_valid_ratio) divide by a Python number, which torch evaluates on the GPU as count * (1 / extent): one rounding more, so e.g.
        # 114 / 168 or 3 / 7 comes out one ulp away from the CPU's quotient, the fixture's and the kernel's.  Measured on MI355X with that form:
        # mask_flat / zeroed / +inf still bit-equal, valid_ratios unequal for (64, 96) main, (72, 104) main and edge and E.
        ext = lambda n: torch.tensor(float(n), device=dev)
        st = {"shapes": shapes, "masks": masks, "mask_flat": torch.cat([m.flatten(1) for m in masks], 1),
              "valid_ratios": torch.stack([torch.stack([(~m[:, 0, :]).sum(1).float() / ext(m.shape[2]), (~m[:, :, 0]).sum(1).float() / ext(m.shape[1])], -1)
                                           for m in masks], 1)}
        st["ref"] = get_reference_points(shapes, st["valid_ratios"], dev)
        st["pos_sine"] = torch.cat([bench_step.sine_position(m) for m in masks], 1)
        st["proposals"], st["zeroed"] = bench_step.encoder_output_proposals(st["mask_flat"], shapes)
        _torch_cache[key] = st
    return _torch_cache[key]


def _fixture(canvas, tag):
    z = np.load(GOLDEN)
    key = f"c{canvas[0]}x{canvas[1]}.{tag}."
    dev = _dev()
    shapes = [tuple(int(v) for v in hw) for hw in z[key + "shapes"]]
    masks = [torch.from_numpy(z[f"{key}mask{l}"]).to(dev) for l in range(len(shapes))]
    st = {k: torch.from_numpy(z[key + k]).to(dev) for k in ("valid_ratios", "ref", "pos_sine", "proposals")}
    st.update({"shapes": shapes, "masks": masks, "mask_flat": torch.cat([m.flatten(1) for m in masks], 1), "zeroed": torch.from_numpy(z[key + "zeroed"]).to(dev)[..., None]})
    return [tuple(int(v) for v in hw) for hw in z[key + "sizes"]], tuple(int(v) for v in z[key + "canvas"]), st


def _check(got, want, what, rows=None):
    """the bounds of this file's docstring; ``rows``: compare pos_sine on these rows of (N * S) only.  -> the measured maxima"""
    assert got["shapes"] == [tuple(s) for s in want["shapes"]], what
    assert got["mask_flat"].dtype == torch.bool and torch.equal(got["mask_flat"], want["mask_flat"]), what
    for a, b in zip(got["masks"], want["masks"]):
        assert a.shape == b.shape and torch.equal(a, b), what
    assert torch.equal(got["valid_ratios"], want["valid_ratios"]), (what, got["valid_ratios"], want["valid_ratios"])
    assert got["zeroed"].shape == want["zeroed"].shape and torch.equal(got["zeroed"], want["zeroed"]), what
    assert torch.equal(torch.isposinf(got["proposals"]), torch.isposinf(want["proposals"])), what
    assert torch.equal(torch.isposinf(got["proposals"]).all(-1, keepdim=True), got["zeroed"]), what      # +inf in all four, exactly where zeroed
    fin = torch.isfinite(want["proposals"])
    assert bool(torch.isfinite(got["proposals"][fin]).all()) and bool(fin.any())
    m = {"proposals": float((got["proposals"][fin] - want["proposals"][fin]).abs().max())}
    assert got["ref"].shape == want["ref"].shape and bool((got["ref"] > 0).all())
    ulps = (got["ref"].contiguous().view(torch.int32) - want["ref"].contiguous().view(torch.int32)).abs()
    m["ref_ulp"] = int(ulps.max())
    a, b = got["pos_sine"].flatten(0, 1), want["pos_sine"].flatten(0, 1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if rows is not None:
        a, b = a[rows], b[rows]
    m["pos_sine"] = float((a - b).abs().max())
    if REPORT:
        print(f"[measured] geometry {what}: pos_sine max abs err {m['pos_sine']:.3g}, proposals {m['proposals']:.3g}, ref "
              f"{'bit-equal' if m['ref_ulp'] == 0 else str(m['ref_ulp']) + ' ulp'}", flush=True)
    assert m["ref_ulp"] <= 1, (what, m)
    assert m["pos_sine"] <= POS_BOUND, (what, m)
    assert m["proposals"] <= PROPOSAL_BOUND, (what, m)
    return m


@pytest.mark.parametrize("tag", ["main", "edge"])
@pytest.mark.parametrize("canvas", SMALL, ids=lambda c: f"{c[0]}x{c[1]}")
def test_against_the_reference_fixture_and_the_torch_composition(canvas, tag):
    sizes, fixture_canvas, want = _fixture(canvas, tag)
    assert fixture_canvas == canvas and sizes == _size_sets(*canvas)[tag] and want["shapes"] == [tuple(s) for s in W.pyramid_shapes(*canvas)]
    got = batch_geometry(_sizes(sizes), canvas)
    torch.cuda.synchronize()
    S = sum(h * w for h, w in got["shapes"])
    assert got["pos_sine"].shape == (len(sizes), S, 256) and got["ref"].shape == (len(sizes), S, 4, 2) and got["proposals"].shape == (len(sizes), S, 4)
    assert got["spatial"].tolist() == [list(s) for s in got["shapes"]] and got["lsi"].tolist() == np.cumsum([0] + [h * w for h, w in got["shapes"]])[:-1].tolist()
    _check(got, want, f"{canvas} {tag} against the reference fixture")
    _check(got, _torch_geometry(sizes, canvas), f"{canvas} {tag} against the torch composition")


@pytest.mark.parametrize("canvas,sizes", [((800, 1344), [(800, 1333), (641, 907)]), ((1280, 1280), [(1280, 1280), (1280, 1280)])], ids=["E", "Em"])
def test_full_size_canvases(canvas, sizes):
    """the sizes the step runs at: masks, valid ratios and zeroed rows exactly, pos_sine on a 4096-row sample"""
    got = batch_geometry(_sizes(sizes), canvas)
    want = _torch_geometry(sizes, canvas)
    rows = torch.randperm(got["mask_flat"].numel(), generator=torch.Generator().manual_seed(5))[:4096].to(_dev())
    _check(got, want, f"{canvas} against the torch composition (4096 rows of pos_sine)", rows)
    _torch_cache.clear()      # (45 - 70 MB of pos_sine each)


def _arena_out(shapes, N, want, guard=0xA5, gap=256):
    """buffers for ``batch_geometry(out=...)`` carved out of ONE byte arena filled with ``guard``, ``gap`` guard bytes between them (and a
    carved, unused region for every output that is not wanted) -> (out, arena, [(name, begin, end)] of the buffers in use)"""
    L, S = len(shapes), sum(h * w for h, w in shapes)
    plan = [("mask_flat", torch.bool, (N, S)), ("valid_ratios", torch.float32, (N, L, 2)), ("ref", torch.float32, (N, S, L, 2)),
            ("pos_sine", torch.float32, (N, S, 256)), ("proposals", torch.float32, (N, S, 4)), ("zeroed", torch.bool, (N, S, 1))]
    offs, cur = [], gap
    for name, dt, shape in plan:
        nbytes = int(np.prod(shape)) * (4 if dt == torch.float32 else 1)
        offs.append((name, cur, cur + nbytes))
        cur = (cur + nbytes + gap + 15) // 16 * 16
    arena = torch.full((cur + gap,), guard, dtype=torch.uint8, device=_dev())
    used = {"mask_flat", "valid_ratios"} | set(want) | ({"zeroed"} if "proposals" in want else set())
    out = {"shapes": shapes}
    for (name, dt, shape), (_, a, b) in zip(plan, offs):
        out[name] = arena[a:b].view(dt).view(shape) if name in used else None
    return out, arena, [o for o in offs if o[0] in used]


@pytest.mark.parametrize("want", [(), ("pos_sine",), ("ref",), ("proposals",), ("pos_sine", "ref"), ("ref", "proposals"), OUTPUTS],
                         ids=lambda w: "+".join(w) or "none")
def test_skipped_outputs_leave_their_neighbours_alone(want):
    canvas, sizes = (72, 104), _size_sets(72, 104)["main"]
    shapes = [tuple(s) for s in W.pyramid_shapes(*canvas)]
    full = batch_geometry(_sizes(sizes), canvas)
    out, arena, used = _arena_out(shapes, len(sizes), want)
    got = batch_geometry(_sizes(sizes), canvas, want=want, out=out)
    torch.cuda.synchronize()
    assert got is out
    for k in ("mask_flat", "valid_ratios", "ref", "pos_sine", "proposals", "zeroed"):
        if k in [u[0] for u in used]:
            assert torch.equal(got[k].view(torch.uint8) if got[k].dtype == torch.bool else got[k], full[k].view(torch.uint8) if full[k].dtype == torch.bool else full[k]), k
        else:
            assert got[k] is None, k
    outside = torch.ones_like(arena, dtype=torch.bool)
    for _, a, b in used:
        outside[a:b] = False
    assert bool((arena[outside] == 0xA5).all()), "a byte outside the requested outputs was written"
    assert int(outside.sum()) >= 256 * 7
    fresh = batch_geometry(_sizes(sizes), canvas, want=want)      # (the allocating form: the same keys, None where not wanted)
    assert all((fresh[k] is None) == (out[k] is None) for k in ("ref", "pos_sine", "proposals", "zeroed"))
    with pytest.raises(ValueError, match="other shapes"):
        batch_geometry(_sizes(sizes), canvas, want=tuple(k for k in OUTPUTS if k not in want) or ("ref",), out=out)


def _same(a, b):
    for k in ("mask_flat", "valid_ratios", "ref", "pos_sine", "proposals", "zeroed"):
        assert torch.equal(a[k], b[k]), k      # bit for bit (no NaN anywhere; +inf equals +inf)
    assert all(torch.equal(x, y) for x, y in zip(a["masks"], b["masks"]))


@pytest.mark.parametrize("canvas", SMALL, ids=lambda c: f"{c[0]}x{c[1]}")
def test_sizes_are_clamped_on_the_device(canvas):
    H, Wd = canvas
    wild = [(0, -5), (H + 10, Wd + 99), (H // 2, 10 ** 6), (-(2 ** 31), 2 ** 31 - 1)]
    tame = [(1, 1), (H, Wd), (H // 2, Wd), (1, Wd)]
    _same(batch_geometry(_sizes(wild), canvas), batch_geometry(_sizes(tame), canvas))


def test_a_captured_call_follows_the_sizes_tensor():
    canvas = (72, 104)
    first, second = _size_sets(*canvas)["main"], [(40, 104), (72, 51), (9, 9)]
    with capture_stream() as side:
        sizes = _sizes(first)
        out = batch_geometry(sizes, canvas)      # eager once; its buffers are the graph's static outputs
        torch.cuda.synchronize()
        graph, res = capture(lambda: batch_geometry(sizes, canvas, out=out), side)
        assert res is out
        sizes.copy_(_sizes(second))
        graph.replay()
        torch.cuda.synchronize()
        _same(out, batch_geometry(_sizes(second), canvas))
        sizes.copy_(_sizes(first))
        graph.replay()
        torch.cuda.synchronize()
        _same(out, batch_geometry(_sizes(first), canvas))
    _check(out, _torch_geometry(first, canvas), "captured call, replayed")


# ---- the composed step (tests/test_gpu_step.py's size) ----------------------------------------------------------------------------------------
H, W_IMG, BOXES = 256, 320, 5


def _small_step(**kw):
    import bench_step
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, seed=0, dev=_dev(), **kw)
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    model.freeze_noise(3)
    return model, images, mask, targets


def _run(model, images, mask, targets, indices=None, topk=None):
    for p in model.parameters():
        p.grad = None
    loss = model(images, mask, targets, indices, topk)
    loss.backward()
    return loss.detach()


def test_step_with_device_geometry_agrees_with_the_default_step():
    """eager: ``last_geometry`` against ``prepare()``'s tensors of the default step (the bounds of ``_check``), and -- under frozen noise, equal
    top-k and equal assignment -- a loss within the bf16-against-fp32 bound of tests/test_gpu_step.py (2e-2 relative,
    profiles/r04_bf16_bounds.txt); the difference expected is orders smaller (pos_sine differs by some 1e-7 before it is rounded to bf16)"""
    model, images, mask, targets = _small_step()
    assert model.last_geometry is None and model.sizes is None
    want = {k: model.static[k] for k in ("shapes", "masks", "mask_flat", "valid_ratios", "ref", "pos_sine", "proposals", "zeroed")}
    loss_default = _run(model, images, mask, targets)
    idx = [[(i.clone(), j.clone()) for i, j in per] for per in model.last_indices]
    topk = model.last_topk.clone()
    del model
    dmodel, dimages, dmask, dtargets = _small_step(device_geometry=True)
    assert torch.equal(dimages, images) and dmodel.sizes.tolist() == [[H, W_IMG]] * 2 and "pos_sine" not in dmodel.static
    loss_device = _run(dmodel, dimages, dmask, dtargets, idx, topk)
    _check(dmodel.last_geometry, want, "composed step, eager")
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in (dmodel.level_embed, dmodel.enc_output.weight))
    rel = abs(float(loss_device) - float(loss_default)) / abs(float(loss_default))
    if REPORT:
        print(f"[measured] step loss, default geometry {float(loss_default):.6g}, device geometry {float(loss_device):.6g}: rel {rel:.3g}", flush=True)
    assert torch.isfinite(loss_device) and rel <= 2e-2, (float(loss_default), float(loss_device))


def test_graphed_step_follows_a_second_batch():
    """``run_graphed(device_geometry=True)``: the geometry is inside the captured model part, so a replay on a second batch -- narrower second
    image in the same canvas -- computes THAT batch's geometry (bit for bit an eager call's on the new sizes), and its loss moves"""
    import bench_step
    res = bench_step.run_graphed(2, _dev(), steps=1, warmup=1, optimizer=False, noise_seed=3, return_model=True, device_geometry=True,
                                 height=H, width=W_IMG, boxes_per_image=BOXES, seed=0)
    model, images, step = res["model"], res["images"], res["step"]
    canvas = (model.H, model.Wpad)
    loss_a, loss_a_again = float(step()), float(step())      # the first batch, twice: what two replays of one batch differ by
    torch.cuda.synchronize()
    _same(model.last_geometry, batch_geometry(_sizes([(H, W_IMG)] * 2), canvas))
    second = [(H, W_IMG), (H - 37, W_IMG - 111)]              # (the first image keeps the canvas)
    images[1, :, second[1][0]:, :] = 0.0
    images[1, :, :, second[1][1]:] = 0.0
    model.sizes.copy_(_sizes(second))
    torch.cuda.synchronize()                                  # (the step runs on its own stream: the new batch is in place before it starts)
    loss_b = float(step())
    torch.cuda.synchronize()
    eager = batch_geometry(_sizes(second), canvas)
    _same(model.last_geometry, eager)
    assert bool(eager["mask_flat"][1].any()) and not bool(eager["mask_flat"][0].any())
    if REPORT:
        print(f"[measured] graphed step: first batch {loss_a:.6g} / {loss_a_again:.6g}, second batch {loss_b:.6g}", flush=True)
    assert loss_b == loss_b and abs(loss_b) != float("inf")
    assert loss_b != loss_a and abs(loss_b - loss_a) > abs(loss_a_again - loss_a), (loss_a, loss_a_again, loss_b)
