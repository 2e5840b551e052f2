"""The sections of the composed step (bench_step.SECTIONS) on the small Step of tests/test_gpu_step.py:

  * the ladder -- the step cut off after each section in turn (``stop_at``): a finite scalar surrogate whose backward reaches exactly the
    parameters of the sections run so far;
  * a choice is an argument -- ``model_part(teacher=..., topk=...)`` and the whole step in either order, with nothing left behind by one call
    that changes the next.

No two forwards are compared bit for bit: the step's forward is not bitwise reproducible (tests/test_gpu_param_caches.py)."""
import pytest
import torch

import bench_step

pytestmark = pytest.mark.gpu

H, W_IMG, BOXES = 256, 320, 5      # pyramid 32 x 40, 16 x 20, 8 x 10, 4 x 5: S = 2100 tokens
# What each section adds to the set of trained parameters its surrogate's backward reaches, as name prefixes.  Taken from the commit before
# the sections were methods (this test body, which uses only ``stop_at``, run there): 42, 59, 155, 166, 168, 342 and 344 names.  The
# backbone's stem and layer1 are frozen.  The decoder refines the boxes itself, so all six ``decoder.bbox_embed`` heads are reached there
# already; the heads add the distillation projection alone.  344 is every trained parameter: the teacher is frozen and the criterion has
# no parameters, so the whole step reaches the SAME set as the last section -- a subset, not a strict one.
ADDS = (("backbone", ("backbone.",)),
        ("input_proj", ("input_proj.", "level_embed")),
        ("encoder", ("encoder.",)),
        ("two_stage", ("enc_output.", "enc_output_norm.", "enc_out_bbox_embed.", "dino_visual_proj.")),
        ("dn", ("label_enc.", "tgt_embed.")),
        ("decoder", ("decoder.",)),
        ("heads", ("proj_dino_hs.",)))
COUNTS = (42, 59, 155, 166, 168, 342, 344)


@pytest.fixture(scope="module")
def small():
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, dev=torch.device("cuda", 0))
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    model.freeze_noise(3)
    return model, images, mask, targets


def _reached(model, images, mask, targets, stop_at):
    """forward + backward of the step cut off after ``stop_at`` -> (loss, the names of the parameters with a gradient)"""
    for p in model.parameters():
        p.grad = None
    model.stop_at = stop_at
    try:
        loss = model(images, mask, targets)
        loss.backward()
    finally:
        model.stop_at = None
    torch.cuda.synchronize()
    return loss.detach(), {n for n, p in model.named_parameters() if p.grad is not None}


def test_the_ladder_names_are_the_sections():
    assert tuple(name for name, _ in ADDS) == bench_step.SECTIONS


def test_the_ladder_reaches_the_parameters_of_the_sections_run_so_far(small):
    model = small[0]
    trained = {n for n, p in model.named_parameters() if p.requires_grad}
    prefixes, before = (), set()
    for (name, adds), count in zip(ADDS, COUNTS):
        loss, got = _reached(*small, name)
        assert loss.dim() == 0 and torch.isfinite(loss), (name, loss)
        prefixes += adds
        assert got == {n for n in trained if n.startswith(prefixes)}, (name, sorted(got ^ {n for n in trained if n.startswith(prefixes)})[:10])
        assert len(got) == count and got > before, (name, len(got))
        before = got
    loss, full = _reached(*small, None)
    assert loss.dim() == 0 and torch.isfinite(loss)
    assert before <= full == trained      # (equal sets: see ADDS)


def _kind(out):
    return "loss" if torch.is_tensor(out) else len(out)


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_a_choice_is_an_argument(small, order):
    model, images, mask, targets = small
    calls = [lambda: model.model_part(images, mask, targets, teacher=False), lambda: model.model_part(images, mask, targets),
             lambda: model(images, mask, targets)]
    want = [5, 6, "loss"]
    if order == "reverse":
        calls, want = calls[::-1], want[::-1]
    with torch.no_grad():
        outs = [c() for c in calls]
    assert [_kind(o) for o in outs] == want
    loss = outs[want.index("loss")]
    assert loss.dim() == 0 and torch.isfinite(loss)
    # the shapes model_part's docstring states
    five, six = outs[want.index(5)], outs[want.index(6)]
    N, Q, C, T = 2, model.static["lay"]["pad_size"] + bench_step.NUM_QUERIES, bench_step.NUM_CLASSES, 2 * BOXES
    shapes = [(6, N, Q, C), (6, N, Q, 4), (N, bench_step.NUM_QUERIES, C), (N, bench_step.NUM_QUERIES, 4), (N, Q, C)]
    assert [tuple(t.shape) for t in five] == shapes
    assert [tuple(t.shape) for t in six] == shapes + [(T, C)]
    assert all(torch.isfinite(t).all() for t in five + six)


def test_topk_is_an_argument_of_model_part(small):
    model, images, mask, targets = small
    with torch.no_grad():
        model.model_part(images, mask, targets, teacher=False)
        own = model.last_topk.clone()
        held = own.flip(1).contiguous()      # the same proposals in another order: a selection the scorer would not return
        assert not torch.equal(held, own)
        model.model_part(images, mask, targets, teacher=False, topk=held)
        assert model.last_topk is held
        model.model_part(images, mask, targets, teacher=False)
        assert model.last_topk is not held and model.last_topk.shape == own.shape      # nothing of the held selection stays behind
