"""GPU (-m gpu): the composed step of bench_step.py with the Hungarian assignment solved on the device (Step(device_matcher=True),
run_graphed(device_matcher=True)) at the small size of tests/test_gpu_step.py, denoising noise frozen: the same pair set and loss as the
host-matcher step, the whole step captured and replayed with the assignment LIVE inside the graph, and the solver's status surfacing
one step late."""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, W_IMG, BOXES = 256, 320, 5
DEV = torch.device("cuda", 0)


def _small_step(seed=0, device_matcher=True):
    import bench_step
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, seed=seed, dev=DEV, device_matcher=device_matcher)
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    model.freeze_noise(3)
    return model, images, mask, targets


def _pair_set(t):
    return sorted(map(tuple, t.t().tolist()))


def _host_query_of_target(model, outs, targets):
    """what the host matcher (scipy) assigns for these model outputs, as (n_out, targets): the query of every target"""
    lists = model.match(*outs[:4], targets)
    off = model.cost_plan.offsets
    qot = torch.full((len(lists), model.cost_plan.total), -1, dtype=torch.int64)
    for o, per_image in enumerate(lists):
        for b, (i, j) in enumerate(per_image):
            qot[o, off[b] + j] = i
    return qot, lists


def test_pair_set_and_loss_equal_the_host_matcher_step():
    model, images, mask, targets = _small_step()
    assert model.matcher.solver == "host"                  # the default matcher object; the step's option picks the device path
    with torch.no_grad():
        outs = model.model_part(images, mask)
    host_qot, lists = _host_query_of_target(model, outs, targets)
    host = model.pack_indices(lists, targets)
    dev = model.match_device(*outs[:4], targets)
    model.late_status.flush()
    assert model.last_qot.shape == (7, 2 * BOXES) and int(model.last_status.abs().sum()) == 0
    assert torch.equal(model.last_qot.cpu(), host_qot)     # all 7 outputs
    for a, b in zip(dev[2:], host[2:]):
        assert a.shape == b.shape and a.dtype == b.dtype == torch.int64
        assert _pair_set(a) == _pair_set(b)
    assert torch.equal(dev[0], host[0]) and torch.equal(dev[1], host[1])
    la, lb = model.loss_part(*outs, *dev), model.loss_part(*outs, *host)
    print(f"loss device pairs {float(la)!r} host pairs {float(lb)!r} rel {abs(float(la) - float(lb)) / abs(float(lb)):.3e}")
    assert abs(float(la) - float(lb)) <= 2e-5 * abs(float(lb))
    # ... and the step's own forward takes that path: its assignment is the host matcher's for the outputs THAT forward computed
    model.keep_match_outputs = True
    loss = model(images, mask, targets)
    loss.backward()
    model.late_status.flush()
    assert torch.isfinite(loss) and int(model.last_status.abs().sum()) == 0
    assert torch.equal(model.last_qot.cpu(), _host_assignment_of(model, model.last_match_outputs, targets))


def test_whole_step_captures_replays_and_trains():
    import bench_step
    first = bench_step.run_graphed(2, DEV, steps=1, warmup=0, optimizer=True, noise_seed=3, height=H, width=W_IMG, boxes_per_image=BOXES,
                                   seed=0, device_matcher=True)
    later = bench_step.run_graphed(2, DEV, steps=2, warmup=10, optimizer=True, noise_seed=3, height=H, width=W_IMG, boxes_per_image=BOXES,
                                   seed=0, device_matcher=True)
    assert first["loss"] == first["loss"] and later["loss"] == later["loss"]      # not NaN
    assert later["loss"] < first["loss"], (first["loss"], later["loss"])
    assert later["grad_norm"] <= bench_step.CLIP_MAX_NORM * 1.01


def _host_assignment_of(model, outputs, targets):
    lists = model.matcher.match_many(outputs, targets)
    qot = torch.full((len(lists), model.cost_plan.total), -1, dtype=torch.int64)
    for o, per_image in enumerate(lists):
        for b, (i, j) in enumerate(per_image):
            qot[o, model.cost_plan.offsets[b] + j] = i
    return qot


def test_assignment_is_live_inside_the_graph():
    """a second batch of images through the CAPTURED step: the replay's query_of_target is what the host matcher (scipy) returns for the
    model outputs of that batch -- the logits and boxes that replay computed, kept referenced by ``keep_match_outputs`` -- and not the
    first batch's assignment"""
    import bench_step
    res = bench_step.run_graphed(2, DEV, steps=1, warmup=0, optimizer=False, noise_seed=3, return_model=True, height=H, width=W_IMG,
                                 boxes_per_image=BOXES, seed=0, device_matcher=True, keep_match_outputs=True)
    model, images, step = res["model"], res["images"], res["step"]
    targets = model._targets
    assert model.matcher.solver == "host"
    torch.cuda.synchronize()
    first = res["query_of_target"].cpu().clone()
    assert res["query_of_target"] is model.last_qot and int(res["status"].abs().sum()) == 0
    outs_first = [{k: v.clone() for k, v in o.items()} for o in model.last_match_outputs]
    assert torch.equal(first, _host_assignment_of(model, outs_first, targets))
    g = torch.Generator().manual_seed(1234)
    images2 = torch.zeros_like(images)
    images2[..., :W_IMG] = torch.randn(images.shape[0], 3, H, W_IMG, generator=g).to(images.device)
    loss2 = step(images2)                                   # replay of the captured step on the second batch
    torch.cuda.synchronize()
    second = model.last_qot.cpu().clone()
    assert torch.isfinite(loss2)
    outs_second = [{k: v.clone() for k, v in o.items()} for o in model.last_match_outputs]
    assert not torch.equal(outs_second[0]["pred_logits"], outs_first[0]["pred_logits"])      # the replay computed the second batch's outputs
    assert torch.equal(second, _host_assignment_of(model, outs_second, targets))             # the gate
    assert not torch.equal(second, first)


def test_poisoned_logits_raise_one_step_late():
    import bench_step
    res = bench_step.run_graphed(2, DEV, steps=1, warmup=0, optimizer=False, noise_seed=3, return_model=True, height=H, width=W_IMG,
                                 boxes_per_image=BOXES, seed=0, device_matcher=True)
    model, step = res["model"], res["step"]
    step()                                                  # healthy
    with torch.no_grad():
        model.decoder.bbox_embed[5].layers[-1].bias.fill_(float("nan"))      # the last decoder layer's boxes, so its cost blocks, are NaN
    step()                                                  # the poisoned step itself passes: its status is read late
    torch.cuda.synchronize()
    assert model.last_status[5].tolist() == [1, 1] and int((model.last_qot[5] != -1).sum()) == 0      # found by the pre-scan, -1 written
    assert int(model.last_status[:5].abs().sum()) == 0 and int(model.last_status[6].abs().sum()) == 0 and int((model.last_qot[:5] < 0).sum()) == 0
    with pytest.raises(ValueError, match="invalid numeric entries"):
        step()
    # eager form: the same late read
    eager, images, mask, targets = _small_step(seed=1)
    eager(images, mask, targets)
    with torch.no_grad():
        eager.decoder.bbox_embed[5].layers[-1].bias.fill_(float("nan"))
    eager(images, mask, targets)
    with pytest.raises(ValueError, match="invalid numeric entries"):
        eager.late_status.flush()
