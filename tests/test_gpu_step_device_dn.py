"""GPU (-m gpu): the composed step with ``Step(device_dn=True)`` -- the denoising queries from one launch that reads the target counts on the
device (richsem_amd/dn.py) -- against the default step's torch composition, on the sizes of tests/test_gpu_geometry.py::_small_step (256 x 320,
5 boxes per image), under frozen noise, equal top-k and equal assignment; and one graphed run.  ``RICHSEM_REPORT=1`` prints the measured
differences."""
import os

import pytest
import torch

import dn_noise_ref as R

pytestmark = pytest.mark.gpu

REPORT = bool(os.environ.get("RICHSEM_REPORT"))
H, W_IMG, BOXES = 256, 320, 5


def _dev():
    return torch.device("cuda", 0)


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
    seen = {}
    hook = model.decoder.register_forward_pre_hook(lambda mod, args, kwargs: seen.update(kwargs), with_kwargs=True)
    loss = model(images, mask, targets, indices, topk)
    hook.remove()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), seen


def test_step_with_device_dn_agrees_with_the_default_step():
    """the decoder's inputs: the denoising rows of ``tgt`` (the embedded noised labels) and the mask bit-equal to the default step's, the noised
    labels and the noised boxes (before inverse_sigmoid) bit-equal slot by slot; the denoising rows of ``refpoints`` (after inverse_sigmoid)
    within three times the bound of tests/test_gpu_dn_queries.py -- the kernel's float64 logarithm is within that bound of the exact value,
    torch's float32 chain within twice it (two roundings of 2^-24 each in front of logf, see
    tests/dn_noise_ref.py q_bbox_bound_float32_chain), so the two are within three times it of each other;
    the loss within the bf16-against-fp32 bound of tests/test_gpu_step.py (2e-2 relative, profiles/r04_bf16_bounds.txt), the difference expected orders smaller"""
    model, images, mask, targets = _small_step()
    loss_default, want = _run(model, images, mask, targets)
    idx = [[(i.clone(), j.clone()) for i, j in per] for per in model.last_indices]
    topk = model.last_topk.clone()
    lay = model.static["lay"]
    pad, bid, slot = lay["pad_size"], lay["known_bid"], lay["map_known_indice"]
    want_lab, want_box = model.last_dn["noised_label"].clone(), model.last_dn["noised_box"].clone()
    del model
    dmodel, dimages, dmask, dtargets = _small_step(device_dn=True)
    assert torch.equal(dimages, images) and dmodel.static["lay"]["pad_size"] == pad == 200
    loss_device, got = _run(dmodel, dimages, dmask, dtargets, idx, topk)
    assert dmodel.last_dn["meta"].tolist() == [BOXES, lay["num_dn_group"], pad, 2 * BOXES, 0]
    assert torch.equal(got["tgt_mask"], want["tgt_mask"]) and got["tgt_mask"].dtype == torch.bool
    assert got["tgt"].dtype == want["tgt"].dtype and torch.equal(got["tgt"].float(), want["tgt"].float())      # (parameters only; no NaN)
    assert torch.equal(dmodel.last_dn["noised_label"][bid, slot], want_lab)
    assert torch.equal(dmodel.last_dn["noised_box"][bid, slot].view(torch.int32), want_box.view(torch.int32))
    assert (dmodel.last_dn["noised_label"] >= 0).sum() == want_lab.numel()      # (5 boxes in both images: every slot is filled)
    ref_got, ref_want = got["refpoints_unsigmoid"][:pad].float(), want["refpoints_unsigmoid"][:pad].float()
    _, bound = R.q_bbox_bound(dmodel.last_dn["noised_box"].cpu().numpy())
    diff = (ref_got - ref_want).abs().transpose(0, 1).double().cpu()
    assert (diff <= 3 * torch.as_tensor(bound)).all(), float((diff / torch.as_tensor(bound)).max())
    g = dmodel.label_enc.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0
    rel = abs(float(loss_device) - float(loss_default)) / abs(float(loss_default))
    if REPORT:
        print(f"[measured] step loss, torch denoising {float(loss_default):.8g}, device denoising {float(loss_device):.8g}: rel {rel:.3g}; "
              f"refpoints max diff / bound {float((diff / torch.as_tensor(bound)).max()):.3g}", flush=True)
    assert torch.isfinite(loss_device) and rel <= 2e-2, (float(loss_default), float(loss_device))


def test_graphed_step_with_device_dn_completes():
    import bench_step
    res = bench_step.run_graphed(2, _dev(), steps=1, warmup=1, optimizer=False, noise_seed=3, device_dn=True, height=H, width=W_IMG,
                                 boxes_per_image=BOXES, seed=0)
    assert res["loss"] == res["loss"] and abs(res["loss"]) != float("inf") and res["grad_norm"] > 0
