"""GPU (-m gpu): the composed step of bench_step.py at a small size with ``--grouped-repack`` semantics -- the plan recorded around the
first forward + backward, attached to the library's optimizer, three training steps: after every step each bound form bit-equals a fresh
build from the current masters, ``plan.unbound`` names only caches whose forms no job covers, and the losses are those of the same run
without the plan (same noise, two-stage selection and assignment) within the bound tests/test_gpu_step.py applies to its eager-against-
graphed comparison."""
import pytest
import torch

from test_gpu_repack import _fresh_form, _same_bits

pytestmark = pytest.mark.gpu

H, W_IMG, BOXES = 256, 320, 5      # tests/test_gpu_step.py's reduced Step
LOSS_TOL = 2e-3                     # tests/test_gpu_step.py: |loss - eager loss| < 2e-3 |eager loss| at equal selection and assignment
# owners of caches the plan does not cover (the issue's "out of scope"): the frozen affines' folds, the class scorer's product pack, the
# attention pool's derived forms
NOT_COVERED = ("_folded", "scorer", "attnpool", "_derived_caches", "attn_pool")


def _three_steps(grouped, guide=None):
    import bench_step
    model = bench_step.Step(n_img=2, height=H, width=W_IMG, boxes_per_image=BOXES, seed=0, dev=torch.device("cuda", 0))
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    model.freeze_noise(3)
    params = [p for p in model.parameters() if p.requires_grad]
    opt = bench_step.make_optimizer(params, 2e-4, library=True)
    rp = bench_step.GroupedRepack(grouped)
    rp.attach(opt)
    losses, taken = [], []
    for k in range(3):
        for p in params:
            p.grad = None
        idx, topk = guide[k] if guide is not None else (None, None)
        with rp.recording():
            loss = model(images, mask, targets, idx, topk)
            loss.backward()
        taken.append(([[(i.clone(), j.clone()) for i, j in per] for per in model.last_indices], model.last_topk.clone()))
        bench_step.optimizer_step(opt, params)
        rp.after_step()
        losses.append(float(loss.detach()))
        if grouped:
            plan = rp.plan
            torch.cuda.synchronize()
            stale = [(j.kind, tuple(j.dst.shape)) for j in plan.jobs() if not _same_bits(j.dst, _fresh_form(j))]
            assert not stale, (k, stale[:8])
            assert plan.launches == k + 1, (k, plan.launches)      # the optimizer's refresh and nothing else
    return model, rp.plan, losses, taken


def test_grouped_repack_step_keeps_every_form_fresh_and_trains_like_the_step_without_it():
    model, plan, losses, taken = _three_steps(True)
    assert plan.n_jobs > 100 and len(plan.bindings) > 50, (plan.n_jobs, len(plan.bindings))
    names = plan.unbound_names(model)
    assert all(any(tag in n for tag in NOT_COVERED) for n, _, _ in names), names
    assert all(u["cache"] not in [b.owner for b in plan.bindings if b.slot == u["slot"]] for u in plan.unbound)
    # every layer cache of the transformer and every trained convolution is bound
    from richsem_amd.conv import PackCache
    from richsem_amd.param_cache import VersionCache
    loose = []
    for mname, m in model.named_modules():
        for attr, c in vars(m).items():
            if any(tag in f"{mname}.{attr}" for tag in NOT_COVERED):
                continue
            if isinstance(c, VersionCache) and c._val is not None:
                loose.append(f"{mname}.{attr}")                      # an unbound cache that was used
            if isinstance(c, PackCache) and c._slots:
                loose.append(f"{mname}.{attr}")
    assert not loose, loose
    del model
    torch.cuda.empty_cache()
    _, none, ref, _ = _three_steps(False, guide=taken)
    assert none is None
    print(f"[measured] losses with the plan {losses} without {ref}", flush=True)
    for a, b in zip(losses, ref):
        assert abs(a - b) < LOSS_TOL * abs(b), (losses, ref)
