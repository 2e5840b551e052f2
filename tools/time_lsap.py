"""Time the Hungarian assignment of one step (7 outputs x 2 images, 900 queries, 1204 classes) both ways: the host path
(HungarianMatcher.match_many: cost kernels + copy + wait + scipy, wall time) against the device path (match_many_device: cost kernels +
msda_lsap_*, HIP events), per layout of the cost blocks, and the solver kernel alone.  One JSON line per target count.

    python tools/time_lsap.py [--targets 12 100 300] [--calls 20] [--once]      (--once: one device call per size, for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from richsem_amd.matcher import CostPlan, HungarianMatcher, cost_blocks, solve_blocks  # noqa: E402


def events_ms(fn, calls):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=int, nargs="+", default=[12, 100, 300])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--outputs", type=int, default=7)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--queries", type=int, default=900)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    m = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0)
    for T in a.targets:
        targets = [{"labels": torch.randint(1, 1204, (T,), device=dev, generator=g),
                    "boxes": torch.cat((torch.rand(T, 2, device=dev, generator=g) * 0.6 + 0.2, torch.rand(T, 2, device=dev, generator=g) * 0.35 + 0.05), 1)}
                   for _ in range(a.images)]
        outs = [{"pred_logits": torch.randn(a.images, a.queries, 1204, device=dev, generator=g) * 2,
                 "pred_boxes": torch.cat((torch.rand(a.images, a.queries, 2, device=dev, generator=g) * 0.6 + 0.2,
                                          torch.rand(a.images, a.queries, 2, device=dev, generator=g) * 0.35 + 0.05), -1)} for _ in range(a.outputs)]
        plan = CostPlan(targets, dev, torch.float32)
        if a.once:
            m.match_many_device(outs, plan)
            torch.cuda.synchronize()
            continue
        row = {"queries": a.queries, "targets_per_image": T, "outputs": a.outputs, "images": a.images}
        m.match_many(outs, targets)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.calls):
            host = m.match_many(outs, targets)
        row["host_match_many_wall_ms"] = round((time.perf_counter() - t0) / a.calls * 1e3, 3)
        for tm in (False, True):
            tag = "target_major" if tm else "query_major"
            row[f"device_cost_plus_solver_{tag}_ms"] = round(events_ms(lambda: m.match_many_device(outs, plan, target_major=tm), a.calls), 4)
            buf = torch.cat([cost_blocks(o["pred_logits"], o["pred_boxes"], plan, 2.0, 5.0, 2.0, 0.25, target_major=tm) for o in outs])
            row[f"solver_alone_{tag}_ms"] = round(events_ms(lambda: solve_blocks(buf, plan, a.outputs, a.queries, tm), a.calls), 4)
        t0 = time.perf_counter()
        for _ in range(a.calls):
            m.match_many_device(outs, plan)
        row["device_host_time_per_call_ms"] = round((time.perf_counter() - t0) / a.calls * 1e3, 3)      # (enqueue only: nothing waits)
        torch.cuda.synchronize()
        qot, status = m.match_many_device(outs, plan)
        same = all(qot[o, plan.offsets[b] + j.to(dev)].tolist() == i.tolist() for o, per in enumerate(host) for b, (i, j) in enumerate(per))
        row["equal_to_host_assignment"], row["status_ok"] = bool(same), int(status.abs().sum()) == 0
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
