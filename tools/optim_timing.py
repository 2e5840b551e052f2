"""Time the tail of the training step -- gradient clipping + AdamW -- in its two forms, on synthetic tensors with the composed step's
trained-parameter sizes (no model is built):

    torch     torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(fused=True).step()      (bench_step.optimizer_step)
    library   richsem_amd.optim.ClipAdamW.step()                                                       (two launches, csrc/msda_optim.h)

Eager: host time per call (the enqueue, no synchronise inside the window) and GPU time per call (device events around a window of
calls).  Captured: each form captured once into a graph, GPU time per replay (torch's fused AdamW must be ``capturable=True`` to be
captured at all: its step counters then live on the device as the library's do).  ``eager_rebuild``: the library's eager call when the
gradients' addresses change every step (its table is rebuilt and uploaded).  The two forms ALTERNATE inside one process, round by round;
per form the median over the rounds and the spread (min .. max) are reported, so a difference can be read against the spread of the same
code.  Bytes: 4 per parameter for the norm, 16 read + 12 written for the update = 32 B per parameter, against the 6.3 TB/s streaming rate
measured on this chip.  ``--step``: also bench_step.run_graphed (the composed step's ``graphed_sections``) with and without the library
optimizer, alternated.

    python tools/optim_timing.py [--rounds 7] [--calls 20] [--step] [--out FILE]      -> one JSON document
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (numel, how many) of the trained parameters of bench_step.Step: 344 tensors, 48 097 308 elements
STEP_SIZES = [(4, 7), (128, 12), (256, 147), (768, 6), (1024, 9), (2048, 12), (32768, 13), (65536, 65), (131072, 4), (147456, 4),
              (196608, 6), (230400, 1), (262144, 14), (308480, 1), (524288, 27), (589824, 6), (1048576, 5), (2097152, 1), (2359296, 3),
              (4718592, 1)]
MAX_NORM, LR, WD = 0.1, 1e-4, 1e-4
STREAM_BYTES_PER_S = 6.3e12
BYTES_PER_PARAM = 32


def make_params(dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    sizes = [n for n, k in STEP_SIZES for _ in range(k)]
    params = [torch.nn.Parameter(torch.randn(n, device=dev, generator=gen) * 0.05) for n in sizes]
    grads = [[torch.randn(n, device=dev, generator=gen) * 0.01 for n in sizes] for _ in range(2)]
    return params, grads


def set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g


def forms(dev):
    from richsem_amd.optim import ClipAdamW
    out = {}
    for name in ("torch", "library"):
        params, grads = make_params(dev, 0)
        set_grads(params, grads[0])
        if name == "torch":
            opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, fused=True)

            def call(params=params, opt=opt):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
                opt.step()
        else:
            opt = ClipAdamW(params, lr=LR, weight_decay=WD, max_norm=MAX_NORM)
            call = opt.step
        out[name] = dict(params=params, grads=grads, opt=opt, call=call)
    return out


def window(call, calls):
    """-> (host ms per call: the enqueue only, GPU ms per call: events around the window)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    host = (time.perf_counter() - t0) / calls * 1e3
    b.record()
    torch.cuda.synchronize()
    return host, a.elapsed_time(b) / calls


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def count_launches(call):
    """kernels and copies one call enqueues (torch's profiler, one call)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            call()
            torch.cuda.synchronize()
    except Exception as e:      # noqa: BLE001  (a profiler that cannot start must not take the timings down)
        return {"error": f"{type(e).__name__}: {str(e)[:200]}"}
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    names = {}
    for e in dev:
        names[e.name[:60]] = names.get(e.name[:60], 0) + 1
    return {"total": len(dev), "by_name": names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also the composed step's graphed_sections with and without the library optimizer")
    ap.add_argument("--step-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_timing.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    n_params = sum(n * k for n, k in STEP_SIZES)
    res = {"tensors": sum(k for _, k in STEP_SIZES), "parameters": n_params, "bytes_per_call": n_params * BYTES_PER_PARAM,
           "least_ms_at_6.3TBps": round(n_params * BYTES_PER_PARAM / STREAM_BYTES_PER_S * 1e3, 4), "rounds": a.rounds, "calls_per_round": a.calls}
    f = forms(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for v in f.values():
            for _ in range(3):
                v["call"]()
        torch.cuda.synchronize()
        res["launches"] = {k: count_launches(v["call"]) for k, v in f.items()}
        # ---- eager, alternated ----
        rows = {k: {"host": [], "gpu": []} for k in f}
        rows["library_rebuild"] = {"host": [], "gpu": []}
        lib, flip = f["library"], [0]

        def rebuild_call():
            flip[0] ^= 1
            set_grads(lib["params"], lib["grads"][flip[0]])
            lib["call"]()
        for _ in range(a.rounds):
            for k, v in f.items():
                h, g = window(v["call"], a.calls)
                rows[k]["host"].append(h)
                rows[k]["gpu"].append(g)
            h, g = window(rebuild_call, a.calls)
            rows["library_rebuild"]["host"].append(h)
            rows["library_rebuild"]["gpu"].append(g)
        set_grads(lib["params"], lib["grads"][0])
        res["eager"] = {k: {"host": summary(v["host"]), "gpu": summary(v["gpu"])} for k, v in rows.items()}
        # ---- captured, alternated ----
        from richsem_amd.capture import capture
        cap = forms(dev)
        cap["torch"]["opt"] = torch.optim.AdamW(cap["torch"]["params"], lr=LR, weight_decay=WD, fused=True, capturable=True)

        def torch_call(params=cap["torch"]["params"], opt=cap["torch"]["opt"]):
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, foreach=True)
            opt.step()
        cap["torch"]["call"] = torch_call
        graphs = {}
        for k, v in cap.items():
            for _ in range(3):
                v["call"]()
            torch.cuda.synchronize()
            graphs[k] = capture(v["call"], side)[0]
        rows = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                rows[k].append(window(g.replay, a.calls)[1])
        res["captured_gpu"] = {k: summary(v) for k, v in rows.items()}
        for k in ("torch", "library"):
            ms = res["captured_gpu"][k]["median_ms"]
            res["captured_gpu"][k]["TB_per_s"] = round(n_params * BYTES_PER_PARAM / (ms * 1e-3) / 1e12, 3)
            res["captured_gpu"][k]["share_of_6.3TBps"] = round(n_params * BYTES_PER_PARAM / (ms * 1e-3) / STREAM_BYTES_PER_S, 3)
        del graphs
    torch.cuda.current_stream().wait_stream(side)
    if a.step:
        import bench_step
        rows = {"torch": [], "library": []}
        for _ in range(2):
            for name, library in (("torch", False), ("library", True)):
                r = bench_step.run_graphed(2, dev, steps=a.step_steps, warmup=5, library=library)
                rows[name].append(r["ms"])
                torch.cuda.empty_cache()
        res["graphed_sections_ms"] = rows
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
