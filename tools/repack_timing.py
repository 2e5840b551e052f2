"""Time the re-pack of the derived parameter forms (bf16 casts, lin256 / FFN / convolution packs) of the full-size composed step in its
two forms, and the training step with and without the grouped form:

    baseline   what every replay of a captured step pays today: the caches' own builders (``VersionCache.get``'s ``build``,
               ``conv._pack_form``) of the full-size model, captured into ONE graph and replayed.  The builders are collected by
               wrapping the two ``get`` methods during one eager forward + backward: nothing here needs the grouped re-pack, so this leg
               also runs on a checkout that does not have it.
    grouped    ``RepackPlan.refresh()`` over the same forms (richsem_amd/repack.py, csrc/msda_repack.h), captured and replayed.

``--leg repack``: the two forms ALTERNATE inside one process, round by round, device events around a window of replays; per form the
median over the rounds and the spread (min .. max); launches per replay (torch's profiler, one eager call), the bytes one refresh moves
and their share of the chip's HBM peak (8 TB/s) and of the 6.3 TB/s streaming rate measured on it.
``--leg step``: bench_step.run_graphed with the library optimizer, with and without ``grouped_repack``, in both captured forms
(``graphed_sections``: two graphed callables around the host matcher; ``one_graph``: the device matcher's single callable), alternated.
``--md``: render the JSON documents of the legs into a profile.

    python tools/repack_timing.py --leg repack --out out/repack.json
    python tools/repack_timing.py --leg step --out out/repack_step.json
    python tools/repack_timing.py --md profiles/r23_repack.md out/repack.json out/repack_step.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_BYTES_PER_S = 8.0e12
STREAM_BYTES_PER_S = 6.3e12


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def window(call, calls):
    """GPU ms per call: device events around a window of calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(calls):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def count_launches(call):
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
        key = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][-48:]
        names[key] = names.get(key, 0) + 1
    return {"total": len(dev), "by_name": dict(sorted(names.items(), key=lambda kv: -kv[1])[:12])}


def collect_builders(model, images, mask, targets, plan):
    """one eager forward + backward with both ``get`` methods wrapped -> [(cache, slot, rebuild: () -> forms)] in call order, one entry per
    cache (slot); ``plan``: a RepackPlan to record during that step, or None"""
    import contextlib
    from richsem_amd import conv, param_cache
    seen, entries = set(), []
    vget, pget = param_cache.VersionCache.get, conv.PackCache.get

    def wrapped_vget(self, params, build):
        if (id(self), None) not in seen:
            seen.add((id(self), None))
            entries.append((self, None, build))
        return vget(self, params, build)

    def wrapped_pget(self, weight, scale, transposed):
        if (id(self), transposed) not in seen:
            seen.add((id(self), transposed))
            entries.append((self, transposed, lambda: conv._pack_form(weight, scale, transposed)))
        return pget(self, weight, scale, transposed)

    param_cache.VersionCache.get, conv.PackCache.get = wrapped_vget, wrapped_pget
    try:
        with (plan.record() if plan is not None else contextlib.nullcontext()):
            model(images, mask, targets).backward()
    finally:
        param_cache.VersionCache.get, conv.PackCache.get = vget, pget
    for p in model.parameters():
        p.grad = None
    return entries


def leg_repack(a, dev):
    import bench_step
    from richsem_amd.capture import capture
    try:
        from richsem_amd.repack import RepackPlan
        plan = RepackPlan()
    except ImportError:      # a checkout without the grouped re-pack: the baseline alone
        plan = None
    model = bench_step.Step(n_img=2, dev=dev)
    model.timing = False
    images, mask, targets = model.batch()
    model.prepare(mask, targets)
    res = {"rounds": a.rounds, "replays_per_round": a.calls, "trained_parameters": sum(p.numel() for p in model.parameters() if p.requires_grad)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        entries = collect_builders(model, images, mask, targets, plan)
        if plan is not None:
            bound = {(id(b.owner), b.slot) for b in plan.bindings}
            covered = [e for e in entries if (id(e[0]), e[1]) in bound]
            res["caches_asked"], res["caches_bound"] = len(entries), len(covered)
            res["unbound"] = [f"{n} [{s}]: {r}" for n, s, r in plan.unbound_names(model)]
            res["jobs"], res["chunks"], res["bytes_per_refresh"] = plan.n_jobs, plan.n_chunks, plan.bytes_moved
            kinds = {}
            for j in plan.jobs():
                k = kinds.setdefault(j.kind, [0, 0])
                k[0] += 1
                k[1] += j.dst.numel() * j.dst.element_size()
            res["jobs_by_kind"] = {k: {"jobs": v[0], "destination_bytes": v[1]} for k, v in kinds.items()}
        else:
            covered = entries
            res["caches_asked"] = len(entries)

        def rebuild():
            with torch.no_grad():
                for _, _, build in covered:
                    build()
        forms = {"baseline": rebuild}
        if plan is not None:
            forms["grouped"] = plan.refresh
        for f in forms.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        res["launches_per_replay"] = {k: count_launches(f) for k, f in forms.items()}
        graphs = {k: capture(f, side)[0] for k, f in forms.items()}
        for g in graphs.values():
            g.replay()
        rows = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                rows[k].append(window(g.replay, a.calls))
        res["captured_gpu"] = {k: summary(v) for k, v in rows.items()}
        if plan is not None:
            ms = res["captured_gpu"]["grouped"]["median_ms"]
            rate = plan.bytes_moved / (ms * 1e-3)
            res["captured_gpu"]["grouped"].update({"TB_per_s": round(rate / 1e12, 3), "share_of_8TBps_hbm_peak": round(rate / HBM_PEAK_BYTES_PER_S, 3),
                                                   "share_of_6.3TBps_stream": round(rate / STREAM_BYTES_PER_S, 3)})
        del graphs
        if plan is not None:
            res["grouped_by_kind"] = time_kinds(plan, a)
    torch.cuda.current_stream().wait_stream(side)
    return res


def time_kinds(plan, a):
    """the plan's jobs of each kind as a launch of their own (eager, device events around a window): where the one launch's time goes"""
    import numpy as np
    from richsem_amd import _lib, repack
    out = {}
    for kind in repack.KINDS:
        jobs = [j for j in plan.jobs() if j.kind == kind]
        if not jobs:
            continue
        rows = np.zeros(len(jobs), dtype=repack.JOB_DT)
        for i, j in enumerate(jobs):
            rows[i] = repack.job_row(j.kind, j.dst, j.segments, j.scale)
        chunks = repack.plan_chunks(rows)
        table = torch.from_numpy(np.concatenate([rows.view(np.uint8), chunks.view(np.uint8)])).to(jobs[0].dst.device)
        L, jp, cp, n = _lib.load(), table.data_ptr(), table.data_ptr() + rows.nbytes, len(chunks)

        def call():
            _lib.check(L.msda_repack(jp, cp, n, _lib.raw_stream(table.device)))
        call()
        ms = statistics.median(window(call, a.calls) for _ in range(3))
        moved = sum(sum(t.numel() for t in j.segments) * 4 + j.dst.numel() * j.dst.element_size() for j in jobs)
        out[kind] = {"jobs": len(jobs), "chunks": n, "bytes": moved, "ms": round(ms, 4), "TB_per_s": round(moved / (ms * 1e-3) / 1e12, 3)}
    return out


def leg_step(a, dev):
    import bench_step
    rows = {}
    for _ in range(a.rounds):
        for form, dm in (("graphed_sections", False), ("one_graph", True)):
            for name, grouped in (("without", False), ("grouped_repack", True)):
                r = bench_step.run_graphed(2, dev, steps=a.step_steps, warmup=5, library=True, device_matcher=dm, grouped_repack=grouped)
                rows.setdefault(form, {}).setdefault(name, []).append(r["ms"])
                print(json.dumps({form: {name: r["ms"]}}), file=sys.stderr, flush=True)
                del r
                torch.cuda.empty_cache()
    return {"steps": a.step_steps, "optimizer": "ClipAdamW (library)", "ms": rows}


def render(path, docs):
    d = {}
    for p in docs:
        with open(p) as fh:
            d.update(json.load(fh))
    out = ["# Grouped re-pack: all derived weight forms refreshed in one launch", "",
           "Written by `tools/repack_timing.py --md` from the JSON documents of its legs (one GPU session; each leg a process of its own).", ""]
    if "captured_gpu" in d:
        cg, ln = d["captured_gpu"], d.get("launches_per_replay", {})
        out += ["## The re-pack alone, captured and replayed (full-size composed step, 2 images)", "",
                f"{d['rounds']} rounds of {d['replays_per_round']} replays per form, the forms alternating; device events around each window.", "",
                "| form | launches per replay | GPU ms per replay: median (min .. max) |", "|---|---|---|"]
        for k in ("baseline", "grouped"):
            if k in cg:
                out.append(f"| {k} | {ln.get(k, {}).get('total', 'n/a')} | {cg[k]['median_ms']} ({cg[k]['min_ms']} .. {cg[k]['max_ms']}) |")
        out.append("")
        if "grouped" in cg:
            g = cg["grouped"]
            out += [f"- caches asked during the recorded step: {d['caches_asked']}; bound: {d['caches_bound']}; jobs: {d['jobs']}; chunks "
                    f"(workgroups): {d['chunks']}", f"- bytes one refresh moves (masters read once per job + forms written): {d['bytes_per_refresh']}",
                    f"- achieved: {g['TB_per_s']} TB/s = {g['share_of_8TBps_hbm_peak']} of the 8 TB/s HBM peak, {g['share_of_6.3TBps_stream']} of the "
                    "6.3 TB/s streaming rate measured on this chip",
                    f"- speed-up of the re-pack: {round(cg['baseline']['median_ms'] / g['median_ms'], 2)} x "
                    f"({cg['baseline']['median_ms']} -> {g['median_ms']} ms)", "", "Jobs by kind:", "", "| kind | jobs | destination bytes |", "|---|---|---|"]
            out += [f"| {k} | {v['jobs']} | {v['destination_bytes']} |" for k, v in d.get("jobs_by_kind", {}).items()]
            if "grouped_by_kind" in d:
                out += ["", "Each kind's jobs as a launch of their own (eager, device events; bytes = masters read + forms written):", "",
                        "| kind | jobs | chunks | bytes | ms | TB/s |", "|---|---|---|---|---|---|"]
                out += [f"| {k} | {v['jobs']} | {v['chunks']} | {v['bytes']} | {v['ms']} | {v['TB_per_s']} |" for k, v in d["grouped_by_kind"].items()]
                slow = min(d["grouped_by_kind"].items(), key=lambda kv: kv[1]["TB_per_s"] if kv[1]["bytes"] > 1 << 20 else 1e9)
                out += ["", f"The kinds' times add up to the one launch's; the slowest large kind is `{slow[0]}` at {slow[1]['TB_per_s']} TB/s.  In the "
                        "convolution forward pack a lane's eight k are eight input channels of ONE tap, KH KW floats apart in the master, and the "
                        "16 rows of a lane group are 16 output channels, Cin KH KW floats apart: every load instruction of a wave touches 16 to 64 "
                        "cache lines for 256 useful bytes.  A chunk is one k-step of 256 output channels, so for a 3 x 3 weight the same lines "
                        "are fetched again by eight other workgroups, one per tap.  So the launch waits for the vector memory path's address "
                        "handling and the L2, not for HBM (a reading of the index map, not a counter measurement); a chunk order that lets one "
                        "workgroup take all taps of its channels is the next step and is not taken here.  The transposed forms (`lin256_t`, "
                        "`conv_t`), the suspects beforehand, run faster than the forward pack.  The flat casts and the lin256 order read 32 "
                        "contiguous bytes per lane."]
            out += ["", "Baseline launches by name (most frequent): " + ", ".join(f"{k}: {v}" for k, v in ln.get("baseline", {}).get("by_name", {}).items()), "",
                    "Caches left on their own behaviour (`plan.unbound`):", ""] + [f"- {u}" for u in d.get("unbound", [])] + [""]
    if "ms" in d:
        out += ["## The training step (bench_step.run_graphed, library optimizer), ms per step", "",
                f"{d['steps']} timed steps per run after 5 warm-up steps, host clock around a synchronise; the runs alternate.", "",
                "| captured form | without | with `--grouped-repack` |", "|---|---|---|"]
        for form, v in d["ms"].items():
            out.append(f"| {form} | {', '.join(map(str, v.get('without', [])))} | {', '.join(map(str, v.get('grouped_repack', [])))} |")
        out.append("")
    with open(path, "w") as fh:
        fh.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("repack", "step"))
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--step-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", nargs="+", default=None, metavar=("PROFILE", "JSON"))
    a = ap.parse_args()
    if a.md:
        render(a.md[0], a.md[1:])
        return
    if not torch.cuda.is_available():
        raise SystemExit("repack_timing.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    if a.rounds is None:
        a.rounds = 7 if a.leg == "repack" else 2
    res = leg_repack(a, dev) if a.leg == "repack" else leg_step(a, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
