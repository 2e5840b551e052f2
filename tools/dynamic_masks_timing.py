#!/usr/bin/env python3
"""Time the dynamic mask head's kernels (csrc/dynamic_masks.hip through richsem_amd.cond_inst) against the torch forms they replace, in ONE
process, the forms alternating, and write the profile.

    python tools/dynamic_masks_timing.py [--calls 5] [--blocks 5] [--out profiles/r37_dynamic_masks.md] [--json FILE.json]
                                         [--resources usage.txt] [--tests tests.log]

Sizes: N = 2 images, mask features 100 x 168 (stride 8 of an 800 x 1344 canvas), C = 16 channels (P = 233), Q = 900 queries, float32 and
bfloat16.
  * eval over all 900 queries, and over 300 selected rows per image (``rows=``), forward under ``no_grad``;
  * training with 24 and with 200 matched queries (``mask_targets=`` / ``query_of_target=``), forward and forward + backward;
  * the comparator is ``dynamic_masks_torch`` (the definition as einsums over the live rows; same device, same type) and, for the eval over all
    queries, the reference-shaped form as well: the features repeated once per instance and three ``F.conv2d(groups=instances)`` -- where it
    fits in memory;
  * the peak memory either form takes beyond what was allocated before the call;
  * for the all-queries forward the share of the fp32 vector peak (157.3 TFLOPS, the specification's figure; 8 (C + 2) + 64 + 8 fused
    multiply-adds per query and pixel) and of the HBM peak on the output bytes (8.0 TB/s, specification).

Method (tools/convnext_timing.py): every form runs untimed first; then ``--blocks`` blocks per form, the forms alternating, each block
``--calls`` calls between two HIP events on the stream; a cell is the median block and the range over the blocks, in microseconds per call.
``--resources`` takes hipcc's -Rpass-analysis=kernel-resource-usage remarks of dynamic_masks.hip (tools/resource_table.py) and ``--tests`` the
output of ``pytest tests/test_gpu_dynamic_masks.py -s``, whose 2x-rule lines go into the profile.  There is no CPU path."""
import argparse
import contextlib
import datetime
import io
import json
import os
import re
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from richsem_amd import cond_inst, masks                          # noqa: E402
from tools.convnext_timing import run_rows                         # noqa: E402
from tools.mask_terms_timing import peak_extra                     # noqa: E402

HBM_PEAK = 8.0e12       # bytes per second (specification)
VALU_PEAK = 157.3e12    # fp32 vector FLOP per second (specification), a fused multiply-add counted as two
N, C, H, W, Q = 2, 16, 100, 168, 900
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def grouped_conv_form(feats, params, ref, sizes):
    """the reference-shaped form over all queries: the input repeated per instance, three grouped 1x1 convolutions"""
    K = N * Q
    rel = cond_inst._relative_coords(ref.flatten(0, 1), sizes.repeat_interleave(Q, 0), H, W, False, feats.dtype)
    x = torch.cat([rel.view(N, Q, 2, H, W), feats[:, None].expand(N, Q, C, H, W)], dim=2).reshape(1, K * (C + 2), H, W)
    p = params.flatten(0, 1)
    a, b, c = 8 * (C + 2), 8 * (C + 2) + 64, 8 * (C + 2) + 72
    x = F.relu(F.conv2d(x, p[:, :a].reshape(K * 8, C + 2, 1, 1), p[:, c:c + 8].reshape(-1), groups=K))
    x = F.relu(F.conv2d(x, p[:, a:b].reshape(K * 8, 8, 1, 1), p[:, c + 8:c + 16].reshape(-1), groups=K))
    x = F.conv2d(x, p[:, b:c].reshape(K, 8, 1, 1), p[:, c + 16], groups=K)
    return cond_inst.aligned_bilinear(x.view(N, Q, H, W), 2)


def setup(dtype, dev):
    gen = torch.Generator().manual_seed(37)
    feats = torch.randn(N, C, H, W, generator=gen).to(dev, dtype).requires_grad_(True)
    params = (torch.randn(N, Q, cond_inst.num_params(C), generator=gen) * 0.3).to(dev, dtype).requires_grad_(True)
    ref = torch.rand(N, Q, 4, generator=gen).to(dev).requires_grad_(True)
    sizes = torch.tensor([[800.0, 1344.0], [760.0, 1280.0]], device=dev)
    return feats, params, ref, sizes


def no_grad(fn):
    def run():
        with torch.no_grad():
            return fn()
    return run


def rows_of(dtype, dev):
    """-> {shape: {what: {form: callable}}}"""
    feats, params, ref, sizes = setup(dtype, dev)
    gen = torch.Generator().manual_seed(38)
    out = {}
    forms = {"library": no_grad(lambda: cond_inst.dynamic_masks(feats, params, ref, sizes)),
             "torch composition": no_grad(lambda: cond_inst.dynamic_masks_torch(feats, params, ref, sizes))}
    try:
        no_grad(lambda: grouped_conv_form(feats, params, ref, sizes))()
        torch.cuda.synchronize()
        forms["repeated input, grouped conv"] = no_grad(lambda: grouped_conv_form(feats, params, ref, sizes))
    except RuntimeError as e:      # (it does not fit, or the grouped convolution refuses the shape)
        print(json.dumps({"grouped conv form": str(e)[:200]}), flush=True)
        torch.cuda.empty_cache()
    out["eval, all 900 queries"] = {"forward": forms}
    rows = torch.stack([torch.randperm(Q, generator=gen)[:300] for _ in range(N)]).to(dev)
    out["eval, 300 selected rows"] = {"forward": {
        "library": no_grad(lambda: cond_inst.dynamic_masks(feats, params, ref, sizes, rows=rows)),
        "torch composition": no_grad(lambda: cond_inst.dynamic_masks_torch(feats, params, ref, sizes, rows=rows))}}
    for pairs in (24, 200):
        per = pairs // N
        mt = masks.MaskTargets(N, pairs, (32, 32), dev).update_([{"masks": torch.ones(per, 8, 8, dtype=torch.bool)} for _ in range(N)])
        qot = torch.cat([torch.randperm(Q, generator=gen)[:per] for _ in range(N)]).to(dev)
        gout = torch.randn(N, Q, 2 * H, 2 * W, generator=gen).to(dev, dtype)

        def fwd(fn, mt=mt, qot=qot):
            return no_grad(lambda: fn(feats, params, ref, sizes, mask_targets=mt, query_of_target=qot))

        def fb(fn, mt=mt, qot=qot, gout=gout):
            def run():
                feats.grad = params.grad = ref.grad = None
                fn(feats, params, ref, sizes, mask_targets=mt, query_of_target=qot).backward(gout)
            return run
        out[f"training, {pairs} matched"] = {
            "forward": {"library": fwd(cond_inst.dynamic_masks), "torch composition": fwd(cond_inst.dynamic_masks_torch)},
            "forward + backward": {"library": fb(cond_inst.dynamic_masks), "torch composition": fb(cond_inst.dynamic_masks_torch)}}
    return out


def measure(calls, blocks):
    dev = torch.device("cuda", 0)
    recs = []
    for name, dtype in DT.items():
        for shape, whats in rows_of(dtype, dev).items():
            rec = {"name": f"{shape}, {name}", "rows": run_rows(whats, calls, blocks), "elem": 2 if dtype == torch.bfloat16 else 4}
            last = list(whats)[-1]
            rec["peak_of"] = last
            rec["peak_extra_bytes"] = {k: peak_extra(fn) for k, fn in whats[last].items()}
            print(json.dumps({"peak_extra_bytes": rec["peak_extra_bytes"]}), flush=True)
            recs.append(rec)
            torch.cuda.empty_cache()
    return recs


def table_of(recs):
    f = lambda d: f"{d['median_us']:.0f} ({d['min_us']:.0f} .. {d['max_us']:.0f})"      # noqa: E731
    lines = ["| shape | what | form | us per call, median (min .. max over blocks) | / library |", "|---|---|---|---|---|"]
    slower = []
    for r in recs:
        for k, forms in r["rows"].items():
            first = forms["library"]["median_us"]
            for form, v in forms.items():
                lines.append(f"| {r['name']} | {k} | {form} | {f(v)} | {v['median_us'] / first:.2f} |")
                if form != "library" and v["median_us"] < first:
                    slower.append(f"{r['name']}, {k}: the library is SLOWER than the {form} ({first:.0f} us against {v['median_us']:.0f} us)")
    lines += ["", "No measured shape is slower than a torch form." if not slower else "\n".join(slower), "",
              "| shape | peak memory beyond what was allocated before the call | library | " + " | ".join(k for k in ("torch composition", "repeated input, grouped conv")) + " |",
              "|---|---|---|---|---|"]
    for r in recs:
        p = r["peak_extra_bytes"]
        cell = lambda k: f"{p[k] / 1e6:.1f} MB" if k in p else "-"      # noqa: E731
        lines.append(f"| {r['name']} | {r['peak_of']} | {cell('library')} | {cell('torch composition')} | {cell('repeated input, grouped conv')} |")
    lines += ["", "| shape | all-queries forward: us | fused multiply-adds | share of the 157.3 TFLOPS fp32 vector peak | output bytes | GB/s | share of the 8.0 TB/s HBM peak |",
              "|---|---|---|---|---|---|---|"]
    for r in recs:
        if r["name"].startswith("eval, all"):
            us = r["rows"]["forward"]["library"]["median_us"]
            fma = (8 * (C + 2) + 64 + 8) * N * Q * H * W
            nbytes = N * Q * 4 * H * W * r["elem"]
            lines.append(f"| {r['name']} | {us:.0f} | {fma / 1e9:.2f} G | {100 * 2 * fma / (us * 1e-6) / VALU_PEAK:.1f} % | {nbytes / 1e6:.0f} MB | "
                         f"{nbytes / (us * 1e-6) / 1e9:.0f} | {100 * nbytes / (us * 1e-6) / HBM_PEAK:.1f} % |")
    return "\n".join(lines)


def resources_of(path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import resource_table
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        resource_table.main(path, "dynmask_")
    return buf.getvalue().strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r37_dynamic_masks.md"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--tests", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dynamic_masks_timing: no GPU; nothing is measured on a CPU")
    recs = measure(a.calls, a.blocks)
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "?")
    parts = ["# Dynamic mask head: per-query mask logits, forward and backward (`csrc/dynamic_masks.hip`, `richsem_amd/cond_inst.py`)", "",
             "What was built is in DESIGN.md section 9, \"Dynamic mask head\".  Everything below was measured with `tools/dynamic_masks_timing.py` and "
             "the GPU tests of `tests/test_gpu_dynamic_masks.py`; nothing here is a CPU timing.", "",
             f"device: {torch.cuda.get_device_name(0)} ({arch}); torch {torch.__version__}; "
             f"{datetime.date.today().isoformat()}; {a.blocks} blocks of {a.calls} calls per form, alternating", "",
             f"## Timing against the torch forms (N = {N}, C = {C}, {H} x {W}, Q = {Q}; same device, same type)", "", table_of(recs)]
    if a.resources:
        parts += ["", "## Registers and LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "", resources_of(a.resources)]
    if a.tests:
        lines = [ln.strip() for ln in open(a.tests) if re.match(r"\.*(2x rule|end to end|peak beyond)", ln.strip())]
        parts += ["", "## The 2x rule, the chain into the mask terms, the memory of a call (`pytest tests/test_gpu_dynamic_masks.py -s`)", "", "```"] + \
            [re.sub(r"^\.+", "", ln) for ln in lines] + ["```"]
    text = "\n".join(parts)
    print(text)
    for path, body in ((a.out, text + "\n"), (a.json, json.dumps(recs, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(body)


if __name__ == "__main__":
    main()
