#!/usr/bin/env python3
"""Tuning aid: host time per call (Python shim + ctypes + the library's planning) against the GPU time of the call.  The operator's forward
and backward, and the fused entry point msda_forward_prep_f32 (MSDeformAttnFusedFunction: fwd_prep_fused = 1 for the decoder-shaped call
Dd -- one launch --, 2 for the encoder-shaped call E -- the fused window kernel)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from richsem_amd import _lib, workload as W                       # noqa: E402
from richsem_amd import MultiScaleDeformableAttention as MSDA    # noqa: E402
from richsem_amd.functions import MSDeformAttnFusedFunction      # noqa: E402


def prep_inputs(call, seed=0):
    """the raw projection (offsets ~ N(0, 1) pixels, logits ~ N(0, 1)) and reference points of the fused entry point"""
    g = torch.Generator().manual_seed(seed)
    qproj = torch.randn(call.N, call.Lq, call.M * call.L * call.P * 3, generator=g)
    if call.encoder:
        ref = W.encoder_reference_points(call)[None, :, None, :].expand(call.N, call.Lq, call.L, 2)
    else:
        ref = (torch.rand(call.N, call.Lq, 1, 2, generator=g) * 0.8 + 0.1).expand(call.N, call.Lq, call.L, 2)
    return qproj.cuda(), ref.contiguous().cuda()


_lib.load()
for name, mk in (("Dd", W.call_Dd), ("E", W.call_E)):
    call = mk(2)
    t = W.make_inputs(call, "init", seed=0, device="cuda")
    qproj, ref = prep_inputs(call)
    for kind in ("fwd", "bwd", "fwd_prep"):
        if kind == "fwd":
            fn = lambda: MSDA.ms_deform_attn_forward(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], 64)
        elif kind == "bwd":
            fn = lambda: MSDA.ms_deform_attn_backward(t["value"], t["shapes"], t["lsi"], t["loc"], t["aw"], t["grad_out"], 64)
        else:
            _lib.set_option("fwd_prep_fused", 2 if call.encoder else 1)
            fn = lambda: MSDeformAttnFusedFunction.apply(t["value"], t["shapes"], t["lsi"], qproj, ref, call.M, call.L, call.P, 64)
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        n = 200
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        t_issue = (time.perf_counter() - t0) / n
        torch.cuda.synchronize()
        t_total = (time.perf_counter() - t0) / n
        print(f"{name} {kind}: host issue {t_issue * 1e6:7.2f} us per call, wall incl. GPU {t_total * 1e6:7.2f} us per call")
