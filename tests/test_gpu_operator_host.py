"""GPU (-m gpu): two things the host layer of msda_api.hip does that no other test pins, at the smallest shape that still takes the window
forward and the routed backward (ENC of tests/test_gpu_dispatch.py).

1. msda_forward_prep_f32 under fwd_prep_fused = 2 once the locality monitor has sent the call to the direct kernel: the choice made in
   msda_forward_prep_* is carried into the forward as an argument (it used to travel through a thread-local override).
2. The library's per-stream buffers (fp32 scratch of the bf16 backward, workspace of the routed backward) outgrown AFTER a graph captured
   their addresses: the old buffers are retired, not freed, so the replay still computes the right numbers.  test_gpu_runtime.py replays a
   routed backward around a SMALLER call only, and test_gpu_dispatch.py::test_bf16_scratch_and_stream_capture never outgrows the scratch."""
import numpy as np
import pytest
import torch

from richsem_amd import _lib, workload as W
from richsem_amd.capture import capture

import test_gpu_dispatch as DSP
from test_gpu_parity import _profiled_variants

pytestmark = pytest.mark.gpu

ENC = DSP.SHAPES["ENC"]
_OPTIONS = ("fwd_variant", "bwd_variant", "fwd_prep_fused", "locality_monitor")


@pytest.fixture(autouse=True)
def _options():
    saved = {k: _lib.get_option(k) for k in _OPTIONS}
    yield
    for k, v in saved.items():
        _lib.set_option(k, v)


def prep_inputs(sigma=None, seed=5):
    """value, the raw projection (logits ~ N(0, 1), offsets) and the encoder's reference points (pixel centres).  The offsets: those that
    put every sampling point at a place of its own drawn from U[0, 1)^2 -- the "uniform" pattern of the suite, all points inside the image,
    none near its query but by chance --, or with ``sigma`` N(0, sigma) as a fraction of the sampled level's width / height."""
    c = ENC
    g = torch.Generator().manual_seed(seed)
    value = torch.randn(c.N, c.S, c.M, c.D, generator=g)
    n_off, n_log = c.M * c.L * c.P * 2, c.M * c.L * c.P
    wh = torch.tensor([[w, h] for h, w in c.shapes], dtype=torch.float32)[None, None, None, :, None, :]
    ref = W.encoder_reference_points(c)[None, :, None, :].expand(c.N, c.Lq, c.L, 2).contiguous()
    if sigma is None:
        off = (torch.rand(c.N, c.Lq, c.M, c.L, c.P, 2, generator=g) - ref[:, :, None, :, None, :]) * wh
    else:
        off = sigma * torch.randn(c.N, c.Lq, c.M, c.L, c.P, 2, generator=g) * wh
    qproj = torch.cat((off.reshape(c.N, c.Lq, n_off), torch.randn(c.N, c.Lq, n_log, generator=g)), -1).contiguous()
    shapes, lsi = W.level_tensors(c)
    t = dict(value=value, qproj=qproj, ref=ref, shapes=shapes, lsi=lsi)
    t = {k: v.cuda() for k, v in t.items()}
    t["host"] = (np.ascontiguousarray(shapes.numpy()), np.ascontiguousarray(lsi.numpy()))
    return t


def _buffers():
    c = ENC
    return dict(out=torch.full((c.N, c.Lq, c.M * c.D), float("nan"), device="cuda"),
                loc=torch.full((c.N, c.Lq, c.M, c.L, c.P, 2), float("nan"), device="cuda"),
                aw=torch.full((c.N, c.Lq, c.M, c.L, c.P), float("nan"), device="cuda"))


def forward_prep(t, b):
    """msda_forward_prep_f32 into the caller-kept buffers ``b`` (the monitor keys on the sampling_loc address)"""
    c = ENC
    n_off, stride = c.M * c.L * c.P * 2, c.M * c.L * c.P * 3
    sh, ls = t["host"]
    _lib.check(_lib.load().msda_forward_prep_f32(
        t["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), t["qproj"].data_ptr(), stride, t["qproj"].data_ptr() + 4 * n_off, stride,
        t["ref"].data_ptr(), 2, c.N, c.S, c.M, c.D, c.L, c.Lq, c.P, 64, b["out"].data_ptr(), b["loc"].data_ptr(), b["aw"].data_ptr(),
        sh.ctypes.data, ls.ctypes.data, _lib.raw_stream()))


def two_call_form(t):
    """msda_prep_forward_f32, then msda_forward_f32 with fwd_variant = 1, on the same inputs: (out, loc, aw)"""
    c = ENC
    b = _buffers()
    n_off, stride = c.M * c.L * c.P * 2, c.M * c.L * c.P * 3
    sh, ls = t["host"]
    lib = _lib.load()
    _lib.check(lib.msda_prep_forward_f32(t["qproj"].data_ptr(), stride, t["qproj"].data_ptr() + 4 * n_off, stride, t["ref"].data_ptr(), 2,
                                         sh.ctypes.data, c.N, c.Lq, c.M, c.L, c.P, b["loc"].data_ptr(), b["aw"].data_ptr(), _lib.raw_stream()))
    saved = _lib.get_option("fwd_variant")
    _lib.set_option("fwd_variant", 1)
    ran = _profiled_variants(lambda: _lib.check(lib.msda_forward_f32(
        t["value"].data_ptr(), t["shapes"].data_ptr(), t["lsi"].data_ptr(), b["loc"].data_ptr(), b["aw"].data_ptr(), c.N, c.S, c.M, c.D, c.L,
        c.Lq, c.P, 64, b["out"].data_ptr(), sh.ctypes.data, ls.ctypes.data, _lib.raw_stream())))
    _lib.set_option("fwd_variant", saved)
    assert ran == [("fwd", 1)], ran
    return b


def monitor_share(t, b):
    """the share the first probe of a fresh monitor brings back for these inputs (the first call is a probe; the next call folds it in)"""
    _lib.set_option("locality_monitor", 1)      # (setting it forgets what was learnt)
    first = _profiled_variants(lambda: forward_prep(t, b))
    torch.cuda.synchronize()
    forward_prep(t, b)
    torch.cuda.synchronize()
    return first, _lib.get_option("locality_share_ppm")


def test_forward_prep_carries_the_monitors_choice_into_the_forward():
    t = prep_inputs()
    want = two_call_form(t)
    b = _buffers()
    _lib.set_option("fwd_prep_fused", 2)
    _lib.set_option("fwd_variant", 0)
    first, share_ppm = monitor_share(t, b)
    assert first == [("fwd", 6)], first      # a probe is a (fused) window-kernel call
    print("locality_share_ppm with uniform sampling points: %d" % share_ppm)
    assert share_ppm > 80000, share_ppm
    for _ in range(10):      # past the warm-up probes
        forward_prep(t, b)
        torch.cuda.synchronize()
    for k in b:
        b[k].fill_(float("nan"))
    ran = _profiled_variants(lambda: forward_prep(t, b))
    assert ran == [("fwd", 1)], ran      # location / softmax kernel (no record), then the direct kernel and nothing else
    assert _lib.get_option("fwd_variant") == 0
    for k in ("loc", "aw", "out"):
        assert torch.equal(b[k], want[k]), k
    # fwd_variant 3 forced: where the window kernel applies this path ends in the 8-lane direct kernel, not the split kernel
    _lib.set_option("fwd_variant", 3)
    for k in b:
        b[k].fill_(float("nan"))
    ran = _profiled_variants(lambda: forward_prep(t, b))
    assert ran == [("fwd", 1)], ran
    assert _lib.get_option("fwd_variant") == 3
    for k in ("loc", "aw", "out"):
        assert torch.equal(b[k], want[k]), k


def _backward_outputs(call, sfx):
    nan = lambda shape, dtype: torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    c = call
    return dict(grad_value=nan((c.N, c.S, c.M, c.D), DSP.TORCH[sfx]), grad_loc=nan((c.N, c.Lq, c.M, c.L, c.P, 2), DSP.WORK[sfx]),
                grad_aw=nan((c.N, c.Lq, c.M, c.L, c.P), DSP.WORK[sfx]))


def test_buffers_outgrown_after_a_capture_are_retired_not_freed():
    """On a stream of its own (high priority, as test_bf16_scratch_and_stream_capture: a pool no other test draws from, so the stream's
    workspace starts empty): a bf16 backward and an f32 routed backward at ENC eagerly, one of each captured, both at four times the
    pixels eagerly -- every buffer of the stream outgrown and replaced --, then the replay: grad_loc / grad_aw bit-equal to the eager run,
    grad_value of f32 within the capture tests' 2e-4 of it, of bf16 within test_gpu_bf16.check of the oracle (the criterion of the bf16
    capture test)."""
    big_call = W.shrunk(W.call_E(2), 2)
    _lib.set_option("bwd_variant", 0)      # Lq == S: the routed kernels; bf16 with the fp32 scratch
    side = torch.cuda.Stream(priority=-1)
    eager, replayed = {}, {}

    def run(name, sfx, tensors, call=None):
        rcs, out = DSP.call_abi(name, sfx, {}, fwd=False, stream=side.cuda_stream, tensors=tensors, call=call)
        assert rcs == [0], _lib.last_error()
        return out

    with torch.cuda.stream(side):
        for sfx in ("bf16", "f32"):
            ran = _profiled_variants(lambda: eager.update({sfx: run("ENC", sfx, _backward_outputs(ENC, sfx))}))
            assert ran == [("bwd", 4)], (sfx, ran)
    side.synchronize()

    replayed.update({sfx: _backward_outputs(ENC, sfx) for sfx in ("bf16", "f32")})
    torch.cuda.synchronize()

    def body():
        for sfx in ("bf16", "f32"):
            run("ENC", sfx, replayed[sfx])
    graph, _ = capture(body, side)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for sfx in ("bf16", "f32"):
            big = run("big", sfx, _backward_outputs(big_call, sfx), call=big_call)
    side.synchronize()
    DSP.assert_matches(big, "big", "f32", note="the larger call", call=big_call)
    for sfx in ("bf16", "f32"):
        for k in ("grad_value", "grad_loc", "grad_aw"):
            replayed[sfx][k].fill_(float("nan"))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for sfx in ("bf16", "f32"):
        for k in ("grad_loc", "grad_aw"):
            assert torch.equal(replayed[sfx][k], eager[sfx][k]), (sfx, k)
    gv, ref = replayed["f32"]["grad_value"], eager["f32"]["grad_value"]
    assert bool(torch.isfinite(gv).all()) and float((gv - ref).abs().max() / (ref.abs().max() + 1e-30)) < 2e-4
    DSP.assert_matches(replayed["bf16"], "ENC", "bf16", note="bf16 replay")
    DSP.assert_matches(replayed["f32"], "ENC", "f32", note="f32 replay")
    del graph
