"""Capturing this library's work into a HIP graph: the one protocol -- stream, pinned accumulators, collector guard.

`torch.cuda.graph.__enter__` of this PyTorch (2.10: torch/cuda/graphs.py) only collects garbage before a capture when
`torch.compiler.config.force_cudagraph_gc` is set.  A collection that starts INSIDE the capture -- any Python allocation can
trigger one -- then destroys whatever unreachable cycles earlier work of the process left behind, and if one of them holds a
`torch.cuda.CUDAGraph` (a previous `make_graphed_callables`, with its autograd.Function classes and closures, is exactly such a
cycle) its destructor calls hipGraphExecDestroy on a capturing thread: the HIP error is thrown from a destructor and the process
aborts ("Fatal Python error: Aborted ... Garbage-collecting", seen in 2 of 4 runs of tests/test_gpu_step.py on one box).

The whole of it, for a forward + backward (a plain forward needs only ``capture_stream`` and ``capture``):

    with capture_stream() as side:
        pinned = pin_grad_accumulators(module.parameters())      # before anything touches a parameter; keep the list
        module(x).sum().backward()                               # eager once: this stream's workspaces, the caches
        torch.cuda.synchronize()
        graphed = graphed_callables(module, (x,))                # or: graph, out = capture(lambda: module(x), side)
"""
import contextlib
import gc

import torch


@contextlib.contextmanager
def quiet_gc():
    """collect now, then keep the cyclic collector off for the body (a capture); reference counting still frees what the body drops"""
    was_on = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


def pin_grad_accumulators(params):
    """Create every parameter's AccumulateGrad node NOW -- on the current stream -- and return the nodes; the caller keeps them alive.
    The autograd engine runs an AccumulateGrad node on the stream that was current when the node was CREATED, and a node lives as long as
    some graph (or this list) references it.  Round 4's harness let the first forward that happened to touch a parameter decide -- for
    torch.cuda.make_graphed_callables that is its private warm-up stream -- and a later backward on the capture stream then synchronised
    with that foreign stream on every step ("AccumulateGrad node's stream does not match ..."), the precondition of the
    hipStreamEndCapture crash of profiles/r04_capture_probe.txt.  Pinned here, every later graph reuses these nodes."""
    return [p.view_as(p).grad_fn.next_functions[0][0] for p in params if p.requires_grad]


@contextlib.contextmanager
def capture_stream():
    """ONE side stream for the eager warm-up, the captures and the replays: created here (it waits for the caller's stream), current for
    the body, and torch's class-wide capture stream -- the one ``make_graphed_callables`` captures on -- for the body too; on exit, also
    by an exception, the capture stream is what it was and the caller's stream waits for the side stream.  Yields the stream.
    Why one stream: an autograd graph pins every parameter's AccumulateGrad node to the stream it was built on.  Round 3 built the eager
    steps on the default stream and captured on another one with the last step's `loss` still referenced: the engine then synchronises
    the capture stream with the foreign stream inside the capture ("AccumulateGrad node's stream does not match ..."; wrong results at
    best), and this ROCm build segfaults in hipStreamEndCapture instead of failing the capture (tools/capture_crash_probe.py,
    profiles/r04_capture_probe.txt: only the variants that keep `loss` alive crash, and none does when the eager phase already ran on
    the capture stream).  The library's workspaces are per (device, stream) as well and are not allocated during capture: a capture on a
    cold stream records the fallback kernels (round 3's 31.0 ms against 27.1 ms on the warmed stream)."""
    caller = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(caller)
    saved = torch.cuda.graph.default_capture_stream
    torch.cuda.graph.default_capture_stream = side
    try:
        with torch.cuda.stream(side):
            yield side
    finally:
        torch.cuda.graph.default_capture_stream = saved
        caller.wait_stream(side)


def capture(fn, stream=None):
    """``fn()`` captured into a new graph on ``stream`` (None: torch's capture stream) with the collector kept out: -> (graph, fn's
    result).  The caller has run ``fn`` eagerly on that stream and synchronised."""
    graph = torch.cuda.CUDAGraph()
    with quiet_gc(), torch.cuda.graph(graph, stream=stream):
        out = fn()
    return graph, out


def graphed_callables(callables, sample_args, num_warmup_iters=3, **kw):
    """``torch.cuda.make_graphed_callables`` with the collector kept out.  The caller is inside ``capture_stream()`` with its
    accumulators pinned (``pin_grad_accumulators``) and one eager forward + backward done.
    make_graphed_callables warms its callables up on a PRIVATE stream of its own making (torch/cuda/graphs.py) before it captures them
    on the capture stream: during those iterations the gradients arrive at the pinned nodes from that other stream, by construction.
    The engine's warning about it is switched off for this one call only; everything after it runs with the warning on, and
    tests/test_gpu_step.py fails on it."""
    torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
    try:
        with quiet_gc():
            return torch.cuda.make_graphed_callables(callables, sample_args, num_warmup_iters=num_warmup_iters, **kw)
    finally:
        torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(True)
