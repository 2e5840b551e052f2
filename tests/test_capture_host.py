"""CPU: the host side of richsem_amd/capture.py -- the collector guard, the pinned AccumulateGrad nodes, and the rule that the capture
protocol is written down in that file and nowhere else (the stream and graph helpers themselves: tests/test_gpu_runtime.py)."""
import gc
import os

import pytest
import torch

from richsem_amd import capture as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("was_on", [True, False])
@pytest.mark.parametrize("raises", [False, True])
def test_quiet_gc_leaves_the_collector_as_it_found_it(was_on, raises):
    before = gc.isenabled()
    try:
        (gc.enable if was_on else gc.disable)()
        if raises:
            with pytest.raises(KeyError):
                with C.quiet_gc():
                    assert not gc.isenabled()
                    raise KeyError("body")
        else:
            with C.quiet_gc():
                assert not gc.isenabled()
        assert gc.isenabled() == was_on
    finally:
        (gc.enable if before else gc.disable)()


def test_pinned_accumulators_are_the_nodes_a_later_backward_uses():
    torch.manual_seed(0)
    mod = torch.nn.Sequential(torch.nn.Linear(8, 8), torch.nn.Linear(8, 8))
    mod[1].bias.requires_grad_(False)
    pinned = C.pin_grad_accumulators(mod.parameters())
    trained = [p for p in mod.parameters() if p.requires_grad]
    assert len(pinned) == len(trained) == 3
    assert all(type(n).__name__ == "AccumulateGrad" for n in pinned)
    assert [n.variable is p for n, p in zip(pinned, trained)] == [True] * 3
    out = mod(torch.randn(4, 8))

    def accumulators(fn, seen):
        if fn is not None and fn not in seen:
            seen.add(fn)
            if type(fn).__name__ == "AccumulateGrad":
                yield fn
            for nxt, _ in fn.next_functions:
                yield from accumulators(nxt, seen)
    used = list(accumulators(out.grad_fn, set()))
    assert len(used) == 3 and all(any(u is n for n in pinned) for u in used)      # the same objects, not new nodes
    out.sum().backward()
    assert all(p.grad is not None for p in trained) and mod[1].bias.grad is None


def test_bench_step_still_offers_the_name():
    import bench_step
    assert bench_step.pin_grad_accumulators is C.pin_grad_accumulators


# The pattern: each of these four strings, literally, anywhere in a .py file of the tree -- code, string or comment.  The three calls carry
# their opening parenthesis, so prose that names ``torch.cuda.make_graphed_callables`` or a graph bare does not match; the other two are
# bare names and nobody else has a reason to spell them.  Who may, and why:
PROTOCOL = ("default_capture_stream", "set_warn_on_accumulate_grad_stream_mismatch", "torch.cuda.make_graphed_callables(", "torch.cuda.graph(")
ALLOWED = {
    "richsem_amd/capture.py": PROTOCOL,                            # the definition
    "tools/capture_crash_probe.py": PROTOCOL,                      # shows the crash the protocol avoids: left as it was
    "tests/test_capture_host.py": PROTOCOL,                        # this list
    "bench.py": ("torch.cuda.graph(",),                            # the benchmark is not edited; its one capture is under quiet_gc()
    "tests/test_gpu_runtime.py": ("default_capture_stream",),      # READS it to check capture_stream(); never assigns (checked below)
}
SOURCE_DIRS = ("richsem_amd", "tests", "tools", "oracle")      # where the tree keeps Python, beside the files at its root
SKIP_DIRS = {"__pycache__", "_ref", "build", "lib"}            # build products inside them


def _python_files():
    yield from (f for f in os.listdir(ROOT) if f.endswith(".py"))
    for top in SOURCE_DIRS:
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if not x.startswith(".") and x not in SKIP_DIRS]
            for f in files:
                if f.endswith(".py"):
                    yield os.path.relpath(os.path.join(d, f), ROOT).replace(os.sep, "/")


def test_the_protocol_is_written_in_capture_py_and_nowhere_else():
    files = sorted(_python_files())
    assert "bench_step.py" in files and "tests/test_gpu_step.py" in files and "tools/accgrad_probe.py" in files, files[:20]
    found = []
    for rel in files:
        text = open(os.path.join(ROOT, rel), encoding="utf-8").read()
        found += [(rel, s) for s in PROTOCOL if s in text and s not in ALLOWED.get(rel, ())]
    assert not found, found
    runtime = open(os.path.join(ROOT, "tests/test_gpu_runtime.py"), encoding="utf-8").read()
    assert "default_capture_stream =" not in runtime and "default_capture_stream=" not in runtime
