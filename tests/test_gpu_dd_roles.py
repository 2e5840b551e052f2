"""GPU (-m gpu): the decoder-shaped backward as ONE launch whose workgroups are either level-sum entries or blocks of split items
(msda_roles.h: bwd_dd_roles_kernel), option bwd_dd_roles = 1.

Two yardsticks, on seeded inputs:
  * the C oracle (oracle/msda_oracle.c) with the bound tests/test_gpu_parity.py applies to the fp32 backward: 2e-4 of the tensor's
    largest magnitude for each of the three gradients;
  * the two-launch path (bwd_dd_roles = 0) on the same inputs: grad_sampling_loc / grad_attn_weight bit for bit (same arithmetic, no
    atomics), grad_value to one fp32 unit in the last place per element (the f64 windows sum to fp32 rounding whatever the band cut;
    the two paths cut the levels into different bands).
Every call must log [("bwd", 1)], and the library's count of calls that took the one-launch path (bwd_dd_roles_calls) must step by
one -- or, for the fallbacks, not at all.  M = 2, D = 32, N <= 2."""
import numpy as np
import pytest
import torch

from oracle import msda_oracle as O
from richsem_amd import _lib, capture, workload as W
from richsem_amd import MultiScaleDeformableAttention as MSDA

pytestmark = pytest.mark.gpu

TG = 2e-4            # tests/test_gpu_parity.py: tols(np.float32)[1]
WINDOW_PX = 75 * 1024 // 32      # pixels of one window of the one-launch path: 75 KB of 4 f64 channels = 2400
M, D = 2, 32


@pytest.fixture(autouse=True)
def _restore():
    yield
    _lib.set_option("bwd_dd_roles", 1)
    _lib.profile_enable(0)


def rel_err(a, b):
    a = a.detach().float().cpu().numpy().astype(np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def make(shapes, Lq, P=4, N=1, seed=0, spread=1.0):
    """seeded inputs; locations U(0, 1) * spread - (spread - 1) / 2 (spread 1.5: U(-0.25, 1.25), samples outside the map)"""
    g = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)
    call = W.Call("roles", N, M, D, P, list(shapes), Lq, False)
    sh, lsi = W.level_tensors(call)
    return dict(value=torch.randn(N, S, M, D, generator=g), shapes=sh, lsi=lsi,
                loc=(torch.rand(N, Lq, M, L, P, 2, generator=g) * spread - (spread - 1.0) / 2).contiguous(),
                aw=torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P).contiguous(),
                grad_out=torch.randn(N, Lq, M * D, generator=g))


def on_gpu(t):
    return {k: v.cuda() for k, v in t.items()}


def backward(c, roles, one_launch):
    """the backward of the device tensors c with bwd_dd_roles = roles -> (grad_value, grad_loc, grad_aw); fails unless the record is
    ("bwd", 1) and the one-launch path ran exactly when `one_launch` says so"""
    _lib.set_option("bwd_dd_roles", roles)
    before = _lib.get_option("bwd_dd_roles_calls")
    _lib.profile_enable(8)
    res = MSDA.ms_deform_attn_backward(c["value"], c["shapes"], c["lsi"], c["loc"], c["aw"], c["grad_out"], 64)
    torch.cuda.synchronize()
    ran = [(r["kind"], r["variant"]) for r in _lib.profile_collect()]
    _lib.profile_enable(0)
    assert ran == [("bwd", 1)], ran
    assert _lib.get_option("bwd_dd_roles_calls") - before == (1 if one_launch else 0)
    return res


def oracle(t):
    return O.backward(t["value"].numpy(), t["shapes"].numpy(), t["lsi"].numpy(), t["loc"].numpy(), t["aw"].numpy(), t["grad_out"].numpy())


def ulps(a, b):
    """largest distance of two fp32 tensors in units in the last place (ordered-integer distance; -0 and +0 are the same number)"""
    def key(x):
        i = x.detach().cpu().numpy().view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.abs(key(a) - key(b)).max())


def check(t, tag=None, one_launch=True):
    """both yardsticks; -> (the one-launch gradients, the oracle's)"""
    c = on_gpu(t)
    gv, gl, ga = backward(c, 1, one_launch)
    gv2, gl2, ga2 = backward(c, 0, False)
    ogv, ogl, oga = oracle(t)
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err grad_value / grad_loc / grad_aw:", errs, "ulps grad_value:", ulps(gv, gv2), tag)
    assert max(errs) < TG, (errs, tag)
    assert torch.equal(gl, gl2) and torch.equal(ga, ga2), tag
    assert ulps(gv, gv2) <= 1, tag
    return (gv, gl, ga), (ogv, ogl, oga)


# ---- role-count edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lq,shapes", [
    (1, [(48, 40), (3, 5)]),        # far more level-sum than split workgroups
    (3000, [(2, 2), (1, 1)]),       # the reverse
    (7, [(6, 5), (3, 2)]),          # items do not fill a workgroup: the tail lanes are clamped
    (33, [(6, 5), (3, 2)]),
])
def test_role_count_edges(Lq, shapes):
    check(make(shapes, Lq, N=2, seed=Lq), tag=(Lq, shapes))


# ---- window edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [
    [(WINDOW_PX // 50, 50)],                   # fits the window exactly
    [(WINDOW_PX // 50 + 1, 50)],               # one row over: must split into bands
    [(1, 1)],
    [(20, 34), (10, 17), (5, 9), (3, 5)],      # four levels, L * P = 16: the shape of the decoder's calls
])
def test_window_edges(shapes):
    assert WINDOW_PX % 50 == 0
    check(make(shapes, Lq=300, N=2, seed=len(shapes) * 1000 + shapes[0][0]), tag=shapes)


# ---- every element written; dropped samples ----------------------------------------------------------------------------------------
SHRUNK = [(20, 34), (10, 17), (5, 9), (3, 5)]


@pytest.fixture(scope="module")
def outside():
    """a third of the samples fall outside the map"""
    t = make(SHRUNK, Lq=273, N=2, seed=44, spread=1.5)
    return t, oracle(t)


def test_poisoned_outputs(outside):
    """C ABI, NaN-filled grad_value / grad_loc / grad_aw: there is no zero-fill on this path, every element must be written"""
    t, (ogv, ogl, oga) = outside
    lib = _lib.load()
    c = on_gpu(t)
    N, Lq, L, P, S = c["loc"].shape[0], c["loc"].shape[1], len(SHRUNK), 4, c["value"].shape[1]
    sh, ls = t["shapes"].numpy(), t["lsi"].numpy()
    gv, gl, ga = (torch.full_like(c[k], float("nan")) for k in ("value", "loc", "aw"))
    _lib.set_option("bwd_dd_roles", 1)
    before = _lib.get_option("bwd_dd_roles_calls")
    _lib.profile_enable(8)
    _lib.check(lib.msda_backward_f32(c["value"].data_ptr(), c["shapes"].data_ptr(), c["lsi"].data_ptr(), c["loc"].data_ptr(),
                                     c["aw"].data_ptr(), c["grad_out"].data_ptr(), N, S, M, D, L, Lq, P, 64, gv.data_ptr(),
                                     gl.data_ptr(), ga.data_ptr(), sh.ctypes.data, ls.ctypes.data,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ran = [(r["kind"], r["variant"]) for r in _lib.profile_collect()]
    _lib.profile_enable(0)
    assert ran == [("bwd", 1)], ran
    assert _lib.get_option("bwd_dd_roles_calls") - before == 1
    for a in (gv, gl, ga):
        assert torch.isfinite(a).all()
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err:", errs)
    assert max(errs) < TG, errs


def test_samples_outside_the_map(outside):
    """the reference drops them: their gradients are zero, and the zeros are written"""
    t, (ogv, ogl, oga) = outside
    c = on_gpu(t)
    gv, gl, ga = backward(c, 1, True)
    errs = (rel_err(gv, ogv), rel_err(gl, ogl), rel_err(ga, oga))
    print("rel_err:", errs)
    assert max(errs) < TG, errs
    dropped = (ogl == 0).all(-1) & (oga == 0)
    assert dropped.mean() > 0.1
    assert (gl.cpu().numpy()[dropped] == 0).all() and (ga.cpu().numpy()[dropped] == 0).all()


# ---- fallbacks still chosen ------------------------------------------------------------------------------------------------------
def test_p3_keeps_two_launches():
    check(make(SHRUNK, Lq=100, P=3, N=2, seed=33), one_launch=False)


def test_unaligned_loc_keeps_two_launches():
    """sampling_loc 8 bytes past a 16-byte boundary: two launches, and the same results as the aligned call's one launch"""
    t = make(SHRUNK, Lq=100, N=2, seed=34)
    c = on_gpu(t)
    res = backward(c, 1, True)
    buf = torch.empty(c["loc"].numel() + 4, device="cuda")
    shifted = buf[(2 if buf.data_ptr() % 16 == 0 else 4):][:c["loc"].numel()].view_as(c["loc"])
    shifted.copy_(c["loc"])
    assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
    res2 = backward(dict(c, loc=shifted), 1, False)
    assert torch.equal(res[1], res2[1]) and torch.equal(res[2], res2[2])
    assert ulps(res[0], res2[0]) <= 1


# ---- capture ---------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay():
    """the path allocates nothing: one call captured into a graph after a warm-up, replayed twice, equals the eager result
    (``_capture_job`` below).  In a process of its own, as tests/test_gpu_criterion_capacity.py::test_one_graph_serves_many_batches and
    for its reason: with a capture of a new test made in the suite's process, the whole suite segfaulted in the HIP runtime's replay
    of a later, unrelated graph (tests/test_gpu_fed_loss.py, the graphed federated step) -- it did so with this
    test's capture too --, so this test leaves the suite's process without a stream, a graph or a graph memory pool of its making."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_dd_roles as t; t._capture_job(); print('capture: ok')"
            % (os.path.dirname(here), here))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "capture: ok" in r.stdout, (r.returncode, r.stderr[-2000:])


def _capture_job():
    """the body of test_capture_and_replay (raises where it does not hold)"""
    t = make(SHRUNK, Lq=273, N=2, seed=55)
    c = on_gpu(t)
    _lib.set_option("bwd_dd_roles", 1)
    with capture.capture_stream():
        def fn():
            return MSDA.ms_deform_attn_backward(c["value"], c["shapes"], c["lsi"], c["loc"], c["aw"], c["grad_out"], 64)
        before = _lib.get_option("bwd_dd_roles_calls")
        eager = [x.clone() for x in fn()]
        torch.cuda.synchronize()
        graph, out = capture.capture(fn)
        assert _lib.get_option("bwd_dd_roles_calls") - before == 2
        for _ in range(2):
            for x in out:
                x.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(out, eager):
                assert torch.equal(a, b)
