"""GPU (-m gpu): the class head (richsem_amd/csrc/cls_head_mfma.hip, richsem_amd/class_head.py) against the float64 restatement, the
ELEMENT-WISE bounds and the EXACT PROBE of tests/class_head_ref.py (derivations in its docstring; tests/test_class_head_ref.py shows that a
correct implementation meets them and three wrong ones do not).  The kernels go through the C ABI with ctypes, so that G, A, the saved
values and the result buffers are the test's own; the fixture and the cache go through ClassHead.  Every result
buffer is NaN-poisoned and longer than needed: the tail holds a sentinel that must be untouched after the call.  An excess over a derived
bound is a bug in the kernel or in the derivation, not a reason to widen it.  RICHSEM_REPORT=1 prints the worst |err| / bound per case.

No test here captures a graph: a capture test was written (forward + backward replayed to the eager bits) and is left out, because whole-
suite runs with it in this file ended in a segmentation fault inside a graph replay of
tests/test_gpu_fed_loss.py::test_graphed_fed_step_draws_fresh_masks_and_matches_the_eager_step, a test that runs none of this code; the
fault is unexplained ("Class head")."""
import ctypes
import os

import numpy as np
import pytest
import torch

import class_head_ref as H
from test_class_head_ref import collapsed, load_fixture

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REPORT = bool(os.environ.get("RICHSEM_REPORT"))
SENTINEL = -12345.0
TAIL = 64


def _say(tag, **kv):
    if REPORT:
        print(f"[measured] {tag} " + " ".join(f"{k}={v:.3g}" for k, v in kv.items()), flush=True)


def _poisoned(n, dtype=torch.float32):
    buf = torch.full((n + TAIL,), float("nan") if dtype.is_floating_point else 0x7FFF, dtype=dtype, device="cuda")
    buf[n:] = SENTINEL
    return buf


def _result(buf, shape):
    n = int(np.prod(shape))
    torch.cuda.synchronize()
    assert bool((buf[n:] == torch.tensor(SENTINEL).to(buf.dtype)).all()), "stored past the end of the result"
    return buf[:n].view(*shape)


class _Head:
    """[A; G] and G^T packed once by msda_cls_head_pack; the three kernels on buffers of the test's own (device tensors in and out)"""

    def __init__(self, G, A):
        from richsem_amd import _lib
        self._lib, self.lib = _lib, _lib.load()
        self.classes = G.shape[0]
        n = ctypes.c_int64(0)
        _lib.check(self.lib.msda_cls_head_packed_elems(self.classes, ctypes.byref(n)))
        pk = _poisoned(n.value, torch.int16)
        self.G, self.A = G.float().contiguous().cuda(), A.float().contiguous().cuda()
        _lib.check(self.lib.msda_cls_head_pack(self.G.data_ptr(), self.classes, self.A.data_ptr(), 256, pk.data_ptr(), _lib.raw_stream()))
        self.packed = _result(pk, (n.value,))

    def forward(self, x, scale, parts):
        R = x.shape[0]
        lg, n2 = _poisoned(R * self.classes), _poisoned(R)
        self._lib.check(self.lib.msda_cls_head_forward(x.data_ptr(), int(x.dtype == BF), self.packed.data_ptr(), R, 256, self.classes, scale,
                                                       parts, lg.data_ptr(), n2.data_ptr(), self._lib.raw_stream()))
        return _result(lg, (R, self.classes)), _result(n2, (R,))

    def rows(self, g, logits, n2, x, scale, parts):
        R = x.shape[0]
        dx, beta = _poisoned(R * 256, x.dtype), _poisoned(R)
        self._lib.check(self.lib.msda_cls_head_backward_rows(g.data_ptr(), logits.data_ptr(), n2.data_ptr(), x.data_ptr(), int(x.dtype == BF),
                                                             self.packed.data_ptr(), R, 256, self.classes, scale, parts, dx.data_ptr(),
                                                             beta.data_ptr(), self._lib.raw_stream()))
        return _result(dx, (R, 256)), _result(beta, (R,))

    def weights(self, g, n2, beta, x, scale, parts):
        R = x.shape[0]
        nb = ctypes.c_int64(0)
        self._lib.check(self.lib.msda_cls_head_workspace_bytes(R, self.classes, ctypes.byref(nb)))
        assert nb.value == H.n_splits(R) * (self.classes + 256) * 256 * 4
        ws, out = _poisoned(nb.value // 4), _poisoned((self.classes + 256) * 256)
        self._lib.check(self.lib.msda_cls_head_backward_weights(g.data_ptr(), n2.data_ptr(), beta.data_ptr(), x.data_ptr(), int(x.dtype == BF), R,
                                                                256, self.classes, scale, parts, ws.data_ptr(), out.data_ptr(),
                                                                self._lib.raw_stream()))
        _result(ws, (nb.value // 4,))
        return _result(out, (self.classes + 256, 256))

    def all(self, x, g, scale, parts, saved=None):
        """forward, then both backward kernels on the forward's own results (or on `saved`) -> dict of CPU tensors"""
        logits, n2 = self.forward(x, scale, parts)
        sl, sn = (logits, n2) if saved is None else (saved[0].cuda(), saved[1].cuda())
        dx, beta = self.rows(g, sl, sn, x, scale, parts)
        dGA = self.weights(g, sn, beta, x, scale, parts)
        return {"logits": logits.cpu(), "n2": n2.cpu(), "dx": dx.cpu(), "beta": beta.cpu(), "dGA": dGA.cpu()}


def _check_case(rows, classes, x_dtype, parts):
    """one shape: the chain (the backward on the forward's results) and the backward alone on saved values of the test's own"""
    p = H.make_head(rows, classes, 0, x_dtype)
    head = _Head(p["G"], p["A"])
    x, g = p["x"].cuda(), p["g"].cuda()
    ref = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], x_dtype, parts)
    assert int(ref["excluded"].sum()) == 0
    got = head.all(x, g, p["scale"], parts)
    worst = {}
    for name in ("logits", "n2", "dx", "beta", "dGA"):
        r = H.ratio(got[name], ref[name], ref["B_" + name])
        print(f"[figures] rows {rows} classes {classes} x {x_dtype} parts {parts} {name}: {r:.3g}", flush=True)
        worst[name] = r
    saved = (ref["logits"].float(), ref["n2"].float())
    ref_s = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], x_dtype, parts, saved=saved)
    got_s = head.all(x, g, p["scale"], parts, saved=saved)
    for name in ("dx", "beta", "dGA"):
        r = H.ratio(got_s[name], ref_s[name], ref_s["B_" + name])
        print(f"[figures] rows {rows} classes {classes} x {x_dtype} parts {parts} {name} (saved): {r:.3g}", flush=True)
        worst[name + "_saved"] = r
    assert all(v <= 1.0 for v in worst.values()), (rows, classes, x_dtype, parts, worst)
    return worst, head, x, g, got, p


@pytest.mark.parametrize("x_dtype,parts", H.MODES, ids=str)
def test_forward_and_backward_within_the_bounds(x_dtype, parts):
    """every element of every output at every tile size +- 1 of the three kernels (class_head_ref.ROW_SWEEP / CLASS_SWEEP)"""
    top = {}
    for rows, classes in H.CASES:
        worst = _check_case(rows, classes, x_dtype, parts)[0]
        top = {k: max(v, top.get(k, 0.0)) for k, v in worst.items()}
    _say(f"class head x={x_dtype} parts={parts}", **top)


@pytest.mark.parametrize("x_dtype,parts", [("f32", 2), ("bf16", 1)], ids=str)
def test_rows_straddling_the_split_boundaries(x_dtype, parts):
    """one row below, at and one above one and two split lengths of the weights kernel: within the bounds, and the same bits from a second
    call whatever the split count"""
    for rows, classes in H.SPLIT_CASES:
        _, head, x, g, got, p = _check_case(rows, classes, x_dtype, parts)
        again = head.all(x, g, p["scale"], parts)
        for name in ("dx", "dGA"):
            assert torch.equal(got[name], again[name]), (rows, name)


@pytest.mark.parametrize("shape", H.PROBE_SHAPES, ids=str)
def test_exact_probes(shape):
    """bit equality of every output: one-hot g at the last class of the last (partial) tile in row 0 and a one-hot g in the last row"""
    T, classes = shape
    for x_dtype in ("f32", "bf16"):
        p = H.head_probe(T, classes, x_dtype)
        want = H.head_probe_expected(p, check_sums=False)      # (the sums' conditions are asserted by the CPU test)
        head = _Head(p["G"], p["A"])
        for parts in (2, 1):
            got = head.all(p["x"].cuda(), p["g"].cuda(), p["scale"], parts)
            for name in ("logits", "n2", "dx"):
                bad = got[name] != want[name]
                assert not bool(bad.any()), (shape, x_dtype, parts, name, int(bad.sum()), torch.nonzero(bad)[:4].tolist())
            assert torch.equal(got["dGA"][:classes], want["dGA"][:classes]), (shape, x_dtype, parts, "dG")
            if parts == 2 or not want["y_needs_lo"]:
                bad = got["dGA"][classes:] != want["dGA"][classes:]
                assert not bool(bad.any()), (shape, x_dtype, parts, "dA", int(bad.sum()), torch.nonzero(bad)[:4].tolist())


def _class_head(wp, text, ls, parts=2):
    from richsem_amd.class_head import ClassHead
    return ClassHead(parts).prepare(wp, text, ls)


def test_reference_fixture_through_the_class_head():
    """tests/golden/cls_head_reference.npz (the reference's forward_hs and autograd, float32 configuration: 1204 classes) through ClassHead
    with fp32 rows and parts = 2: logits, hs.grad and proj_weight.grad within the bounds, taken against the float64 restatement from
    (Wp, text) -- which test_class_head_ref.py ties to the fixture -- and the fixture's own float32 values within bound + their own error"""
    f = load_fixture("f32")
    G, A, te = collapsed(f)
    classes = G.shape[0]
    scale = float(np.exp(np.float64(f["logit_scale"])))
    ref = H.reference(G, A, f["x"], f["g_full"], scale, "f32", 2, oracle=True)
    assert int(ref["excluded"].sum()) == 0
    dwp, B_dwp = H.dwp_reference(ref, f["proj_weight"].double(), te, classes)
    wp = f["proj_weight"].cuda().requires_grad_(True)
    head = _class_head(wp, f["text_embed"].cuda(), f["logit_scale"])
    hs = f["hs"].cuda().requires_grad_(True)                        # (2, 1, rows, 256): the leading dimensions travel
    logits = head(hs)
    assert logits.shape == (*f["hs"].shape[:-1], classes) and logits.dtype == torch.float32
    logits.backward(f["g_full"].view(*logits.shape).cuda())
    got = {"logits": logits.detach().cpu().view(-1, classes), "dx": hs.grad.cpu().view(-1, 256), "dwp": wp.grad.cpu()}
    figures = {"logits": H.ratio(got["logits"], ref["logits"], ref["B_logits"]), "dx": H.ratio(got["dx"], ref["dx"], ref["B_dx"]),
               "dWp": H.ratio(got["dwp"], dwp, B_dwp)}
    print(f"[figures] fixture through ClassHead {figures}", flush=True)
    assert all(v <= 1.0 for v in figures.values()), figures
    # the fixture's float32 values themselves: the reference's own fp32 error is taken from its distance to the float64 restatement
    for name, mine, theirs, truth, bound in (("logits", got["logits"][:, f["cls_idx"]], f["logits_slice"], ref["logits"][:, f["cls_idx"]], ref["B_logits"][:, f["cls_idx"]]),
                                             ("dx", got["dx"], f["x_grad"], ref["dx"], ref["B_dx"]), ("dWp", got["dwp"], f["proj_weight_grad"], dwp, B_dwp)):
        own = (theirs.double() - truth).abs()
        assert bool(((mine.double() - theirs.double()).abs() <= bound + own).all()), name


def test_a_zero_row_is_nan_alone():
    """x = 0 in one row: NaN logits in that row only, finite dx in every other row, NaN [dG; dA] (as the reference's weight gradient)"""
    for x_dtype in ("f32", "bf16"):
        p = H.make_head(65, 33, 1, x_dtype)
        p["x"][17] = 0
        head = _Head(p["G"], p["A"])
        got = head.all(p["x"].cuda(), p["g"].cuda(), p["scale"], 2)
        other = torch.arange(65) != 17
        assert torch.isnan(got["logits"][17]).all() and float(got["n2"][17]) == 0.0
        assert torch.isfinite(got["logits"][other]).all() and torch.isfinite(got["dx"][other].float()).all()
        assert torch.isnan(got["dx"][17].float()).all()
        assert torch.isnan(got["dGA"]).any()
        ref = H.reference(p["G"], p["A"], p["x"], p["g"], p["scale"], x_dtype, 2)
        for name in ("logits", "dx"):
            assert H.ratio(got[name][other], ref[name][other], ref["B_" + name][other]) <= 1.0, name


def test_two_backward_calls_give_the_same_bits():
    p = H.make_head(2 * H.SPLIT_ROWS + 77, 97, 2, "bf16")
    head = _Head(p["G"], p["A"])
    a = head.all(p["x"].cuda(), p["g"].cuda(), p["scale"], 2)
    b = head.all(p["x"].cuda(), p["g"].cuda(), p["scale"], 2)
    for name in ("logits", "n2", "dx", "beta", "dGA"):
        assert torch.equal(a[name], b[name]), name
    dG, dA = a["dGA"][:97], a["dGA"][97:]
    assert torch.isfinite(dG).all() and torch.isfinite(dA).all()


def test_cpu_tensors_and_an_unprepared_head_are_refused():
    from richsem_amd.class_head import ClassHead
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ClassHead().prepare(torch.zeros(8, 256), torch.zeros(3, 8), torch.tensor(0.0))
    with pytest.raises(RuntimeError, match="prepare has not been called"):
        ClassHead()(torch.zeros(1, 256, device="cuda"))
    head = _class_head(torch.randn(8, 256, device="cuda"), torch.randn(3, 8, device="cuda"), torch.tensor(0.0))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        head(torch.zeros(1, 256))
    with pytest.raises(RuntimeError, match="float32 / bfloat16"):
        head(torch.zeros(1, 256, device="cuda", dtype=torch.float16))
    assert head(torch.zeros(0, 256, device="cuda")).shape == (0, 3)


def test_the_packed_operand_follows_an_in_place_update():
    """copy_ into the projection (what load_state_dict and an optimizer step do): the next call computes with the new weights"""
    gen = torch.Generator().manual_seed(5)
    wp0, wp1 = (torch.randn(64, 256, generator=gen) / 8 for _ in range(2))
    text, ls = torch.randn(33, 64, generator=gen), torch.tensor(float(np.log(1 / 0.07)))
    x = torch.randn(49, 256, generator=gen)
    wp = wp0.clone().cuda().requires_grad_(True)
    head = _class_head(wp, text.cuda(), ls)
    first = head(x.cuda()).detach().cpu()
    with torch.no_grad():
        wp.copy_(wp1)
    second = head(x.cuda()).detach().cpu()
    for w, got in ((wp0, first), (wp1, second)):
        te = text.double() / text.double().norm(dim=-1, keepdim=True)
        ref = H.reference(te @ w.double(), w.double().t() @ w.double(), x, torch.zeros(49, 33), float(ls.double().exp()), "f32", 2, oracle=True)
        assert H.ratio(got, ref["logits"], ref["B_logits"]) <= 1.0
    assert not torch.equal(first, second)


def test_the_operands_are_the_class_scorers_bit_for_bit():
    """class_head.collapsed_operands restates the arithmetic of ClassScorer._pack: G and A from it, packed by msda_cls_pack, are the
    scorer's own packed operand bit for bit (the two must not drift apart while they are two functions)"""
    from richsem_amd import _lib
    from richsem_amd.class_head import collapsed_operands
    from richsem_amd.two_stage import ClassScorer
    gen = torch.Generator().manual_seed(11)
    for classes, proj in ((33, 64), (1204, 1024)):
        wp, text = (torch.randn(proj, 256, generator=gen) / 8).cuda(), torch.randn(classes, proj, generator=gen).cuda()
        want = ClassScorer(2).prepare(wp, text, torch.tensor(2.0)).packed
        G, A, _ = collapsed_operands(wp, text)
        got = torch.zeros_like(want)
        _lib.check(_lib.load().msda_cls_pack(G.data_ptr(), classes, A.data_ptr(), 256, got.data_ptr(), _lib.raw_stream()))
        torch.cuda.synchronize()
        assert torch.equal(got, want), (classes, proj)
