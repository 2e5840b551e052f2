"""CPU: the grouped re-pack's table layouts, chunk planner, host argument checks and binding logic (no kernel is launched).

The binding logic runs with CPU stand-ins for the builders, in the style of tests/test_param_caches.py: a recorded cache is bound, a
version mismatch costs exactly one ``refresh`` and no ``build``, a deep copy is unbound, a cache whose value holds a tensor no job writes
stays unbound and is listed, and ``release()`` gives every cache back its own behaviour."""
import copy
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from richsem_amd import _build, _lib, conv, param_cache, repack
from richsem_amd.param_cache import VersionCache

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "richsem_msda.h")
CHUNK = repack.CHUNK


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


# ---- layouts -------------------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_header(tmp_path):
    """sizes and offsets of msda_repack_job / msda_repack_chunk as a C compiler lays them out, against the numpy dtypes"""
    src = tmp_path / "layout.c"
    fields = {"msda_repack_job": ["dst", "scale", "src", "seg_end", "n_dst", "kind", "n_segs", "dims", "reserved"],
              "msda_repack_chunk": ["offset", "job", "count"]}
    body = "".join(f'printf("{s} %zu\\n", sizeof({s}));' + "".join(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));' for f in fs)
                   for s, fs in fields.items())
    body += 'printf("CHUNK %d\\nMAX_SEGS %d\\n", MSDA_REPACK_CHUNK, MSDA_REPACK_MAX_SEGS);'
    body += "".join(f'printf("kind.{k} %d\\n", MSDA_REPACK_{k.upper()});' for k in repack.KINDS)
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{ {body} return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-o", str(exe), str(src)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, dt in (("msda_repack_job", repack.JOB_DT), ("msda_repack_chunk", repack.CHUNK_DT)):
        assert int(got[name]) == dt.itemsize, name
        for f in fields[name]:
            assert int(got[f"{name}.{f}"]) == dt.fields[f][1], (name, f)
    assert int(got["CHUNK"]) == CHUNK == _lib.REPACK_CHUNK and int(got["MAX_SEGS"]) == repack.MAX_SEGS == _lib.REPACK_MAX_SEGS
    for k, v in repack.KINDS.items():
        assert int(got[f"kind.{k}"]) == v, k


def test_symbols_are_declared_bound_and_exported_and_the_abi_version_stays(lib):
    header = open(HEADER).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.lib_path()], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for sym in ("msda_repack_plan", "msda_repack"):
        assert sym in _lib.SYMBOLS and re.search(r"\bint %s\(" % sym, header) and sym in exported, sym
        assert getattr(lib, sym).argtypes is not None
    assert "repack_api.hip" in _build.SOURCES
    assert lib.msda_abi_version() == 13 == _lib.ABI_VERSION
    assert b"repack_kernel" in open(_lib.lib_path(), "rb").read()


# ---- the planner -----------------------------------------------------------------------------------------------------------------------
def _cast_jobs(sizes, base=0x10000):
    """flat-cast jobs of the given destination sizes over fake (never dereferenced) pointers: one source element each, the rest of every
    destination is zero padding"""
    rows = np.zeros(len(sizes), dtype=repack.JOB_DT)
    for i, n in enumerate(sizes):
        rows[i]["dst"], rows[i]["n_dst"], rows[i]["kind"], rows[i]["n_segs"] = base + 0x100000 * i, n, repack.KINDS["cast"], 1
        rows[i]["src"][0], rows[i]["seg_end"][0] = base + 4, 1
    return rows


def _expected_chunks(sizes):
    want = []
    for j, n in enumerate(sizes):
        for off in range(0, n, CHUNK):
            want.append((off, j, min(CHUNK, n - off)))
    return want


@pytest.mark.parametrize("sizes", [[1], [CHUNK - 1], [CHUNK], [CHUNK + 1], [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 0, 3 * CHUNK + 5],
                                   [7] * 300 + [2 * CHUNK + 1] * 40])
def test_plan_chunk_tables(lib, sizes):
    chunks = repack.plan_chunks(_cast_jobs(sizes))
    assert [tuple(int(x) for x in c) for c in chunks] == _expected_chunks(sizes)
    assert all(int(c["offset"]) % CHUNK == 0 and 1 <= int(c["count"]) <= CHUNK for c in chunks)


def test_plan_of_only_empty_jobs_has_no_chunks(lib):
    rows = _cast_jobs([0, 0])
    n = ctypes.c_int64(-1)
    assert lib.msda_repack_plan(rows.ctypes.data, 2, None, 0, ctypes.byref(n)) == 0 and n.value == 0
    assert len(repack.plan_chunks(rows)) == 0


def _good_row():
    rows = _cast_jobs([100])
    rows["seg_end"][0, 0] = 100
    return rows


def test_host_checks_of_the_planner(lib):
    n = ctypes.c_int64(0)
    out = np.zeros(8, dtype=repack.CHUNK_DT)
    rows = _good_row()
    plan = lambda r, cap=0, chunks=None, nj=1: lib.msda_repack_plan(r.ctypes.data, nj, chunks, cap, ctypes.byref(n))
    assert plan(rows) == 0 and n.value == 1
    assert lib.msda_repack_plan(None, 1, None, 0, ctypes.byref(n)) == -1
    assert lib.msda_repack_plan(rows.ctypes.data, 1, None, 0, None) == -1
    assert plan(rows, nj=0) == -2
    assert plan(rows, 0, out.ctypes.data) == -2 and "msda_repack_plan" in _lib.last_error()      # no room
    assert lib.msda_repack_plan(rows.ctypes.data + 4, 1, None, 0, ctypes.byref(n)) == -5
    big = _good_row()
    big["n_dst"] = 3 * CHUNK + 1
    assert plan(big, 3, out.ctypes.data) == -2 and plan(big, 4, out.ctypes.data) == 0 and n.value == 4

    def bad(code, **changes):
        r = _good_row()
        for k, v in changes.items():
            if isinstance(v, tuple):
                r[k][0, v[0]] = v[1]
            else:
                r[k] = v
        assert plan(r) == code, changes
        assert "msda_repack_plan" in _lib.last_error()

    bad(-1, dst=0)
    bad(-1, src=(0, 0))
    bad(-5, dst=0x10008)                    # destinations are written 16 bytes at a time
    bad(-5, src=(0, 0x10002))
    bad(-2, kind=7)
    bad(-2, kind=-1)
    bad(-2, n_segs=0)
    bad(-2, n_segs=repack.MAX_SEGS + 1)
    bad(-2, n_dst=-1)
    bad(-2, n_dst=99)                       # smaller than its source
    bad(-2, seg_end=(0, 0))
    bad(-4, n_dst=1 << 31)
    bad(-2, kind=repack.KINDS["lin256"])                                # dims do not fit
    bad(-2, kind=repack.KINDS["ffn_w2"])
    bad(-2, kind=repack.KINDS["conv"])
    # a well-formed job of every other kind, and what each kind refuses
    r = _good_row()
    r["kind"], r["n_dst"], r["seg_end"][0, 0], r["dims"][0, 0] = repack.KINDS["lin256"], 64 * 256, 4, 64
    assert plan(r) == 0 and n.value == 2
    r["seg_end"][0, 0] = 65
    assert plan(r) == -2
    r["kind"], r["seg_end"][0, 0] = repack.KINDS["lin256_t"], 256
    assert plan(r) == 0
    r["seg_end"][0, 0] = 255
    assert plan(r) == -2
    r = _good_row()
    r["kind"], r["n_dst"], r["seg_end"][0, 0] = repack.KINDS["ffn_w2"], 256 * 96, 256 * 96
    r["dims"][0, :2] = (256, 96)
    assert plan(r) == 0 and n.value == 3
    r["dims"][0, 1] = 100
    assert plan(r) == -2
    r = _good_row()
    r["kind"], r["n_dst"], r["seg_end"][0, 0] = repack.KINDS["conv"], 16 * 160, 16 * 3 * 7 * 7
    r["dims"][0, :5] = (16, 3, 7, 7, 160)
    assert plan(r) == 0
    r["dims"][0, 4] = 147
    assert plan(r) == -2
    r = _good_row()
    r["kind"], r["n_dst"], r["seg_end"][0, 0] = repack.KINDS["conv_t"], 32 * 288, 32 * 32 * 9
    r["dims"][0, :5] = (32, 32, 3, 3, 288)
    assert plan(r) == -1                    # the input-gradient form needs its scale
    r["scale"] = 0x20000
    assert plan(r) == 0
    r["scale"] = 0x20002
    assert plan(r) == -5
    r["scale"], r["n_segs"] = 0x20000, 2
    r["src"][0, 1], r["seg_end"][0, 1] = 0x30000, 32 * 32 * 9 + 1
    assert plan(r) == -2                    # a convolution weight is one segment


def test_host_checks_of_the_launch(lib):
    buf = (ctypes.c_char * 1024)()
    p = (ctypes.addressof(buf) + 255) & ~255
    assert lib.msda_repack(None, p, 1, None) == -1
    assert lib.msda_repack(p, None, 1, None) == -1 and "msda_repack" in _lib.last_error()
    assert lib.msda_repack(p, p, -1, None) == -2
    assert lib.msda_repack(p + 4, p, 1, None) == -5
    assert lib.msda_repack(p, p + 4, 1, None) == -5
    assert lib.msda_repack(p, p, 0, None) == 0      # nothing to do: nothing launched
    with pytest.raises(RuntimeError, match="msda_repack.*MSDA_ERR_BAD_DIMS"):
        _lib.check(lib.msda_repack(p, p, -1, None))


def test_job_row_mirrors_the_builders_arguments():
    w = [torch.zeros(128, 256), torch.zeros(64, 256)]
    row = repack.job_row("lin256", torch.zeros(192, 256, dtype=torch.bfloat16), w)
    assert int(row["kind"]) == 2 and int(row["n_segs"]) == 2 and list(row["seg_end"][:2]) == [128, 192] and int(row["dims"][0]) == 192
    assert int(row["n_dst"]) == 192 * 256 and int(row["src"][1]) == w[1].data_ptr()
    row = repack.job_row("cast", torch.zeros(192, 256, dtype=torch.bfloat16), w)
    assert list(row["seg_end"][:2]) == [128 * 256, 192 * 256]
    cw, s = torch.zeros(32, 64, 3, 3), torch.ones(32)
    row = repack.job_row("conv_t", torch.zeros(64 * 288, dtype=torch.int16), [cw], s)
    assert list(row["dims"][:5]) == [32, 64, 3, 3, 288] and int(row["scale"]) == s.data_ptr() and int(row["seg_end"][0]) == cw.numel()


# ---- the binding logic, with CPU stand-ins for the builders ----------------------------------------------------------------------------
class _HostPlan(repack.RepackPlan):
    """a plan whose refresh runs the jobs on the host: the kernel's definition for the flat kinds (what the stand-ins use)"""

    def __init__(self):
        super().__init__()
        self.refreshes = 0

    def _finalise(self):
        pass

    def _build_table(self):
        self._table, self._dirty = ("host",), False

    def _launch(self):
        self.refreshes += 1
        for j in self.jobs():
            flat = torch.cat([t.reshape(-1) for t in j.segments])
            assert j.kind in ("cast", "copy")
            j.dst.reshape(-1)[:flat.numel()] = flat.to(j.dst.dtype)


class _Counting:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(64, 32, generator=g) * 0.5), torch.nn.Parameter(torch.randn(64, generator=g) * 0.5)]


def _grads(params, seed):
    g = torch.Generator().manual_seed(seed)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


def _forms(params):
    return {"w16": param_cache.cast_bf16(params[0]), "b16": param_cache.cast_bf16(params[1]), "rows": [64]}


def _fresh(params):
    return {"w16": params[0].detach().to(torch.bfloat16), "b16": params[1].detach().to(torch.bfloat16)}


def _same(val, params):
    want = _fresh(params)
    return all(torch.equal(val[k], want[k]) for k in want)


def test_record_binds_and_a_version_mismatch_costs_one_refresh_and_no_build():
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        v0 = cache.get(params, build)
        assert cache.get(params, build) is v0      # (the backward's lookup during the same recording)
    assert build.calls == 1 and cache._binding is not None and len(plan.bindings) == 1 and plan.n_jobs == 2 and not plan.unbound
    assert cache.get(params, build) is v0 and plan.refreshes == 0
    opt = torch.optim.AdamW(params, lr=0.1, fused=True)
    for step in range(3):
        _grads(params, 10 + step)
        opt.step()                                       # (the step hook bumps the versions)
        got = cache.get(params, build)
        assert got is v0 and _same(got, params), step    # the same persistent tensors, refreshed in place
        assert plan.refreshes == step + 1 and build.calls == 1
        assert cache.get(params, build) is v0 and plan.refreshes == step + 1
    with torch.no_grad():
        params[0].copy_(torch.randn(64, 32))
    assert _same(cache.get(params, build), params) and plan.refreshes == 4 and build.calls == 1
    other = _params(5)
    torch.nn.ParameterList(params).load_state_dict(torch.nn.ParameterList(other).state_dict())
    assert _same(cache.get(params, build), params) and plan.refreshes == 5 and build.calls == 1
    params[0].data.mul_(0.5)                             # invisible to the version counter: clear() is the documented remedy
    cache.clear()
    assert _same(cache.get(params, build), params) and plan.refreshes == 6 and build.calls == 1


def test_an_explicit_refresh_after_the_step_is_the_only_launch():
    """any optimizer + ``plan.refresh()`` after its step: the next get finds the forms as new as the masters"""
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        cache.get(params, build)
    opt = torch.optim.SGD(params, lr=0.1, fused=True)
    _grads(params, 3)
    opt.step()
    plan.refresh()
    assert plan.refreshes == 1
    assert _same(cache.get(params, build), params) and plan.refreshes == 1 and build.calls == 1


def test_a_step_that_ends_with_the_refresh_is_not_refreshed_again():
    """an optimizer that carries the plan (``ClipAdamW.attach_repack``): its step refreshes, the step hook then bumps the versions and
    records them as what the forms were refreshed from"""
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        cache.get(params, build)

    class Carrying(torch.optim.SGD):
        def step(self):
            super().step()
            self._repack.refresh(_snapshot=False)
            self._repack._stepped = True

    opt = Carrying(params, lr=0.1)
    opt._repack = plan
    for step in range(2):
        _grads(params, 20 + step)
        opt.step()
        assert plan.refreshes == step + 1
        assert _same(cache.get(params, build), params) and plan.refreshes == step + 1 and build.calls == 1
    # a plain optimizer's step on the same parameters is still seen
    _grads(params, 30)
    torch.optim.SGD(params, lr=0.1).step()
    assert _same(cache.get(params, build), params) and plan.refreshes == 3


def test_a_deep_copy_of_a_bound_cache_is_unbound():
    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w, self.b = _params()
            self.cache = VersionCache()
            self.builds = 0

        def forms(self):
            def build():
                self.builds += 1
                return _forms([self.w, self.b])
            return self.cache.get([self.w, self.b], build)

    m = Holder()
    plan = _HostPlan()
    with plan.record():
        v0 = m.forms()
    twin = copy.deepcopy(m)
    assert twin.cache._binding is None and twin.cache._val is None and len(plan.bindings) == 1
    tv = twin.forms()
    assert twin.builds == 2 and tv["w16"].data_ptr() != v0["w16"].data_ptr()      # its own build from its own parameters
    with torch.no_grad():
        m.w.mul_(2.0)
    assert _same(m.forms(), [m.w, m.b]) and plan.refreshes == 1
    assert torch.equal(twin.forms()["w16"], twin.w.detach().to(torch.bfloat16)) and not torch.equal(twin.forms()["w16"], m.forms()["w16"])
    # an unbound cache deep-copies as before: value and key travel
    plain = VersionCache()
    ps = _params(2)
    plain.get(ps, lambda: _fresh(ps))
    c = copy.deepcopy(plain)
    assert c._ver == plain._ver and torch.equal(c._val["w16"], plain._val["w16"]) and c._val["w16"] is not plain._val["w16"]


def test_a_value_with_an_unnoted_tensor_stays_unbound_and_is_listed():
    params = _params()
    cache, loose = VersionCache(), VersionCache()
    build = _Counting(lambda: _forms(params))
    build_loose = _Counting(lambda: {"w16": param_cache.cast_bf16(params[0]), "t": params[0].detach().t().contiguous()})
    plan = _HostPlan()
    with plan.record():
        cache.get(params, build)
        l0 = loose.get(params, build_loose)
        assert loose.get(params, build_loose) is l0 and build_loose.calls == 1      # cached as ever
    assert loose._binding is None and [u["cache"] for u in plan.unbound] == [loose] and "no job" in plan.unbound[0]["reason"]
    assert plan.n_jobs == 2                                                          # none of the loose cache's notes is kept
    opt = torch.optim.AdamW(params, lr=0.1, fused=True)
    _grads(params, 7)
    opt.step()
    l1 = loose.get(params, build_loose)
    assert build_loose.calls == 2 and torch.equal(l1["t"], params[0].detach().t())   # follows the optimizer the old way
    never = VersionCache()                                                           # not asked during the recording: untouched
    assert never._binding is None and never.get(params, build) is not None and build.calls == 2


def test_a_view_of_the_master_needs_no_job():
    params = _params()
    cache = VersionCache()
    plan = _HostPlan()

    def build():
        b32 = params[1].detach().float().contiguous()      # the fp32 bias itself
        param_cache.note("copy", b32, [params[1]])
        return {"w16": param_cache.cast_bf16(params[0]), "b32": b32}
    with plan.record():
        v = cache.get(params, build)
    assert cache._binding is not None and plan.n_jobs == 1 and v["b32"].data_ptr() == params[1].data_ptr()


def test_release_restores_rebuilding():
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        v0 = cache.get(params, build)
    plan.release()
    assert cache._binding is None and not plan.bindings
    v1 = cache.get(params, build)
    assert build.calls == 2 and v1 is not v0
    _grads(params, 1)
    torch.optim.AdamW(params, lr=0.1, fused=True).step()
    assert _same(cache.get(params, build), params) and build.calls == 3 and plan.refreshes == 0


def test_parameters_that_moved_unbind_the_cache():
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        cache.get(params, build)
    params[0].data = params[0].data.clone() * 3.0        # other memory: the job's pointer is the old one
    got = cache.get(params, build)
    assert cache._binding is None and build.calls == 2 and _same(got, params) and not plan.bindings
    assert "moved" in plan.unbound[-1]["reason"]


def test_a_bound_cache_refuses_a_capture_before_the_plan_is_ready(monkeypatch):
    params = _params()
    cache = VersionCache()
    build = _Counting(lambda: _forms(params))
    plan = _HostPlan()
    with plan.record():
        v0 = cache.get(params, build)
    monkeypatch.setattr(param_cache, "capturing", lambda t: True)
    with pytest.raises(RuntimeError, match="before the plan was finalised"):
        cache.get(params, build)                          # (this stand-in plan builds its table at the first refresh)
    monkeypatch.setattr(param_cache, "capturing", lambda t: False)
    plan.refresh()
    monkeypatch.setattr(param_cache, "capturing", lambda t: True)
    _grads(params, 2)
    torch.optim.SGD(params, lr=0.1).step()
    assert cache.get(params, build) is v0 and plan.refreshes == 1 and build.calls == 1      # the buffers, and no launch
    # a cache that is not bound still builds on every call while capturing
    plain = VersionCache()
    assert plain.get(params, build) is not plain.get(params, build) and build.calls == 3


def test_pack_cache_slots_bind_separately(monkeypatch):
    def stand_in(weight, scale, transposed):
        w = weight.detach().float()
        if transposed:                                    # (no job can write this stand-in form: the slot stays unbound)
            return (w * scale.view(-1, 1, 1, 1)).flip(2, 3).permute(1, 0, 2, 3).contiguous().to(torch.bfloat16)
        return param_cache.cast_bf16(weight)

    pack = _Counting(stand_in)
    monkeypatch.setattr(conv, "_pack_form", pack)
    g = torch.Generator().manual_seed(1)
    w = torch.nn.Parameter(torch.randn(32, 16, 3, 3, generator=g) * 0.2)
    scale = torch.rand(32, generator=g) + 0.5
    cache = conv.PackCache()
    plan = _HostPlan()
    with plan.record():
        f0 = cache.get(w, scale, False)
        t0 = cache.get(w, scale, True)
        assert cache.get(w, scale, False) is f0 and cache.get(w, scale, True) is t0
    assert pack.calls == 2 and list(cache._bound) == [False] and [(u["cache"], u["slot"]) for u in plan.unbound] == [(cache, True)]
    _grads([w], 4)
    torch.optim.AdamW([w], lr=0.1, fused=True).step()
    assert cache.get(w, scale, False) is f0 and torch.equal(f0, w.detach().to(torch.bfloat16)) and plan.refreshes == 1 and pack.calls == 2
    assert torch.equal(cache.get(w, scale, True), stand_in(w, scale, True)) and pack.calls == 3
    twin = copy.deepcopy(cache)
    assert not twin._bound and not twin._slots
    plan.release()
    assert not cache._bound
    assert cache.get(w, scale, False) is not f0 and pack.calls == 4
