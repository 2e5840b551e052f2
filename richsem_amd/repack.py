"""Grouped re-pack: every derived form of the trained parameters (bf16 casts, lin256's fragment order, the feed-forward kernel's W2 order,
the convolutions' forward and input-gradient packs) refreshed from the fp32 masters in ONE launch (csrc/msda_repack.h).

    plan = RepackPlan()
    with plan.record():                 # ONE eager forward + backward of the model
        loss = model(...); loss.backward()
    plan.refresh()                      # one launch; capturable; no host synchronisation
    opt.attach_repack(plan)             # ClipAdamW.step(): sumsq, step, then the refresh (a third launch)
    plan.release()                      # every cache back to its own behaviour

While recording, every ``VersionCache.get`` / ``PackCache.get`` (param_cache.py, conv.py) that is asked for its forms builds them with
its own ``build()``, and the builders note one job per tensor they return (``param_cache.note``).  A cache whose value consists of noted
tensors (and of views of its own parameters) is BOUND: the tensors built during the recording become the plan's persistent destinations,
and from then on the cache hands those out.  Outside a capture a bound cache compares its parameters' ``(data_ptr, _version)`` with what
the plan last refreshed from and, on a mismatch, refreshes the WHOLE plan in one launch instead of building; during a capture it returns
the buffers and launches nothing.  A cache whose value holds a tensor no job writes stays as it was and is listed in ``plan.unbound``;
so does a cache that was not asked during the recording.  A bound cache whose parameters have moved to other memory unbinds itself.
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib, param_cache

CHUNK = _lib.REPACK_CHUNK
MAX_SEGS = _lib.REPACK_MAX_SEGS
JOB_DT, CHUNK_DT = _lib.repack_dtypes()      # include/richsem_msda.h: msda_repack_job / msda_repack_chunk
KINDS = {"cast": 0, "copy": 1, "lin256": 2, "lin256_t": 3, "ffn_w2": 4, "conv": 5, "conv_t": 6}
_ROW_KINDS = ("lin256", "lin256_t")      # seg_end counts rows; the others count elements


def plan_chunks(jobs):
    """the chunk table of a HOST job table (structured array of JOB_DT; host only: msda_repack_plan, which also checks the jobs) ->
    structured array of CHUNK_DT"""
    jobs = np.ascontiguousarray(jobs, dtype=JOB_DT)
    L = _lib.load()
    count = ctypes.c_int64(0)
    _lib.check(L.msda_repack_plan(jobs.ctypes.data, len(jobs), None, 0, ctypes.byref(count)))
    out = np.zeros(count.value, dtype=CHUNK_DT)
    if count.value:
        _lib.check(L.msda_repack_plan(jobs.ctypes.data, len(jobs), out.ctypes.data, count.value, ctypes.byref(count)))
    return out


def job_row(kind, dst, segments, scale=None):
    """one JOB_DT row: ``dst`` is the form ``kind`` of the fp32 ``segments`` (param_cache.note's arguments)"""
    row = np.zeros((), dtype=JOB_DT)
    row["dst"], row["n_dst"], row["kind"], row["n_segs"] = dst.data_ptr(), dst.numel(), KINDS[kind], len(segments)
    end = 0
    for s, t in enumerate(segments):
        end += t.shape[0] if kind in _ROW_KINDS else t.numel()
        row["src"][s], row["seg_end"][s] = t.data_ptr(), end
    if kind in _ROW_KINDS:
        row["dims"][0] = dst.shape[0]
    elif kind == "ffn_w2":
        row["dims"][:2] = dst.shape
    elif kind in ("conv", "conv_t"):
        w = segments[0]
        row["dims"][:4] = w.shape
        row["dims"][4] = dst.numel() // (w.shape[1] if kind == "conv_t" else w.shape[0])
        if scale is not None:
            row["scale"] = scale.data_ptr()
    return row


def _leaves(val, out):
    if torch.is_tensor(val):
        out.append(val)
    elif isinstance(val, dict):
        for v in val.values():
            _leaves(v, out)
    elif isinstance(val, (list, tuple)):
        for v in val:
            _leaves(v, out)
    return out


def _key(t):
    return (t.data_ptr(), t.dtype, tuple(t.shape))


class _Job:
    __slots__ = ("kind", "dst", "segments", "scale")

    def __init__(self, kind, dst, segments, scale):
        self.kind, self.dst, self.segments, self.scale = kind, dst, segments, scale


class Binding:
    """one cache (or one slot of a PackCache) bound to a plan: the value it hands out, the parameters it is keyed on and what the plan
    last refreshed from"""

    def __init__(self, plan, owner, slot, params, val, jobs):
        self.plan, self.owner, self.slot, self.params, self.val, self.jobs = plan, owner, slot, tuple(params), val, jobs
        self.ptrs = tuple(p.data_ptr() for p in params)
        self.ver = tuple((p.data_ptr(), p._version) for p in params)

    def get(self, params):
        if param_cache.capturing(params[0]):
            self.plan._require_ready()
            return self.val
        ver = tuple((p.data_ptr(), p._version) for p in params)
        if ver != self.ver:
            if tuple(a for a, _ in ver) != self.ptrs:
                self.plan._drop(self)
                return param_cache.UNBOUND
            self.plan.refresh()
        return self.val


class RepackPlan:
    """See the module docstring.  ``unbound``: one ``{"cache", "slot", "reason"}`` per cache that was asked for its forms during the
    recording and stays on its own behaviour; :meth:`unbound_names` names their owners in a model."""

    def __init__(self):
        self.bindings = []
        self.unbound = []
        self._scopes = []
        self._declined = set()       # (id(cache), slot) of what this recording left unbound: asked again, it answers from its own cache
        self._table = None           # (device bytes, jobs ptr, chunks ptr, n_chunks, n_jobs, bytes moved)
        self._tables = []            # every table ever uploaded: a captured graph may hold its address
        self._dirty = True
        self._recording = False
        self._stepped = False
        self.launches = 0            # refresh launches issued (eager) or recorded (capturing)

    # ---- recording ----------------------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def record(self):
        if param_cache.stream_capturing():
            raise RuntimeError("RepackPlan.record(): not inside a graph capture (the destinations live outside any graph's memory pool)")
        if param_cache._RECORDING is not None:
            raise RuntimeError("RepackPlan.record(): another plan is recording")
        param_cache._RECORDING, self._recording = self, True
        try:
            yield self
        finally:
            param_cache._RECORDING, self._recording = None, False
            self._scopes = []
        self._finalise()

    def _note(self, kind, dst, segments, scale):
        if not self._scopes:
            return      # a builder called outside any cache: nobody keeps what it returns
        segments = [t.detach() for t in segments]
        ok = (kind in KINDS and 1 <= len(segments) <= MAX_SEGS and dst.is_contiguous()
              and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dst.device and t.numel() > 0 for t in segments)
              and (kind != "conv_t" or (scale is not None and scale.dtype == torch.float32 and scale.is_contiguous()
                                        and scale.device == dst.device and scale.numel() == segments[0].shape[0])))
        if not ok:
            return      # (its cache then holds a tensor no job writes, and stays unbound)
        if any(dst.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for t in segments):
            return      # a view of the master itself (``bias.float().contiguous()`` of an fp32 bias): always fresh
        self._scopes[-1].append(_Job(kind, dst, segments, scale))

    def declined(self, owner, slot):
        return (id(owner), slot) in self._declined

    def _record(self, owner, slot, params, build):
        """``build()`` with the builders' notes collected -> (value, Binding or None)"""
        scope = []
        self._scopes.append(scope)
        try:
            with torch.no_grad():
                val = build()
        finally:
            self._scopes.pop()
        noted = {_key(j.dst) for j in scope}
        own = {p.untyped_storage().data_ptr() for p in params}
        leaves = _leaves(val, [])
        loose = [t for t in leaves if _key(t) not in noted and t.untyped_storage().data_ptr() not in own]
        if loose or not scope:
            reason = (f"{len(loose)} of {len(leaves)} tensors of its value are written by no job" if loose else "no job noted")
            self.unbound.append({"cache": owner, "slot": slot, "reason": reason})
            self._declined.add((id(owner), slot))
            return val, None
        held = {_key(t) for t in leaves}
        b = Binding(self, owner, slot, params, val, [j for j in scope if _key(j.dst) in held])
        self.bindings.append(b)
        self._dirty = True
        return val, b

    def _finalise(self):
        jobs = self.jobs()
        if jobs and jobs[0].dst.is_cuda:      # (the table of CPU stand-ins is never built: there is no CPU implementation)
            self._build_table()

    # ---- the device table ----------------------------------------------------------------------------------------------------------
    def jobs(self):
        return [j for b in self.bindings for j in b.jobs]

    def _build_table(self):
        jobs = self.jobs()
        if not jobs:
            self._table, self._dirty = None, False
            return
        dev = jobs[0].dst.device
        if dev.type != "cuda" or any(j.dst.device != dev for j in jobs):
            raise RuntimeError("richsem_amd.repack.RepackPlan: every form must be on one GPU (no CPU implementation)")
        rows = np.zeros(len(jobs), dtype=JOB_DT)
        for i, j in enumerate(jobs):
            rows[i] = job_row(j.kind, j.dst, j.segments, j.scale)
        chunks = plan_chunks(rows)
        at = rows.nbytes
        nbytes = at + chunks.nbytes
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        host = pinned.numpy()
        host[:at].view(JOB_DT)[:] = rows
        host[at:nbytes].view(CHUNK_DT)[:] = chunks
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        buf.copy_(pinned, non_blocking=True)
        moved = sum(sum(t.numel() for t in j.segments) * 4 + j.dst.numel() * j.dst.element_size() for j in jobs)
        self._table = (buf, buf.data_ptr(), buf.data_ptr() + at, len(chunks), len(jobs), moved)
        self._tables.append((buf, pinned))
        self._dirty = False

    @property
    def n_jobs(self):
        return len(self.jobs())

    @property
    def n_chunks(self):
        return 0 if self._table is None else self._table[3]

    @property
    def bytes_moved(self):
        """bytes one refresh reads from the masters and writes to the forms (the minimum: every source element counted once per job)"""
        return 0 if self._table is None else self._table[5]

    def _require_ready(self):
        if self._recording or self._dirty or (self._table is None and self.bindings):
            raise RuntimeError("RepackPlan: a bound cache was asked for its forms inside a graph capture before the plan was finalised "
                               "(leave `with plan.record():`, and call plan.refresh() once after dropping a binding)")

    # ---- the refresh ---------------------------------------------------------------------------------------------------------------
    def _launch(self):
        buf, jobs_ptr, chunks_ptr, n_chunks = self._table[:4]
        dev = buf.device
        with _lib.on_device(dev):
            _lib.check(_lib.load().msda_repack(jobs_ptr, chunks_ptr, n_chunks, _lib.raw_stream(dev)))

    def refresh(self, _snapshot=True):
        """every bound form from the current masters: one launch on the current stream, no host synchronisation; inside a graph capture
        the launch is recorded"""
        if self._recording:
            raise RuntimeError("RepackPlan.refresh(): the plan is still recording")
        cap = param_cache.stream_capturing()
        if self._dirty:
            if cap:
                raise RuntimeError("RepackPlan.refresh(): the job table must be built outside a graph capture (call refresh() once before it)")
            self._build_table()
        if self._table is not None:
            self._launch()
            self.launches += 1
        if not cap and _snapshot:
            self._snapshot()

    def _snapshot(self):
        """the forms are as new as the masters are now; a binding whose parameters moved is dropped"""
        for b in list(self.bindings):
            ver = tuple((p.data_ptr(), p._version) for p in b.params)
            if tuple(a for a, _ in ver) != b.ptrs:
                self._drop(b)
                _unbind(b)
            else:
                b.ver = ver

    def _after_step(self):
        """(the optimizer step hook) a ClipAdamW step that ended with this plan's refresh has just had its parameters' versions bumped"""
        if self._stepped:
            self._stepped = False
            if not param_cache.stream_capturing():
                self._snapshot()

    def _drop(self, b):
        if b in self.bindings:
            self.bindings.remove(b)
            self._dirty = True
            self.unbound.append({"cache": b.owner, "slot": b.slot, "reason": "its parameters moved to other memory"})

    def release(self):
        """every bound cache back to its own behaviour (it rebuilds on its next ``get``)"""
        for b in self.bindings:
            _unbind(b)
        self.bindings = []
        self._table, self._dirty = None, True

    def unbound_names(self, model):
        """``unbound`` with the owners' names in ``model``: [(attribute path, slot, reason)].  The caches are looked for in the modules
        and in the plain objects they hold (the class scorer, the frozen teacher), a few levels deep."""
        names, seen = {}, set()

        def walk(obj, path, depth):
            if id(obj) in seen or depth > 6:
                return
            seen.add(id(obj))
            if isinstance(obj, param_cache.VersionCache) or type(obj).__name__ == "PackCache":
                names[id(obj)] = path
            elif isinstance(obj, dict):
                for k, v in obj.items():
                    walk(v, f"{path}[{k}]", depth + 1)
            elif isinstance(obj, (list, tuple)):
                for i, v in enumerate(obj):
                    walk(v, f"{path}[{i}]", depth + 1)
            elif isinstance(obj, torch.nn.Module):
                for k, v in obj._modules.items():
                    walk(v, f"{path}.{k}" if path else k, depth)
                for k, v in vars(obj).items():
                    if k not in ("_modules", "_parameters", "_buffers") and not k.startswith("_forward") and not k.startswith("_backward"):
                        walk(v, f"{path}.{k}" if path else k, depth + 1)
            elif hasattr(obj, "__dict__") and not torch.is_tensor(obj) and not type(obj).__module__.startswith(("torch", "builtins", "numpy")):
                for k, v in vars(obj).items():
                    walk(v, f"{path}.{k}" if path else k, depth + 1)
        walk(model, "", 0)
        return [(names.get(id(u["cache"]), repr(u["cache"])), u["slot"], u["reason"]) for u in self.unbound]


def _unbind(b):
    owner = b.owner
    if b.slot is None:
        if owner._binding is b:
            owner._binding = None
            owner._ver = owner._val = None
    else:
        owner._unbind_slot(b)
