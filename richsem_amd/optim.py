"""What follows ``losses.backward()`` in the reference's training loop (engine.py:110-120) on the library's kernels: gradient clipping,
AdamW and the EMA of the weights in two launches (csrc/msda_optim.h), plus the parameter groups of util/get_param_dicts.py.

    groups = param_groups(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, param_dict_type="large_wd")
    opt = ClipAdamW(groups, lr=1e-4, weight_decay=1e-4, max_norm=0.1)
    ema = ModelEma(model, decay=0.9997); opt.attach_ema(ema)
    ...
    loss.backward(); opt.step(); ema.update(model)          # opt.total_norm: the gradient norm, a device tensor

Everything the kernels read lives in device tables: the tensor / chunk table (pointers, rebuilt when a parameter's or a gradient's
address changes), the group table (lr, betas, eps, weight_decay per group) and the call-wide settings (max_norm, ema_decay, ema_on).  A
step captured into a graph therefore follows a schedule without being captured again: ``scheduler.step(); opt.sync(); graph.replay()``.
"""
import ctypes
from copy import deepcopy

import numpy as np
import torch

from . import _lib

CHUNK = _lib.OPTIM_CHUNK
# include/richsem_msda.h: msda_optim_tensor / _chunk / _group / _settings
TENSOR_DT = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("ema", "<u8"), ("step", "<u8"),
                      ("numel", "<i8"), ("group", "<i4"), ("reserved", "<i4")])
CHUNK_DT = np.dtype([("offset", "<i8"), ("tensor", "<i4"), ("count", "<i4")])
GROUP_DT = np.dtype([("lr", "<f8"), ("beta1", "<f8"), ("beta2", "<f8"), ("eps", "<f8"), ("weight_decay", "<f8")])
SETTINGS_DT = np.dtype([("max_norm", "<f8"), ("ema_decay", "<f8"), ("ema_on", "<i4"), ("reserved", "<i4")])
assert (TENSOR_DT.itemsize, CHUNK_DT.itemsize, GROUP_DT.itemsize, SETTINGS_DT.itemsize) == (64, 16, 40, 24)
_GROUPS_AT = 32      # the group table follows the settings in one device buffer, at this byte


def plan_chunks(numels):
    """the chunk table of a list of element counts (host only: msda_optim_plan) -> structured array of CHUNK_DT"""
    n = np.ascontiguousarray(numels, dtype=np.int64)
    L = _lib.load()
    count = ctypes.c_int64(0)
    _lib.check(L.msda_optim_plan(n.ctypes.data, len(n), None, 0, ctypes.byref(count)))
    out = np.zeros(count.value, dtype=CHUNK_DT)
    _lib.check(L.msda_optim_plan(n.ctypes.data, len(n), out.ctypes.data, count.value, ctypes.byref(count)))
    return out


def _check_tensor(t, what):
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: float32 only (got {t.dtype}); bf16 masters and state are not supported")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous (shape {tuple(t.shape)}, strides {t.stride()})")


class _Table:
    """one uploaded tensor + chunk table: the pinned host copy, the device copy and the partial sums of its chunks.  Never rewritten: a
    rebuild makes a new one, so a graph that recorded the upload of this one copies the same bytes into the same buffer on every replay."""

    def __init__(self, rows, numels, device, pinned=None):
        chunks = plan_chunks(numels)
        self.n_chunks = len(chunks)
        at = rows.nbytes
        nbytes = at + chunks.nbytes
        if pinned is None or pinned.numel() < nbytes:
            pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.pinned = pinned
        host = pinned.numpy()
        host[:at].view(TENSOR_DT)[:] = rows
        host[at:nbytes].view(CHUNK_DT)[:] = chunks
        self.dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.dev.copy_(pinned[:nbytes], non_blocking=True)      # on the current stream; recorded when that stream is capturing
        self.partials = torch.empty(self.n_chunks, dtype=torch.float64, device=device)
        self.tensors_ptr = self.dev.data_ptr()
        self.chunks_ptr = self.tensors_ptr + at


def _table_bytes(numels):
    return sum(TENSOR_DT.itemsize + CHUNK_DT.itemsize * (-(-int(n) // CHUNK)) for n in numels)


class ClipAdamW(torch.optim.Optimizer):
    """``clip_grad_norm_(params, max_norm)`` + ``torch.optim.AdamW.step()`` (+ the EMA of an attached :class:`ModelEma`) as two kernel
    launches and no host synchronisation; ``total_norm`` (a device tensor) is the gradient norm of the last step.

    Takes torch's parameter-group dicts; ``max_norm <= 0`` means no clipping (the reference's ``if max_norm > 0``).  ``step`` is kept per
    parameter as torch keeps it: a parameter whose ``.grad`` is None is left out of the norm and untouched, and its step does not advance.
    ``state_dict()`` has torch.optim.AdamW's layout (``exp_avg``, ``exp_avg_sq``, ``step``; the group keys of ``AdamW(fused=True)``), so a
    checkpoint moves between the two in both directions.

    DIFFERENCE from ``clip_grad_norm_``: ``p.grad`` is read, never written.  The clipped gradient exists only in registers; after
    ``step()`` the gradients still hold what backward left there.

    Under ``torch.cuda.graph``: call :meth:`init_state` (or take one eager step) first; the capture records the upload of a table built for
    the gradients of that capture and the two kernels.  Hyper-parameters are read from device memory: outside a capture ``step()`` uploads
    them when ``param_groups``, ``max_norm`` or the EMA settings differ from what was last uploaded; before a replay call :meth:`sync`.
    float32, contiguous parameters only; no ``amsgrad``, no ``maximize``."""

    _SPARES = 4      # pinned buffers kept for tables built during a capture (pinned memory is not allocated while capturing)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, amsgrad=False, maximize=False):
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= weight_decay or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid hyper-parameters: lr={lr} betas={betas} eps={eps} weight_decay={weight_decay}")
        self.max_norm = float(max_norm)
        self.ema_on = False
        self._ema = None
        self._repack = None
        self._table = self._table_sig = None
        self._captured = []          # tables built during a capture: alive (and unchanged) as long as the optimizer
        self._spare = []
        self._hyper = self._hyper_key = None
        self._state_complete = False
        self._static = self._static_epoch = None
        self._epoch = 0              # bumped by whatever changes a pointer the table holds without changing (param, grad)
        self.total_norm = None
        # the group keys of torch.optim.AdamW(fused=True): a state_dict loads into it unchanged
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=True, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # ---- construction -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group):
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("ClipAdamW: amsgrad and maximize are not supported")
        if group.get("decoupled_weight_decay") is False:
            raise ValueError("ClipAdamW: decoupled weight decay only (an Adam checkpoint with L2 decay is another optimizer)")
        for p in group["params"]:
            _check_tensor(p, "ClipAdamW parameter")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._check_group(self.param_groups[-1])
        self._state_complete = False
        self._epoch = getattr(self, "_epoch", 0) + 1

    def init_state(self):
        """allocate ``exp_avg`` / ``exp_avg_sq`` / ``step`` of every parameter that has none yet (not while capturing: state lives
        outside any graph's memory pool)"""
        missing = [p for g in self.param_groups for p in g["params"] if len(self.state.get(p, ())) == 0]
        if missing:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ClipAdamW: optimizer state cannot be created inside a graph capture; call init_state() before it")
            steps = torch.zeros(len(missing), dtype=torch.float32, device=missing[0].device)
            for i, p in enumerate(missing):
                self.state[p] = {"step": steps[i] if p.device == steps.device else torch.zeros((), dtype=torch.float32, device=p.device),
                                 "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                                 "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
            self._epoch += 1
        self._state_complete = True

    def load_state_dict(self, state_dict):
        """torch's AdamW layout (torch.optim.AdamW checkpoints load unchanged)"""
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            self._check_group(g)
            for p in g["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                if "max_exp_avg_sq" in st:
                    raise ValueError("ClipAdamW: the checkpoint carries amsgrad state")
                step = st["step"] if torch.is_tensor(st["step"]) else torch.tensor(float(st["step"]))
                st["step"] = step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone()
                for k in ("exp_avg", "exp_avg_sq"):
                    st[k] = st[k].detach().to(device=p.device, dtype=torch.float32).contiguous()
        self._state_complete = False
        self._epoch += 1
        self._hyper_key = None

    def attach_ema(self, ema):
        """fold the update of ``ema``'s shadows of this optimizer's parameters into the step kernel (active while ``ema_on``); ``ema.update``
        then covers only the rest of the model's state"""
        self._ema = ema
        ema._opt = self
        self._epoch += 1
        self._hyper_key = None

    def attach_repack(self, plan):
        """end every ``step()`` -- eager or captured -- with ``plan.refresh()`` (richsem_amd/repack.py): the derived forms of the
        parameters follow the masters in one more launch on the same stream; ``None`` detaches"""
        self._repack = plan

    def folded(self):
        """ids of the parameters whose shadows the last ``step()`` updated"""
        if self._ema is None or not self.ema_on or self._table_sig is None:
            return frozenset()
        return self._folded

    # ---- tables -----------------------------------------------------------------------------------------------------------------
    def _device(self):
        return self.param_groups[0]["params"][0].device

    def _refill_spares(self):
        if len(self._spare) < self._SPARES:
            nbytes = _table_bytes([p.numel() for g in self.param_groups for p in g["params"]])
            while len(self._spare) < self._SPARES:
                self._spare.append(torch.empty(nbytes, dtype=torch.uint8, pin_memory=True))

    def _current_table(self, capturing):
        live, sig = [], [self._epoch, capturing]
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                grad = p.grad
                if grad is not None:
                    live.append((p, grad, gi))
                    sig.append(p.data_ptr())
                    sig.append(grad.data_ptr())
        if not live:
            return None
        if not capturing and sig == self._table_sig:
            return self._table
        dev = live[0][0].device
        if dev.type != "cuda":
            raise RuntimeError("richsem_amd.optim.ClipAdamW: parameters must be on the GPU (no CPU implementation)")
        if self._static_epoch != self._epoch:
            # what a rebuild for new gradients does not change: state, shadow, size and group of every parameter
            shadow = self._ema.shadow_of if self._ema is not None else (lambda p: None)
            self._static = {}
            for gi, g in enumerate(self.param_groups):
                for p in g["params"]:
                    st, e = self.state[p], shadow(p)
                    if e is not None:
                        _check_tensor(e, "EMA shadow")
                    self._static[id(p)] = (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), 0 if e is None else e.data_ptr(),
                                           st["step"].data_ptr(), p.numel(), gi)
            self._static_epoch = self._epoch
        for p, grad, _ in live:
            if grad.dtype != torch.float32 or not grad.is_contiguous() or grad.is_sparse or grad.device != dev or p.device != dev:
                raise ValueError(f"ClipAdamW: gradient of a {tuple(p.shape)} parameter must be dense contiguous float32 on {dev} "
                                 f"(got {grad.dtype}, strides {grad.stride()}, {grad.device})")
        rows = np.zeros(len(live), dtype=TENSOR_DT)
        rows["param"], rows["grad"] = sig[2::2], sig[3::2]
        static = [self._static[id(p)] for p, _, _ in live]
        for k, name in enumerate(("exp_avg", "exp_avg_sq", "ema", "step", "numel", "group")):
            rows[name] = [t[k] for t in static]
        numels = rows["numel"]
        if capturing:
            # a table of the capture's own: its pinned host copy is never rewritten and feeds a device buffer nothing else writes
            table = _Table(rows, numels, dev, self._spare.pop() if self._spare else None)
            self._captured.append(table)
        else:
            table = _Table(rows, numels, dev)
        self._table, self._table_sig = table, sig
        self._folded = frozenset(id(p) for (p, _, _), t in zip(live, static) if t[2])
        return table

    # ---- hyper-parameters -------------------------------------------------------------------------------------------------------
    def _hyper_now(self):
        return (self.max_norm, float(self._ema.decay) if self._ema is not None else 0.0, bool(self.ema_on and self._ema is not None),
                tuple((float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
                      for g in self.param_groups))

    def sync(self):
        """upload the group table and the settings (lr, betas, eps, weight_decay per group; max_norm, ema_decay, ema_on) on the current
        stream.  Outside a capture ``step()`` does this itself when something changed; call it before replaying a captured step."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ClipAdamW.sync(): not inside a graph capture (the upload would be replayed with stale values)")
        self._refill_spares()
        key = self._hyper_now()
        n = len(key[3])
        nbytes = _GROUPS_AT + n * GROUP_DT.itemsize
        if self._hyper is None or self._hyper.numel() != nbytes:
            self._hyper = torch.empty(nbytes, dtype=torch.uint8, device=self._device())
            self.total_norm = torch.zeros((), dtype=torch.float32, device=self._device())
        pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)      # a fresh one per upload: the last may still be in flight
        host = pinned.numpy()
        host[:] = 0
        host[: SETTINGS_DT.itemsize].view(SETTINGS_DT)[0] = (key[0], key[1], int(key[2]), 0)
        host[_GROUPS_AT:].view(GROUP_DT)[:] = np.array(key[3], dtype=np.float64).view(GROUP_DT).reshape(n)
        self._hyper.copy_(pinned, non_blocking=True)
        self._hyper_key = key

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        if not self._state_complete:
            self.init_state()
        if capturing:
            if self._hyper_key is None:
                raise RuntimeError("ClipAdamW: call sync() (or take one eager step) before capturing a step")
        else:
            if len(self._spare) < self._SPARES:
                self._refill_spares()
            if self._hyper_key != self._hyper_now():
                self.sync()
        table = self._current_table(capturing)
        if table is None:      # no parameter has a gradient: nothing moves, the norm of nothing is 0
            if self.total_norm is not None:
                self.total_norm.zero_()
            return loss
        dev = table.dev.device
        L = _lib.load()
        with _lib.on_device(dev):
            stream = _lib.raw_stream(dev)
            hyper = self._hyper.data_ptr()
            _lib.check(L.msda_optim_sumsq(table.tensors_ptr, table.chunks_ptr, table.n_chunks, table.partials.data_ptr(), stream))
            _lib.check(L.msda_optim_step(table.tensors_ptr, table.chunks_ptr, table.n_chunks, table.partials.data_ptr(), hyper + _GROUPS_AT,
                                         hyper, self.total_norm.data_ptr(), stream))
        if self._repack is not None:      # (the step hook records what the forms were refreshed from, once it has bumped the versions)
            self._repack.refresh(_snapshot=False)
            self._repack._stepped = True
        return loss


class ModelEma(torch.nn.Module):
    """The reference's ``ModelEma`` (util/utils.py:375-400): ``.module`` is an eval deep copy of the model, ``update(model)`` moves every
    entry of its ``state_dict`` towards the model's (``e = decay * e + (1 - decay) * m``), ``set(model)`` copies.  float32 entries are
    updated by one kernel launch over a device table (``msda_optim_ema``); the handful of integer entries (``num_batches_tracked``) take
    the reference's expression.  Attached to a :class:`ClipAdamW` (``opt.attach_ema(ema)``), the trained parameters' shadows are updated
    inside the optimizer's step kernel while ``opt.ema_on`` and ``update`` covers only the remaining state."""

    def __init__(self, model, decay=0.9997):
        super().__init__()
        self.module = deepcopy(model)
        self.module.eval()
        self.decay = decay
        self._opt = None
        self._shadow = {id(p): e for p, e in zip(model.parameters(), self.module.parameters())}
        self._params = list(model.parameters())      # (keeps the ids above valid)
        self._table = self._table_sig = None
        self._settings = self._settings_decay = None

    def shadow_of(self, p):
        e = self._shadow.get(id(p))
        return None if e is None else e.data

    @torch.no_grad()
    def set(self, model):
        for e, m in zip(self.module.state_dict().values(), model.state_dict().values()):
            e.copy_(m)

    @torch.no_grad()
    def update(self, model):
        folded = self._opt.folded() if self._opt is not None else frozenset()
        folded_ptrs = {p.data_ptr() for p in self._params if id(p) in folded}
        pairs = []
        for (name, e), m in zip(self.module.state_dict().items(), model.state_dict().values()):
            if m.data_ptr() in folded_ptrs and m.dtype == torch.float32:
                continue
            if not e.dtype.is_floating_point:
                e.copy_(self.decay * e + (1.0 - self.decay) * m)      # the reference's expression (integer counters)
                continue
            _check_tensor(e, f"EMA entry {name}")
            _check_tensor(m, f"model entry {name}")
            if not (e.is_cuda and m.device == e.device):
                raise RuntimeError("richsem_amd.optim.ModelEma: the model and its copy must be on one GPU (no CPU implementation)")
            if e.numel():
                pairs.append((e, m))
        if not pairs:
            return
        dev = pairs[0][0].device
        capturing = torch.cuda.is_current_stream_capturing()
        if self._settings_decay != float(self.decay):
            if capturing:
                raise RuntimeError("ModelEma: call update() once eagerly (or keep decay unchanged) before capturing it")
            if self._settings is None:
                self._settings = torch.empty(SETTINGS_DT.itemsize, dtype=torch.uint8, device=dev)
            pinned = torch.empty(SETTINGS_DT.itemsize, dtype=torch.uint8, pin_memory=True)
            pinned.numpy().view(SETTINGS_DT)[0] = (0.0, float(self.decay), 1, 0)
            self._settings.copy_(pinned, non_blocking=True)
            self._settings_decay = float(self.decay)
        sig = [x for e, m in pairs for x in (e.data_ptr(), m.data_ptr())]
        if sig != self._table_sig:
            if capturing:
                raise RuntimeError("ModelEma: call update() once eagerly before capturing it (its table is built outside a capture)")
            rows = np.zeros(len(pairs), dtype=TENSOR_DT)
            for i, (e, m) in enumerate(pairs):
                rows[i] = (m.data_ptr(), 0, 0, 0, e.data_ptr(), 0, e.numel(), 0, 0)
            self._table, self._table_sig = _Table(rows, rows["numel"], dev), sig
        t = self._table
        with _lib.on_device(dev):
            _lib.check(_lib.load().msda_optim_ema(t.tensors_ptr, t.chunks_ptr, t.n_chunks, self._settings.data_ptr(), _lib.raw_stream(dev)))


def _match(name, keywords):
    return any(k in name for k in keywords)


def param_groups(model, lr, lr_backbone, weight_decay, param_dict_type="default", lr_backbone_names=("backbone.0",),
                 lr_linear_proj_names=("reference_points", "sampling_offsets"), lr_linear_proj_mult=0.1):
    """The parameter groups of the reference's util/get_param_dicts.py:23-84 (substring matching on the parameter names, trained parameters
    only), as torch param-group dicts:

    ``default``         everything without "backbone" in its name; the rest at ``lr_backbone``
    ``ddetr_in_mmdet``  neither list / ``lr_backbone_names`` at ``lr_backbone`` / ``lr_linear_proj_names`` at ``lr * lr_linear_proj_mult``
                        (a name on both lists lands in both groups, as in the reference: torch's optimizers refuse that)
    ``large_wd``        "backbone" x ("norm" or "bias"): no weight decay on norms and biases, ``lr_backbone`` on the backbone"""
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    if param_dict_type == "default":
        return [{"params": [p for n, p in named if "backbone" not in n]},
                {"params": [p for n, p in named if "backbone" in n], "lr": lr_backbone}]
    if param_dict_type == "ddetr_in_mmdet":
        bb, lp = list(lr_backbone_names), list(lr_linear_proj_names)
        return [{"params": [p for n, p in named if not _match(n, bb) and not _match(n, lp)], "lr": lr},
                {"params": [p for n, p in named if _match(n, bb)], "lr": lr_backbone},
                {"params": [p for n, p in named if _match(n, lp)], "lr": lr * lr_linear_proj_mult}]
    if param_dict_type == "large_wd":
        bb, nb = ["backbone"], ["norm", "bias"]
        return [{"params": [p for n, p in named if not _match(n, bb) and not _match(n, nb)]},
                {"params": [p for n, p in named if _match(n, bb) and _match(n, nb)], "lr": lr_backbone, "weight_decay": 0.0},
                {"params": [p for n, p in named if _match(n, bb) and not _match(n, nb)], "lr": lr_backbone, "weight_decay": weight_decay},
                {"params": [p for n, p in named if not _match(n, bb) and _match(n, nb)], "lr": lr, "weight_decay": 0.0}]
    raise ValueError(f"param_dict_type must be 'default', 'ddetr_in_mmdet' or 'large_wd' (got {param_dict_type!r})")
