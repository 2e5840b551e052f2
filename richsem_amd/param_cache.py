"""Derived forms of parameters kept across calls (bf16 casts, packed weights, folded affines) and the two rules that keep them fresh.

1. Every cache is keyed on ``(p.data_ptr(), p._version)`` of the parameters it derives from.  Autograd's version counter sees in-place
   ops (``copy_``, ``load_state_dict``, foreach / for-loop optimizers) but NOT the fused optimizers: ``aten::_fused_adamw_`` and its
   siblings write the parameters without bumping it.  So this module registers, at import, a global optimizer step post-hook that bumps
   the version of every parameter an optimizer step may have written (the ones with a gradient): any ``torch.optim.Optimizer``, fused or
   not, invalidates the caches built from the parameters it updates.  Writes THROUGH ``param.data`` are still invisible: call the
   owner's ``clear()`` / ``invalidate_bf16_cache()`` after them.
2. While the current stream is capturing a graph, a cache BUILDS its value on every call and does not keep it: the build kernels are then
   recorded into the graph and re-run on every replay (after an optimizer step they read the new masters), and nothing kept outside the
   graph points into the graph's private memory pool.  The builders launch on the current stream and make no host synchronisation.

A cache BOUND to a :class:`richsem_amd.repack.RepackPlan` follows neither rule by itself: its forms are the plan's persistent buffers, which
one launch of the plan refreshes together with every other bound cache's (repack.py).  Nothing here changes for a cache that is not bound.
"""
import copy

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook


def _bump_versions(opt, args, kwargs):
    torch.autograd.graph.increment_version([p for g in opt.param_groups for p in g["params"] if p.grad is not None])
    plan = getattr(opt, "_repack", None)
    if plan is not None:      # (a ClipAdamW whose step ended with the plan's refresh: the forms are as new as the bumped versions)
        plan._after_step()


_STEP_HOOK = register_optimizer_step_post_hook(_bump_versions)


def capturing(t):
    """True when ``t`` is a GPU tensor and the current stream is capturing a graph (rule 2 above)"""
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def stream_capturing():
    """True when the current stream is capturing a graph (False, without touching the runtime, in a process that has not used the GPU)"""
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


# ---- what a recording RepackPlan hears from the builders -------------------------------------------------------------------------------
_RECORDING = None      # the RepackPlan inside ``with plan.record():``, or None
UNBOUND = object()     # what a binding answers when its parameters are no longer the tensors it was recorded with


def recording():
    return _RECORDING


def note(kind, dst, segments, scale=None):
    """(the builders) ``dst`` is the form ``kind`` of the fp32 ``segments`` (concatenated along the output dimension): one job of the
    recording plan.  ``kind``: "cast", "copy", "lin256", "lin256_t", "ffn_w2", "conv", "conv_t" (include/richsem_msda.h: msda_repack_kind).
    Nothing unless a plan is recording."""
    if _RECORDING is not None:
        _RECORDING._note(kind, dst, segments, scale)


def cast_bf16(*tensors):
    """the bf16 cast of the row concatenation of ``tensors``: ``cat(tensors).detach().to(torch.bfloat16).contiguous()``"""
    t = tensors[0] if len(tensors) == 1 else torch.cat(tensors, 0)
    out = t.detach().to(torch.bfloat16).contiguous()
    if _RECORDING is not None:
        note("cast", out, tensors)
    return out


class VersionCache:
    """A derived form of a few parameters (bf16 casts, packed weights, stacked projections) kept across calls and rebuilt when one of
    them has been modified in place: any optimizer step (fused ones included, through this module's step hook), ``load_state_dict``,
    ``copy_`` -- whatever bumps autograd's version counter.  Writes THROUGH ``param.data`` bypass that counter: call :meth:`clear` after
    them.  During a graph capture :meth:`get` builds and returns a fresh value and keeps nothing (module docstring, rule 2).

    Bound to a RepackPlan (repack.py) the value is the plan's: a version mismatch refreshes the whole plan in one launch instead of
    calling ``build``, and a capture returns the plan's buffers and launches nothing.  A ``copy.deepcopy`` of a bound cache is unbound."""

    _binding = None

    def __init__(self):
        self._ver = self._val = None

    def clear(self):
        self._ver = self._val = None
        if self._binding is not None:
            self._binding.ver = None

    def __deepcopy__(self, memo):
        if self._binding is not None:
            return type(self)()
        new = type(self).__new__(type(self))
        memo[id(self)] = new
        new.__dict__.update(copy.deepcopy(self.__dict__, memo))
        return new

    def get(self, params, build):
        if self._binding is not None:
            val = self._binding.get(params)
            if val is not UNBOUND:
                return val
            self._binding = None      # (the parameters moved: back to this cache's own behaviour)
        elif _RECORDING is not None and not capturing(params[0]) and not _RECORDING.declined(self, None):
            val, self._binding = _RECORDING._record(self, None, params, build)
            if self._binding is None:
                self._val, self._ver = val, tuple((p.data_ptr(), p._version) for p in params)
            return val
        if capturing(params[0]):
            with torch.no_grad():
                return build()
        ver = tuple((p.data_ptr(), p._version) for p in params)
        if ver != self._ver:
            with torch.no_grad():
                self._val = build()
            self._ver = ver
        return self._val
