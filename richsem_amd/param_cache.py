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
"""
import torch
from torch.optim.optimizer import register_optimizer_step_post_hook


def _bump_versions(opt, args, kwargs):
    torch.autograd.graph.increment_version([p for g in opt.param_groups for p in g["params"] if p.grad is not None])


_STEP_HOOK = register_optimizer_step_post_hook(_bump_versions)


def capturing(t):
    """True when ``t`` is a GPU tensor and the current stream is capturing a graph (rule 2 above)"""
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


class VersionCache:
    """A derived form of a few parameters (bf16 casts, packed weights, stacked projections) kept across calls and rebuilt when one of
    them has been modified in place: any optimizer step (fused ones included, through this module's step hook), ``load_state_dict``,
    ``copy_`` -- whatever bumps autograd's version counter.  Writes THROUGH ``param.data`` bypass that counter: call :meth:`clear` after
    them.  During a graph capture :meth:`get` builds and returns a fresh value and keeps nothing (module docstring, rule 2)."""

    def __init__(self):
        self._ver = self._val = None

    def clear(self):
        self._ver = self._val = None

    def get(self, params, build):
        if capturing(params[0]):
            with torch.no_grad():
                return build()
        ver = tuple((p.data_ptr(), p._version) for p in params)
        if ver != self._ver:
            with torch.no_grad():
                self._val = build()
            self._ver = ver
        return self._val
