"""The all-negative focal term's library calls: the one Python call site of ``msda_focal_neg_sum_f32`` / ``msda_focal_neg_grad_f32`` and of
their masked forms (csrc/rows_api.hip, csrc/msda_fed.h).  ``matcher.FocalNegativeSum``, ``fed_loss.MaskedFocalNegativeSum`` and the capacity
criterion (criterion.py) all go through :func:`neg_sum` and :func:`neg_grad`.  ``row_group`` (rows) int32 and ``class_mask`` (G, C) float32
are given together or not at all: with them row r counts class c only where ``class_mask[row_group[r], c] != 0``.  Arguments are checked,
contiguous device tensors; the caller has made their device current (``_lib.on_device``).
"""
import ctypes

import torch

from . import _lib

NEG_PARTIALS = 4096      # the size of the partial buffer: the sum kernel's grid cap (csrc/rows_api.hip)


def neg_sum(x, w, alpha, row_group=None, class_mask=None):
    """``x`` (..., C), ``w`` (...) float32 -> the float64 per-workgroup partials of ``sum_rows w[row] sum_c (1 - alpha) p^2 softplus(x)``; the
    caller adds them up"""
    partial = torch.empty(NEG_PARTIALS, dtype=torch.float64, device=x.device)
    n = ctypes.c_int(0)
    if class_mask is None:
        _lib.check(_lib.load().msda_focal_neg_sum_f32(x.data_ptr(), w.data_ptr(), w.numel(), x.shape[-1], alpha, partial.data_ptr(), NEG_PARTIALS,
                                                      ctypes.byref(n), _lib.raw_stream(x.device)))
    else:
        _lib.check(_lib.load().msda_focal_neg_sum_masked_f32(x.data_ptr(), w.data_ptr(), row_group.data_ptr(), class_mask.data_ptr(),
                                                             class_mask.shape[0], w.numel(), x.shape[-1], alpha, partial.data_ptr(), NEG_PARTIALS,
                                                             ctypes.byref(n), _lib.raw_stream(x.device)))
    return partial[:n.value]


def neg_grad(x, w, alpha, gs, row_group=None, class_mask=None):
    """-> ``gs[0]`` * d / dx of that sum, shaped as ``x``: every element written, exact zeros off the mask and in rows that count nothing"""
    gx = torch.empty_like(x)
    if class_mask is None:
        _lib.check(_lib.load().msda_focal_neg_grad_f32(x.data_ptr(), w.data_ptr(), w.numel(), x.shape[-1], alpha, gs.data_ptr(), gx.data_ptr(),
                                                       _lib.raw_stream(x.device)))
    else:
        _lib.check(_lib.load().msda_focal_neg_grad_masked_f32(x.data_ptr(), w.data_ptr(), row_group.data_ptr(), class_mask.data_ptr(),
                                                              class_mask.shape[0], w.numel(), x.shape[-1], alpha, gs.data_ptr(), gx.data_ptr(),
                                                              _lib.raw_stream(x.device)))
    return gx
