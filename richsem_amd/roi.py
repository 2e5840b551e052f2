"""ROIAlign forward on the GPU: drop-in for the reference's
``detectron2.layers.roi_align.ROIAlign(output_size, spatial_scale, sampling_ratio, aligned).forward(input, rois)``
(models/richsem/richsem.py:25, :878) -- detectron2 is not needed.  Kernel richsem_amd/csrc/msda_roi.h, C ABI
``msda_roi_align_forward_{f32,f64}``.  Forward only (RichSem pools the frozen CLIP feature map).
:func:`roi_align_targets` pools the target boxes of a capacity buffer instead of a roi list (csrc/msda_roi_targets.h)."""
import torch

from . import _lib


class ROIAlign:
    def __init__(self, output_size, spatial_scale, sampling_ratio, aligned=True):
        self.output_size = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
        self.spatial_scale, self.sampling_ratio, self.aligned = float(spatial_scale), int(sampling_ratio), bool(aligned)

    def forward(self, input, rois):
        """input (N, C, H, W); rois (K, 5) = (batch index, x1, y1, x2, y2) -> (K, C, output_h, output_w)"""
        if not input.is_cuda:
            raise RuntimeError("Not implemented on the CPU")
        assert rois.dim() == 2 and rois.size(1) == 5
        dt = input.dtype
        if dt not in (torch.float32, torch.float64):
            raise RuntimeError(f"ROIAlign: float32 / float64 input, got {dt}")
        x, r = input.contiguous(), rois.to(dt).contiguous()
        N, C, H, W = x.shape
        ph, pw = self.output_size
        out = torch.empty((r.shape[0], C, ph, pw), dtype=dt, device=x.device)
        if r.shape[0] == 0:
            return out
        fn = getattr(_lib.load(), "msda_roi_align_forward_" + ("f32" if dt == torch.float32 else "f64"))
        with _lib.on_device(x.device):
            _lib.check(fn(x.data_ptr(), r.data_ptr(), r.shape[0], N, C, H, W, ph, pw, self.spatial_scale, self.sampling_ratio,
                          int(self.aligned), out.data_ptr(), _lib.raw_stream(x.device)))
        return out

    __call__ = forward


def roi_align(input, rois, output_size, spatial_scale=1.0, sampling_ratio=0, aligned=True):
    return ROIAlign(output_size, spatial_scale, sampling_ratio, aligned).forward(input, rois)


def roi_align_targets(input, targets, sizes, output_size, spatial_scale, sampling_ratio=0, return_status=False):
    """ROIAlign (aligned) of the TARGET boxes over capacity buffers (``msda_roi_align_targets_f32``, csrc/msda_roi_targets.h).

    ``input`` (N, C, H, W) float32; ``targets``: a ``matcher.TargetBuffers`` (or a ``CostPlan``: the exact-size case) -- its ``offsets_dev``
    and normalised cxcywh ``tgt_boxes`` are read on the device; ``sizes`` (N, 2) int32 (h, w) on the device, as
    ``geometry.sizes_from_targets`` makes it.  -> (targets.total, C, output_h, output_w) float32: slot t < offsets_dev[-1] holds what
    ``ROIAlign(output_size, spatial_scale, sampling_ratio, True)`` gives for the pixel box ``clip_box_targets`` forms of target t, every
    other slot exact zeros.  ``return_status``: also the int32[4] status (word 3: a prefix that does not describe targets inside the
    capacity; everything is zeros then).  One launch, no host synchronisation, no shape that depends on the counts: capturable."""
    if input.dtype != torch.float32 or targets.tgt_boxes.dtype != torch.float32:
        raise TypeError("roi_align_targets: the feature map and the target boxes are float32 tensors")
    if sizes.dtype != torch.int32 or targets.offsets_dev.dtype != torch.int64:
        raise TypeError("roi_align_targets: sizes is an int32 tensor (geometry.sizes_from_targets), the target prefix int64")
    if not all(t.is_cuda for t in (input, sizes, targets.offsets_dev, targets.tgt_boxes)):
        raise RuntimeError("Not implemented on the CPU")
    cap = int(targets.total)
    if input.dim() != 4 or cap < 1:
        raise ValueError("roi_align_targets: input is (N, C, H, W), the target capacity >= 1")
    N, C, H, W = input.shape
    if tuple(sizes.shape) != (N, 2) or targets.offsets_dev.numel() != N + 1 or tuple(targets.tgt_boxes.shape) != (cap, 4):
        raise ValueError("roi_align_targets: sizes is (N, 2), the target buffers hold N + 1 offsets and (capacity, 4) boxes")
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    x, s, boxes = input.contiguous(), sizes.contiguous(), targets.tgt_boxes.contiguous()
    out = torch.empty((cap, C, ph, pw), dtype=torch.float32, device=x.device)
    status = torch.empty(4, dtype=torch.int32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.load().msda_roi_align_targets_f32(x.data_ptr(), targets.offsets_dev.data_ptr(), boxes.data_ptr(), s.data_ptr(), N, C, H, W,
                                                          cap, ph, pw, float(spatial_scale), int(sampling_ratio), out.data_ptr(),
                                                          status.data_ptr(), _lib.raw_stream(x.device)))
    return (out, status) if return_status else out
