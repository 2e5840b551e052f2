"""The batch-geometry tensors: everything the reference derives from the padding mask at the start of each forward -- the per-level masks
(``F.interpolate`` of the image mask, models/richsem/richsem.py:593-612), ``get_valid_ratio`` (deformable_transformer.py:253-260), the encoder's
reference points (:513-525), ``PositionEmbeddingSineHW`` (position_encoding.py:46-92, normalised) and the geometry half of
``gen_encoder_output_proposals`` (utils.py:10-65: anchors, ``+inf`` fill, the mask of zeroed memory rows).

Every padding mask the reference builds (``nested_tensor_from_tensor_list``) is a bottom / right rectangle, so all of these are closed forms
of the ``(N, 2)`` image sizes and the canvas.  Here they come from ONE kernel (csrc/msda_geometry.h, ``msda_batch_geometry_f32``) that reads
the sizes on the device: no host synchronisation, no allocation when ``out`` is given, so the call can be captured into a graph and a replay
follows the current contents of the ``sizes`` tensor -- a captured training step no longer freezes the geometry of the batch it was captured on.
"""
import ctypes

import torch

from . import _lib
from . import workload as W

OUTPUTS = ("pos_sine", "ref", "proposals")


def sizes_from_targets(targets, device):
    """the reference's ``target["size"]`` (h, w) of every image -> ``(N, 2)`` int32 on ``device`` (one host -> device copy: not for a captured
    region -- copy into the static tensor outside it: ``static.copy_(sizes_from_targets(...))``)"""
    rows = [[int(v) for v in torch.as_tensor(t["size"]).reshape(-1).tolist()] for t in targets]
    if not rows or any(len(r) != 2 for r in rows):
        raise ValueError("sizes_from_targets: every target needs size = (h, w)")
    return torch.tensor(rows, dtype=torch.int32).to(device)


def _buffers(N, S, L, C, want, dev):
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"mask_flat": torch.empty((N, S), dtype=torch.bool, device=dev), "valid_ratios": torch.empty((N, L, 2), **f32),
           "ref": None, "pos_sine": None, "proposals": None, "zeroed": None}
    if "ref" in want:
        out["ref"] = torch.empty((N, S, L, 2), **f32)
    if "pos_sine" in want:
        out["pos_sine"] = torch.empty((N, S, C), **f32)
    if "proposals" in want:
        out["proposals"], out["zeroed"] = torch.empty((N, S, 4), **f32), torch.empty((N, S, 1), dtype=torch.bool, device=dev)
    return out


def batch_geometry(sizes, canvas, shapes=None, num_pos_feats=128, temperature=(20.0, 20.0), want=OUTPUTS, out=None):
    """``sizes`` (N, 2) int32 on the GPU -- (h, w) of every image, clamped on the device to ``[1, canvas]`` --, ``canvas`` = (H, W) of the padded
    batch, ``shapes`` = [(h_l, w_l)] of the pyramid's levels (default ``workload.pyramid_shapes(*canvas)``) -> the dict ``Step.prepare`` builds:

        shapes, spatial (L, 2) int64, lsi (L) int64, masks [(N, h_l, w_l) bool views of mask_flat], mask_flat (N, S) bool,
        valid_ratios (N, L, 2), ref (N, S, L, 2), pos_sine (N, S, 2 * num_pos_feats), proposals (N, S, 4), zeroed (N, S, 1) bool

    ``temperature`` = (temperatureH, temperatureW); ``want``: which of "pos_sine", "ref", "proposals" (with ``zeroed``) to compute -- the others
    are None.  ``out``: a previous result whose buffers are written again (the static outputs of a graph; its ``shapes``, ``N`` and ``want`` must
    be this call's): with it the call allocates nothing.  CPU tensors raise: there is no CPU fallback."""
    if not torch.is_tensor(sizes) or not sizes.is_cuda:
        raise RuntimeError("Not implemented on the CPU")
    if sizes.dtype != torch.int32 or sizes.dim() != 2 or sizes.shape[1] != 2 or not sizes.is_contiguous():
        raise TypeError("batch_geometry: sizes is a contiguous (N, 2) int32 tensor of (h, w)")
    unknown = [k for k in want if k not in OUTPUTS]
    if unknown:
        raise ValueError(f"batch_geometry: want {unknown}: any of {OUTPUTS}")
    H, Wd = int(canvas[0]), int(canvas[1])
    shapes = [(int(h), int(w)) for h, w in (W.pyramid_shapes(H, Wd) if shapes is None else shapes)]
    N, L, C, dev = sizes.shape[0], len(shapes), 2 * int(num_pos_feats), sizes.device
    S = sum(h * w for h, w in shapes)
    t_h, t_w = (float(temperature), float(temperature)) if isinstance(temperature, (int, float)) else (float(temperature[0]), float(temperature[1]))
    if out is None:
        spatial = torch.tensor(shapes, dtype=torch.int64).reshape(L, 2)
        lsi = torch.cat((spatial.new_zeros(1), spatial.prod(1).cumsum(0)[:-1]))
        out = {"shapes": shapes, "spatial": spatial.to(dev), "lsi": lsi.to(dev), **_buffers(N, S, L, C, want, dev)}
        cur = 0
        out["masks"] = []
        for h, w in shapes:
            out["masks"].append(out["mask_flat"][:, cur:cur + h * w].view(N, h, w))
            cur += h * w
    else:
        have = tuple(k for k in OUTPUTS if out.get(k) is not None)
        if out["shapes"] != shapes or tuple(out["mask_flat"].shape) != (N, S) or set(have) != set(want) or out["mask_flat"].device != dev or \
                (out["pos_sine"] is not None and out["pos_sine"].shape[-1] != C):
            raise ValueError("batch_geometry: `out` was made for other shapes, another batch size, device or set of outputs")
    host_shapes = (ctypes.c_int32 * (2 * L))(*[v for hw in shapes for v in hw])
    ptr = lambda k: None if out[k] is None else out[k].data_ptr()
    with _lib.on_device(dev):
        _lib.check(_lib.load().msda_batch_geometry_f32(sizes.data_ptr(), N, H, Wd, host_shapes, L, int(num_pos_feats), t_h, t_w, ptr("mask_flat"),
                                                       ptr("valid_ratios"), ptr("ref"), ptr("pos_sine"), ptr("proposals"), ptr("zeroed"),
                                                       _lib.raw_stream(dev)))
    return out
