"""GPU (-m gpu): ROIAlign of the target boxes over capacity buffers (``msda_roi_align_targets_f32``, csrc/msda_roi_targets.h; richsem_amd/roi.py
``roi_align_targets``) against oracle/roi_oracle.py in float64, element by element.

Reference: the rois are formed in float64 from the same float32 boxes and int sizes -- (b, w_b (cx - w / 2), h_b (cy - h / 2), w_b (cx + w / 2),
h_b (cy + h / 2)) -- and pooled by the oracle in float64.

Bound, per element, with M = max |input| over that image and channel and G = the largest sampling grid per axis:

    |got - want| <= (64 max(H, W) + G^2 + 16) 2^-24 M

Derivation.  A sample position is start + ph * bin + (i + 0.5) * bin / grid with start = box * scale - 0.5 and the box made by three float32
operations: at most 12 roundings on quantities of magnitude <= max(H, W) (the positions lie inside (-1, H) x (-1, W)), so a position is off
by at most 12 * 2^-24 * max(H, W) per axis.  Bilinear interpolation of values bounded by M is 2 M-Lipschitz per axis (the weight of a corner
moves by the displacement, two corners gain what two lose; the clamping at the borders is continuous), so a sample is off by at most
2 * 2 M * 12 * 2^-24 max(H, W) = 48 max(H, W) 2^-24 M from its position; 64 leaves a quarter for the products that form the position being
rounded where this reasoning took them exact.  The interpolation itself is 4 products of 3 factors and 3 additions on values <= M: below
16 * 2^-24 M.  The mean adds G^2 samples: each addition rounds a partial sum of magnitude <= G^2 M / G^2 after the division, G^2 * 2^-24 M in
all, and the division one more.  An excess over this bound is a bug in the kernel or in the derivation, not a reason to widen it.

Conditions (asserted in float64 on the test's own boxes; they keep the comparison away from the two places where the operator is
discontinuous): every roi_h / PH and roi_w / PW is at least 1e-3 from an integer (the adaptive grid is a ceil of it), and every sample lies
at least 1e-3 inside (-1, H) x (-1, W) (outside, a sample counts 0).
"""
import math

import numpy as np
import pytest
import torch

from oracle import roi_oracle
from richsem_amd.matcher import TargetBuffers
from richsem_amd.roi import roi_align_targets

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, C, PH, PW, SCALE = 3, 5, 7, 7, 1.0 / 32
COUNTS = (0, 5, 2)
MAPS = {(7, 11): [(211, 333), (197, 349), (220, 301)], (29, 29): [(900, 850), (911, 925), (870, 905)]}      # map -> image sizes (h, w) < canvas
# normalised cxcywh: image 1 -- smaller than a bin; the whole image (touches every border); on the left and top borders; on the right and bottom
# borders; inside -- image 2 -- inside; on the top and right borders
BOXES = np.array([[0.413, 0.587, 0.003, 0.002], [0.5, 0.5, 1.0, 1.0], [0.15, 0.2, 0.3, 0.4], [0.72, 0.81, 0.56, 0.38], [0.44, 0.37, 0.23, 0.51],
                  [0.61, 0.42, 0.37, 0.29], [0.79, 0.17, 0.42, 0.34]], dtype=np.float32)
_REF = {}


def _rois64(sizes):
    """the float64 rois (7, 5) of BOXES in images of ``sizes``"""
    img = np.repeat(np.arange(N), COUNTS)
    b = BOXES.astype(np.float64)
    h, w = np.array([sizes[i][0] for i in img], dtype=np.float64), np.array([sizes[i][1] for i in img], dtype=np.float64)
    return np.stack((img.astype(np.float64), w * (b[:, 0] - 0.5 * b[:, 2]), h * (b[:, 1] - 0.5 * b[:, 3]), w * (b[:, 0] + 0.5 * b[:, 2]),
                     h * (b[:, 1] + 0.5 * b[:, 3])), 1)


def _conditions(rois, H, W, ratio):
    """asserts the two conditions of the module docstring; -> the largest sampling grid per axis"""
    G = 1
    for r in rois:
        sw, sh, ew, eh = (v * SCALE - 0.5 for v in r[1:])
        for start, size, bins, lim in ((sh, eh - sh, PH, H), (sw, ew - sw, PW, W)):
            per_bin = size / bins
            assert abs(per_bin - round(per_bin)) >= 1e-3, ("bin size near an integer", r, per_bin)
            grid = ratio if ratio > 0 else int(math.ceil(per_bin))
            G = max(G, grid)
            for p in range(bins):
                for i in range(grid):
                    pos = start + p * per_bin + (i + 0.5) * per_bin / grid
                    assert -1 + 1e-3 <= pos <= lim - 1e-3, ("sample near the map's edge", r, pos)
    return G


def _reference(hw, ratio):
    """(input (N, C, H, W) float32 numpy, sizes, want (7, C, PH, PW) float64, bound (7, C, 1, 1)) of one case, computed once"""
    key = (hw, ratio)
    if key not in _REF:
        H, W = hw
        sizes = MAPS[hw]
        assert all(h < 32 * H and w < 32 * W for h, w in sizes)
        rng = np.random.default_rng(1000 * H + ratio)
        inp = rng.standard_normal((N, C, H, W)).astype(np.float32)
        rois = _rois64(sizes)
        G = _conditions(rois, H, W, ratio)
        want = roi_oracle.roi_align(inp, rois, (PH, PW), SCALE, ratio, True)
        M = np.abs(inp).max((2, 3))[rois[:, 0].astype(int)]      # (7, C)
        bound = (64 * max(H, W) + G * G + 16) * 2.0 ** -24 * M[:, :, None, None]
        _REF[key] = (inp, sizes, want, bound, G)
    return _REF[key]


def _buffers(capacity):
    at, targets = 0, []
    for tb in COUNTS:
        targets.append({"labels": torch.zeros(tb, dtype=torch.int64), "boxes": torch.from_numpy(BOXES[at: at + tb])})
        at += tb
    return TargetBuffers(N, capacity, DEV).update_(targets)


@pytest.mark.parametrize("hw", sorted(MAPS))
@pytest.mark.parametrize("ratio", [0, 2])
def test_live_rows_against_the_oracle_dead_rows_zero(hw, ratio):
    inp, sizes, want, bound, G = _reference(hw, ratio)
    if hw == (29, 29) and ratio == 0:
        assert G == 5      # the adaptive grid reaches 5
    x, s = torch.from_numpy(inp).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV)
    outs = {}
    for capacity in (7, 16):
        out, status = roi_align_targets(x, _buffers(capacity), s, (PH, PW), SCALE, ratio, return_status=True)
        assert out.shape == (capacity, C, PH, PW) and out.dtype == torch.float32 and status.tolist() == [0, 0, 0, 0]
        outs[capacity] = out.cpu()
    err = np.abs(outs[7].double().numpy() - want)
    print(f"map {hw} ratio {ratio} grid {G}: worst error / bound {float((err / bound).max()):.4f}")
    assert (err <= bound).all(), float((err / bound).max())
    assert torch.equal(outs[16][:7].view(torch.int32), outs[7].view(torch.int32))      # live rows: the same bits at either capacity
    assert not outs[16][7:].view(torch.int32).any()                                     # dead rows: exact (positive) zeros


def test_dead_slots_read_nothing_through_their_boxes():
    inp, sizes, want, bound, _ = _reference((7, 11), 0)
    x, s = torch.from_numpy(inp).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV)
    bufs = _buffers(16)
    base = roi_align_targets(x, bufs, s, (PH, PW), SCALE, 0)
    with torch.no_grad():
        bufs.tgt_boxes[7:] = torch.tensor([float("nan"), float("inf"), 1e30, -1e30], device=DEV)
    again = roi_align_targets(x, bufs, s, (PH, PW), SCALE, 0)
    assert torch.equal(base.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("cum", [[1, 1, 6, 8], [0, 6, 5, 7], [0, 0, 5, 17], [0, 0, 5, 1 << 40]])
def test_a_bad_prefix_sets_the_status_and_zeroes_everything(cum):
    inp, sizes, _, _, _ = _reference((7, 11), 0)
    x, s = torch.from_numpy(inp).to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV)
    bufs = _buffers(16)
    with torch.no_grad():
        bufs.offsets_dev.copy_(torch.tensor(cum, device=DEV))
    out, status = roi_align_targets(x, bufs, s, (PH, PW), SCALE, 0, return_status=True)
    assert status.tolist() == [0, 0, 0, 1] and not out.view(torch.int32).any()
