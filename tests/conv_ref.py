"""Float64 restatements of the convolution family (richsem_amd/csrc/conv_mfma.hip, conv_wgrad.hip) with an ELEMENT-WISE error bound
for every tensor the kernels write, EXACT PROBES whose results do not depend on the summation order, and value mutations of the
references.  The comparator of tests/test_gpu_conv_bounds.py (the kernels against the bounds and the probes) and of
tests/test_conv_ref.py (two correct fp32 implementations against the bounds; the mutations against the comparators).  Test helper only:
the package never imports it.

Notation as in tests/ffn_ref.py (the constants are imported from there): u = 2^-8 is the unit round-off of bf16 under round-to-nearest-
even, e = 2^-24 that of fp32; "an fp32 sum of n terms in any order errs by at most n e sum|term|" (first order; the bounds never rely on
the order); TINY = 1e-30 is added to every bound so that exact zeros compare.  All inputs are bf16 or fp32 values, so their float64 copies
are exact and the float64 results are the reference.  Tensors here are NCHW on the CPU; a case is (N, H, W, C_in, C_out, k, stride, pad).

Forward  y = act(scale conv(x, bf16(w)) + shift (+ residual)),  K = KH KW C_in products per element, S = sum_k |x_k| |w_k|:
    the packed weight is bf16(w), round to nearest even (conv_pack_kernel): the reference rounds the same way, no error term;
    acc    K exact products (bf16 x bf16 fits fp32) summed in fp32 in the MFMA's order                      K e S
    fma    fmaf(acc, scale, shift): the exact value of acc scale + shift, ONE rounding at |.| <= |scale| S + |shift|
    + res  one rounding at |.| <= |scale| S + |shift| + |residual|
        e_f = e ((K + 2) |scale| S + 2 |shift| + |residual|)
    relu is 1-Lipschitz and keeps 0; then ONE bf16 rounding of the fp32 value v, |v - y| <= e_f:  u |v| <= u |y| + u e_f
        B = u |y| + (1 + u) e ((K + c) |scale| S + 2 |shift| + |residual|),        c = 2
    (|shift| counts twice: the fma's rounding and the residual add's both see it.)
    k split (choose_ksplit: at most 16 slices): every slice sums its own products (together the K e S above); the slices' partial
    sums go through LDS unrounded and are added to the zeroed fp32 image by atomics, one rounding at |.| <= S per slice:  c = 2 + 16.

Input gradient  dx = mask(dgrad(dz, w_t) + add),  w_t = bf16(fp32(w scale[co])) flipped and transposed (richsem_amd.conv._pack_form; the
    fp32 product is the same IEEE operation on the CPU), K = KH KW C_out, S = sum |dz| |w_t| over the taps that meet data:
    acc K e S;  scale = shift = NULL: fmaf(acc, 1, 0) is exact;  acc + add is rounded ONCE in fp32, then once to bf16:
        B = u |dx| + (1 + u) e ((K + c) S + |add|),        c = 1   (k split: c = 1 + 16)
    The ring kernel's parity classes walk fewer taps: fewer terms, the same bound.  Elements with relu_out <= 0 (the kernel: the bf16's
    bits as int16 <= 0) must be EXACTLY zero, and so must elements no tap reaches when add is absent (S = 0).

Weight gradient  dw[co, ci, kh, kw] = scale[co] sum_p dz[p, co] x[p + tap, ci],  P = N Ho Wo products, fp32 out:
    products exact, P of them summed per chunk in the MFMA's order, the chunks' `split` partial sums added by the reduce kernel
    (or none: one chunk writes directly), then ONE multiplication by scale:
        B = (P + split + c) e |scale| sum_p |dz| |x|,        c = 2
    split <= min(512, ceil(P / 64)) (wgrad_split / plan_group: chunks are multiples of 64 pixels); that ceiling is what the bound uses.
    dbias = sum_p dz[p, co] (register sums folded through LDS, or a product with a fragment of ones; the chunks added in four phases):
        B = (P + split + c) e sum_p |dz|
    Through MIOpen (ConvAffineFunction's branch for other channel counts) the operands are bf16 and so is the result of
    aten::convolution_backward: fp32 accumulation, ONE bf16 rounding, then the fp32 product with scale:
        B = |scale| (u |dw0| + (1 + u) (P + 2) e S) + e |dw|,      dw0 the unscaled sum.

The n e model for products accumulated INSIDE an MFMA is the one ffn_ref.py uses; it held on the hardware there.

Exact probes.  If all products and all partial sums are integers (or multiples of a fixed power of two) below 2^24 in magnitude, every fp32
addition is exact, whatever the order: atomics, chunk reductions, rings and every tile shape must then give the float64 result bit for bit.
    bf16-output probe (forward, input gradient): x in {0, +-1, +-2}, w in {0, +-1}, non-zero with density min(1, sqrt(48 / K)) each, scale in
        {1, 2, 0.5, -1} per channel, shift / residual / add integers in [-16, 16].  CONDITION (asserted by probe_conditions for every
        element): sum |x| |w| |scale| < 2^22 and the float64 result is a bf16 value.  Then the result is ref.to(bfloat16) exactly.
    fp32-output probe (weight gradient, dbias): dense integers in [-3, 3], scale a power of two.  CONDITION: 9 P < 2^24.
    mask probe: relu_out holding +-0, the +- smallest and largest subnormals, the +- smallest normal, +-1, +-inf: kept iff relu_out > 0.
        NaN apart: the kernel's rule is "bits as int16 > 0", which keeps +NaN and zeroes a NaN with the sign bit set;
        aten::threshold_backward keeps both.  The forward's fmaxf never produces a NaN activation.
"""
import math

import torch
import torch.nn.functional as F

from ffn_ref import BF, E, TINY, U, ratio  # noqa: F401  (ratio: re-exported for the tests)

KSPLIT_MAX = 16          # choose_ksplit (conv_mfma.hip): never more slices


# ---- the host's rules, restated ---------------------------------------------------------------------------------------------------------
def conv_group(Cout):
    """conv_mfma.hip, conv_group(): row tiles per permutation group"""
    tiles = Cout // 16
    return 4 if tiles % 4 == 0 else (2 if tiles % 2 == 0 else 1)


def forced_tile_is_taken(Cout, ct):
    """whether msda_conv_set_tiling(ct, .) changes the tile of a call with `Cout` output channels (the input gradient: its C_in); the
    host otherwise keeps the automatic tile WITHOUT an error -- conv_mfma.hip:994 (forward) and :1127 (input gradient):
    `(Cout / 16) % ct == 0 && ct % conv_group(Cout) == 0`"""
    return ct in (1, 2, 4, 8, 16) and (Cout // 16) % ct == 0 and ct % conv_group(Cout) == 0


def valid_tiles(Cout):
    return [ct for ct in (1, 2, 4, 8, 16) if forced_tile_is_taken(Cout, ct)]


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


# ---- the cases (shared by the CPU and the GPU test) -------------------------------------------------------------------------------------
EPILOGUES = ("plain", "affine_relu", "residual_relu")
PIXEL_EDGE_P = (1, 15, 16, 17, 63, 64, 65, 191, 192, 193)
PIXEL_EDGE_COUT = (48, 96, 64, 128, 256)          # G = 1: ct 1; G = 2: ct 2; ct 4; ct 4, 8; ct 4, 8, 16


def pixel_edge_shapes(Cout):
    return [(1, 1, P, 64, Cout, 1, 1, 0) for P in PIXEL_EDGE_P] + [(1, H, W, 64, Cout, 3, 1, 1) for H, W in ((3, 21), (8, 8), (5, 13))]


CHANNEL_CASES = [c for cin in (32, 96, 64, 128, 192) for c in ((2, 5, 7, cin, 64, 3, 1, 1), (2, 8, 10, cin, 32, 1, 2, 0))]      # (stride 2 on even extents: floor((H - 1) / 2) rounds)
FEW_CHANNEL = ((3, 7), (3, 13), (8, 8), (16, 3), (24, 3), (48, 3), (48, 1), (1, 3))      # (C_in, k): K = 147, 507, 512, 144, 216, 432, 48, 9
FEW_CASES = [(2, 16, 18, cin, 32, k, s, k // 2) for cin, k in FEW_CHANNEL for s in (1, 2)]      # (even extents: the strided Ho, Wo round down)
RING_SLOTS = (3, 4, 6)


def ring_lengths(R):
    return sorted({s for s in (1, 2, R - 2, R - 1, R, R + 1) if s >= 1})


def ring_case(S, Cout):
    """k loop of S iterations (64 channels each) on 35 pixels: 1 x 1 with C_in = 64 S, or 3 x 3 with C_in = 64 for S = 9"""
    return (1, 5, 7, 64, Cout, 3, 1, 1) if S == 9 else (1, 5, 7, 64 * S, Cout, 1, 1, 0)


RING_TILES = ((96, 2, 1), (96, 2, 2), (128, 4, 1), (128, 8, 2))      # C_out, ct, pt
KSPLIT_FWD = [(1, 5, 7, 512, 64, 3, 1, 1), (1, 5, 7, 576, 128, 3, 1, 1)]      # S = 72 in 9 slices; S = 81 in 10 uneven slices
KSPLIT_DGRAD = (1, 5, 7, 64, 512, 3, 1, 1)
DGRAD_GEOM = [(6, 7, 3, 2, 1), (7, 6, 3, 2, 1), (1, 9, 3, 2, 1), (9, 1, 3, 2, 1), (7, 6, 1, 2, 0), (8, 10, 3, 3, 1), (7, 9, 5, 1, 0), (7, 9, 5, 1, 2),
              (7, 9, 5, 1, 4)]      # H, W, k, stride, pad
DGRAD_COUT = (32, 96, 64, 128)
DGRAD_CASES = [(2, H, W, 64, cout, k, s, p) for (H, W, k, s, p) in DGRAD_GEOM for cout in DGRAD_COUT] + [(2, 6, 7, 48, 64, 3, 2, 1)]
DGRAD_VARIANTS = ((False, False), (True, False), (False, True), (True, True))      # add, relu_out
WGRAD_P = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
WGRAD_CASES = [(1, 1, P, 128, 128, 1, 1, 0) for P in WGRAD_P] + [(5, 9, 7, 128, 128, 3, 1, 1), (5, 9, 7, 128, 128, 3, 2, 1), (70, 3, 3, 128, 128, 3, 1, 0),
                                                                  (2, 5, 7, 256, 128, 1, 1, 0), (2, 5, 7, 128, 256, 1, 1, 0)]
GROUP_POOL = [(1, 1, 33, 128, 128, 1, 1, 0), (2, 26, 30, 128, 128, 3, 2, 1), (5, 9, 7, 128, 128, 3, 1, 1), (2, 5, 7, 256, 128, 1, 1, 0),
              (1, 1, 257, 128, 128, 1, 1, 0), (2, 5, 7, 128, 256, 1, 1, 0), (1, 40, 40, 128, 128, 1, 1, 0), (70, 3, 3, 128, 128, 3, 1, 0)]
MODULE_CASES = [(2, 9, 7, 128, 128, 3, 2, 1), (2, 5, 7, 64, 96, 1, 1, 0)]      # own weight-gradient kernel; MIOpen's

# every case of the GPU file, for the CPU file's checks of the probes' conditions, of the bounds and of the mutations
ALL_FWD_CASES = sorted({c for cout in PIXEL_EDGE_COUT for c in pixel_edge_shapes(cout)} | set(CHANNEL_CASES) | set(FEW_CASES) | set(KSPLIT_FWD) |
                       {ring_case(S, cout) for R_ in RING_SLOTS for S in ring_lengths(R_) + [9] for cout, _, _ in RING_TILES} | {MODULE_CASES[0], MODULE_CASES[1]})
ALL_DGRAD_CASES = DGRAD_CASES + [KSPLIT_DGRAD, MODULE_CASES[0], MODULE_CASES[1]]
ALL_WGRAD_CASES = WGRAD_CASES + [c for c in GROUP_POOL if c not in WGRAD_CASES]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def _gen(case, seed, salt):
    return torch.Generator().manual_seed(100003 * seed + 7919 * salt + sum((i + 1) * int(v) for i, v in enumerate(case)))


def _sparse(g, shape, values, density):
    v = torch.tensor(values, dtype=torch.float32)[torch.randint(len(values), shape, generator=g)]
    return v * (torch.rand(shape, generator=g) < density)


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


_SCALES = (1.0, 2.0, 0.5, -1.0)


def make_forward(case, epilogue, seed=0, probe=False):
    """-> {"x" (N, C_in, H, W) bf16, "w" (C_out, C_in, k, k) fp32, "scale", "shift" fp32 or None, "residual" bf16 or None, "relu", "stride",
    "pad"}; the real-valued weight is NOT pre-rounded to bf16: the pack kernel's rounding is part of what is tested"""
    N, H, W, Cin, Cout, k, stride, pad = case
    Ho, Wo = out_hw(H, W, k, stride, pad)
    K = Cin * k * k
    g = _gen(case, seed, EPILOGUES.index(epilogue) + (10 if probe else 0))
    if probe:
        d = min(1.0, math.sqrt(48.0 / K))
        x = _sparse(g, (N, Cin, H, W), (1.0, -1.0, 2.0, -2.0), d)
        w = _sparse(g, (Cout, Cin, k, k), (1.0, -1.0), d)
        scale = torch.tensor(_SCALES)[torch.randint(4, (Cout,), generator=g)]
        shift = _ints(g, (Cout,), -16, 16)
        res = _ints(g, (N, Cout, Ho, Wo), -16, 16)
    else:
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) * K ** -0.5
        scale = 1 + 0.3 * torch.randn(Cout, generator=g)
        shift = torch.randn(Cout, generator=g)
        res = torch.randn(N, Cout, Ho, Wo, generator=g)
    plain = epilogue == "plain"
    return {"x": x.to(BF), "w": w.float(), "scale": None if plain else scale.float(), "shift": None if plain else shift.float(),
            "residual": res.to(BF) if epilogue == "residual_relu" else None, "relu": not plain, "stride": stride, "pad": pad}


MASK_VALUES = (0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 127 * 2.0 ** -133, -127 * 2.0 ** -133, 2.0 ** -126, -(2.0 ** -126), 1.0, -1.0, float("inf"),
               float("-inf"))


def mask_probe_values():
    """+-0, +- smallest and largest bf16 subnormal, +- smallest normal, +-1, +-inf as bf16 (the bit patterns are asserted)"""
    v = torch.tensor(MASK_VALUES, dtype=torch.float32).to(BF)
    bits = [b & 0xFFFF for b in v.view(torch.int16).tolist()]
    assert bits == [0x0000, 0x8000, 0x0001, 0x8001, 0x007F, 0x807F, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x7F80, 0xFF80], [hex(b) for b in bits]
    return v


def make_dgrad(case, add, relu_out, seed=0, probe=False, mask_probe=False):
    """-> {"dz" (N, C_out, Ho, Wo) bf16, "w" (C_out, C_in, k, k) fp32, "scale" (C_out) fp32, "add", "relu_out" (N, C_in, H, W) bf16 or None,
    "x_shape", "stride", "pad"}.  relu_out is a ReLU's output (about half zeros) with the mask probe's values cycled over its first
    elements -- or, with mask_probe, over ALL its elements"""
    N, H, W, Cin, Cout, k, stride, pad = case
    Ho, Wo = out_hw(H, W, k, stride, pad)
    K = Cout * k * k
    g = _gen(case, seed, 20 + (10 if probe else 0))
    if probe:
        d = min(1.0, math.sqrt(48.0 / K))
        dz = _sparse(g, (N, Cout, Ho, Wo), (1.0, -1.0, 2.0, -2.0), d)
        w = _sparse(g, (Cout, Cin, k, k), (1.0, -1.0), d)
        scale = torch.tensor(_SCALES)[torch.randint(4, (Cout,), generator=g)]
        a = _ints(g, (N, Cin, H, W), -16, 16)
    else:
        dz = torch.randn(N, Cout, Ho, Wo, generator=g)
        w = torch.randn(Cout, Cin, k, k, generator=g) * K ** -0.5
        scale = 1 + 0.3 * torch.randn(Cout, generator=g)
        a = torch.randn(N, Cin, H, W, generator=g)
    act = torch.relu(torch.randn(N, Cin, H, W, generator=g)).to(BF)
    mv = mask_probe_values()
    flat = act.permute(0, 2, 3, 1).reshape(-1)      # (a copy: NHWC order, where the kernel's 8-byte mask loads see the values side by side)
    n = flat.numel() if mask_probe else min(flat.numel(), 5 * len(mv) + 3)
    flat[:n] = mv[torch.arange(n) % len(mv)]
    act = flat.view(N, H, W, Cin).permute(0, 3, 1, 2).contiguous()
    return {"dz": dz.to(BF), "w": w.float(), "scale": scale.float(), "add": a.to(BF) if add else None, "relu_out": act if relu_out else None,
            "x_shape": (N, Cin, H, W), "stride": stride, "pad": pad}


def make_wgrad(case, seed=0, probe=False):
    """-> {"dz" (N, C_out, Ho, Wo), "x" (N, C_in, H, W) bf16, "scale" (C_out) fp32 (the caller passes it or NULL), "k", "stride", "pad"}"""
    N, H, W, Cin, Cout, k, stride, pad = case
    Ho, Wo = out_hw(H, W, k, stride, pad)
    g = _gen(case, seed, 40 + (10 if probe else 0))
    if probe:
        dz, x = _ints(g, (N, Cout, Ho, Wo), -3, 3), _ints(g, (N, Cin, H, W), -3, 3)
        scale = 2.0 ** torch.randint(-3, 4, (Cout,), generator=g).float() * (1 - 2 * torch.randint(2, (Cout,), generator=g).float())
    else:
        dz, x = torch.randn(N, Cout, Ho, Wo, generator=g), torch.randn(N, Cin, H, W, generator=g)
        scale = 1 + 0.3 * torch.randn(Cout, generator=g)
    return {"dz": dz.to(BF), "x": x.to(BF), "scale": scale.float(), "k": k, "stride": stride, "pad": pad}


# ---- float64 references with bounds; `mutate` names a deliberate defect (MUTATIONS) ---------------------------------------------------
FWD_MUTATIONS = ("kstep", "pad", "ceil", "swap", "halves", "scale2")
DGRAD_MUTATIONS = ("kstep", "pad", "swap", "halves", "parity", "scale2")
WGRAD_MUTATIONS = ("tail", "pad", "scale2")


def _swap_halves(t):
    """channels 0..7 and 8..15 of every 64 exchanged (the two 8-channel halves a lane group reads in the two k-steps of a pair)"""
    idx = torch.arange(t.shape[1])
    j = idx % 64
    idx = torch.where(j < 8, idx + 8, torch.where(j < 16, idx - 8, idx))
    return t[:, idx]


def _swap_channels(t):
    """output channels 1 and 5: rows 4 u + i with i = 1 of tiles u = 0 and u = 1 of the first group"""
    idx = torch.arange(t.shape[1])
    idx[1], idx[5] = 5, 1
    return t[:, idx]


def _shift_right(t):
    """every image moved one pixel to the right (zero column in front): a left padding one too large"""
    return F.pad(t, (1, 0))[..., :-1]


def mutation_applies(op, name, case):
    N, H, W, Cin, Cout, k, stride, pad = case
    kdim, odim = (Cin, Cout) if op == "forward" else (Cout, Cin)
    if name == "kstep":      # ... and the tap whose last k-step is dropped meets data somewhere
        Ho, Wo = out_hw(H, W, k, stride, pad)
        met = (k - 1 - pad < H and k - 1 - pad < W) if op == "forward" else ((Ho - 1) * stride >= pad and (Wo - 1) * stride >= pad)
        return kdim % 32 == 0 and met
    if name == "halves":
        return kdim % 64 == 0
    if name == "swap":
        return conv_group(odim) >= 2
    if name == "ceil":
        return op == "forward" and ((W + 2 * pad - k) % stride != 0 or (N > 1 and (H + 2 * pad - k) % stride != 0))
    if name == "parity":
        return op == "dgrad" and stride > 1
    if name == "pad":
        return W > 1
    return True


def forward_reference(p, ksplit=False, mutate=None):
    """-> (y float64 (N, C_out, Ho, Wo), bound)"""
    x, w = p["x"].double(), p["w"].to(BF).double()
    stride, pad = p["stride"], p["pad"]
    Cout, Cin, k, _ = w.shape
    N, _, H, W = x.shape
    Ho, Wo = out_hw(H, W, k, stride, pad)
    scale = p["scale"].double() if p["scale"] is not None else torch.ones(Cout, dtype=torch.float64)
    shift = p["shift"].double() if p["shift"] is not None else torch.zeros(Cout, dtype=torch.float64)
    if mutate == "kstep":
        w = w.clone()
        w[:, -32:, -1, -1] = 0
    elif mutate == "halves":
        x = _swap_halves(x)
    elif mutate == "pad":
        x = _shift_right(x)
    elif mutate == "scale2":
        scale = scale * scale
    if mutate == "ceil":      # pixel p decoded with Ho' = ceil(.) + 1, Wo' likewise: the kernel's flat pixel order over the wrong grid
        full = F.conv2d(F.pad(x, (0, stride - 1, 0, stride - 1)), w, None, stride, pad)
        conv = full.permute(1, 0, 2, 3).flatten(1)[:, :N * Ho * Wo].reshape(Cout, N, Ho, Wo).permute(1, 0, 2, 3)
    else:
        conv = F.conv2d(x, w, None, stride, pad)
    if mutate == "swap":
        conv = _swap_channels(conv)
    mag = F.conv2d(p["x"].double().abs(), p["w"].to(BF).double().abs(), None, stride, pad) * scale.abs()[None, :, None, None]
    y = conv * scale[None, :, None, None] + shift[None, :, None, None]
    tail = 2 * shift.abs()[None, :, None, None].expand_as(y)
    if p["residual"] is not None:
        y = y + p["residual"].double()
        tail = tail + p["residual"].double().abs()
    if p["relu"]:
        y = torch.relu(y)
    c = 2 + (KSPLIT_MAX if ksplit else 0)
    return y, U * y.abs() + (1 + U) * E * ((Cin * k * k + c) * mag + tail) + TINY


def dgrad_weight(p, twice=False):
    """bf16(fp32(w scale[co])) as float64, (C_out, C_in, k, k): what _pack_form packs, before its flip and transposition"""
    w = p["w"] * p["scale"].view(-1, 1, 1, 1)
    if twice:
        w = w * p["scale"].view(-1, 1, 1, 1)
    return w.to(BF).double()


def dgrad_reference(p, ksplit=False, mutate=None):
    """-> (dx float64 (N, C_in, H, W), bound, must_be_zero)"""
    dz, w = p["dz"].double(), dgrad_weight(p, mutate == "scale2")
    stride, pad = p["stride"], p["pad"]
    Cout, Cin, k, _ = w.shape
    shape = p["x_shape"]
    if mutate == "kstep":      # the last tap the kernel walks is tap (0, 0) of the unflipped weight
        w = w.clone()
        w[-32:, :, 0, 0] = 0
    elif mutate == "halves":
        dz = _swap_halves(dz)
    dx = torch.nn.grad.conv2d_input(shape, w, dz, stride=stride, padding=pad)
    if mutate == "pad":
        dx = _shift_right(dx)
    elif mutate == "swap":
        dx = _swap_channels(dx)
    elif mutate == "parity":      # the class (pad % s, pad % s), whose first tap is (0, 0) (class 0 where the image has no such row / column:
        dx = dx.clone()           # its first tap is pad % s < k): never a class without taps
        ph, pw = (pad % stride if pad % stride < shape[2] else 0), (pad % stride if pad % stride < shape[3] else 0)
        dx[:, :, ph::stride, pw::stride] = 0
    mag = torch.nn.grad.conv2d_input(shape, dgrad_weight(p).abs(), p["dz"].double().abs(), stride=stride, padding=pad)
    zero = (mag == 0) if p["add"] is None else torch.zeros_like(mag, dtype=torch.bool)
    tail = torch.zeros_like(mag)
    if p["add"] is not None:
        dx = dx + p["add"].double()
        tail = p["add"].double().abs()
    if p["relu_out"] is not None:
        dead = ~(p["relu_out"] > 0)
        dx = torch.where(dead, torch.zeros_like(dx), dx)
        zero = zero | dead
    c = 1 + (KSPLIT_MAX if ksplit else 0)
    return dx, U * dx.abs() + (1 + U) * E * ((Cout * k * k + c) * mag + tail) + TINY, zero


def wgrad_split_ceiling(P):
    return min(512, (P + 63) // 64)


def wgrad_reference(p, scaled=True, mutate=None):
    """-> ({"dw" (C_out, C_in, k, k), "dbias" (C_out)} float64, bounds); torch_layout 0 is dw.permute(0, 2, 3, 1)"""
    dz, x = p["dz"].double(), p["x"].double()
    k, stride, pad = p["k"], p["stride"], p["pad"]
    N, Cout, Ho, Wo = dz.shape
    Cin = x.shape[1]
    P = N * Ho * Wo
    scale = p["scale"].double() if scaled else torch.ones(Cout, dtype=torch.float64)
    if mutate == "scale2":
        scale = scale * scale
    elif mutate == "pad":
        x = _shift_right(x)
    elif mutate == "tail":      # the last pixel of the last chunk
        dz = dz.clone()
        dz[-1, :, -1, -1] = 0
    dw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dz, stride=stride, padding=pad) * scale.view(-1, 1, 1, 1)
    mag = torch.nn.grad.conv2d_weight(p["x"].double().abs(), (Cout, Cin, k, k), p["dz"].double().abs(), stride=stride, padding=pad)
    n = P + wgrad_split_ceiling(P) + 2
    val = {"dw": dw, "dbias": dz.sum(dim=(0, 2, 3))}
    bound = {"dw": n * E * scale.abs().view(-1, 1, 1, 1) * mag + TINY, "dbias": n * E * p["dz"].double().abs().sum(dim=(0, 2, 3)) + TINY}
    return val, bound


def miopen_dw_bound(p):
    """dw through aten::convolution_backward on bf16 operands (bf16 result), times scale in fp32: see the module docstring"""
    val, _ = wgrad_reference(p, scaled=False)
    P = p["dz"].shape[0] * p["dz"].shape[2] * p["dz"].shape[3]
    mag = torch.nn.grad.conv2d_weight(p["x"].double().abs(), tuple(val["dw"].shape), p["dz"].double().abs(), stride=p["stride"], padding=p["pad"])
    s = p["scale"].double().abs().view(-1, 1, 1, 1)
    return s * (U * val["dw"].abs() + (1 + U) * (P + 2) * E * mag) + E * s * val["dw"].abs() + TINY


# ---- the probes' conditions -------------------------------------------------------------------------------------------------------------
def is_bf16(t):
    return bool((t.float().to(BF).double() == t).all())


def probe_conditions(op, p):
    """the exact probe's premises for EVERY element -> (holds, share of non-zero outputs, largest sum of |products|)"""
    if op == "forward":
        y, _ = forward_reference(p)
        s = p["scale"].double().abs().view(1, -1, 1, 1) if p["scale"] is not None else 1.0
        mag = F.conv2d(p["x"].double().abs(), p["w"].double().abs(), None, p["stride"], p["pad"]) * s
        ok = is_bf16(p["w"]) and is_bf16(y) and float(mag.max()) + 64 < 2 ** 22
        base = F.conv2d(p["x"].double(), p["w"].double(), None, p["stride"], p["pad"])
        return ok, float((base != 0).double().mean()), float(mag.max())
    if op == "dgrad":
        y, _, _ = dgrad_reference(p)
        w = p["w"].double() * p["scale"].double().view(-1, 1, 1, 1)
        mag = torch.nn.grad.conv2d_input(p["x_shape"], w.abs(), p["dz"].double().abs(), stride=p["stride"], padding=p["pad"])
        ok = bool((dgrad_weight(p) == w).all()) and is_bf16(y) and float(mag.max()) + 64 < 2 ** 22
        base = torch.nn.grad.conv2d_input(p["x_shape"], w, p["dz"].double(), stride=p["stride"], padding=p["pad"])
        return ok, float((base != 0).double().mean()), float(mag.max())
    val, _ = wgrad_reference(p)
    P = p["dz"].shape[0] * p["dz"].shape[2] * p["dz"].shape[3]
    frac, _ = torch.frexp(p["scale"])
    ok = 9 * P < 2 ** 24 and bool((frac.abs() == 0.5).all()) and float(p["dz"].abs().max()) <= 3 and float(p["x"].abs().max()) <= 3 and \
        bool((val["dw"].float().double() == val["dw"]).all())
    return ok, float((val["dw"] != 0).double().mean()), 9.0 * P


# ---- two correct fp32 implementations (tests/test_conv_ref.py) --------------------------------------------------------------------------
def _chunks(n, g, size):
    perm = torch.randperm(n, generator=g)
    return [perm[i:i + size] for i in range(0, n, size)]


def fp32_forward(p, g=None):
    """fp32 F.conv2d with the kernel's roundings (bf16 weight, fp32 epilogue, one bf16 result); g: the input channels summed in shuffled chunks"""
    x, w = p["x"].float(), p["w"].to(BF).float()
    if g is None:
        acc = F.conv2d(x, w, None, p["stride"], p["pad"])
    else:
        acc = None
        for idx in _chunks(x.shape[1], g, 24):
            part = F.conv2d(x[:, idx], w[:, idx], None, p["stride"], p["pad"])
            acc = part if acc is None else acc + part
    if p["scale"] is not None:
        acc = acc * p["scale"][None, :, None, None] + p["shift"][None, :, None, None]
    if p["residual"] is not None:
        acc = acc + p["residual"].float()
    return (torch.relu(acc) if p["relu"] else acc).to(BF)


def fp32_dgrad(p, g=None):
    dz, w = p["dz"].float(), dgrad_weight(p).float()
    if g is None:
        acc = torch.nn.grad.conv2d_input(p["x_shape"], w, dz, stride=p["stride"], padding=p["pad"])
    else:
        acc = None
        for idx in _chunks(dz.shape[1], g, 24):
            part = torch.nn.grad.conv2d_input(p["x_shape"], w[idx], dz[:, idx], stride=p["stride"], padding=p["pad"])
            acc = part if acc is None else acc + part
    if p["add"] is not None:
        acc = acc + p["add"].float()
    if p["relu_out"] is not None:
        acc = torch.where(p["relu_out"] > 0, acc, torch.zeros_like(acc))
    return acc.to(BF)


def fp32_wgrad(p, g=None, scaled=True):
    dz, x = p["dz"].float(), p["x"].float()
    shape = (dz.shape[1], x.shape[1], p["k"], p["k"])
    if g is None:
        dw, db = torch.nn.grad.conv2d_weight(x, shape, dz, stride=p["stride"], padding=p["pad"]), dz.sum(dim=(0, 2, 3))
    else:      # the pixels in four random chunks, as the pixel split sums them
        owner = torch.randint(4, (dz.shape[0], 1, dz.shape[2], dz.shape[3]), generator=g)
        dw, db = 0, 0
        for j in range(4):
            part = dz * (owner == j)
            dw = dw + torch.nn.grad.conv2d_weight(x, shape, part, stride=p["stride"], padding=p["pad"])
            db = db + part.sum(dim=(0, 2, 3))
    return {"dw": dw * p["scale"].view(-1, 1, 1, 1) if scaled else dw, "dbias": db}
