"""Float64 definitions of what csrc/swin_stage.hip writes (richsem_amd.swin: merge_norm_kernel, norm_nchw_kernel, patch rows and their
backwards), with element-wise bounds, fp32 emulations and wrong variants that must leave the bounds.  Test helper only: the package never
imports it.

NO NEW BOUND is derived here and no tolerance chosen.  The kernels are the LayerNorm of csrc/swin_block_mfma.hip, operation for operation,
on rows whose elements live elsewhere; so value and bound are ``swin_block_ref.layernorm_reference`` / ``layernorm_backward_reference``
applied to the GATHERED matrix, with ``dx`` and its bound scattered back; for the NCHW norm the same, transposed.  The gather / scatter
index helpers are written from the formulas of include/richsem_msda.h:

    merging norm   row (b, i, j) of (B H2 W2, 4 C), H2 = (H + 1) // 2, W2 = (W + 1) // 2; channel q C + c = pixel (2 i + (q & 1), 2 j + (q >> 1))
                   of the map (B, H, W, C); a pixel outside the map is a zero that takes part in the statistics; its gradient is dropped,
                   its xhat = (0 - mean) rstd counts in dgamma
    NCHW norm      out[b, c, t] = LayerNorm(x[b, t, :])[c];  dy (B, C, HW) -> dx (B, HW, C), dgamma / dbeta sums over the B HW tokens
    patch rows     rows[(b, i, j), (c ph + dy) pw + dx] = img[b, c, i ph + dy, j pw + dx], zeros past the image and past Cin ph pw

The fp32 emulations are swin_block_ref's (the same roundings in the same places) on the gathered matrix.  The wrong variants are index or
padding mistakes; each must leave the bounds on every shape of tests/test_gpu_swin_stage.py on which it is a different function at all
(``*_applies``: a map of even H and W has no padding; H = W = 1 has nothing to exchange), which is what makes those shapes the smallest at
which the kernels can go wrong."""
import torch

import swin_block_ref as R

BF = torch.bfloat16
MERGE_SHAPES = [(1, 1, 1, 32), (2, 3, 5, 32), (1, 4, 6, 96), (2, 13, 9, 32), (1, 18, 16, 32), (1, 2, 3, 1024)]      # (B, H, W, C)
NCHW_SHAPES = [(1, 1, 32), (2, 35, 64), (2, 130, 32), (1, 67, 1536), (1, 200, 4096)]                              # (B, HW, C)
PATCH_SHAPES = [((2, 3, 40, 52), (4, 4)), ((1, 3, 13, 18), (4, 4)), ((1, 3, 1, 1), (4, 4)), ((1, 1, 4, 4), (4, 4)), ((1, 5, 7, 9), (2, 4))]
MERGE_WRONG = ("quadrants_swapped", "pad_out_of_statistics", "hw_exchanged")
MERGE_BWD_WRONG = ("quadrants_swapped", "pad_out_of_dgamma", "hw_exchanged", "pad_gradient_to_neighbour")
NCHW_WRONG = ("tile_not_transposed",)
NCHW_BWD_WRONG = ("tile_not_transposed", "dbeta_over_channels")


# ---- index helpers ---------------------------------------------------------------------------------------------------------------------
def merge_index(B, H, W, C, swapped=False, clamp=False):
    """(B H2 W2, 4 C) int64: the element of the flattened map (B H W C) a row element is, -1 for a pixel outside the map.  `swapped`: the
    quadrants in (dy, dx)-swapped order; `clamp`: a pixel outside goes to its nearest neighbour inside (with a mask of those elements)"""
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    b, i, j, q = torch.meshgrid(torch.arange(B), torch.arange(H2), torch.arange(W2), torch.arange(4), indexing="ij")
    oy, ox = (q >> 1, q & 1) if swapped else (q & 1, q >> 1)
    y, x = 2 * i + oy, 2 * j + ox
    inside = (y < H) & (x < W)
    pix = (b * H + y.clamp(max=H - 1)) * W + x.clamp(max=W - 1)
    idx = pix[..., None] * C + torch.arange(C)
    inside = inside[..., None].expand_as(idx)
    if not clamp:
        idx = torch.where(inside, idx, torch.full_like(idx, -1))
    idx, inside = idx.reshape(B * H2 * W2, 4 * C), inside.reshape(B * H2 * W2, 4 * C)
    return (idx, inside) if clamp else idx


def gather(xmap, idx):
    """xmap (B, H, W, C) -> the rows (idx.shape), zeros where idx is -1"""
    flat = xmap.reshape(-1)
    return torch.where(idx >= 0, flat[idx.clamp(min=0)], torch.zeros((), dtype=flat.dtype))


def scatter(rows, idx, shape, fill=0.0):
    """the inverse: rows' elements to their places in a map of `shape`; every element of the map must be hit exactly once"""
    hit = torch.zeros(torch.Size(shape).numel(), dtype=torch.int64)
    keep = idx >= 0
    hit.index_add_(0, idx[keep], torch.ones_like(idx[keep]))
    assert bool((hit == 1).all()), "the index is not a bijection onto the map"
    out = torch.full((hit.numel(),), fill, dtype=rows.dtype)
    out[idx[keep]] = rows[keep]
    return out.reshape(shape)


def patch_rows_reference(img, ph, pw):
    """a torch unfold of the zero-padded image -> (B Wh Ww, Kp), in the image's dtype (pure data movement)"""
    B, Cin, H, W = img.shape
    Wh, Ww = -(-H // ph), -(-W // pw)
    pad = torch.zeros(B, Cin, Wh * ph, Ww * pw, dtype=img.dtype)
    pad[:, :, :H, :W] = img
    rows = pad.view(B, Cin, Wh, ph, Ww, pw).permute(0, 2, 4, 1, 3, 5).reshape(B * Wh * Ww, Cin * ph * pw)
    Kp = -(-Cin * ph * pw // 32) * 32
    return torch.cat([rows, torch.zeros(rows.shape[0], Kp - rows.shape[1], dtype=img.dtype)], 1)


def patch_rows_backward_reference(drows, shape, ph, pw):
    B, Cin, H, W = shape
    Wh, Ww = -(-H // ph), -(-W // pw)
    d = drows[:, :Cin * ph * pw].reshape(B, Wh, Ww, Cin, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B, Cin, Wh * ph, Ww * pw)
    return d[:, :, :H, :W].contiguous()


# ---- merging norm ----------------------------------------------------------------------------------------------------------------------
def merge_inputs(B, H, W, C, gen):
    """bf16 map x (B, H, W, C) (pixels of different offsets and spreads), bf16 dy (rows, 4 C), fp32 gamma, beta (4 C)"""
    x = R.layernorm_inputs(B * H * W, C, gen, with_add=False)[0].view(B, H, W, C)
    rows = B * ((H + 1) // 2) * ((W + 1) // 2)
    dy = torch.randn(rows, 4 * C, generator=gen).to(BF)
    return x, dy, 1 + 0.5 * torch.randn(4 * C, generator=gen), 0.5 * torch.randn(4 * C, generator=gen)


def merge_wrong_applies(wrong, B, H, W, C):
    if wrong in ("quadrants_swapped", "hw_exchanged"):
        return (H, W) != (1, 1) and (wrong == "quadrants_swapped" or H != W)
    return bool(H % 2 or W % 2)      # the padding variants


def _merge_idx(x, wrong):
    B, H, W, C = x.shape
    if wrong == "hw_exchanged":
        return merge_index(B, W, H, C)
    return merge_index(B, H, W, C, swapped=wrong == "quadrants_swapped")


def _masked_layernorm(g, keep, gamma, beta, eps):
    """LayerNorm whose statistics leave the elements outside `keep` out (they still read as zeros in the numerator)"""
    n = keep.sum(1, keepdim=True)
    mean = (g * keep).sum(1, keepdim=True) / n
    var = (((g - mean) ** 2) * keep).sum(1, keepdim=True) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    return {"out": (g - mean) * rstd * gamma + beta, "mean": mean[:, 0], "rstd": rstd[:, 0]}


def merge_norm_reference(x, gamma, beta, eps, wrong=None):
    """-> (values, bounds): "out" (rows, 4 C), "mean", "rstd" (rows) in float64"""
    idx = _merge_idx(x, wrong)
    if wrong == "pad_out_of_statistics":
        return _masked_layernorm(gather(x.double(), idx), (idx >= 0).double(), gamma.double(), beta.double(), eps), None
    return R.layernorm_reference(gather(x, idx), gamma, beta, eps)


def merge_norm_emulate(x, gamma, beta, eps):
    return R.layernorm_emulate(gather(x, merge_index(*x.shape)), gamma, beta, eps)


def _scatter_dx(res, x, idx, wrong=None):
    """`dx` of a row-layout result back to the map"""
    if wrong == "pad_gradient_to_neighbour":      # a padded quadrant's gradient lands on the nearest pixel inside, after that pixel's own
        cidx, inside = merge_index(*x.shape, clamp=True)
        out = scatter(res["dx"], idx, x.shape).reshape(-1).clone()
        out[cidx[~inside]] = res["dx"][~inside]
        return out.reshape(x.shape)
    return scatter(res["dx"], idx, x.shape)


def merge_norm_backward_reference(dy, x, gamma, eps, wrong=None):
    """-> (values, bounds): "dx" (B, H, W, C), "dgamma", "dbeta" (4 C); the statistics are the float64 moments of the gathered rows"""
    idx = _merge_idx(x, wrong)
    g = gather(x, idx)
    val, bound = R.layernorm_backward_reference(dy, g, gamma, None, eps)
    if wrong == "pad_out_of_dgamma":
        mean, _, rstd, xhat, _, _, _ = R._stat_bounds(g, eps)
        val["dgamma"] = (dy.double() * xhat * (idx >= 0)).sum(0)
    val["dx"], bound["dx"] = _scatter_dx(val, x, idx, wrong), scatter(bound["dx"], idx, x.shape)
    return val, bound


def merge_norm_backward_emulate(dy, x, gamma, eps):
    idx = merge_index(*x.shape)
    res = R.layernorm_backward_emulate(dy, gather(x, idx), gamma, None, eps)
    res["dx"] = scatter(res["dx"], idx, x.shape)
    return res


# ---- output norm to NCHW ---------------------------------------------------------------------------------------------------------------
def nchw_inputs(B, HW, C, gen):
    """bf16 tokens x (B, HW, C), bf16 dy (B, C, HW), fp32 gamma, beta (C)"""
    x, _, _, gamma, beta = R.layernorm_inputs(B * HW, C, gen, with_add=False)
    return x.view(B, HW, C), torch.randn(B, C, HW, generator=gen).to(BF), gamma, beta


def nchw_wrong_applies(wrong, B, HW, C):
    return HW > 1


def _to_nchw(rows, B, HW, C, wrong=None):
    if wrong == "tile_not_transposed":      # the (tokens, channels) tile written as it stands into the (channels, tokens) buffer
        return rows.reshape(B, C, HW)
    return rows.view(B, HW, C).transpose(1, 2).contiguous()


def _from_nchw(t, wrong=None):
    B, C, HW = t.shape
    if wrong == "tile_not_transposed":
        return t.reshape(B * HW, C)
    return t.transpose(1, 2).reshape(B * HW, C)


def norm_nchw_reference(x, gamma, beta, eps, wrong=None):
    """-> (values, bounds): "out" (B, C, HW), "mean", "rstd" (B HW)"""
    B, HW, C = x.shape
    val, bound = R.layernorm_reference(x.reshape(B * HW, C), gamma, beta, eps)
    val["out"], bound["out"] = _to_nchw(val["out"], B, HW, C, wrong), _to_nchw(bound["out"], B, HW, C)
    return val, bound


def norm_nchw_emulate(x, gamma, beta, eps):
    B, HW, C = x.shape
    res = R.layernorm_emulate(x.reshape(B * HW, C), gamma, beta, eps)
    res["out"] = _to_nchw(res["out"], B, HW, C)
    return res


def norm_nchw_backward_reference(dy, x, gamma, eps, wrong=None):
    """-> (values, bounds): "dx" (B, HW, C), "dgamma", "dbeta" (C)"""
    B, HW, C = x.shape
    val, bound = R.layernorm_backward_reference(_from_nchw(dy, "tile_not_transposed" if wrong == "tile_not_transposed" else None),
                                                x.reshape(B * HW, C), gamma, None, eps)
    if wrong == "dbeta_over_channels":      # the sum runs along the buffer's other axis
        val["dbeta"] = dy.double().reshape(B * HW, C).sum(0)
    val["dx"], bound["dx"] = val["dx"].view(B, HW, C), bound["dx"].view(B, HW, C)
    if wrong == "tile_not_transposed":
        bound = norm_nchw_backward_reference(dy, x, gamma, eps)[1]
    return val, bound


def norm_nchw_backward_emulate(dy, x, gamma, eps):
    B, HW, C = x.shape
    res = R.layernorm_backward_emulate(_from_nchw(dy), x.reshape(B * HW, C), gamma, None, eps)
    res["dx"] = res["dx"].view(B, HW, C)
    return res


# ---- the exact probe -------------------------------------------------------------------------------------------------------------------
def sign_probe(shape, gen):
    """x[..., c] = s (-1)^c with a seeded sign s per leading index: every row built from such elements has mean 0 and variance 1 exactly,
    so with eps = 0 its LayerNorm is rnd(s (-1)^c gamma + beta) bit for bit.  -> x (shape) bf16"""
    s = torch.randint(0, 2, shape[:-1], generator=gen).float() * 2 - 1
    alt = 1 - 2 * (torch.arange(shape[-1]) % 2).float()
    return (s[..., None] * alt).to(BF)


ratios = R.ratios
