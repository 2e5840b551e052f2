"""Float64 definitions of what csrc/convnext_dw.hip writes (richsem_amd.convnext: dwconv7_kernel, dwconv7_wgrad_kernel, layer_scale_kernel,
layer_scale_backward_kernel) with an ELEMENT-WISE error bound per tensor, an fp32 emulation of the kernels' roundings and wrong variants
that must leave the bounds; and the loader of tests/golden/layer_convnext_reference.npz.  Test helper only: the package never imports it.

Inputs are the stored values (bf16 maps, fp32 weights / bias / gamma), so their float64 copies are exact.  The map is channels-last.

    dwconv      out[b,y,x,c] = add[b,y,x,c] + bias[c] + sum_{ky,kx} w[t(ky,kx), c] x[b, y+ky-3, x+kx-3, c],  zeros outside the image,
                t = 7 ky + kx (flip = 0) or 7 (6 - ky) + (6 - kx) (flip = 1)
    wgrad       dw[7 ky + kx, c] = sum_{b,y,x} dy[b,y,x,c] x[b, y+ky-3, x+kx-3, c],   dbias[c] = sum_{b,y,x} dy[b,y,x,c]
    layer scale out = res + gamma z;   dz = gamma dout,   dgamma[c] = sum_t dout[t,c] z[t,c]

The bounds.  u = 2^-8 is the unit round-off of bf16, e = 2^-24 that of fp32; every stored bf16 element is rounded ONCE, at its store.

  dwconv    49 products (one rounding each) added in fp32 in any order, then bias and add: a sum of n + 1 terms in any order is off by at
            most n e times the sum of the magnitudes (to first order), each product brings one more e: 49 + 2 additions + 1 for the products
            gives (49 + 3) e S with S = sum |x| |w| + |bias| + |add|; the store rounds:
                B_out = u |v| + (1 + u) (49 + 3) e S
  dw        n = B H W products added in fp32 in a fixed (but here: any) order, partial sums included:
                B_dw = (n + 2) e sum |dy| |x|,        B_dbias = n e sum |dy|      (no products: dy is exact in fp32)
  out       one product, one sum, one store:   B = u |v| + (1 + u) 2 e (|res| + |gamma z|)
  dz        one product, one store:            B = (u + 2 e) |v|
  dgamma    as dw with n = tokens:             B = (n + 2) e sum |dout z|

1e-30 is added to every bound so that exact zeros compare.

The fp32 emulation (torch on the CPU, the same roundings, taps added in tap order) stays inside the bounds; its worst error / bound
ratios over SHAPES are recorded in profiles/r34_convnext.md (0.97 to 0.99 on the bf16 tensors: one rounding to nearest alone reaches
u |value| just above a power of two; the fp32 tensors stay far below 1).  A torch bf16 convolution, which rounds its result from an
accumulator of its own choosing and adds bias and ``add`` in further roundings, is 100 to 300 bounds away; taps flipped the wrong way
more than 10^4.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -8
E = 2.0 ** -24
TINY = 1e-30
BF = torch.bfloat16
TILE = 16      # kDwTile of csrc/convnext_dw.hip

# (B, H, W, C) of the GPU tests: a map smaller than the kernel; one pixel; an odd map with a width that is no power of two; one just past a
# tile; a wide strip; the tile's edge, T - 1 and T + 1 in either direction
SHAPES = ((2, 3, 5, 32), (2, 1, 1, 128), (2, 13, 9, 96), (1, 16, 17, 64), (1, 7, 40, 32), (1, TILE - 1, TILE + 1, 32), (2, TILE + 1, TILE - 1, 64))
# the weight gradient alone: a part of 3 (image, tile) pairs that crosses from one image into the next, at the widest C
WGRAD_SHAPES = SHAPES + ((3, 17, 17, 4096),)
# (tokens, C): the 64-token parts' edges; 16449 tokens = 258 such parts, past the 256 at which a part grows to 128 tokens (129 parts, the last of 65)
SCALE_SHAPES = tuple((t, c) for c in (32, 96) for t in (1, 63, 65, 130)) + ((16449, 32),)

CONV_WRONG = ("taps_flipped", "clamp_to_edge", "halo_next_image", "bias_dropped", "add_dropped", "last_tap_column_dropped")
WGRAD_WRONG = ("border_pixels_dropped", "taps_flipped")
SCALE_WRONG = ("res_dropped",)
SCALE_BWD_WRONG = ("dgamma_from_out",)


def same_function(wrong, shape):
    """True where a wrong variant is, mathematically, the right function on maps of this shape -- so no bound can tell them apart and the
    tests assert equality instead: on a 1 x 1 map only the centre tap ever meets a pixel (flipping the taps keeps it in place), and tap
    column kx = 6 reads x + 3, outside every map of width <= 3"""
    _, H, W, _ = shape
    return (wrong == "taps_flipped" and H == 1 and W == 1) or (wrong == "last_tap_column_dropped" and W <= 3)


def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def ident(t):
    return t


# ---- depthwise convolution --------------------------------------------------------------------------------------------------------------
def _padded(x, wrong=None):
    """(B, H + 6, W + 6, C): zeros outside each image -- or what a wrong kernel would read there"""
    B, H, W, C = x.shape
    if wrong == "clamp_to_edge":
        return F.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3), mode="replicate").permute(0, 2, 3, 1)
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    if wrong == "halo_next_image":      # the batch as one tall image (cyclic): rows above / below an image belong to its neighbours
        tall = x.reshape(B * H, W, C)
        rows = (torch.arange(-3, H + 3)[None, :] + H * torch.arange(B)[:, None]) % (B * H)      # (B, H + 6)
        xp = F.pad(tall[rows], (0, 0, 3, 3))
    return xp


def _taps(xp, H, W):
    """yields (7 ky + kx, the shifted map x[b, y + ky - 3, x + kx - 3, c])"""
    for ky in range(7):
        for kx in range(7):
            yield 7 * ky + kx, xp[:, ky:ky + H, kx:kx + W, :]


def _dwconv(x, w, bias, add, flip, dtype, rnd, wrong=None):
    B, H, W, C = x.shape
    x, w = x.to(dtype), w.to(dtype)
    if wrong == "taps_flipped":
        flip = 1 - flip
    xp = _padded(x, wrong)
    acc = torch.zeros(B, H, W, C, dtype=dtype)
    for t, shifted in _taps(xp, H, W):
        if wrong == "last_tap_column_dropped" and t % 7 == 6:
            continue
        acc = acc + w[48 - t if flip else t] * shifted
    if bias is not None and wrong != "bias_dropped":
        acc = acc + bias.to(dtype)
    if add is not None and wrong != "add_dropped":
        acc = acc + add.to(dtype)
    return {"out": rnd(acc)}


def dwconv_reference(x, w, bias, add, flip, wrong=None):
    """-> (values, bounds), dicts of float64 tensors with the key "out" """
    val = _dwconv(x, w, bias, add, flip, torch.float64, ident, wrong)
    mag = _dwconv(x.abs(), w.abs(), bias.abs() if bias is not None else None, add.abs() if add is not None else None, flip, torch.float64, ident)["out"]
    return val, {"out": U * val["out"].abs() + (1 + U) * (49 + 3) * E * mag + TINY}


def dwconv_emulate(x, w, bias, add, flip):
    return _dwconv(x, w, bias, add, flip, torch.float32, rnd_bf16)


def dwconv_inputs(shape, gen, with_bias=True, with_add=True):
    """bf16 x and add, fp32 w (49, C) and bias"""
    C = shape[-1]
    x = torch.randn(*shape, generator=gen).to(BF)
    w = torch.randn(49, C, generator=gen) * 0.25
    bias = torch.randn(C, generator=gen) * 0.5 if with_bias else None
    add = torch.randn(*shape, generator=gen).to(BF) if with_add else None
    return x, w, bias, add


def _wgrad(dy, x, dtype, wrong=None):
    B, H, W, C = x.shape
    dy, x = dy.to(dtype), x.to(dtype)
    if wrong == "border_pixels_dropped":
        keep = torch.zeros(H, W, dtype=dtype)
        keep[1:H - 1, 1:W - 1] = 1
        dy = dy * keep[None, :, :, None]
    xp = _padded(x)
    dw = torch.zeros(49, C, dtype=dtype)
    for t, shifted in _taps(xp, H, W):
        dw[48 - t if wrong == "taps_flipped" else t] = (dy * shifted).sum((0, 1, 2))
    return {"dw": dw, "dbias": dy.sum((0, 1, 2))}


def wgrad_reference(dy, x, wrong=None):
    val = _wgrad(dy, x, torch.float64, wrong)
    n = dy.shape[0] * dy.shape[1] * dy.shape[2]
    mag = _wgrad(dy.abs(), x.abs(), torch.float64)
    return val, {"dw": (n + 2) * E * mag["dw"] + TINY, "dbias": n * E * mag["dbias"] + TINY}


def wgrad_emulate(dy, x):
    return _wgrad(dy, x, torch.float32)


# ---- layer scale ------------------------------------------------------------------------------------------------------------------------
def _scale(z, gamma, res, dtype, rnd, wrong=None):
    z, gamma, res = z.to(dtype), gamma.to(dtype), res.to(dtype)
    return {"out": rnd(gamma * z if wrong == "res_dropped" else res + gamma * z)}


def scale_reference(z, gamma, res, wrong=None):
    val = _scale(z, gamma, res, torch.float64, ident, wrong)
    mag = res.double().abs() + (gamma.double() * z.double()).abs()
    return val, {"out": U * val["out"].abs() + (1 + U) * 2 * E * mag + TINY}


def scale_emulate(z, gamma, res):
    return _scale(z, gamma, res, torch.float32, rnd_bf16)


def _scale_backward(dout, z, gamma, res, dtype, rnd, wrong=None):
    dout, z, gamma = dout.to(dtype), z.to(dtype), gamma.to(dtype)
    other = res.to(dtype) + gamma * z if wrong == "dgamma_from_out" else z
    return {"dz": rnd(gamma * dout), "dgamma": (dout * other).sum(0)}


def scale_backward_reference(dout, z, gamma, res, wrong=None):
    val = _scale_backward(dout, z, gamma, res, torch.float64, ident, wrong)
    n = dout.shape[0]
    return val, {"dz": (U + 2 * E) * val["dz"].abs() + TINY, "dgamma": (n + 2) * E * (dout.double() * z.double()).abs().sum(0) + TINY}


def scale_backward_emulate(dout, z, gamma, res):
    return _scale_backward(dout, z, gamma, res, torch.float32, rnd_bf16)


def scale_inputs(tokens, C, gen):
    """bf16 z, res, dout (tokens, C); fp32 gamma"""
    z, res, dout = (torch.randn(tokens, C, generator=gen).to(BF) for _ in range(3))
    return z, 1 + 0.5 * torch.randn(C, generator=gen), res, dout


def ratios(got, val, bound):
    """worst |got - want| / bound per tensor of `val` that `got` holds (inf for a NaN)"""
    res = {}
    for n in val:
        if got.get(n) is None:
            continue
        r = (got[n].double().cpu() - val[n]).abs() / bound[n]
        res[n] = float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())
    return res


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_convnext_reference.npz")) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def fixture_exact(name, dtype=torch.float64):
    """a tensor stored as int16 multiples of 2^-6"""
    return (torch.from_numpy(fixture()[name].astype(np.float64)) / 64).to(dtype)


def fixture_state_dict(tag, dtype=torch.float64):
    sd = {}
    for k, a in fixture().items():
        if k.startswith(tag + ".sd."):
            sd[k[len(tag) + 4:]] = fixture_exact(k, dtype) if a.dtype == np.int16 else torch.from_numpy(a)
    return sd


def fixture_compare(name, got):
    """-> (stored float64 values, the matching values of `got`): the whole tensor, or every stride-th element plus the sum of all"""
    fx = fixture()
    want = torch.from_numpy(np.atleast_1d(fx[name])).double().reshape(-1)
    flat = got.detach().double().cpu().reshape(-1)
    if name + ".stride" in fx:
        flat = torch.cat([flat[::int(fx[name + ".stride"])], flat.sum().reshape(1)])
        want = torch.cat([want, torch.tensor([float(fx[name + ".sum"])], dtype=torch.float64)])
    assert flat.shape == want.shape, (name, flat.shape, want.shape)
    return want, flat
