"""Float64 definitions of what csrc/focalnet_ctx.hip writes (richsem_amd.focalnet: context_forward_kernel, context_backward_kernel,
modulate_kernel, modulate_backward_kernel), each tensor from the STORED inputs of the kernel that writes it, with an ELEMENT-WISE error
bound per tensor, an fp32 emulation of the kernels' roundings and wrong variants that must leave the bounds; and the loader of
tests/golden/layer_focalnet_reference.npz.  Test helper only: the package never imports it.

Inputs are the stored values (bf16 maps and gates, fp32 weights), so their float64 copies are exact.  Maps are channels-last.  L levels,
K_l = window + 2 l, s = 1 / (L + 1) with ``normalize`` else 1, ctx_l = GELU(u_l) of the STORED u_l, x_l = the input of level l's
convolution = ctx0 (l = 0) or ctx_{l-1}:

    u{l}     conv_{K_l}(x_l):  sum_{ky,kx} w_l[K ky + kx, c] x_l[b, y + ky - K/2, x + kx - K/2, c], zeros outside the image
    m, g     m[b,c] = mean_{y,x} ctx_{L-1};  g = GELU(m) of the stored m
    A        s (sum_{l<L} gate_l ctx_l + gate_L g) with the stored g
    dgates   [..., l] = s sum_c dA ctx_l (l < L);  [..., L] = s sum_c dA g
    du{L-1}  (s gate_{L-1} dA + dm / (H W)) GELU'(u_{L-1}),  dm = s (sum_p dA gate_L) GELU'(m)
    du{l-1}  (conv_flip_{K_l}(du_l) + s gate_{l-1} dA) GELU'(u_{l-1}) from the stored du_l, l = L-1 .. 1
    dctx0    conv_flip_{K_0}(du_0)
    dw{l}    [K ky + kx, c] = sum_{b,y,x} du_l[b,y,x,c] x_l[b, y + ky - K/2, x + kx - K/2, c]
    out, dq, dmod    q mod,  dout mod,  dout q

The bounds.  u = 2^-8 is the unit round-off of bf16, e = 2^-24 that of fp32; every stored bf16 element is rounded once, at its store.
GELU in fp32 (x/2 erfc(-x/sqrt 2)): the argument's rounding moves erfc by a relative x^2 e in the lower tail, the library's erfc is good
to a few units, two products: |error| <= (8 + x^2) e |GELU(x)| =: ge(x).  GELU' = cdf + x pdf with a fast exp whose argument x^2/2 is
rounded: |error| <= e (8 cdf + (8 + x^2/2) |x| pdf) =: gpe(x).  Where ctx_{l-1} is the input of a convolution or of a weight gradient
the kernel rounds it to bf16 (the LDS tile holds bf16): an input perturbation of u |ctx| + ge, carried through the sum.

  u{l}     K^2 products added in fp32 in any order:  B = u |v| + (1 + u) ((K^2 + 1) e S + P),  S = sum |w| |x_l|,
           P = sum |w| (u |ctx_{l-1}| + ge(u_{l-1})) for l > 0, else 0
  m        n = H W terms:  B = (n + 2) e mean |ctx| + mean ge;      g:  B = ge(m)
  A        B = u |v| + (1 + u) s ((L + 3) e T + sum_l |gate_l| ge(u_l)),  T = sum_l |gate_l ctx_l| + |gate_L g|
  dgates   B = u |v| + (1 + u) s ((C + 3) e sum_c |dA ctx_l| + sum_c |dA| ge(u_l));  the last: (C + 3) e sum_c |dA g|
  du{L-1}  t = s gate dA (3 e |t|), d = dm / (H W) with B_d = (n + 5) e D |GELU'(m)| + D gpe(m), D = s sum_p |dA gate_L| / (H W);
           B = u |v| + (1 + u) ((3 e |t| + B_d + e (|t| + |d|)) |GELU'(u)| + (|t| + |d|) (gpe(u) + e |GELU'(u)|))
  du{l-1}  the same with the convolution c in place of d:  B_c = (K^2 + 1) e sum |w| |du_l|
  dctx0    B = u |v| + (1 + u) (K^2 + 1) e sum |w| |du_0|
  dw{l}    n = B H W products:  B = (n + 2) e sum |du_l| |x_l| + sum |du_l| (u |ctx_{l-1}| + ge(u_{l-1})) (the last for l > 0)
  out, dq, dmod    one product, one store:  B = (u + 2 e) |v|

1e-30 is added to every bound so that exact zeros compare.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -8
E = 2.0 ** -24
TINY = 1e-30
BF = torch.bfloat16

CONFIGS = ((3, 5, False), (4, 3, True))      # (L, window, normalize): K = 5, 7, 9 and K = 3, 5, 7, 9 -- the named models' levels
# (B, H, W, C) of the GPU tests: a map smaller than every kernel; one pixel at a width of four groups; an odd map of width 96; one just past
# a 16 x 16 tile; the tile's edge, T - 1 and T + 1 in either direction, with one image and with two
SHAPES = ((2, 2, 3, 32), (2, 1, 1, 128), (2, 13, 9, 96), (1, 16, 17, 64), (1, 15, 17, 32), (2, 17, 15, 64))
WGRAD_SHAPE = (3, 17, 17, 4096)      # the weight gradient alone: parts of 3 (image, tile) pairs that cross from one image into the next

CONV_WRONG = ("taps_flipped", "clamp_to_edge", "halo_next_image")
FORWARD_WRONG = CONV_WRONG + ("gate_of_next_level", "global_term_dropped", "mean_over_batch", "normaliser_dropped")
BACKWARD_WRONG = CONV_WRONG + ("gelu_grad_dropped", "border_pixels_dropped")


def sizes(L, window):
    return tuple(window + 2 * l for l in range(L))


def same_function(wrong, shape, normalize=True):
    """True where a wrong variant is, mathematically, the right function: on a 1 x 1 map only the centre tap ever meets a pixel (flipping
    the taps keeps it in place); with one image the mean over the batch is the mean per image; without the normaliser none is dropped"""
    B, H, W, _ = shape
    return ((wrong == "taps_flipped" and H == 1 and W == 1) or (wrong == "mean_over_batch" and B == 1)
            or (wrong == "normaliser_dropped" and not normalize))


def affected(wrong, L):
    """the tensors a wrong variant changes"""
    if wrong in CONV_WRONG:
        return [f"u{l}" for l in range(L)] + [f"du{l}" for l in range(L - 1)] + ["dctx0"]
    return {"gate_of_next_level": ["A"], "global_term_dropped": ["A"], "normaliser_dropped": ["A"], "mean_over_batch": ["m"],
            "gelu_grad_dropped": [f"du{l}" for l in range(L)], "border_pixels_dropped": [f"dw{l}" for l in range(L)]}[wrong]


def rnd_bf16(t):
    return t.to(BF).to(t.dtype)


def cdf(x):
    return 0.5 * torch.erfc(-x * math.sqrt(0.5))


def pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gelu(x):
    return x * cdf(x)


def gelu_grad(x):
    return cdf(x) + x * pdf(x)


def ge(x):
    return (8 + x * x) * E * gelu(x).abs()


def gpe(x):
    return E * (8 * cdf(x) + (8 + 0.5 * x * x) * x.abs() * pdf(x))


# ---- the convolution and the weight gradient, any odd K --------------------------------------------------------------------------------
def _padded(x, K, wrong=None):
    """(B, H + K - 1, W + K - 1, C): zeros outside each image -- or what a wrong kernel would read there"""
    B, H, W, C = x.shape
    p = K // 2
    if wrong == "clamp_to_edge":
        return F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), mode="replicate").permute(0, 2, 3, 1)
    if wrong == "halo_next_image":      # the batch as one tall image (cyclic): rows above / below an image belong to its neighbours
        tall = x.reshape(B * H, W, C)
        rows = (torch.arange(-p, H + p)[None, :] + H * torch.arange(B)[:, None]) % (B * H)
        return F.pad(tall[rows], (0, 0, p, p))
    return F.pad(x, (0, 0, p, p, p, p))


def conv(x, w, K, flip=0, wrong=None):
    """x (B, H, W, C), w (K K, C) of one dtype -> (B, H, W, C), the taps added in tap order"""
    B, H, W, C = x.shape
    if wrong == "taps_flipped":
        flip = 1 - flip
    xp = _padded(x, K, wrong)
    acc = torch.zeros(B, H, W, C, dtype=x.dtype)
    for ky in range(K):
        for kx in range(K):
            t = K * ky + kx
            acc = acc + w[K * K - 1 - t if flip else t] * xp[:, ky:ky + H, kx:kx + W, :]
    return acc


def wgrad(dy, x, K, wrong=None):
    B, H, W, C = x.shape
    if wrong == "border_pixels_dropped":
        keep = torch.zeros(H, W, dtype=dy.dtype)
        keep[1:H - 1, 1:W - 1] = 1
        dy = dy * keep[None, :, :, None]
    xp = _padded(x, K)
    dw = torch.zeros(K * K, C, dtype=x.dtype)
    for ky in range(K):
        for kx in range(K):
            dw[K * ky + kx] = (dy * xp[:, ky:ky + H, kx:kx + W, :]).sum((0, 1, 2))
    return dw


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def make_inputs(shape, L, window, gen):
    """bf16 ctx0, gates (B, H, W, L + 1) and dA; fp32 weights [(K_l K_l, C)] with std 1 / K_l (the levels keep their scale)"""
    B, H, W, C = shape
    ctx0 = torch.randn(*shape, generator=gen).to(BF)
    gates = torch.randn(B, H, W, L + 1, generator=gen).to(BF)
    ws = [torch.randn(K * K, C, generator=gen) / K for K in sizes(L, window)]
    dA = torch.randn(*shape, generator=gen).to(BF)
    return ctx0, gates, ws, dA


def weight_form(ws):
    return torch.cat(ws, 0).contiguous()


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
def forward_emulate(ctx0, gates, ws, L, window, normalize):
    """fp32 with the kernels' roundings -> {"u0".., "m", "g", "A"} (u and A bf16 values in fp32).  GELU in the kernels' erfc form: torch's
    fp32 F.gelu forms 1 + erf, which cancels in the lower tail and is not what the bounds describe"""
    s = 1.0 / (L + 1) if normalize else 1.0
    out, x = {}, ctx0.float()
    for l, K in enumerate(sizes(L, window)):
        out[f"u{l}"] = rnd_bf16(conv(x, ws[l].float(), K))
        x = rnd_bf16(gelu(out[f"u{l}"]))      # the tile's rounding
    out["m"] = gelu(out[f"u{L - 1}"]).mean((1, 2))
    out["g"] = gelu(out["m"])
    acc = torch.zeros_like(x)
    for l in range(L):
        acc = acc + gates[..., l:l + 1].float() * gelu(out[f"u{l}"])
    acc = acc + gates[..., L:].float() * out["g"][:, None, None, :]
    out["A"] = rnd_bf16(torch.tensor(s, dtype=torch.float32) * acc)
    return out


def forward_reference(ctx0, gates, ws, L, window, normalize, stored, wrong=None):
    """``stored``: the u_l, m and g a run wrote (keys as forward_emulate's) -> (values, bounds), dicts of float64 tensors"""
    s = 1.0 / (L + 1) if normalize and wrong != "normaliser_dropped" else 1.0
    cw = wrong if wrong in CONV_WRONG else None
    val, bound = {}, {}
    gts = gates.double()
    for l, K in enumerate(sizes(L, window)):
        w = ws[l].double()
        if l == 0:
            x, pert = ctx0.double(), None
        else:
            up = stored[f"u{l - 1}"].double()
            x, pert = gelu(up), U * gelu(up).abs() + ge(up)
        v = conv(x, w, K, 0, cw)
        b = (K * K + 1) * E * conv(x.abs(), w.abs(), K)
        if pert is not None:
            b = b + conv(pert, w.abs(), K)
        val[f"u{l}"], bound[f"u{l}"] = v, U * v.abs() + (1 + U) * b + TINY
    ul = stored[f"u{L - 1}"].double()
    n = ul.shape[1] * ul.shape[2]
    ctx = gelu(ul)
    val["m"] = ctx.mean((0, 1, 2))[None].expand(ul.shape[0], -1) if wrong == "mean_over_batch" else ctx.mean((1, 2))
    bound["m"] = (n + 2) * E * ctx.abs().mean((1, 2)) + ge(ul).mean((1, 2)) + TINY
    m = stored["m"].double()
    val["g"], bound["g"] = gelu(m), ge(m) + TINY
    g = stored["g"].double()[:, None, None, :]
    acc, mag, err = 0, 0, 0
    for l in range(L):
        u = stored[f"u{l}"].double()
        gate = gts[..., (l + 1 if wrong == "gate_of_next_level" else l):][..., :1]
        acc = acc + gate * gelu(u)
        mag = mag + (gts[..., l:l + 1] * gelu(u)).abs()
        err = err + gts[..., l:l + 1].abs() * ge(u)
    if wrong != "global_term_dropped":
        acc = acc + gts[..., L:] * g
    mag = mag + (gts[..., L:] * g).abs()
    s_true = 1.0 / (L + 1) if normalize else 1.0
    val["A"] = s * acc
    bound["A"] = U * val["A"].abs() + (1 + U) * s_true * ((L + 3) * E * mag + err) + TINY
    return val, bound


# ---- backward -----------------------------------------------------------------------------------------------------------------------------
def backward_emulate(dA, ctx0, gates, ws, L, window, normalize, stored):
    """fp32 with the kernels' roundings from a forward's ``stored`` -> {"dgates", "du0".., "dctx0", "dw0"..}"""
    s = torch.tensor(1.0 / (L + 1) if normalize else 1.0, dtype=torch.float32)
    ks = sizes(L, window)
    d, gts = dA.float(), gates.float()
    us = [stored[f"u{l}"].float() for l in range(L)]
    m, g = stored["m"].float(), stored["g"].float()
    n = dA.shape[1] * dA.shape[2]
    out = {}
    dg = [s * (d * gelu(us[l])).sum(-1) for l in range(L)] + [s * (d * g[:, None, None, :]).sum(-1)]
    out["dgates"] = rnd_bf16(torch.stack(dg, -1))
    gg32 = lambda x: gelu_grad(x.double()).float()      # noqa: E731  (GELU' itself is not what the emulation probes)
    dmn = s * (d * gts[..., L:]).sum((1, 2)) * gg32(m) / n
    out[f"du{L - 1}"] = rnd_bf16((s * gts[..., L - 1:L] * d + dmn[:, None, None, :]) * gg32(us[L - 1]))
    for l in range(L - 1, 0, -1):
        c = conv(out[f"du{l}"], ws[l].float(), ks[l], 1)
        out[f"du{l - 1}"] = rnd_bf16((c + s * gts[..., l - 1:l] * d) * gg32(us[l - 1]))
    out["dctx0"] = rnd_bf16(conv(out["du0"], ws[0].float(), ks[0], 1))
    for l in range(L):
        x = ctx0.float() if l == 0 else rnd_bf16(gelu(us[l - 1]))
        out[f"dw{l}"] = wgrad(out[f"du{l}"], x, ks[l])
    return out


def backward_reference(dA, ctx0, gates, ws, L, window, normalize, stored, wrong=None, only=None):
    """``stored``: the forward's u_l, m, g and the backward's du_l -> (values, bounds); ``only``: a prefix of the keys to compute"""
    s = 1.0 / (L + 1) if normalize else 1.0
    cw = wrong if wrong in CONV_WRONG else None
    ks = sizes(L, window)
    d, gts = dA.double(), gates.double()
    us = [stored[f"u{l}"].double() for l in range(L)]
    dus = [stored[f"du{l}"].double() for l in range(L)]
    B, H, W, C = dA.shape
    n = H * W
    val, bound = {}, {}
    want = lambda k: only is None or k.startswith(only)      # noqa: E731

    def prime(u):
        return torch.ones_like(u) if wrong == "gelu_grad_dropped" else gelu_grad(u)

    if want("dgates"):
        g = stored["g"].double()[:, None, None, :]
        v = [s * (d * gelu(us[l])).sum(-1) for l in range(L)] + [s * (d * g).sum(-1)]
        b = [s * ((C + 3) * E * (d * gelu(us[l])).abs().sum(-1) + (d.abs() * ge(us[l])).sum(-1)) for l in range(L)]
        b.append(s * (C + 3) * E * (d * g).abs().sum(-1))
        val["dgates"] = torch.stack(v, -1)
        bound["dgates"] = U * val["dgates"].abs() + (1 + U) * torch.stack(b, -1) + TINY
    if want("du"):
        m = stored["m"].double()
        big = s * (d * gts[..., L:]).abs().sum((1, 2)) / n
        dmn = (s * (d * gts[..., L:]).sum((1, 2)) * gelu_grad(m) / n)[:, None, None, :]
        b_d = ((n + 5) * E * big * gelu_grad(m).abs() + big * gpe(m))[:, None, None, :]
        for l in range(L - 1, -1, -1):
            t = s * gts[..., l:l + 1] * d
            if l == L - 1:
                c, b_c = dmn, b_d
            else:
                K, w = ks[l + 1], ws[l + 1].double()
                c, b_c = conv(dus[l + 1], w, K, 1, cw), (K * K + 1) * E * conv(dus[l + 1].abs(), w.abs(), K)
            gp, gt = prime(us[l]), gelu_grad(us[l]).abs()
            both = t.abs() + c.abs()
            val[f"du{l}"] = (t + c) * gp
            bound[f"du{l}"] = U * val[f"du{l}"].abs() + (1 + U) * ((3 * E * t.abs() + b_c + E * both) * gt + both * (gpe(us[l]) + E * gt)) + TINY
    if want("dctx0"):
        K, w = ks[0], ws[0].double()
        v = conv(dus[0], w, K, 1, cw)
        val["dctx0"], bound["dctx0"] = v, U * v.abs() + (1 + U) * (K * K + 1) * E * conv(dus[0].abs(), w.abs(), K) + TINY
    if want("dw"):
        for l in range(L):
            if l == 0:
                x, pert = ctx0.double(), None
            else:
                x, pert = gelu(us[l - 1]), U * gelu(us[l - 1]).abs() + ge(us[l - 1])
            val[f"dw{l}"] = wgrad(dus[l], x, ks[l], wrong if wrong == "border_pixels_dropped" else None)
            mag = (B * n + 2) * E * x.abs()
            bound[f"dw{l}"] = wgrad(dus[l].abs(), mag if pert is None else mag + pert, ks[l]) + TINY
    return val, bound


# ---- the modulation product ---------------------------------------------------------------------------------------------------------------
def modulate_reference(q, mod, dout):
    q, mod, dout = q.double(), mod.double(), dout.double()
    val = {"out": q * mod, "dq": dout * mod, "dmod": dout * q}
    return val, {k: (U + 2 * E) * v.abs() + TINY for k, v in val.items()}


def modulate_emulate(q, mod, dout):
    q, mod, dout = q.float(), mod.float(), dout.float()
    return {"out": rnd_bf16(q * mod), "dq": rnd_bf16(dout * mod), "dmod": rnd_bf16(dout * q)}


def ratios(got, val, bound):
    """worst |got - want| / bound per tensor of `val` that `got` holds (inf for a NaN)"""
    res = {}
    for n in val:
        if got.get(n) is None:
            continue
        r = (got[n].double().cpu() - val[n]).abs() / bound[n]
        res[n] = float(torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r).max())
    return res


# ---- the torch bf16 composition the device tests compare with (the formulas, not the package's code) ---------------------------------------
def comp_modulation(P, pre, x, L, normalize, postln):
    """FocalModulation on (B, H, W, C) in the reference's NCHW order, parameters ``P[pre + name]``"""
    C = x.shape[-1]
    y = F.linear(x, P[pre + "f.weight"], P[pre + "f.bias"]).permute(0, 3, 1, 2).contiguous()
    q, ctx, gates = torch.split(y, (C, C, L + 1), 1)
    acc = 0
    for l in range(L):
        w = P[pre + f"focal_layers.{l}.0.weight"]
        ctx = F.gelu(F.conv2d(ctx, w, None, padding=w.shape[-1] // 2, groups=C))
        acc = acc + ctx * gates[:, l:l + 1]
    acc = acc + F.gelu(ctx.mean(2, keepdim=True).mean(3, keepdim=True)) * gates[:, L:]
    if normalize:
        acc = acc / (L + 1)
    out = (q * F.conv2d(acc, P[pre + "h.weight"], P[pre + "h.bias"])).permute(0, 2, 3, 1).contiguous()
    if postln:
        out = F.layer_norm(out, (C,), P[pre + "ln.weight"], P[pre + "ln.bias"], 1e-5)
    return F.linear(out, P[pre + "proj.weight"], P[pre + "proj.bias"])


def comp_block(P, pre, x, H, W, L, normalize, postln_in_modulation):
    """a post-LN block with layer scale on (B, H W, C)"""
    B, N, C = x.shape
    z = comp_modulation(P, pre + "modulation.", x.view(B, H, W, C), L, normalize, postln_in_modulation).reshape(B, N, C)
    x = x + P[pre + "gamma_1"] * F.layer_norm(z, (C,), P[pre + "norm1.weight"], P[pre + "norm1.bias"], 1e-5)
    z = F.linear(F.gelu(F.linear(x, P[pre + "mlp.fc1.weight"], P[pre + "mlp.fc1.bias"])), P[pre + "mlp.fc2.weight"], P[pre + "mlp.fc2.bias"])
    return x + P[pre + "gamma_2"] * F.layer_norm(z, (C,), P[pre + "norm2.weight"], P[pre + "norm2.bias"], 1e-5)


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_focalnet_reference.npz")) as z:
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
