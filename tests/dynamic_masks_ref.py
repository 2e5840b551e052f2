"""Float64 definition of what csrc/dynamic_masks.hip computes (richsem_amd.cond_inst: the CondInst dynamic mask head and its gradients) with an
ELEMENT-WISE error bound per output, wrong variants that must leave the bounds, the ReLU margin condition on the inputs, and the loader of
tests/golden/dynamic_masks/dynamic_masks_reference.npz (in a directory of its own: every .npz directly under tests/golden is taken for an
operator fixture by the suite's collection).  Test helper only: the package never imports it.

A case is a dict: ``feats`` (N, C, H, W), ``params`` (N, Q, P), ``ref`` (N, Q, 4) normalised (x, y, w, h), ``sizes`` (N, 2) = (height, width),
``inst`` (N, R) the query of every output row (-1: none), ``rel`` 0 / 1, ``factor`` 1 / 2, ``gout`` (N, R, F H, F W) the cotangent.

    in    = [rx, ry, feats[n, :, y, x]],  rx = ref_x size_w - (8 x + 4),  ry = ref_y size_h - (8 y + 4)      (rel = 0: the features alone)
    z0    = W0 in + b0,  h0 = relu(z0),  z1 = W1 h0 + b1,  h1 = relu(z1),  t = w2 . h1 + b2
    row   = W0 (8, Cin) row-major, W1 (8, 8), w2 (8), b0 (8), b1 (8), b2 (1)
    out   = U t U^T per map, U (F H x H): F[0] = T[0], F[2 k + 1] = T[k], F[2 k] = (T[k - 1] + T[k]) / 2
    back  dt = U^T gout U;  dz1 = [z1 > 0] dt w2;  dz0 = [z0 > 0] W1^T dz1;  din = W0^T dz0
          grad_params = the sums over the pixels of the outer products, grad_feats = the sum over the image's rows of din[2:],
          grad_ref = (size_w, size_h) * the sum over the pixels of din[0:2]

The bounds.  e = 2^-24 is the unit round-off of fp32, u = 2^-8 that of bf16; to first order.  The inputs are exact in the kernels' storage type.
  rx, ry     the product and the difference are rounded one after the other: B_c = e (|ref size| + |rx|)
  z0         a chain of Cin fused multiply-adds onto the bias: (Cin + 1) e (|W0| |in| + |b0|) + |W0[:, :2]| B_c
  z1, t      9 e (|W| |h| + |b|) + |W| B_h: the running error goes through |W| and the 1-Lipschitz ReLU
  out        U B_t U^T + 3 e U |t| U^T: the halves are exact, a corner takes three additions
  dt         nine taps: 10 e U^T |gout| U
  dz1, dz0, din   as forward, with the masks of the float64 pre-activations (see the margin below)
  sums       a sum of n terms added in a tree or chain of depth d: d e sum |terms| + the terms' own bounds.  Parameter gradients: d = 6 (the
             lanes' butterfly) + 3 (the waves) + the tiles of 8 x 32 pixels + 1; grad_feats: d = the image's live rows
  bf16       an output stored in bf16 is rounded once: u |v| + (1 + u) B
1e-30 is added to every bound so that exact zeros compare.

The ReLU margin.  The masks of the backward depend on the sign of an fp32 pre-activation, so the gradient bounds hold only where no
pre-activation is within its forward bound of zero.  ``margin`` returns the smallest |z| / B_z over every pre-activation of every live row
and pixel; the inputs of every test are drawn (``synthetic`` and the fixture's generator redraw the seed) until it exceeds MARGIN = 4.
"""
import os

import numpy as np

E = 2.0 ** -24
U = 2.0 ** -8
TINY = 1e-30
MARGIN = 4.0
HID = 8

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynamic_masks", "dynamic_masks_reference.npz")

WRONG = ("bias_before_weight", "w0_transposed", "features_before_coords", "pixel_minus_instance", "offset_missing", "xy_swapped",
         "align_corners_false", "upsample_shifted", "relu2_missing")

# where a wrong variant is, mathematically, the right function -- no bound can tell them apart there and the tests assert equality instead.
# The tags of a case (``tags``): "empty" no live row, so every output is zero; "rel_off" no coordinates in the input vector; "factor1" no
# up-sampling; "map1x1" a 1 x 1 map, whose x2 map holds T[0] four times under every rule.
SAME = {
    "bias_before_weight": ("empty",),
    "w0_transposed": ("empty",),
    "features_before_coords": ("empty", "rel_off"),
    "pixel_minus_instance": ("empty", "rel_off"),
    "offset_missing": ("empty", "rel_off"),
    "xy_swapped": ("empty", "rel_off"),
    "align_corners_false": ("empty", "factor1", "map1x1"),
    "upsample_shifted": ("empty", "factor1", "map1x1"),
    "relu2_missing": ("empty",),
}


def load_golden():
    """-> (dynamic cases, branch cases): name -> dict of arrays"""
    z = np.load(GOLDEN)
    pick = lambda n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")}      # noqa: E731
    return {n: pick(n) for n in z["dynamic_cases"].tolist()}, {n: dict(pick("branch_in"), **pick(n)) for n in z["branch_cases"].tolist()}


def load_branch_weights():
    """the state dict of the fixture's ``MaskBranch(32, channel_div=8)``: key -> float32 array"""
    z = np.load(GOLDEN)
    return {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("branch_sd/")}


def tags(case):
    N, C, H, W = case["feats"].shape
    out = set()
    if not (case["inst"] >= 0).any():
        out.add("empty")
    if not int(case["rel"]):
        out.add("rel_off")
    if int(case["factor"]) == 1:
        out.add("factor1")
    if H == 1 and W == 1:
        out.add("map1x1")
    return out


def is_same(variant, case):
    return bool(tags(case) & set(SAME[variant]))


def num_params(C, rel):
    return HID * (C + 2 * int(rel)) + HID * HID + 3 * HID + 1


def split_params(p, cin, variant=None):
    """a parameter row -> W0 (8, cin), W1 (8, 8), w2 (8), b0 (8), b1 (8), b2 ()"""
    sizes = [HID * cin, HID * HID, HID, HID, HID, 1]
    order = [3, 4, 5, 0, 1, 2] if variant == "bias_before_weight" else [0, 1, 2, 3, 4, 5]
    parts, o = {}, 0
    for k in order:
        parts[k] = p[o:o + sizes[k]]
        o += sizes[k]
    W0 = parts[0].reshape(cin, HID).T if variant == "w0_transposed" else parts[0].reshape(HID, cin)
    return W0, parts[1].reshape(HID, HID), parts[2], parts[3], parts[4], parts[5][0]


def up_matrix(n, factor, variant=None):
    """U (factor n x n) of aligned_bilinear along one axis"""
    if factor == 1:
        return np.eye(n)
    Um = np.zeros((2 * n, n))
    if variant == "align_corners_false":      # F.interpolate(scale_factor=2, mode="bilinear", align_corners=False)
        for d in range(2 * n):
            s = max((d + 0.5) / 2 - 0.5, 0.0)
            i0 = min(int(np.floor(s)), n - 1)
            i1 = min(i0 + 1, n - 1)
            Um[d, i0] += 1 - (s - i0)
            Um[d, i1] += s - i0
        return Um
    for k in range(n):
        Um[2 * k + 1, k] = 1.0
        Um[2 * k, k] += 0.5
        Um[2 * k, max(k - 1, 0)] += 0.5
    if variant == "upsample_shifted":      # the left replicate pad missing: F'[j] = F[j + 1]
        Um = np.concatenate([Um[1:], Um[-1:]])
    return Um


def coords(case, n, q, variant=None):
    """-> (rx, ry (H, W), their bound B_c (2, H, W))"""
    H, W = case["feats"].shape[-2:]
    off = 0.0 if variant == "offset_missing" else 4.0
    xs, ys = 8.0 * np.arange(W) + off, 8.0 * np.arange(H) + off
    ref, (sh, sw) = case["ref"][n, q], case["sizes"][n]
    lx, ly = (ref[0] * sw, ref[1] * sh) if variant != "xy_swapped" else (ref[1] * sh, ref[0] * sw)
    rx = np.broadcast_to(lx - xs[None, :], (H, W))
    ry = np.broadcast_to(ly - ys[:, None], (H, W))
    if variant == "pixel_minus_instance":
        rx, ry = -rx, -ry
    B = E * np.stack([abs(lx) + np.abs(rx), abs(ly) + np.abs(ry)])
    return rx, ry, B


def tiles_of(H, W):
    return ((H + 7) // 8) * ((W + 31) // 32)


def dynamic_masks(case, out_dtype="f32", variant=None, grads=True):
    """the definition in float64 -> dict: out, b_out, and with ``grads`` g_feats, g_params, g_ref (N, Q, 2) with b_*; ``margin`` the smallest
    |z| / B_z over every pre-activation"""
    feats, params, inst = case["feats"].astype(np.float64), case["params"].astype(np.float64), case["inst"]
    rel, F = int(case["rel"]), int(case["factor"])
    N, C, H, W = feats.shape
    Q, R = params.shape[1], inst.shape[1]
    cin = C + 2 * rel
    Uy, Ux = up_matrix(H, F, variant), up_matrix(W, F, variant)
    Uy0, Ux0 = up_matrix(H, F), up_matrix(W, F)
    out, b_out = np.zeros((N, R, F * H, F * W)), np.full((N, R, F * H, F * W), TINY)
    res = {"margin": np.inf}
    if grads:
        gout = case["gout"].astype(np.float64)
        gf, bf = np.zeros_like(feats), np.full(feats.shape, TINY)
        gp, bp = np.zeros_like(params), np.full(params.shape, TINY)
        gr, br = np.zeros((N, Q, 2)), np.full((N, Q, 2), TINY)
        depth = 6 + 3 + tiles_of(H, W) + 1
    for n in range(N):
        live = [(r, int(inst[n, r])) for r in range(R) if 0 <= inst[n, r] < Q]
        for r, q in live:
            W0, W1, w2, b0, b1, b2 = split_params(params[n, q], cin, variant)
            if rel:
                rx, ry, Bc = coords(case, n, q, variant)
                x_in = np.concatenate([feats[n], rx[None], ry[None]]) if variant == "features_before_coords" else \
                    np.concatenate([rx[None], ry[None], feats[n]])
                B_in = np.concatenate([Bc, np.zeros_like(feats[n])])
            else:
                x_in, B_in = feats[n], np.zeros_like(feats[n])
            aW0, aW1, aw2 = np.abs(W0), np.abs(W1), np.abs(w2)
            z0 = np.einsum("ic,chw->ihw", W0, x_in) + b0[:, None, None]
            B0 = (cin + 1) * E * (np.einsum("ic,chw->ihw", aW0, np.abs(x_in)) + np.abs(b0)[:, None, None]) + np.einsum("ic,chw->ihw", aW0, B_in)
            h0 = np.maximum(z0, 0)
            z1 = np.einsum("ji,ihw->jhw", W1, h0) + b1[:, None, None]
            B1 = 9 * E * (np.einsum("ji,ihw->jhw", aW1, h0) + np.abs(b1)[:, None, None]) + np.einsum("ji,ihw->jhw", aW1, B0)
            h1 = z1 if variant == "relu2_missing" else np.maximum(z1, 0)
            t = np.einsum("j,jhw->hw", w2, h1) + b2
            Bt = 9 * E * (np.einsum("j,jhw->hw", aw2, np.abs(h1)) + abs(b2)) + np.einsum("j,jhw->hw", aw2, B1)
            res["margin"] = min(res["margin"], float((np.abs(z0) / (B0 + TINY)).min()), float((np.abs(z1) / (B1 + TINY)).min()))
            out[n, r] = Uy @ t @ Ux.T
            b_out[n, r] += Uy0 @ Bt @ Ux0.T + (3 * E * (Uy0 @ np.abs(t) @ Ux0.T) if F == 2 else 0.0)
            if not grads:
                continue
            dt = Uy.T @ gout[n, r] @ Ux
            Bdt = 10 * E * (Uy0.T @ np.abs(gout[n, r]) @ Ux0) if F == 2 else np.zeros_like(dt)
            m1, m0 = (z1 > 0), (z0 > 0)
            dz1 = m1 * dt[None] * w2[:, None, None]
            Bz1 = m1 * (aw2[:, None, None] * Bdt[None] + E * np.abs(dz1))
            dh0 = np.einsum("ji,jhw->ihw", W1, dz1)
            dz0 = m0 * dh0
            Bz0 = m0 * (9 * E * np.einsum("ji,jhw->ihw", aW1, np.abs(dz1)) + np.einsum("ji,jhw->ihw", aW1, Bz1))
            din = np.einsum("ic,ihw->chw", W0, dz0)
            Bdin = 9 * E * np.einsum("ic,ihw->chw", aW0, np.abs(dz0)) + np.einsum("ic,ihw->chw", aW0, Bz0)

            def summed(a, Ba, b, Bb):      # sum over the pixels of the outer product a (k, H, W) x b (c, H, W) -> (k, c) and its bound
                v = np.einsum("khw,chw->kc", a, b)
                mag = np.einsum("khw,chw->kc", np.abs(a), np.abs(b))
                own = np.einsum("khw,chw->kc", Ba, np.abs(b)) + np.einsum("khw,chw->kc", np.abs(a), Bb)
                return v, own + (depth + 1) * E * mag

            one, zero = np.ones((1, H, W)), np.zeros((1, H, W))
            gW0, bW0 = summed(dz0, Bz0, x_in, B_in)
            gW1, bW1 = summed(dz1, Bz1, h0, B0)
            gw2, bw2 = summed(dt[None], Bdt[None], h1, B1)
            gb0, bb0 = summed(dz0, Bz0, one, zero)
            gb1, bb1 = summed(dz1, Bz1, one, zero)
            gb2, bb2 = summed(dt[None], Bdt[None], one, zero)
            gp[n, q] += np.concatenate([v.reshape(-1) for v in (gW0, gW1, gw2, gb0, gb1, gb2)])
            bp[n, q] += np.concatenate([v.reshape(-1) for v in (bW0, bW1, bw2, bb0, bb1, bb2)])
            gf[n] += din[2 * rel:]
            bf[n] += Bdin[2 * rel:] + len(live) * E * np.abs(din[2 * rel:])
            if rel:
                wh = np.array([case["sizes"][n][1], case["sizes"][n][0]], dtype=np.float64)
                # the reference's relative coordinates are a float32 tensor (its .float()), so autograd rounds their gradient to float32 pixel
                # by pixel before it sums: restated as it is, and one more e |din| per pixel in the bound
                s = din[:2].astype(np.float32).astype(np.float64).sum(axis=(1, 2))
                gr[n, q] += wh * s
                br[n, q] += wh * (Bdin[:2].sum(axis=(1, 2)) + (depth + 1) * E * np.abs(din[:2]).sum(axis=(1, 2))) + 2 * E * np.abs(wh * s)
    res.update(out=out, b_out=b_out)
    if grads:
        res.update(g_feats=gf, b_g_feats=bf, g_params=gp, b_g_params=bp, g_ref=gr, b_g_ref=br)
    if out_dtype == "bf16":      # grad_ref stays fp32
        for k in ("out", "g_feats", "g_params"):
            if k in res:
                res["b_" + k] = U * np.abs(res[k]) + (1 + U) * res["b_" + k]
    return res


def bf16_exact(a):
    """round a float array to the nearest bfloat16 (ties to even), returned as float64"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) << 16
    return bits.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(a))


def draw(rng, C, H, W, Q, inst, rel, factor, N=None):
    """one draw of a case: bf16-exact features, parameters and cotangent; reference points and sizes whose products are multiples of 1 / 8"""
    inst = np.asarray(inst, dtype=np.int64)
    N = inst.shape[0]
    sizes = np.stack([8.0 * rng.integers(max(H, 2), 2 * max(H, 2) + 1, N), 8.0 * rng.integers(max(W, 2), 2 * max(W, 2) + 1, N)], axis=1)
    ref = rng.integers(1, 64, (N, Q, 4)) / 64.0      # (k / 64) * (8 m) = k m / 8: exact in fp32
    return {"feats": bf16_exact(rng.standard_normal((N, C, H, W))), "params": bf16_exact(0.5 * rng.standard_normal((N, Q, num_params(C, rel)))),
            "ref": ref, "sizes": sizes, "inst": inst, "rel": np.int64(rel), "factor": np.int64(factor),
            "gout": bf16_exact(rng.standard_normal((N, inst.shape[1], factor * H, factor * W)))}


def synthetic(C, H, W, Q, inst, rel=1, factor=2, seed=0):
    """a case in the fixture's format (without results) whose pre-activations keep the ReLU margin: the seed is redrawn until they do"""
    for attempt in range(200):
        case = draw(np.random.default_rng([seed, attempt]), C, H, W, Q, inst, rel, factor)
        if dynamic_masks(case, grads=False)["margin"] > MARGIN:
            return case
    raise RuntimeError("no draw keeps the ReLU margin")
