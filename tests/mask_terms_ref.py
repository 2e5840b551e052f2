"""Float64 definitions of what csrc/mask_terms.hip computes (richsem_amd.masks: the mask terms of the criterion, their gradient, the mask
post-processor) with an ELEMENT-WISE error bound per output, wrong variants that must leave the bounds, and the loader of
tests/golden/mask_terms/mask_terms_reference.npz (in a directory of its own: every .npz directly under tests/golden is
taken for an operator fixture by the suite's collection).  Test helper only: the package never imports it.

    resize      A(in, out) (out x in): row d has 1 - l at i0 and l at i1, src = max(0, (d + 0.5) in / out - 0.5), i0 = floor(src),
                i1 = min(i0 + 1, in - 1), l = src - i0;  x = A_y P A_x^T on the (Hp, Wp) canvas
    focal       a_t ce m^2,  ce = softplus(x) - x t,  m = 1 - p_t = p + t - 2 p t,  a_t = alpha t + (1 - alpha)(1 - t)
    losses      loss_mask = sum_k (sum focal_k / (Hp Wp)) / nb,   loss_dice = sum_k (1 - (2 sum p t + 1) / (sum p + sum t + 1)) / nb
    gradient    G = g0 focal'(x) / (Hp Wp nb) + g1 dice'(p) p (1 - p) / nb,   grad P = A_y^T G A_x
    post        out[r, oy, ox] = sigmoid(x4[Y, X]) > thr,  Y = min(floor(oy ch / oh), ch - 1) in float32 (torch's nearest rule), (ch, cw) =
                (min(img_h, 4 h), min(img_w, 4 w)),  x4 = A(h, 4 h) P A(w, 4 w)^T

The bounds.  e = 2^-24 is the unit round-off of fp32, u = 2^-8 that of bf16; to first order.
  x           the kernels form scale, the source coordinate and the weights in fp32: three roundings on a number of size <= in, so a weight
              is off by at most d = 4 e in, per axis; the four products and three sums bring 6 e:  B_x = (4 e (h + w) + 6 e) M, M = the sum of
              the four corners' magnitudes
  focal       |focal'| B_x + a_t (dce m^2 + 2 ce m dm) + 4 e focal,  dce = 4 e (|x| (1 + t) + log1p) (expf and log1pf within 2 ulp, two sums),
              dm = 4 e (p + t + 2 p t) (p within 3 e p, two sums)
  sums        a lane adds DEPTH = 16 ceil(8 Wp / 4096) of its own elements, then 6 shuffle steps and 3 wave sums, all fp32: DEPTH + 9 roundings
              of a partial sum <= the sum of the magnitudes; the bands are added in fp64
  losses      the pairs' bounds added and divided as the losses are, + 2 e |loss| for the division and the fp32 store
  G           through x: max |G(x +- B_x) - G(x)|; its own arithmetic: the terms above pushed through focal' and dice', with the per-pair
              sums off by their bound + e (they are stored in fp32)
  gradient    A_y^T dG A_x, + the weights' error d on either axis times |G|, + (ny + nx + 3) e for the additions (ny, nx: the most canvas
              rows / columns a source pixel gathers from); a bf16 gradient is rounded once at its store: u |v| + (1 + u) B
1e-30 is added to every bound so that exact zeros compare.
"""
import os

import numpy as np

E = 2.0 ** -24
U = 2.0 ** -8
TINY = 1e-30
ALPHA = 0.25

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_terms", "mask_terms_reference.npz")

LOSS_WRONG = ("align_corners", "negative_not_clamped", "i1_not_clamped", "mean_over_own_mask", "canvas_not_rounded", "canvas_of_image",
              "dice_without_one", "alpha_on_wrong_class", "other_images_query", "range_short_y_first", "range_short_y_last",
              "range_short_x_first", "range_short_x_last")
POST_WRONG = ("round_to_nearest", "crop_after_resize", "greater_equal")

# where a wrong variant is, mathematically, the right function -- no bound can tell them apart there and the tests assert equality instead:
#   a 1 x 1 source has weight 1 on its only pixel whatever the coordinate (as long as i1 is clamped onto it); when down-sizing, the last
#   source coordinate stays below in - 1, so i1 is never clamped, and the first one is positive, so nothing is clamped at 0 either; the masks of s1x1 reach 32 x 32 unrounded, and on the 32 x 32 canvases every image's own canvas is the batch's: nothing to
#   tell apart; a case without pairs has no loss at all
SAME = {
    "align_corners": ("s1x1", "no_pair"),
    "negative_not_clamped": ("s1x1", "s40x40_down", "no_pair"),
    "i1_not_clamped": ("s40x40_down", "no_pair"),
    "mean_over_own_mask": ("no_pair",),
    "canvas_not_rounded": ("s1x1", "no_pair"),
    "canvas_of_image": ("s1x1", "s8x8_empty_image", "s40x40_down", "no_pair"),
    "dice_without_one": ("no_pair",),
    "alpha_on_wrong_class": ("no_pair",),
    "other_images_query": ("no_pair",),
    "range_short_y_first": ("no_pair",), "range_short_y_last": ("no_pair",), "range_short_x_first": ("no_pair",),
    "range_short_x_last": ("no_pair",),
}


def load_golden():
    z = np.load(GOLDEN)
    loss = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["loss_cases"].tolist()}
    post = {n: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(n + "/")} for n in z["post_cases"].tolist()}
    return loss, post


def round_up(v, m=32):
    return (int(v) + m - 1) // m * m


def resize_matrix(n_in, n_out, wrong=None):
    """-> (A (n_out, n_in) float64, B: 1 where A has an index) of torch's bilinear resize, align_corners=False"""
    A, B = np.zeros((n_out, n_in)), np.zeros((n_out, n_in))
    for d in range(n_out):
        if wrong == "align_corners":
            src = d * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            src = (d + 0.5) * n_in / n_out - 0.5
        if src < 0 and wrong != "negative_not_clamped":
            src = 0.0
        i0 = min(int(src), n_in - 1)      # (int() truncates towards zero: what a C cast does to an unclamped negative coordinate)
        l = src - i0
        A[d, i0] += 1 - l
        B[d, i0] = 1
        if i0 + 1 <= n_in - 1:
            A[d, i0 + 1] += l
            B[d, i0 + 1] = 1
        elif wrong != "i1_not_clamped":      # (the unclamped index reads past the map: that weight is lost)
            A[d, i0] += l
    return A, B


def _short(A, end):
    """the gather matrix of a backward whose range per source index is one canvas index short at its first / last end"""
    A = A.copy()
    for i in range(A.shape[1]):
        nz = np.nonzero(A[:, i])[0]
        if nz.size:
            A[nz[0] if end == "first" else nz[-1], i] = 0
    return A


def _elem(x, t, alpha, wrong=None):
    """focal element, p, and the magnitudes the bounds are built from"""
    e = np.exp(-np.abs(x))
    p = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    l1p = np.log1p(e)
    ce = np.maximum(x, 0) - x * t + l1p
    m = p + t - 2 * p * t
    at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else np.ones_like(x)
    if wrong == "alpha_on_wrong_class":
        at = alpha * (1 - t) + (1 - alpha) * t
    return dict(p=p, ce=ce, m=m, at=at, focal=at * ce * m * m, pq=p * (1 - p), Tce=np.abs(x) * (1 + t) + l1p, Tm=p + t + 2 * p * t)


def _dfocal(v, t):
    return v["at"] * v["m"] * ((v["p"] - t) * v["m"] + 2 * v["ce"] * (1 - 2 * t) * v["pq"])


def _G(x, t, alpha, c0, c1, num, den, wrong=None):
    v = _elem(x, t, alpha, wrong)
    return c0 * _dfocal(v, t) - c1 * (2 * t * den - num) / den ** 2 * v["pq"]


def pairs_of(case):
    """-> [(slot, image, query)] of a fixture case, slot order"""
    out, s = [], 0
    for b, c in enumerate(case["counts"].tolist()):
        for _ in range(c):
            if case["qot"][s] >= 0:
                out.append((s, b, int(case["qot"][s])))
            s += 1
    return out


def depth(Wp):
    return 16 * -(-8 * Wp // 4096) + 9


def mask_terms(case, alpha=ALPHA, wrong=None, canvas=None, out_dtype="f32"):
    """the losses and the gradient of a fixture case (its pred, masks, counts, qot, num_boxes, g) in float64, with their bounds: -> dict with
    loss_mask, loss_dice, grad and b_loss_mask, b_loss_dice, b_grad.  ``canvas``: the (larger) canvas of the buffers under test."""
    pred, g, nb = case["pred"].astype(np.float64), case["g"].astype(np.float64), float(case["num_boxes"])
    N, Q, h, w = pred.shape
    Hp, Wp = (int(v) for v in (case["canvas"] if canvas is None else canvas))
    own = case["mask_hw"]
    if wrong == "canvas_not_rounded":
        Hp, Wp = int(own[:, 0].max()), int(own[:, 1].max())
    lm = ld = b_lm = b_ld = 0.0
    grad, b_grad = np.zeros_like(pred), np.zeros_like(pred)
    for s, b, q in pairs_of(case):
        hp, wp = Hp, Wp
        if wrong == "canvas_of_image":
            hp, wp = round_up(own[b, 0]), round_up(own[b, 1])
        t = np.zeros((hp, wp))
        src_t = case["masks"][s].astype(np.float64)
        t[:min(hp, src_t.shape[0]), :min(wp, src_t.shape[1])] = src_t[:hp, :wp]
        Ay, By = resize_matrix(h, hp, wrong)
        Ax, Bx_ = resize_matrix(w, wp, wrong)
        P = pred[(b + 1) % N if wrong == "other_images_query" else b, q]
        x = Ay @ P @ Ax.T
        bx = (4 * E * (h + w) + 6 * E) * (By @ np.abs(P) @ Bx_.T)
        v = _elem(x, t, alpha, wrong)
        area = float(own[b, 0] * own[b, 1]) if wrong == "mean_over_own_mask" else float(hp * wp)
        one = 0.0 if wrong == "dice_without_one" else 1.0
        S = [v["focal"].sum(), (v["p"] * t).sum(), v["p"].sum(), t.sum()]
        num, den = 2 * S[1] + one, S[2] + S[3] + one
        lm += S[0] / area / nb
        ld += (1 - num / den) / nb
        # ---- bounds of the sums
        D = depth(wp)
        dfoc = np.abs(_dfocal(v, t))
        b_focal = dfoc * bx + v["at"] * (4 * E * v["Tce"] * v["m"] ** 2 + 8 * E * v["ce"] * v["m"] * v["Tm"]) + 4 * E * v["focal"]
        bS0 = b_focal.sum() + D * E * S[0]
        b_p = v["pq"] * bx + 3 * E * v["p"]
        bS2 = b_p.sum() + D * E * S[2]
        bS1 = (b_p * t).sum() + D * E * S[1]
        b_lm += bS0 / area / nb
        b_ld += (2 * bS1 / den + num * bS2 / den ** 2) / nb
        # ---- gradient
        c0, c1 = g[0] / (area * nb), g[1] / nb
        G = _G(x, t, alpha, c0, c1, num, den, wrong)
        Gy = _short(Ay, wrong.rsplit("_", 1)[1]) if wrong and wrong.startswith("range_short_y") else Ay
        Gx = _short(Ax, wrong.rsplit("_", 1)[1]) if wrong and wrong.startswith("range_short_x") else Ax
        grad[b, q] += Gy.T @ G @ Gx
        dGx = 1.01 * np.maximum(np.abs(_G(x + bx, t, alpha, c0, c1, num, den) - G), np.abs(_G(x - bx, t, alpha, c0, c1, num, den) - G))
        dm, dce = 4 * E * v["Tm"], 4 * E * v["Tce"]
        d_dfocal = v["at"] * (dm * (2 * v["m"] * np.abs(v["p"] - t) + 2 * v["ce"] * v["pq"])
                              + v["m"] * (v["m"] * 4 * E * (v["p"] + t) + 2 * (dce * v["pq"] + v["ce"] * 4 * E * v["pq"]))) + 6 * E * dfoc
        dnum, dden = 2 * bS1 + E * num, bS2 + E * den
        ddice = np.abs(2 * t * den - num) / den ** 2 * v["pq"]
        d_ddice = v["pq"] * ((2 * t * dden + dnum) / den ** 2 + 2 * np.abs(2 * t * den - num) * dden / den ** 3
                             + 3 * E * (2 * t * den + num) / den ** 2) + 8 * E * ddice
        dG = dGx + abs(c0) * d_dfocal + abs(c1) * d_ddice + 3 * E * (abs(c0) * dfoc + abs(c1) * ddice)
        ny, nx = int((Ay != 0).sum(0).max()), int((Ax != 0).sum(0).max())
        aG = np.abs(G)
        b_grad[b, q] += (Ay.T @ dG @ Ax + 4 * E * h * (By.T @ aG @ Ax) + 4 * E * w * (Ay.T @ aG @ Bx_) + (ny + nx + 3) * E * (Ay.T @ aG @ Ax))
    b_lm += 2 * E * abs(lm)
    b_ld += 2 * E * abs(ld)
    if out_dtype == "bf16":
        b_grad = U * np.abs(grad) + (1 + U) * b_grad
    return dict(loss_mask=lm, loss_dice=ld, grad=grad, b_loss_mask=b_lm + TINY, b_loss_dice=b_ld + TINY, b_grad=b_grad + TINY)


def leaves_bounds(right, other):
    """does ``other`` (a wrong variant, or a kernel's result) leave the bounds of ``right`` somewhere?"""
    return bool(abs(other["loss_mask"] - right["loss_mask"]) > right["b_loss_mask"] or abs(other["loss_dice"] - right["loss_dice"]) > right["b_loss_dice"]
                or (np.abs(np.asarray(other["grad"], dtype=np.float64) - right["grad"]) > right["b_grad"]).any())


# ---- post-processor -----------------------------------------------------------------------------------------------------------------------
def _nearest(n_in, n_out, wrong=None):
    scale = np.float32(n_in) / np.float32(n_out)      # torch's nearest rule, in float32 as torch computes it
    d = np.arange(n_out, dtype=np.float32) * scale
    idx = np.floor(d + np.float32(0.5)) if wrong == "round_to_nearest" else np.floor(d)
    return np.minimum(idx.astype(np.int64), n_in - 1)


def postprocess(pred, max_sizes, orig_sizes, threshold, items=None, wrong=None):
    """-> per image (mask uint8 (rows, 1, oh, ow), near (same shape, bool): the pixels whose float64 logit lies within
    8 e sum |weight value| of the threshold's logit -- the ones a float32 evaluation may decide either way)"""
    pred = np.asarray(pred, dtype=np.float64)
    N, Q, h, w = pred.shape
    Ay, _ = resize_matrix(h, 4 * h)
    Ax, _ = resize_matrix(w, 4 * w)
    cut = np.log(threshold / (1 - threshold))
    out = []
    for n in range(N):
        rows = np.arange(Q) if items is None else np.asarray(items[n], dtype=np.int64)
        P = pred[n][rows]
        x4 = np.einsum("yi,rij,xj->ryx", Ay, P, Ax)
        mag = np.einsum("yi,rij,xj->ryx", Ay, np.abs(P), Ax)
        img_h, img_w = (int(v) for v in max_sizes[n])
        oh, ow = (int(v) for v in orig_sizes[n])
        if wrong == "crop_after_resize":
            iy, ix = _nearest(4 * h, oh), _nearest(4 * w, ow)
            x, m = np.full((len(rows), oh, ow), -np.inf), np.zeros((len(rows), oh, ow))
            ch, cw = min(img_h, oh), min(img_w, ow)
            x[:, :ch, :cw] = x4[:, iy][:, :, ix][:, :ch, :cw]
        else:
            ch, cw = min(img_h, 4 * h), min(img_w, 4 * w)
            iy, ix = _nearest(ch, oh, wrong), _nearest(cw, ow, wrong)
            x, m = x4[:, iy][:, :, ix], mag[:, iy][:, :, ix]
        p = 1 / (1 + np.exp(-x))
        hit = p >= threshold if wrong == "greater_equal" else p > threshold
        out.append((hit.astype(np.uint8)[:, None], (np.abs(x - cut) <= 8 * E * m)[:, None]))
    return out
