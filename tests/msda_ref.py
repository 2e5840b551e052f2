"""Float64 restatement of MSDeformAttn forward and backward with an ELEMENT-WISE error bound for each of the four outputs, the input
recipe and the exact-operand probes of tests/test_gpu_msda_bounds.py (the kernels against the bounds) and tests/test_msda_ref.py (the
float32 evaluation and the C oracle against the bounds; wrong variants far outside them).  Test helper only; reads nothing but its
arguments.

The operation (header of richsem_amd/csrc/msda_common.h), per (image b, query q, head m), level l of (H, W), point p:

    h_im = loc_y H - 0.5,  w_im = loc_x W - 0.5;      the sample is DROPPED unless  h_im > -1 && w_im > -1 && h_im < H && w_im < W
    h_low = floor(h_im), lh = h_im - h_low, hh = 1 - lh  (w alike);   corners c = (h_low | h_low + 1, w_low | w_low + 1), each read only
    if inside [0, H) x [0, W), weights w_c = hh hw, hh lw, lh hw, lh lw
    out[b, q, m, d]         = sum_{l, p} aw sum_c w_c v_c[d]
    grad_aw[b, q, m, l, p]  = sum_d go[d] sum_c w_c v_c[d]
    grad_loc[..., (x, y)]   = (W, H) aw sum_d go[d] sum_c (dw_c/dlw, dw_c/dlh) v_c[d]
    grad_value[pixel c, d] += aw w_c go[d]

The bounds.  u is the unit round-off of the compute type (2^-24 for f32 and for bf16 storage, whose arithmetic is fp32; 2^-53 for f64).
Every bound is   gamma(R) * (sum of the absolute values of the terms added into the element)   +   location term   [+ storage term],
gamma(R) = R u / (1 - R u), R = the roundings on the longest path from the inputs to the element in ANY summation order:

  R_OUT  = 4 L P + 4     a term aw w_c v_c: 1 - lh and 1 - lw (2), their product (1), times aw (1), times v_c (1) = 5; then at most
                         4 L P - 1 additions (four corners, L P points; any order, any split over lanes)
  R_AW   = D + 7         a term go_d w_c v_c: the two differences (2), w_c (1), times v_c (1), three corner additions (3), times go_d (1),
                         D - 1 additions over the channels (sequential, by shuffles, or as the routed kernel's corner dots)
  R_LOC  = D + 8         a term (W | H) aw go_d dw_c v_c: 1 - lw (1), a corner difference / addition (<= 3), the product (1), go_d aw (1),
                         their product (1), times H or W (1), D - 1 additions; + 1 where a kernel multiplies aw into the fraction first
                         (msda_rps.h RpsEnt::hwa / lwa)
  R_GV   = n + 5         a contribution aw w_c go_d: differences (2), w_c (1), go_d aw (1), the product (1) = 5; n = the number of
                         contributions to that pixel (a scatter of ones): n - 1 additions in whatever order the atomics land, + 1 for
                         the bf16 path's fp32 image that is read back

Location term.  h_im is formed in the compute type: the product loc_y H rounds (u |loc_y H|), the difference rounds (u |h_im|); a kernel
that rebases to a window origin rounds once more (u |h_im|); and lh = h_im - floor(h_im) is exact for h_im >= 0 but rounds for
-1 < h_im < 0 (msda_common.h resolve_point, `lh = h_im - hf`: h_im + 1 needs up to two more bits than h_im has), u lh:
    d_h = u (|loc_y H| + 2 |h_im| + [h_im < 0] lh)          (w alike)
propagated to first order through the bilinear weights (dw_c/dlh = -hw, -lw, hw, lw; dw_c/dlw = -hh, hh, -lh, lh; d2w_c/dlh dlw = +-1):
    out, grad_aw   d_h sum_c |dw_c/dlh v_c| + d_w sum_c |dw_c/dlw v_c|      (times |aw|, summed over the points / times |go_d|, summed over d)
    grad_loc.y     d_w H |aw| sum_d |go_d| sum_c |v_c|                       (.x: d_h W ...)
    grad_value     |aw go_d| (d_h |dw_c/dlh| + d_w |dw_c/dlw|)               per contribution

Storage term, bf16 only: out and grad_value are rounded once at the store, 2^-8 (|ref| + bound).  bf16 keeps 8 significant bits: half an
ulp of a number in [2^k, 2^(k+1)) is 2^(k-8), so the unit round-off of the store is 2^-8 -- not 2^-9, which the correctly rounded fp32
sum itself misses by up to a factor 2 (1 + 2^-8 is stored as 1 or as 1 + 2^-7; tests/test_msda_ref.py holds that).  That term is far above the
fp32 ones, so bf16 stores are also held to the sharper, monotone form: stored_interval() below.

An element nothing is added into (every sample dropped; a pixel nobody touched) has bound 0: exactly 0 is asked for.  The first-order
propagation holds because make_inputs() keeps every sampling position 2^-10 of a pixel away from every integer (floor() and the drop test
then decide alike in f32 and f64) -- d_h is below 2^-16 of a pixel at the sizes tested.
"""
import numpy as np
import torch

from richsem_amd import workload as W

U32, U64 = 2.0 ** -24, 2.0 ** -53
U_BF16 = 2.0 ** -8      # unit round-off of a bf16 store (8 significant bits)
OUTPUTS = ("out", "grad_value", "grad_loc", "grad_aw")
# wrong restatements: the bounds must tell every one of them apart (tests/test_msda_ref.py); a kernel has one code path per output
# group, so each error sits where one kernel would have it
MUTANTS = (
    "fwd_aw_coarse",          # forward: attention weight of the coarsest level times (1 - 2^-6)
    "fwd_corner_coarse",      # forward: corner weight lh lw of the coarsest level times (1 + 2^-6)
    "bwd_corner_coarse",      # backward: the same corner weight, in grad_value / grad_aw
    "gloc_y_coarse",          # backward: grad_loc.y of the coarsest level times (1 + 2^-6)
    "border_corner_dropped",  # every output: the corner row h_high = H - 1 treated as outside the map (h_high < H - 1)
    "bf16_sum",               # bf16 storage: the forward sum kept in bf16 between points instead of fp32
)
_CORNERS = ((0, 0), (0, 1), (1, 0), (1, 1))


def _gamma(r, u):
    return r * u / (1.0 - r * u)


def _bf16(x):
    return x.float().to(torch.bfloat16).to(x.dtype)


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a).to(dtype)


def evaluate(value, shapes, lsi, loc, aw, grad_out, dtype=torch.float64, mutant=None, bounds=None):
    """The restatement in ``dtype`` (float64: the reference; float32: the "honest float32 run").  bounds: None, or "f32" / "f64" /
    "bf16" -- the storage type whose kernels the bounds are for (computed in float64 whatever ``dtype``).  -> dict of the four outputs as
    numpy arrays of ``dtype`` and, with bounds, a second dict of float64 arrays."""
    assert mutant in (None,) + MUTANTS
    value, loc, aw, go = (_t(a, dtype) for a in (value, loc, aw, grad_out))
    shapes = [(int(h), int(w)) for h, w in np.asarray(shapes)]
    lsi = [int(s) for s in np.asarray(lsi)]
    N, S, M, D = value.shape
    Lq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    go = go.reshape(N, Lq, M, D)
    f64 = torch.float64
    u = {"f32": U32, "bf16": U32, "f64": U64, None: 0.0}[bounds]
    nb = torch.arange(N).view(N, 1, 1, 1)
    mb = torch.arange(M).view(1, 1, M, 1)

    out = torch.zeros(N, Lq, M, D, dtype=dtype)
    g_val = torch.zeros(N * S * M, D, dtype=dtype)
    g_loc = torch.zeros(N, Lq, M, L, P, 2, dtype=dtype)
    g_aw = torch.zeros(N, Lq, M, L, P, dtype=dtype)
    B = None
    if bounds:
        B = dict(out_abs=torch.zeros(N, Lq, M, D, dtype=f64), out_loc=torch.zeros(N, Lq, M, D, dtype=f64),
                 gv_abs=torch.zeros(N * S * M, D, dtype=f64), gv_loc=torch.zeros(N * S * M, D, dtype=f64),
                 gv_n=torch.zeros(N * S * M, dtype=f64), grad_loc=torch.zeros(N, Lq, M, L, P, 2, dtype=f64),
                 grad_aw=torch.zeros(N, Lq, M, L, P, dtype=f64))
    for l, (H, Wd) in enumerate(shapes):
        coarse = l == L - 1
        x, y, a = loc[:, :, :, l, :, 0], loc[:, :, :, l, :, 1], aw[:, :, :, l, :]            # (N, Lq, M, P)
        h_im, w_im = y * H - 0.5, x * Wd - 0.5
        keep = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < Wd)
        hf, wf = torch.floor(h_im), torch.floor(w_im)
        lh, lw = h_im - hf, w_im - wf
        hh, hw = 1 - lh, 1 - lw
        h_low, w_low = hf.long(), wf.long()
        wts = [hh * hw, hh * lw, lh * hw, lh * lw]
        dwh = [-hw, -lw, hw, lw]
        dww = [-hh, hh, -lh, lh]
        vs, oks, rows = [], [], []
        for dy, dx in _CORNERS:
            hc, wc = h_low + dy, w_low + dx
            row_ok = (hc >= 0) & ((hc < H - 1) if (mutant == "border_corner_dropped" and dy == 1) else (hc <= H - 1))
            ok = keep & row_ok & (wc >= 0) & (wc <= Wd - 1)
            px = torch.where(ok, hc * Wd + wc, torch.zeros_like(hc)) + lsi[l]
            v = value[nb, px, mb] * ok.unsqueeze(-1).to(dtype)                                # (N, Lq, M, P, D); 0 where not read
            vs.append(v)
            oks.append(ok)
            rows.append(((nb * S + px) * M + mb).reshape(-1))
        got = go.unsqueeze(3)                                                                 # (N, Lq, M, 1, D)
        wf_ = list(wts)                                                                       # the forward's corner weights
        wb_ = list(wts)                                                                       # the backward's
        if coarse and mutant == "fwd_corner_coarse":
            wf_[3] = wf_[3] * (1 + 2.0 ** -6)
        if coarse and mutant == "bwd_corner_coarse":
            wb_[3] = wb_[3] * (1 + 2.0 ** -6)
        a_f = a * (1 - 2.0 ** -6) if (coarse and mutant == "fwd_aw_coarse") else a
        val_f = sum(w.unsqueeze(-1) * v for w, v in zip(wf_, vs))
        val_b = sum(w.unsqueeze(-1) * v for w, v in zip(wb_, vs))
        if mutant == "bf16_sum":
            for p in range(P):
                out = _bf16(out + a_f[..., p, None] * val_f[:, :, :, p])
        else:
            out = out + (a_f.unsqueeze(-1) * val_f).sum(3)
        g_aw[:, :, :, l] = (got * val_b).sum(-1)
        gh = sum(d.unsqueeze(-1) * v for d, v in zip(dwh, vs))
        gw = sum(d.unsqueeze(-1) * v for d, v in zip(dww, vs))
        tgv = got * a.unsqueeze(-1)                                                           # (N, Lq, M, P, D)
        g_loc[:, :, :, l, :, 0] = Wd * (gw * tgv).sum(-1)
        gy = H * (gh * tgv).sum(-1)
        g_loc[:, :, :, l, :, 1] = gy * (1 + 2.0 ** -6) if (coarse and mutant == "gloc_y_coarse") else gy
        for w, ok, r in zip(wb_, oks, rows):
            g_val.index_add_(0, r, ((w * ok.to(dtype)).unsqueeze(-1) * tgv).reshape(-1, D))
        if not bounds:
            continue
        # ---- bounds (module docstring), in float64 from this evaluation's operands ----
        d_ = lambda t: t.to(f64)
        keep64 = keep.to(f64)
        # d_h = u (|loc_y H| (product) + 2 |h_im| (difference, rebase) + [h_im < 0] lh (h_im - floor(h_im) rounds there))
        dh = u * (d_(y * H).abs() + 2 * d_(h_im).abs() + (h_im < 0).to(f64) * d_(lh)) * keep64
        dw = u * (d_(x * Wd).abs() + 2 * d_(w_im).abs() + (w_im < 0).to(f64) * d_(lw)) * keep64
        av = [d_(v).abs() for v in vs]
        A_val = sum(d_(w).abs().unsqueeze(-1) * v for w, v in zip(wts, av))                   # sum_c |w_c v_c|
        A_dh = sum(d_(t).abs().unsqueeze(-1) * v for t, v in zip(dwh, av))                    # sum_c |dw_c/dlh v_c|
        A_dw = sum(d_(t).abs().unsqueeze(-1) * v for t, v in zip(dww, av))
        A_v = sum(av)                                                                         # sum_c |v_c|
        a64, go64 = d_(a).abs().unsqueeze(-1), d_(got).abs()
        loc_val = dh.unsqueeze(-1) * A_dh + dw.unsqueeze(-1) * A_dw
        B["out_abs"] += (a64 * A_val).sum(3)
        B["out_loc"] += (a64 * loc_val).sum(3)
        # grad_aw: R_AW = D + 7 roundings on sum_d |go_d| sum_c |w_c v_c|
        B["grad_aw"][:, :, :, l] = _gamma(D + 7, u) * (go64 * A_val).sum(-1) + (go64 * loc_val).sum(-1)
        # grad_loc: R_LOC = D + 8 roundings on (W | H) |aw| sum_d |go_d| sum_c |dw_c v_c|; the mixed term of the OTHER coordinate's error
        s_v = (go64 * A_v).sum(-1) * a64.squeeze(-1)
        B["grad_loc"][:, :, :, l, :, 0] = Wd * (_gamma(D + 8, u) * (go64 * a64 * A_dw).sum(-1) + dh * s_v)
        B["grad_loc"][:, :, :, l, :, 1] = H * (_gamma(D + 8, u) * (go64 * a64 * A_dh).sum(-1) + dw * s_v)
        tg64 = go64 * a64
        for w, th, tw, ok, r in zip(wts, dwh, dww, oks, rows):
            ok64 = ok.to(f64)
            B["gv_abs"].index_add_(0, r, ((d_(w).abs() * ok64).unsqueeze(-1) * tg64).reshape(-1, D))
            B["gv_loc"].index_add_(0, r, (((dh * d_(th).abs() + dw * d_(tw).abs()) * ok64).unsqueeze(-1) * tg64).reshape(-1, D))
            B["gv_n"].index_add_(0, r, ok64.reshape(-1))                                      # the scatter of ones
    res = dict(out=out.reshape(N, Lq, M * D), grad_value=g_val.view(N, S, M, D), grad_loc=g_loc, grad_aw=g_aw)
    res = {k: v.numpy() for k, v in res.items()}
    if not bounds:
        return res
    # out: R_OUT = 4 L P + 4 roundings;  grad_value: R_GV = n + 5 per pixel
    b_out = _gamma(4 * L * P + 4, u) * B["out_abs"] + B["out_loc"]
    b_gv = _gamma(B["gv_n"] + 5, u).unsqueeze(-1) * B["gv_abs"] + B["gv_loc"]
    bnd = dict(out=b_out.reshape(N, Lq, M * D), grad_value=b_gv.view(N, S, M, D), grad_loc=B["grad_loc"], grad_aw=B["grad_aw"])
    if bounds == "bf16":      # storage term: out and grad_value are rounded to bf16 once, at the store: U_BF16 (|ref| + bound)
        for k in ("out", "grad_value"):
            bnd[k + "_sum"] = bnd[k]      # (the bound of the fp32 sum that is stored: stored_interval)
            bnd[k] = bnd[k] + U_BF16 * (torch.from_numpy(res[k]).to(f64).abs().reshape(bnd[k].shape) + bnd[k])
    return res, {k: v.numpy() for k, v in bnd.items()}


def reference(value, shapes, lsi, loc, aw, grad_out, sfx="f32", mutant=None):
    """-> (values, bounds): dicts over OUTPUTS of float64 numpy arrays.  The arguments are exact float64 copies of what the kernel of
    storage type ``sfx`` ("f32", "f64", "bf16") is given -- for bf16 the bf16-rounded value and grad_out."""
    return evaluate(value, shapes, lsi, loc, aw, grad_out, torch.float64, mutant, bounds=sfx)


def ratios(got, ref, bound):
    """-> (worst |got - ref| / bound, flat index of that element).  Where the bound is zero -- dropped samples, pixels nobody touched --
    exactly zero is asked for: anything else (and a NaN anywhere) is inf."""
    got = got.detach().double().cpu().numpy() if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    got = got.reshape(ref.shape)
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / bound)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i


def stored_interval(ref, bound_sum):
    """bf16 storage, the sharper statement behind the storage term: rounding is monotone, so the stored number lies between the bf16
    roundings of ref - bound and ref + bound of the fp32 SUM (bounds[k + "_sum"]) -- where the sum's error cannot reach a rounding
    boundary, that is the correctly rounded reference and nothing else.  -> (lo, hi) as float64 arrays of bf16 numbers.  (The ends go
    through float32 on their way to bf16; they are moved one float32 step outwards first, so that the double rounding cannot tighten.)"""
    def rn(x, direction):
        x32 = torch.from_numpy(np.ascontiguousarray(x)).float()
        x32 = torch.nextafter(x32, torch.full_like(x32, direction * float("inf")))
        return x32.to(torch.bfloat16).double().numpy()
    return rn(ref - bound_sum, -1.0), rn(ref + bound_sum, 1.0)


def outside_interval(got, ref, bound_sum):
    """how many stored elements lie outside stored_interval"""
    got = got.detach().double().cpu().numpy() if hasattr(got, "detach") else np.asarray(got, dtype=np.float64)
    lo, hi = stored_interval(ref, bound_sum)
    return int((~((got.reshape(ref.shape) >= lo) & (got.reshape(ref.shape) <= hi))).sum())


def worst(got, ref, bnd, keys=OUTPUTS):
    """{output: worst ratio} for dicts of outputs"""
    return {k: ratios(got[k], ref[k], bnd[k])[0] for k in keys if k in got}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
NEAR, NUDGE = 2.0 ** -10, 2.0 ** -8


def near_boundary(loc, shapes):
    """how many sampling positions lie within 2^-10 of an integer (a pixel boundary; the drop limits -1, H, W are integers too), in the
    float32 OR the float64 evaluation of h_im / w_im"""
    n = 0
    loc32 = np.asarray(loc, dtype=np.float32)
    for l, (H, Wd) in enumerate(np.asarray(shapes)):
        for c, size in ((0, int(Wd)), (1, int(H))):
            v = loc32[:, :, :, l, :, c]
            for im in (v * np.float32(size) - np.float32(0.5), v.astype(np.float64) * size - 0.5):
                n += int((np.abs(im - np.rint(im)) < NEAR).sum())
    return n


def boundary_distance(loc, shapes):
    """the smallest distance, in pixels, of a sampling position from an integer (float64 evaluation of the given numbers)"""
    loc = np.asarray(loc, dtype=np.float64)
    best = 1.0
    for l, (H, Wd) in enumerate(np.asarray(shapes)):
        for c, size in ((0, int(Wd)), (1, int(H))):
            im = loc[:, :, :, l, :, c] * size - 0.5
            best = min(best, float(np.abs(im - np.rint(im)).min()))
    return best


def _nudge(loc, shapes):
    """every position within 2^-10 of an integer moves to 2^-8 of a pixel beside it, on the side it was on (grad_loc is discontinuous
    across a pixel boundary, and a float32 kernel may floor differently from float64 there)"""
    loc = loc.clone()
    for l, (H, Wd) in enumerate(shapes):
        for c, size in ((0, Wd), (1, H)):
            v = loc[:, :, :, l, :, c].double()
            im = v * size - 0.5
            k = torch.round(im)
            d = im - k
            d32 = (v.float() * size - 0.5).double() - k
            close = (d.abs() < NEAR) | (d32.abs() < NEAR)
            side = torch.where(d < 0, -torch.ones_like(d), torch.ones_like(d))
            moved = ((k + side * NUDGE + 0.5) / size).float()
            loc[:, :, :, l, :, c] = torch.where(close, moved, loc[:, :, :, l, :, c])
    return loc


def make_inputs(call, seed):
    """richsem_amd.workload.make_inputs("init") with: the value of level l scaled by 2^-4l; grad_out scaled per query by 2^-k, k in 0..7;
    the first queries of image 0 moved by loc * 3 - 1 (dropped samples, border corners: test_gpu_dispatch.host_inputs); an eighth of the
    points redrawn from U[-0.15, 1.15]; no position within 2^-10 of a pixel boundary.  -> dict of float32 numpy arrays (+ shapes, lsi)."""
    t = W.make_inputs(call, "init", seed=seed)
    g = torch.Generator().manual_seed(1000 + seed)
    for l, ((H, Wd), s) in enumerate(zip(call.shapes, t["lsi"].tolist())):
        t["value"][:, s:s + H * Wd] *= 2.0 ** (-4 * l)
    k = torch.randint(0, 8, (call.N, call.Lq, 1), generator=g)
    t["grad_out"] = t["grad_out"] * torch.pow(2.0, -k.float())
    loc = t["loc"]
    loc[0, :7] = loc[0, :7] * 3.0 - 1.0
    redraw = torch.rand(loc.shape[:-1], generator=g) < 0.125
    wide = torch.rand(loc.shape, generator=g) * 1.3 - 0.15
    loc = torch.where(redraw.unsqueeze(-1), wide, loc)
    loc = _nudge(loc, call.shapes)
    t["loc"] = loc.contiguous()
    z = {k_: v.numpy() for k_, v in t.items()}
    assert near_boundary(z["loc"], z["shapes"]) == 0
    return z


def typed(z, sfx):
    """the inputs as exact float64 copies of what the kernel of ``sfx`` is given (bf16: value and grad_out rounded to bf16 first)"""
    r = dict(z)
    for k in ("value", "grad_out"):
        a = torch.from_numpy(np.ascontiguousarray(z[k]))
        r[k] = (a.to(torch.bfloat16) if sfx == "bf16" else a).double().numpy()
    for k in ("loc", "aw"):
        r[k] = z[k].astype(np.float64)
    return r


def exact_probe(shapes, N, Lq, M=2, D=32, P=4, per_query_go=True):
    """Inputs on which every intermediate of every kernel is exactly representable in float32 -- and the results in bf16 where bf16 is
    stored, with per_query_go=False --, so that all four outputs must equal the float64 reference BIT FOR BIT in any summation order.

    shapes: power-of-two level shapes.  The queries walk, level after level, over every quarter-pixel position from -1.25 to H + 0.25 and
    from -1.25 to W + 0.25 (h_im = k / 4 - 1.25 exactly: loc = (h_im + 0.5) / H is a small multiple of 2^-2 / H) -- the exact positions
    -1, 0, H - 1 and H and every pixel boundary among them; queries past the last position start over.  Query i of that walk has ONE
    non-zero attention weight per head, 2^-(m % 3), at (its level, point i % P); its other points sit on the same grid of their levels, at
    positions that depend on (i, l, p), with weight zero (grad_aw is still formed for them).  value: integers 0..7 that depend on (pixel,
    head, channel); grad_out = 2^-((d + q) % 4) (per_query_go: a row of another query gives another result), or 2^-(d % 4) for all
    queries (the sums a pixel of grad_value receives then stay within bf16's eight bits).
    -> dict(value, shapes, lsi, loc, aw, grad_out) of float32 numpy arrays, (N, Lq, ...)-shaped."""
    shapes = [(int(h), int(w)) for h, w in shapes]
    L = len(shapes)
    assert all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes)
    lsi = np.concatenate(([0], np.cumsum([h * w for h, w in shapes])[:-1])).astype(np.int64)
    S = int(sum(h * w for h, w in shapes))
    grids = []                                                      # (level, ky, kx) of the walk
    for l, (H, Wd) in enumerate(shapes):
        ky, kx = np.meshgrid(np.arange(4 * H + 7), np.arange(4 * Wd + 7), indexing="ij")
        grids.append(np.stack((np.full(ky.size, l), ky.reshape(-1), kx.reshape(-1)), 1))
    walk = np.concatenate(grids, 0)
    assert N * Lq >= len(walk), (N * Lq, len(walk))
    i = np.arange(N * Lq)
    w_ = walk[i % len(walk)]
    loc = np.zeros((N * Lq, M, L, P, 2), dtype=np.float64)
    aw = np.zeros((N * Lq, M, L, P), dtype=np.float64)
    for l, (H, Wd) in enumerate(shapes):
        for p in range(P):
            for m in range(M):
                # a deterministic position of this level's grid for every (query, head, point) ...
                ky = (i * 7 + 3 * p + 5 * m + l) % (4 * H + 7)
                kx = (i * 11 + 5 * p + 3 * m + 2 * l) % (4 * Wd + 7)
                # ... and the walk's own position at the query's level and point
                mine = (w_[:, 0] == l) & (i % P == p)
                ky, kx = np.where(mine, w_[:, 1], ky), np.where(mine, w_[:, 2], kx)
                loc[:, m, l, p, 1] = (ky / 4.0 - 1.25 + 0.5) / H
                loc[:, m, l, p, 0] = (kx / 4.0 - 1.25 + 0.5) / Wd
                aw[:, m, l, p] = np.where(mine, 2.0 ** -(m % 3), 0.0)
    s, m, d = np.meshgrid(np.arange(S), np.arange(M), np.arange(D), indexing="ij")
    value = np.broadcast_to(((s * 3 + m * 5 + d) % 8).astype(np.float64), (N, S, M, D))
    q, d = np.meshgrid(i % Lq, np.arange(M * D) % D, indexing="ij")
    go = 2.0 ** -((d + (q if per_query_go else 0)) % 4)
    z = dict(value=value, shapes=np.asarray(shapes, dtype=np.int64), lsi=lsi, loc=loc.reshape(N, Lq, M, L, P, 2),
             aw=aw.reshape(N, Lq, M, L, P), grad_out=go.reshape(N, Lq, M * D))
    for k in ("value", "loc", "aw", "grad_out"):
        f = np.ascontiguousarray(z[k], dtype=np.float32)
        assert np.array_equal(f.astype(np.float64), z[k]), k      # every input is a float32 number
        z[k] = f
    return z
