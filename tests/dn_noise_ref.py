"""Test infrastructure: a numpy restatement of the reference's ``prepare_for_cdn`` (models/richsem/dn_components.py:11-193, training branch,
check_pos_dn=False) in the form the device kernel takes it -- per (image, slot) uniforms instead of the reference's four draws -- and the
map from the reference's draws to those uniforms.  float32 operation by operation (numpy rounds every float32 operation on its own, as
torch's element-wise kernels do), so labels, noised boxes and the embedded rows are expected bit-equal to the reference's; the final
``inverse_sigmoid`` follows the reference's float32 chain too (1 - x, x1 / x2, log), so ``q_bbox`` differs from the reference's only by the
two libraries' float32 logarithms; the kernel, which takes the logarithm in float64, is compared with the float64 value instead
(``q_bbox_bound``)."""
import numpy as np

F32 = np.float32
LOGF_ULPS = 2      # the k of q_bbox_bound: no statement of the HIP math library's logf accuracy was found with the toolkit's documents, so 2


def group_count(dn_number, max_count, add_gt=False):
    """dn_components.py:27-41"""
    g = dn_number * 2
    if max_count == 0:
        g = 1
    elif g >= 100:
        g = g // (max_count * 2)
    elif g < 1:
        g = 1
    if g == 0:
        g = 1
    return g + (1 if add_gt else 0)


def layout(counts, dn_number, use_cdn=True, add_gt=False):
    single = int(max(counts)) if len(counts) else 0
    groups = group_count(dn_number, single, add_gt)
    pad = single * 2 * groups
    return single, groups, (pad if use_cdn else pad // 2)


def slot_of(g2, j, single, use_cdn):
    """the slot of (group-half g2, box j of its image) in the padded block, or None for a negative half that use_cdn=False drops"""
    if use_cdn:
        return g2 * single + j
    return None if g2 % 2 else (g2 // 2) * single + j


def uniform_from_draws(counts, p, new_label, sign01, rand, num_classes, pad_cap, use_cdn=True, fill_seed=0):
    """the reference's draws, in its row order g2 * total + cum[b] + j -- ``p`` (n,), ``new_label`` (n,) with -1 where not chosen, ``sign01``
    (n, 4) the raw 0 / 1 of randint_like, ``rand`` (n, 4) -- as the kernel's (N, pad_cap, 10) uniforms: sign 0 / 1 -> 0.25 / 0.75, label
    k -> (k + 0.5) / num_classes (which floors back to k in float32).  Slots no draw maps to keep random values: they must not matter."""
    counts = [int(c) for c in counts]
    N, total = len(counts), sum(counts)
    single = max(counts) if counts else 0
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    u = np.random.default_rng(fill_seed).random((N, pad_cap, 10), dtype=F32)
    groups2 = (len(p) // total) if total else 0
    for g2 in range(groups2):
        for b in range(N):
            for j in range(counts[b]):
                s = slot_of(g2, j, single, use_cdn)
                if s is None:
                    continue
                i = g2 * total + cum[b] + j
                k = int(new_label[i])
                u[b, s, 0] = p[i]
                u[b, s, 1] = F32(F32(k + 0.5) / F32(num_classes)) if k >= 0 else F32(0.0)
                u[b, s, 2:6] = np.where(np.asarray(sign01[i]) > 0.5, F32(0.75), F32(0.25))
                u[b, s, 6:10] = rand[i]
    return u


def rows_from_slots(counts, per_slot, groups2, use_cdn=True):
    """a per-slot array (N, pad, ...) in the reference's row order g2 * total + cum[b] + j (n, ...): NaN rows where use_cdn=False dropped the
    slot (float arrays only)"""
    counts = [int(c) for c in counts]
    total, single = sum(counts), max(counts) if counts else 0
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    rows = np.full((groups2 * total,) + per_slot.shape[2:], np.nan, per_slot.dtype)
    for g2 in range(groups2):
        for b in range(len(counts)):
            for j in range(counts[b]):
                s = slot_of(g2, j, single, use_cdn)
                if s is not None:
                    rows[g2 * total + cum[b] + j] = per_slot[b, s]
    return rows


def inverse_sigmoid(x, dtype=F32):
    """util/misc.py:605-609, eps 1e-3"""
    x = np.clip(np.asarray(x, dtype=dtype), dtype(0), dtype(1))
    x1, x2 = np.maximum(x, dtype(1e-3)), np.maximum(dtype(1) - x, dtype(1e-3))
    return np.log(x1 / x2)


def inverse_sigmoid64_of_f32(x):
    """float64 inverse_sigmoid of float32 boxes with the float32 eps the reference's float32 tensors see"""
    x = np.clip(np.asarray(x, dtype=F32), F32(0), F32(1)).astype(np.float64)
    eps = np.float64(F32(1e-3))
    return np.log(np.maximum(x, eps) / np.maximum(1.0 - x, eps))


def ulp32(y):
    y = np.abs(np.asarray(y, dtype=np.float64)).astype(F32)
    return np.spacing(y).astype(np.float64)


def q_bbox_bound(noised_box):
    """-> (y64, bound): |q_bbox - y64| <= 2^-24 + LOGF_ULPS * ulp32(|y64|) element-wise.  2^-24: the float32 roundings of 1 - x and of x1 / x2 in
    front of the logarithm move its argument by about one part in 2^24 (d log = d r / r); k ulp: the logarithm itself."""
    y64 = inverse_sigmoid64_of_f32(noised_box)
    return y64, 2.0 ** -24 + LOGF_ULPS * ulp32(y64)


def q_bbox_bound_float32_chain(noised_box):
    """-> (y64, bound) for a float32 evaluation in the reference's order: |q - y64| <= 2^-23 + LOGF_ULPS * ulp32(|y64|).  The chain rounds twice
    in front of the logarithm -- 1 - x and x1 / x2, each by at most 2^-24 relative --, and d log r = d r / r, so each moves the result by at
    most 2^-24 (plus terms of order 2^-48): 2^-23 together, where ``q_bbox_bound`` has room for one of them."""
    y64 = inverse_sigmoid64_of_f32(noised_box)
    return y64, 2.0 ** -23 + LOGF_ULPS * ulp32(y64)


def attn_mask_ref(pad_size, group_pad, pad_cap, num_queries):
    """dn_components.py:157-179 on rows / columns [0, pad_size) + [pad_cap, T); tail columns masked for every row, tail rows see the matching
    queries only"""
    T = pad_cap + num_queries
    m = np.zeros((T, T), dtype=bool)
    m[:, pad_size:pad_cap] = True
    m[pad_size:, :pad_size] = True
    if group_pad > 0:
        g = np.arange(pad_size) // group_pad
        m[:pad_size, :pad_size] = g[:, None] != g[None, :]
    return m


def denoising_queries_ref(counts, labels, boxes, uniform, table, *, pad_cap, num_queries, num_classes, dn_number, label_noise_ratio,
                          box_noise_scale, use_cdn=True, add_gt=False, return_preclamp=False):
    """-> dict: q_label (N, pad_cap, D), q_bbox, noised_box (N, pad_cap, 4) float32, noised_label (N, pad_cap) int64, attn_mask (T, T) bool,
    meta int64[5] = single_pad, num_dn_group, pad_size, total, overflow"""
    counts = [int(c) for c in counts]
    N, total = len(counts), sum(counts)
    labels, boxes = np.asarray(labels, dtype=np.int64), np.asarray(boxes, dtype=F32).reshape(-1, 4)
    uniform, table = np.asarray(uniform, dtype=F32), np.asarray(table, dtype=F32)
    single, groups, pad_size = layout(counts, dn_number, use_cdn, add_gt)
    overflow = int(pad_size > pad_cap)
    if overflow:
        pad_size = 0
    cum = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    D = table.shape[1]
    out = {"q_label": np.zeros((N, pad_cap, D), F32), "q_bbox": np.zeros((N, pad_cap, 4), F32), "noised_box": np.zeros((N, pad_cap, 4), F32),
           "noised_label": np.full((N, pad_cap), -1, np.int64), "meta": np.array([single, groups, pad_size, total, overflow], np.int64),
           "attn_mask": attn_mask_ref(pad_size, 2 * single if use_cdn else single, pad_cap, num_queries)}
    pre = []
    thr, scale = F32(label_noise_ratio * 0.5), F32(box_noise_scale)
    for b in range(N):
        for s in range(pad_size):
            gi, j = divmod(s, single)
            g2 = gi if use_cdn else 2 * gi
            if j >= counts[b]:
                continue
            t, u = cum[b] + j, uniform[b, s]
            keep = add_gt and g2 == 0
            lab = int(labels[t])
            if not keep and u[0] < thr:
                lab = min(int(np.floor(u[1] * F32(num_classes))), num_classes - 1)
            bx = boxes[t]
            nb = bx.copy()
            if box_noise_scale > 0:
                half = bx[2:] / F32(2)
                xyxy = np.concatenate((bx[:2] - half, bx[:2] + half)).astype(F32)
                diff = np.concatenate((half, half)).astype(F32)
                part = (u[6:10] + F32(1)) if g2 % 2 else u[6:10]
                rp = part * np.where(u[2:6] < F32(0.5), F32(-1), F32(1)).astype(F32)
                if keep:
                    rp = np.zeros(4, F32)
                v = xyxy + (rp * diff) * scale
                pre.append(v)
                c = np.clip(v, F32(0), F32(1))
                nb = np.concatenate(((c[:2] + c[2:]) / F32(2), c[2:] - c[:2])).astype(F32)
            out["noised_label"][b, s] = lab
            out["noised_box"][b, s] = nb
            out["q_bbox"][b, s] = inverse_sigmoid(nb)
            if 0 <= lab < table.shape[0]:
                out["q_label"][b, s] = table[lab]
    if return_preclamp:
        out["preclamp"] = np.stack(pre) if pre else np.zeros((0, 4), F32)
    return out
