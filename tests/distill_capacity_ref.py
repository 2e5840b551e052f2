"""What the tests of the distillation term over capacity buffers share (tests/test_distill_capacity_host.py, tests/test_gpu_distill_capacity.py;
the fixture's generator tests/golden/make_golden_distill_capacity.py uses :func:`expand` too): the fixture's reader and a numpy restatement of
``msda_distill_pairs`` (csrc/msda_distill_pairs.h).  No GPU, no library call.

The fixture keeps its student tensors as 16-dimensional embeddings: a logit row is ``round_to_float16(scale * unit(e) @ unit(text).T)``, an
L1 row ``round_to_float16(scale * e @ basis)``; the generator asserts that every product v lies at least 1e-12 (|v| + 1) away from a float16
rounding boundary, so :func:`expand` returns the same float16-exact numbers on any machine."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_distill_capacity_reference.npz")
KL_SCALE, L1_SCALE = 40.0, 3.0
CASES = ("kl_gt_dyn0", "kl_gt_dyn1", "kl_gt_fed", "kl_pred", "l1_gt")
LAYER_SETS = ((1,), (0, 1))
PROJ = 0.37      # the third checksum of a gradient row: sum_c g_c cos(PROJ c)
_Z = None


def unit_rows(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def products(e, table, kind):
    """the float64 values :func:`expand` rounds: ``kind`` 'kl' -- KL_SCALE * cosines of the rows of e against the rows of table (C, 16);
    'l1' -- L1_SCALE * e @ table (16, D)"""
    e, table = np.asarray(e, dtype=np.float64), np.asarray(table, dtype=np.float64)
    return KL_SCALE * (unit_rows(e) @ unit_rows(table).T) if kind == "kl" else L1_SCALE * (e @ table)


def expand(e, table, kind):
    """embeddings (rows, 16) -> the float16-exact tensor (rows, C or D) as float64"""
    return products(e, table, kind).astype(np.float16).astype(np.float64)


def fixture():
    global _Z
    if _Z is None:
        _Z = dict(np.load(FIXTURE))
    return _Z


def config(ci):
    """config ``ci`` of the fixture: counts, dn_number, groups, pad_size, num_boxes, qot (nl + 1, total), the student tensors kl (nl, N, pad_size +
    Q, C) / l1 (nl, N, pad_size + Q, D) in the batch's own layout (denoising rows first), teacher_gt (total, C), prompt_gt (total, D), and the
    arrays of every case under their names"""
    z, p = fixture(), f"c{ci}."
    nl, N, Q, C, D = (int(v) for v in z["dims"])
    pad = int(z[p + "pad_size"])
    c = {k[len(p):]: v for k, v in z.items() if k.startswith(p)}
    c.update(nl=nl, N=N, Q=Q, C=C, D=D, counts=[int(v) for v in z["cfgs"][ci][:3]], dn_number=int(z["cfgs"][ci][3]), pad=pad,
             groups=int(z[p + "groups"]), total=int(sum(z["cfgs"][ci][:3])))
    c["kl"] = expand(c["e_kl"], z["text"], "kl").reshape(nl, N, pad + Q, C)
    c["l1"] = expand(c["e_l1"], z["basis"], "l1").reshape(nl, N, pad + Q, D)
    c["teacher_gt"] = expand(c["e_tgt"], z["text"], "kl").reshape(-1, C)
    c["prompt_gt"] = c["prompt_gt"].astype(np.float64).reshape(-1, D)
    return c


def calls_of(layers, nl):
    """the fixture's per-call arrays are ordered matching part of layer 0..nl-1, then their denoising parts: -> the indices of the calls of a
    layer set, in the order of ``row_group`` (matching parts, then denoising parts)"""
    return [l for l in layers] + [nl + l for l in layers]


def pairs_numpy(cum, qot, meta, num_boxes, nl, N, Q, pad_cap, cap, layers, objective):
    """``msda_distill_pairs`` restated: -> pred_row, tgt_row (K) int64, row_weight (K) float32, row_group (K) int32, status int32[4]"""
    cum, qot = np.asarray(cum, dtype=np.int64), np.asarray(qot, dtype=np.int64)
    n_d, QT = len(layers), pad_cap + Q
    K = n_d * (cap + N * pad_cap)
    pred_row, tgt_row = np.full(K, -1, dtype=np.int64), np.full(K, -1, dtype=np.int64)
    w, grp = np.zeros(K, dtype=np.float32), np.zeros(K, dtype=np.int32)
    status = np.zeros(4, dtype=np.int32)
    cum_ok = cum[0] == 0 and bool((np.diff(cum) >= 0).all()) and bool((cum <= cap).all())
    status[3] = 0 if cum_ok else 1
    total = int(cum[N]) if cum_ok else 0
    pad_size, groups, overflow = 0, 1, False
    if meta is not None:
        m = [int(v) for v in meta]
        if m[4] != 0 or m[1] < 1 or m[2] < 0 or m[2] > pad_cap or m[2] % m[1] != 0:
            overflow = True
        else:
            pad_size, groups = m[2], m[1]
    status[0] = int(overflow)
    stride = pad_size // groups
    if num_boxes is None:
        q_last = qot[nl - 1, :total]
        num_boxes = float(max(int(((q_last >= 0) & (q_last < Q)).sum()), 1))
    w_m, w_d = np.float32(1.0 / float(num_boxes)), np.float32(1.0 / (float(num_boxes) * groups))
    for i, l in enumerate(layers):
        grp[i * cap: (i + 1) * cap] = i
        grp[n_d * cap + i * N * pad_cap: n_d * cap + (i + 1) * N * pad_cap] = n_d + i
        for t in range(total):
            q = int(qot[l, t])
            if not 0 <= q < Q:
                status[1] += 1
                continue
            b = int(np.searchsorted(cum[1:], t, side="right"))
            k = i * cap + t
            pred_row[k], tgt_row[k], w[k] = (i * N + b) * QT + pad_cap + q, t, w_m
        if cum_ok and not overflow:
            for b in range(N):
                for s in range(pad_size):
                    j = s % stride
                    if j < cum[b + 1] - cum[b]:
                        k = n_d * cap + (i * N + b) * pad_cap + s
                        pred_row[k], tgt_row[k], w[k] = (i * N + b) * QT + s, cum[b] + j, w_d
    if objective == "pred":
        tgt_row = pred_row.copy()
    return pred_row, tgt_row, w, grp, status


def checksums(grad):
    """(rows, C) float64 -> (rows, 3): sum, sum of magnitudes, the projection on cos(PROJ c)"""
    g = np.asarray(grad, dtype=np.float64)
    return np.stack((g.sum(-1), np.abs(g).sum(-1), (g * np.cos(PROJ * np.arange(g.shape[-1]))).sum(-1)), -1)
