"""Numpy restatement of what ``msda_fed_class_mask_slots_f32`` (csrc/msda_fed_slots.h) reads from the slot space -- the appeared classes of
each of the 2 nl + 1 get_loss calls -- and of its count ``n_chosen``; plus the loader of tests/golden/criterion_fed_capacity_reference.npz.
No GPU, no library: the host tests hold it to the reference's recorded ``unique(target_classes_o)``, the GPU tests hold the kernel to it."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "criterion_fed_capacity_reference.npz")
OWN = ("fed_ids", "appeared", "per_call", "loss", "grad_il", "grad_ib")      # what an enc_cls_agn case stores itself; the rest is its twin's
_Z = None


def fixture():
    global _Z
    if _Z is None:
        _Z = dict(np.load(FIXTURE))
    return _Z


def case(ci):
    """case ``ci`` as a dict without the prefix; an enc_cls_agn case (odd ``ci``) takes what it does not store from the case before it"""
    z = fixture()
    agn = int(z["cases"][ci][4])
    out = {}
    for src in ([ci - 1, ci] if agn else [ci]):
        p = f"c{src}."
        out.update({k[len(p):]: v for k, v in z.items() if k.startswith(p)})
    out["agn"] = agn
    return out


def prefix_ok(cum, capacity):
    cum = np.asarray(cum, dtype=np.int64)
    return bool(cum[0] == 0 and (np.diff(cum) >= 0).all() and (cum <= capacity).all())


def label_lists(cum, tgt_ids, qot, meta, nl, Q, Qi, capacity, flags=0):
    """the exact label list of each of the 2 nl + 1 get_loss calls, with repeats and with labels outside the class range as they stand --
    what ``msda_fed_class_mask_f32`` takes as ``labels``.  ``cum`` (N + 1), ``tgt_ids`` (capacity), ``qot`` (nl + 1, capacity), ``meta`` None
    or (single_pad, num_dn_group, pad_size, total, overflow)"""
    cum, ids, qot = np.asarray(cum, dtype=np.int64), np.asarray(tgt_ids, dtype=np.int64), np.asarray(qot, dtype=np.int64)
    ok = prefix_ok(cum, capacity)
    total = int(cum[-1]) if ok else 0
    out = []
    for g in range(2 * nl + 1):
        labels = []
        if not ok:      # (nothing is read through a prefix that does not describe targets inside the capacity)
            pass
        elif g < nl or g == 2 * nl:
            o = g if g < nl else nl
            nq = Qi if o == nl else Q
            for t in range(total):
                if 0 <= qot[o, t] < nq:
                    labels.append(0 if (o == nl and flags & 1) else int(ids[t]))
        elif meta is not None:
            groups, pad, over = int(meta[1]), int(meta[2]), int(meta[4])
            if over == 0 and groups >= 1 and pad > 0 and pad % groups == 0:
                stride = pad // groups
                for b in range(len(cum) - 1):
                    for j in range(min(int(cum[b + 1] - cum[b]), stride)):
                        labels.append(int(ids[cum[b] + j]))
        out.append(np.array(labels, dtype=np.int64))
    return out


def appeared_sets(cum, tgt_ids, qot, meta, nl, Q, Qi, C, capacity, flags=0):
    """-> a list of 2 nl + 1 sorted int64 arrays: the distinct labels inside [0, C) of :func:`label_lists`"""
    return [np.unique(l[(l >= 0) & (l < C)]) for l in label_lists(cum, tgt_ids, qot, meta, nl, Q, Qi, capacity, flags)]


def n_chosen_of(appeared, weight, num_sample_cats):
    """appeared + min(max(num_sample_cats - appeared, 0), eligible): eligible = weight > 0 and not appeared"""
    w = np.asarray(weight)
    elig = w > 0
    elig[appeared] = False
    return len(appeared) + min(max(num_sample_cats - len(appeared), 0), int(elig.sum()))
