// msda_fed_slots.h -- the federated loss's class subsets over CAPACITY buffers: the appeared classes of every get_loss call are read on the
// device from the slot space of msda_criterion.h (the target prefix `cum`, the solver's `query_of_target`, the denoising `meta`), so one
// captured launch draws the subsets of whatever batch the buffers hold.  Included by criterion_api.hip.
//
// Reference: get_fed_loss_inds (models/richsem/fed_loss.py:15-25) through SetCriterion.loss_labels (richsem.py:938-964, use_fed_loss): the
// subset of a call is unique(target_classes_o) -- the classes of THAT call's matched pairs -- topped up to num_sample_cats by weighted draws
// without replacement.  msda_fed_class_mask_f32 (msda_fed.h, rows_api.hip) takes the label list of exact length; the draw below is that
// kernel's, RESTATED operation for operation (this file is part of another translation unit, and nothing the existing kernel is built from
// changes with it): keys -log1pf(-u) / w packed as (float bits << 32) | class, ineligible classes 0xffffffff in the high word, bitonic sort
// ascending, take = min(max(num_sample_cats - appeared, 0), eligible).  The keys are a total order (the class is part of the key), so the
// result does not depend on the thread count: given a group's exact label list and the same uniform row the two kernels agree bit for bit.
//
// One workgroup per get_loss call g, numbered as the `terms` of msda_criterion_pairs_f32:
//   g < nl             matching part of layer g: label of slot t for t < cum[N] with 0 <= query_of_target[g][t] < Q
//   nl <= g < 2 nl     denoising part of layer g - nl: empty without meta, on overflow or a layout that is none (groups < 1, pad_size <= 0
//                      or no multiple of the group count); else label of target cum[b] + j for j < min(T_b, pad_size / num_dn_group)
//   g == 2 nl          the two-stage output: as a matching part with Qi queries; with flags & 1 every live slot has label 0
// A label outside [0, C) appears nowhere (the pair kernel leaves its pairs out); a prefix that does not start at 0, decreases or exceeds
// the capacity leaves every group empty (the pair kernel leaves out every pair).  A class is appeared iff the pair kernel counts a
// positive entry of that class in that call.  (One condition the pair kernel sees and this one cannot: pad_size > pad_cap.  The meta of
// msda_dn_queries_f32 run with the same pad_cap has `overflow` set then, which both read.)
// LDS atomics only; no global atomic, no workspace; all output through plain stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msda_criterion.h"

namespace msda {

constexpr int kFedSlotsMaxClasses = 4096;      // the keys of one group sort in LDS: 4096 x 8 bytes
constexpr int kFedSlotsThreads = 1024;

struct FedSlotsArgs {
    const int64_t *cum, *tgt_ids, *qot, *meta;
    const float *weight, *uniform;
    int nl, N, Q, Qi, C, P2, num_sample_cats, flags;
    int64_t cap;
    float *mask;
    int32_t *n_chosen;
};

__global__ __launch_bounds__(kFedSlotsThreads) void fed_class_mask_slots_kernel(FedSlotsArgs a)
{
    extern __shared__ unsigned long long keys[];
    __shared__ int64_t s_cum[kCritMaxImages + 1];
    __shared__ unsigned seen[kFedSlotsMaxClasses / 32], taken[kFedSlotsMaxClasses / 32];
    __shared__ int n_seen, n_eligible, s_bad;
    const int tid = threadIdx.x, nt = blockDim.x, g = blockIdx.x, C = a.C, P2 = a.P2, N = a.N, nl = a.nl, words = (C + 31) >> 5;
    for (int i = tid; i < words; i += nt) seen[i] = taken[i] = 0u;
    for (int i = tid; i <= N; i += nt) s_cum[i] = a.cum[i];
    if (tid == 0) n_seen = n_eligible = s_bad = 0;
    __syncthreads();
    {      // the prefix, checked as criterion_pairs_kernel checks it
        bool bad = false;
        for (int i = tid; i <= N; i += nt) {
            const int64_t v = s_cum[i];
            bad |= i == 0 ? v != 0 : v < s_cum[i - 1];
            bad |= v > a.cap;
        }
        if (bad) s_bad = 1;      // (any thread: the same value)
    }
    __syncthreads();
    const int64_t total = s_bad == 0 ? s_cum[N] : 0;

    // ---- the appeared classes of this call -----------------------------------------------------------------------------------------------
    if (g < nl || g == 2 * nl) {
        const int o = g < nl ? g : nl;
        const bool two_stage = o == nl;
        const int nq = two_stage ? a.Qi : a.Q;
        const bool agnostic = two_stage && (a.flags & 1);
        const int64_t *q_row = a.qot + (int64_t)o * a.cap;
        for (int64_t t = tid; t < total; t += nt) {
            const int64_t q = q_row[t];
            if (q < 0 || q >= nq) continue;
            const int64_t l = agnostic ? 0 : a.tgt_ids[t];
            if (l >= 0 && l < C) atomicOr(&seen[l >> 5], 1u << (l & 31));
        }
    } else if (a.meta) {
        const int64_t m_groups = a.meta[1], m_pad = a.meta[2], m_over = a.meta[4];
        if (m_over == 0 && m_groups >= 1 && m_pad > 0 && m_pad % m_groups == 0) {
            const int64_t stride = m_pad / m_groups;
            for (int64_t t = tid; t < total; t += nt) {
                const int b = crit_image_of(s_cum, N, t);
                if (t - s_cum[b] >= stride) continue;      // (a target past the layout's single_pad has no denoising slot)
                const int64_t l = a.tgt_ids[t];
                if (l >= 0 && l < C) atomicOr(&seen[l >> 5], 1u << (l & 31));
            }
        }
    }
    __syncthreads();

    // ---- the draw: fed_class_mask_kernel's, restated -------------------------------------------------------------------------------------
    for (int i = tid; i < words; i += nt) atomicAdd(&n_seen, __popc(seen[i]));
    const float *u = a.uniform + (long long)g * C;
    int elig = 0;
    for (int c = tid; c < P2; c += nt) {
        unsigned long long k = ~0ull;      // (the padding past C sorts last)
        if (c < C) {
            const float w = a.weight[c];
            unsigned hi = 0xffffffffu;
            if (!((seen[c >> 5] >> (c & 31)) & 1u) && w > 0.f) {
                const float key = -log1pf(-u[c]) / w;
                hi = key > 0.f ? __float_as_uint(key) : (key == 0.f ? 0u : 0x7f800000u);      // (-0 -> +0; a NaN key -- u outside [0, 1) -- counts as +inf)
                ++elig;
            }
            k = (unsigned long long)hi << 32 | (unsigned)c;
        }
        keys[c] = k;
    }
    if (elig) atomicAdd(&n_eligible, elig);
    __syncthreads();
    // bitonic sort of the P2 keys, ascending
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (P2 >> 1); i += nt) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    keys[lo] = y;
                    keys[hi] = x;
                }
            }
            __syncthreads();
        }
    const int m = a.num_sample_cats - n_seen > 0 ? a.num_sample_cats - n_seen : 0;
    const int take = m < n_eligible ? m : n_eligible;      // (fewer eligible classes than m: every one of them)
    for (int i = tid; i < take; i += nt) {
        const unsigned c = (unsigned)(keys[i] & 0xffffffffu);
        atomicOr(&taken[c >> 5], 1u << (c & 31));
    }
    __syncthreads();
    float *out = a.mask + (long long)g * C;
    for (int c = tid; c < C; c += nt) out[c] = ((seen[c >> 5] | taken[c >> 5]) >> (c & 31)) & 1u ? 1.f : 0.f;
    if (tid == 0) a.n_chosen[g] = n_seen + take;
}

}  // namespace msda
