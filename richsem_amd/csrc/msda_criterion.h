// msda_criterion.h -- the criterion's classification and box terms over CAPACITY buffers: which (prediction, target) pairs carry a loss is
// read on the device, from the target prefix `cum`, the denoising layout's `meta` and the solver's `query_of_target`, so one captured
// launch serves every batch that fits the capacities.
//
// Reference: SetCriterion.forward (models/richsem/richsem.py:1124-1298) -- num_boxes (:1143-1147), the denoising positive indices
// (:1158-1171, with prep_for_dn :1300-1306), and per output loss_labels (:938-964) / loss_boxes (:1045-1071).  The per-pair formulas are
// the ones of msda_focal_pos_sum_f32 / msda_box_pair_loss_f32 (rows_api.hip), RESTATED below in namespace crit, operation for operation:
// those two kernels keep their formulas inline and this file is a translation unit of its own (criterion_api.hip), so that nothing the
// existing kernels are built from changes with it.  Folding both onto one definition is a follow-up (tools/kernel_isa_diff.py shows
// whether the existing kernels' code stays the same).
//
// Slot space (fixed by the capacities; a thread per slot; a workgroup never spans two of the reference's get_loss calls):
//   matched  (o, t), o in 0..nl (nl decoder outputs, then the two-stage output), t in 0..capacity
//            live iff t < cum[N] and 0 <= q = query_of_target[o][t] < Q (Qi for o == nl); image b from cum;
//            prediction logits[o, b, pad_cap + q, label_t] / coords[o, b, pad_cap + q]  (il[b, q, label_t] / ib[b, q] for o == nl); weight 1 / num_boxes
//   denoising (l, b, s), s in 0..pad_cap, from meta = (single_pad, num_dn_group, pad_size, total, overflow):
//            stride = pad_size / num_dn_group; live iff no overflow, s < pad_size and j = s % stride < T_b; target cum[b] + j;
//            prediction logits[l, b, s, label] / coords[l, b, s]; weight 1 / (num_boxes * num_dn_group)
//   rows     one thread per row of logits / il writes the row weight the all-negative focal kernels take -- and, where the caller asks for
//            it, the row's get_loss call (0..nl-1 matching parts, nl..2nl-1 denoising parts, 2 nl the two-stage output): the row_group of
//            the masked focal kernels (the federated loss, msda_fed_slots.h).
// num_boxes = max(1, live pairs of the last decoder output), counted by every workgroup for itself (an integer: the same in each), or the
// caller's value.  Every weight is formed in float64 and rounded to float32 once.
//
// Sums: wave shuffles -> one float64 partial per workgroup and term -> criterion_reduce_kernel adds each call's partials in workgroup
// order.  No floating-point atomic anywhere: the results are reproducible bit for bit.
#pragma once

#include <stdint.h>

#include "msda_common.h"

namespace msda {

namespace crit {

// forward-mode value + four tangents (d / d cx, cy, w, h of the predicted box), torch's conventions: |x|' = sign x, a maximum / minimum
// passes the gradient to the larger / smaller operand and halves it on a tie, clamp(min = 0) passes it where x >= 0
struct Dual4 {
    float v, d[4];
};
__device__ __forceinline__ Dual4 d4_const(float v) { return Dual4{v, {0.f, 0.f, 0.f, 0.f}}; }
__device__ __forceinline__ Dual4 d4_var(float v, int i) { Dual4 r = d4_const(v); r.d[i] = 1.f; return r; }
__device__ __forceinline__ Dual4 operator+(Dual4 a, Dual4 b) { return Dual4{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2], a.d[3] + b.d[3]}}; }
__device__ __forceinline__ Dual4 operator-(Dual4 a, Dual4 b) { return Dual4{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2], a.d[3] - b.d[3]}}; }
__device__ __forceinline__ Dual4 operator*(Dual4 a, Dual4 b)
{
    return Dual4{a.v * b.v, {a.d[0] * b.v + a.v * b.d[0], a.d[1] * b.v + a.v * b.d[1], a.d[2] * b.v + a.v * b.d[2], a.d[3] * b.v + a.v * b.d[3]}};
}
__device__ __forceinline__ Dual4 operator/(Dual4 a, Dual4 b)
{
    const float q = a.v / b.v, ib = 1.f / b.v;
    return Dual4{q, {(a.d[0] - q * b.d[0]) * ib, (a.d[1] - q * b.d[1]) * ib, (a.d[2] - q * b.d[2]) * ib, (a.d[3] - q * b.d[3]) * ib}};
}
__device__ __forceinline__ Dual4 d4_scale(Dual4 a, float s) { return Dual4{a.v * s, {a.d[0] * s, a.d[1] * s, a.d[2] * s, a.d[3] * s}}; }
__device__ __forceinline__ Dual4 d4_max(Dual4 a, Dual4 b) { return a.v > b.v ? a : (b.v > a.v ? b : d4_scale(a + b, 0.5f)); }
__device__ __forceinline__ Dual4 d4_min(Dual4 a, Dual4 b) { return a.v < b.v ? a : (b.v < a.v ? b : d4_scale(a + b, 0.5f)); }
__device__ __forceinline__ Dual4 d4_relu(Dual4 a) { return a.v >= 0.f ? a : d4_const(0.f); }
__device__ __forceinline__ Dual4 d4_abs(Dual4 a) { return a.v > 0.f ? a : (a.v < 0.f ? d4_scale(a, -1.f) : d4_const(0.f)); }

// one pair: the L1 distance and the GIoU of prediction pv against target tv (cx, cy, w, h), each with its tangents w.r.t. pv
// (box_pair_loss_kernel's body, SetCriterion.loss_boxes with util/box_ops.py:9-64 on the diagonal)
__device__ __forceinline__ void box_pair_terms(float4 pv, float4 tv, Dual4 &l1, Dual4 &giou)
{
    const Dual4 cx = d4_var(pv.x, 0), cy = d4_var(pv.y, 1), pw = d4_var(pv.z, 2), ph = d4_var(pv.w, 3);
    l1 = d4_abs(cx - d4_const(tv.x)) + d4_abs(cy - d4_const(tv.y)) + d4_abs(pw - d4_const(tv.z)) + d4_abs(ph - d4_const(tv.w));
    const Dual4 half = d4_const(0.5f);
    const Dual4 ax0 = cx - half * pw, ay0 = cy - half * ph, ax1 = cx + half * pw, ay1 = cy + half * ph;
    const Dual4 bx0 = d4_const(tv.x - 0.5f * tv.z), by0 = d4_const(tv.y - 0.5f * tv.w), bx1 = d4_const(tv.x + 0.5f * tv.z), by1 = d4_const(tv.y + 0.5f * tv.w);
    const Dual4 area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
    const Dual4 iw = d4_relu(d4_min(ax1, bx1) - d4_max(ax0, bx0)), ih = d4_relu(d4_min(ay1, by1) - d4_max(ay0, by0));
    const Dual4 inter = iw * ih, uni = area_a + area_b - inter;
    const Dual4 iou = inter / (uni + d4_const(1e-6f));
    const Dual4 hw = d4_relu(d4_max(ax1, bx1) - d4_min(ax0, bx0)), hh = d4_relu(d4_max(ay1, by1) - d4_min(ay0, by0));
    const Dual4 hull = hw * hh;
    giou = iou - (hull - uni) / (hull + d4_const(1e-6f));
}
// c_l1 * L1 + c_giou * (1 - GIoU) of one pair, value and tangents
__device__ __forceinline__ Dual4 box_pair_loss(Dual4 l1, Dual4 giou, float c_l1, float c_giou)
{
    return d4_scale(l1, c_l1) + d4_scale(d4_const(1.f) - giou, c_giou);
}

// what a positive entry contributes to the sigmoid focal loss instead of the all-negative term (focal_pos_sum_kernel's body):
// alpha (1 - q)^2 softplus(-v) - (1 - alpha) q^2 softplus(v), q = sigmoid(v); dl = its derivative
__device__ __forceinline__ float focal_pos_term(float v, float alpha, float &dl)
{
    const float q = 1.f / (1.f + expf(-v));
    const float sp_pos = v > 20.f ? v : log1pf(expf(v)), sp_neg = -v > 20.f ? -v : log1pf(expf(-v));      // softplus(x), softplus(-x) (torch's threshold 20)
    const float omq = 1.f - q;
    // d/dx: q' = q (1 - q); softplus(x)' = q; softplus(-x)' = -(1 - q)
    dl = alpha * (-2.f * omq * q * omq * sp_neg - omq * omq * omq) - (1.f - alpha) * (2.f * q * q * omq * sp_pos + q * q * q);
    return alpha * omq * omq * sp_neg - (1.f - alpha) * q * q * sp_pos;
}

}  // namespace crit

constexpr int kCritThreads = 256;
constexpr int kCritMaxImages = 1024;      // cum is kept in LDS

// where the pair launch keeps what the backward needs and what the reduction adds up: one caller-owned workspace
struct CritLayout {
    int64_t slots_m, slots_d;            // (nl + 1) * cap matched slots, then nl * N * pad_cap denoising slots
    int blocks_m, blocks_d, blocks_r;    // workgroups per matched call, per denoising call, for the row weights
    int grid_pairs;                      // (nl + 1) * blocks_m + nl * blocks_d: the workgroups that leave partials
    size_t off_gb, off_gx, off_row, off_label, off_partial, off_stat, bytes;
};

__host__ __device__ inline CritLayout crit_layout(int nl, int N, int Q, int Qi, int64_t cap, int pad_cap)
{
    CritLayout L;
    L.slots_m = (int64_t)(nl + 1) * cap;
    L.slots_d = (int64_t)nl * N * pad_cap;
    L.blocks_m = (int)((cap + kCritThreads - 1) / kCritThreads);
    L.blocks_d = (int)(((int64_t)N * pad_cap + kCritThreads - 1) / kCritThreads);
    const int64_t rows = (int64_t)nl * N * (pad_cap + Q) + (int64_t)N * Qi;
    L.blocks_r = (int)((rows + kCritThreads - 1) / kCritThreads);
    L.grid_pairs = (nl + 1) * L.blocks_m + nl * L.blocks_d;
    const size_t S = (size_t)(L.slots_m + L.slots_d);
    size_t at = 0;
    L.off_gb = at;      at += S * 16;                                  // float4: d loss / d box of the slot's prediction
    L.off_partial = at; at += (size_t)L.grid_pairs * 3 * 8;            // double[grid_pairs][3]
    L.off_gx = at;      at += S * 4;                                   // float: d loss / d logit of the slot's positive entry
    L.off_row = at;     at += S * 4;                                   // int32: row of the prediction in its tensor, -1 = dead slot
    L.off_label = at;   at += S * 4;                                   // int32: class of the positive entry
    L.off_stat = at;    at += (size_t)L.grid_pairs * 4 * 4;            // int32[grid_pairs][4]
    L.bytes = (at + 15) & ~(size_t)15;
    return L;
}

struct CritArgs {
    const float *logits, *coords, *il, *ib;
    const int64_t *cum, *tgt_ids;
    const float *tgt_boxes;
    const int64_t *qot, *meta;
    const float *num_boxes_in;
    int nl, N, Q, Qi, C, pad_cap;
    int64_t cap;
    float alpha, c_cls, c_l1, c_giou;
    float *row_weight, *row_weight_int;
    int flags;                               // bit 0: the two-stage output's slots take label 0 (enc_cls_agn, richsem.py:1249-1255)
    int32_t *row_group, *row_group_int;      // or null: each row's get_loss call, for msda_focal_neg_*_masked_f32
    float4 *rec_gb;
    float *rec_gx;
    int32_t *rec_row, *rec_label;
    double *partial;
    int32_t *stat;
};

__device__ __forceinline__ float crit_wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// image of target t: the b with cum[b] <= t < cum[b + 1] (cum non-decreasing, cum[0] = 0, t < cum[N])
__device__ __forceinline__ int crit_image_of(const int64_t *cum, int N, int64_t t)
{
    int lo = 1, hi = N;      // the first index in [1, N] whose cum is > t (cum[N] is)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo - 1;
}

__global__ __launch_bounds__(kCritThreads) void criterion_pairs_kernel(CritArgs a, CritLayout L)
{
    __shared__ int64_t s_cum[kCritMaxImages + 1];
    __shared__ int s_int[kCritThreads / 64];
    __shared__ float s_red[3][kCritThreads / 64];
    __shared__ int s_flags[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, nl = a.nl, QT = a.pad_cap + a.Q;

    // ---- cum into LDS, checked: nothing is read through a prefix that does not describe targets inside the capacity ------------------
    for (int i = tid; i <= N; i += kCritThreads) s_cum[i] = a.cum[i];
    if (tid < 4) s_flags[tid] = 0;
    __syncthreads();
    {
        bool bad = false;
        for (int i = tid; i <= N; i += kCritThreads) {
            const int64_t v = s_cum[i];
            bad |= i == 0 ? v != 0 : v < s_cum[i - 1];
            bad |= v > a.cap;
        }
        if (bad) s_flags[3] = 1;      // (any thread: the same value)
    }
    __syncthreads();
    const bool cum_ok = s_flags[3] == 0;
    const int64_t total = cum_ok ? s_cum[N] : 0;

    // ---- the denoising layout ------------------------------------------------------------------------------------------------------------
    int pad_size = 0, groups = 1, stride = 1;
    bool overflow = false;
    if (a.meta) {
        const int64_t m_groups = a.meta[1], m_pad = a.meta[2], m_over = a.meta[4];
        if (m_over != 0 || m_groups < 1 || m_pad < 0 || m_pad > a.pad_cap || m_pad % m_groups != 0) {
            overflow = true;
        } else {
            pad_size = (int)m_pad;
            groups = (int)m_groups;
            stride = pad_size / groups;
        }
    }

    // ---- num_boxes: live pairs of the last decoder output, clamped to >= 1 (richsem.py:1143-1147) -- or the caller's ----------------------
    double nb;
    if (a.num_boxes_in) {
        nb = (double)a.num_boxes_in[0];
    } else {
        int cnt = 0;
        const int64_t *q_last = a.qot + (int64_t)(nl - 1) * a.cap;
        for (int64_t t = tid; t < total; t += kCritThreads) {
            const int64_t q = q_last[t];
            cnt += q >= 0 && q < a.Q;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) s_int[wave] = cnt;
        __syncthreads();
        cnt = 0;
        for (int w = 0; w < kCritThreads / 64; ++w) cnt += s_int[w];
        nb = cnt > 1 ? (double)cnt : 1.0;
    }
    const float w_m = (float)(1.0 / nb), w_d = (float)(1.0 / (nb * (double)groups));

    // ---- the row weights ---------------------------------------------------------------------------------------------------------------------
    int blk = blockIdx.x;
    if (blk >= L.grid_pairs) {
        const int64_t r = (int64_t)(blk - L.grid_pairs) * kCritThreads + tid;
        const int64_t rows_dec = (int64_t)nl * N * QT;
        if (r < rows_dec) {
            const int s = (int)(r % QT);
            a.row_weight[r] = s >= a.pad_cap ? w_m : (!overflow && s < pad_size ? w_d : 0.f);
            if (a.row_group) {
                const int l = (int)(r / ((int64_t)N * QT));
                a.row_group[r] = s >= a.pad_cap ? l : nl + l;
            }
        } else if (r < rows_dec + (int64_t)N * a.Qi) {
            a.row_weight_int[r - rows_dec] = w_m;
            if (a.row_group_int) a.row_group_int[r - rows_dec] = 2 * nl;
        }
        return;
    }

    // ---- one slot ----------------------------------------------------------------------------------------------------------------------------
    const bool matched = blk < (nl + 1) * L.blocks_m;
    int64_t slot;                 // the slot's record
    int row = -1, label = 0;      // the prediction's row in its tensor; -1: a dead slot
    int64_t t = -1;               // its target
    bool two_stage = false;
    float w = 0.f;
    int n_noquery = 0, n_badlabel = 0;
    bool in_range;
    if (matched) {
        const int o = blk / L.blocks_m;
        const int64_t tt = (int64_t)(blk - o * L.blocks_m) * kCritThreads + tid;
        in_range = tt < a.cap;
        slot = (int64_t)o * a.cap + tt;
        two_stage = o == nl;
        if (in_range && tt < total) {
            const int64_t q = a.qot[slot];
            const int nq = two_stage ? a.Qi : a.Q;
            if (q >= 0 && q < nq) {
                const int b = crit_image_of(s_cum, N, tt);
                row = two_stage ? b * a.Qi + (int)q : (o * N + b) * QT + a.pad_cap + (int)q;
                t = tt;
                w = w_m;
            } else {
                n_noquery = 1;
            }
            if (o == nl - 1) {      // (every live target's label is looked at once: by the last decoder output's slots)
                const int64_t lab = a.tgt_ids[tt];
                n_badlabel = lab < 0 || lab >= a.C;
            }
        }
    } else {
        const int d = blk - (nl + 1) * L.blocks_m;
        const int l = d / L.blocks_d;
        const int64_t bs = (int64_t)(d - l * L.blocks_d) * kCritThreads + tid;
        in_range = bs < (int64_t)N * a.pad_cap;
        slot = L.slots_m + (int64_t)l * N * a.pad_cap + bs;
        if (in_range && cum_ok && !overflow) {
            const int b = (int)(bs / a.pad_cap), s = (int)(bs - (int64_t)b * a.pad_cap);
            if (s < pad_size) {
                const int j = s % stride;
                if (j < s_cum[b + 1] - s_cum[b]) {
                    row = (l * N + b) * QT + s;
                    t = s_cum[b] + j;
                    w = w_d;
                }
            }
        }
    }
    float v_cls = 0.f, v_l1 = 0.f, v_giou = 0.f, gx = 0.f;
    float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0) {
        const int64_t lab = two_stage && (a.flags & 1) ? 0 : a.tgt_ids[t];
        if (lab < 0 || lab >= a.C) {
            row = -1;      // skipped: nothing is read through the label
        } else {
            label = (int)lab;
            const float *xs = two_stage ? a.il : a.logits;
            const float *ps = two_stage ? a.ib : a.coords;
            float dl;
            const float lc = crit::focal_pos_term(xs[(int64_t)row * a.C + label], a.alpha, dl);
            v_cls = lc * w;
            gx = a.c_cls * (dl * w);
            crit::Dual4 l1, giou;
            crit::box_pair_terms(reinterpret_cast<const float4 *>(ps)[row], reinterpret_cast<const float4 *>(a.tgt_boxes)[t], l1, giou);
            const crit::Dual4 lb = crit::box_pair_loss(l1, giou, a.c_l1, a.c_giou);
            v_l1 = l1.v * w;
            v_giou = (1.f - giou.v) * w;
            gb = make_float4(lb.d[0] * w, lb.d[1] * w, lb.d[2] * w, lb.d[3] * w);
        }
    }
    if (in_range) {
        a.rec_row[slot] = row;
        a.rec_label[slot] = label;
        a.rec_gx[slot] = gx;
        a.rec_gb[slot] = gb;
    }
    // ---- this workgroup's partials: wave shuffles, then the waves in order, in float64 -------------------------------------------------------
    v_cls = crit_wave_sum(v_cls);
    v_l1 = crit_wave_sum(v_l1);
    v_giou = crit_wave_sum(v_giou);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_noquery += __shfl_xor(n_noquery, o);
        n_badlabel += __shfl_xor(n_badlabel, o);
    }
    __syncthreads();      // (s_int was read above)
    if (lane == 0) {
        s_red[0][wave] = v_cls;
        s_red[1][wave] = v_l1;
        s_red[2][wave] = v_giou;
        s_int[wave] = n_noquery;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
        for (int w2 = 0; w2 < kCritThreads / 64; ++w2) s += (double)s_red[tid][w2];
        a.partial[(int64_t)blk * 3 + tid] = s;
    }
    if (tid == 3) {
        int s = 0;
        for (int w2 = 0; w2 < kCritThreads / 64; ++w2) s += s_int[w2];
        a.stat[(int64_t)blk * 4 + 1] = s;
        a.stat[(int64_t)blk * 4 + 0] = blk == 0 && overflow ? 1 : 0;
        a.stat[(int64_t)blk * 4 + 3] = blk == 0 && !cum_ok ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) s_int[wave] = n_badlabel;
    __syncthreads();
    if (tid == 3) {
        int s = 0;
        for (int w2 = 0; w2 < kCritThreads / 64; ++w2) s += s_int[w2];
        a.stat[(int64_t)blk * 4 + 2] = s;
    }
}

// terms (2 nl + 1, 3) and status[4] from the workgroups' partials, each call's in workgroup order: one workgroup of 64
__global__ __launch_bounds__(64) void criterion_reduce_kernel(const double *__restrict__ partial, const int32_t *__restrict__ stat, int nl, CritLayout L,
                                                              float *__restrict__ terms, int32_t *__restrict__ status)
{
    const int n_calls = 2 * nl + 1;
    for (int i = threadIdx.x; i < n_calls * 3; i += 64) {
        const int call = i / 3, k = i - call * 3;
        // call -> its workgroups: layers' matching parts 0..nl-1, their denoising parts nl..2nl-1, the two-stage output 2 nl
        int first, count;
        if (call < nl) { first = call * L.blocks_m; count = L.blocks_m; }
        else if (call < 2 * nl) { first = (nl + 1) * L.blocks_m + (call - nl) * L.blocks_d; count = L.blocks_d; }
        else { first = nl * L.blocks_m; count = L.blocks_m; }
        double s = 0.0;
        for (int g = 0; g < count; ++g) s += partial[(int64_t)(first + g) * 3 + k];
        terms[i] = (float)s;
    }
    if (threadIdx.x < 4) {
        long long s = 0;
        for (int g = 0; g < L.grid_pairs; ++g) s += stat[(int64_t)g * 4 + threadIdx.x];
        status[threadIdx.x] = s > 0x7fffffffll ? 0x7fffffff : (int32_t)s;
    }
}

// The backward of the pair terms.  grad_coords / grad_ib are written whole (zero where no slot points); the positive entries' gradients are
// ADDED to grad_logits / grad_il, which msda_focal_neg_grad_f32 has written before on the same stream.  Workgroup (o, b) owns the matching
// rows of output o, image b -- it clears them, then scatters the records of image b's targets, which point nowhere else --; a denoising
// slot IS a row, so the remaining workgroups write one row per thread.  Every positive entry is touched by one slot: plain read-modify-write.
struct CritBackArgs {
    const float4 *rec_gb;
    const float *rec_gx;
    const int32_t *rec_row, *rec_label;
    const int64_t *cum;
    const float *gscale;
    int nl, N, Q, Qi, C, pad_cap;
    int64_t cap;
    float *grad_logits, *grad_il;
    float4 *grad_coords, *grad_ib;
};

__global__ __launch_bounds__(kCritThreads) void criterion_pairs_backward_kernel(CritBackArgs a, CritLayout L)
{
    const int tid = threadIdx.x, N = a.N, nl = a.nl, QT = a.pad_cap + a.Q;
    const float g = a.gscale[0];
    const int n_ob = (nl + 1) * N;
    if ((int)blockIdx.x < n_ob) {
        const int o = blockIdx.x / N, b = blockIdx.x - o * N;
        const bool two_stage = o == nl;
        const int nq = two_stage ? a.Qi : a.Q;
        float4 *rows = two_stage ? a.grad_ib + (int64_t)b * a.Qi : a.grad_coords + ((int64_t)(o * N + b) * QT + a.pad_cap);
        for (int q = tid; q < nq; q += kCritThreads) rows[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
        // image b's targets, as far as they lie inside the capacity (the forward left every slot outside a valid prefix dead)
        int64_t t0 = a.cum[b], t1 = a.cum[b + 1];
        t0 = t0 < 0 ? 0 : t0;
        t1 = t1 > a.cap ? a.cap : t1;
        float4 *base = two_stage ? a.grad_ib : a.grad_coords;
        float *gl = two_stage ? a.grad_il : a.grad_logits;
        const int row_lo = two_stage ? b * a.Qi : (o * N + b) * QT + a.pad_cap;
        for (int64_t t = t0 + tid; t < t1; t += kCritThreads) {
            const int64_t slot = (int64_t)o * a.cap + t;
            const int row = a.rec_row[slot];
            if (row < row_lo || row >= row_lo + nq) continue;      // dead, or not this workgroup's: nothing written
            const float4 gb = a.rec_gb[slot];
            base[row] = make_float4(gb.x * g, gb.y * g, gb.z * g, gb.w * g);
            gl[(int64_t)row * a.C + a.rec_label[slot]] += a.rec_gx[slot] * g;
        }
        return;
    }
    const int64_t i = (int64_t)(blockIdx.x - n_ob) * kCritThreads + tid;      // (l, b, s) = the denoising slot and the row
    if (i >= L.slots_d) return;
    const int64_t lb = i / a.pad_cap;
    const int s = (int)(i - lb * a.pad_cap);
    const int64_t row_here = lb * QT + s;
    const int64_t slot = L.slots_m + i;
    const int row = a.rec_row[slot];
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0 && row == row_here) {
        const float4 gb = a.rec_gb[slot];
        out = make_float4(gb.x * g, gb.y * g, gb.z * g, gb.w * g);
        a.grad_logits[row_here * a.C + a.rec_label[slot]] += a.rec_gx[slot] * g;
    }
    a.grad_coords[row_here] = out;
}

}  // namespace msda
