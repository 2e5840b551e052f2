// msda_distill_pairs.h -- the distillation term over CAPACITY buffers: which (student row, teacher row) pairs carry the loss is read on the
// device, and the gradient rows go back to the student's tensor without an atomic.  Included by distill_api.hip.
//
// distill_pairs_kernel writes the arguments msda_distill_kl_f32 / _bf16 / msda_distill_l1_f32 (msda_distill.h) take -- pred_row, tgt_row,
// row_weight, row_group -- for a slot space the capacities fix; those kernels skip a row whose index is negative or whose weight is 0, so
// they run unchanged over all K slots.  The slots are those of msda_criterion.h, for the n_d decoder layers `layer_mask` selects (bit l =
// decoder layer l; the student tensor (n_d, N, pad_cap + Q, C) stacks them in increasing order, QT = pad_cap + Q):
//   matched   k = i * capacity + t                      live iff t < cum[N] and 0 <= q = query_of_target[layer_i][t] < Q;  image b from cum
//             pred_row = (i * N + b) * QT + pad_cap + q;  tgt_row = t ('gt') or pred_row ('pred');  weight 1 / num_boxes;  row_group = i
//   denoising k = n_d * capacity + (i * N + b) * pad_cap + s   from meta = (single_pad, num_dn_group, pad_size, total, overflow):
//             live iff no overflow, s < pad_size and j = s % (pad_size / num_dn_group) < T_b
//             pred_row = (i * N + b) * QT + s;  tgt_row = cum[b] + j or pred_row;  weight 1 / (num_boxes * num_dn_group);  row_group = n_d + i
//   a dead slot gets pred_row = tgt_row = -1 and weight 0 (its row_group is still its call's).
// num_boxes = max(1, live pairs of the LAST decoder output (row nl - 1 of query_of_target)), counted by every workgroup for itself, or the
// caller's value.  Weights are formed in float64 and rounded once.  Everything else is integer: the results are exact.
// status int32[4] (the words of msda_criterion_pairs_f32): [0] the denoising layout does not fit, [1] live targets without a query over the
// n_d selected layers, [2] always 0 (no label is read), [3] cum does not start at 0, decreases or exceeds the capacity: every slot is dead.
// Workgroup 0 counts [1] by itself: one launch, no workspace, no atomic.
//
// distill_scatter_kernel is the backward: grad_pred (n_d, N, QT, C) <- gscale[0] * grad_rows[k] at pred_row[k] for the live slots, written
// WHOLE (zero elsewhere), with plain stores.  A workgroup per destination row (grid-stride): a denoising row IS a slot; a matching row finds
// its slot among its image's targets (cum[b] .. cum[b + 1], a few hundred int64 at most).  A dead row reads nothing of grad_rows.  The
// product is formed in float32 (one rounding; + 0 so that a negative zero becomes the +0 an accumulation into zeros leaves) and, for a bf16
// student, rounded to bf16 once.  Rows are C elements wide and C is arbitrary (1203 in the workload), so a row starts at any element:
// 16-byte stores run between a scalar head and tail.  The assignment is one-to-one per image and output (msda_lsap_*); if a hand-made
// query_of_target sends two live targets of an image to one query, the row of the LARGER target index lands (the row kernels still count
// both in the loss): such input has no defined gradient here.
#pragma once

#include <stdint.h>

#include "msda_common.h"

namespace msda {

constexpr int kDistPairThreads = 256;
constexpr int kDistPairMaxImages = 1024;      // cum is kept in LDS

struct DistPairArgs {
    const int64_t *cum, *qot, *meta;
    const float *num_boxes_in;
    int nl, N, Q, pad_cap, n_d, objective;
    int64_t cap;
    unsigned long long layer_mask;
    int64_t *pred_row, *tgt_row;
    float *row_weight;
    int32_t *row_group, *status;
};

// the decoder layer of the i-th set bit of mask
__device__ __forceinline__ int dist_layer_of(unsigned long long mask, int i)
{
    int l = 0;
    for (;; ++l) {
        if (mask >> l & 1ull) {
            if (i == 0) break;
            --i;
        }
    }
    return l;
}

__global__ __launch_bounds__(kDistPairThreads) void distill_pairs_kernel(DistPairArgs a, int blocks_m, int blocks_d)
{
    __shared__ int64_t s_cum[kDistPairMaxImages + 1];
    __shared__ int s_int[kDistPairThreads / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = a.N, QT = a.pad_cap + a.Q;

    // ---- cum into LDS, checked: nothing is read through a prefix that does not describe targets inside the capacity ------------------
    for (int i = tid; i <= N; i += kDistPairThreads) s_cum[i] = a.cum[i];
    if (tid == 0) s_bad = 0;
    __syncthreads();
    {
        bool bad = false;
        for (int i = tid; i <= N; i += kDistPairThreads) {
            const int64_t v = s_cum[i];
            bad |= i == 0 ? v != 0 : v < s_cum[i - 1];
            bad |= v > a.cap;
        }
        if (bad) s_bad = 1;      // (any thread: the same value)
    }
    __syncthreads();
    const bool cum_ok = s_bad == 0;
    const int64_t total = cum_ok ? s_cum[N] : 0;

    // ---- the denoising layout (msda_criterion.h) -----------------------------------------------------------------------------------------
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

    // ---- num_boxes: live pairs of the last decoder output, clamped to >= 1 -- or the caller's ---------------------------------------------
    double nb;
    if (a.num_boxes_in) {
        nb = (double)a.num_boxes_in[0];
    } else {
        int cnt = 0;
        const int64_t *q_last = a.qot + (int64_t)(a.nl - 1) * a.cap;
        for (int64_t t = tid; t < total; t += kDistPairThreads) {
            const int64_t q = q_last[t];
            cnt += q >= 0 && q < a.Q;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) s_int[wave] = cnt;
        __syncthreads();
        cnt = 0;
        for (int w = 0; w < kDistPairThreads / 64; ++w) cnt += s_int[w];
        nb = cnt > 1 ? (double)cnt : 1.0;
        __syncthreads();      // (s_int is used again below)
    }
    const float w_m = (float)(1.0 / nb), w_d = (float)(1.0 / (nb * (double)groups));

    // ---- the status: workgroup 0 looks at every live target of the selected layers -----------------------------------------------------------
    if (blockIdx.x == 0) {
        int cnt = 0;
        for (int i = 0; i < a.n_d; ++i) {
            const int64_t *q_i = a.qot + (int64_t)dist_layer_of(a.layer_mask, i) * a.cap;
            for (int64_t t = tid; t < total; t += kDistPairThreads) {
                const int64_t q = q_i[t];
                cnt += !(q >= 0 && q < a.Q);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0) s_int[wave] = cnt;
        __syncthreads();
        if (tid == 0) {
            int s = 0;
            for (int w = 0; w < kDistPairThreads / 64; ++w) s += s_int[w];
            a.status[0] = overflow ? 1 : 0;
            a.status[1] = s;
            a.status[2] = 0;
            a.status[3] = cum_ok ? 0 : 1;
        }
    }

    // ---- one slot ----------------------------------------------------------------------------------------------------------------------------
    const int blk = blockIdx.x;
    int64_t k, row = -1, trow = -1;
    int group;
    float w = 0.f;
    if (blk < a.n_d * blocks_m) {
        const int i = blk / blocks_m;
        const int64_t t = (int64_t)(blk - i * blocks_m) * kDistPairThreads + tid;
        if (t >= a.cap) return;
        k = (int64_t)i * a.cap + t;
        group = i;
        if (t < total) {
            const int64_t q = a.qot[(int64_t)dist_layer_of(a.layer_mask, i) * a.cap + t];
            if (q >= 0 && q < a.Q) {
                int lo = 1, hi = N;      // the first index in [1, N] whose cum is > t (cum[N] is)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_cum[mid] > t) hi = mid;
                    else lo = mid + 1;
                }
                row = ((int64_t)i * N + (lo - 1)) * QT + a.pad_cap + q;
                trow = t;
                w = w_m;
            }
        }
    } else {
        const int d = blk - a.n_d * blocks_m;
        const int i = d / blocks_d;
        const int64_t bs = (int64_t)(d - i * blocks_d) * kDistPairThreads + tid;
        if (bs >= (int64_t)N * a.pad_cap) return;
        k = (int64_t)a.n_d * a.cap + (int64_t)i * N * a.pad_cap + bs;
        group = a.n_d + i;
        if (cum_ok && !overflow) {
            const int b = (int)(bs / a.pad_cap), s = (int)(bs - (int64_t)b * a.pad_cap);
            if (s < pad_size) {
                const int j = s % stride;
                if (j < s_cum[b + 1] - s_cum[b]) {
                    row = ((int64_t)i * N + b) * QT + s;
                    trow = s_cum[b] + j;
                    w = w_d;
                }
            }
        }
    }
    a.pred_row[k] = row;
    a.tgt_row[k] = a.objective == 0 ? trow : row;
    a.row_weight[k] = w;
    a.row_group[k] = group;
}

// ---- the backward ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dist_scaled(float g, float v) { return __fadd_rn(__fmul_rn(g, v), 0.f); }

// one destination row: dst[0..C) <- g * src[0..C) (src == nullptr: zeros).  16-byte stores between a scalar head and tail.
__device__ __forceinline__ void dist_store_row(float *dst, const float *src, float g, int C, int tid, int nthreads)
{
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
    if (head > C) head = C;
    const int n4 = (C - head) >> 2;
    if (tid < head) dst[tid] = src ? dist_scaled(g, src[tid]) : 0.f;
    float4 *d4 = reinterpret_cast<float4 *>(dst + head);
    for (int i = tid; i < n4; i += nthreads) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src) {
            const float *s = src + head + 4 * i;
            v = make_float4(dist_scaled(g, s[0]), dist_scaled(g, s[1]), dist_scaled(g, s[2]), dist_scaled(g, s[3]));
        }
        d4[i] = v;
    }
    for (int i = head + 4 * n4 + tid; i < C; i += nthreads) dst[i] = src ? dist_scaled(g, src[i]) : 0.f;
}

__device__ __forceinline__ unsigned short dist_bf16_bits(float v)
{
    const bf16_t h = __float2bfloat16(v);      // round to nearest even
    return *reinterpret_cast<const unsigned short *>(&h);
}

// the same for a bf16 destination: 8 elements per 16-byte store
__device__ __forceinline__ void dist_store_row(bf16_t *dst, const float *src, float g, int C, int tid, int nthreads)
{
    unsigned short *d = reinterpret_cast<unsigned short *>(dst);
    int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 1);
    if (head > C) head = C;
    const int n8 = (C - head) >> 3;
    if (tid < head) d[tid] = src ? dist_bf16_bits(dist_scaled(g, src[tid])) : (unsigned short)0;
    uint4 *d8 = reinterpret_cast<uint4 *>(d + head);
    for (int i = tid; i < n8; i += nthreads) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src) {
            const float *s = src + head + 8 * i;
            unsigned r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                r[j] = (unsigned)dist_bf16_bits(dist_scaled(g, s[2 * j])) | (unsigned)dist_bf16_bits(dist_scaled(g, s[2 * j + 1])) << 16;
            v = make_uint4(r[0], r[1], r[2], r[3]);
        }
        d8[i] = v;
    }
    for (int i = head + 8 * n8 + tid; i < C; i += nthreads) d[i] = src ? dist_bf16_bits(dist_scaled(g, src[i])) : (unsigned short)0;
}

template <typename TP>
__global__ __launch_bounds__(kDistPairThreads) void distill_scatter_kernel(const float *__restrict__ grad_rows, const int64_t *__restrict__ pred_row,
                                                                           const int64_t *__restrict__ cum, const float *__restrict__ gscale,
                                                                           int n_d, int N, int Q, int pad_cap, int64_t cap, int C,
                                                                           TP *__restrict__ grad_pred)
{
    __shared__ long long s_found[kDistPairThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int QT = pad_cap + Q;
    const int64_t rows = (int64_t)n_d * N * QT;
    const float g = gscale[0];
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {      // (everything that decides a branch below is uniform over the workgroup)
        const int64_t ib = r / QT;
        const int s = (int)(r - ib * QT);
        long long k = -1;
        if (s < pad_cap) {
            const int64_t kk = (int64_t)n_d * cap + ib * pad_cap + s;
            if (pred_row[kk] == r) k = kk;
        } else {
            const int i = (int)(ib / N), b = (int)(ib - (int64_t)i * N);
            int64_t t0 = cum[b], t1 = cum[b + 1];      // (the forward left every slot outside a valid prefix dead: clamping is enough)
            t0 = t0 < 0 ? 0 : t0;
            t1 = t1 > cap ? cap : t1;
            long long mine = -1;
            for (int64_t t = t0 + tid; t < t1; t += kDistPairThreads) {
                const int64_t kk = (int64_t)i * cap + t;
                if (pred_row[kk] == r) mine = kk;      // (increasing t: the largest stays)
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long other = __shfl_xor(mine, o);
                mine = other > mine ? other : mine;
            }
            __syncthreads();      // (the previous row's readers of s_found are done)
            if (lane == 0) s_found[wave] = mine;
            __syncthreads();
            k = s_found[0];
            for (int w = 1; w < kDistPairThreads / 64; ++w) k = s_found[w] > k ? s_found[w] : k;
        }
        dist_store_row(grad_pred + r * C, k >= 0 ? grad_rows + k * C : nullptr, g, C, tid, kDistPairThreads);
    }
}

}  // namespace msda
