// msda_distill.h -- the CLIP distillation term of the criterion (reference SetCriterion.loss_labels, models/richsem/richsem.py:967-1024): the
// detector's CLIP-space outputs pulled toward the frozen teacher's, as a KL divergence of class distributions (distill_type 'clip_logits')
// or an L1 distance of unit vectors ('clip_l1'), over gathered rows.  Included by rows_api.hip.
//
// Both are row kernels: one workgroup of 256 threads per gathered row k, grid-stride over the rows; row k reads pred[pred_row[k]] and
// tgt[tgt_row[k]] (the gather is part of the kernel: no copy of the rows is made), f32 arithmetic, the row reductions by wave shuffles and one
// LDS exchange in a fixed order.  The value and the compact gradient grad_rows (K, C) come from the one launch; the caller scatters the
// gradient rows.  Each workgroup adds its rows' losses up in f64 and leaves one partial in the CALLER's workspace (kDistillMaxGrid doubles:
// the library owns no memory here, so a call is as capturable and as stream-safe as its arguments); a second, single-workgroup launch adds
// the partials in a fixed order.  There is no floating-point atomic anywhere: the same inputs give the same bits.
//
// KL form, S_k = the class subset of row k (all C classes, or those with class_mask[row_group[k]][c] != 0):
//     p = softmax(pred row over S_k), t = softmax(tgt row over S_k)
//     row_loss_k = w_k dw_k sum_{c in S_k} t_c (log t_c - log p_c),      grad_rows[k][c] = w_k dw_k (p_c - t_c) on S_k, exactly 0 elsewhere
//     dw_k = 1, or with dynamic_weight 2 H(softmax(tgt row over ALL C classes)) / ln C (the reference forms it before the fed slicing)
// log t and log p are formed analytically (x - max - log sum exp), so an underflowed t_c = 0 contributes exactly 0: F.kl_div's xlogy
// convention.  The entropy H = -sum t log t is formed the same way (log Z - sum e (y - max) / Z); THE REFERENCE DIFFERS THERE: it computes
// tgt_prob * tgt_prob.log(), which is 0 * -inf = NaN once a probability underflows (a logit more than ~103 below the row's maximum in
// float32).  Here no term is NaN for finite inputs, and H is clamped at 0 from below (rounding can leave -1e-7 at a one-hot teacher).
//
// L1 form:  u = pred row / |pred row|_2,  v = tgt row (normalize_target = 0) or tgt row / |tgt row|_2 (1)
//     row_loss_k = w_k |u - v|_1,   grad_rows[k] = w_k (s - u (u . s)) / |pred row|_2,   s = sign(u - v), sign(0) = 0 as torch differentiates |x|
// A zero pred row divides by zero as the reference does.
//
// In both forms a row contributes loss 0 and a zero gradient row when w_k == 0, when its row_group lies outside [0, groups), when its subset
// is empty, or when pred_row[k] / tgt_row[k] lies outside [0, pred_rows) / [0, tgt_rows): the indices are device data, the kernel guards them.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "msda_common.h"

namespace msda {

constexpr int kDistillThreads = 256;
constexpr int kDistillWaves = kDistillThreads / kWave;
constexpr int kDistillCache = 8;             // row elements a thread keeps in registers: rows up to 2048 wide are read from memory once
constexpr int kDistillMaxGrid = 2048;        // workgroups (= f64 partials) per call: 8 per CU

struct DistillSum {
    __device__ static float id() { return 0.f; }
    __device__ static float op(float a, float b) { return a + b; }
};
struct DistillMax {
    __device__ static float id() { return -INFINITY; }
    __device__ static float op(float a, float b) { return fmaxf(a, b); }
};

// N values per thread -> their reduction over the workgroup, in every thread.  red: N * kDistillWaves floats of LDS; the leading barrier
// keeps the previous use of `red` apart.
template <typename Op, int N>
__device__ __forceinline__ void distill_reduce(float (&v)[N], float *red)
{
#pragma unroll
    for (int j = 0; j < N; ++j)
        for (int o = kWave / 2; o > 0; o >>= 1) v[j] = Op::op(v[j], __shfl_xor(v[j], o, kWave));
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[j * kDistillWaves + (threadIdx.x / kWave)] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float s = red[j * kDistillWaves];
#pragma unroll
        for (int w = 1; w < kDistillWaves; ++w) s = Op::op(s, red[j * kDistillWaves + w]);
        v[j] = s;
    }
}

// the rows' losses of this workgroup (the same value in every thread) -> partial[blockIdx.x], or straight to loss[0] when it is the only one
__device__ __forceinline__ void distill_leave_partial(double acc, double *__restrict__ partial, float *__restrict__ loss)
{
    if (threadIdx.x != 0) return;
    if (gridDim.x == 1) loss[0] = (float)acc;
    else partial[blockIdx.x] = acc;
}

// loss[0] <- partial[0] + ... + partial[n - 1] in f64, a fixed tree
__global__ __launch_bounds__(kDistillThreads) void distill_total_kernel(const double *__restrict__ partial, int n, float *__restrict__ loss)
{
    __shared__ double red[kDistillThreads];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += kDistillThreads) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = kDistillThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
}

template <typename TP>
__global__ __launch_bounds__(kDistillThreads) void distill_kl_kernel(const TP *__restrict__ pred, long long pred_rows, const float *__restrict__ tgt,
                                                                     long long tgt_rows, int C, const int64_t *__restrict__ pred_row,
                                                                     const int64_t *__restrict__ tgt_row, const float *__restrict__ row_weight,
                                                                     long long K, const int32_t *__restrict__ row_group,
                                                                     const float *__restrict__ class_mask, int groups, int dynamic_weight,
                                                                     double *__restrict__ partial, float *__restrict__ loss,
                                                                     float *__restrict__ grad_rows)
{
    __shared__ float red[4 * kDistillWaves];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long k = blockIdx.x; k < K; k += gridDim.x) {      // (everything that decides a branch below is uniform over the workgroup)
        float *__restrict__ g = grad_rows + k * C;
        const float wk = row_weight[k];
        const long long pr = pred_row[k], tr = tgt_row[k];
        const int gr = class_mask ? row_group[k] : 0;
        const bool live = wk != 0.f && pr >= 0 && pr < pred_rows && tr >= 0 && tr < tgt_rows && gr >= 0 && (!class_mask || gr < groups);
        if (!live) {
            for (int c = tid; c < C; c += kDistillThreads) g[c] = 0.f;
            continue;
        }
        const TP *__restrict__ x = pred + pr * C;
        const float *__restrict__ y = tgt + tr * C;
        const float *__restrict__ m = class_mask ? class_mask + (long long)gr * C : nullptr;
        float xs[kDistillCache], ys[kDistillCache];
        unsigned in_s = 0u;
#pragma unroll
        for (int i = 0; i < kDistillCache; ++i) {
            const int c = tid + i * kDistillThreads;
            xs[i] = ys[i] = 0.f;
            if (c < C) {
                xs[i] = ld1(x + c);
                ys[i] = y[c];
                if (!m || m[c] != 0.f) in_s |= 1u << i;
            }
        }
        // f(c, x_c, y_c, c in S_k) over this thread's classes: the cached ones, then what lies past the cache
        auto each = [&](auto f) {
#pragma unroll
            for (int i = 0; i < kDistillCache; ++i) {
                const int c = tid + i * kDistillThreads;
                if (c < C) f(c, xs[i], ys[i], (in_s >> i & 1u) != 0u);
            }
            for (int c = tid + kDistillCache * kDistillThreads; c < C; c += kDistillThreads) f(c, ld1(x + c), y[c], !m || m[c] != 0.f);
        };
        // 1: the maxima over the subset, and of the whole teacher row
        float mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        int any_s = 0;      // does this thread hold a class of the subset -- among ALL its classes, the cached ones and those past the cache
        each([&](int, float xv, float yv, bool s) {
            if (s) {
                any_s = 1;
                mx[0] = fmaxf(mx[0], xv);
                mx[1] = fmaxf(mx[1], yv);
            }
            mx[2] = fmaxf(mx[2], yv);
        });
        distill_reduce<DistillMax>(mx, red);
        if (__syncthreads_or(any_s) == 0) {      // an empty subset
            for (int c = tid; c < C; c += kDistillThreads) g[c] = 0.f;
            continue;
        }
        // 2: the partition sums; with the dynamic weight also those of the whole teacher row's entropy
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        each([&](int, float xv, float yv, bool s) {
            if (s) {
                z[0] += expf(xv - mx[0]);
                z[1] += expf(yv - mx[1]);
            }
            if (dynamic_weight) {
                const float d = yv - mx[2], e = expf(d);
                z[2] += e;
                z[3] += e * d;      // (e = 0 where it underflows: the term is 0, not NaN)
            }
        });
        distill_reduce<DistillSum>(z, red);
        float dw = 1.f;
        if (dynamic_weight) dw = 2.f * fmaxf(logf(z[2]) - z[3] / z[2], 0.f) / logf((float)C);
        const float scale = wk * dw, log_zp = logf(z[0]), log_zt = logf(z[1]), inv_zp = 1.f / z[0], inv_zt = 1.f / z[1];
        // 3: the divergence and the gradient row
        float kl[1] = {0.f};
        each([&](int c, float xv, float yv, bool s) {
            float gc = 0.f;
            if (s) {
                const float dx = xv - mx[0], dy = yv - mx[1];
                const float p = expf(dx) * inv_zp, t = expf(dy) * inv_zt;
                kl[0] += t * ((dy - log_zt) - (dx - log_zp));
                gc = scale * (p - t);
            }
            g[c] = gc;
        });
        distill_reduce<DistillSum>(kl, red);
        acc += (double)(scale * kl[0]);
    }
    distill_leave_partial(acc, partial, loss);
}

__global__ __launch_bounds__(kDistillThreads) void distill_l1_kernel(const float *__restrict__ pred, long long pred_rows, const float *__restrict__ tgt,
                                                                     long long tgt_rows, int D, const int64_t *__restrict__ pred_row,
                                                                     const int64_t *__restrict__ tgt_row, const float *__restrict__ row_weight,
                                                                     long long K, int normalize_target, double *__restrict__ partial,
                                                                     float *__restrict__ loss, float *__restrict__ grad_rows)
{
    __shared__ float red[2 * kDistillWaves];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (long long k = blockIdx.x; k < K; k += gridDim.x) {
        float *__restrict__ g = grad_rows + k * D;
        const float wk = row_weight[k];
        const long long pr = pred_row[k], tr = tgt_row[k];
        if (!(wk != 0.f && pr >= 0 && pr < pred_rows && tr >= 0 && tr < tgt_rows)) {
            for (int c = tid; c < D; c += kDistillThreads) g[c] = 0.f;
            continue;
        }
        const float *__restrict__ x = pred + pr * D;
        const float *__restrict__ y = tgt + tr * D;
        float xs[kDistillCache], ys[kDistillCache];
#pragma unroll
        for (int i = 0; i < kDistillCache; ++i) {
            const int c = tid + i * kDistillThreads;
            xs[i] = c < D ? x[c] : 0.f;
            ys[i] = c < D ? y[c] : 0.f;
        }
        auto each = [&](auto f) {
#pragma unroll
            for (int i = 0; i < kDistillCache; ++i) {
                const int c = tid + i * kDistillThreads;
                if (c < D) f(c, xs[i], ys[i]);
            }
            for (int c = tid + kDistillCache * kDistillThreads; c < D; c += kDistillThreads) f(c, x[c], y[c]);
        };
        float n2[2] = {0.f, 0.f};
        each([&](int, float xv, float yv) {
            n2[0] += xv * xv;
            n2[1] += yv * yv;
        });
        distill_reduce<DistillSum>(n2, red);
        const float nu = sqrtf(n2[0]), nv = normalize_target ? sqrtf(n2[1]) : 1.f;
        float s2[2] = {0.f, 0.f};      // |u - v|_1 and u . s
        each([&](int, float xv, float yv) {
            const float u = xv / nu, d = u - (normalize_target ? yv / nv : yv);
            s2[0] += fabsf(d);
            s2[1] += d > 0.f ? u : (d < 0.f ? -u : 0.f);
        });
        distill_reduce<DistillSum>(s2, red);
        each([&](int c, float xv, float yv) {
            const float u = xv / nu, d = u - (normalize_target ? yv / nv : yv);
            const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            g[c] = wk * (s - u * s2[1]) / nu;
        });
        acc += (double)(wk * s2[0]);
    }
    distill_leave_partial(acc, partial, loss);
}

}  // namespace msda
