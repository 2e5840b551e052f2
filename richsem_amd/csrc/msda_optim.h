// msda_optim.h -- gradient clipping + AdamW + EMA over a device-resident tensor table (include/richsem_msda.h: msda_optim_*).
//
// What follows losses.backward() in the reference's loop (engine.py:110-120): clip_grad_norm_(max_norm), AdamW.step(), ModelEma.update().
// Two launches over the same chunk table, one workgroup of kOptimThreads per chunk (at most MSDA_OPTIM_CHUNK elements of ONE tensor):
//
//   optim_sumsq_kernel   partial[c] = sum of g^2 over chunk c (double; a fixed order: thread t takes elements t, t + 256, ... of the head /
//                        body / tail split below, then a fixed tree over the threads); the chunk at offset 0 advances its tensor's step
//   optim_step_kernel    every workgroup adds up ALL partials in the same fixed order (so every workgroup holds the same bits), forms
//                        total_norm and the clip coefficient as clip_grad_norm_ does in fp32, the tensor's bias corrections in double
//                        (once, thread 0), then streams its chunk: p, g, m, v (and the EMA shadow) read once, p, m, v (shadow) written once
//
// No atomics, no LDS beyond the reduction tree and the broadcast of the per-workgroup constants.  The gradient is read, never written: the
// clipped gradient coef * g exists only in registers.
//
// Memory access: a chunk whose arrays share one address modulo 16 bytes is walked as a scalar head (up to 3 elements, to the 16-byte
// boundary), a float4 body and a scalar tail; a chunk whose arrays disagree (a parameter that is a view at a 4-byte-only aligned address,
// with a freshly allocated gradient) is walked element by element.  Chunk offsets are multiples of MSDA_OPTIM_CHUNK, so a tensor's
// chunks all take the same path.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/richsem_msda.h"

namespace msda {

constexpr int kOptimThreads = 256;

// The kernels get their data pointers out of a table in memory, where the compiler cannot see an address space and would use flat
// loads and stores; every one of them is global memory.
typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ inline gfloat *optim_global(const float *p) { return (gfloat *)reinterpret_cast<uintptr_t>(p); }
__device__ inline gf32x4 *optim_global4(const gfloat *p) { return (gf32x4 *)(uintptr_t)p; }

// head / body / tail of a chunk: `head` scalar elements, `nvec` float4, then `tail` scalar elements
struct OptimSplit {
    int head, nvec, tail;
};

// `bits`: the OR of (address ^ first address) over the chunk's arrays (zero in the low four bits = one address modulo 16)
__device__ inline OptimSplit optim_split(uintptr_t first, uintptr_t bits, int count)
{
    OptimSplit s;
    if (bits & 15) {
        s.head = count; s.nvec = 0; s.tail = 0;
        return s;
    }
    int head = (int)(((16 - (first & 15)) & 15) >> 2);
    if (head > count) head = count;
    s.head = head;
    s.nvec = (count - head) >> 2;
    s.tail = count - head - 4 * s.nvec;
    return s;
}

// fixed-order sum over the workgroup: a tree over LDS; every thread returns the total
__device__ inline double optim_block_sum(double x, double *red)
{
    const int t = threadIdx.x;
    red[t] = x;
    __syncthreads();
    for (int s = kOptimThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kOptimThreads) void optim_sumsq_kernel(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, double *partials)
{
    __shared__ double red[kOptimThreads];
    const msda_optim_chunk ck = chunks[blockIdx.x];
    const msda_optim_tensor *T = tensors + ck.tensor;
    const gfloat *g = optim_global(T->grad + ck.offset);
    const int t = threadIdx.x;
    if (t == 0 && ck.offset == 0) *T->step += 1.0f;      // (one workgroup per tensor: its first chunk)
    const OptimSplit sp = optim_split((uintptr_t)g, 0, ck.count);
    double acc = 0.0;
    for (int i = t; i < sp.head; i += kOptimThreads) {
        const double x = g[i];
        acc += x * x;
    }
    const gf32x4 *g4 = optim_global4(g + sp.head);
    for (int i = t; i < sp.nvec; i += kOptimThreads) {
        const f32x4 x = g4[i];
        acc += (double)x.x * x.x;
        acc += (double)x.y * x.y;
        acc += (double)x.z * x.z;
        acc += (double)x.w * x.w;
    }
    const gfloat *gt = g + sp.head + 4 * sp.nvec;
    for (int i = t; i < sp.tail; i += kOptimThreads) {
        const double x = gt[i];
        acc += x * x;
    }
    const double total = optim_block_sum(acc, red);
    if (t == 0) partials[blockIdx.x] = total;
}

// what one workgroup of the step kernel needs per element, formed once (thread 0) and broadcast through LDS
struct OptimConsts {
    float coef;         // clip coefficient: g' = coef * g
    float decay;        // 1 - lr * weight_decay
    float b1, omb1;     // beta1, 1 - beta1
    float b2, omb2;     // beta2, 1 - beta2
    float step_size;    // lr / (1 - beta1^step)
    float rsq_bc2;      // sqrt(1 - beta2^step): the denominator is sqrt(v) / rsq_bc2 + eps
    float eps;
    float ema_d, ema_omd;      // decay, 1 - decay of the shadow
    int ema;            // fold the shadow's update
};

__device__ inline void optim_update(const OptimConsts &c, float &p, float g, float &m, float &v)
{
    const float gc = c.coef * g;
    p = p * c.decay;
    m = c.b1 * m + c.omb1 * gc;
    v = c.b2 * v + c.omb2 * (gc * gc);
    const float denom = sqrtf(v) / c.rsq_bc2 + c.eps;
    p = p - c.step_size * m / denom;
}

__device__ inline float optim_ema(const OptimConsts &c, float e, float p) { return c.ema_d * e + c.ema_omd * p; }

__global__ __launch_bounds__(kOptimThreads) void optim_step_kernel(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks,
                                                                   const double *partials, const msda_optim_group *groups,
                                                                   const msda_optim_settings *settings, float *total_norm)
{
    __shared__ double red[kOptimThreads];
    __shared__ OptimConsts sc;
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int i = t; i < n_chunks; i += kOptimThreads) acc += partials[i];
    const double sumsq = optim_block_sum(acc, red);
    const msda_optim_chunk ck = chunks[blockIdx.x];
    const msda_optim_tensor T = tensors[ck.tensor];
    if (t == 0) {
        // clip_grad_norm_'s arithmetic in fp32: coef = min(1, max_norm / (total_norm + 1e-6)); a NaN stays a NaN (torch.clamp keeps it)
        const float tn = (float)sqrt(sumsq);
        float coef = 1.0f;
        if (settings->max_norm > 0.0) {
            const float q = (float)settings->max_norm / (tn + 1e-6f);
            coef = q > 1.0f ? 1.0f : q;
        }
        if (blockIdx.x == 0) *total_norm = tn;
        const msda_optim_group G = groups[T.group];
        const double step = (double)*T.step;
        const double bc1 = 1.0 - pow(G.beta1, step), bc2 = 1.0 - pow(G.beta2, step);
        OptimConsts c;
        c.coef = coef;
        c.decay = (float)(1.0 - G.lr * G.weight_decay);
        c.b1 = (float)G.beta1; c.omb1 = (float)(1.0 - G.beta1);
        c.b2 = (float)G.beta2; c.omb2 = (float)(1.0 - G.beta2);
        c.step_size = (float)(G.lr / bc1);
        c.rsq_bc2 = (float)sqrt(bc2);
        c.eps = (float)G.eps;
        c.ema_d = (float)settings->ema_decay; c.ema_omd = (float)(1.0 - settings->ema_decay);
        c.ema = settings->ema_on != 0 && T.ema != nullptr;
        sc = c;
    }
    __syncthreads();
    const OptimConsts c = sc;
    gfloat *p = optim_global(T.param + ck.offset), *m = optim_global(T.exp_avg + ck.offset), *v = optim_global(T.exp_avg_sq + ck.offset);
    const gfloat *g = optim_global(T.grad + ck.offset);
    gfloat *e = c.ema ? optim_global(T.ema + ck.offset) : nullptr;
    const uintptr_t a0 = (uintptr_t)p;
    uintptr_t bits = (a0 ^ (uintptr_t)g) | (a0 ^ (uintptr_t)m) | (a0 ^ (uintptr_t)v);
    if (e) bits |= a0 ^ (uintptr_t)e;
    const OptimSplit sp = optim_split(a0, bits, ck.count);
    const int vec0 = sp.head, tail0 = sp.head + 4 * sp.nvec;

    auto scalar = [&](int i) {
        float pi = p[i], mi = m[i], vi = v[i];
        optim_update(c, pi, g[i], mi, vi);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (e) e[i] = optim_ema(c, e[i], pi);
    };
    for (int i = t; i < sp.head; i += kOptimThreads) scalar(i);
    gf32x4 *p4 = optim_global4(p + vec0), *m4 = optim_global4(m + vec0), *v4 = optim_global4(v + vec0);
    const gf32x4 *g4 = optim_global4(g + vec0);
    gf32x4 *e4 = e ? optim_global4(e + vec0) : nullptr;
    for (int i = t; i < sp.nvec; i += kOptimThreads) {
        f32x4 pi = p4[i], mi = m4[i], vi = v4[i];
        const f32x4 gi = g4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pi[k], mk = mi[k], vk = vi[k];
            optim_update(c, pk, gi[k], mk, vk);
            pi[k] = pk; mi[k] = mk; vi[k] = vk;
        }
        p4[i] = pi; m4[i] = mi; v4[i] = vi;
        if (e4) {
            f32x4 ei = e4[i];
            ei.x = optim_ema(c, ei.x, pi.x); ei.y = optim_ema(c, ei.y, pi.y);
            ei.z = optim_ema(c, ei.z, pi.z); ei.w = optim_ema(c, ei.w, pi.w);
            e4[i] = ei;
        }
    }
    for (int i = tail0 + t; i < ck.count; i += kOptimThreads) scalar(i);
}

// e = decay * e + (1 - decay) * p over a table whose tensors carry `ema` and `param` only: the state an optimizer does not own
__global__ __launch_bounds__(kOptimThreads) void optim_ema_kernel(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks,
                                                                  const msda_optim_settings *settings)
{
    const msda_optim_chunk ck = chunks[blockIdx.x];
    const msda_optim_tensor T = tensors[ck.tensor];
    OptimConsts c;
    c.ema_d = (float)settings->ema_decay; c.ema_omd = (float)(1.0 - settings->ema_decay);
    const int t = threadIdx.x;
    gfloat *e = optim_global(T.ema + ck.offset);
    const gfloat *p = optim_global(T.param + ck.offset);
    const uintptr_t a0 = (uintptr_t)e;
    const OptimSplit sp = optim_split(a0, a0 ^ (uintptr_t)p, ck.count);
    const int vec0 = sp.head, tail0 = sp.head + 4 * sp.nvec;
    for (int i = t; i < sp.head; i += kOptimThreads) e[i] = optim_ema(c, e[i], p[i]);
    gf32x4 *e4 = optim_global4(e + vec0);
    const gf32x4 *p4 = optim_global4(p + vec0);
    for (int i = t; i < sp.nvec; i += kOptimThreads) {
        f32x4 ei = e4[i];
        const f32x4 pi = p4[i];
        ei.x = optim_ema(c, ei.x, pi.x); ei.y = optim_ema(c, ei.y, pi.y);
        ei.z = optim_ema(c, ei.z, pi.z); ei.w = optim_ema(c, ei.w, pi.w);
        e4[i] = ei;
    }
    for (int i = tail0 + t; i < ck.count; i += kOptimThreads) e[i] = optim_ema(c, e[i], p[i]);
}

}  // namespace msda
