// dynamic_masks.hip -- the CondInst dynamic mask head ("Dynamic mask head"): MaskBranch.dynamic_mask_with_coords of the
// reference (models/richsem/cond_inst.py:337-435 with compute_locations, parse_dynamic_params and aligned_bilinear of the same file) forward
// and backward.  C ABI msda_dynmask_* (include/richsem_msda.h).
//
// The contract.  feat (N, C, H, W), params (N, Q, P) and out (N, R, F H, F W) fp32 or bf16, read and written as stored; ref (N, Q, 2) fp32 the
// normalised reference point (x, y); sizes (N, 2) fp32 the image size (h, w); inst (N, R) int32: the query of output row r, anything outside
// [0, Q) = no query = a row of zeros.  C is 8 or 16, the hidden width 8, F = 2 (mask_out_stride 4) or 1 (mask_out_stride 8).
//
//   in         = [rx, ry, feat[n, :, y, x]],  rx = ref_x size_w - (8 x + 4),  ry = ref_y size_h - (8 y + 4)   (rel_coord = 0: the features alone)
//   t[y, x]    = w2 . relu(W1 relu(W0 in + b0) + b1) + b2
//   params row = W0 (8, Cin) row-major, W1 (8, 8), w2 (8), b0 (8), b1 (8), b2 (1):  P = 8 Cin + 89
//   out        = aligned_bilinear(t, F): per axis F[0] = T[0], F[2 k + 1] = T[k], F[2 k] = (T[k - 1] + T[k]) / 2
//   backward   dT[k] = dF[2 k + 1] + dF[2 k] / 2 + dF[2 k + 2] / 2 (dF[0] whole, terms past the end absent), the chain recomputed
//
// All arithmetic fp32; no atomics, no allocation, no synchronisation, every reduction in a fixed order.
//
// The cut.  A query's parameters are staged in LDS as fp32 in an order of the kernels' own (DmLay: the two coordinate columns of W0 apart, every
// block a multiple of four floats, so the wave-uniform reads are 16-byte broadcasts); a lane holds ONE stride-8 pixel's features in registers.
//   dynmask_table_kernel     inst from int64 rows, from (offsets, query_of_target) -- inst[n, q] = q where the image has a pair for q -- or
//                            the identity.
//   dynmask_fwd_kernel       a workgroup takes (image, tile of 8 x 32 pixels, chunk of 16 rows).  For F = 2 the tile's first row and column are
//                            the halo (7 x 31 pixels are owned): four rows' logits go to LDS, then every owning lane writes the 2 x 2 outputs of
//                            its pixel from its own logit and the three to the top and left.  Dead rows: plain zero stores.
//   dynmask_bwd_kernel       a workgroup takes (image, tile of 8 x 32 pixels) and walks the rows in ascending order, skipping dead ones: dT
//                            gathered from grad_out (nine taps), the chain recomputed, grad_feat accumulated in registers, the parameter
//                            gradients summed over the wave's lanes by a halving butterfly (64 values at a time: after six exchange steps lane l
//                            holds value l), over the four waves in wave order: one partial row of DmLay::PS per (image, tile, row).
//   dynmask_sum_kernel       a workgroup per (image, query): the rows that name the query in ascending order, their tiles in ascending order ->
//                            grad_params in the reference's order and grad_ref; exact zeros for a query no row names.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msda_host.h"

namespace {

constexpr int kDmTH = 8, kDmTW = 32;      // the pixel tile: one pixel per lane of 256
constexpr int kDmRows = 16;               // output rows per forward workgroup
constexpr int kDmBatch = 4;               // rows whose logits are in LDS at once
constexpr int kDmHid = 8;                 // the dynamic width

// the parameters of one query in LDS
template <int C>
struct DmLay {
    static constexpr int Wc = 0;                 // W0[:, 0:2]  (8, 2)
    static constexpr int Wf = 16;                // W0[:, 2:]   (8, C)
    static constexpr int W1 = 16 + 8 * C;        // (8, 8)
    static constexpr int w2 = W1 + 64;
    static constexpr int b0 = w2 + 8;
    static constexpr int b1 = b0 + 8;
    static constexpr int b2 = b1 + 8;
    static constexpr int gx = b2 + 1;            // (backward: the sums of d rx and d ry ride in the row's last block)
    static constexpr int gy = b2 + 2;
    static constexpr int PS = b2 + 4;            // 172 / 236
    static constexpr int Groups = (PS + 63) / 64;
};

struct DmGeom {
    int N, C, H, W, Q, R, rel, F, tx, ty, P;
};

__device__ __forceinline__ float dm_ld(const float *p) { return *p; }
__device__ __forceinline__ float dm_ld(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ uint16_t dm_bf16(float v)      // round to nearest even
{
    const unsigned u = __float_as_uint(v);
    return (v != v) ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ void dm_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void dm_st(uint16_t *p, float v) { *p = dm_bf16(v); }
__device__ __forceinline__ void dm_st2(float *p, float a, float b) { *reinterpret_cast<float2 *>(p) = make_float2(a, b); }
__device__ __forceinline__ void dm_st2(uint16_t *p, float a, float b)
{
    *reinterpret_cast<unsigned *>(p) = (unsigned)dm_bf16(a) | ((unsigned)dm_bf16(b) << 16);
}

// where element k of a parameter row (the reference's order) lives in DmLay
template <int C>
__device__ __forceinline__ int dm_slot(int k, int rel)
{
    const int cin = rel ? C + 2 : C;
    if (k >= 8 * cin) return DmLay<C>::W1 + (k - 8 * cin);      // W1, w2, b0, b1, b2 follow one another in both orders
    const int r = k / cin, c = k - r * cin;
    if (!rel) return DmLay<C>::Wf + r * C + c;
    return c < 2 ? DmLay<C>::Wc + 2 * r + c : DmLay<C>::Wf + r * C + (c - 2);
}

template <int C, typename T>
__device__ __forceinline__ void dm_stage(const T *__restrict__ row, int P, int rel, float *__restrict__ dst, int tid)
{
    if (!rel && tid < 16) dst[DmLay<C>::Wc + tid] = 0.f;
    for (int k = tid; k < P; k += 256) dst[dm_slot<C>(k, rel)] = dm_ld(row + k);
}

// the chain on one pixel: p the staged parameters (wave-uniform reads)
template <int C>
__device__ __forceinline__ float dm_chain(const float *__restrict__ p, float rx, float ry, const float (&f)[C], float (&h0)[kDmHid],
                                          float (&h1)[kDmHid])
{
    using L = DmLay<C>;
#pragma unroll
    for (int i = 0; i < kDmHid; ++i) {
        float a = p[L::b0 + i];
        a = fmaf(p[L::Wc + 2 * i], rx, a);
        a = fmaf(p[L::Wc + 2 * i + 1], ry, a);
#pragma unroll
        for (int c = 0; c < C; ++c) a = fmaf(p[L::Wf + i * C + c], f[c], a);
        h0[i] = fmaxf(a, 0.f);
    }
#pragma unroll
    for (int j = 0; j < kDmHid; ++j) {
        float a = p[L::b1 + j];
#pragma unroll
        for (int i = 0; i < kDmHid; ++i) a = fmaf(p[L::W1 + 8 * j + i], h0[i], a);
        h1[j] = fmaxf(a, 0.f);
    }
    float t = p[L::b2];
#pragma unroll
    for (int j = 0; j < kDmHid; ++j) t = fmaf(p[L::w2 + j], h1[j], t);
    return t;
}

// rx, ry of a pixel: the product and the difference rounded one after the other, as the reference forms them
__device__ __forceinline__ void dm_rel(const float *__restrict__ ref, const float *__restrict__ sizes, int n, int q, int Q, int y, int x, int rel,
                                       float &rx, float &ry)
{
    rx = ry = 0.f;
    if (!rel) return;
    const float *r = ref + ((size_t)n * Q + q) * 2;
    rx = __fsub_rn(__fmul_rn(r[0], sizes[2 * n + 1]), (float)(8 * x + 4));
    ry = __fsub_rn(__fmul_rn(r[1], sizes[2 * n]), (float)(8 * y + 4));
}

__global__ __launch_bounds__(256) void dynmask_table_kernel(const int64_t *__restrict__ rows, const int64_t *__restrict__ offsets,
                                                            const int64_t *__restrict__ qot, int N, int R, int Q, int64_t cap,
                                                            int *__restrict__ inst)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= N * R) return;
    const int n = id / R, r = id - n * R;
    int found = -1;
    if (rows) {
        const int64_t q = rows[id];
        if (q >= 0 && q < Q) found = (int)q;
    } else if (offsets) {
        const int64_t live = min(offsets[N], cap);
        const int64_t s0 = max(offsets[n], (int64_t)0), s1 = min(offsets[n + 1], live);
        for (int64_t s = s0; s < s1; ++s)
            if (qot[s] == r) {
                found = r;
                break;
            }
    } else {
        found = r;
    }
    inst[id] = found;
}

template <int C, int F, typename T>
__global__ __launch_bounds__(256) void dynmask_fwd_kernel(const T *__restrict__ feat, const T *__restrict__ params, const float *__restrict__ ref,
                                                          const float *__restrict__ sizes, const int *__restrict__ inst, DmGeom g,
                                                          T *__restrict__ out)
{
    using L = DmLay<C>;
    constexpr int HALO = F == 2 ? 1 : 0;
    __shared__ __attribute__((aligned(16))) float prm[kDmBatch][L::PS];
    __shared__ float tile[kDmBatch][kDmTH][kDmTW + 1];
    __shared__ int qs[kDmBatch];
    const int tid = threadIdx.x, lx = tid & (kDmTW - 1), ly = tid / kDmTW;
    const int n = blockIdx.z, r0 = blockIdx.y * kDmRows;
    const int tyi = blockIdx.x / g.tx, txi = blockIdx.x - tyi * g.tx;
    // the lane's pixel; with a halo the first row and column of the tile are the neighbours' (clamped at the border: T[-1] = T[0])
    const int py = tyi * (kDmTH - HALO) + ly - HALO, px = txi * (kDmTW - HALO) + lx - HALO;
    const int y = min(max(py, 0), g.H - 1), x = min(max(px, 0), g.W - 1);
    const bool owns = ly >= HALO && lx >= HALO && py < g.H && px < g.W;
    float f[C];
    {
        const T *src = feat + (size_t)n * C * g.H * g.W + (size_t)y * g.W + x;
#pragma unroll
        for (int c = 0; c < C; ++c) f[c] = dm_ld(src + (size_t)c * g.H * g.W);
    }
    const int OW = F * g.W;
    const size_t plane = (size_t)F * g.H * OW;
    const int rend = min(r0 + kDmRows, g.R);
    for (int rb = r0; rb < rend; rb += kDmBatch) {
        const int nb = min(kDmBatch, rend - rb);
        __syncthreads();      // the previous batch's logits and parameters have been read
        if (tid < nb) {
            const int q = inst[(size_t)n * g.R + rb + tid];
            qs[tid] = (q >= 0 && q < g.Q) ? q : -1;
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b)
            if (qs[b] >= 0) dm_stage<C>(params + ((size_t)n * g.Q + qs[b]) * g.P, g.P, g.rel, prm[b], tid);
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const int q = qs[b];      // (the same for every lane)
            float t = 0.f;
            if (q >= 0) {
                float rx, ry, h0[kDmHid], h1[kDmHid];
                dm_rel(ref, sizes, n, q, g.Q, y, x, g.rel, rx, ry);
                t = dm_chain<C>(prm[b], rx, ry, f, h0, h1);
            }
            tile[b][ly][lx] = t;
        }
        __syncthreads();
        if (!owns) continue;
        for (int b = 0; b < nb; ++b) {
            T *o = out + ((size_t)n * g.R + rb + b) * plane;
            const float d = tile[b][ly][lx];
            if (F == 1) {
                dm_st(o + (size_t)py * OW + px, d);
            } else {
                const float a = tile[b][ly - 1][lx - 1], u = tile[b][ly - 1][lx], l = tile[b][ly][lx - 1];
                // torch's bilinear order: along x first, then along y; the halves are exact
                const float top = 0.5f * (0.5f * (a + u) + 0.5f * (l + d));
                T *o0 = o + (size_t)(2 * py) * OW + 2 * px;
                dm_st2(o0, top, 0.5f * (u + d));
                dm_st2(o0 + OW, 0.5f * (l + d), d);
            }
        }
    }
}

// the halving butterfly over 64 values: in the step over NN values the lanes with bit NN / 2 set keep the upper half and hand over the lower,
// the others the reverse, so every step halves what a lane holds; afterwards v[0] of lane l is the sum over the wave's lanes of value l.
// (A template per step: the indices must be constants for the values to stay in registers.)
template <int NN>
__device__ __forceinline__ void dm_halve(float (&v)[64], int lane)
{
    constexpr int HALF = NN / 2;
    const bool up = (lane & HALF) != 0;
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const float keep = up ? v[i + HALF] : v[i], send = up ? v[i] : v[i + HALF];
        v[i] = keep + __shfl_xor(send, HALF, 64);
    }
    if constexpr (HALF > 1) dm_halve<HALF>(v, lane);
}
__device__ __forceinline__ float dm_wave_transpose_sum(float (&v)[64], int lane)
{
    dm_halve<64>(v, lane);
    return v[0];
}

// value k of a row of parameter gradients (DmLay order) of one pixel
template <int C>
__device__ __forceinline__ float dm_gval(int k, float rx, float ry, const float (&f)[C], const float (&h0)[kDmHid], const float (&h1)[kDmHid],
                                         const float (&dz0)[kDmHid], const float (&dz1)[kDmHid], float dt, float drx, float dry)
{
    using L = DmLay<C>;
    if (k < L::Wf) return dz0[k >> 1] * ((k & 1) ? ry : rx);
    if (k < L::W1) return dz0[(k - L::Wf) / C] * f[(k - L::Wf) % C];
    if (k < L::w2) return dz1[(k - L::W1) >> 3] * h0[(k - L::W1) & 7];
    if (k < L::b0) return dt * h1[k - L::w2];
    if (k < L::b1) return dz0[k - L::b0];
    if (k < L::b2) return dz1[k - L::b1];
    if (k == L::b2) return dt;
    if (k == L::gx) return drx;
    if (k == L::gy) return dry;
    return 0.f;
}

template <int C, int F, typename T>
__global__ __launch_bounds__(256) void dynmask_bwd_kernel(const T *__restrict__ gout, const T *__restrict__ feat, const T *__restrict__ params,
                                                          const float *__restrict__ ref, const float *__restrict__ sizes,
                                                          const int *__restrict__ inst, DmGeom g, float *__restrict__ partial,
                                                          T *__restrict__ grad_feat)
{
    using L = DmLay<C>;
    __shared__ __attribute__((aligned(16))) float prm[L::PS];
    __shared__ float red[4][L::Groups * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lx = tid & (kDmTW - 1), ly = tid / kDmTW;
    const int n = blockIdx.y, tiles = g.tx * g.ty;
    const int tyi = blockIdx.x / g.tx, txi = blockIdx.x - tyi * g.tx;
    const int py = tyi * kDmTH + ly, px = txi * kDmTW + lx;
    const bool owns = py < g.H && px < g.W;
    const int y = min(py, g.H - 1), x = min(px, g.W - 1);
    float f[C], gf[C];
    {
        const T *src = feat + (size_t)n * C * g.H * g.W + (size_t)y * g.W + x;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            f[c] = dm_ld(src + (size_t)c * g.H * g.W);
            gf[c] = 0.f;
        }
    }
    const int OH = F * g.H, OW = F * g.W;
    const size_t plane = (size_t)OH * OW;
    for (int r = 0; r < g.R; ++r) {
        const int q = inst[(size_t)n * g.R + r];      // (the same for every lane)
        if (q < 0 || q >= g.Q) continue;
        __syncthreads();      // the previous row's parameters and wave sums have been read
        dm_stage<C>(params + ((size_t)n * g.Q + q) * g.P, g.P, g.rel, prm, tid);
        // the adjoint of the up-sampling: a gather
        float dt = 0.f;
        if (owns) {
            const T *go = gout + ((size_t)n * g.R + r) * plane;
            if (F == 1) {
                dt = dm_ld(go + (size_t)y * OW + x);
            } else {
                // taps 2 k (half; whole for k = 0), 2 k + 1 (whole), 2 k + 2 (half; absent past the end), rows then columns ascending
                const float wy[3] = {y ? 0.5f : 1.f, 1.f, 2 * y + 2 < OH ? 0.5f : 0.f};
                const float wx[3] = {x ? 0.5f : 1.f, 1.f, 2 * x + 2 < OW ? 0.5f : 0.f};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int oy = min(2 * y + a, OH - 1);
                    float rowsum = 0.f;
#pragma unroll
                    for (int b = 0; b < 3; ++b) rowsum += wx[b] * dm_ld(go + (size_t)oy * OW + min(2 * x + b, OW - 1));
                    dt += wy[a] * rowsum;
                }
            }
        }
        __syncthreads();
        float rx, ry, h0[kDmHid], h1[kDmHid], dz0[kDmHid], dz1[kDmHid];
        dm_rel(ref, sizes, n, q, g.Q, y, x, g.rel, rx, ry);
        dm_chain<C>(prm, rx, ry, f, h0, h1);
        // h > 0 exactly where the pre-activation is > 0
#pragma unroll
        for (int j = 0; j < kDmHid; ++j) dz1[j] = h1[j] > 0.f ? dt * prm[L::w2 + j] : 0.f;
#pragma unroll
        for (int i = 0; i < kDmHid; ++i) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < kDmHid; ++j) a = fmaf(prm[L::W1 + 8 * j + i], dz1[j], a);
            dz0[i] = h0[i] > 0.f ? a : 0.f;
        }
        float drx = 0.f, dry = 0.f;
#pragma unroll
        for (int i = 0; i < kDmHid; ++i) {
            drx = fmaf(prm[L::Wc + 2 * i], dz0[i], drx);
            dry = fmaf(prm[L::Wc + 2 * i + 1], dz0[i], dry);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < kDmHid; ++i) a = fmaf(prm[L::Wf + i * C + c], dz0[i], a);
            gf[c] += a;
        }
#pragma unroll
        for (int grp = 0; grp < L::Groups; ++grp) {
            float v[64];
#pragma unroll
            for (int k = 0; k < 64; ++k) v[k] = dm_gval<C>(grp * 64 + k, rx, ry, f, h0, h1, dz0, dz1, dt, drx, dry);
            red[wave][grp * 64 + lane] = dm_wave_transpose_sum(v, lane);
        }
        __syncthreads();
        if (tid < L::PS)
            partial[(((size_t)n * tiles + blockIdx.x) * g.R + r) * L::PS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
    if (owns) {
        T *dst = grad_feat + (size_t)n * C * g.H * g.W + (size_t)y * g.W + x;
#pragma unroll
        for (int c = 0; c < C; ++c) dm_st(dst + (size_t)c * g.H * g.W, gf[c]);
    }
}

template <int C, typename T>
__global__ __launch_bounds__(256) void dynmask_sum_kernel(const float *__restrict__ partial, const int *__restrict__ inst,
                                                          const float *__restrict__ sizes, DmGeom g, T *__restrict__ grad_params,
                                                          float *__restrict__ grad_ref)
{
    using L = DmLay<C>;
    const int tid = threadIdx.x, n = blockIdx.x / g.Q, q = blockIdx.x - n * g.Q, tiles = g.tx * g.ty;
    // thread k < P sums element k of the row; threads P and P + 1 the two coordinate sums
    const int slot = tid < g.P ? dm_slot<C>(tid, g.rel) : (tid == g.P ? L::gx : L::gy);
    if (tid >= g.P + 2) return;
    float acc = 0.f;
    for (int r = 0; r < g.R; ++r) {
        if (inst[(size_t)n * g.R + r] != q) continue;      // (the same for every lane)
        const float *p = partial + ((size_t)n * tiles * g.R + r) * L::PS + slot;
        for (int t = 0; t < tiles; ++t) acc += p[(size_t)t * g.R * L::PS];
    }
    if (tid < g.P) {
        dm_st(grad_params + ((size_t)n * g.Q + q) * g.P + tid, acc);
    } else if (grad_ref) {
        const int k = tid - g.P;      // d rx / d ref_x = size_w, d ry / d ref_y = size_h
        grad_ref[((size_t)n * g.Q + q) * 2 + k] = g.rel ? acc * sizes[2 * n + 1 - k] : 0.f;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct DmPlan {
    DmGeom g;
    int ftx, fty, chunks;      // the forward's tiles (the halo shortens them) and row chunks
    int64_t ws_bytes;
};

int dm_plan(int N, int C, int H, int W, int Q, int R, int rel_coord, int factor, DmPlan *p)
{
    if (N < 1 || H < 1 || W < 1 || Q < 1 || R < 1 || (rel_coord != 0 && rel_coord != 1)) return MSDA_ERR_BAD_DIMS;
    if ((C != 8 && C != 16) || (factor != 1 && factor != 2)) return MSDA_ERR_BAD_DIMS;      // (the template instances)
    if (N > 65535 || H > (1 << 14) || W > (1 << 14) || Q > (1 << 24) || R > (1 << 20)) return MSDA_ERR_TOO_LARGE;
    if ((int64_t)N * R * 4 * H * W >= (int64_t)1 << 40 || (int64_t)N * Q * 256 >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    DmGeom &g = p->g;
    g = DmGeom{N, C, H, W, Q, R, rel_coord, factor, (W + kDmTW - 1) / kDmTW, (H + kDmTH - 1) / kDmTH, 8 * (C + 2 * rel_coord) + 89};
    const int halo = factor == 2 ? 1 : 0;
    p->ftx = (W + kDmTW - halo - 1) / (kDmTW - halo);
    p->fty = (H + kDmTH - halo - 1) / (kDmTH - halo);
    p->chunks = (R + kDmRows - 1) / kDmRows;
    if ((int64_t)p->ftx * p->fty >= (int64_t)1 << 31 || p->chunks > 65535) return MSDA_ERR_TOO_LARGE;
    const int PS = C == 8 ? DmLay<8>::PS : DmLay<16>::PS;
    p->ws_bytes = ((int64_t)N * g.tx * g.ty * R * PS * (int64_t)sizeof(float) + 255) / 256 * 256;
    if (p->ws_bytes >= (int64_t)1 << 40) return MSDA_ERR_TOO_LARGE;
    return MSDA_OK;
}

template <int C, int F, typename T>
void dm_launch_fwd(const DmPlan &p, const T *feat, const T *params, const float *ref, const float *sizes, const int *inst, T *out, hipStream_t s)
{
    DmGeom g = p.g;
    g.tx = p.ftx;
    g.ty = p.fty;
    dynmask_fwd_kernel<C, F, T><<<dim3((unsigned)(p.ftx * p.fty), (unsigned)p.chunks, (unsigned)g.N), 256, 0, s>>>(feat, params, ref, sizes, inst, g,
                                                                                                                  out);
}

template <int C, int F, typename T>
void dm_launch_bwd(const DmPlan &p, const T *gout, const T *feat, const T *params, const float *ref, const float *sizes, const int *inst,
                   float *partial, T *grad_params, T *grad_feat, float *grad_ref, hipStream_t s)
{
    const DmGeom &g = p.g;
    dynmask_bwd_kernel<C, F, T><<<dim3((unsigned)(g.tx * g.ty), (unsigned)g.N), 256, 0, s>>>(gout, feat, params, ref, sizes, inst, g, partial,
                                                                                            grad_feat);
    dynmask_sum_kernel<C, T><<<(unsigned)(g.N * g.Q), 256, 0, s>>>(partial, inst, sizes, g, grad_params, grad_ref);
}

template <typename T>
int dm_forward(const char *fn, const T *feat, const T *params, const float *ref, const float *sizes, const int *inst, int N, int C, int H, int W,
               int Q, int R, int rel_coord, int factor, T *out, msda_stream_t stream)
{
    DmPlan p;
    if (!feat || !params || !inst || !out || (rel_coord && (!ref || !sizes))) return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
    if (const int e = dm_plan(N, C, H, W, Q, R, rel_coord, factor, &p)) return msda::arg_fail(e, fn);
    if (!msda::aligned(4, {ref, sizes, inst}) || !msda::aligned(sizeof(T), {feat, params}) || !msda::aligned(factor * sizeof(T), {out}))      // (the x2 map is stored two elements at a time)
        return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    hipStream_t s = (hipStream_t)stream;
    if (C == 8 && factor == 2) dm_launch_fwd<8, 2, T>(p, feat, params, ref, sizes, inst, out, s);
    if (C == 8 && factor == 1) dm_launch_fwd<8, 1, T>(p, feat, params, ref, sizes, inst, out, s);
    if (C == 16 && factor == 2) dm_launch_fwd<16, 2, T>(p, feat, params, ref, sizes, inst, out, s);
    if (C == 16 && factor == 1) dm_launch_fwd<16, 1, T>(p, feat, params, ref, sizes, inst, out, s);
    return msda::launched(fn);
}

template <typename T>
int dm_backward(const char *fn, const T *gout, const T *feat, const T *params, const float *ref, const float *sizes, const int *inst, int N, int C,
                int H, int W, int Q, int R, int rel_coord, int factor, T *grad_params, T *grad_feat, float *grad_ref, void *workspace,
                msda_stream_t stream)
{
    DmPlan p;
    if (!gout || !feat || !params || !inst || !grad_params || !grad_feat || !workspace || (rel_coord && (!ref || !sizes)))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
    if (const int e = dm_plan(N, C, H, W, Q, R, rel_coord, factor, &p)) return msda::arg_fail(e, fn);
    if (!msda::aligned(16, {workspace}) || !msda::aligned(4, {ref, sizes, inst, grad_ref}) ||
        !msda::aligned(sizeof(T), {gout, feat, params, grad_params, grad_feat}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    hipStream_t s = (hipStream_t)stream;
    float *partial = static_cast<float *>(workspace);
    if (C == 8 && factor == 2) dm_launch_bwd<8, 2, T>(p, gout, feat, params, ref, sizes, inst, partial, grad_params, grad_feat, grad_ref, s);
    if (C == 8 && factor == 1) dm_launch_bwd<8, 1, T>(p, gout, feat, params, ref, sizes, inst, partial, grad_params, grad_feat, grad_ref, s);
    if (C == 16 && factor == 2) dm_launch_bwd<16, 2, T>(p, gout, feat, params, ref, sizes, inst, partial, grad_params, grad_feat, grad_ref, s);
    if (C == 16 && factor == 1) dm_launch_bwd<16, 1, T>(p, gout, feat, params, ref, sizes, inst, partial, grad_params, grad_feat, grad_ref, s);
    return msda::launched(fn);
}

}  // namespace

extern "C" {

int msda_dynmask_workspace_bytes(int N, int C, int H, int W, int Q, int R, int64_t *bytes)
{
    DmPlan p;
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = dm_plan(N, C, H, W, Q, R, 1, 2, &p)) return msda::arg_fail(e, __func__);
    *bytes = p.ws_bytes;
    return MSDA_OK;
}

int msda_dynmask_table(const int64_t *rows, const int64_t *offsets, const int64_t *query_of_target, int N, int R, int Q, int64_t cap, int *inst,
                       msda_stream_t stream)
{
    if (!inst || (!rows && (offsets != nullptr) != (query_of_target != nullptr))) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (N < 1 || R < 1 || Q < 1 || (!rows && R != Q) || (offsets && cap < 1)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if ((int64_t)N * R >= (int64_t)1 << 31) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (!msda::aligned(8, {rows, offsets, query_of_target}) || !msda::aligned(4, {inst})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    dynmask_table_kernel<<<(unsigned)((N * R + 255) / 256), 256, 0, (hipStream_t)stream>>>(rows, rows ? nullptr : offsets, query_of_target, N, R, Q,
                                                                                         cap, inst);
    return msda::launched(__func__);
}

int msda_dynmask_forward_f32(const float *feat, const float *params, const float *ref, const float *sizes, const int *inst, int N, int C, int H,
                             int W, int Q, int R, int rel_coord, int factor, float *out, msda_stream_t stream)
{
    return dm_forward(__func__, feat, params, ref, sizes, inst, N, C, H, W, Q, R, rel_coord, factor, out, stream);
}

int msda_dynmask_forward_bf16(const uint16_t *feat, const uint16_t *params, const float *ref, const float *sizes, const int *inst, int N, int C,
                              int H, int W, int Q, int R, int rel_coord, int factor, uint16_t *out, msda_stream_t stream)
{
    return dm_forward(__func__, feat, params, ref, sizes, inst, N, C, H, W, Q, R, rel_coord, factor, out, stream);
}

int msda_dynmask_backward_f32(const float *grad_out, const float *feat, const float *params, const float *ref, const float *sizes, const int *inst,
                              int N, int C, int H, int W, int Q, int R, int rel_coord, int factor, float *grad_params, float *grad_feat,
                              float *grad_ref, void *workspace, msda_stream_t stream)
{
    return dm_backward(__func__, grad_out, feat, params, ref, sizes, inst, N, C, H, W, Q, R, rel_coord, factor, grad_params, grad_feat, grad_ref,
                       workspace, stream);
}

int msda_dynmask_backward_bf16(const uint16_t *grad_out, const uint16_t *feat, const uint16_t *params, const float *ref, const float *sizes,
                               const int *inst, int N, int C, int H, int W, int Q, int R, int rel_coord, int factor, uint16_t *grad_params,
                               uint16_t *grad_feat, float *grad_ref, void *workspace, msda_stream_t stream)
{
    return dm_backward(__func__, grad_out, feat, params, ref, sizes, inst, N, C, H, W, Q, R, rel_coord, factor, grad_params, grad_feat, grad_ref,
                       workspace, stream);
}

}  // extern "C"
