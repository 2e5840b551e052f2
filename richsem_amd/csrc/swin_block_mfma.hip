// swin_block_mfma.hip -- what a Swin block does outside its window attention, on library kernels ("Swin block"):
// a linear layer of general width with four fused epilogues, and a LayerNorm of general width, forward and backward.
//
// Reference: models/richsem/swin_transformer.py:27-44 (Mlp: fc1, GELU, fc2), :108-139 (qkv, proj) and :183-239 (norm1, norm2 and the two
// residual adds of SwinTransformerBlock.forward).  Storage is bf16, accumulation and all element-wise arithmetic fp32, every stored element
// is rounded once, at its store (round to nearest even).  No atomics, no allocation, no synchronisation: the same bits on every call.
//
// Linear:  acc = x (tokens, K) . w (N, K)^T with mfma_f32_16x16x32_bf16, K and N multiples of 32.  Both operands are read in their natural
// row-major order (w needs no packed form; the input gradient is the same entry point on w^T).
//   The cut: a workgroup of four waves owns 128 tokens x BN output channels (BN = 128, or 64 where that fills the chip better: the grid
//   is cut along N as well as along the tokens), walks K in blocks of 64 and keeps the two operand blocks in LDS (32 KB at BN = 128); the
//   next block is fetched into registers under the current block's products and parked between two barriers.  Rows are 128 bytes in
//   LDS with their 16-byte slots XOR-swizzled by the row, so a fragment read -- lane (c, q): row c, bytes 16 q .. 16 q + 15 of a 32-wide
//   k step -- is free of bank conflicts.  Rows past `tokens` / `N` are clamped (their results are never stored), columns past K are zeros.
//   The product is taken transposed (A = w rows, B = x rows): a token on the lane, channels in the registers.  A wave owns 64 tokens x
//   BN / 2 channels; inside every 32-channel block the rows of the two A tiles are permuted (row 4 g + i of tile u = channel 8 g + 4 u + i)
//   so that lane (c, g) ends with eight CONSECUTIVE channels of token c: 16-byte loads of aux and 16-byte stores.
//   Epilogues: 0 bias, 1 GELU (u = rnd(acc + bias) to out2, out = rnd(gelu(u)) of the ROUNDED u), 2 residual (+ aux), 3 GELU backward
//   (out = rnd(acc gelu'(aux)), out2 = rnd(gelu(aux))).  GELU is the exact form x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2 (erfc keeps the
//   relative accuracy in the negative tail that 1 + erf loses).  K is never split across workgroups.
//
// LayerNorm forward: one wave per token; the row (C <= 4096: at most 8 x 16 bytes per lane) is read once into registers; mean, then
// the biased variance as the mean of squared deviations (two passes over registers, fp32), 64-lane butterfly sums.
// LayerNorm backward: dx by the same cut (xhat recomputed from x, mean, rstd; the residual stream's gradient `add` fused so that the sum
// is rounded once).  dgamma / dbeta: a second kernel sums 64-token parts per 128-channel group (a lane owns two channels, a wave every
// fourth row, the four waves are added in wave order) into the workspace, a third adds the parts in ascending order.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"
#include "swin_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBM = 128;            // tokens of a workgroup's tile
constexpr int kBK = 64;             // K block
constexpr int kLd = kBK;            // LDS row stride in shorts (128 bytes: two rows per 256-byte bank row)
constexpr int kMaxWidth = 8192;     // linear: K and N

constexpr float kRsqrt2 = 0.70710678118654752f;
constexpr float kRsqrt2Pi = 0.39894228040143268f;

__device__ __forceinline__ float norm_cdf(float x) { return 0.5f * erfcf(-x * kRsqrt2); }
__device__ __forceinline__ float gelu(float x) { return x * norm_cdf(x); }
__device__ __forceinline__ float gelu_grad(float x) { return norm_cdf(x) + x * (kRsqrt2Pi * __expf(-0.5f * x * x)); }
__device__ __forceinline__ float round_bf16(float v) { return bf16_lo(pack_bf16(v, 0.f)); }

// ---- linear ----------------------------------------------------------------------------------------------------------------------------
// The 16-byte slot `ks` (0..7) of LDS row `row` lives at slot ks ^ swizzle(row).  ds_read_b128 serves lanes {0-3, 12-15, 20-27} (and the
// three like groups) together; a fragment read has lane (c, g) on row base + c (x) or base + 8 (c / 4) + c % 4 (w, base a multiple of 4)
// and slot 4 s + g: with bits 1..3 of the row, and bit 4 moved to bit 1, XORed in, the sixteen lanes of every group hit sixteen different
// slots of the 256-byte bank row (unswizzled, or with 16 bytes of row padding, every group is two-way conflicted).
__device__ __forceinline__ int swizzle(int row) { return ((row >> 1) & 7) ^ (((row >> 4) & 1) << 1); }
__device__ __forceinline__ int lds_at(int row, int ks) { return row * kLd + 8 * (ks ^ swizzle(row)); }

// one K block of `ROWS` rows of a row-major (rows, K) operand: CH 16-byte chunks per thread; rows past the end clamp, columns past K are zero
template <int ROWS>
struct BlockStager {
    static constexpr int CH = ROWS * (kBK / 8) / kThreads;
    u32x4 reg[CH];
    __device__ __forceinline__ void fetch(const uint16_t *__restrict__ src, int row0, int rows, int K, int k0, int tid)
    {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + i * kThreads, r = e >> 3, k = k0 + 8 * (e & 7);
            reg[i] = (u32x4){0u, 0u, 0u, 0u};
            if (k < K) reg[i] = *reinterpret_cast<const u32x4 *>(src + (size_t)min(row0 + r, rows - 1) * K + k);
        }
    }
    __device__ __forceinline__ void park(short *slot, int tid) const
    {
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int e = tid + i * kThreads;
            *reinterpret_cast<u32x4 *>(slot + lds_at(e >> 3, e & 7)) = reg[i];
        }
    }
};

template <int BN, int EPI>
__global__ __launch_bounds__(kThreads) void swin_linear_kernel(const uint16_t *__restrict__ x, const uint16_t *__restrict__ w,
                                                               const float *__restrict__ bias, const uint16_t *__restrict__ aux, int tokens,
                                                               int K, int N, uint16_t *__restrict__ out, uint16_t *__restrict__ out2)
{
    constexpr int NT = BN / 32;      // 16-channel tiles of a wave (BN / 2 channels)
    __shared__ __attribute__((aligned(16))) short xs[kBM * kLd];
    __shared__ __attribute__((aligned(16))) short ws[BN * kLd];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int tok0 = blockIdx.x * kBM, n0 = blockIdx.y * BN;

    BlockStager<kBM> sx;
    BlockStager<BN> sw;
    sx.fetch(x, tok0, tokens, K, 0, tid);
    sw.fetch(w, n0, N, K, 0, tid);
    sx.park(xs, tid);
    sw.park(ws, tid);
    __syncthreads();

    f32x4 acc[4][NT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // A rows of this lane: tile u of the wave covers channels 32 (u / 2) .. + 31 of its half; row c <-> channel 8 (c / 4) + 4 (u % 2) + c % 4
    const int a_row = wn * (BN / 2) + 8 * (c >> 2) + (c & 3);
    const int nblk = (K + kBK - 1) / kBK;
    int xoff[kBK / 32][4], woff[kBK / 32][NT];
#pragma unroll
    for (int s = 0; s < kBK / 32; ++s) {
#pragma unroll
        for (int t = 0; t < 4; ++t) xoff[s][t] = lds_at(wm * 64 + 16 * t + c, 4 * s + g);
#pragma unroll
        for (int u = 0; u < NT; ++u) woff[s][u] = lds_at(a_row + 32 * (u >> 1) + 4 * (u & 1), 4 * s + g);
    }
    for (int b = 0; b < nblk; ++b) {
        if (b + 1 < nblk) {      // the next block's loads fly under this block's products
            sx.fetch(x, tok0, tokens, K, (b + 1) * kBK, tid);
            sw.fetch(w, n0, N, K, (b + 1) * kBK, tid);
        }
#pragma unroll
        for (int s = 0; s < kBK / 32; ++s) {
            bf16x8 xf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) xf[t] = *reinterpret_cast<const bf16x8 *>(xs + xoff[s][t]);
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(ws + woff[s][u]);
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf[t], acc[t][u], 0, 0, 0);
            }
        }
        if (b + 1 < nblk) {
            __syncthreads();      // every wave has read block b
            sx.park(xs, tid);
            sw.park(ws, tid);
            __syncthreads();
        }
    }

    // lane (c, g): token tok0 + 64 wm + 16 t + c, channels n0 + wn BN / 2 + 32 p + 8 g + 0..7 (acc[t][2 p + u][i] = channel .. + 4 u + i)
#pragma unroll
    for (int p = 0; p < NT / 2; ++p) {
        const int ch = n0 + wn * (BN / 2) + 32 * p + 8 * g;
        if (ch >= N) continue;
        float bb[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) bb[i] = (EPI != 3 && bias) ? bias[ch + i] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int tok = tok0 + wm * 64 + 16 * t + c;
            if (tok >= tokens) continue;
            const size_t at = (size_t)tok * N + ch;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = acc[t][2 * p + (i >> 2)][i & 3] + bb[i];
            if (EPI == 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = round_bf16(v[i]);
                if (out2) *reinterpret_cast<u32x4 *>(out2 + at) = pack8(v);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = gelu(v[i]);
            } else if (EPI == 2) {
                float a[8];
                unpack8(*reinterpret_cast<const u32x4 *>(aux + at), a);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] += a[i];
            } else if (EPI == 3) {
                float a[8];
                unpack8(*reinterpret_cast<const u32x4 *>(aux + at), a);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] *= gelu_grad(a[i]);
                if (out2) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) a[i] = gelu(a[i]);
                    *reinterpret_cast<u32x4 *>(out2 + at) = pack8(a);
                }
            }
            *reinterpret_cast<u32x4 *>(out + at) = pack8(v);
        }
    }
}

template <int BN>
void launch_linear(int epilogue, dim3 grid, hipStream_t stream, const uint16_t *x, const uint16_t *w, const float *bias, const uint16_t *aux,
                   int tokens, int K, int N, uint16_t *out, uint16_t *out2)
{
    switch (epilogue) {
    case 0: swin_linear_kernel<BN, 0><<<grid, kThreads, 0, stream>>>(x, w, bias, aux, tokens, K, N, out, out2); break;
    case 1: swin_linear_kernel<BN, 1><<<grid, kThreads, 0, stream>>>(x, w, bias, aux, tokens, K, N, out, out2); break;
    case 2: swin_linear_kernel<BN, 2><<<grid, kThreads, 0, stream>>>(x, w, bias, aux, tokens, K, N, out, out2); break;
    default: swin_linear_kernel<BN, 3><<<grid, kThreads, 0, stream>>>(x, w, bias, aux, tokens, K, N, out, out2); break;
    }
}

// ---- LayerNorm (limits, unpack8 / pack8, wave_sum and the last stage of dgamma / dbeta: swin_rows.h) ---------------------------------------
__global__ __launch_bounds__(kLnRows * 64) void swin_ln_fwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta, float eps, int tokens, int C,
                                                                   uint16_t *__restrict__ out, float *__restrict__ mean, float *__restrict__ rstd)
{
    const int lane = threadIdx.x & 63, tok = blockIdx.x * kLnRows + (threadIdx.x >> 6), nch = C >> 3;
    if (tok >= tokens) return;
    const uint16_t *row = x + (size_t)tok * C;
    float v[kLnChunks][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            unpack8(*reinterpret_cast<const u32x4 *>(row + 8 * ch), v[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        }
    }
    const float fc = (float)C, mu = wave_sum(s) / fc;      // (a division: a constant row's mean is the constant, exactly)
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q += (v[i][j] - mu) * (v[i][j] - mu);
        }
    const float rs = 1.f / sqrtf(wave_sum(q) / fc + eps);
    if (lane == 0) {
        if (mean) mean[tok] = mu;
        if (rstd) rstd[tok] = rs;
    }
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mu) * rs * gamma[8 * ch + j] + beta[8 * ch + j];
            *reinterpret_cast<u32x4 *>(out + (size_t)tok * C + 8 * ch) = pack8(o);
        }
    }
}

__global__ __launch_bounds__(kLnRows * 64) void swin_ln_bwd_rows_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                        const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                        const float *__restrict__ gamma, const uint16_t *__restrict__ add,
                                                                        int tokens, int C, uint16_t *__restrict__ dx)
{
    const int lane = threadIdx.x & 63, tok = blockIdx.x * kLnRows + (threadIdx.x >> 6), nch = C >> 3;
    if (tok >= tokens) return;
    const size_t base = (size_t)tok * C;
    const float mu = mean[tok], rs = rstd[tok];
    float gv[kLnChunks][8], xh[kLnChunks][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            unpack8(*reinterpret_cast<const u32x4 *>(dy + base + 8 * ch), gv[i]);
            unpack8(*reinterpret_cast<const u32x4 *>(x + base + 8 * ch), xh[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gv[i][j] *= gamma[8 * ch + j];
                xh[i][j] = (xh[i][j] - mu) * rs;
                s1 += gv[i][j];
                s2 += gv[i][j] * xh[i][j];
            }
        }
    }
    const float fc = (float)C, m1 = wave_sum(s1) / fc, m2 = wave_sum(s2) / fc;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = rs * (gv[i][j] - m1 - xh[i][j] * m2);
            if (add) {
                float a[8];
                unpack8(*reinterpret_cast<const u32x4 *>(add + base + 8 * ch), a);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] += a[j];
            }
            *reinterpret_cast<u32x4 *>(dx + base + 8 * ch) = pack8(o);
        }
    }
}

// part p = blockIdx.x (tokens 64 p .. 64 p + 63) of channels 128 blockIdx.y + 2 lane + {0, 1}: workspace[(2 p + {0 dgamma, 1 dbeta}) C + channel]
__global__ __launch_bounds__(256) void swin_ln_bwd_cols_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                               const float *__restrict__ mean, const float *__restrict__ rstd, int tokens, int C,
                                                               float *__restrict__ workspace)
{
    __shared__ float part[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = blockIdx.y * kColGroup + 2 * lane;
    const int t0 = blockIdx.x * kPartRows, t1 = min(t0 + kPartRows, tokens);
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    if (ch < C)
        for (int t = t0 + wave; t < t1; t += 4) {
            const size_t at = (size_t)t * C + ch;
            const unsigned d = *reinterpret_cast<const unsigned *>(dy + at), xv = *reinterpret_cast<const unsigned *>(x + at);
            const float mu = mean[t], rs = rstd[t];
            dg0 += bf16_lo(d) * ((bf16_lo(xv) - mu) * rs);
            dg1 += bf16_hi(d) * ((bf16_hi(xv) - mu) * rs);
            db0 += bf16_lo(d);
            db1 += bf16_hi(d);
        }
    part[wave][0][lane] = dg0;
    part[wave][1][lane] = dg1;
    part[wave][2][lane] = db0;
    part[wave][3][lane] = db1;
    __syncthreads();
    if (wave == 0 && ch < C) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = ((part[0][k][lane] + part[1][k][lane]) + part[2][k][lane]) + part[3][k][lane];
        float *dst = workspace + (size_t)blockIdx.x * 2 * C + ch;
        dst[0] = r[0];
        dst[1] = r[1];
        dst[C] = r[2];
        dst[C + 1] = r[3];
    }
}

}  // namespace

extern "C" {

int msda_swin_linear_bf16(const uint16_t *x, const uint16_t *w, const float *bias, const uint16_t *aux, int epilogue, int tokens, int K, int N,
                          uint16_t *out, uint16_t *out2, msda_stream_t stream)
{
    if (!x || !w || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (epilogue < 0 || epilogue > 3 || tokens < 1 || K < 32 || N < 32 || K > kMaxWidth || N > kMaxWidth || K % 32 || N % 32)
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (epilogue >= 2 && !aux) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if ((int64_t)tokens * K >= (int64_t)1 << 31 || (int64_t)tokens * N >= (int64_t)1 << 31) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (!msda::aligned(16, {x, w, aux, out, out2}) || !msda::aligned(4, {bias})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int gx = (tokens + kBM - 1) / kBM;
    hipStream_t s = (hipStream_t)stream;
    // 128-wide tiles (a third fewer LDS reads per product) where they still give half the CUs of a 256-CU chip a workgroup, else 64-wide ones
    if (N % 128 == 0 && (int64_t)gx * (N / 128) >= 128)
        launch_linear<128>(epilogue, dim3(gx, N / 128), s, x, w, bias, aux, tokens, K, N, out, out2);
    else
        launch_linear<64>(epilogue, dim3(gx, (N + 63) / 64), s, x, w, bias, aux, tokens, K, N, out, out2);
    return msda::launched(__func__);
}

int msda_swin_layernorm_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int tokens, int C, uint16_t *out,
                                     float *mean, float *rstd, msda_stream_t stream)
{
    if (!x || !gamma || !beta || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, out}) || !msda::aligned(4, {gamma, beta, mean, rstd})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    swin_ln_fwd_kernel<<<(tokens + kLnRows - 1) / kLnRows, kLnRows * 64, 0, (hipStream_t)stream>>>(x, gamma, beta, eps, tokens, C, out, mean, rstd);
    return msda::launched(__func__);
}

int msda_swin_layernorm_workspace_bytes(int tokens, int C, int64_t *bytes)
{
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    *bytes = (int64_t)((tokens + kPartRows - 1) / kPartRows) * 2 * C * (int64_t)sizeof(float);
    return MSDA_OK;
}

int msda_swin_layernorm_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma,
                                      const uint16_t *add, int tokens, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace,
                                      msda_stream_t stream)
{
    if (!dy || !x || !mean || !rstd || !gamma || !dx || ((dgamma || dbeta) && !workspace)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {dy, x, add, dx}) || !msda::aligned(4, {mean, rstd, gamma, dgamma, dbeta, workspace}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    swin_ln_bwd_rows_kernel<<<(tokens + kLnRows - 1) / kLnRows, kLnRows * 64, 0, s>>>(dy, x, mean, rstd, gamma, add, tokens, C, dx);
    if (dgamma || dbeta) {
        const int parts = (tokens + kPartRows - 1) / kPartRows;
        float *ws = static_cast<float *>(workspace);
        swin_ln_bwd_cols_kernel<<<dim3(parts, (C + kColGroup - 1) / kColGroup), 256, 0, s>>>(dy, x, mean, rstd, tokens, C, ws);
        swin_ln_bwd_sum_kernel<<<dim3((C + 255) / 256, 2), 256, 0, s>>>(ws, parts, C, dgamma, dbeta);
    }
    return msda::launched(__func__);
}

}  // extern "C"
