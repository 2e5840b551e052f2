// swin_stage.hip -- where the Swin backbone changes layout, on library kernels ("Swin stage boundaries"): the norm of
// PatchMerging on rows gathered from the map, the output norms stored as NCHW, and the patch embedding's image <-> rows movement.
//
// Reference: models/richsem/swin_transformer.py:242-277 (PatchMerging), :399-434 (PatchEmbed) and :640-660 (the output norms of
// SwinTransformer.forward).  Storage is bf16, statistics and all arithmetic fp32, every stored element is rounded once, at its store.  The
// formulas are those of swin_ln_fwd_kernel / swin_ln_bwd_*_kernel (csrc/swin_block_mfma.hip), operation for operation: the mean by a
// division, the biased variance as the mean of squared deviations, dgamma / dbeta as 64-row parts (a wave every fourth row, the four waves
// added in wave order) through the workspace, the parts added in ascending order.  Only where a row's elements live changes.  No atomics,
// no allocation, no synchronisation: the same bits on every call.
//
// Merging norm: row (b, i, j) of (B H2 W2, 4 C), channel q C + c = pixel (2 i + (q & 1), 2 j + (q >> 1)) of the map (B, H, W, C); a pixel
//   outside the map is a zero that takes part in the statistics.  One wave per row, the row in registers; C is a multiple of 32, so a
//   16-byte chunk never straddles two quadrants.  The backward stores dx at the pixel a chunk came from (every pixel belongs to exactly one
//   (row, quadrant): plain stores, nothing pre-zeroed) and drops the chunks outside.
// Output norm to NCHW: a workgroup of four waves takes TT consecutive tokens of one image (TT = the largest of 64, 32, ... 4 with
//   TT (C + 8) bf16 elements inside 64 KB of LDS), a wave per token forms the statistics and parks the normalised, rounded row in LDS;
//   then channel c's run of tokens is stored in the 16-byte chunks OF THE BUFFER it touches -- a chunk that lies wholly inside the run with
//   one 16-byte store, the ragged ones at either end element by element: HW is arbitrary, a channel row may start on any 2-byte boundary.
//   The backward reads dy's runs into the same tile by the same chunks (16-byte loads inside, 2-byte loads at the ends) and then is the
//   row kernel; its column kernel transposes a (64 tokens x 128 channels) block of dy through LDS and then is the column kernel.
// Patch rows: rows (B Wh Ww, Kp), column (c ph + dy) pw + dx = image (b, c, i ph + dy, j pw + dx); zeros past the image and past Cin ph pw.
//   Pure data movement; the backward is the inverse (patches do not overlap: plain stores).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"
#include "swin_rows.h"

namespace {

constexpr int kTileShorts = 32768;      // the NCHW norm's tile: 64 KB of static LDS at most
constexpr int kTilePad = 8;             // bf16 elements between the tile's rows: 16-byte aligned rows
constexpr int kMaxKp = 8192;            // patch rows
constexpr int kColLd = kColGroup + 2;   // row stride of the transposed dy block (65 dwords: consecutive tokens on consecutive banks)

// ---- merging norm ----------------------------------------------------------------------------------------------------------------------
struct MergeRow {
    int b, i, j;
};
__device__ __forceinline__ MergeRow merge_row(int row, int H2, int W2)
{
    const int bi = row / W2;
    return {bi / H2, bi % H2, row - bi * W2};
}
// element offset in the map of channels k0 .. (k0 < 4 C, k0 and the run inside one quadrant) of row r, or -1 for a pixel outside the map
__device__ __forceinline__ int64_t merge_at(MergeRow r, int k0, int H, int W, int C)
{
    const int q = k0 / C, y = 2 * r.i + (q & 1), x = 2 * r.j + (q >> 1);
    if (y >= H || x >= W) return -1;
    return ((int64_t)(r.b * H + y) * W + x) * C + (k0 - q * C);
}

__global__ __launch_bounds__(kLnRows * 64) void merge_norm_fwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ gamma,
                                                                      const float *__restrict__ beta, float eps, int rows, int H, int W, int C,
                                                                      uint16_t *__restrict__ out, float *__restrict__ mean, float *__restrict__ rstd)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * kLnRows + (threadIdx.x >> 6), C4 = 4 * C, nch = C4 >> 3;
    if (row >= rows) return;
    const MergeRow r = merge_row(row, (H + 1) >> 1, (W + 1) >> 1);
    float v[kLnChunks][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const int64_t at = merge_at(r, 8 * ch, H, W, C);
            u32x4 u = (u32x4){0u, 0u, 0u, 0u};
            if (at >= 0) u = *reinterpret_cast<const u32x4 *>(x + at);
            unpack8(u, v[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += v[i][j];
        }
    }
    const float fc = (float)C4, mu = wave_sum(s) / fc;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i)
        if (lane + 64 * i < nch) {
#pragma unroll
            for (int j = 0; j < 8; ++j) q += (v[i][j] - mu) * (v[i][j] - mu);
        }
    const float rs = 1.f / sqrtf(wave_sum(q) / fc + eps);
    if (lane == 0) {
        if (mean) mean[row] = mu;
        if (rstd) rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mu) * rs * gamma[8 * ch + j] + beta[8 * ch + j];
            *reinterpret_cast<u32x4 *>(out + (size_t)row * C4 + 8 * ch) = pack8(o);
        }
    }
}

__global__ __launch_bounds__(kLnRows * 64) void merge_norm_bwd_rows_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                           const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                           const float *__restrict__ gamma, int rows, int H, int W, int C,
                                                                           uint16_t *__restrict__ dx)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * kLnRows + (threadIdx.x >> 6), C4 = 4 * C, nch = C4 >> 3;
    if (row >= rows) return;
    const MergeRow r = merge_row(row, (H + 1) >> 1, (W + 1) >> 1);
    const size_t base = (size_t)row * C4;
    const float mu = mean[row], rs = rstd[row];
    float gv[kLnChunks][8], xh[kLnChunks][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const int64_t at = merge_at(r, 8 * ch, H, W, C);
            u32x4 u = (u32x4){0u, 0u, 0u, 0u};
            if (at >= 0) u = *reinterpret_cast<const u32x4 *>(x + at);
            unpack8(*reinterpret_cast<const u32x4 *>(dy + base + 8 * ch), gv[i]);
            unpack8(u, xh[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gv[i][j] *= gamma[8 * ch + j];
                xh[i][j] = (xh[i][j] - mu) * rs;
                s1 += gv[i][j];
                s2 += gv[i][j] * xh[i][j];
            }
        }
    }
    const float fc = (float)C4, m1 = wave_sum(s1) / fc, m2 = wave_sum(s2) / fc;
#pragma unroll
    for (int i = 0; i < kLnChunks; ++i) {
        const int ch = lane + 64 * i;
        if (ch < nch) {
            const int64_t at = merge_at(r, 8 * ch, H, W, C);
            if (at < 0) continue;      // a padded quadrant has no pixel: its gradient is dropped
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = rs * (gv[i][j] - m1 - xh[i][j] * m2);
            *reinterpret_cast<u32x4 *>(dx + at) = pack8(o);
        }
    }
}

// part p = blockIdx.x (rows 64 p .. 64 p + 63) of channels 128 blockIdx.y + 2 lane + {0, 1} of the 4 C: workspace[(2 p + {0, 1}) 4 C + channel]
__global__ __launch_bounds__(256) void merge_norm_bwd_cols_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                  const float *__restrict__ mean, const float *__restrict__ rstd, int rows, int H,
                                                                  int W, int C, float *__restrict__ workspace)
{
    __shared__ float part[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = blockIdx.y * kColGroup + 2 * lane, C4 = 4 * C;
    const int t0 = blockIdx.x * kPartRows, t1 = min(t0 + kPartRows, rows), H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    if (ch < C4)
        for (int t = t0 + wave; t < t1; t += 4) {
            const int64_t at = merge_at(merge_row(t, H2, W2), ch, H, W, C);
            const unsigned d = *reinterpret_cast<const unsigned *>(dy + (size_t)t * C4 + ch);
            const unsigned xv = at >= 0 ? *reinterpret_cast<const unsigned *>(x + at) : 0u;      // (a padded zero's xhat is -mean rstd: it counts)
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
    if (wave == 0 && ch < C4) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = ((part[0][k][lane] + part[1][k][lane]) + part[2][k][lane]) + part[3][k][lane];
        float *dst = workspace + (size_t)blockIdx.x * 2 * C4 + ch;
        dst[0] = r[0];
        dst[1] = r[1];
        dst[C4] = r[2];
        dst[C4 + 1] = r[3];
    }
}

// ---- output norm to NCHW ---------------------------------------------------------------------------------------------------------------
// tokens of a workgroup's tile: TT (C + kTilePad) <= kTileShorts
int nchw_tile_tokens(int C)
{
    int tt = 64;
    while (tt * (C + kTilePad) > kTileShorts) tt >>= 1;
    return tt;      // 64 up to C = 480, 32 up to 992, 16 up to 2016, 8 up to 4064, 4 at 4096
}
// the narrow maps' tiles need a fraction of that: the kernels are built with 16, 32 and 64 KB of LDS (more workgroups per CU where 64 tokens fit
// in less); -> the smallest that holds TT tokens
int nchw_tile_shorts(int C, int TT)
{
    const int need = TT * (C + kTilePad);
    return need <= kTileShorts / 4 ? kTileShorts / 4 : need <= kTileShorts / 2 ? kTileShorts / 2 : kTileShorts;
}

template <int TILE>
__global__ __launch_bounds__(256) void norm_nchw_fwd_kernel(const uint16_t *__restrict__ x, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, float eps, int HW, int C, int TT, int tiles,
                                                            uint16_t *__restrict__ out, float *__restrict__ mean, float *__restrict__ rstd)
{
    __shared__ __attribute__((aligned(16))) uint16_t tile[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nch = C >> 3, ld = C + kTilePad;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, n = min(TT, HW - t0);
    for (int t = wave; t < n; t += 4) {
        const size_t tok = (size_t)b * HW + t0 + t;
        const uint16_t *row = x + tok * C;
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
        const float fc = (float)C, mu = wave_sum(s) / fc;
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
                *reinterpret_cast<u32x4 *>(tile + t * ld + 8 * ch) = pack8(o);      // (rounded here: the store below moves bits)
            }
        }
    }
    __syncthreads();
    // channel c's run: elements e0 .. e0 + n - 1 of out, e0 = (b C + c) HW + t0.  Item (c, k): the k-th 16-byte chunk of the buffer the run touches.
    const int nck = (TT + 7) / 8 + 1;
    for (int item = tid; item < C * nck; item += 256) {
        const int c = item / nck, k = item - c * nck;
        const int64_t e0 = ((int64_t)b * C + c) * HW + t0, e1 = e0 + n, g0 = ((e0 >> 3) + k) << 3;
        if (g0 >= e1) continue;
        const int first = (int)(g0 - e0), lo = max(0, -first), hi = (int)min((int64_t)8, e1 - g0);      // chunk element i = token first + i of the tile
        const uint16_t *src = tile + c;
        if (lo == 0 && hi == 8) {
            u32x4 u;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                u[i] = (unsigned)src[(first + 2 * i) * ld] | ((unsigned)src[(first + 2 * i + 1) * ld] << 16);
            *reinterpret_cast<u32x4 *>(out + g0) = u;
        } else {
            for (int i = lo; i < hi; ++i) out[g0 + i] = src[(first + i) * ld];
        }
    }
}

template <int TILE>
__global__ __launch_bounds__(256) void norm_nchw_bwd_rows_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                 const float *__restrict__ mean, const float *__restrict__ rstd,
                                                                 const float *__restrict__ gamma, int HW, int C, int TT, int tiles,
                                                                 uint16_t *__restrict__ dx)
{
    __shared__ __attribute__((aligned(16))) uint16_t tile[TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nch = C >> 3, ld = C + kTilePad;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x - b * tiles) * TT, n = min(TT, HW - t0);
    // dy's runs into the tile, in the 16-byte chunks of the buffer they touch (item (c, k) as in the forward's store): whole chunks with one
    // 16-byte load, the ragged ones at either end element by element
    const int nck = (TT + 7) / 8 + 1;
#pragma unroll 4
    for (int item = tid; item < C * nck; item += 256) {
        const int c = item / nck, k = item - c * nck;
        const int64_t e0 = ((int64_t)b * C + c) * HW + t0, e1 = e0 + n, g0 = ((e0 >> 3) + k) << 3;
        if (g0 >= e1) continue;
        const int first = (int)(g0 - e0), lo = max(0, -first), hi = (int)min((int64_t)8, e1 - g0);
        uint16_t *dst = tile + c;
        if (lo == 0 && hi == 8) {
            const u32x4 u = *reinterpret_cast<const u32x4 *>(dy + g0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dst[(first + 2 * i) * ld] = (uint16_t)(u[i] & 0xFFFFu);
                dst[(first + 2 * i + 1) * ld] = (uint16_t)(u[i] >> 16);
            }
        } else {
            for (int i = lo; i < hi; ++i) dst[(first + i) * ld] = dy[g0 + i];
        }
    }
    __syncthreads();
    for (int t = wave; t < n; t += 4) {
        const size_t tok = (size_t)b * HW + t0 + t, base = tok * C;
        const float mu = mean[tok], rs = rstd[tok];
        float gv[kLnChunks][8], xh[kLnChunks][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < kLnChunks; ++i) {
            const int ch = lane + 64 * i;
            if (ch < nch) {
                unpack8(*reinterpret_cast<const u32x4 *>(tile + t * ld + 8 * ch), gv[i]);
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
                *reinterpret_cast<u32x4 *>(dx + base + 8 * ch) = pack8(o);
            }
        }
    }
}

// part p = blockIdx.x (tokens 64 p .. 64 p + 63 of the B HW, images back to back) of channels 128 blockIdx.y + 2 lane + {0, 1}
__global__ __launch_bounds__(256) void norm_nchw_bwd_cols_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x,
                                                                 const float *__restrict__ mean, const float *__restrict__ rstd, int tokens,
                                                                 int HW, int C, float *__restrict__ workspace)
{
    __shared__ __attribute__((aligned(4))) uint16_t dyt[kPartRows * kColLd];      // (token of the part, channel of the group)
    __shared__ float part[4][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c0 = blockIdx.y * kColGroup, ch = c0 + 2 * lane;
    const int t0 = blockIdx.x * kPartRows, t1 = min(t0 + kPartRows, tokens);
    if (t0 + lane < t1) {      // lane <-> token: a wave reads 64 consecutive tokens of one channel row (two rows where the part spans two images)
        const int b = (t0 + lane) / HW, t = t0 + lane - b * HW;
        const uint16_t *src = dy + (size_t)b * C * HW + t;
        const int ncl = min(kColGroup, C - c0);
#pragma unroll 8
        for (int cl = wave; cl < ncl; cl += 4) dyt[lane * kColLd + cl] = src[(size_t)(c0 + cl) * HW];
    }
    __syncthreads();
    float dg0 = 0.f, dg1 = 0.f, db0 = 0.f, db1 = 0.f;
    if (ch < C)
        for (int t = t0 + wave; t < t1; t += 4) {
            const unsigned d = *reinterpret_cast<const unsigned *>(dyt + (t - t0) * kColLd + 2 * lane);
            const unsigned xv = *reinterpret_cast<const unsigned *>(x + (size_t)t * C + ch);
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

// ---- patch rows ------------------------------------------------------------------------------------------------------------------------
struct PatchGeom {
    int Cin, H, W, ph, pw, Wh, Ww, K, Kp;      // K = Cin ph pw, Kp = K rounded up to a multiple of 32
};

// one thread per 16-byte chunk of the rows
__global__ __launch_bounds__(256) void patch_rows_kernel(const uint16_t *__restrict__ img, PatchGeom g, int64_t chunks, uint16_t *__restrict__ rows)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int per = g.Kp >> 3, row = (int)(id / per), k0 = 8 * (int)(id - (int64_t)row * per);
    const int bi = row / g.Ww, j = row - bi * g.Ww, b = bi / g.Wh, i = bi - b * g.Wh, area = g.ph * g.pw;
    unsigned v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = k0 + e, c = k / area, r = k - c * area, dy = r / g.pw, y = i * g.ph + dy, xx = j * g.pw + (r - dy * g.pw);
        v[e] = 0u;
        if (k < g.K && y < g.H && xx < g.W) v[e] = img[((size_t)(b * g.Cin + c) * g.H + y) * g.W + xx];
    }
    *reinterpret_cast<u32x4 *>(rows + (size_t)row * g.Kp + k0) = (u32x4){v[0] | v[1] << 16, v[2] | v[3] << 16, v[4] | v[5] << 16, v[6] | v[7] << 16};
}

// one thread per image element
__global__ __launch_bounds__(256) void patch_rows_bwd_kernel(const uint16_t *__restrict__ drows, PatchGeom g, int64_t elems, uint16_t *__restrict__ dimg)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    const int64_t ey = e / g.W, ec = ey / g.H;
    const int xx = (int)(e - ey * g.W), y = (int)(ey - ec * g.H), b = (int)(ec / g.Cin), c = (int)(ec - (int64_t)b * g.Cin);
    const int i = y / g.ph, j = xx / g.pw, col = (c * g.ph + (y - i * g.ph)) * g.pw + (xx - j * g.pw);
    dimg[e] = drows[((size_t)(b * g.Wh + i) * g.Ww + j) * g.Kp + col];
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------------
int merge_dims(int B, int H, int W, int C, int *rows)
{
    if (B < 1 || H < 1 || W < 1 || C < 32 || C % 32 || 4 * (int64_t)C > kMaxC) return MSDA_ERR_BAD_DIMS;
    const int64_t r = (int64_t)B * ((H + (int64_t)1) / 2) * ((W + (int64_t)1) / 2);
    if ((int64_t)B * H * W * C >= (int64_t)1 << 31 || r * 4 * C >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    *rows = (int)r;
    return MSDA_OK;
}

int nchw_dims(int B, int HW, int C)
{
    if (B < 1 || HW < 1) return MSDA_ERR_BAD_DIMS;
    return ln_dims((int64_t)B * HW, C);
}

int patch_dims(int B, int Cin, int H, int W, int ph, int pw, PatchGeom *g, int64_t *rows)
{
    if (B < 1 || Cin < 1 || H < 1 || W < 1 || ph < 1 || pw < 1) return MSDA_ERR_BAD_DIMS;
    const int64_t K = (int64_t)Cin * ph * pw, Kp = (K + 31) / 32 * 32;
    if (Kp > kMaxKp) return MSDA_ERR_BAD_DIMS;
    const int64_t Wh = ((int64_t)H + ph - 1) / ph, Ww = ((int64_t)W + pw - 1) / pw;
    if ((int64_t)B * Cin * H * W >= (int64_t)1 << 31 || B * Wh * Ww * Kp >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    *g = {Cin, H, W, ph, pw, (int)Wh, (int)Ww, (int)K, (int)Kp};
    *rows = B * Wh * Ww;
    return MSDA_OK;
}

}  // namespace

extern "C" {

int msda_swin_merge_norm_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int B, int H, int W, int C,
                                      uint16_t *out, float *mean, float *rstd, msda_stream_t stream)
{
    int rows = 0;
    if (!x || !gamma || !beta || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = merge_dims(B, H, W, C, &rows)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, out}) || !msda::aligned(4, {gamma, beta, mean, rstd})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    merge_norm_fwd_kernel<<<(rows + kLnRows - 1) / kLnRows, kLnRows * 64, 0, (hipStream_t)stream>>>(x, gamma, beta, eps, rows, H, W, C, out, mean,
                                                                                                    rstd);
    return msda::launched(__func__);
}

int msda_swin_merge_norm_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma, int B,
                                       int H, int W, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace, msda_stream_t stream)
{
    int rows = 0;
    if (!dy || !x || !mean || !rstd || !gamma || !dx || ((dgamma || dbeta) && !workspace)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = merge_dims(B, H, W, C, &rows)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {dy, x, dx}) || !msda::aligned(4, {mean, rstd, gamma, dgamma, dbeta, workspace}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    merge_norm_bwd_rows_kernel<<<(rows + kLnRows - 1) / kLnRows, kLnRows * 64, 0, s>>>(dy, x, mean, rstd, gamma, rows, H, W, C, dx);
    if (dgamma || dbeta) {
        const int parts = (rows + kPartRows - 1) / kPartRows, C4 = 4 * C;
        float *ws = static_cast<float *>(workspace);
        merge_norm_bwd_cols_kernel<<<dim3(parts, (C4 + kColGroup - 1) / kColGroup), 256, 0, s>>>(dy, x, mean, rstd, rows, H, W, C, ws);
        swin_ln_bwd_sum_kernel<<<dim3((C4 + 255) / 256, 2), 256, 0, s>>>(ws, parts, C4, dgamma, dbeta);
    }
    return msda::launched(__func__);
}

int msda_swin_norm_nchw_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int B, int HW, int C, uint16_t *out,
                                     float *mean, float *rstd, msda_stream_t stream)
{
    if (!x || !gamma || !beta || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = nchw_dims(B, HW, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, out}) || !msda::aligned(4, {gamma, beta, mean, rstd})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int TT = nchw_tile_tokens(C), tiles = (HW + TT - 1) / TT;
    hipStream_t s = (hipStream_t)stream;
    switch (nchw_tile_shorts(C, TT)) {
    case kTileShorts / 4: norm_nchw_fwd_kernel<kTileShorts / 4><<<B * tiles, 256, 0, s>>>(x, gamma, beta, eps, HW, C, TT, tiles, out, mean, rstd); break;
    case kTileShorts / 2: norm_nchw_fwd_kernel<kTileShorts / 2><<<B * tiles, 256, 0, s>>>(x, gamma, beta, eps, HW, C, TT, tiles, out, mean, rstd); break;
    default: norm_nchw_fwd_kernel<kTileShorts><<<B * tiles, 256, 0, s>>>(x, gamma, beta, eps, HW, C, TT, tiles, out, mean, rstd); break;
    }
    return msda::launched(__func__);
}

int msda_swin_norm_nchw_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma, int B,
                                      int HW, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace, msda_stream_t stream)
{
    if (!dy || !x || !mean || !rstd || !gamma || !dx || ((dgamma || dbeta) && !workspace)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = nchw_dims(B, HW, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {dy, x, dx}) || !msda::aligned(4, {mean, rstd, gamma, dgamma, dbeta, workspace}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    const int TT = nchw_tile_tokens(C), tiles = (HW + TT - 1) / TT, tokens = B * HW;
    switch (nchw_tile_shorts(C, TT)) {
    case kTileShorts / 4: norm_nchw_bwd_rows_kernel<kTileShorts / 4><<<B * tiles, 256, 0, s>>>(dy, x, mean, rstd, gamma, HW, C, TT, tiles, dx); break;
    case kTileShorts / 2: norm_nchw_bwd_rows_kernel<kTileShorts / 2><<<B * tiles, 256, 0, s>>>(dy, x, mean, rstd, gamma, HW, C, TT, tiles, dx); break;
    default: norm_nchw_bwd_rows_kernel<kTileShorts><<<B * tiles, 256, 0, s>>>(dy, x, mean, rstd, gamma, HW, C, TT, tiles, dx); break;
    }
    if (dgamma || dbeta) {
        const int parts = (tokens + kPartRows - 1) / kPartRows;
        float *ws = static_cast<float *>(workspace);
        norm_nchw_bwd_cols_kernel<<<dim3(parts, (C + kColGroup - 1) / kColGroup), 256, 0, s>>>(dy, x, mean, rstd, tokens, HW, C, ws);
        swin_ln_bwd_sum_kernel<<<dim3((C + 255) / 256, 2), 256, 0, s>>>(ws, parts, C, dgamma, dbeta);
    }
    return msda::launched(__func__);
}

int msda_swin_patch_rows_bf16(const uint16_t *img, int B, int Cin, int H, int W, int ph, int pw, uint16_t *rows, msda_stream_t stream)
{
    PatchGeom g;
    int64_t n = 0;
    if (!img || !rows) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = patch_dims(B, Cin, H, W, ph, pw, &g, &n)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(2, {img}) || !msda::aligned(16, {rows})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int64_t chunks = n * (g.Kp >> 3);
    patch_rows_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>(img, g, chunks, rows);
    return msda::launched(__func__);
}

int msda_swin_patch_rows_backward_bf16(const uint16_t *drows, int B, int Cin, int H, int W, int ph, int pw, uint16_t *dimg, msda_stream_t stream)
{
    PatchGeom g;
    int64_t n = 0;
    if (!drows || !dimg) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = patch_dims(B, Cin, H, W, ph, pw, &g, &n)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {drows}) || !msda::aligned(2, {dimg})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int64_t elems = (int64_t)B * Cin * H * W;
    patch_rows_bwd_kernel<<<(unsigned)((elems + 255) / 256), 256, 0, (hipStream_t)stream>>>(drows, g, elems, dimg);
    return msda::launched(__func__);
}

}  // extern "C"
