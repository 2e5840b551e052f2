// convnext_dw.hip -- the two operators a ConvNeXt block needs that the library did not have ("ConvNeXt"): the depthwise
// 7 x 7 convolution (forward, input gradient, weight gradient) and the layer scale x + gamma z with its dgamma.
//
// Reference: models/richsem/convnext.py:18-53 (Block: dwconv, ..., gamma, residual).  The map is channels-last (B, H, W, C) bf16, "map
// layout"; all arithmetic and accumulation is fp32, every stored bf16 element is rounded once, at its store.  No atomics, no allocation, no
// synchronisation: the same bits on every call.
//
// Depthwise convolution.  A workgroup of 256 threads takes a 16 x 16 pixel tile of one image and 32 channels: the 22 x 22 halo tile is
//   staged once in LDS (16-byte loads; a pixel outside THIS image is a zero, so a halo never reads the neighbouring image of the batch),
//   rows padded to 23 pixels so that the four rows of a wave fall on different banks.  A lane owns a channel PAIR (one dword: global and
//   LDS accesses are contiguous along C) and one row of the tile, as two strips of 8 outputs; per tap row it loads the row's 7 x 2 weights
//   (tap-major (49, C) fp32: coalesced along channels) and slides along x: each LDS dword is read once per tap row and feeds up to 7 x 2
//   accumulators.  32 accumulators + 14 weights: no kernel keeps 49 x 2 weights live.  `flip` reads tap 48 - t in place of t: the input
//   gradient is the same kernel, with the residual stream's gradient as `add`.
// Weight gradient.  The same tile and the same sliding window with the roles changed: dy of the lane's 16 pixels in registers, 49 x 2
//   accumulators that persist over the tiles of a part (a part = `tiles per part` consecutive (image, tile) pairs, a function of the shape
//   alone); at the end the four rows of a wave are added by two shuffles, the four waves in wave order through LDS, and the part's 50 rows
//   (49 taps + dbias) go to the workspace; one pass adds the parts in ascending order.
// Layer scale.  Element-wise kernels on 16-byte chunks; dgamma as parts of 64 k tokens (a wave every fourth token, the four waves added in
//   wave order; k = 1 up to 16384 tokens, then the smallest that keeps the parts at 256 or fewer) through the LayerNorm workspace and
//   swin_ln_bwd_sum_kernel, the parts added in ascending order.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"
#include "swin_rows.h"

namespace {

constexpr int kDwTile = 16;                     // output pixels per tile side
constexpr int kDwHalo = kDwTile + 6;            // 22
constexpr int kDwLdX = kDwHalo + 1;             // pixels per LDS row: 23 x 16 dwords = 16 (mod 32), consecutive rows on the other half of the banks
constexpr int kDwGroup = 32;                    // channels per workgroup (16 lanes x 2)
constexpr int kDwStrip = 8;                     // outputs a lane slides over at a time
constexpr int kDwTileDwords = kDwHalo * kDwLdX * (kDwGroup / 2);      // 8096 dwords = 32384 bytes
constexpr int kDwRows = 50;                     // rows of a part in the workspace: 49 taps + dbias
constexpr int kDwTargetGroups = 512;            // workgroups the weight gradient aims at (parts = this / channel groups, at least 1)
constexpr int kScaleMaxParts = 256;             // partial rows of the layer scale's dgamma, at most

struct DwGeom {
    int H, W, C, tilesX, tiles;      // tiles = per image
};

// the halo tile of image b, tile origin (ty0, tx0), channels c0 .. c0 + 31: tile[(py * kDwLdX + px) * 16 + channel pair]
__device__ __forceinline__ void dw_load_halo(unsigned *tile, const uint16_t *__restrict__ x, DwGeom g, int b, int ty0, int tx0, int c0, int tid)
{
    for (int id = tid; id < kDwHalo * kDwHalo * 4; id += 256) {
        const int pix = id >> 2, q = id & 3, py = pix / kDwHalo, px = pix - py * kDwHalo, gy = ty0 + py - 3, gx = tx0 + px - 3;
        u32x4 u = (u32x4){0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W)
            u = *reinterpret_cast<const u32x4 *>(x + ((size_t)(b * g.H + gy) * g.W + gx) * g.C + c0 + 8 * q);
        *reinterpret_cast<u32x4 *>(tile + (py * kDwLdX + px) * 16 + 4 * q) = u;
    }
}

__global__ __launch_bounds__(256) void dwconv7_kernel(const uint16_t *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                      const uint16_t *__restrict__ add, int flip, DwGeom g, uint16_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) unsigned tile[kDwTileDwords];
    const int tid = threadIdx.x, cp = tid & 15, r = tid >> 4, ncg = g.C >> 5;
    const int cg = blockIdx.x % ncg, rest = blockIdx.x / ncg, tl = rest % g.tiles, b = rest / g.tiles;
    const int ty0 = (tl / g.tilesX) * kDwTile, tx0 = (tl % g.tilesX) * kDwTile, ch = cg * kDwGroup + 2 * cp;
    dw_load_halo(tile, x, g, b, ty0, tx0, cg * kDwGroup, tid);
    __syncthreads();
    float acc[2][kDwStrip][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o = 0; o < kDwStrip; ++o) acc[s][o][0] = acc[s][o][1] = 0.f;
#pragma unroll 1      // (unrolled, the compiler hoists all 98 weight loads and the LDS reads: 256 VGPRs, one wave per SIMD)
    for (int ky = 0; ky < 7; ++ky) {
        float wk[7][2];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) {
            const int t = 7 * ky + kx, tt = flip ? 48 - t : t;
            wk[kx][0] = w[(size_t)tt * g.C + ch];
            wk[kx][1] = w[(size_t)tt * g.C + ch + 1];
        }
        const unsigned *row = tile + (r + ky) * kDwLdX * 16 + cp;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < kDwStrip + 6; ++i) {
                const unsigned u = row[(kDwStrip * s + i) * 16];
                const float lo = bf16_lo(u), hi = bf16_hi(u);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const int o = i - kx;      // input column i of the strip = output column o + tap kx
                    if (o >= 0 && o < kDwStrip) {
                        acc[s][o][0] += wk[kx][0] * lo;
                        acc[s][o][1] += wk[kx][1] * hi;
                    }
                }
            }
    }
    const int y = ty0 + r;
    if (y >= g.H) return;
    const float b0 = bias ? bias[ch] : 0.f, b1 = bias ? bias[ch + 1] : 0.f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o = 0; o < kDwStrip; ++o) {
            const int xx = tx0 + kDwStrip * s + o;
            if (xx >= g.W) continue;
            const size_t at = ((size_t)(b * g.H + y) * g.W + xx) * g.C + ch;
            float v0 = acc[s][o][0] + b0, v1 = acc[s][o][1] + b1;
            if (add) {
                const unsigned a = *reinterpret_cast<const unsigned *>(add + at);
                v0 += bf16_lo(a);
                v1 += bf16_hi(a);
            }
            *reinterpret_cast<unsigned *>(out + at) = pack_bf16(v0, v1);
        }
}

// part p = blockIdx.x / (C / 32): the (image, tile) pairs p tpp .. p tpp + tpp - 1 of the B * tiles; workspace[(p 50 + row) C + channel]
__global__ __launch_bounds__(256) void dwconv7_wgrad_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x, DwGeom g, int total,
                                                            int tpp, float *__restrict__ workspace)
{
    __shared__ __attribute__((aligned(16))) unsigned tile[kDwTileDwords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = tid & 15, r = tid >> 4, ncg = g.C >> 5;
    const int cg = blockIdx.x % ncg, part = blockIdx.x / ncg, ch = cg * kDwGroup + 2 * cp;
    float acc[49][2];
#pragma unroll
    for (int t = 0; t < 49; ++t) acc[t][0] = acc[t][1] = 0.f;
    float db0 = 0.f, db1 = 0.f;
    for (int k = 0; k < tpp; ++k) {
        const int item = part * tpp + k;
        if (item >= total) break;      // (the same for every thread of the workgroup)
        const int b = item / g.tiles, tl = item - b * g.tiles, ty0 = (tl / g.tilesX) * kDwTile, tx0 = (tl % g.tilesX) * kDwTile, y = ty0 + r;
        __syncthreads();      // the previous tile has been read
        dw_load_halo(tile, x, g, b, ty0, tx0, cg * kDwGroup, tid);
        float d[2][kDwStrip][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int o = 0; o < kDwStrip; ++o) {
                const int xx = tx0 + kDwStrip * s + o;
                unsigned u = 0u;
                if (y < g.H && xx < g.W) u = *reinterpret_cast<const unsigned *>(dy + ((size_t)(b * g.H + y) * g.W + xx) * g.C + ch);
                d[s][o][0] = bf16_lo(u);
                d[s][o][1] = bf16_hi(u);
                db0 += d[s][o][0];
                db1 += d[s][o][1];
            }
        __syncthreads();
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const unsigned *row = tile + (r + ky) * kDwLdX * 16 + cp;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int i = 0; i < kDwStrip + 6; ++i) {
                    const unsigned u = row[(kDwStrip * s + i) * 16];
                    const float lo = bf16_lo(u), hi = bf16_hi(u);
#pragma unroll
                    for (int kx = 0; kx < 7; ++kx) {
                        const int o = i - kx;
                        if (o >= 0 && o < kDwStrip) {
                            acc[7 * ky + kx][0] += d[s][o][0] * lo;
                            acc[7 * ky + kx][1] += d[s][o][1] * hi;
                        }
                    }
                }
        }
    }
    // the four rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48), then the four waves in wave order through LDS
    __syncthreads();
    float *parts = reinterpret_cast<float *>(tile);      // [wave][row][32 channels]: 4 x 50 x 32 floats = 25600 bytes of the 32384
#pragma unroll
    for (int t = 0; t < kDwRows; ++t) {
        float v0 = t < 49 ? acc[t < 49 ? t : 0][0] : db0, v1 = t < 49 ? acc[t < 49 ? t : 0][1] : db1;
        v0 += __shfl_xor(v0, 16, 64);
        v1 += __shfl_xor(v1, 16, 64);
        v0 += __shfl_xor(v0, 32, 64);
        v1 += __shfl_xor(v1, 32, 64);
        if (lane < 16) {
            parts[(wave * kDwRows + t) * kDwGroup + 2 * cp] = v0;
            parts[(wave * kDwRows + t) * kDwGroup + 2 * cp + 1] = v1;
        }
    }
    __syncthreads();
    for (int item = tid; item < kDwRows * kDwGroup; item += 256) {
        const int row = item >> 5, c = item & 31;
        const float s = ((parts[row * kDwGroup + c] + parts[(kDwRows + row) * kDwGroup + c]) + parts[(2 * kDwRows + row) * kDwGroup + c]) +
                        parts[(3 * kDwRows + row) * kDwGroup + c];
        workspace[((size_t)part * kDwRows + row) * g.C + cg * kDwGroup + c] = s;
    }
}

// dw (49, C) and dbias (C) = the parts' rows added in ascending order
__global__ __launch_bounds__(256) void dwconv7_wgrad_sum_kernel(const float *__restrict__ workspace, int parts, int C, float *__restrict__ dw,
                                                                float *__restrict__ dbias)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= kDwRows * C) return;
    const int row = id / C, c = id - row * C;
    float *dst = row < 49 ? dw + id : (dbias ? dbias + c : nullptr);
    if (!dst) return;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += workspace[((size_t)p * kDwRows + row) * C + c];
    *dst = s;
}

// ---- layer scale -----------------------------------------------------------------------------------------------------------------------
// one thread per 16-byte chunk: out = rnd(res + gamma z), or with res == nullptr out = rnd(gamma z) (dz of the backward, z = dout)
__global__ __launch_bounds__(256) void layer_scale_kernel(const uint16_t *__restrict__ z, const float *__restrict__ gamma,
                                                          const uint16_t *__restrict__ res, int64_t chunks, int C, uint16_t *__restrict__ out)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int c0 = (int)((id * 8) % C);
    float v[8], a[8];
    unpack8(*reinterpret_cast<const u32x4 *>(z + id * 8), v);
    if (res) {
        unpack8(*reinterpret_cast<const u32x4 *>(res + id * 8), a);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = a[j] + gamma[c0 + j] * v[j];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = gamma[c0 + j] * v[j];
    }
    *reinterpret_cast<u32x4 *>(out + id * 8) = pack8(v);
}

// part p = blockIdx.x (tokens rows p .. rows p + rows - 1) of channels 128 blockIdx.y + 2 lane + {0, 1}: workspace[2 p C + channel] (the dgamma
// row of the LayerNorm workspace's layout; the dbeta row stays unwritten and unread)
__global__ __launch_bounds__(256) void layer_scale_bwd_cols_kernel(const uint16_t *__restrict__ dout, const uint16_t *__restrict__ z, int tokens,
                                                                   int rows, int C, float *__restrict__ workspace)
{
    __shared__ float part[4][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = blockIdx.y * kColGroup + 2 * lane;
    const int t0 = blockIdx.x * rows, t1 = min(t0 + rows, tokens);
    float g0 = 0.f, g1 = 0.f;
    if (ch < C)
#pragma unroll 8
        for (int t = t0 + wave; t < t1; t += 4) {
            const unsigned d = *reinterpret_cast<const unsigned *>(dout + (size_t)t * C + ch);
            const unsigned v = *reinterpret_cast<const unsigned *>(z + (size_t)t * C + ch);
            g0 += bf16_lo(d) * bf16_lo(v);
            g1 += bf16_hi(d) * bf16_hi(v);
        }
    part[wave][0][lane] = g0;
    part[wave][1][lane] = g1;
    __syncthreads();
    if (wave == 0 && ch < C) {
        float *dst = workspace + (size_t)blockIdx.x * 2 * C + ch;
        dst[0] = ((part[0][0][lane] + part[1][0][lane]) + part[2][0][lane]) + part[3][0][lane];
        dst[1] = ((part[0][1][lane] + part[1][1][lane]) + part[2][1][lane]) + part[3][1][lane];
    }
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------------
int dw_dims(int B, int H, int W, int C, DwGeom *g)
{
    if (B < 1 || H < 1 || W < 1 || C < 32 || C > kMaxC || C % 32) return MSDA_ERR_BAD_DIMS;
    if ((int64_t)B * H * W * C >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    const int tilesX = (W + kDwTile - 1) / kDwTile, tilesY = (H + kDwTile - 1) / kDwTile;
    *g = {H, W, C, tilesX, tilesX * tilesY};
    return MSDA_OK;
}

// -> parts; *tpp = (image, tile) pairs per part.  A function of the shape alone.
int dw_wgrad_parts(int B, const DwGeom &g, int *tpp)
{
    const int total = B * g.tiles, want = kDwTargetGroups / (g.C >> 5) > 0 ? kDwTargetGroups / (g.C >> 5) : 1;
    *tpp = (total + want - 1) / want;
    return (total + *tpp - 1) / *tpp;
}

}  // namespace

extern "C" {

int msda_dwconv7_bf16(const uint16_t *x, const float *w, const float *bias, const uint16_t *add, int flip, int B, int H, int W, int C,
                      uint16_t *out, msda_stream_t stream)
{
    DwGeom g;
    if (!x || !w || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (flip != 0 && flip != 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (const int e = dw_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, add, out}) || !msda::aligned(4, {w, bias})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    dwconv7_kernel<<<(unsigned)(B * g.tiles * (C >> 5)), 256, 0, (hipStream_t)stream>>>(x, w, bias, add, flip, g, out);
    return msda::launched(__func__);
}

int msda_dwconv7_workspace_bytes(int B, int H, int W, int C, int64_t *bytes)
{
    DwGeom g;
    int tpp = 0;
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = dw_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    *bytes = (int64_t)dw_wgrad_parts(B, g, &tpp) * kDwRows * C * (int64_t)sizeof(float);
    return MSDA_OK;
}

int msda_dwconv7_wgrad_bf16(const uint16_t *dy, const uint16_t *x, int B, int H, int W, int C, float *dw, float *dbias, void *workspace,
                            msda_stream_t stream)
{
    DwGeom g;
    int tpp = 0;
    if (!dy || !x || !dw || !workspace) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = dw_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {dy, x}) || !msda::aligned(4, {dw, dbias, workspace})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int parts = dw_wgrad_parts(B, g, &tpp);
    hipStream_t s = (hipStream_t)stream;
    float *ws = static_cast<float *>(workspace);
    dwconv7_wgrad_kernel<<<(unsigned)(parts * (C >> 5)), 256, 0, s>>>(dy, x, g, B * g.tiles, tpp, ws);
    dwconv7_wgrad_sum_kernel<<<(kDwRows * C + 255) / 256, 256, 0, s>>>(ws, parts, C, dw, dbias);
    return msda::launched(__func__);
}

int msda_layer_scale_forward_bf16(const uint16_t *z, const float *gamma, const uint16_t *res, int tokens, int C, uint16_t *out,
                                  msda_stream_t stream)
{
    if (!z || !gamma || !res || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {z, res, out}) || !msda::aligned(4, {gamma})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int64_t chunks = (int64_t)tokens * C / 8;
    layer_scale_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>(z, gamma, res, chunks, C, out);
    return msda::launched(__func__);
}

int msda_layer_scale_backward_bf16(const uint16_t *dout, const uint16_t *z, const float *gamma, int tokens, int C, uint16_t *dz, float *dgamma,
                                   void *workspace, msda_stream_t stream)
{
    if (!dout || !gamma || !dz || (dgamma && (!workspace || !z))) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {dout, z, dz}) || !msda::aligned(4, {gamma, dgamma, workspace})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = (int64_t)tokens * C / 8;
    layer_scale_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(dout, gamma, nullptr, chunks, C, dz);
    if (dgamma) {
        // The workspace holds a row per 64 tokens; the last pass adds the rows one after the other, in one thread per channel.  So that this
        // chain stays short on a large map a part takes 64 k tokens, k the smallest for which there are at most kScaleMaxParts parts (a
        // function of `tokens` alone: the same bits on every call), and only the first `parts` rows of the workspace are used.
        const int rows = kPartRows * (((tokens + kPartRows - 1) / kPartRows + kScaleMaxParts - 1) / kScaleMaxParts);
        const int parts = (tokens + rows - 1) / rows;
        float *ws = static_cast<float *>(workspace);
        layer_scale_bwd_cols_kernel<<<dim3(parts, (C + kColGroup - 1) / kColGroup), 256, 0, s>>>(dout, z, tokens, rows, C, ws);
        swin_ln_bwd_sum_kernel<<<dim3((C + 255) / 256, 1), 256, 0, s>>>(ws, parts, C, dgamma, nullptr);
    }
    return msda::launched(__func__);
}

}  // extern "C"
