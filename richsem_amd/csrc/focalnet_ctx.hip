// focalnet_ctx.hip -- the hierarchical context aggregation of a FocalNet block ("FocalNet"): the core of
// FocalModulation.forward (reference models/richsem/focal.py:84-110), forward and backward, and the modulation product q * h(A).
// C ABI msda_fmod_* (include/richsem_msda.h).
//
// The contract.  L = focal_level in 1..4, K_l = window + 2 l in {3, 5, 7, 9}, s = 1 / (L + 1) with `normalize`, else 1.  Maps are
// channels-last (B, H, W, C) bf16, C a multiple of 32; a map argument with a row stride `ld*` (elements per pixel, a multiple of 8) is read
// or written in place in wider rows (the output rows of `f`, or their gradient); the gates are (B, H, W, L + 1) bf16 with a stride of their
// own.  Weights are fp32, tap-major (K_l K_l, C), the levels one after the other.  fp32 arithmetic and accumulation, zero padding per image
// (a halo never reads the neighbouring image), no atomics, no allocation, no synchronisation, every reduction in a fixed order.
//
//   u_l    = dwconv_{K_l}(ctx_{l-1}),  ctx_l = GELU(u_l) (erf form),  l = 0 .. L-1;  ctx_{-1} = ctx0
//   m[b,c] = mean_{y,x} ctx_{L-1}[b,y,x,c]  per image;  g = GELU(m)
//   A      = s (sum_{l<L} gate_l ctx_l + gate_L g)
//   backward, given dA:
//   dgate_l[p] = s sum_c dA[p,c] ctx_l[p,c] (l < L),  dgate_L[p] = s sum_c dA[p,c] g[b,c]
//   dg[b,c]    = s sum_p dA[p,c] gate_L[p],  dm = dg GELU'(m)
//   du_{L-1}   = (s gate_{L-1} dA + dm / (H W)) GELU'(u_{L-1})
//   du_{l-1}   = (dwconv_flip_{K_l}(du_l) + s gate_{l-1} dA) GELU'(u_{l-1}),  l = L-1 .. 1
//   dctx0      = dwconv_flip_{K_0}(du_0);   dW_l = wgrad_{K_l}(du_l, ctx_{l-1})
//
// The rounding points.  Stored in bf16, each rounded once at its store: u_l, A, du_l, dctx0, dgate_l (and out, dq, dmod of the product).
// Only the pre-activations u_l are kept between levels; every consumer regenerates ctx_l = GELU(u_l) from the STORED u_l in fp32 -- with one
// exception that is a rounding point of its own: where ctx_l is the INPUT of a convolution or of a weight gradient it is rounded to bf16 as
// the LDS tile is filled (the tile holds bf16 channel pairs; an fp32 tile of a 9 x 9 halo does not fit beside a second workgroup).  m, g,
// dg, dm and dW are fp32 and never rounded to bf16.  The mean is taken over GELU of the stored (rounded) u_{L-1}.
//
// The cut.
//   fmod_conv_kernel<K>      dwconv7's tile generalised: a workgroup takes 16 x 16 pixels x 32 channels, the (16 + K - 1)^2 halo tile in LDS
//                            (rows padded to an odd number of pixels), a lane owns a channel pair and one row as two strips of 8 outputs and
//                            slides along x.  Options: GELU on the input as the tile is filled; flipped taps; the epilogue
//                            "+ s gate dA, times GELU'(u)"; per-tile sums of GELU(out) (last level: the four rows of a wave by two shuffles,
//                            the four waves in wave order through LDS).
//   fmod_mean_kernel         adds the tiles' sums in ascending order: m, g.
//   fmod_gather_kernel       A from the stored u_l, levels in ascending order, the global term last, one rounding.
//   fmod_gate_grad_kernel    a wave per pixel over all of C: the L + 1 gate gradients.
//   fmod_dg_cols_kernel      partial sums of dg per image (a wave every fourth pixel of a part, the waves in wave order);
//   fmod_dm_kernel           adds them in ascending order: dm / (H W).
//   fmod_top_kernel          element-wise du_{L-1}.
//   fmod_wgrad_kernel<K>     one TAP ROW ky per workgroup (grid: parts x channel groups x K), so a lane keeps K x 2 accumulators, not
//                            K K x 2 (81 x 2 would not fit without scratch): dy of the lane's 16 pixels in registers, the 16 rows of the
//                            halo tile this tap row reads in LDS; partial rows per part, added in ascending order by fmod_wgrad_sum_kernel.
//   fmod_product_kernel      element-wise on 16-byte chunks, either operand and the result in rows of their own stride: msda_fmod_modulate_*
//                            are out = rnd(q mod) and dq = rnd(dout mod), dmod = rnd(dout q).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"
#include "swin_rows.h"

namespace {

constexpr int kFmTile = 16;                // output pixels per tile side
constexpr int kFmGroup = 32;               // channels per workgroup (16 lanes x 2)
constexpr int kFmStrip = 8;                // outputs a lane slides over at a time
constexpr int kFmMaxL = 4;                 // focal levels, at most (K = 3, 5, 7, 9)
constexpr int kFmTargetGroups = 512;       // workgroups per tap row the weight gradient aims at
constexpr int kFmMaxDgParts = 64;          // partial rows of dg per image, at most

constexpr float kFmRsqrt2 = 0.70710678118654752f;
constexpr float kFmRsqrt2Pi = 0.39894228040143268f;

__device__ __forceinline__ float fm_cdf(float x) { return 0.5f * erfcf(-x * kFmRsqrt2); }
__device__ __forceinline__ float fm_gelu(float x) { return x * fm_cdf(x); }
__device__ __forceinline__ float fm_gelu_grad(float x) { return fm_cdf(x) + x * (kFmRsqrt2Pi * __expf(-0.5f * x * x)); }
__device__ __forceinline__ float fm_bf16(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }

struct FmGeom {
    int B, H, W, C, tilesX, tiles;      // tiles = per image
};

template <int K>
struct FmTile {
    static constexpr int pad = K / 2, halo = kFmTile + K - 1, ldx = halo + 1;      // ldx odd: 16 ldx dwords = 16 (mod 32)
    static constexpr int dwords = halo * ldx * (kFmGroup / 2);                      // K = 9: 9600 dwords = 38400 bytes
};

// rows py0 .. py0 + nrows - 1 of the halo tile of image b, tile origin (ty0, tx0), channels c0 .. c0 + 31, from a map with `ld` elements
// per pixel: tile[(py * ldx + px) * 16 + channel pair]; a pixel outside THIS image is a zero (GELU(0) = 0 as well)
template <int K>
__device__ __forceinline__ void fm_fill(unsigned *tile, const uint16_t *__restrict__ x, int64_t ld, const FmGeom &g, int b, int ty0, int tx0,
                                        int c0, int tid, int gelu_in, int py0, int nrows)
{
    constexpr int halo = FmTile<K>::halo, ldx = FmTile<K>::ldx, pad = FmTile<K>::pad;
    for (int id = tid; id < nrows * halo * 4; id += 256) {
        const int pix = id >> 2, q = id & 3, pr = pix / halo, px = pix - pr * halo, py = py0 + pr, gy = ty0 + py - pad, gx = tx0 + px - pad;
        u32x4 u = (u32x4){0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < g.H && gx >= 0 && gx < g.W) {
            u = *reinterpret_cast<const u32x4 *>(x + ((int64_t)(b * g.H + gy) * g.W + gx) * ld + c0 + 8 * q);
            if (gelu_in) {
                float v[8];
                unpack8(u, v);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = fm_gelu(v[j]);
                u = pack8(v);
            }
        }
        *reinterpret_cast<u32x4 *>(tile + (py * ldx + px) * 16 + 4 * q) = u;
    }
}

struct FmConv {
    const uint16_t *x;          // input map, ldx elements per pixel
    int64_t ldx;
    const float *w;             // (K K, C)
    int flip, gelu_in;
    const uint16_t *gate;       // epilogue (dA != nullptr): out = (acc + s gate[p ldg] dA[p, c]) GELU'(uprev[p, c]); dA, uprev dense
    int64_t ldg;
    float s;
    const uint16_t *dA, *uprev;
    float *psum;                // or nullptr: [(b tiles + tile) C + c] = sum over the tile's pixels of GELU(rnd(out))
    uint16_t *out;              // ldo elements per pixel
    int64_t ldo;
};

template <int K>
__global__ __launch_bounds__(256) void fmod_conv_kernel(FmConv a, FmGeom g)
{
    constexpr int ldx = FmTile<K>::ldx;
    __shared__ __attribute__((aligned(16))) unsigned tile[FmTile<K>::dwords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = tid & 15, r = tid >> 4, ncg = g.C >> 5;
    const int cg = blockIdx.x % ncg, rest = blockIdx.x / ncg, tl = rest % g.tiles, b = rest / g.tiles;
    const int ty0 = (tl / g.tilesX) * kFmTile, tx0 = (tl % g.tilesX) * kFmTile, ch = cg * kFmGroup + 2 * cp;
    fm_fill<K>(tile, a.x, a.ldx, g, b, ty0, tx0, cg * kFmGroup, tid, a.gelu_in, 0, FmTile<K>::halo);
    __syncthreads();
    float acc[2][kFmStrip][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int o = 0; o < kFmStrip; ++o) acc[s][o][0] = acc[s][o][1] = 0.f;
#pragma unroll 1
    for (int ky = 0; ky < K; ++ky) {
        float wk[K][2];
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int t = K * ky + kx, tt = a.flip ? K * K - 1 - t : t;
            wk[kx][0] = a.w[(size_t)tt * g.C + ch];
            wk[kx][1] = a.w[(size_t)tt * g.C + ch + 1];
        }
        const unsigned *row = tile + (r + ky) * ldx * 16 + cp;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < kFmStrip + K - 1; ++i) {
                const unsigned u = row[(kFmStrip * s + i) * 16];
                const float lo = bf16_lo(u), hi = bf16_hi(u);
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int o = i - kx;      // input column i of the strip = output column o + tap kx
                    if (o >= 0 && o < kFmStrip) {
                        acc[s][o][0] += wk[kx][0] * lo;
                        acc[s][o][1] += wk[kx][1] * hi;
                    }
                }
            }
    }
    const int y = ty0 + r;
    float s0 = 0.f, s1 = 0.f;
    if (y < g.H) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int o = 0; o < kFmStrip; ++o) {
                const int xx = tx0 + kFmStrip * s + o;
                if (xx >= g.W) continue;
                const int64_t p = (int64_t)(b * g.H + y) * g.W + xx;
                float v0 = acc[s][o][0], v1 = acc[s][o][1];
                if (a.dA) {
                    const float gt = a.s * fm_bf16(a.gate + p * a.ldg);
                    const unsigned d = *reinterpret_cast<const unsigned *>(a.dA + p * g.C + ch);
                    const unsigned up = *reinterpret_cast<const unsigned *>(a.uprev + p * g.C + ch);
                    v0 = (v0 + gt * bf16_lo(d)) * fm_gelu_grad(bf16_lo(up));
                    v1 = (v1 + gt * bf16_hi(d)) * fm_gelu_grad(bf16_hi(up));
                }
                const unsigned packed = pack_bf16(v0, v1);
                *reinterpret_cast<unsigned *>(a.out + p * a.ldo + ch) = packed;
                if (a.psum) {
                    s0 += fm_gelu(bf16_lo(packed));
                    s1 += fm_gelu(bf16_hi(packed));
                }
            }
    }
    if (a.psum) {      // (the same for every thread)
        s0 += __shfl_xor(s0, 16, 64);
        s1 += __shfl_xor(s1, 16, 64);
        s0 += __shfl_xor(s0, 32, 64);
        s1 += __shfl_xor(s1, 32, 64);
        __syncthreads();      // the tile has been read
        float *parts = reinterpret_cast<float *>(tile);      // [wave][32 channels]
        if (lane < 16) {
            parts[wave * kFmGroup + 2 * cp] = s0;
            parts[wave * kFmGroup + 2 * cp + 1] = s1;
        }
        __syncthreads();
        if (tid < kFmGroup)
            a.psum[((size_t)b * g.tiles + tl) * g.C + cg * kFmGroup + tid] =
                ((parts[tid] + parts[kFmGroup + tid]) + parts[2 * kFmGroup + tid]) + parts[3 * kFmGroup + tid];
    }
}

// mg[b C + c] = m = (the tiles' sums added in ascending order) / (H W);  mg[B C + b C + c] = g = GELU(m)
__global__ __launch_bounds__(256) void fmod_mean_kernel(const float *__restrict__ psum, FmGeom g, float *__restrict__ mg)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= g.B * g.C) return;
    const int b = id / g.C, c = id - b * g.C;
    float s = 0.f;
    for (int t = 0; t < g.tiles; ++t) s += psum[((size_t)b * g.tiles + t) * g.C + c];
    const float m = s / (float)(g.H * g.W);
    mg[id] = m;
    mg[g.B * g.C + id] = fm_gelu(m);
}

// one thread per 16-byte chunk: A = rnd(s (sum_{l<L} gate_l GELU(u_l) + gate_L g)), the levels in ascending order
__global__ __launch_bounds__(256) void fmod_gather_kernel(const uint16_t *__restrict__ u, const uint16_t *__restrict__ gates, int64_t ldg,
                                                          const float *__restrict__ mg, int L, float s, FmGeom g, int64_t chunks,
                                                          uint16_t *__restrict__ A)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int cpr = g.C >> 3;
    const int64_t p = id / cpr, n = (int64_t)g.B * g.H * g.W * g.C;
    const int c0 = (int)(id - p * cpr) * 8, b = (int)(p / ((int64_t)g.H * g.W));
    float acc[8], v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int l = 0; l < L; ++l) {
        const float gt = fm_bf16(gates + p * ldg + l);
        unpack8(*reinterpret_cast<const u32x4 *>(u + (size_t)l * n + p * g.C + c0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += gt * fm_gelu(v[j]);
    }
    const float gt = fm_bf16(gates + p * ldg + L);
    const float *gg = mg + (size_t)g.B * g.C + (size_t)b * g.C + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = s * (acc[j] + gt * gg[j]);
    *reinterpret_cast<u32x4 *>(A + p * g.C + c0) = pack8(acc);
}

// a wave per pixel: dgate_l = rnd(s sum_c dA ctx_l), l < L;  dgate_L = rnd(s sum_c dA g)
__global__ __launch_bounds__(256) void fmod_gate_grad_kernel(const uint16_t *__restrict__ dA, const uint16_t *__restrict__ u,
                                                             const float *__restrict__ mg, int L, float s, FmGeom g, int64_t pixels,
                                                             uint16_t *__restrict__ dgates, int64_t lddg)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * 4 + wave, n = pixels * g.C;
    if (p >= pixels) return;      // (a whole wave)
    const int b = (int)(p / ((int64_t)g.H * g.W));
    float acc[kFmMaxL + 1];
#pragma unroll
    for (int l = 0; l <= kFmMaxL; ++l) acc[l] = 0.f;
    for (int c0 = lane * 8; c0 < g.C; c0 += 512) {
        float d[8], v[8];
        unpack8(*reinterpret_cast<const u32x4 *>(dA + p * g.C + c0), d);
#pragma unroll
        for (int l = 0; l < kFmMaxL; ++l)
            if (l < L) {
                unpack8(*reinterpret_cast<const u32x4 *>(u + (size_t)l * n + p * g.C + c0), v);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[l] += d[j] * fm_gelu(v[j]);
            }
        const float *gg = mg + (size_t)g.B * g.C + (size_t)b * g.C + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[kFmMaxL] += d[j] * gg[j];
    }
#pragma unroll
    for (int l = 0; l <= kFmMaxL; ++l) {
        const float v = s * wave_sum(acc[l]);
        const int at = l == kFmMaxL ? L : l;
        if (lane == 0 && (l < L || l == kFmMaxL)) dgates[p * lddg + at] = (uint16_t)(pack_bf16(v, 0.f) & 0xFFFFu);
    }
}

// part = blockIdx.x of image blockIdx.z (pixels rows part .. rows part + rows - 1 of the image), channels 128 blockIdx.y + 2 lane + {0, 1}:
// workspace[(b parts + part) C + channel] = sum_p dA[p, c] gate_L[p]
__global__ __launch_bounds__(256) void fmod_dg_cols_kernel(const uint16_t *__restrict__ dA, const uint16_t *__restrict__ gateL, int64_t ldg,
                                                           FmGeom g, int rows, float *__restrict__ workspace)
{
    __shared__ float part[4][2][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ch = blockIdx.y * kColGroup + 2 * lane, b = blockIdx.z, hw = g.H * g.W;
    const int t0 = blockIdx.x * rows, t1 = min(t0 + rows, hw);
    float g0 = 0.f, g1 = 0.f;
    if (ch < g.C)
        for (int t = t0 + wave; t < t1; t += 4) {
            const int64_t p = (int64_t)b * hw + t;
            const unsigned d = *reinterpret_cast<const unsigned *>(dA + p * g.C + ch);
            const float gt = fm_bf16(gateL + p * ldg);
            g0 += bf16_lo(d) * gt;
            g1 += bf16_hi(d) * gt;
        }
    part[wave][0][lane] = g0;
    part[wave][1][lane] = g1;
    __syncthreads();
    if (wave == 0 && ch < g.C) {
        float *dst = workspace + ((size_t)b * gridDim.x + blockIdx.x) * g.C + ch;
        dst[0] = ((part[0][0][lane] + part[1][0][lane]) + part[2][0][lane]) + part[3][0][lane];
        dst[1] = ((part[0][1][lane] + part[1][1][lane]) + part[2][1][lane]) + part[3][1][lane];
    }
}

// dmn[b C + c] = s (the parts added in ascending order) GELU'(m) / (H W)
__global__ __launch_bounds__(256) void fmod_dm_kernel(const float *__restrict__ workspace, int parts, const float *__restrict__ mg, float s,
                                                      FmGeom g, float *__restrict__ dmn)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= g.B * g.C) return;
    const int b = id / g.C, c = id - b * g.C;
    float sum = 0.f;
    for (int p = 0; p < parts; ++p) sum += workspace[((size_t)b * parts + p) * g.C + c];
    dmn[id] = s * sum * fm_gelu_grad(mg[id]) / (float)(g.H * g.W);
}

// one thread per 16-byte chunk: du_{L-1} = rnd((s gate_{L-1} dA + dm / (H W)) GELU'(u_{L-1}))
__global__ __launch_bounds__(256) void fmod_top_kernel(const uint16_t *__restrict__ dA, const uint16_t *__restrict__ ulast,
                                                       const uint16_t *__restrict__ gate, int64_t ldg, const float *__restrict__ dmn, float s,
                                                       FmGeom g, int64_t chunks, uint16_t *__restrict__ du)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int cpr = g.C >> 3;
    const int64_t p = id / cpr;
    const int c0 = (int)(id - p * cpr) * 8, b = (int)(p / ((int64_t)g.H * g.W));
    const float gt = s * fm_bf16(gate + p * ldg);
    float d[8], v[8];
    unpack8(*reinterpret_cast<const u32x4 *>(dA + p * g.C + c0), d);
    unpack8(*reinterpret_cast<const u32x4 *>(ulast + p * g.C + c0), v);
    const float *dm = dmn + (size_t)b * g.C + c0;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (gt * d[j] + dm[j]) * fm_gelu_grad(v[j]);
    *reinterpret_cast<u32x4 *>(du + p * g.C + c0) = pack8(d);
}

// tap row ky = blockIdx.x % K, channel group, part: the (image, tile) pairs part tpp .. part tpp + tpp - 1 of the B * tiles;
// workspace[((part K + ky) K + kx) C + channel]
template <int K>
__global__ __launch_bounds__(256) void fmod_wgrad_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x, int64_t ldx, int gelu_in,
                                                         FmGeom g, int total, int tpp, float *__restrict__ workspace)
{
    constexpr int ldsx = FmTile<K>::ldx;
    __shared__ __attribute__((aligned(16))) unsigned tile[FmTile<K>::dwords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = tid & 15, r = tid >> 4, ncg = g.C >> 5;
    const int ky = blockIdx.x % K, rest = blockIdx.x / K, cg = rest % ncg, part = rest / ncg, ch = cg * kFmGroup + 2 * cp;
    float acc[K][2];
#pragma unroll
    for (int kx = 0; kx < K; ++kx) acc[kx][0] = acc[kx][1] = 0.f;
    for (int k = 0; k < tpp; ++k) {
        const int item = part * tpp + k;
        if (item >= total) break;      // (the same for every thread of the workgroup)
        const int b = item / g.tiles, tl = item - b * g.tiles, ty0 = (tl / g.tilesX) * kFmTile, tx0 = (tl % g.tilesX) * kFmTile, y = ty0 + r;
        __syncthreads();      // the previous tile has been read
        fm_fill<K>(tile, x, ldx, g, b, ty0, tx0, cg * kFmGroup, tid, gelu_in, ky, kFmTile);      // the 16 halo rows this tap row reads
        float d[2][kFmStrip][2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int o = 0; o < kFmStrip; ++o) {
                const int xx = tx0 + kFmStrip * s + o;
                unsigned u = 0u;
                if (y < g.H && xx < g.W) u = *reinterpret_cast<const unsigned *>(dy + ((int64_t)(b * g.H + y) * g.W + xx) * g.C + ch);
                d[s][o][0] = bf16_lo(u);
                d[s][o][1] = bf16_hi(u);
            }
        __syncthreads();
        const unsigned *row = tile + (r + ky) * ldsx * 16 + cp;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < kFmStrip + K - 1; ++i) {
                const unsigned u = row[(kFmStrip * s + i) * 16];
                const float lo = bf16_lo(u), hi = bf16_hi(u);
#pragma unroll
                for (int kx = 0; kx < K; ++kx) {
                    const int o = i - kx;
                    if (o >= 0 && o < kFmStrip) {
                        acc[kx][0] += d[s][o][0] * lo;
                        acc[kx][1] += d[s][o][1] * hi;
                    }
                }
            }
    }
    // the four rows of a wave (lanes l, l ^ 16, l ^ 32, l ^ 48), then the four waves in wave order through LDS
    __syncthreads();
    float *parts = reinterpret_cast<float *>(tile);      // [wave][kx][32 channels]
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
        float v0 = acc[kx][0], v1 = acc[kx][1];
        v0 += __shfl_xor(v0, 16, 64);
        v1 += __shfl_xor(v1, 16, 64);
        v0 += __shfl_xor(v0, 32, 64);
        v1 += __shfl_xor(v1, 32, 64);
        if (lane < 16) {
            parts[(wave * K + kx) * kFmGroup + 2 * cp] = v0;
            parts[(wave * K + kx) * kFmGroup + 2 * cp + 1] = v1;
        }
    }
    __syncthreads();
    for (int item = tid; item < K * kFmGroup; item += 256) {
        const int kx = item >> 5, c = item & 31;
        const float s = ((parts[kx * kFmGroup + c] + parts[(K + kx) * kFmGroup + c]) + parts[(2 * K + kx) * kFmGroup + c]) +
                        parts[(3 * K + kx) * kFmGroup + c];
        workspace[(((size_t)part * K + ky) * K + kx) * g.C + cg * kFmGroup + c] = s;
    }
}

// dw (rows, C) = the parts' rows added in ascending order
__global__ __launch_bounds__(256) void fmod_wgrad_sum_kernel(const float *__restrict__ workspace, int parts, int rows, int C, float *__restrict__ dw)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= rows * C) return;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += workspace[(size_t)p * rows * C + id];
    dw[id] = s;
}

// one thread per 16-byte chunk: out = rnd(a b), a with lda elements per token, b and out dense
__global__ __launch_bounds__(256) void fmod_product_kernel(const uint16_t *__restrict__ a, int64_t lda, const uint16_t *__restrict__ b, int64_t ldb,
                                                           int C, int64_t chunks, uint16_t *__restrict__ out, int64_t ldo)
{
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= chunks) return;
    const int cpr = C >> 3;
    const int64_t t = id / cpr;
    const int c0 = (int)(id - t * cpr) * 8;
    float v[8], w[8];
    unpack8(*reinterpret_cast<const u32x4 *>(a + t * lda + c0), v);
    unpack8(*reinterpret_cast<const u32x4 *>(b + t * ldb + c0), w);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= w[j];
    *reinterpret_cast<u32x4 *>(out + t * ldo + c0) = pack8(v);
}

// ---- argument checks and launch plans ------------------------------------------------------------------------------------------------
int fm_dims(int B, int H, int W, int C, FmGeom *g)
{
    if (B < 1 || H < 1 || W < 1 || C < 32 || C > kMaxC || C % 32) return MSDA_ERR_BAD_DIMS;
    if ((int64_t)B * H * W * C >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    const int tilesX = (W + kFmTile - 1) / kFmTile, tilesY = (H + kFmTile - 1) / kFmTile;
    *g = {B, H, W, C, tilesX, tilesX * tilesY};
    return MSDA_OK;
}

// 1 <= L <= 4, window odd, every K_l = window + 2 l in {3, 5, 7, 9}
int fm_levels(int L, int window)
{
    if (L < 1 || L > kFmMaxL || window < 3 || !(window & 1) || window + 2 * (L - 1) > 9) return MSDA_ERR_BAD_DIMS;
    return MSDA_OK;
}

bool fm_stride(int64_t ld, int least) { return ld >= least && ld % 8 == 0 && ld < ((int64_t)1 << 31); }

// -> parts; *tpp = (image, tile) pairs per part.  A function of the shape alone.
int fm_wgrad_parts(const FmGeom &g, int *tpp)
{
    const int total = g.B * g.tiles, want = kFmTargetGroups / (g.C >> 5) > 0 ? kFmTargetGroups / (g.C >> 5) : 1;
    *tpp = (total + want - 1) / want;
    return (total + *tpp - 1) / *tpp;
}

// -> parts per image of dg; *rows = pixels per part (64 k, k the smallest that keeps the parts at kFmMaxDgParts or fewer)
int fm_dg_parts(const FmGeom &g, int *rows)
{
    const int hw = g.H * g.W;
    *rows = kPartRows * (((hw + kPartRows - 1) / kPartRows + kFmMaxDgParts - 1) / kFmMaxDgParts);
    return (hw + *rows - 1) / *rows;
}

int64_t fm_workspace_floats(const FmGeom &g)
{
    int tpp = 0, rows = 0;
    const int64_t fwd = (int64_t)g.B * g.tiles * g.C;
    const int64_t bwd = (int64_t)g.B * fm_dg_parts(g, &rows) * g.C + (int64_t)g.B * g.C;
    const int64_t wg = (int64_t)fm_wgrad_parts(g, &tpp) * 81 * g.C;
    const int64_t most = fwd > bwd ? fwd : bwd;
    return most > wg ? most : wg;
}

template <int K>
void fm_conv_launch(const FmConv &a, const FmGeom &g, hipStream_t s)
{
    fmod_conv_kernel<K><<<(unsigned)(g.B * g.tiles * (g.C >> 5)), 256, 0, s>>>(a, g);
}

void fm_conv(int K, const FmConv &a, const FmGeom &g, hipStream_t s)
{
    switch (K) {
    case 3: fm_conv_launch<3>(a, g, s); break;
    case 5: fm_conv_launch<5>(a, g, s); break;
    case 7: fm_conv_launch<7>(a, g, s); break;
    default: fm_conv_launch<9>(a, g, s); break;
    }
}

template <int K>
void fm_wgrad_launch(const uint16_t *dy, const uint16_t *x, int64_t ldx, int gelu_in, const FmGeom &g, int parts, int tpp, float *ws, float *dw,
                     hipStream_t s)
{
    fmod_wgrad_kernel<K><<<(unsigned)(parts * (g.C >> 5) * K), 256, 0, s>>>(dy, x, ldx, gelu_in, g, g.B * g.tiles, tpp, ws);
    fmod_wgrad_sum_kernel<<<(K * K * g.C + 255) / 256, 256, 0, s>>>(ws, parts, K * K, g.C, dw);
}

void fm_wgrad(int K, const uint16_t *dy, const uint16_t *x, int64_t ldx, int gelu_in, const FmGeom &g, float *ws, float *dw, hipStream_t s)
{
    int tpp = 0;
    const int parts = fm_wgrad_parts(g, &tpp);
    switch (K) {
    case 3: fm_wgrad_launch<3>(dy, x, ldx, gelu_in, g, parts, tpp, ws, dw, s); break;
    case 5: fm_wgrad_launch<5>(dy, x, ldx, gelu_in, g, parts, tpp, ws, dw, s); break;
    case 7: fm_wgrad_launch<7>(dy, x, ldx, gelu_in, g, parts, tpp, ws, dw, s); break;
    default: fm_wgrad_launch<9>(dy, x, ldx, gelu_in, g, parts, tpp, ws, dw, s); break;
    }
}

}  // namespace

extern "C" {

int msda_fmod_workspace_bytes(int B, int H, int W, int C, int64_t *bytes)
{
    FmGeom g;
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = fm_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    *bytes = fm_workspace_floats(g) * (int64_t)sizeof(float);
    return MSDA_OK;
}

int msda_fmod_context_forward_bf16(const uint16_t *ctx0, int64_t ld0, const uint16_t *gates, int64_t ldg, const float *w, int B, int H, int W,
                                   int C, int L, int window, int normalize, uint16_t *u, float *mg, uint16_t *A, void *workspace,
                                   msda_stream_t stream)
{
    FmGeom g;
    if (!ctx0 || !gates || !w || !u || !mg || !A || !workspace) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = fm_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    if (const int e = fm_levels(L, window)) return msda::arg_fail(e, __func__);
    if ((normalize != 0 && normalize != 1) || !fm_stride(ld0, C) || ldg < L + 1 || ldg >= ((int64_t)1 << 31))
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {ctx0, u, A}) || !msda::aligned(4, {w, mg, workspace}) || !msda::aligned(2, {gates}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    float *ws = static_cast<float *>(workspace);
    const int64_t n = (int64_t)B * H * W * C, chunks = n / 8;
    const float scale = normalize ? 1.f / (float)(L + 1) : 1.f;
    int64_t woff = 0;
    for (int l = 0; l < L; ++l) {
        const int K = window + 2 * l;
        FmConv a = {};
        a.x = l ? u + (l - 1) * n : ctx0;
        a.ldx = l ? C : ld0;
        a.w = w + woff * C;
        a.gelu_in = l > 0;
        a.psum = l == L - 1 ? ws : nullptr;
        a.out = u + l * n;
        a.ldo = C;
        fm_conv(K, a, g, s);
        woff += K * K;
    }
    fmod_mean_kernel<<<(B * C + 255) / 256, 256, 0, s>>>(ws, g, mg);
    fmod_gather_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(u, gates, ldg, mg, L, scale, g, chunks, A);
    return msda::launched(__func__);
}

int msda_fmod_context_backward_bf16(const uint16_t *dA, const uint16_t *ctx0, int64_t ld0, const uint16_t *gates, int64_t ldg, const float *w,
                                    const uint16_t *u, const float *mg, int B, int H, int W, int C, int L, int window, int normalize,
                                    uint16_t *du, uint16_t *dctx0, int64_t ldd0, uint16_t *dgates, int64_t lddg, float *dw, void *workspace,
                                    msda_stream_t stream)
{
    FmGeom g;
    if (!dA || !ctx0 || !gates || !w || !u || !mg || !du || !dctx0 || !dgates || !workspace)
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = fm_dims(B, H, W, C, &g)) return msda::arg_fail(e, __func__);
    if (const int e = fm_levels(L, window)) return msda::arg_fail(e, __func__);
    if ((normalize != 0 && normalize != 1) || !fm_stride(ld0, C) || !fm_stride(ldd0, C) || ldg < L + 1 || lddg < L + 1 ||
        ldg >= ((int64_t)1 << 31) || lddg >= ((int64_t)1 << 31))
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {dA, ctx0, u, du, dctx0}) || !msda::aligned(4, {w, mg, dw, workspace}) || !msda::aligned(2, {gates, dgates}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    float *ws = static_cast<float *>(workspace);
    const int64_t pixels = (int64_t)B * H * W, n = pixels * C, chunks = n / 8;
    const float scale = normalize ? 1.f / (float)(L + 1) : 1.f;
    int rows = 0;
    const int parts = fm_dg_parts(g, &rows);
    float *dmn = ws + (size_t)B * parts * C;
    fmod_gate_grad_kernel<<<(unsigned)((pixels + 3) / 4), 256, 0, s>>>(dA, u, mg, L, scale, g, pixels, dgates, lddg);
    fmod_dg_cols_kernel<<<dim3(parts, (C + kColGroup - 1) / kColGroup, B), 256, 0, s>>>(dA, gates + L, ldg, g, rows, ws);
    fmod_dm_kernel<<<(B * C + 255) / 256, 256, 0, s>>>(ws, parts, mg, scale, g, dmn);
    fmod_top_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(dA, u + (L - 1) * n, gates + (L - 1), ldg, dmn, scale, g, chunks,
                                                                     du + (L - 1) * n);
    int64_t woff[kFmMaxL + 1] = {0};
    for (int l = 0; l < L; ++l) woff[l + 1] = woff[l] + (window + 2 * l) * (window + 2 * l);
    for (int l = L - 1; l >= 0; --l) {
        const int K = window + 2 * l;
        FmConv a = {};
        a.x = du + l * n;
        a.ldx = C;
        a.w = w + woff[l] * C;
        a.flip = 1;
        if (l) {
            a.gate = gates + (l - 1);
            a.ldg = ldg;
            a.s = scale;
            a.dA = dA;
            a.uprev = u + (l - 1) * n;
            a.out = du + (l - 1) * n;
            a.ldo = C;
        } else {
            a.out = dctx0;
            a.ldo = ldd0;
        }
        fm_conv(K, a, g, s);
    }
    if (dw)      // (after dm has been read: the weight gradient's parts take the workspace over)
        for (int l = 0; l < L; ++l)
            fm_wgrad(window + 2 * l, du + l * n, l ? u + (l - 1) * n : ctx0, l ? C : ld0, l > 0, g, ws, dw + woff[l] * C, s);
    return msda::launched(__func__);
}

int msda_fmod_modulate_forward_bf16(const uint16_t *q, int64_t ldq, const uint16_t *mod, int64_t tokens, int C, uint16_t *out,
                                    msda_stream_t stream)
{
    if (!q || !mod || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!fm_stride(ldq, C)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {q, mod, out})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int64_t chunks = tokens * C / 8;
    fmod_product_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, (hipStream_t)stream>>>(q, ldq, mod, C, C, chunks, out, C);
    return msda::launched(__func__);
}

int msda_fmod_modulate_backward_bf16(const uint16_t *dout, const uint16_t *q, int64_t ldq, const uint16_t *mod, int64_t tokens, int C,
                                     uint16_t *dq, int64_t lddq, uint16_t *dmod, msda_stream_t stream)
{
    if (!dout || !q || !mod || !dq || !dmod) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ln_dims(tokens, C)) return msda::arg_fail(e, __func__);
    if (!fm_stride(ldq, C) || !fm_stride(lddq, C)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {dout, q, mod, dq, dmod})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = tokens * C / 8;
    fmod_product_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(dout, C, mod, C, C, chunks, dq, lddq);
    fmod_product_kernel<<<(unsigned)((chunks + 255) / 256), 256, 0, s>>>(dout, C, q, ldq, C, chunks, dmod, C);
    return msda::launched(__func__);
}

}  // extern "C"
