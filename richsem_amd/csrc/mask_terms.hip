// mask_terms.hip -- the mask terms of the criterion and the mask post-processor ("Mask terms"): SetCriterion.loss_masks
// (reference models/richsem/richsem.py:1073-1100 with dice_loss / sigmoid_focal_loss of segmentation.py:168-211) forward and backward over
// capacity buffers, and PostProcessSegm.forward (segmentation.py:214-242).  C ABI msda_mask_* (include/richsem_msda.h).
//
// The contract.  pred (N, Q, h, w) fp32 or bf16, read as stored; target uint8 (cap, Hp, Wp) in target-slot order, Wp a multiple of 16; a slot s
// below offsets[N] with 0 <= query_of_target[s] < Q is a PAIR of image b (offsets[b] <= s < offsets[b + 1]) and query query_of_target[s].
// The resize is torch's bilinear one with align_corners = False: scale = in / out (fp32), source coordinate max(0, (dst + 0.5) scale - 0.5),
// i0 = floor, i1 = min(i0 + 1, in - 1), weights fp32.  All arithmetic fp32, the final sums fp64; no atomics, no allocation, no
// synchronisation, every reduction in a fixed order.  No buffer of the target resolution is written in float: the resized logit lives in a
// register, the per-pixel gradient factor in an LDS tile of four canvas rows.
//
//   x[y, x']   = bilinear(pred[b, q], y, x'),  p = sigmoid(x),  t = target[s, y, x']
//   focal      = a_t (softplus(x) - x t) (p + t - 2 p t)^2,  a_t = alpha t + (1 - alpha)(1 - t)  (alpha < 0: a_t = 1),  gamma = 2
//   sums[s]    = (sum focal, sum p t, sum p, sum t) over the Hp Wp pixels of the canvas
//   loss_mask  = sum_pairs (sums[0] / (Hp Wp)) / num_boxes,  loss_dice = sum_pairs (1 - (2 sums[1] + 1) / (sums[2] + sums[3] + 1)) / num_boxes
//   backward   G[y, x'] = g0 focal'(x, t) / (Hp Wp nb) + g1 dice'(p, t; sums) p (1 - p) / nb,
//              grad_pred[b, q, sy, sx] = sum_{y, x'} wy(y -> sy) wx(x' -> sx) G[y, x'],  y and x' ascending
//
// The cut.
//   mask_loss_fwd_kernel     a workgroup takes one slot and a band of 8 canvas rows: the source rows the band reads staged in LDS as fp32, a lane
//                            takes 16 pixels (one 16-byte read of the target) at a time, four running sums, the lanes of a wave by shuffles, the
//                            four waves in wave order: one partial row of 4 per workgroup.
//   mask_loss_sum_kernel     one workgroup: per slot the bands in ascending order in fp64 -> sums; the slots in ascending order -> the two losses.
//   mask_slot_map_kernel     slot_of_query (N, Q): the first pair of each query (-1: none), a thread per query scanning its image's slots.
//   mask_loss_bwd_kernel     a workgroup takes one (image, query) and a band of SR source rows (SR w <= 1024: up to 4 source pixels per lane).
//                            No pair: plain zero stores.  Else the source rows r0 - 1 .. r0 + SR staged in LDS; the canvas rows that touch the
//                            band (first_ge: closed form, then confirmed by recomputing the index) four at a time: G of the four rows into the
//                            LDS tile, then every lane adds wy wx G over the canvas columns that touch its source pixel.  One store per element.
//   mask_postprocess_kernel  a lane per 16 output bytes of the flat (rows, oh, ow) map of one image: nearest index into the cropped x4 map,
//                            bilinear value of that x4 pixel from the logits, fp32 sigmoid > threshold.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msda_host.h"

namespace {

constexpr int kMlBand = 8;            // canvas rows per forward workgroup
constexpr int kMlGRows = 4;           // canvas rows of the backward's LDS tile
constexpr int kMlMaxAcc = 4;          // source pixels per lane in the backward
constexpr int kMlMaxLds = 64 * 1024;  // dynamic LDS either kernel may ask for
constexpr int kMpMaxImages = 8;       // images per post-process launch

struct MlGeom {
    int N, Q, h, w, Hp, Wp, cap, bands;
    float sh, sw;      // h / Hp, w / Wp
};

__device__ __forceinline__ float ml_ld(const float *p) { return *p; }
__device__ __forceinline__ float ml_ld(const uint16_t *p) { return __uint_as_float((unsigned)*p << 16); }
__device__ __forceinline__ void ml_st(float *p, float v) { *p = v; }
__device__ __forceinline__ void ml_st(uint16_t *p, float v)      // round to nearest even
{
    const unsigned u = __float_as_uint(v);
    *p = (v != v) ? (uint16_t)0x7fc0 : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ float ml_src(int dst, float scale)
{
    const float s = ((float)dst + 0.5f) * scale - 0.5f;
    return s < 0.f ? 0.f : s;
}
__device__ __forceinline__ int ml_i0(float src, int in) { return min((int)src, in - 1); }

// the first dst in [0, n] whose i0 is >= v (n: none).  i0 never decreases with dst, so the closed form only has to land near it: the two
// loops move it to where the recomputed index says it is.
__device__ __forceinline__ int ml_first_ge(int v, float scale, int in, int n)
{
    if (v <= 0) return 0;
    if (v > in - 1) return n;
    int y = (int)ceilf(((float)v + 0.5f) / scale - 0.5f);
    y = max(0, min(y, n));
    while (y > 0 && ml_i0(ml_src(y - 1, scale), in) >= v) --y;
    while (y < n && ml_i0(ml_src(y, scale), in) < v) ++y;
    return y;
}

__device__ __forceinline__ bool ml_pair(const int64_t *__restrict__ offsets, const int64_t *__restrict__ qot, int N, int Q, int cap, int s, int &b,
                                        int &q)
{
    const int64_t live = min(offsets[N], (int64_t)cap);
    if (s >= live) return false;
    const int64_t qq = qot[s];
    if (qq < 0 || qq >= Q) return false;
    b = 0;
    while (b + 1 < N && offsets[b + 1] <= s) ++b;
    q = (int)qq;
    return true;
}

// e = exp(-|x|), p = sigmoid(x), softplus(x) = max(x, 0) + log1p(e)
__device__ __forceinline__ void ml_sigmoid(float x, float &e, float &p)
{
    e = expf(-fabsf(x));
    const float inv = 1.f / (1.f + e);
    p = x >= 0.f ? inv : e * inv;
}

template <typename T>
__global__ __launch_bounds__(256) void mask_loss_fwd_kernel(const T *__restrict__ pred, const uint8_t *__restrict__ target,
                                                            const int64_t *__restrict__ offsets, const int64_t *__restrict__ qot, float alpha,
                                                            MlGeom g, int max_rows, float *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) float ml_rows[];
    __shared__ float red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x / g.bands, band = blockIdx.x - s * g.bands;
    float *out = partial + (size_t)blockIdx.x * 4;
    int b, q;
    if (!ml_pair(offsets, qot, g.N, g.Q, g.cap, s, b, q)) {      // (the same for every lane)
        if (tid < 4) out[tid] = 0.f;
        return;
    }
    const int y0 = band * kMlBand;
    const int lo = ml_i0(ml_src(y0, g.sh), g.h), nrows = min(max_rows, g.h - lo);
    const T *src = pred + ((size_t)b * g.Q + q) * g.h * g.w + (size_t)lo * g.w;
    for (int i = tid; i < nrows * g.w; i += 256) ml_rows[i] = ml_ld(src + i);
    __syncthreads();
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int ppr = g.Wp >> 4, rows = min(kMlBand, g.Hp - y0);
    for (int id = tid; id < rows * ppr; id += 256) {
        const int ry = id / ppr, x0 = (id - ry * ppr) << 4, y = y0 + ry;
        const float sy = ml_src(y, g.sh);
        const int iy0 = ml_i0(sy, g.h), iy1 = min(iy0 + 1, g.h - 1);
        const float ly = sy - (float)iy0, hy = 1.f - ly;
        const float *r0 = ml_rows + min(iy0 - lo, nrows - 1) * g.w, *r1 = ml_rows + min(iy1 - lo, nrows - 1) * g.w;
        const uint4 tv = *reinterpret_cast<const uint4 *>(target + ((size_t)s * g.Hp + y) * g.Wp + x0);
        const unsigned tw[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float sx = ml_src(x0 + j, g.sw);
            const int ix0 = ml_i0(sx, g.w), ix1 = min(ix0 + 1, g.w - 1);
            const float lx = sx - (float)ix0, hx = 1.f - lx;
            const float x = hy * (hx * r0[ix0] + lx * r0[ix1]) + ly * (hx * r1[ix0] + lx * r1[ix1]);
            const float t = (float)((tw[j >> 2] >> (8 * (j & 3))) & 0xffu);
            float e, p;
            ml_sigmoid(x, e, p);
            const float ce = fmaxf(x, 0.f) - x * t + log1pf(e), m = p + t - 2.f * p * t;
            const float at = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
            acc[0] += at * ce * m * m;
            acc[1] += p * t;
            acc[2] += p;
            acc[3] += t;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float v = acc[k];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (tid < 4) out[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(256) void mask_loss_sum_kernel(const float *__restrict__ partial, const int64_t *__restrict__ offsets,
                                                            const int64_t *__restrict__ qot, const float *__restrict__ num_boxes, MlGeom g,
                                                            float *__restrict__ sums, float *__restrict__ losses)
{
    __shared__ double part[2][256];
    const int tid = threadIdx.x;
    const double area = (double)g.Hp * (double)g.Wp;
    double focal = 0.0, dice = 0.0;
    for (int s = tid; s < g.cap; s += 256) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        int b, q;
        if (ml_pair(offsets, qot, g.N, g.Q, g.cap, s, b, q)) {
            const float *p = partial + (size_t)s * g.bands * 4;
            for (int band = 0; band < g.bands; ++band)
                for (int k = 0; k < 4; ++k) v[k] += (double)p[band * 4 + k];
            focal += v[0] / area;
            dice += 1.0 - (2.0 * v[1] + 1.0) / (v[2] + v[3] + 1.0);
        }
        for (int k = 0; k < 4; ++k) sums[(size_t)s * 4 + k] = (float)v[k];
    }
    part[0][tid] = focal;
    part[1][tid] = dice;
    __syncthreads();
    if (tid < 2) {
        double a = 0.0;
        for (int i = 0; i < 256; ++i) a += part[tid][i];
        losses[tid] = (float)(a / (double)num_boxes[0]);
    }
}

__global__ __launch_bounds__(256) void mask_slot_map_kernel(const int64_t *__restrict__ offsets, const int64_t *__restrict__ qot, MlGeom g,
                                                            int *__restrict__ slot_of_query)
{
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= g.N * g.Q) return;
    const int b = id / g.Q, q = id - b * g.Q;
    const int64_t live = min(offsets[g.N], (int64_t)g.cap);
    const int64_t s0 = max(offsets[b], (int64_t)0), s1 = min(offsets[b + 1], live);
    int found = -1;
    for (int64_t s = s0; s < s1; ++s)
        if (qot[s] == q) {
            found = (int)s;
            break;
        }
    slot_of_query[id] = found;
}

template <typename T>
__global__ __launch_bounds__(256) void mask_loss_bwd_kernel(const T *__restrict__ pred, const uint8_t *__restrict__ target,
                                                            const int *__restrict__ slot_of_query, const float *__restrict__ sums,
                                                            const float *__restrict__ num_boxes, const float *__restrict__ gl, float alpha,
                                                            MlGeom g, int SR, int sbands, T *__restrict__ grad)
{
    extern __shared__ __attribute__((aligned(16))) float ml_bwd[];
    const int tid = threadIdx.x;
    const int nq = blockIdx.x / sbands, band = blockIdx.x - nq * sbands;
    const int r0 = band * SR, nr = min(SR, g.h - r0), elems = nr * g.w;
    T *gout = grad + ((size_t)nq * g.h + r0) * g.w;
    const int s = slot_of_query[nq];
    if (s < 0) {      // (the same for every lane)
        for (int i = tid; i < elems; i += 256) ml_st(gout + i, 0.f);
        return;
    }
    const int lo = max(r0 - 1, 0), hi = min(r0 + nr, g.h - 1), nst = hi - lo + 1;
    float *rows = ml_bwd, *G = ml_bwd + (size_t)(SR + 2) * g.w;
    const T *src = pred + ((size_t)nq * g.h + lo) * g.w;
    for (int i = tid; i < nst * g.w; i += 256) rows[i] = ml_ld(src + i);
    // the canvas rows y with r0 - 1 <= i0(y) <= r0 + nr - 1: the ones that touch a source row of the band
    const int Ya = ml_first_ge(r0 - 1, g.sh, g.h, g.Hp), Yb = ml_first_ge(r0 + nr, g.sh, g.h, g.Hp) - 1;
    int esr[kMlMaxAcc], esx[kMlMaxAcc], xa[kMlMaxAcc], xb[kMlMaxAcc];
    float acc[kMlMaxAcc];
#pragma unroll
    for (int k = 0; k < kMlMaxAcc; ++k) {
        const int e = tid + 256 * k;
        acc[k] = 0.f;
        esr[k] = -2;      // (matches no index)
        esx[k] = 0;
        xa[k] = 0;
        xb[k] = -1;
        if (e < elems) {
            esr[k] = r0 + e / g.w;
            esx[k] = e % g.w;
            xa[k] = ml_first_ge(esx[k] - 1, g.sw, g.w, g.Wp);
            xb[k] = ml_first_ge(esx[k] + 1, g.sw, g.w, g.Wp) - 1;
        }
    }
    const float nb = num_boxes[0], c0 = gl[0] / ((float)g.Hp * (float)g.Wp * nb), c1 = gl[1] / nb;
    const float *sm = sums + (size_t)s * 4;
    const float num = 2.f * sm[1] + 1.f, den = sm[2] + sm[3] + 1.f, inv_den2 = 1.f / (den * den);
    const int ppr = g.Wp >> 4;
    const uint8_t *tgt = target + (size_t)s * g.Hp * g.Wp;
    for (int yt = Ya; yt <= Yb; yt += kMlGRows) {
        const int trows = min(kMlGRows, Yb - yt + 1);
        __syncthreads();      // the staged rows are in place (first round); the tile's previous rows have been read (later rounds)
        for (int id = tid; id < trows * ppr; id += 256) {
            const int ry = id / ppr, x0 = (id - ry * ppr) << 4, y = yt + ry;
            const float sy = ml_src(y, g.sh);
            const int iy0 = ml_i0(sy, g.h), iy1 = min(iy0 + 1, g.h - 1);
            const float ly = sy - (float)iy0, hy = 1.f - ly;
            const float *q0 = rows + max(0, min(iy0 - lo, nst - 1)) * g.w, *q1 = rows + max(0, min(iy1 - lo, nst - 1)) * g.w;
            const uint4 tv = *reinterpret_cast<const uint4 *>(tgt + (size_t)y * g.Wp + x0);
            const unsigned tw[4] = {tv.x, tv.y, tv.z, tv.w};
            float *Grow = G + ry * g.Wp + x0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float sx = ml_src(x0 + j, g.sw);
                const int ix0 = ml_i0(sx, g.w), ix1 = min(ix0 + 1, g.w - 1);
                const float lx = sx - (float)ix0, hx = 1.f - lx;
                const float x = hy * (hx * q0[ix0] + lx * q0[ix1]) + ly * (hx * q1[ix0] + lx * q1[ix1]);
                const float t = (float)((tw[j >> 2] >> (8 * (j & 3))) & 0xffu);
                float e, p;
                ml_sigmoid(x, e, p);
                const float ce = fmaxf(x, 0.f) - x * t + log1pf(e), m = p + t - 2.f * p * t, pq = p * (1.f - p);
                const float at = alpha >= 0.f ? alpha * t + (1.f - alpha) * (1.f - t) : 1.f;
                // d/dx of a_t ce m^2: ce' = p - t, m' = (1 - 2 t) p (1 - p)
                const float dfocal = at * m * ((p - t) * m + 2.f * ce * (1.f - 2.f * t) * pq);
                // d/dp of 1 - num / den: -(2 t den - num) / den^2
                const float ddice = -(2.f * t * den - num) * inv_den2 * pq;
                Grow[j] = c0 * dfocal + c1 * ddice;
            }
        }
        __syncthreads();
        for (int ry = 0; ry < trows; ++ry) {
            const float sy = ml_src(yt + ry, g.sh);
            const int iy0 = ml_i0(sy, g.h), iy1 = min(iy0 + 1, g.h - 1);
            const float ly = sy - (float)iy0;
            const float *Grow = G + ry * g.Wp;
#pragma unroll
            for (int k = 0; k < kMlMaxAcc; ++k) {
                if (iy0 != esr[k] && iy1 != esr[k]) continue;
                const float wy = (iy0 == esr[k] ? 1.f - ly : 0.f) + (iy1 == esr[k] ? ly : 0.f);
                float hsum = 0.f;
                for (int x = xa[k]; x <= xb[k]; ++x) {
                    const float sx = ml_src(x, g.sw);
                    const int ix0 = ml_i0(sx, g.w), ix1 = min(ix0 + 1, g.w - 1);
                    const float lx = sx - (float)ix0;
                    const float wx = (ix0 == esx[k] ? 1.f - lx : 0.f) + (ix1 == esx[k] ? lx : 0.f);
                    hsum += wx * Grow[x];
                }
                acc[k] += wy * hsum;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kMlMaxAcc; ++k) {
        const int e = tid + 256 * k;
        if (e < elems) ml_st(gout + e, acc[k]);
    }
}

struct MpImage {
    const int64_t *items;      // rows int64 on the device, or nullptr: rows 0 .. rows - 1
    uint8_t *out;              // (rows, 1, oh, ow)
    int n, rows, ch, cw, oh, ow;
    int64_t bytes;             // rows oh ow
};
struct MpImages {
    MpImage im[kMpMaxImages];
};

template <typename T>
__global__ __launch_bounds__(256) void mask_postprocess_kernel(const T *__restrict__ pred, int Q, int h, int w, float threshold, MpImages imgs)
{
    const MpImage &im = imgs.im[blockIdx.y];
    const int64_t c0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (c0 >= im.bytes) return;
    const int64_t plane = (int64_t)im.oh * im.ow;
    int r = (int)(c0 / plane);
    const int64_t rem = c0 - (int64_t)r * plane;
    int oy = (int)(rem / im.ow), ox = (int)(rem - (int64_t)oy * im.ow);
    const float ny = (float)im.ch / (float)im.oh, nx = (float)im.cw / (float)im.ow;
    const int count = (int)min((int64_t)16, im.bytes - c0);
    unsigned packed[4] = {0u, 0u, 0u, 0u};
    const T *map = nullptr;
    int cur = -1;
    for (int j = 0; j < count; ++j) {
        if (r != cur) {
            int64_t row = im.items ? im.items[r] : (int64_t)r;
            if (row < 0) row += Q;      // (an index from the end, as torch's indexing takes it)
            row = max((int64_t)0, min(row, (int64_t)Q - 1));
            map = pred + ((size_t)im.n * Q + (size_t)row) * h * w;
            cur = r;
        }
        // torch's nearest rule, then the x4 map's bilinear pixel
        const int Y = min((int)floorf((float)oy * ny), im.ch - 1), X = min((int)floorf((float)ox * nx), im.cw - 1);
        const float sy = ml_src(Y, 0.25f), sx = ml_src(X, 0.25f);
        const int iy0 = ml_i0(sy, h), iy1 = min(iy0 + 1, h - 1), ix0 = ml_i0(sx, w), ix1 = min(ix0 + 1, w - 1);
        const float ly = sy - (float)iy0, hy = 1.f - ly, lx = sx - (float)ix0, hx = 1.f - lx;
        const T *q0 = map + (size_t)iy0 * w, *q1 = map + (size_t)iy1 * w;
        const float x = hy * (hx * ml_ld(q0 + ix0) + lx * ml_ld(q0 + ix1)) + ly * (hx * ml_ld(q1 + ix0) + lx * ml_ld(q1 + ix1));
        const float p = 1.f / (1.f + expf(-x));
        packed[j >> 2] |= (p > threshold ? 1u : 0u) << (8 * (j & 3));
        if (++ox == im.ow) {
            ox = 0;
            if (++oy == im.oh) {
                oy = 0;
                ++r;
            }
        }
    }
    if (count == 16) {
        *reinterpret_cast<uint4 *>(im.out + c0) = make_uint4(packed[0], packed[1], packed[2], packed[3]);
    } else {
        for (int j = 0; j < count; ++j) im.out[c0 + j] = (uint8_t)((packed[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct MlPlan {
    MlGeom g;
    int max_rows, SR, sbands;
    size_t fwd_lds, bwd_lds;
    int64_t partial_bytes, map_bytes;
};

int ml_plan(int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, MlPlan *p)
{
    if (N < 1 || Q < 1 || h < 1 || w < 1 || Hp < 1 || Wp < 16 || Wp % 16 || cap < 1) return MSDA_ERR_BAD_DIMS;
    if (w > 256 * kMlMaxAcc || cap > (1 << 24) || Hp > (1 << 20) || Wp > (1 << 20)) return MSDA_ERR_TOO_LARGE;
    if ((int64_t)N * Q * h * w >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    MlGeom &g = p->g;
    g = MlGeom{N, Q, h, w, Hp, Wp, (int)cap, (Hp + kMlBand - 1) / kMlBand, (float)h / (float)Hp, (float)w / (float)Wp};
    if (cap * g.bands >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    // a band's rows reach from i0 of its first row to i1 of its last: at most 7 scale + 3 source rows
    const int64_t mr = (int64_t)((double)kMlBand * (double)h / (double)Hp) + 3;
    p->max_rows = (int)(mr < h ? mr : h);
    p->fwd_lds = (size_t)p->max_rows * w * sizeof(float);
    p->SR = 256 * kMlMaxAcc / w < kMlMaxAcc ? 256 * kMlMaxAcc / w : kMlMaxAcc;
    if (p->SR > h) p->SR = h;
    p->sbands = (h + p->SR - 1) / p->SR;
    p->bwd_lds = ((size_t)(p->SR + 2) * w + (size_t)kMlGRows * Wp) * sizeof(float);
    if (p->fwd_lds > (size_t)kMlMaxLds || p->bwd_lds > (size_t)kMlMaxLds) return MSDA_ERR_TOO_LARGE;
    if ((int64_t)N * Q * p->sbands >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    p->partial_bytes = ((cap * g.bands * 4 * (int64_t)sizeof(float)) + 255) / 256 * 256;
    p->map_bytes = (int64_t)N * Q * (int64_t)sizeof(int);
    return MSDA_OK;
}

template <typename T>
int ml_forward(const char *fn, const T *pred, const uint8_t *target, const int64_t *offsets, const int64_t *qot, const float *num_boxes, int N,
               int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, float *losses, float *sums, void *workspace, msda_stream_t stream)
{
    MlPlan p;
    if (!pred || !target || !offsets || !qot || !num_boxes || !losses || !sums || !workspace) return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
    if (const int e = ml_plan(N, Q, h, w, Hp, Wp, cap, &p)) return msda::arg_fail(e, fn);
    if (!msda::aligned(16, {target, workspace}) || !msda::aligned(8, {offsets, qot}) || !msda::aligned(4, {num_boxes, losses, sums}) ||
        !msda::aligned(sizeof(T), {pred}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    hipStream_t s = (hipStream_t)stream;
    float *partial = static_cast<float *>(workspace);
    mask_loss_fwd_kernel<T><<<(unsigned)(cap * p.g.bands), 256, p.fwd_lds, s>>>(pred, target, offsets, qot, alpha, p.g, p.max_rows, partial);
    mask_loss_sum_kernel<<<1, 256, 0, s>>>(partial, offsets, qot, num_boxes, p.g, sums, losses);
    return msda::launched(fn);
}

template <typename T>
int ml_backward(const char *fn, const T *pred, const uint8_t *target, const int64_t *offsets, const int64_t *qot, const float *num_boxes,
                const float *sums, const float *g, int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, T *grad_pred,
                void *workspace, msda_stream_t stream)
{
    MlPlan p;
    if (!pred || !target || !offsets || !qot || !num_boxes || !sums || !g || !grad_pred || !workspace)
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
    if (const int e = ml_plan(N, Q, h, w, Hp, Wp, cap, &p)) return msda::arg_fail(e, fn);
    if (!msda::aligned(16, {target, workspace}) || !msda::aligned(8, {offsets, qot}) || !msda::aligned(4, {num_boxes, sums, g}) ||
        !msda::aligned(sizeof(T), {pred, grad_pred}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    hipStream_t s = (hipStream_t)stream;
    int *map = reinterpret_cast<int *>(static_cast<char *>(workspace) + p.partial_bytes);
    mask_slot_map_kernel<<<(unsigned)((N * Q + 255) / 256), 256, 0, s>>>(offsets, qot, p.g, map);
    mask_loss_bwd_kernel<T><<<(unsigned)((int64_t)N * Q * p.sbands), 256, p.bwd_lds, s>>>(pred, target, map, sums, num_boxes, g, alpha, p.g, p.SR,
                                                                                           p.sbands, grad_pred);
    return msda::launched(fn);
}

template <typename T>
int mp_run(const char *fn, const T *pred, int N, int Q, int h, int w, const int64_t *const *item_indices, const int *rows, const int *sizes,
           float threshold, uint8_t *const *out, msda_stream_t stream)
{
    if (!pred || !rows || !sizes || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
    if (N < 1 || Q < 1 || h < 1 || w < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, fn);
    if (h > (1 << 20) || w > (1 << 20) || (int64_t)N * Q * h * w >= (int64_t)1 << 31) return msda::arg_fail(MSDA_ERR_TOO_LARGE, fn);
    if (!msda::aligned(sizeof(T), {pred})) return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    for (int n = 0; n < N; ++n) {
        const int *sz = sizes + 4 * n;
        if (rows[n] < 0 || sz[0] < 1 || sz[1] < 1 || sz[2] < 1 || sz[3] < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, fn);
        if (rows[n] && !out[n]) return msda::arg_fail(MSDA_ERR_NULL_POINTER, fn);
        if ((int64_t)rows[n] * sz[2] * sz[3] >= (int64_t)1 << 40) return msda::arg_fail(MSDA_ERR_TOO_LARGE, fn);
        if (!msda::aligned(16, {out[n]}) || (item_indices && !msda::aligned(8, {item_indices[n]}))) return msda::arg_fail(MSDA_ERR_MISALIGNED, fn);
    }
    for (int n0 = 0; n0 < N; n0 += kMpMaxImages) {
        MpImages imgs = {};
        const int cnt = N - n0 < kMpMaxImages ? N - n0 : kMpMaxImages;
        int64_t most = 0;
        for (int i = 0; i < cnt; ++i) {
            const int n = n0 + i, *sz = sizes + 4 * n;
            MpImage &im = imgs.im[i];
            im.items = item_indices ? item_indices[n] : nullptr;
            im.out = out[n];
            im.n = n;
            im.rows = rows[n];
            im.ch = sz[0] < 4 * h ? sz[0] : 4 * h;
            im.cw = sz[1] < 4 * w ? sz[1] : 4 * w;
            im.oh = sz[2];
            im.ow = sz[3];
            im.bytes = (int64_t)rows[n] * sz[2] * sz[3];
            if (im.bytes > most) most = im.bytes;
        }
        if (!most) continue;
        const int64_t blocks = (most + 16 * 256 - 1) / (16 * 256);
        if (blocks >= (int64_t)1 << 31) return msda::arg_fail(MSDA_ERR_TOO_LARGE, fn);
        mask_postprocess_kernel<T><<<dim3((unsigned)blocks, (unsigned)cnt), 256, 0, (hipStream_t)stream>>>(pred, Q, h, w, threshold, imgs);
    }
    return msda::launched(fn);
}

}  // namespace

extern "C" {

int msda_mask_loss_workspace_bytes(int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, int64_t *bytes)
{
    MlPlan p;
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = ml_plan(N, Q, h, w, Hp, Wp, cap, &p)) return msda::arg_fail(e, __func__);
    *bytes = p.partial_bytes + p.map_bytes;
    return MSDA_OK;
}

int msda_mask_loss_forward_f32(const float *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                               const float *num_boxes, int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, float *losses,
                               float *pair_sums, void *workspace, msda_stream_t stream)
{
    return ml_forward(__func__, pred, target, offsets, query_of_target, num_boxes, N, Q, h, w, Hp, Wp, cap, alpha, losses, pair_sums, workspace, stream);
}

int msda_mask_loss_forward_bf16(const uint16_t *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                const float *num_boxes, int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, float *losses,
                                float *pair_sums, void *workspace, msda_stream_t stream)
{
    return ml_forward(__func__, pred, target, offsets, query_of_target, num_boxes, N, Q, h, w, Hp, Wp, cap, alpha, losses, pair_sums, workspace, stream);
}

int msda_mask_loss_backward_f32(const float *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                const float *num_boxes, const float *pair_sums, const float *g, int N, int Q, int h, int w, int Hp, int Wp,
                                int64_t cap, float alpha, float *grad_pred, void *workspace, msda_stream_t stream)
{
    return ml_backward(__func__, pred, target, offsets, query_of_target, num_boxes, pair_sums, g, N, Q, h, w, Hp, Wp, cap, alpha, grad_pred, workspace,
                       stream);
}

int msda_mask_loss_backward_bf16(const uint16_t *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                 const float *num_boxes, const float *pair_sums, const float *g, int N, int Q, int h, int w, int Hp, int Wp,
                                 int64_t cap, float alpha, uint16_t *grad_pred, void *workspace, msda_stream_t stream)
{
    return ml_backward(__func__, pred, target, offsets, query_of_target, num_boxes, pair_sums, g, N, Q, h, w, Hp, Wp, cap, alpha, grad_pred, workspace,
                       stream);
}

int msda_mask_postprocess_f32(const float *pred, int N, int Q, int h, int w, const int64_t *const *item_indices, const int *rows, const int *sizes,
                              float threshold, uint8_t *const *out, msda_stream_t stream)
{
    return mp_run(__func__, pred, N, Q, h, w, item_indices, rows, sizes, threshold, out, stream);
}

int msda_mask_postprocess_bf16(const uint16_t *pred, int N, int Q, int h, int w, const int64_t *const *item_indices, const int *rows,
                               const int *sizes, float threshold, uint8_t *const *out, msda_stream_t stream)
{
    return mp_run(__func__, pred, N, Q, h, w, item_indices, rows, sizes, threshold, out, stream);
}

}  // extern "C"
