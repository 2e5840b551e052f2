// msda_repack.h -- every derived form of the trained parameters refreshed from the fp32 masters in ONE launch (include/richsem_msda.h:
// msda_repack*).
//
// The bf16 casts, lin256's fragment order, the feed-forward kernel's W2 order and the convolutions' forward and input-gradient packs are
// all destination-indexed gathers: an output element is one source element, at most multiplied by one fp32 scale, rounded to bf16.  The
// kernel walks a device job table as msda_optim.h walks its tensor table: one workgroup of kRepackThreads per chunk (at most
// MSDA_REPACK_CHUNK destination elements of ONE job), a thread writes 16 bytes of destination at a time (8 bf16, 4 fp32 for the copy
// kind) -- a plain vector store; the last unit of a job whose size is not a multiple of that is written element by element.
//
// The index maps restate those of lin256_pack_kernel (lin256_mfma.hip), pack_w2_kernel (ffn_mfma.hip) and conv_pack_kernel
// (conv_mfma.hip): those kernels stay as they are, and tests/test_gpu_repack.py holds the two bit-equal.  No atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/richsem_msda.h"
#include "mfma_common.h"

namespace msda {

constexpr int kRepackThreads = 256;

// The kernel gets its data pointers out of a table in memory, where the compiler cannot see an address space and would use flat loads
// and stores; every one of them is global memory.
typedef __attribute__((address_space(1))) const float rp_gfloat;
typedef __attribute__((address_space(1))) const f32x4 rp_gf32x4;
typedef __attribute__((address_space(1))) u32x4 rp_gu32x4;
typedef __attribute__((address_space(1))) uint16_t rp_gu16;
typedef __attribute__((address_space(1))) float rp_gfloat_w;
__device__ inline rp_gfloat *repack_global(const float *p) { return (rp_gfloat *)reinterpret_cast<uintptr_t>(p); }

// the segment that holds row (or flat element) `r` of the concatenation: its base pointer and `r` relative to its start; nullptr past
// the last segment (the zero padding)
__device__ inline rp_gfloat *repack_segment(const msda_repack_job &J, int r, int &local)
{
    rp_gfloat *base = nullptr;
    int start = 0;
    for (int s = 0; s < J.n_segs; ++s) {
        const int end = J.seg_end[s];
        if (r >= start && r < end) {
            base = repack_global(J.src[s]);
            local = r - start;
        }
        start = end;
    }
    return base;
}

// four consecutive floats of a row-major run at `p` (nullptr: zeros): one 16-byte load where the address allows it
__device__ inline void repack_load4(rp_gfloat *p, float *v)
{
    if (!p) {
        v[0] = v[1] = v[2] = v[3] = 0.f;
    } else if (((uintptr_t)p & 15) == 0) {
        const f32x4 x = *(rp_gf32x4 *)(uintptr_t)p;
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
        v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    }
}

// four consecutive elements from flat element `e` (a multiple of 4) of the concatenation of the job's segments, zero past its end
__device__ inline void repack_flat4(const msda_repack_job &J, int e, float *v)
{
    int l0 = 0, l3 = 0;
    rp_gfloat *p0 = repack_segment(J, e, l0), *p3 = repack_segment(J, e + 3, l3);
    if (p0 && p0 == p3 && l3 == l0 + 3) {
        repack_load4(p0 + l0, v);
        return;
    }
    for (int j = 0; j < 4; ++j) {      // a segment boundary or the end of the data inside the four
        int l = 0;
        rp_gfloat *p = repack_segment(J, e + j, l);
        v[j] = p ? p[l] : 0.f;
    }
}

// ---- the index maps: v[0..7] = the eight consecutive destination elements from i0 (a multiple of 8) -----------------------------------
__device__ inline void repack_unit_cast(const msda_repack_job &J, long long i0, float *v)
{
    repack_flat4(J, (int)i0, v);
    repack_flat4(J, (int)i0 + 4, v + 4);
}

// lin256_pack_kernel's order: packed[block][k-step][tile u][lane][8]; lane (r = 4 q' + i, q) of tile u = output channel
// 64 block + 16 q' + 4 u + i, input channels 32 step + 8 q + 0..7
__device__ inline void repack_lin256_coords(long long i0, int &ch, int &k0)
{
    const int lane = (int)((i0 >> 3) & 63), u = (int)((i0 >> 9) & 3), s = (int)((i0 >> 11) & 7), blk = (int)(i0 >> 14);
    const int r = lane & 15, q = lane >> 4;
    ch = 64 * blk + 16 * (r >> 2) + 4 * u + (r & 3);
    k0 = 32 * s + 8 * q;
}

// of the (N x 256) concatenation (rows past its end are zero)
__device__ inline void repack_unit_lin256(const msda_repack_job &J, long long i0, float *v)
{
    int ch, k0, local = 0;
    repack_lin256_coords(i0, ch, k0);
    rp_gfloat *base = repack_segment(J, ch, local);
    rp_gfloat *p = base ? base + (long long)local * 256 + k0 : nullptr;
    repack_load4(p, v);
    repack_load4(p ? p + 4 : nullptr, v + 4);
}

// of the transpose of a (256 x N) source: destination (ch, k) = source row k, column ch
__device__ inline void repack_unit_lin256_t(const msda_repack_job &J, long long i0, float *v)
{
    int ch, k0;
    repack_lin256_coords(i0, ch, k0);
    const int N = J.dims[0];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        int local = 0;
        rp_gfloat *base = repack_segment(J, k0 + j, local);
        v[j] = base ? base[(long long)local * N + ch] : 0.f;
    }
}

// pack_w2_kernel's order: inside every 32 hidden columns, position 8 q + j holds column 4 q + j (j < 4) or 16 + 4 q + (j - 4)
__device__ inline void repack_unit_w2(const msda_repack_job &J, long long i0, float *v)
{
    const int q = (int)(i0 & 31) >> 3;
    const int b = (int)(i0 & ~31ll);
    repack_flat4(J, b + 4 * q, v);
    repack_flat4(J, b + 16 + 4 * q, v + 4);
}

__device__ inline int repack_conv_group(int rows)
{
    const int tiles = rows / 16;
    return tiles % 4 == 0 ? 4 : (tiles % 2 == 0 ? 2 : 1);
}

// conv_pack_kernel's order for a logical weight of `rows` output and `cin` input channels: packed[k-step][row tile][lane][8], flat
// k = (kh KW + kw) cin + ci, zero from K = KH KW cin on; inside every group of G row tiles, row 4 q + i of tile u is channel
// q (4 G) + 4 u + i of the group; with cin % 64 == 0 the k-steps go in pairs over 64 channels.
// TRANSPOSED = false: the logical weight is the source (Cout, Cin, KH, KW) itself.
// TRANSPOSED = true:  it is w_t[a][b][kh][kw] = source[b][a][KH - 1 - kh][KW - 1 - kw] * scale[b] (a < Cin, b < Cout), the fp32 product
//                     rounded to bf16 -- the weight of the input gradient.
template <bool TRANSPOSED>
__device__ inline void repack_unit_conv(const msda_repack_job &J, long long i0, float *v)
{
    const int Cout = J.dims[0], Cin = J.dims[1], KH = J.dims[2], KW = J.dims[3];
    const int rows = TRANSPOSED ? Cin : Cout, cin = TRANSPOSED ? Cout : Cin;
    const int tiles = rows / 16, K = KH * KW * cin, G = repack_conv_group(rows);
    const bool pairs = cin % 64 == 0;
    const int lane = (int)((i0 >> 3) & 63);
    const long long r = i0 >> 9;
    const int tile = (int)(r % tiles), s = (int)(r / tiles);
    const int row = lane & 15, q = lane >> 4;
    const int co = (tile / G) * 16 * G + (row >> 2) * 4 * G + 4 * (tile % G) + (row & 3);
    const int k0 = pairs ? 64 * (s >> 1) + 16 * q + 8 * (s & 1) : 32 * s + 8 * q;
    rp_gfloat *w = repack_global(J.src[0]);
    rp_gfloat *scale = repack_global(J.scale);
    const bool one_tap = cin % 8 == 0;      // k0 is a multiple of 8: the eight share their tap
    int ci = k0 % cin, tap = k0 / cin;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        if (!one_tap) {
            ci = k % cin;
            tap = k / cin;
        }
        float x = 0.f;
        if (k < K) {
            const int kh = tap / KW, kw = tap - kh * KW;
            if (TRANSPOSED)
                x = w[(((long long)ci * Cin + co) * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)] * scale[ci];
            else
                x = w[(((long long)co * Cin + ci) * KH + kh) * KW + kw];
        }
        v[j] = x;
        if (one_tap) ++ci;
    }
}

// one chunk of a bf16 destination: UNIT(job, first element, v) fills the eight values of a 16-byte unit
template <typename UNIT>
__device__ inline void repack_chunk_bf16(const msda_repack_job &J, const msda_repack_chunk &ck, UNIT unit)
{
    rp_gu16 *dst = (rp_gu16 *)reinterpret_cast<uintptr_t>(J.dst) + ck.offset;
    const int units = (ck.count + 7) >> 3;
    for (int u = threadIdx.x; u < units; u += kRepackThreads) {
        float v[8];
        unit(J, ck.offset + 8ll * u, v);
        const u32x4 packed = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
        const int left = ck.count - 8 * u;
        if (left >= 8) {
            *(rp_gu32x4 *)(uintptr_t)(dst + 8 * u) = packed;
        } else {      // the tail of a job whose size is no multiple of 8: nothing past its end is written
            for (int j = 0; j < left; ++j) dst[8 * u + j] = (uint16_t)((packed[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
        }
    }
}

// the fp32 copy: units of four
__device__ inline void repack_chunk_copy(const msda_repack_job &J, const msda_repack_chunk &ck)
{
    rp_gfloat_w *dst = (rp_gfloat_w *)reinterpret_cast<uintptr_t>(J.dst) + ck.offset;
    const int units = (ck.count + 3) >> 2;
    for (int u = threadIdx.x; u < units; u += kRepackThreads) {
        float v[4];
        repack_flat4(J, (int)ck.offset + 4 * u, v);
        const int left = ck.count - 4 * u;
        if (left >= 4) {
            *(__attribute__((address_space(1))) f32x4 *)(uintptr_t)(dst + 4 * u) = (f32x4){v[0], v[1], v[2], v[3]};
        } else {
            for (int j = 0; j < left; ++j) dst[4 * u + j] = v[j];
        }
    }
}

__global__ __launch_bounds__(kRepackThreads) void repack_kernel(const msda_repack_job *jobs, const msda_repack_chunk *chunks)
{
    const msda_repack_chunk ck = chunks[blockIdx.x];
    const msda_repack_job &J = jobs[ck.job];
    switch (J.kind) {
    case MSDA_REPACK_CAST: repack_chunk_bf16(J, ck, repack_unit_cast); break;
    case MSDA_REPACK_COPY: repack_chunk_copy(J, ck); break;
    case MSDA_REPACK_LIN256: repack_chunk_bf16(J, ck, repack_unit_lin256); break;
    case MSDA_REPACK_LIN256_T: repack_chunk_bf16(J, ck, repack_unit_lin256_t); break;
    case MSDA_REPACK_FFN_W2: repack_chunk_bf16(J, ck, repack_unit_w2); break;
    case MSDA_REPACK_CONV: repack_chunk_bf16(J, ck, repack_unit_conv<false>); break;
    case MSDA_REPACK_CONV_T: repack_chunk_bf16(J, ck, repack_unit_conv<true>); break;
    default: break;
    }
}

}  // namespace msda
