// swin_rows.h -- what the row-wise Swin kernels share (csrc/swin_block_mfma.hip: LayerNorm of general width; csrc/swin_stage.hip: the same
// norm where the backbone changes layout): the limits, eight bf16 <-> eight floats, the 64-lane sum, the last stage of dgamma / dbeta
// and the dimension check.  Internal; every translation unit that includes it gets its own copy (unnamed namespace).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"

namespace {

constexpr int kMaxC = 4096;         // LayerNorm
constexpr int kLnRows = 4;          // tokens (waves) per workgroup of the row kernels
constexpr int kPartRows = 64;       // tokens per partial row of dgamma / dbeta
constexpr int kColGroup = 128;      // channels per workgroup of the column kernel
constexpr int kLnChunks = kMaxC / 8 / 64;      // 16-byte chunks of a row per lane, at most

__device__ __forceinline__ void unpack8(u32x4 u, float (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = bf16_lo(u[i]);
        v[2 * i + 1] = bf16_hi(u[i]);
    }
}
__device__ __forceinline__ u32x4 pack8(const float (&v)[8])
{
    return (u32x4){pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// dgamma / dbeta = the partial rows workspace[(2 p + {0, 1}) C + channel], p = 0 .. parts - 1, added in ascending order
__global__ __launch_bounds__(256) void swin_ln_bwd_sum_kernel(const float *__restrict__ workspace, int parts, int C, float *__restrict__ dgamma,
                                                              float *__restrict__ dbeta)
{
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= C) return;
    float *dst = blockIdx.y ? dbeta : dgamma;
    if (!dst) return;
    const float *src = workspace + (size_t)blockIdx.y * C + ch;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += src[(size_t)p * 2 * C];
    dst[ch] = s;
}

int ln_dims(int64_t tokens, int C)
{
    if (tokens < 1 || C < 32 || C > kMaxC || C % 32) return MSDA_ERR_BAD_DIMS;
    if (tokens * C >= (int64_t)1 << 31) return MSDA_ERR_TOO_LARGE;
    return MSDA_OK;
}

}  // namespace
