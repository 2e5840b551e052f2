// mfma_common.h -- the device prelude the bf16 MFMA translation units share (lin256 / cls / ffn / conv / attn / conv_wgrad): vector
// types, bf16 packing, the operand-fragment size and the inline LDS reads the hand-scheduled kernels issue.  Per-kernel constants
// (kD, kTokWave, kWaves, ...) stay with their kernels.
#pragma once

#include <hip/hip_runtime.h>

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

constexpr int kFragShorts = 512;   // one MFMA operand fragment: 64 lanes x 8 bf16

__device__ __forceinline__ unsigned pack_bf16(float a, float b)   // one v_cvt_pk_bf16_f32 (round to nearest even)
{
    const bf16x2_t p = __builtin_convertvector((f32x2_t){a, b}, bf16x2_t);
    return __builtin_bit_cast(unsigned, p);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }

// one operand fragment from LDS, not visible to the compiler's wait-count bookkeeping (a __syncthreads, or any LDS read the compiler can
// see, waits for every LDS DMA in flight)
#define MFMA_LDS_READ(dst, addr, byte_off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(byte_off))
// "at most n LDS reads still in flight": everything older has arrived.  The operand ties the fragment to the wait.
#define MFMA_LDS_WAIT(n, a) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(n))
