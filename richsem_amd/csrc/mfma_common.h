// mfma_common.h -- the device prelude the bf16 MFMA translation units share (lin256 / cls / ffn / conv / attn / conv_wgrad): vector
// types, bf16 packing and the fp32 -> bf16 hi + lo split, the register stager of a packed operand, the x fragments of a wave that owns
// 48 tokens of a 256-wide input, the lane-group reductions, the LDS-DMA request and the inline LDS reads and partial waits the
// hand-scheduled kernels issue.  Every helper here has at least two kernels using it and leaves their instructions as they were when
// the code was written out (tools/kernel_isa_diff.py, profiles/r11_device_helpers.md).  Per-kernel constants (kD, kTokWave, kWaves, ring
// sizes, ...) stay with their kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

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

// four consecutive bf16 <-> four floats, eight floats -> one operand fragment
__device__ __forceinline__ f32x4 unpack_bf16x4(uint2 u) { return (f32x4){bf16_lo(u.x), bf16_hi(u.x), bf16_lo(u.y), bf16_hi(u.y)}; }
__device__ __forceinline__ uint2 pack_bf16x4(f32x4 v) { return make_uint2(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3])); }
__device__ __forceinline__ bf16x8 pack_bf16x8(const float (&p)[8])
{
    const unsigned u0 = pack_bf16(p[0], p[1]), u1 = pack_bf16(p[2], p[3]), u2 = pack_bf16(p[4], p[5]), u3 = pack_bf16(p[6], p[7]);
    return __builtin_bit_cast(bf16x8, (u32x4){u0, u1, u2, u3});
}

// fp32 -> bf16 hi + lo parts (hi = bf16(v), lo = bf16(v - hi), both rounded to nearest even): hi.hi + lo.hi + hi.lo products with fp32
// accumulation are exact to fp32 level (the dropped lo.lo term is 2^-18 relative).  One element (the pack kernels) ...
struct Bf16Split {
    uint16_t hi, lo;
};
__device__ __forceinline__ Bf16Split split_bf16(float v)
{
    const unsigned hi = pack_bf16(v, 0.f) & 0xFFFFu;
    const unsigned lo = pack_bf16(v - __uint_as_float(hi << 16), 0.f) & 0xFFFFu;
    return {(uint16_t)hi, (uint16_t)lo};
}
// ... and the eight consecutive floats at `p` (16-byte aligned) as one operand fragment of each part
__device__ __forceinline__ void split_bf16x8(const float *p, bf16x8 &hi, bf16x8 &lo)
{
    const float4 a = *reinterpret_cast<const float4 *>(p), b = *reinterpret_cast<const float4 *>(p + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = pack_bf16(v[2 * i], v[2 * i + 1]);
        l[i] = pack_bf16(v[2 * i] - bf16_lo(h[i]), v[2 * i + 1] - bf16_hi(h[i]));
    }
    hi = __builtin_bit_cast(bf16x8, h);
    lo = __builtin_bit_cast(bf16x8, l);
}

// The x fragments (B operand) of a wave that owns the 48 tokens from tok0 of a 256-wide row-major input: lane (c, q) holds
// x[tok0 + 16 t + c][32 s + 8 q + 0..7] in xf[t][s]; rows past the end are clamped to T - 1 (their results are never stored).
constexpr int kXfWidth = 256;
__device__ __forceinline__ void load_x_frags(const uint16_t *x, int tok0, int T, int c, int q, bf16x8 (&xf)[3][8])
{
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const uint16_t *row = x + (size_t)min(tok0 + 16 * t + c, T - 1) * kXfWidth + 8 * q;
#pragma unroll
        for (int s = 0; s < 8; ++s) xf[t][s] = *reinterpret_cast<const bf16x8 *>(row + 32 * s);
    }
}
// (an fp32 input goes row by row through split_bf16x8 in the kernel's own loops: a whole-wave form of it renumbers the registers of
// cls_score_kernel<true, *>)

// Memory -> registers -> LDS for one block of a packed operand (CHUNKS x 16 bytes per thread, THREADS threads): fetch() early, park()
// into the free slot after the products that hide the loads' latency.
template <int CHUNKS, int THREADS>
struct OperandStager {
    u32x4 reg[CHUNKS];
    __device__ __forceinline__ void fetch(const uint16_t *block, int tid)
    {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(block);
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) reg[i] = src[tid + i * THREADS];
    }
    __device__ __forceinline__ void park(short *slot, int tid) const
    {
        u32x4 *dst = reinterpret_cast<u32x4 *>(slot);
#pragma unroll
        for (int i = 0; i < CHUNKS; ++i) dst[tid + i * THREADS] = reg[i];
    }
};

// sum / maximum over the four lane groups (lanes l, l ^ 16, l ^ 32, l ^ 48: the rows of one MFMA column).  (The 64-lane sum of the
// LayerNorm kernels in ffn_mfma.hip is not here: as a function its loop is unrolled before it is inlined, and the lane indices of the
// exchanges are then hoisted out of the kernels' token loops.)
__device__ __forceinline__ float lane_groups_sum(float v)
{
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float lane_groups_max(float v)
{
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}

// one LDS-DMA request (global_load_lds_dwordx4): lane l's 16 bytes at `src` land at dst + 16 l, without passing through registers
__device__ __forceinline__ void lds_dma16(const void *src, void *dst)
{
    __builtin_amdgcn_global_load_lds(src, reinterpret_cast<__attribute__((address_space(3))) void *>(reinterpret_cast<uintptr_t>(dst)), 16, 0, 0);
}

// one operand fragment from LDS, not visible to the compiler's wait-count bookkeeping (a __syncthreads, or any LDS read the compiler can
// see, waits for every LDS DMA in flight)
#define MFMA_LDS_READ(dst, addr, byte_off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(byte_off))
// "at most n LDS reads still in flight": everything older has arrived.  The operand ties the fragment to the wait.
#define MFMA_LDS_WAIT(n, a) asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(n))
// "at most n of this wave's memory requests (LDS-DMA included) still in flight": what was asked for before them has landed
#define MFMA_VM_WAIT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
