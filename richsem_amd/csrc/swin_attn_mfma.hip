// swin_attn_mfma.hip -- the shifted-window self-attention of a Swin block on the gfx950 matrix cores, forward and backward
// ("Swin window attention").
//
// Reference: models/richsem/swin_transformer.py:108-139 (WindowAttention.forward) inside :183-239 (SwinTransformerBlock.forward: pad, roll,
// window_partition, attention with the gathered relative-position bias and the additive region mask of :353-369, window_reverse, roll
// back).  Here roll, partition, reverse and un-roll are index arithmetic: the operands stay in map layout,
//     qkv   (B, Hp, Wp, 3 C) bf16, last dimension ordered (3, nH, 32); Hp, Wp multiples of the window w
//     table ((2w-1)^2, nH) fp32
//     out   (B, Hp, Wp, C) bf16;  lse (B, Hp, Wp, nH) fp32 (natural log-sum-exp of a token's score row, saved for the backward)
// Window (wy, wx) of the rolled map holds rolled coordinates py = wy w + i, px = wx w + j, token t = i w + j, which lives at
// ((py + s) mod Hp, (px + s) mod Wp).  Score of (t, t') on head h:
//     q_t . k_t' / sqrt(32) + table[(i - i' + w - 1)(2w - 1) + (j - j' + w - 1), h] - 100 [region(t) != region(t')]      (s > 0)
//     region = 3 r(py, Hp) + r(px, Wp),  r(c, n) = [c >= n - w] + [c >= n - s]
//
// The cut: one workgroup of four waves per (image, window, head).  The window's Q, K, V rows (w w <= 144 tokens x 32 channels, bf16)
// are read from the map once into LDS; every 16-token tile is a contiguous 1 KB block there, so a fragment read (lane (c, g): row c,
// channels 8 g .. 8 g + 7) is conflict-free.  A wave owns query tiles wave, wave + 4, ...  The products are taken transposed as in
// attn_mfma.hip: S^T = K . Q^T puts the query on the lane and the keys in the registers; a whole score row of a query (<= 160 keys) is
// 40 registers on the four lanes of its column, so the softmax is exact (one maximum, one sum, no rescaling) and the probabilities,
// rounded to bf16, are directly the B operand of O^T += V^T . P^T, V^T being read from a transposed copy in LDS.
// Token counts that are no multiple of 16 (w = 7: 49 -> 64) pad: rows past the last token are zero in LDS, padded keys get score -inf
// (probability exactly 0), padded queries are computed and not stored.
// Backward: the same workgroup cut, two phases over the same LDS rows.  Phase A has the queries on the lanes (dQ^T += K^T . dS^T) and
// accumulates the workgroup's part of dtable; phase B has the keys on the lanes (dV^T += dO^T . P, dK^T += Q^T . dS).  Probabilities are
// recomputed from lse; delta = rowsum(dO * out) is formed from the stored (bf16) out.  Every token is in one window: dqkv is written once,
// with plain stores.
// dtable: for one query the keys map to distinct bias indices, and for one key the queries do; in phase A the 16 lanes of one lane
// group g hold 16 queries against the SAME key per register, so their indices are distinct.  A wave adds its dS tile to a table of its
// own in LDS lane group by lane group (four steps, plain read-add-write), the four waves' tables are added in wave order, the
// workgroup's table goes to the workspace and one kernel adds the workgroups in ascending order: no atomics, the same bits every call.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"

namespace {

typedef short bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float lds_float;

constexpr int kHd = 32;             // head dimension
constexpr int kMaxTok = 144;        // tokens of a window (w w), at most nine 16-token tiles
constexpr int kMaxBlk = 5;          // 32-token blocks covering them
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kTS = 152;            // row stride (shorts) of a transposed copy X^T[32][tokens]
constexpr int kMaxTab = 23 * 23;    // (2 w - 1)^2 at w = 12
constexpr int kTabSlot = kMaxTab + 3;      // a wave's table + the slot dead pairs add to
constexpr float kLog2e = 1.4426950408889634f;

struct Geom {
    int Hp, Wp, w, s, nH;
    int nwx, nwin;      // windows per row, windows per image
};

// ---- what both kernels put into LDS first ----------------------------------------------------------------------------------------------
// tok_pix[t]: pixel index (b Hp + y) Wp + x of token t; tok_inf[t]: i | j << 8 | region << 16
__device__ __forceinline__ void window_tokens(const Geom &gm, int win, int *tok_pix, int *tok_inf, int tid)
{
    const int b = win / gm.nwin, wi = win - b * gm.nwin, wy = wi / gm.nwx, wx = wi - wy * gm.nwx;
    const int N = gm.w * gm.w;
    for (int t = tid; t < N; t += kThreads) {
        const int i = t / gm.w, j = t - i * gm.w;
        const int py = wy * gm.w + i, px = wx * gm.w + j;
        int y = py + gm.s, x = px + gm.s;
        if (y >= gm.Hp) y -= gm.Hp;
        if (x >= gm.Wp) x -= gm.Wp;
        int region = 0;
        if (gm.s > 0) {
            const int ry = (py >= gm.Hp - gm.w) + (py >= gm.Hp - gm.s), rx = (px >= gm.Wp - gm.w) + (px >= gm.Wp - gm.s);
            region = 3 * ry + rx;
        }
        tok_pix[t] = (b * gm.Hp + y) * gm.Wp + x;
        tok_inf[t] = i | (j << 8) | (region << 16);
    }
}

// rows [0, 16 nt) of one (token, 32) operand: 16 bytes per (token, part); rows past N are zero
__device__ __forceinline__ void fill_rows(const uint16_t *__restrict__ src, size_t ld, int col, const int *tok_pix, int N, int nt, short *rows,
                                          int tid)
{
    for (int e = tid; e < 64 * nt; e += kThreads) {
        const int t = e >> 2, part = e & 3;
        bf16x8 v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (t < N) v = *reinterpret_cast<const bf16x8 *>(src + (size_t)tok_pix[t] * ld + col + 8 * part);
        *reinterpret_cast<bf16x8 *>(rows + t * kHd + 8 * part) = v;
    }
}

// X^T[d][t] from the rows in LDS (columns past N are the rows' zeros)
__device__ __forceinline__ void fill_transposed(const short *rows, int nt, short *xt, int tid)
{
    for (int e = tid; e < 64 * nt; e += kThreads) {
        const int t = e >> 2, part = e & 3;
        const bf16x8 v = *reinterpret_cast<const bf16x8 *>(rows + t * kHd + 8 * part);
#pragma unroll
        for (int j = 0; j < 8; ++j) xt[(8 * part + j) * kTS + t] = v[j];
    }
}

// fragment of 16 rows (tile) of a row operand: lane (c, g) holds row 16 tile + c, channels 8 g .. 8 g + 7; zero past the last tile
__device__ __forceinline__ bf16x8 row_frag(const short *rows, int tile, int nt, int c, int g)
{
    if (tile >= nt) return (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    return *reinterpret_cast<const bf16x8 *>(rows + (16 * tile + c) * kHd + 8 * g);
}

// fragment of a transposed copy for the product that sums over an accumulator tile's rows: lane (row d, group g), element j <->
// token 32 blk + 16 (j >> 2) + 4 g + (j & 3); zero past the last tile
__device__ __forceinline__ bf16x8 frag_t(const short *xt, int d, int blk, int nt, int g)
{
    const short *p = xt + d * kTS + 32 * blk + 4 * g;
    bf16x4 lo = (bf16x4){0, 0, 0, 0}, hi = lo;
    if (2 * blk < nt) lo = *reinterpret_cast<const bf16x4 *>(p);
    if (2 * blk + 1 < nt) hi = *reinterpret_cast<const bf16x4 *>(p + 16);
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// bias index and mask of the pair (query info, key info)
__device__ __forceinline__ int bias_index(int iq, int ik, int w)
{
    const int di = (iq & 255) - (ik & 255) + w - 1, dj = ((iq >> 8) & 255) - ((ik >> 8) & 255) + w - 1;
    return di * (2 * w - 1) + dj;
}
__device__ __forceinline__ float region_mask(int iq, int ik) { return (iq >> 16) != (ik >> 16) ? -100.f : 0.f; }

// ---- forward ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void swin_attn_fwd_kernel(const uint16_t *__restrict__ qkv, const float *__restrict__ table, Geom gm,
                                                                 uint16_t *__restrict__ out, float *__restrict__ lse)
{
    __shared__ __attribute__((aligned(16))) short qr[kMaxTok * kHd], kr[kMaxTok * kHd], vr[kMaxTok * kHd];
    __shared__ __attribute__((aligned(16))) short vt[kHd * kTS];
    __shared__ float tab[kMaxTab];
    __shared__ int tok_pix[kMaxTok], tok_inf[kMaxTok];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, C = gm.nH * kHd, N = gm.w * gm.w, nt = (N + 15) / 16, nR = (2 * gm.w - 1) * (2 * gm.w - 1);
    const float scale = 0.17677669529663687f;      // 1 / sqrt(32)

    window_tokens(gm, blockIdx.x, tok_pix, tok_inf, tid);
    for (int r = tid; r < nR; r += kThreads) tab[r] = table[(size_t)r * gm.nH + h];
    __syncthreads();
    fill_rows(qkv, 3 * (size_t)C, h * kHd, tok_pix, N, nt, qr, tid);
    fill_rows(qkv, 3 * (size_t)C, C + h * kHd, tok_pix, N, nt, kr, tid);
    fill_rows(qkv, 3 * (size_t)C, 2 * C + h * kHd, tok_pix, N, nt, vr, tid);
    __syncthreads();
    fill_transposed(vr, nt, vt, tid);
    __syncthreads();

    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int qt = wave; qt < nt; qt += kWaves) {
        const int tq = 16 * qt + c;
        const int iq = tok_inf[min(tq, N - 1)];
        const bf16x8 qf = row_frag(qr, qt, nt, c, g);
        float sc[kMaxBlk][8];
        float mx = -__builtin_inff();
#pragma unroll
        for (int kb = 0; kb < kMaxBlk; ++kb) {
            if (2 * kb < nt) {
                const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(kr, 2 * kb, nt, c, g), qf, zero, 0, 0, 0);
                const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(kr, 2 * kb + 1, nt, c, g), qf, zero, 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int tk = 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3);
                    float v = -__builtin_inff();
                    if (tk < N) {
                        const int ik = tok_inf[tk];
                        v = (j < 4 ? s0[j & 3] : s1[j & 3]) * scale + tab[bias_index(iq, ik, gm.w)] + region_mask(iq, ik);
                    }
                    sc[kb][j] = v;
                    mx = fmaxf(mx, v);
                }
            }
        }
        mx = lane_groups_max(mx);      // (key 0 is always alive: finite)
        float l = 0.f;
        f32x4 o0 = zero, o1 = zero;
#pragma unroll
        for (int kb = 0; kb < kMaxBlk; ++kb) {
            if (2 * kb < nt) {
                float p[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    p[j] = exp2f((sc[kb][j] - mx) * kLog2e);
                    l += p[j];
                }
                const bf16x8 pb = pack_bf16x8(p);
                o0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(vt, c, kb, nt, g), pb, o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(vt, 16 + c, kb, nt, g), pb, o1, 0, 0, 0);
            }
        }
        l = lane_groups_sum(l);
        if (tq < N) {
            const float inv = 1.f / l;
            const size_t pix = (size_t)tok_pix[tq];
            uint16_t *op = out + pix * C + h * kHd + 4 * g;
            *reinterpret_cast<uint2 *>(op) = pack_bf16x4(o0 * inv);
            *reinterpret_cast<uint2 *>(op + 16) = pack_bf16x4(o1 * inv);
            if (g == 0) lse[pix * gm.nH + h] = mx + logf(l);
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void swin_attn_bwd_kernel(const uint16_t *__restrict__ qkv, const float *__restrict__ table,
                                                                 const uint16_t *__restrict__ out, const float *__restrict__ lse,
                                                                 const uint16_t *__restrict__ dout, Geom gm, uint16_t *__restrict__ dqkv,
                                                                 float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) short qr[kMaxTok * kHd], kr[kMaxTok * kHd], vr[kMaxTok * kHd], gr[kMaxTok * kHd];
    __shared__ __attribute__((aligned(16))) short xt[2][kHd * kTS];      // phase A: K^T and the waves' tables; phase B: Q^T and dO^T
    __shared__ float tab[kMaxTab];
    __shared__ float lse_s[kMaxTok], delta_s[kMaxTok];
    __shared__ int tok_pix[kMaxTok], tok_inf[kMaxTok];
    static_assert(kWaves * kTabSlot * sizeof(float) <= sizeof(short) * kHd * kTS, "the waves' tables lie over xt[1]");
    float *wtab = reinterpret_cast<float *>(xt[1]);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, C = gm.nH * kHd, N = gm.w * gm.w, nt = (N + 15) / 16, nR = (2 * gm.w - 1) * (2 * gm.w - 1);
    const float scale = 0.17677669529663687f;

    window_tokens(gm, blockIdx.x, tok_pix, tok_inf, tid);
    for (int r = tid; r < nR; r += kThreads) tab[r] = table[(size_t)r * gm.nH + h];
    for (int r = tid; r < kWaves * kTabSlot; r += kThreads) wtab[r] = 0.f;
    __syncthreads();
    fill_rows(qkv, 3 * (size_t)C, h * kHd, tok_pix, N, nt, qr, tid);
    fill_rows(qkv, 3 * (size_t)C, C + h * kHd, tok_pix, N, nt, kr, tid);
    fill_rows(qkv, 3 * (size_t)C, 2 * C + h * kHd, tok_pix, N, nt, vr, tid);
    fill_rows(dout, (size_t)C, h * kHd, tok_pix, N, nt, gr, tid);
    for (int t = tid; t < N; t += kThreads) {      // delta from the stored out and dout
        const size_t pix = (size_t)tok_pix[t];
        const uint16_t *o = out + pix * C + h * kHd, *d = dout + pix * C + h * kHd;
        float sum = 0.f;
#pragma unroll
        for (int part = 0; part < 4; ++part) {
            const bf16x8 a = *reinterpret_cast<const bf16x8 *>(o + 8 * part), b = *reinterpret_cast<const bf16x8 *>(d + 8 * part);
#pragma unroll
            for (int j = 0; j < 8; ++j)
                sum += __uint_as_float((unsigned)(uint16_t)a[j] << 16) * __uint_as_float((unsigned)(uint16_t)b[j] << 16);
        }
        delta_s[t] = sum;
        lse_s[t] = lse[pix * gm.nH + h];
    }
    __syncthreads();
    fill_transposed(kr, nt, xt[0], tid);
    __syncthreads();

    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    // (as an LDS pointer, the way lds_dma16 forms one: the low 32 bits of a generic LDS address are the LDS offset)
    volatile lds_float *mytab_lds = reinterpret_cast<volatile lds_float *>(reinterpret_cast<uintptr_t>(wtab + wave * kTabSlot));

    // phase A: queries on the lanes -- dQ and the table
    for (int qt = wave; qt < nt; qt += kWaves) {
        const int tq = 16 * qt + c, tqc = min(tq, N - 1);
        const int iq = tok_inf[tqc];
        const float lq = lse_s[tqc], dl = delta_s[tqc];
        const bf16x8 qf = row_frag(qr, qt, nt, c, g), gf = row_frag(gr, qt, nt, c, g);
        f32x4 dq0 = zero, dq1 = zero;
#pragma unroll
        for (int kb = 0; kb < kMaxBlk; ++kb) {
            if (2 * kb < nt) {
                const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(kr, 2 * kb, nt, c, g), qf, zero, 0, 0, 0);
                const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(kr, 2 * kb + 1, nt, c, g), qf, zero, 0, 0, 0);
                const f32x4 p0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(vr, 2 * kb, nt, c, g), gf, zero, 0, 0, 0);
                const f32x4 p1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(vr, 2 * kb + 1, nt, c, g), gf, zero, 0, 0, 0);
                float ds[8];
                int ri[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int tk = 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3);
                    ds[j] = 0.f;
                    ri[j] = kMaxTab + (j & 1);      // dead pairs: a slot nobody reads
                    if (tk < N && tq < N) {
                        const int ik = tok_inf[tk];
                        ri[j] = bias_index(iq, ik, gm.w);
                        const float sv = (j < 4 ? s0[j & 3] : s1[j & 3]) * scale + tab[ri[j]] + region_mask(iq, ik);
                        const float pj = exp2f((sv - lq) * kLog2e);
                        ds[j] = pj * ((j < 4 ? p0[j & 3] : p1[j & 3]) - dl);
                    }
                }
                // the 16 lanes of a group hold one key per register against 16 queries: distinct indices within one read-add-write.
                // Group after group, register after register: a wave's LDS accesses complete in program order.
#pragma unroll
                for (int g0 = 0; g0 < 4; ++g0) {
                    // (the step's number is hidden from the compiler: to one thread the four steps are one `if` that is always
                    // taken once, and merged into that the four groups would read and write in the same instructions)
                    int step = g0;
#if defined(__HIP_DEVICE_COMPILE__)
                    asm volatile("" : "+s"(step));
#endif
                    __builtin_amdgcn_wave_barrier();
                    if (g == step) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            volatile lds_float *slot = mytab_lds + ri[j];
                            *slot = *slot + ds[j];
                        }
                    }
                }
                const bf16x8 dsb = pack_bf16x8(ds);
                dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[0], c, kb, nt, g), dsb, dq0, 0, 0, 0);
                dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[0], 16 + c, kb, nt, g), dsb, dq1, 0, 0, 0);
            }
        }
        if (tq < N) {
            uint16_t *pq = dqkv + (size_t)tok_pix[tq] * (3 * (size_t)C) + h * kHd + 4 * g;
            *reinterpret_cast<uint2 *>(pq) = pack_bf16x4(dq0 * scale);
            *reinterpret_cast<uint2 *>(pq + 16) = pack_bf16x4(dq1 * scale);
        }
    }
    __syncthreads();
    {   // the waves' tables in wave order -> this workgroup's row of the workspace
        float *row = ws + ((size_t)blockIdx.x * gm.nH + h) * nR;
        for (int r = tid; r < nR; r += kThreads) {
            float a = wtab[r];
#pragma unroll
            for (int wv = 1; wv < kWaves; ++wv) a += wtab[wv * kTabSlot + r];
            row[r] = a;
        }
    }
    __syncthreads();
    fill_transposed(qr, nt, xt[0], tid);
    fill_transposed(gr, nt, xt[1], tid);
    __syncthreads();

    // phase B: keys on the lanes -- dK and dV
    for (int kt = wave; kt < nt; kt += kWaves) {
        const int tk = 16 * kt + c;
        const int ik = tok_inf[min(tk, N - 1)];
        const bf16x8 kf = row_frag(kr, kt, nt, c, g), vf = row_frag(vr, kt, nt, c, g);
        f32x4 dk0 = zero, dk1 = zero, dv0 = zero, dv1 = zero;
#pragma unroll
        for (int qb = 0; qb < kMaxBlk; ++qb) {
            if (2 * qb < nt) {
                const f32x4 s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(qr, 2 * qb, nt, c, g), kf, zero, 0, 0, 0);
                const f32x4 s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(qr, 2 * qb + 1, nt, c, g), kf, zero, 0, 0, 0);
                const f32x4 p0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(gr, 2 * qb, nt, c, g), vf, zero, 0, 0, 0);
                const f32x4 p1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(row_frag(gr, 2 * qb + 1, nt, c, g), vf, zero, 0, 0, 0);
                float p[8], ds[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int tq = 32 * qb + 16 * (j >> 2) + 4 * g + (j & 3);
                    p[j] = 0.f;
                    ds[j] = 0.f;
                    if (tk < N && tq < N) {
                        const int iq = tok_inf[tq];
                        const float sv = (j < 4 ? s0[j & 3] : s1[j & 3]) * scale + tab[bias_index(iq, ik, gm.w)] + region_mask(iq, ik);
                        p[j] = exp2f((sv - lse_s[tq]) * kLog2e);
                        ds[j] = p[j] * ((j < 4 ? p0[j & 3] : p1[j & 3]) - delta_s[tq]);
                    }
                }
                const bf16x8 pb = pack_bf16x8(p), dsb = pack_bf16x8(ds);
                dv0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[1], c, qb, nt, g), pb, dv0, 0, 0, 0);
                dv1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[1], 16 + c, qb, nt, g), pb, dv1, 0, 0, 0);
                dk0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[0], c, qb, nt, g), dsb, dk0, 0, 0, 0);
                dk1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_t(xt[0], 16 + c, qb, nt, g), dsb, dk1, 0, 0, 0);
            }
        }
        if (tk < N) {
            uint16_t *pk = dqkv + (size_t)tok_pix[tk] * (3 * (size_t)C) + C + h * kHd + 4 * g, *pv = pk + C;
            *reinterpret_cast<uint2 *>(pk) = pack_bf16x4(dk0 * scale);
            *reinterpret_cast<uint2 *>(pk + 16) = pack_bf16x4(dk1 * scale);
            *reinterpret_cast<uint2 *>(pv) = pack_bf16x4(dv0);
            *reinterpret_cast<uint2 *>(pv + 16) = pack_bf16x4(dv1);
        }
    }
}

// dtable[r, h] = the workgroups' rows added in ascending order
__global__ void swin_attn_table_reduce_kernel(const float *__restrict__ ws, int groups, int nR, int nH, float *__restrict__ dtable)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nR * nH) return;
    const int h = idx / nR, r = idx - h * nR;
    float a = 0.f;
    for (int gi = 0; gi < groups; ++gi) a += ws[((size_t)gi * nH + h) * nR + r];
    dtable[(size_t)r * nH + h] = a;
}

// what every entry point checks first: MSDA_OK, or the class of error
int check_dims(int B, int Hp, int Wp, int channels, int heads, int w, int s, Geom *gm)
{
    if (B < 1 || Hp < 1 || Wp < 1 || heads < 1 || channels != heads * kHd || w < 1 || w * w > kMaxTok || s < 0 || s >= w || Hp % w || Wp % w)
        return MSDA_ERR_BAD_DIMS;
    const long long pixels = (long long)B * Hp * Wp, groups = pixels / (w * w);
    if (pixels * 3 * channels >= (1LL << 40) || pixels >= (1LL << 31) || groups >= (1LL << 31) || heads > 65535) return MSDA_ERR_TOO_LARGE;
    *gm = Geom{Hp, Wp, w, s, heads, Wp / w, (Hp / w) * (Wp / w)};
    return MSDA_OK;
}

}  // namespace

extern "C" {

int msda_swin_attn_workspace_bytes(int B, int Hp, int Wp, int channels, int heads, int window, int64_t *bytes)
{
    Geom gm;
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(B, Hp, Wp, channels, heads, window, 0, &gm)) return msda::arg_fail(e, __func__);
    *bytes = (int64_t)B * gm.nwin * heads * (2 * window - 1) * (2 * window - 1) * (int64_t)sizeof(float);
    return MSDA_OK;
}

int msda_swin_attn_forward_bf16(const uint16_t *qkv, const float *table, int B, int Hp, int Wp, int channels, int heads, int window,
                                int shift, uint16_t *out, float *lse, msda_stream_t stream)
{
    Geom gm;
    if (!qkv || !table || !out || !lse) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(B, Hp, Wp, channels, heads, window, shift, &gm)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {qkv, out}) || !msda::aligned(4, {table, lse})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipLaunchKernelGGL(swin_attn_fwd_kernel, dim3(B * gm.nwin, heads), dim3(kThreads), 0, static_cast<hipStream_t>(stream), qkv, table, gm,
                       out, lse);
    return msda::launched(__func__);
}

int msda_swin_attn_backward_bf16(const uint16_t *qkv, const float *table, const uint16_t *out, const float *lse, const uint16_t *dout, int B,
                                 int Hp, int Wp, int channels, int heads, int window, int shift, uint16_t *dqkv, float *dtable,
                                 void *workspace, msda_stream_t stream)
{
    Geom gm;
    if (!qkv || !table || !out || !lse || !dout || !dqkv || !dtable || !workspace) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(B, Hp, Wp, channels, heads, window, shift, &gm)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {qkv, out, dout, dqkv}) || !msda::aligned(4, {table, lse, dtable, workspace}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int groups = B * gm.nwin, nR = (2 * window - 1) * (2 * window - 1);
    hipLaunchKernelGGL(swin_attn_bwd_kernel, dim3(groups, heads), dim3(kThreads), 0, st, qkv, table, out, lse, dout, gm, dqkv,
                       static_cast<float *>(workspace));
    hipLaunchKernelGGL(swin_attn_table_reduce_kernel, dim3((nR * heads + 255) / 256), dim3(256), 0, st,
                       static_cast<const float *>(workspace), groups, nR, heads, dtable);
    return msda::launched(__func__);
}

}  // extern "C"
