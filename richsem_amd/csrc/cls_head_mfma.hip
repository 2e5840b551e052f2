// cls_head_mfma.hip -- the CLIP-text class head, forward and backward, as gfx950 MFMA kernels ("Class head").
//
// Reference: models/richsem/richsem.py:182-205 (CLIPAlign.forward / forward_hs, shipped configuration: dino_visual_proj a bias-free
// nn.Linear(256, 1024), frozen text side and logit_scale):
//     f = Wp x;  logits_c = exp(logit_scale) * (f / |f|) . (t_c / |t_c|)
// With G = T^ Wp (classes x 256) and A = Wp^T Wp (256 x 256) -- the operands of csrc/cls_mfma.hip -- the head collapses onto the 256-wide
// input, forward and backward (s = exp(logit_scale), g = dL/dlogits, beta = sum_c g_c logits_c):
//     n2 = x . (A x),  n = sqrt(n2),  logits_c = s (G x)_c / n
//     dx      = (s / n) G^T g - (beta / n2) (A x)
//     [dG;dA] = Y^T x,   Y = [ (s / n) g | -(beta / (2 n2)) x ]     (rows x (classes + 256)), contraction over the rows
// (the caller finishes dWp = T^^T dG + Wp (dA + dA^T) with two small fp32 products).  The 1024-wide feature is never written.
//
// Operand: msda_cls_head_pack writes, in MFMA fragment order as bf16 hi + lo parts (the tile format of msda_cls_pack),
//     region 1   the 16-row tiles of [A; G; zero rows up to a multiple of 16] -- A FIRST, so that a row's norm is complete before its
//                first logit is formed (msda_cls_pack's order, G first, is unchanged and stays ClassScorer's);
//     region 2   G^T by k-steps of 32 classes (zero past `classes`): the operand of the rows backward, which contracts over the classes.
//
// Precision (the rule of cls_mfma.hip): fp32 operands are split into bf16 hi + lo parts, products hi.hi + lo.hi + hi.lo, fp32 accumulation.
//   forward        [A; G] hi + lo under parts = 2, hi under parts = 1; fp32 x hi + lo (both parts values), bf16 x as it is.
//                  logit = acc * (s / sqrtf(n2)).
//   backward       THE CHOICE FOR g: under parts = 2 g enters the MFMA as bf16 hi + lo -- in the rows kernel g itself against G^T hi + lo,
//                  in the weights kernel y = fp32((s / n) g), resp. fp32(-(beta / (2 n2)) x), as hi + lo against x hi + lo (a bf16 x has no lo
//                  part); under parts = 1 every backward operand is rounded to bf16 once (hi . hi: a plain bf16 product).  beta is an fp32
//                  sum of fp32 products g_c * logits_c; A x is recomputed with the forward's products; the epilogue is fp32.
// The element-wise bounds that follow from these points, the exact probes and the emulation are in tests/class_head_ref.py.
// A row x = 0 has n2 = 0: its logits and its dx are NaN as the reference's f / |f| is, no other row's are; [dG; dA] is then NaN as the
// reference's weight gradient is.
//
// Structure.  Forward (as cls_score_kernel): transposed product, tokens on the lanes, a wave keeps the x fragments of its 48 tokens in
// registers, the operand streams through LDS in 16 KB tiles; the class tiles are cut into chunks over blockIdx.y (every chunk repeats
// the 16 tiles of A) so that 13 104 rows fill the device.  A lane's accumulator holds 4 classes of one token -- stored directly that is
// 16-byte pieces a logits row apart -- so two class tiles go through a per-wave LDS block and leave as 128-byte runs of a row.
// Backward, rows: channels on the MFMA rows, 16 tokens of a wave on the lanes, K = classes in steps of 32; g and logits are read once, in
// fragment order -- 32 bytes per lane, a wave's request spans 16 rows -- and dx leaves as 16-byte (8-byte for bf16) pieces per lane, 64-byte
// runs of a row 1 KB apart: NOT the coalesced form the forward's stores have (dx is 13 MB against 63 MB of g at the step's shape).  Every
// class chunk of the forward repeats A's 16 tiles (at 1 800 rows most of its products): a first pass writing n2 once would remove that.
// Backward, weights: [dG; dA] in groups of 64 rows x 256 columns per workgroup, the rows of x cut into splits of kSplitRows; every split writes its partial sum to the workspace and one kernel adds the splits in ascending order: no atomics, the
// same bits on every run.  No kernel allocates, synchronises with the host or depends on anything but its arguments.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mfma_common.h"
#include "msda_host.h"

namespace {

constexpr int kD = 256;
constexpr int kMaxClasses = 8192;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * 64;
constexpr int kATiles = kD / 16;                      // the tiles of A in front of region 1
constexpr int kTileShorts = 2 * 8 * kFragShorts;      // region 1: 16 rows x 256 k, hi + lo parts: 16 KB
constexpr int kStepShorts = 2 * 16 * kFragShorts;     // region 2: 32 classes x 256 channels, hi + lo parts: 32 KB
constexpr int kFwdTokWave = 48, kFwdTokWg = kFwdTokWave * kWaves;
constexpr int kRowTokWave = 16, kRowTokWg = kRowTokWave * kWaves;
constexpr int kSplitRows = 512;                       // rows of one split of the weights kernel (a multiple of 32)
constexpr int kGroupRows = 64;                        // rows of [dG; dA] per workgroup of the weights kernel
constexpr int kOutStride = 36;                        // floats per token in the forward's store block: 32 classes + 4 (bank spread)
constexpr int kFillCus = 256;                         // the forward cuts the classes until about this many workgroups exist

__host__ __device__ inline int class_tiles(int classes) { return (classes + 15) / 16; }
__host__ __device__ inline int class_steps(int classes) { return (classes + 31) / 32; }
__host__ __device__ inline long long region1_shorts(int classes) { return (long long)(kATiles + class_tiles(classes)) * kTileShorts; }

__global__ void cls_head_pack_kernel(const float *__restrict__ G, int classes, const float *__restrict__ A, uint16_t *__restrict__ packed)
{
    const long long n1 = region1_shorts(classes) / 2, n2 = (long long)class_steps(classes) * (kStepShorts / 2);
    uint16_t *r2 = packed + region1_shorts(classes);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n1 + n2; i += (long long)gridDim.x * blockDim.x) {
        float v = 0.f;
        long long hi_at, lo_off;
        uint16_t *base;
        if (i < n1) {      // [tile][part][k-step][lane][8]: lane (r, q) = row 16 tile + r, k = 32 step + 8 q + 0..7
            const int j = (int)(i & 7), lane = (int)((i >> 3) & 63), s = (int)((i >> 9) & 7), t = (int)(i >> 12);
            const int row = 16 * t + (lane & 15), k = 32 * s + 8 * (lane >> 4) + j;
            if (t < kATiles) v = A[(long long)row * kD + k];
            else if (row - kD < classes) v = G[(long long)(row - kD) * kD + k];
            base = packed;
            hi_at = (long long)t * kTileShorts + (long long)s * kFragShorts + lane * 8 + j;
            lo_off = 8 * kFragShorts;
        } else {           // [k-step][part][channel tile][lane][8]: lane (r, q) = channel 16 tile + r, class = 32 step + 8 q + 0..7
            const long long e = i - n1;
            const int j = (int)(e & 7), lane = (int)((e >> 3) & 63), jt = (int)((e >> 9) & 15), s = (int)(e >> 13);
            const int cls = 32 * s + 8 * (lane >> 4) + j, ch = 16 * jt + (lane & 15);
            if (cls < classes) v = G[(long long)cls * kD + ch];
            base = r2;
            hi_at = (long long)s * kStepShorts + (long long)jt * kFragShorts + lane * 8 + j;
            lo_off = 16 * kFragShorts;
        }
        const Bf16Split parts = split_bf16(v);
        base[hi_at] = parts.hi;
        base[hi_at + lo_off] = parts.lo;
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------------
// XF32: x is fp32 (split into hi + lo here), else bf16.  WPARTS: 2 = the operand's hi + lo parts, 1 = hi part only.
// grid (row blocks, class chunks): chunk y owns the class tiles [2 y gpc, 2 (y + 1) gpc) after the 16 tiles of A; chunk 0 stores n2.
template <bool XF32, int WPARTS>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
void cls_head_forward_kernel(const void *__restrict__ xv, const uint16_t *__restrict__ packed, int T, int classes, float scale, int gpc,
                             float *__restrict__ logits, float *__restrict__ n2_out)
{
    __shared__ __attribute__((aligned(16))) short wbuf[2][WPARTS * 8 * kFragShorts];
    __shared__ __attribute__((aligned(16))) float obuf[kWaves][kFwdTokWave * kOutStride];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int tok0 = blockIdx.x * kFwdTokWg + wave * kFwdTokWave;
    const int ct = class_tiles(classes);
    const int gt0 = 2 * (int)blockIdx.y * gpc, gt1 = min(ct, gt0 + 2 * gpc);
    const int n_tiles = kATiles + (gt1 - gt0);

    bf16x8 xh[3][8], xl[XF32 ? 3 : 1][8];
    if constexpr (XF32) {
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) {
            const float *row = static_cast<const float *>(xv) + (size_t)min(tok0 + 16 * t3 + c, T - 1) * kD + 8 * q;
#pragma unroll
            for (int s = 0; s < 8; ++s) split_bf16x8(row + 32 * s, xh[t3][s], xl[t3][s]);
        }
    } else {
        load_x_frags(static_cast<const uint16_t *>(xv), tok0, T, c, q, xh);
    }

    float nrm[3] = {0.f, 0.f, 0.f}, inv[3] = {0.f, 0.f, 0.f};
    float *ob = obuf[wave];

    // tile i of this workgroup: A's tiles, then its own class tiles
    auto tile_at = [&](int i) { return packed + (size_t)(i < kATiles ? i : i + gt0) * kTileShorts; };
    OperandStager<WPARTS * 8 * kFragShorts * 2 / 16 / kThreads, kThreads> stage;
    stage.fetch(tile_at(0), tid);
    stage.park(wbuf[0], tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        if (t + 1 < n_tiles) stage.fetch(tile_at(t + 1), tid);
        const short *wt = wbuf[t & 1];
        f32x4 acc[3];
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3) acc[t3] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(wt + s * kFragShorts + lane * 8);
            bf16x8 al;
            if (WPARTS == 2) al = *reinterpret_cast<const bf16x8 *>(wt + (8 + s) * kFragShorts + lane * 8);
            if (WPARTS == 2) {
#pragma unroll
                for (int t3 = 0; t3 < 3; ++t3) acc[t3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xh[t3][s], acc[t3], 0, 0, 0);
            }
            if (XF32) {
#pragma unroll
                for (int t3 = 0; t3 < 3; ++t3) acc[t3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xl[XF32 ? t3 : 0][s], acc[t3], 0, 0, 0);
            }
#pragma unroll
            for (int t3 = 0; t3 < 3; ++t3) acc[t3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xh[t3][s], acc[t3], 0, 0, 0);
        }
        const int lt = t - kATiles;      // class tile of this chunk (negative: a tile of A)
        if (lt < 0) {      // rows of A x: channels 16 t + 4 q + i, times x of the same channels
            const int ch0 = 16 * t + 4 * q;
#pragma unroll
            for (int t3 = 0; t3 < 3; ++t3) {
                const int tok = min(tok0 + 16 * t3 + c, T - 1);
                f32x4 xs;
                if (XF32) {
                    const float4 v = *reinterpret_cast<const float4 *>(static_cast<const float *>(xv) + (size_t)tok * kD + ch0);
                    xs = (f32x4){v.x, v.y, v.z, v.w};
                } else {
                    xs = unpack_bf16x4(*reinterpret_cast<const uint2 *>(static_cast<const uint16_t *>(xv) + (size_t)tok * kD + ch0));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) nrm[t3] = fmaf(acc[t3][i], xs[i], nrm[t3]);
            }
            if (t == kATiles - 1) {      // the norm is complete: one factor per token for every logit that follows
#pragma unroll
                for (int t3 = 0; t3 < 3; ++t3) {
                    const float n2 = lane_groups_sum(nrm[t3]);
                    const int tok = tok0 + 16 * t3 + c;
                    if (blockIdx.y == 0 && q == 0 && tok < T) n2_out[tok] = n2;
                    inv[t3] = scale / sqrtf(n2);
                }
            }
        } else {           // classes 16 (gt0 + lt) + 4 q + i of token c: into this wave's store block, columns 16 (lt & 1) + 4 q + i
#pragma unroll
            for (int t3 = 0; t3 < 3; ++t3) {
                const f32x4 v = acc[t3] * inv[t3];
                *reinterpret_cast<f32x4 *>(ob + (16 * t3 + c) * kOutStride + 16 * (lt & 1) + 4 * q) = v;
            }
        }
        if (t + 1 < n_tiles) stage.park(wbuf[(t + 1) & 1], tid);
        __syncthreads();
        if (lt >= 0 && ((lt & 1) || t + 1 == n_tiles)) {      // two tiles (or the last one) are in the block: half a wave per row, 128-byte runs
            const int cls = 16 * (gt0 + (lt & ~1)) + (lane & 31);
            const bool col_ok = cls < classes && (lane & 31) < 16 * ((lt & 1) + 1);
#pragma unroll 4
            for (int it = 0; it < kFwdTokWave / 2; ++it) {
                const int r = 2 * it + (lane >> 5), tok = tok0 + r;
                const float v = ob[r * kOutStride + (lane & 31)];
                if (col_ok && tok < T) logits[(size_t)tok * classes + cls] = v;
            }
        }
    }
}

// ---- backward, rows -------------------------------------------------------------------------------------------------------------------
// eight consecutive floats of a row of g / logits from class `cls0`, zero past `classes`; vec: the row starts 16-byte aligned and
// classes is a multiple of 4 (cls0 is a multiple of 8)
__device__ __forceinline__ void load_row8(const float *__restrict__ row, int cls0, int classes, bool vec, float (&v)[8])
{
    if (vec && cls0 + 8 <= classes) {
        const float4 a = *reinterpret_cast<const float4 *>(row + cls0), b = *reinterpret_cast<const float4 *>(row + cls0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = cls0 + j < classes ? row[cls0 + j] : 0.f;
    }
}

__device__ __forceinline__ void split8(const float (&v)[8], bf16x8 &hi, bf16x8 &lo)
{
    u32x4 h, l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = pack_bf16(v[2 * i], v[2 * i + 1]);
        l[i] = pack_bf16(v[2 * i] - bf16_lo(h[i]), v[2 * i + 1] - bf16_hi(h[i]));
    }
    hi = __builtin_bit_cast(bf16x8, h);
    lo = __builtin_bit_cast(bf16x8, l);
}

template <bool XF32, int PARTS>
__global__ __launch_bounds__(kThreads)
void cls_head_bwd_rows_kernel(const float *__restrict__ g, const float *__restrict__ logits, const float *__restrict__ n2v,
                              const void *__restrict__ xv, const uint16_t *__restrict__ packed, int T, int classes, float scale, int vec,
                              void *__restrict__ dxv, float *__restrict__ beta_out)
{
    // (PARTS = 2: 65 536 bytes, exactly the limit of static LDS -- one more __shared__ byte in this kernel does not build)
    __shared__ __attribute__((aligned(16))) short wbuf[2][PARTS * 16 * kFragShorts];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int tok = blockIdx.x * kRowTokWg + wave * kRowTokWave + c, tokc = min(tok, T - 1);
    const int ks = class_steps(classes);
    const uint16_t *gT = packed + region1_shorts(classes);
    const float *grow = g + (size_t)tokc * classes, *lrow = logits + (size_t)tokc * classes;

    f32x4 acc[16];
#pragma unroll
    for (int jt = 0; jt < 16; ++jt) acc[jt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float betap = 0.f;

    // pass 1: G^T g over the classes, beta on the way
    {
        OperandStager<PARTS * 16 * kFragShorts * 2 / 16 / kThreads, kThreads> stage;
        stage.fetch(gT, tid);
        stage.park(wbuf[0], tid);
        float gn[8], ln[8];
        load_row8(grow, 8 * q, classes, vec, gn);
        load_row8(lrow, 8 * q, classes, vec, ln);
        __syncthreads();
        for (int s = 0; s < ks; ++s) {
            float gc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                gc[j] = gn[j];
                betap = fmaf(gn[j], ln[j], betap);
            }
            if (s + 1 < ks) {
                stage.fetch(gT + (size_t)(s + 1) * kStepShorts, tid);
                load_row8(grow, 32 * (s + 1) + 8 * q, classes, vec, gn);
                load_row8(lrow, 32 * (s + 1) + 8 * q, classes, vec, ln);
            }
            bf16x8 gh, gl;
            split8(gc, gh, gl);
            const short *wt = wbuf[s & 1];
#pragma unroll
            for (int jt = 0; jt < 16; ++jt) {
                const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(wt + jt * kFragShorts + lane * 8);
                if (PARTS == 2) {
                    const bf16x8 al = *reinterpret_cast<const bf16x8 *>(wt + (16 + jt) * kFragShorts + lane * 8);
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, gh, acc[jt], 0, 0, 0);
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, gl, acc[jt], 0, 0, 0);
                }
                acc[jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, gh, acc[jt], 0, 0, 0);
            }
            if (s + 1 < ks) stage.park(wbuf[(s + 1) & 1], tid);
            __syncthreads();
        }
    }
    const float beta = lane_groups_sum(betap);
    if (q == 0 && tok < T) beta_out[tok] = beta;
    const float n2 = n2v[tokc];
    const float c1 = scale / sqrtf(n2), c2 = beta / n2;

    // pass 2: A x again (the forward's products), channel tile by channel tile, and the store
    bf16x8 xh[8], xl[XF32 ? 8 : 1];
    if constexpr (XF32) {
        const float *row = static_cast<const float *>(xv) + (size_t)tokc * kD + 8 * q;
#pragma unroll
        for (int s = 0; s < 8; ++s) split_bf16x8(row + 32 * s, xh[s], xl[s]);
    } else {
        const uint16_t *row = static_cast<const uint16_t *>(xv) + (size_t)tokc * kD + 8 * q;
#pragma unroll
        for (int s = 0; s < 8; ++s) xh[s] = *reinterpret_cast<const bf16x8 *>(row + 32 * s);
    }
    OperandStager<PARTS * 8 * kFragShorts * 2 / 16 / kThreads, kThreads> stage;
    stage.fetch(packed, tid);
    stage.park(wbuf[0], tid);      // (every wave is past the last barrier of pass 1: nobody reads wbuf)
    __syncthreads();
#pragma unroll
    for (int jt = 0; jt < 16; ++jt) {
        if (jt + 1 < 16) stage.fetch(packed + (size_t)(jt + 1) * kTileShorts, tid);
        const short *wt = wbuf[jt & 1];
        f32x4 ax = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8 *>(wt + s * kFragShorts + lane * 8);
            if (PARTS == 2) {
                const bf16x8 al = *reinterpret_cast<const bf16x8 *>(wt + (8 + s) * kFragShorts + lane * 8);
                ax = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, xh[s], ax, 0, 0, 0);
            }
            if (XF32) ax = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xl[XF32 ? s : 0], ax, 0, 0, 0);
            ax = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, xh[s], ax, 0, 0, 0);
        }
        f32x4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = c1 * acc[jt][i] - c2 * ax[i];
        if (tok < T) {
            const size_t at = (size_t)tok * kD + 16 * jt + 4 * q;
            if (XF32) *reinterpret_cast<f32x4 *>(static_cast<float *>(dxv) + at) = d;
            else *reinterpret_cast<uint2 *>(static_cast<uint16_t *>(dxv) + at) = pack_bf16x4(d);
        }
        if (jt + 1 < 16) stage.park(wbuf[(jt + 1) & 1], tid);
        __syncthreads();
    }
}

// ---- backward, weights ----------------------------------------------------------------------------------------------------------------
// grid (row groups of [dG; dA], splits).  Per step of 32 rows the workgroup writes the fragments of x (B operand: lane (k, q) = rows
// 8 q + 0..7 of column k) and of its 64 columns of Y (A operand) to LDS; wave w owns the column tiles 4 w .. 4 w + 3 of x.
template <bool XF32, int PARTS>
__global__ __launch_bounds__(kThreads)
void cls_head_bwd_weights_kernel(const float *__restrict__ g, const float *__restrict__ n2v, const float *__restrict__ beta,
                                 const void *__restrict__ xv, int T, int classes, float scale, float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) short xb[2][16 * kFragShorts];
    __shared__ __attribute__((aligned(16))) short yb[2][4 * kFragShorts];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int n_g = (classes + kGroupRows - 1) / kGroupRows;
    const bool is_g = (int)blockIdx.x < n_g;
    const int m0 = is_g ? kGroupRows * blockIdx.x : kGroupRows * ((int)blockIdx.x - n_g);      // first class, or first row of dA
    const int row_begin = blockIdx.y * kSplitRows, row_end = min(T, row_begin + kSplitRows);
    const int ml = tid & 63, yq = tid >> 6;      // the Y fill: column m0 + ml, rows 8 yq + 0..7 of the step
    constexpr bool XLO = XF32 && PARTS == 2;

    auto x_at = [&](int r, int k) -> float {
        if (XF32) return static_cast<const float *>(xv)[(size_t)r * kD + k];
        return __uint_as_float((unsigned)static_cast<const uint16_t *>(xv)[(size_t)r * kD + k] << 16);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) acc[mt][kk] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int r0 = row_begin; r0 < row_end; r0 += 32) {
        {   // x: this thread's four columns 4 cq + 0..3 of the rows 8 xq + 0..7 (one 8- or 16-byte load per row)
            const int cq = tid & 63, xq = tid >> 6;
            float v[4][8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = r0 + 8 * xq + j;
                f32x4 t = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (r < row_end) {
                    if (XF32) {
                        const float4 w = *reinterpret_cast<const float4 *>(static_cast<const float *>(xv) + (size_t)r * kD + 4 * cq);
                        t = (f32x4){w.x, w.y, w.z, w.w};
                    } else {
                        t = unpack_bf16x4(*reinterpret_cast<const uint2 *>(static_cast<const uint16_t *>(xv) + (size_t)r * kD + 4 * cq));
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i][j] = t[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bf16x8 hi, lo;
                split8(v[i], hi, lo);
                const int k = 4 * cq + i, at = (k >> 4) * kFragShorts + (xq * 16 + (k & 15)) * 8;
                *reinterpret_cast<bf16x8 *>(xb[0] + at) = hi;
                if (XLO) *reinterpret_cast<bf16x8 *>(xb[1] + at) = lo;
            }
        }
        {   // Y: (s / n) g, or -(beta / (2 n2)) x
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = r0 + 8 * yq + j;
                v[j] = 0.f;
                if (r < row_end) {
                    const float n2 = n2v[r];
                    if (is_g) {
                        if (m0 + ml < classes) v[j] = (scale / sqrtf(n2)) * g[(size_t)r * classes + m0 + ml];
                    } else {
                        v[j] = -(beta[r] / (2.f * n2)) * x_at(r, m0 + ml);
                    }
                }
            }
            bf16x8 hi, lo;
            split8(v, hi, lo);
            const int at = (ml >> 4) * kFragShorts + (yq * 16 + (ml & 15)) * 8;
            *reinterpret_cast<bf16x8 *>(yb[0] + at) = hi;
            if (PARTS == 2) *reinterpret_cast<bf16x8 *>(yb[1] + at) = lo;
        }
        __syncthreads();
        bf16x8 bh[4], bl[XLO ? 4 : 1];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bh[kk] = *reinterpret_cast<const bf16x8 *>(xb[0] + (4 * wave + kk) * kFragShorts + lane * 8);
            if (XLO) bl[kk] = *reinterpret_cast<const bf16x8 *>(xb[1] + (4 * wave + kk) * kFragShorts + lane * 8);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const bf16x8 yh = *reinterpret_cast<const bf16x8 *>(yb[0] + mt * kFragShorts + lane * 8);
            if (PARTS == 2) {
                const bf16x8 yl = *reinterpret_cast<const bf16x8 *>(yb[1] + mt * kFragShorts + lane * 8);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[mt][kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yl, bh[kk], acc[mt][kk], 0, 0, 0);
            }
            if (XLO) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) acc[mt][kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, bl[XLO ? kk : 0], acc[mt][kk], 0, 0, 0);
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) acc[mt][kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(yh, bh[kk], acc[mt][kk], 0, 0, 0);
        }
        __syncthreads();
    }

    // rows m0 + 16 mt + 4 q + i of this group (classes, or classes + rows of dA), columns 16 (4 wave + kk) + c
    float *out = ws + (size_t)blockIdx.y * (size_t)(classes + kD) * kD;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = m0 + 16 * mt + 4 * q + i;
            if (is_g && m >= classes) continue;
            const size_t row = is_g ? m : classes + m;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) out[row * kD + 16 * (4 * wave + kk) + c] = acc[mt][kk][i];
        }
}

// the splits added in ascending order, four values per thread
__global__ void cls_head_reduce_kernel(const float *__restrict__ ws, int splits, long long n4, float *__restrict__ out)
{
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        float4 a = reinterpret_cast<const float4 *>(ws)[i];
        for (int s = 1; s < splits; ++s) {
            const float4 b = reinterpret_cast<const float4 *>(ws)[(long long)s * n4 + i];
            a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
        }
        reinterpret_cast<float4 *>(out)[i] = a;
    }
}

inline int n_splits(int tokens) { return (tokens + kSplitRows - 1) / kSplitRows; }

// what every entry point checks first: the name of the failing class of error, or MSDA_OK
int check_dims(int tokens, int d_model, int classes, int parts)
{
    if (tokens < 1 || d_model != kD || classes < 1 || classes > kMaxClasses || (parts != 1 && parts != 2)) return MSDA_ERR_BAD_DIMS;
    return MSDA_OK;
}

template <bool XF32, int PARTS>
int launch_forward(const void *x, const uint16_t *packed, int tokens, int classes, float scale, float *logits, float *n2, hipStream_t st)
{
    const int row_blocks = (tokens + kFwdTokWg - 1) / kFwdTokWg, groups = (class_tiles(classes) + 1) / 2;
    const int want = min(groups, max(1, kFillCus / row_blocks)), gpc = (groups + want - 1) / want, chunks = (groups + gpc - 1) / gpc;
    hipLaunchKernelGGL((cls_head_forward_kernel<XF32, PARTS>), dim3(row_blocks, chunks), dim3(kThreads), 0, st, x, packed, tokens, classes,
                       scale, gpc, logits, n2);
    return msda::launched("msda_cls_head_forward");
}

template <bool XF32, int PARTS>
int launch_rows(const float *g, const float *logits, const float *n2, const void *x, const uint16_t *packed, int tokens, int classes,
                float scale, void *dx, float *beta, hipStream_t st)
{
    const int vec = classes % 4 == 0 && msda::aligned(16, {g, logits});
    hipLaunchKernelGGL((cls_head_bwd_rows_kernel<XF32, PARTS>), dim3((tokens + kRowTokWg - 1) / kRowTokWg), dim3(kThreads), 0, st, g, logits,
                       n2, x, packed, tokens, classes, scale, vec, dx, beta);
    return msda::launched("msda_cls_head_backward_rows");
}

template <bool XF32, int PARTS>
int launch_weights(const float *g, const float *n2, const float *beta, const void *x, int tokens, int classes, float scale, float *ws,
                   float *dGA, hipStream_t st)
{
    const int groups = (classes + kGroupRows - 1) / kGroupRows + kD / kGroupRows, splits = n_splits(tokens);
    hipLaunchKernelGGL((cls_head_bwd_weights_kernel<XF32, PARTS>), dim3(groups, splits), dim3(kThreads), 0, st, g, n2, beta, x, tokens,
                       classes, scale, ws);
    const long long n4 = (long long)(classes + kD) * kD / 4;
    hipLaunchKernelGGL(cls_head_reduce_kernel, dim3((unsigned)min(1024LL, (n4 + 255) / 256)), dim3(256), 0, st, ws, splits, n4, dGA);
    return msda::launched("msda_cls_head_backward_weights");
}

// one of the four instances of a launcher template
#define CLS_HEAD_DISPATCH(fn, x_is_bf16, parts, ...)                                                          \
    ((x_is_bf16) ? ((parts) == 2 ? fn<false, 2>(__VA_ARGS__) : fn<false, 1>(__VA_ARGS__))                     \
                 : ((parts) == 2 ? fn<true, 2>(__VA_ARGS__) : fn<true, 1>(__VA_ARGS__)))

}  // namespace

extern "C" {

int msda_cls_head_packed_elems(int classes, int64_t *elems)
{
    if (!elems) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (classes < 1 || classes > kMaxClasses) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    *elems = (int64_t)(region1_shorts(classes) + (long long)class_steps(classes) * kStepShorts);
    return MSDA_OK;
}

int msda_cls_head_pack(const float *G, int classes, const float *A, int d_model, uint16_t *packed, msda_stream_t stream)
{
    if (!G || !A || !packed) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (classes < 1 || classes > kMaxClasses || d_model != kD) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    hipLaunchKernelGGL(cls_head_pack_kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream), G, classes, A, packed);
    return msda::launched(__func__);
}

int msda_cls_head_forward(const void *x, int x_is_bf16, const uint16_t *packed, int tokens, int d_model, int classes, float scale,
                          int parts, float *logits, float *n2, msda_stream_t stream)
{
    if (!x || !packed || !logits || !n2) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(tokens, d_model, classes, parts)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, packed}) || !msda::aligned(4, {logits, n2})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    return CLS_HEAD_DISPATCH(launch_forward, x_is_bf16, parts, x, packed, tokens, classes, scale, logits, n2, static_cast<hipStream_t>(stream));
}

int msda_cls_head_backward_rows(const float *g, const float *logits, const float *n2, const void *x, int x_is_bf16, const uint16_t *packed,
                                int tokens, int d_model, int classes, float scale, int parts, void *dx, float *beta, msda_stream_t stream)
{
    if (!g || !logits || !n2 || !x || !packed || !dx || !beta) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(tokens, d_model, classes, parts)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, packed, dx}) || !msda::aligned(4, {g, logits, n2, beta})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    return CLS_HEAD_DISPATCH(launch_rows, x_is_bf16, parts, g, logits, n2, x, packed, tokens, classes, scale, dx, beta,
                             static_cast<hipStream_t>(stream));
}

int msda_cls_head_workspace_bytes(int tokens, int classes, int64_t *bytes)
{
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(tokens, kD, classes, 2)) return msda::arg_fail(e, __func__);
    *bytes = (int64_t)n_splits(tokens) * (classes + kD) * kD * (int64_t)sizeof(float);
    return MSDA_OK;
}

int msda_cls_head_backward_weights(const float *g, const float *n2, const float *beta, const void *x, int x_is_bf16, int tokens, int d_model,
                                   int classes, float scale, int parts, void *workspace, float *dGA, msda_stream_t stream)
{
    if (!g || !n2 || !beta || !x || !workspace || !dGA) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (const int e = check_dims(tokens, d_model, classes, parts)) return msda::arg_fail(e, __func__);
    if (!msda::aligned(16, {x, workspace, dGA}) || !msda::aligned(4, {g, n2, beta})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    return CLS_HEAD_DISPATCH(launch_weights, x_is_bf16, parts, g, n2, beta, x, tokens, classes, scale, static_cast<float *>(workspace), dGA,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
