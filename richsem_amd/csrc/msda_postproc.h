// msda_postproc.h -- the detector's PostProcess (reference models/richsem/richsem.py:1309-1367) on the device: exact top-k over the
// flattened query x class axis of a long row, fused with the decode of the winners, and the NMS of the selected boxes.
//
// Selection (one row per image, n = Q * C up to 2^31 - 1 elements, k <= 1024):
//   The order is that of the LOGITS (sigmoid is monotone; only the k winners get one), as order-preserving 32-bit keys: float
//   comparison, -0.0 == +0.0, every NaN above +inf; equal keys lowest flat index first.  So the result is a function of the input alone.
//   * three radix-select rounds (11 + 11 + 10 bits): every workgroup counts the digits of its chunk of 8192 elements in LDS and adds
//     the non-empty bins to the image's histogram with vector atomics; the LAST workgroup to take the round's ticket resolves the
//     digit (state: the known prefix of the k-th largest key and how many elements of that prefix are still wanted);
//   * one compaction pass: every element above the threshold goes to the image's candidate list; of the elements equal to it every
//     chunk records its count and the indices of its first 16, in index order.  The last workgroup to arrive takes a prefix over the
//     chunks' counts, so it knows which chunks hold the first `need` equal elements and how many each contributes; it takes them from
//     the chunks' records, or -- where one chunk contributes more than 16 -- reads that chunk again (at most need / 17 chunks), sorts
//     the <= 1024 candidates by (key descending, index ascending) with a bitonic network and writes score, label, box and query index.
//   Nothing ever waits for another workgroup: a ticket is an atomic counter that is incremented once and never polled.  Histograms,
//   tickets and counters are zeroed by the first launch of every call (pp_zero_kernel), so a replayed graph or a second call on the
//   same workspace starts clean whatever the previous one left.
//
// NMS (one workgroup per image, K <= 1024 boxes in descending score order): the K x K suppression bits ("i suppresses j", j > i) in
// LDS (128 KB at K = 1024), then the greedy sweep in one wave, 64 boxes per step.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msda {

constexpr int kPpThreads = 1024;
constexpr int kPpPerThread = 8;
constexpr int kPpChunk = kPpThreads * kPpPerThread;      // elements of a row one workgroup reads
constexpr int kPpMaxK = 1024;
constexpr int kPpBins = 2048;
constexpr int kPpRounds = 3;
// workspace, in 32-bit words: [B][kPpZeroWords] zeroed per call (3 histograms, then the state), [B][2 * kPpMaxK] candidates (keys, then
// indices), [B][chunks] per-chunk counts of the elements equal to the threshold, [B][chunks][kPpEqSlots] the first of their indices
constexpr int kPpEqSlots = 16;      // per chunk: the indices of its first 16 elements equal to the threshold
constexpr int kPpStateWords = 16;
constexpr int kPpZeroWords = kPpRounds * kPpBins + kPpStateWords;
enum { kPpPrefix = 0, kPpNeed = 1, kPpTicket = 2 /* + round; + kPpRounds: the compaction's */, kPpCount = 6 };

constexpr int kNmsMaxK = 1024;

// chunks of a row: its first element may sit up to 7 elements behind a 16-byte boundary (the chunks are cut at aligned addresses)
inline int pp_chunks(int64_t n) { return (int)((n + 7 + kPpChunk - 1) / kPpChunk); }

__device__ __forceinline__ unsigned pp_key(unsigned u)      // bits of a float -> key; ascending float order = ascending unsigned order
{
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;      // NaN: above +inf, as torch.topk
    if (u == 0x80000000u) u = 0u;                                  // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool BF16>
__device__ __forceinline__ unsigned pp_load_bits(const void *row, long long i)
{
    return BF16 ? (unsigned)static_cast<const uint16_t *>(row)[i] << 16 : static_cast<const unsigned *>(row)[i];
}

// f(key, index) for every element of chunk `chunk` of the row: 16-byte loads where the whole vector lies inside the row, element loads
// at its two ends (a row of an odd length starts and ends off the vector grid)
template <bool BF16, typename F>
__device__ __forceinline__ void pp_for_chunk(const void *row, int n, int chunk, F &&f)
{
    constexpr int V = BF16 ? 8 : 4, ES = BF16 ? 2 : 4;
    const int off = (int)((reinterpret_cast<uintptr_t>(row) & 15) / ES);
#pragma unroll
    for (int v = 0; v < kPpPerThread / V; ++v) {
        const long long i0 = (long long)chunk * kPpChunk + (long long)threadIdx.x * kPpPerThread + v * V - off;      // (a thread: 8 consecutive elements)
        if (i0 >= n || i0 + V <= 0) continue;
        if (i0 >= 0 && i0 + V <= n) {
            const uint4 q = *reinterpret_cast<const uint4 *>(static_cast<const char *>(row) + i0 * ES);
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const unsigned bits = BF16 ? ((e & 1) ? (w[e >> 1] & 0xFFFF0000u) : (w[e >> 1] << 16)) : w[e & 3];
                f(pp_key(bits), (int)(i0 + e));
            }
        } else {
            for (int e = 0; e < V; ++e)
                if (i0 + e >= 0 && i0 + e < n) f(pp_key(pp_load_bits<BF16>(row, i0 + e)), (int)(i0 + e));
        }
    }
}

__device__ __forceinline__ unsigned pp_peek(const unsigned *p)      // what another workgroup of this launch wrote (after the ticket's fence)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive prefix of v over the workgroup's 1024 threads (in thread order); total = the sum.  scan: 16 words of LDS
__device__ __forceinline__ unsigned pp_block_scan(unsigned v, unsigned *scan, unsigned &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
    unsigned before = 0u, sum = 0u;
#pragma unroll
    for (int w = 0; w < kPpThreads / 64; ++w) {
        const unsigned t = scan[w];
        before += w < wave ? t : 0u;
        sum += t;
    }
    total = sum;
    __syncthreads();
    return before + incl - v;
}

// true in every thread of the one workgroup that takes the last of an image's `count` tickets; what the others wrote before they took
// theirs is visible to it afterwards.  One thread fences for the workgroup: the barrier orders every thread's stores before it, and its
// device-scope release covers them (fences are cumulative).  A fence in every wave costs an L2 write-back per wave on this multi-die
// part: 16 x 266 of them made these kernels three to five times slower (profiles/r09_postprocess.md, "Where the time goes").
__device__ __forceinline__ bool pp_last_arriver(unsigned *ticket, unsigned count, int *s_last)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        *s_last = atomicAdd(ticket, 1u) == count - 1u;
    }
    __syncthreads();
    const bool last = *s_last != 0;
    if (last) __threadfence();
    return last;
}

// histograms, tickets and counters of every image start a call at zero (a kernel, not a memset node: plain vector stores on the stream)
__global__ __launch_bounds__(kPpThreads) void pp_zero_kernel(unsigned *__restrict__ ws, int words)
{
    const int i = blockIdx.x * kPpThreads + threadIdx.x;
    if (i < words) ws[i] = 0u;
}

template <bool BF16>
__global__ __launch_bounds__(kPpThreads) void pp_hist_kernel(const void *__restrict__ logits, int n, int k, int nchunks, int round,
                                                             unsigned *__restrict__ ws)
{
    __shared__ unsigned lh[kPpBins];
    __shared__ unsigned scan[kPpThreads / 64];
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x / nchunks, chunk = blockIdx.x - b * nchunks;      // (a flat grid: image-major)
    unsigned *img = ws + (size_t)b * kPpZeroWords, *gh = img + round * kPpBins, *state = img + kPpRounds * kPpBins;
    const void *row = static_cast<const char *>(logits) + (size_t)b * n * (BF16 ? 2 : 4);
    for (int i = tid; i < kPpBins; i += kPpThreads) lh[i] = 0u;
    // bits [shift, shift + 11 | 10) of the keys whose bits above them equal the prefix the earlier rounds found
    const int shift = round == 0 ? 21 : (round == 1 ? 10 : 0);
    const unsigned hi_mask = round == 0 ? 0u : (round == 1 ? 0xFFE00000u : 0xFFFFFC00u), digit_mask = round == 2 ? 1023u : 2047u;
    const unsigned prefix = state[kPpPrefix], need = round == 0 ? (unsigned)k : state[kPpNeed];
    __syncthreads();
    pp_for_chunk<BF16>(row, n, chunk, [&](unsigned key, int) {
        if ((key & hi_mask) == prefix) atomicAdd(&lh[(key >> shift) & digit_mask], 1u);
    });
    __syncthreads();
    for (int i = tid; i < kPpBins; i += kPpThreads) {
        const unsigned c = lh[i];
        if (c) atomicAdd(&gh[i], c);
    }
    if (!pp_last_arriver(&state[kPpTicket + round], (unsigned)nchunks, &s_last)) return;
    // digits from the top: the first one at which the running count reaches `need` holds the k-th largest key.  Thread t: bins 2047 - 2t, 2046 - 2t
    const int b0 = kPpBins - 1 - 2 * tid;
    const unsigned h0 = pp_peek(&gh[b0]), h1 = pp_peek(&gh[b0 - 1]);
    unsigned total;
    const unsigned excl = pp_block_scan(h0 + h1, scan, total);
    if (excl < need && need <= excl + h0 + h1) {
        const bool first = need <= excl + h0;
        state[kPpPrefix] = prefix | (unsigned)(first ? b0 : b0 - 1) << shift;
        state[kPpNeed] = first ? need - excl : need - excl - h0;
    }
}

// reference util/box_ops.py:9-13 (box_cxcywh_to_xyxy), richsem.py:1342-1354 (test: x2 - x1; the scale by (w, h, w, h)); every operation
// rounded on its own, as the float32 tensor operations of the reference are
__device__ __forceinline__ float4 pp_decode_box(float4 c, int box_mode, float img_h, float img_w)
{
    float4 r = c;
    if (box_mode != 0) {
        const float hw = __fmul_rn(0.5f, c.z), hh = __fmul_rn(0.5f, c.w);
        r = make_float4(__fsub_rn(c.x, hw), __fsub_rn(c.y, hh), __fadd_rn(c.x, hw), __fadd_rn(c.y, hh));
        if (box_mode == 2) {
            r.z = __fsub_rn(r.z, r.x);
            r.w = __fsub_rn(r.w, r.y);
        }
    }
    return make_float4(__fmul_rn(r.x, img_w), __fmul_rn(r.y, img_h), __fmul_rn(r.z, img_w), __fmul_rn(r.w, img_h));
}

template <bool BF16>
__global__ __launch_bounds__(kPpThreads) void pp_compact_kernel(const void *__restrict__ logits, const float *__restrict__ boxes,
                                                                const float *__restrict__ sizes_hw, int Q, int C, int k, int nchunks,
                                                                int box_mode, unsigned *__restrict__ ws, unsigned *__restrict__ cand,
                                                                unsigned *__restrict__ chunk_eq, unsigned *__restrict__ eq_slots,
                                                                float *__restrict__ scores,
                                                                int64_t *__restrict__ labels, float *__restrict__ out_boxes,
                                                                int64_t *__restrict__ query_idx)
{
    __shared__ unsigned ckey[kPpMaxK];
    __shared__ int cidx[kPpMaxK];
    __shared__ unsigned scan[kPpThreads / 64];
    __shared__ int wl_chunk[kPpMaxK];
    __shared__ unsigned wl_before[kPpMaxK], wl_count[kPpMaxK];
    __shared__ unsigned s_eq, s_nwl;
    __shared__ int s_last;
    const int tid = threadIdx.x, b = blockIdx.x / nchunks, chunk = blockIdx.x - b * nchunks, n = Q * C;
    unsigned *state = ws + (size_t)b * kPpZeroWords + kPpRounds * kPpBins;
    unsigned *gkey = cand + (size_t)b * 2 * kPpMaxK, *gidx = gkey + kPpMaxK, *geq = chunk_eq + (size_t)b * nchunks;
    unsigned *gslots = eq_slots + (size_t)b * nchunks * kPpEqSlots;
    const void *row = static_cast<const char *>(logits) + (size_t)b * n * (BF16 ? 2 : 4);
    const unsigned thr = state[kPpPrefix], need = state[kPpNeed];      // key of the k-th largest; how many of the elements equal to it belong to the top k
    if (tid == 0) { s_eq = 0u; s_nwl = 0u; }
    __syncthreads();
    constexpr int ES = BF16 ? 2 : 4;
    const int off = (int)((reinterpret_cast<uintptr_t>(row) & 15) / ES);
    const long long mine0 = (long long)chunk * kPpChunk + (long long)tid * kPpPerThread - off;      // index of this thread's first element
    unsigned eq_mask = 0u;
    pp_for_chunk<BF16>(row, n, chunk, [&](unsigned key, int i) {
        if (key > thr) {
            const unsigned slot = atomicAdd(&state[kPpCount], 1u);      // (k - need of them in all: fewer than kPpMaxK)
            if (slot < (unsigned)kPpMaxK) {
                gkey[slot] = key;
                gidx[slot] = (unsigned)i;
            }
        } else if (key == thr) {
            eq_mask |= 1u << (int)(i - mine0);
        }
    });
    const unsigned eq = __popc(eq_mask);
    if (eq) atomicAdd(&s_eq, eq);
    __syncthreads();
    if (tid == 0) geq[chunk] = s_eq;
    if (s_eq) {      // (workgroup-uniform) the chunk's first kPpEqSlots elements equal to the threshold, in index order
        unsigned total;
        unsigned rank = pp_block_scan(eq, scan, total);
        for (unsigned m = eq_mask; m && rank < (unsigned)kPpEqSlots; m &= m - 1u, ++rank)
            gslots[(size_t)chunk * kPpEqSlots + rank] = (unsigned)(mine0 + (__ffs(m) - 1));
    }
    if (!pp_last_arriver(&state[kPpTicket + kPpRounds], (unsigned)nchunks, &s_last)) return;

    // ---- the image's last workgroup: the candidates above the threshold ...
    const unsigned above = (unsigned)k - need;
    if ((unsigned)tid < above) {
        ckey[tid] = pp_peek(&gkey[tid]);
        cidx[tid] = (int)pp_peek(&gidx[tid]);
    } else {      // (padding sorts to the end)
        ckey[tid] = 0u;
        cidx[tid] = 0x7FFFFFFF;
    }
    // ... the chunks that hold the first `need` elements equal to it, each with the number of such elements before it ...
    unsigned before = 0u;
    for (int base = 0; base < nchunks && before < need; base += kPpThreads) {
        const int c = base + tid;
        const unsigned e = c < nchunks ? pp_peek(&geq[c]) : 0u;
        unsigned total;
        const unsigned mine = before + pp_block_scan(e, scan, total);
        if (e && mine < need) {      // (at most `need` chunks: every one of them holds an element of the first `need`)
            const unsigned slot = atomicAdd(&s_nwl, 1u);
            if (slot < (unsigned)kPpMaxK) {
                wl_chunk[slot] = c;
                wl_before[slot] = mine;
                wl_count[slot] = min(e, need - mine);      // how many of the chunk's equal elements belong to the top k
            }
        }
        before += total;
    }
    __syncthreads();
    const unsigned nwl = min(s_nwl, (unsigned)kPpMaxK);
    // ... and those elements, in index order: from the chunk's slots where they suffice (a thread per chunk) ...
    if ((unsigned)tid < nwl && wl_count[tid] <= (unsigned)kPpEqSlots) {
        const unsigned at = above + wl_before[tid];
        for (unsigned j = 0; j < wl_count[tid]; ++j) {
            ckey[at + j] = thr;
            cidx[at + j] = (int)pp_peek(&gslots[(size_t)wl_chunk[tid] * kPpEqSlots + j]);
        }
        wl_chunk[tid] = -1;
    }
    __syncthreads();
    // ... by reading the chunk again where a chunk holds more of them (a thread: its 8 consecutive elements)
    for (unsigned w = 0; w < nwl; ++w) {
        if (wl_chunk[w] < 0) continue;
        const long long i0 = (long long)wl_chunk[w] * kPpChunk + (long long)tid * kPpPerThread - off;
        unsigned keys[kPpPerThread], cnt = 0u;
#pragma unroll
        for (int e = 0; e < kPpPerThread; ++e) {
            const bool in = i0 + e >= 0 && i0 + e < n;
            keys[e] = in ? pp_key(pp_load_bits<BF16>(row, i0 + e)) : 0u;
            cnt += in && keys[e] == thr ? 1u : 0u;
        }
        unsigned total;
        unsigned rank = wl_before[w] + pp_block_scan(cnt, scan, total);
#pragma unroll
        for (int e = 0; e < kPpPerThread; ++e)
            if (i0 + e >= 0 && i0 + e < n && keys[e] == thr) {
                if (rank < need) {
                    ckey[above + rank] = thr;
                    cidx[above + rank] = (int)(i0 + e);
                }
                ++rank;
            }
    }
    __syncthreads();

    // ---- bitonic sort of the 1024 (key, index) pairs: key descending, index ascending
    for (int size = 2; size <= kPpMaxK; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int a = tid, o = tid ^ stride;
            if (o > a) {
                const unsigned ka = ckey[a], ko = ckey[o];
                const int ia = cidx[a], io = cidx[o];
                const bool a_first = ka > ko || (ka == ko && ia < io);
                const bool up = (a & size) == 0;
                if (up != a_first) {
                    ckey[a] = ko; ckey[o] = ka;
                    cidx[a] = io; cidx[o] = ia;
                }
            }
            __syncthreads();
        }
    if (tid < k) {
        const int idx = min(cidx[tid], n - 1), q = idx / C;      // (the k first are elements of the row: the clamp only keeps a broken invariant inside it)
        const size_t o = (size_t)b * k + tid;
        const float x = __uint_as_float(pp_load_bits<BF16>(row, idx));
        scores[o] = 1.f / (1.f + expf(-x));
        labels[o] = idx - q * C;
        query_idx[o] = q;
        const float4 box = reinterpret_cast<const float4 *>(boxes)[(size_t)b * Q + q];
        reinterpret_cast<float4 *>(out_boxes)[o] = pp_decode_box(box, box_mode, sizes_hw[2 * b], sizes_hw[2 * b + 1]);
    }
}

// ---- NMS -------------------------------------------------------------------------------------------------------------------------------
inline size_t nms_lds_bytes(int K)
{
    const size_t kw = (size_t)(K + 63) / 64;
    return (((size_t)K * kw * 8 + 15) & ~(size_t)15) + (size_t)K * 16 + (size_t)K * 8 + 16 * 8;
}

__device__ __forceinline__ unsigned long long nms_readlane64(unsigned long long v, int lane)      // lane: wave-uniform
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(v >> 32), lane);
    return (unsigned long long)hi << 32 | lo;
}

// torchvision.ops.nms on boxes that are already in descending score order (so the kept positions come out ascending): box i, if kept,
// suppresses every later j with inter / (area_i + area_j - inter) > thr in float32 (a 0 / 0 is NaN and suppresses nothing); with
// `labels` only where labels[i] == labels[j] (batched_nms).  A NaN coordinate: fmaxf(.., 0.f) below drops the NaN where torch's
// clamp(min=0) propagates it; the pair is not suppressed either way for thr >= 0 (0 and NaN are both not above it), and only for those
__global__ __launch_bounds__(kNmsMaxK) void nms_kernel(const float *__restrict__ boxes, const int64_t *__restrict__ labels, int K, float thr,
                                                       uint8_t *__restrict__ keep, int64_t *__restrict__ kept_idx, int32_t *__restrict__ n_kept)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nms_smem[];
    typedef unsigned long long u64;
    const int KW = (K + 63) >> 6, tid = threadIdx.x, b = blockIdx.x;
    u64 *mat = reinterpret_cast<u64 *>(nms_smem);                                                               // [K][KW]: bit j of row i = i suppresses j
    float4 *bx = reinterpret_cast<float4 *>(nms_smem + (((size_t)K * KW * 8 + 15) & ~(size_t)15));              // [K]
    int64_t *lb = reinterpret_cast<int64_t *>(bx + K);                                                          // [K]
    u64 *keepw = reinterpret_cast<u64 *>(lb + K);                                                               // [16]
    for (int i = tid; i < K; i += kNmsMaxK) {
        bx[i] = reinterpret_cast<const float4 *>(boxes)[(size_t)b * K + i];
        lb[i] = labels ? labels[(size_t)b * K + i] : 0;
    }
    __syncthreads();
    for (int word = tid; word < K * KW; word += kNmsMaxK) {
        const int i = word / KW, w = word - i * KW;
        u64 bits = 0;
        if (64 * w + 63 > i) {
            const float4 a = bx[i];
            const float area_a = __fmul_rn(__fsub_rn(a.z, a.x), __fsub_rn(a.w, a.y));
            const int64_t la = lb[i];
            const int j1 = min(64 * w + 64, K);
            for (int j = max(64 * w, i + 1); j < j1; ++j) {
                if (lb[j] != la) continue;
                const float4 c = bx[j];
                const float iw = fmaxf(__fsub_rn(fminf(a.z, c.z), fmaxf(a.x, c.x)), 0.f), ih = fmaxf(__fsub_rn(fminf(a.w, c.w), fmaxf(a.y, c.y)), 0.f);
                const float inter = __fmul_rn(iw, ih);
                if (inter > 0.f || thr < 0.f) {      // (an empty intersection gives 0, -0 or NaN: never above a threshold >= 0)
                    const float area_c = __fmul_rn(__fsub_rn(c.z, c.x), __fsub_rn(c.w, c.y));
                    const float uni = __fsub_rn(__fadd_rn(area_a, area_c), inter);
                    if (__fdiv_rn(inter, uni) > thr) bits |= (u64)1 << (j - 64 * w);
                }
            }
        }
        mat[word] = bits;
    }
    __syncthreads();
    if (tid < 64) {      // the greedy sweep: lane l carries word l of the "suppressed" bits
        u64 rem = 0;
        for (int wb = 0; wb < KW; ++wb) {
            u64 cur = nms_readlane64(rem, wb);
            const int r = 64 * wb + tid;
            const u64 diag = r < K ? mat[r * KW + wb] : 0;
            for (int j = 0; j < 64; ++j)      // inside the block of 64: box j, if it survived the earlier ones, suppresses its later ones
                if (!((cur >> j) & 1)) cur |= nms_readlane64(diag, j);
            const int valid = min(64, K - 64 * wb);
            const u64 kept = ~cur & (valid == 64 ? ~(u64)0 : ((u64)1 << valid) - 1);
            if (tid == 0) keepw[wb] = kept;
            for (int j = 0; j < valid; ++j)
                if (((kept >> j) & 1) && tid > wb && tid < KW) rem |= mat[(64 * wb + j) * KW + tid];
        }
    }
    __syncthreads();
    int total = 0;
    for (int w = 0; w < KW; ++w) total += __popcll(keepw[w]);
    for (int i = tid; i < K; i += kNmsMaxK) {
        const int w = i >> 6, bit = i & 63;
        const u64 kw = keepw[w];
        const bool kept = (kw >> bit) & 1;
        keep[(size_t)b * K + i] = kept ? 1 : 0;
        if (kept) {
            int pos = __popcll(kw & (((u64)1 << bit) - 1));
            for (int v = 0; v < w; ++v) pos += __popcll(keepw[v]);
            kept_idx[(size_t)b * K + pos] = i;
        }
        if (i >= total) kept_idx[(size_t)b * K + i] = -1;
    }
    if (tid == 0) n_kept[b] = total;
}

}  // namespace msda
