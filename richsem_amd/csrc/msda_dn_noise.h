// msda_dn_noise.h -- the floating-point part of the reference's contrastive-denoising set-up (prepare_for_cdn,
// models/richsem/dn_components.py:11-193) on the device, from the per-image target counts READ ON THE DEVICE: the noised labels and
// boxes, the label embedding, the padded query block and the self-attention mask in ONE launch, and the embedding table's gradient in
// one more.  Included by rows_api.hip.  (msda_dn.h keeps the integer layout for callers that take the counts on the host.)
//
//   group count        dn_components.py:27-41      from dn_number, max count and add_gt          -> meta
//   label noise        :58-64                      p < label_noise_ratio * 0.5 takes a random class
//   box noise          :73-90, :120-122            xyxy + rand_part * diff * scale, clamp, back to cxcywh
//   label_enc, inverse_sigmoid, scatter  :127-143  -> q_label (N, pad_cap, D), q_bbox (N, pad_cap, 4)
//   use_cdn=False      :146-153                    the positive halves only
//   attn_mask          :157-179                    -> (pad_cap + num_queries)^2 u8
//
// The buffers have a fixed capacity pad_cap >= pad_size; slots [pad_size, pad_cap) are zero rows that no query sees (their mask columns
// are set for every row) and that see the matching queries only (so their softmax rows are not empty).  Every element of every output is
// written by exactly one thread: no memset, no atomic, nothing read back, so the launch can be captured and a replay follows the current
// contents of cum / labels / boxes / uniform.
//
// Arithmetic: the box chain up to the cxcywh conversion is the reference's float32 operations one by one, with contraction switched off
// (a fused multiply-add would round once where torch rounds twice), so noised_box equals torch's bit for bit; inverse_sigmoid of it is
// taken in float64 and rounded once (dn_inverse_sigmoid).
//
// Launch: workgroups of 256 threads; the first `row_blocks` take kDnRows consecutive (image, slot) rows each -- one lane per row for the
// noise, one per coordinate for inverse_sigmoid, all lanes for the 16-byte pieces of the embedding rows --, the others 16 mask bytes per lane.  Every workgroup derives the layout
// (max count -> groups -> pad_size) from cum itself: N + 1 loads, no header kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace msda {

constexpr int kDnThreads = 256;
constexpr int kDnRows = 16;                       // (image, slot) rows per workgroup
constexpr int kDnMaskBytes = kDnThreads * 16;     // mask bytes per workgroup

struct DnParams {
    int N, pad_cap, D, V, num_classes, num_queries, dn_number, use_cdn, add_gt;
    long long target_cap;                         // rows of labels / boxes the caller owns
    float label_thr, box_noise_scale;             // label_thr = label_noise_ratio * 0.5
    int row_blocks;                               // workgroups of the row part; the mask part follows
};

struct DnLayout {
    long long single_pad, groups, pad_size, total;
    int overflow;
};

// dn_components.py:27-41, :65-67, :146-155 from the counts on the device.  Called by all threads of the workgroup.
__device__ __forceinline__ DnLayout dn_layout(const DnParams &p, const int64_t *__restrict__ cum, long long *red_s)
{
    const int tid = threadIdx.x;
    long long mx = 0;
    for (int b = tid; b < p.N; b += kDnThreads) mx = max(mx, (long long)(cum[b + 1] - cum[b]));
    red_s[tid] = mx;
    __syncthreads();
    for (int w = kDnThreads / 2; w > 0; w >>= 1) {
        if (tid < w) red_s[tid] = max(red_s[tid], red_s[tid + w]);
        __syncthreads();
    }
    DnLayout lay;
    lay.single_pad = red_s[0];
    lay.total = cum[p.N];
    long long g = 2ll * p.dn_number;
    if (lay.single_pad == 0) g = 1;
    else if (g >= 100) g = g / (lay.single_pad * 2);
    else if (g < 1) g = 1;
    if (g == 0) g = 1;
    if (p.add_gt) g += 1;
    lay.groups = g;
    long long pad = lay.single_pad * 2 * g;
    if (!p.use_cdn) pad /= 2;
    // a graph cannot raise: a layout that does not fit the buffers is reported and leaves every slot empty
    lay.overflow = (pad > p.pad_cap || lay.total > p.target_cap || lay.total < 0) ? 1 : 0;
    lay.pad_size = lay.overflow ? 0 : pad;
    return lay;
}

// util/misc.py:605-609 with eps = 1e-3, the quotient and the logarithm in float64: 1 - x is then exact and the float32 result is the
// correctly rounded one up to float64's own error -- torch's float32 chain (1 - x, x1 / x2 and logf, a rounding each) is up to
// 1.5 * 2^-24 + logf's error away from it, which near x = 0.5, where the result is small, is many of its ulps
__device__ __forceinline__ float dn_inverse_sigmoid(float x)
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const double eps = (double)1e-3f;
    const double x1 = fmax((double)x, eps), x2 = fmax(1.0 - (double)x, eps);
    return (float)log(x1 / x2);
}

// one coordinate of dn_components.py:89-90, :120: pre + (rand_part * diff) * scale, clamped -- three roundings, as torch's three kernels
__device__ __forceinline__ float dn_noised_corner(float pre, float rand_part, float diff, float scale)
{
#pragma clang fp contract(off)
    const float m = rand_part * diff;
    const float ms = m * scale;
    const float v = pre + ms;
    return fminf(fmaxf(v, 0.f), 1.f);
}

__global__ __launch_bounds__(kDnThreads) void dn_queries_kernel(const DnParams p, const int64_t *__restrict__ cum,
                                                                const int64_t *__restrict__ labels, const float *__restrict__ boxes,
                                                                const float *__restrict__ uniform, const float *__restrict__ table,
                                                                float *__restrict__ q_label, float *__restrict__ q_bbox,
                                                                int64_t *__restrict__ noised_label, float *__restrict__ noised_box,
                                                                uint8_t *__restrict__ attn_mask, int64_t *__restrict__ meta)
{
#pragma clang fp contract(off)      // every float32 operation below rounds on its own, as torch's element-wise kernels do
    __shared__ long long red_s[kDnThreads];
    __shared__ long long lab_s[kDnRows];
    __shared__ float4 box_s[kDnRows];      // the rows' noised boxes
    __shared__ int fill_s[kDnRows];        // is the row's slot filled?
    const int tid = threadIdx.x;
    const DnLayout lay = dn_layout(p, cum, red_s);
    if (blockIdx.x == 0 && tid == 0) {
        meta[0] = lay.single_pad, meta[1] = lay.groups, meta[2] = lay.pad_size, meta[3] = lay.total, meta[4] = lay.overflow;
    }

    if ((int)blockIdx.x < p.row_blocks) {
        const int rows = p.N * p.pad_cap, row0 = (int)blockIdx.x * kDnRows;      // (N * pad_cap < 2^31: checked on the host)
        const int nrows = min(kDnRows, rows - row0);
        if (tid < nrows) {
            const int row = row0 + tid;
            const int b = row / p.pad_cap, s = row - b * p.pad_cap;
            long long lab = -1;
            float4 nb = make_float4(0.f, 0.f, 0.f, 0.f);
            bool filled = false;
            if (s < lay.pad_size) {      // (0 < single_pad <= pad_size <= pad_cap here: int arithmetic)
                const int single = (int)lay.single_pad, gi = s / single, j = s - gi * single;
                const int g2 = p.use_cdn ? gi : 2 * gi;      // the group-half: even = positive, odd = negative
                const long long c0 = cum[b], t = c0 + j;
                if (j < cum[b + 1] - c0 && t >= 0 && t < p.target_cap) {
                    const float *u = uniform + (long long)row * 10;
                    const bool keep_gt = p.add_gt && g2 == 0;      // :60-61, :86-87
                    lab = labels[t];
                    if (!keep_gt && u[0] < p.label_thr) lab = min((int)floorf(u[1] * (float)p.num_classes), p.num_classes - 1);
                    const float4 bx = reinterpret_cast<const float4 *>(boxes)[t];
                    nb = bx;
                    if (p.box_noise_scale > 0.f) {
                        const float hw = bx.z / 2.f, hh = bx.w / 2.f;
                        const float pre[4] = {bx.x - hw, bx.y - hh, bx.x + hw, bx.y + hh}, diff[4] = {hw, hh, hw, hh};
                        float c[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float part = (g2 & 1) ? u[6 + k] + 1.f : u[6 + k];
                            const float rp = keep_gt ? 0.f : part * (u[2 + k] < 0.5f ? -1.f : 1.f);
                            c[k] = dn_noised_corner(pre[k], rp, diff[k], p.box_noise_scale);
                        }
                        nb = make_float4((c[0] + c[2]) / 2.f, (c[1] + c[3]) / 2.f, c[2] - c[0], c[3] - c[1]);
                    }
                    filled = true;
                }
            }
            noised_label[row] = lab;
            box_s[tid] = nb, fill_s[tid] = filled;
            if (noised_box) reinterpret_cast<float4 *>(noised_box)[row] = nb;
            lab_s[tid] = (lab >= 0 && lab < p.V) ? lab : -1;      // a label outside the table embeds as a zero row
        }
        __syncthreads();
        if (tid < 4 * nrows) {
            const float x = reinterpret_cast<const float *>(box_s)[tid];
            q_bbox[(long long)row0 * 4 + tid] = fill_s[tid >> 2] ? dn_inverse_sigmoid(x) : 0.f;
        }
        const int d4 = p.D / 4;
        const float4 *tab = reinterpret_cast<const float4 *>(table);
        float4 *out = reinterpret_cast<float4 *>(q_label) + (long long)row0 * d4;
        for (int i = tid; i < nrows * d4; i += kDnThreads) {
            const int r = i / d4, c = i - r * d4;
            const long long lab = lab_s[r];
            out[i] = lab >= 0 ? tab[lab * d4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }

    // ---- the mask: 16 consecutive bytes of the row-major (T, T) matrix per lane ----
    const long long T = (long long)p.pad_cap + p.num_queries, n = T * T;
    const long long i0 = ((long long)((int)blockIdx.x - p.row_blocks) * kDnThreads + tid) * 16;
    if (i0 >= n) return;
    const int Ti = (int)T, pad = (int)lay.pad_size, group_pad = (int)(p.use_cdn ? 2 * lay.single_pad : lay.single_pad);      // (T < 2^31)
    int r = (int)(i0 / T), c = (int)(i0 - (long long)r * T);
    int lo = 0, hi = 0;      // the columns of row r's own denoising group (rows of the block only)
    if (r < pad) lo = r / group_pad * group_pad, hi = lo + group_pad;
    union { uint4 v; uint8_t b[16]; } pack;
    const int cnt = (int)min(16ll, n - i0);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        uint8_t m = 0;
        if (c < p.pad_cap) m = (c >= pad || r >= pad || c < lo || c >= hi) ? 1 : 0;      // a tail column; a matching query or a tail row looking
                                                                                          // at the block; another denoising group
        pack.b[k] = m;
        if (++c == Ti) {
            c = 0, ++r;
            if (r < pad) lo = r / group_pad * group_pad, hi = lo + group_pad;
        }
    }
    if (cnt == 16) reinterpret_cast<uint4 *>(attn_mask)[i0 / 16] = pack.v;
    else
        for (int k = 0; k < cnt; ++k) attn_mask[i0 + k] = pack.b[k];
}

// grad_table[v] = the sum over rows r (in ascending order) with noised_label[r] == v of grad_q_label[r]: one wave per table row finds its
// rows 64 at a time with a ballot and adds them one after the other, so the result does not depend on anything but the inputs; rows
// nobody hits are written as zeros.
__global__ __launch_bounds__(kDnThreads) void dn_queries_backward_kernel(const float *__restrict__ grad_q_label,
                                                                         const int64_t *__restrict__ noised_label, long long rows, int D,
                                                                         int V, float *__restrict__ grad_table)
{
    const int lane = threadIdx.x & 63;
    const long long v = (long long)blockIdx.x * (kDnThreads / 64) + (threadIdx.x >> 6);
    if (v >= V) return;      // (wave-uniform)
    const int d4 = D / 4;
    const float4 *g = reinterpret_cast<const float4 *>(grad_q_label);
    float4 *out = reinterpret_cast<float4 *>(grad_table) + v * d4;
    for (int c0 = 0; c0 < d4; c0 += 64) {
        const int c = c0 + lane;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (long long base = 0; base < rows; base += 64) {
            const long long r = base + lane;
            unsigned long long hits = __ballot(r < rows && noised_label[r] == v);
            while (hits) {
                const int i = __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                if (c < d4) {
                    const float4 x = g[(base + i) * d4 + c];
                    acc.x += x.x, acc.y += x.y, acc.z += x.z, acc.w += x.w;
                }
            }
        }
        if (c < d4) out[c] = acc;
    }
}

}  // namespace msda
