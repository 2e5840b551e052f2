// msda_roi_targets.h -- ROIAlign forward of the TARGET boxes over capacity buffers: what clip_box_targets (richsem_amd/modules/attnpool.py;
// reference models/richsem/richsem.py:745-761) pools from the frozen CLIP feature map, with the boxes, their images and their count read
// on the device -- the target prefix `cum`, the (capacity, 4) box buffer and the (N, 2) image sizes -- so that one captured launch serves
// every batch that fits the capacity.  Included by distill_api.hip.
//
// Slot t in 0..capacity is live iff t < cum[N]; its image is the b with cum[b] <= t < cum[b + 1].  A dead slot is written as exact zeros and
// reads nothing through its box.  A prefix that does not start at 0, decreases or exceeds the capacity leaves every slot dead and sets
// status[3] (the convention of msda_criterion_pairs_f32; the other three words are written as 0).
//
// Arithmetic of a live slot: the pixel box is formed with the float32 roundings clip_box_targets makes in torch, one per operation and no
// contraction -- hw = 0.5 * w, cx -+ hw, times the image's width (height) --, then the algorithm of msda_roi.h (aligned = true: scaled by
// spatial_scale, shifted by -0.5; a bin averages sampling_ratio^2, or ceil(roi / bins)^2, bilinear samples).  Two refusals keep a launch
// finite whatever the box buffer holds: a live slot whose pixel box is not finite, or whose sampling grid would exceed kRoiTgtMaxGrid (msda_roi.h) per
// axis, is written as zeros (a normalised box inside its image never comes near either).
//
// Mapping: a workgroup per (slot, chunk of kRoiTgtChunk channels); thread = (bin, channel lane): consecutive threads own consecutive bins,
// the next channel lane the next channel, so a workgroup's stores are contiguous.  A thread resolves its bin's geometry once, outside the
// channel loop.  Liveness is uniform over the workgroup: a dead one leaves after one load of cum[N] and its zero stores (16-byte stores
// between a scalar head and tail).  No atomic: workgroup 0 writes the status.
#pragma once

#include <stdint.h>

#include "msda_common.h"
#include "msda_roi.h"

namespace msda {

constexpr int kRoiTgtThreads = 256;
constexpr int kRoiTgtChunk = 64;          // channels per workgroup
constexpr int kRoiTgtMaxImages = 1024;    // cum is kept in LDS

struct RoiTgtArgs {
    const float *input;
    const int64_t *cum;
    const float *tgt_boxes;
    const int32_t *sizes;
    int N, C, H, W, PH, PW, sampling_ratio;
    int64_t cap;
    float spatial_scale;
    float *output;
    int32_t *status;
};

// n zeros at p: scalar stores up to the first 16-byte boundary, float4 stores, a scalar tail (the whole workgroup takes part)
__device__ __forceinline__ void roi_tgt_zero(float *p, int64_t n, int tid, int nthreads)
{
    int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const int64_t n4 = (n - head) >> 2;
    if (tid < head) p[tid] = 0.f;
    float4 *p4 = reinterpret_cast<float4 *>(p + head);
    for (int64_t i = tid; i < n4; i += nthreads) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t i = head + 4 * n4 + tid; i < n; i += nthreads) p[i] = 0.f;
}

// the pixel box (x1, y1, x2, y2) of a normalised cxcywh box in an image of (h, w) pixels: clip_box_targets' float32 operations one by one
__device__ __forceinline__ float4 roi_tgt_pixel_box(float4 c, float img_h, float img_w)
{
    const float hw = __fmul_rn(0.5f, c.z), hh = __fmul_rn(0.5f, c.w);
    return make_float4(__fmul_rn(img_w, __fsub_rn(c.x, hw)), __fmul_rn(img_h, __fsub_rn(c.y, hh)), __fmul_rn(img_w, __fadd_rn(c.x, hw)),
                       __fmul_rn(img_h, __fadd_rn(c.y, hh)));
}

__global__ __launch_bounds__(kRoiTgtThreads) void roi_align_targets_kernel(RoiTgtArgs a)
{
    __shared__ int64_t s_cum[kRoiTgtMaxImages + 1];
    __shared__ int s_bad;
    const int tid = threadIdx.x, N = a.N;
    const int chunks = (a.C + kRoiTgtChunk - 1) / kRoiTgtChunk;
    const int64_t t = blockIdx.x / chunks;
    const int c0 = (int)(blockIdx.x - t * chunks) * kRoiTgtChunk;
    const int c1 = c0 + kRoiTgtChunk < a.C ? c0 + kRoiTgtChunk : a.C;
    const int nb = a.PH * a.PW;
    float *out = a.output + (t * a.C + c0) * nb;
    const int64_t n_out = (int64_t)(c1 - c0) * nb;

    const int64_t total = a.cum[N];
    bool live = t < total && total <= a.cap;      // (uniform: one load decides a dead slot)
    if (live || blockIdx.x == 0) {                // a live slot trusts the prefix only after looking at all of it; workgroup 0 reports
        if (tid == 0) s_bad = 0;
        for (int i = tid; i <= N; i += kRoiTgtThreads) s_cum[i] = a.cum[i];
        __syncthreads();
        bool bad = false;
        for (int i = tid; i <= N; i += kRoiTgtThreads) {
            const int64_t v = s_cum[i];
            bad |= i == 0 ? v != 0 : v < s_cum[i - 1];
            bad |= v > a.cap;
        }
        if (bad) s_bad = 1;      // (any thread: the same value)
        __syncthreads();
        const bool cum_bad = s_bad != 0;
        if (blockIdx.x == 0 && tid < 4) a.status[tid] = tid == 3 && cum_bad ? 1 : 0;
        live = live && !cum_bad;
    }
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    int b = 0;
    if (live) {
        int lo = 1, hi = N;      // the first index in [1, N] whose cum is > t (cum[N] is)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_cum[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        b = lo - 1;
        box = roi_tgt_pixel_box(reinterpret_cast<const float4 *>(a.tgt_boxes)[t], (float)a.sizes[2 * b], (float)a.sizes[2 * b + 1]);
        live = isfinite(box.x) && isfinite(box.y) && isfinite(box.z) && isfinite(box.w);
    }
    // the slot's geometry (msda_roi.h, aligned)
    const float start_w = box.x * a.spatial_scale - 0.5f, start_h = box.y * a.spatial_scale - 0.5f;
    const float end_w = box.z * a.spatial_scale - 0.5f, end_h = box.w * a.spatial_scale - 0.5f;
    const float roi_w = end_w - start_w, roi_h = end_h - start_h;
    const float bin_h = roi_h / (float)a.PH, bin_w = roi_w / (float)a.PW;
    int grid_h = a.sampling_ratio, grid_w = a.sampling_ratio;
    live = live && isfinite(start_w) && isfinite(start_h) && isfinite(roi_w) && isfinite(roi_h);      // (every sample position is finite then)
    if (live && a.sampling_ratio <= 0) {
        const float gh = ceilf(roi_h / (float)a.PH), gw = ceilf(roi_w / (float)a.PW);
        live = gh <= (float)kRoiTgtMaxGrid && gw <= (float)kRoiTgtMaxGrid;      // (false for NaN too)
        grid_h = live ? (int)gh : 0;
        grid_w = live ? (int)gw : 0;
    }
    if (!live) {
        roi_tgt_zero(out, n_out, tid, kRoiTgtThreads);
        return;
    }
    const float count = (float)(grid_h * grid_w > 1 ? grid_h * grid_w : 1);
    // thread -> (bin, channel lane)
    const int lanes_c = nb <= kRoiTgtThreads ? kRoiTgtThreads / nb : 1;
    const int bin0 = nb <= kRoiTgtThreads ? tid % nb : tid, bin_step = nb <= kRoiTgtThreads ? nb : kRoiTgtThreads;
    const int cl = nb <= kRoiTgtThreads ? tid / nb : 0;
    if (cl >= lanes_c) return;
    const int64_t plane_elems = (int64_t)a.H * a.W;
    for (int bin = bin0; bin < nb; bin += bin_step) {
        const int ph = bin / a.PW, pw = bin - ph * a.PW;
        const float y0 = start_h + (float)ph * bin_h, x0 = start_w + (float)pw * bin_w;
        for (int c = c0 + cl; c < c1; c += lanes_c) {
            const float *plane = a.input + ((int64_t)b * a.C + c) * plane_elems;
            float acc = 0.f;
            for (int iy = 0; iy < grid_h; ++iy) {
                const float y = y0 + ((float)iy + 0.5f) * bin_h / (float)grid_h;
                for (int ix = 0; ix < grid_w; ++ix) {
                    const float x = x0 + ((float)ix + 0.5f) * bin_w / (float)grid_w;
                    acc += roi_bilinear<float>(plane, a.H, a.W, y, x);
                }
            }
            out[(int64_t)(c - c0) * nb + bin] = acc / count;
        }
    }
}

}  // namespace msda
