// msda_geometry.h -- the batch-geometry tensors: everything the reference derives from the padding mask at the start of a forward, as ONE
// launch from the (N, 2) image sizes.  Included by rows_api.hip.
//
//   per-level masks        F.interpolate(mask, size=level) (models/richsem/richsem.py:593-612)            -> mask_flat (N, S) u8
//   get_valid_ratio        (deformable_transformer.py:253-260)                                             -> valid_ratios (N, L, 2): w, h
//   get_reference_points   (deformable_transformer.py:513-525)                                             -> ref (N, S, L, 2)
//   PositionEmbeddingSineHW (position_encoding.py:46-92, normalize=True, scale 2 pi)                       -> pos_sine (N, S, 2 F): y half | x half
//   gen_encoder_output_proposals' geometry half (utils.py:10-65)                                           -> proposals (N, S, 4), zeroed (N, S) u8
//
// Every padding mask the reference builds (nested_tensor_from_tensor_list) is a bottom / right rectangle: pixel (y, x) of image n is
// padding iff y >= h_n or x >= w_n.  Nearest-neighbour interpolation keeps that shape: with src(i) = min(int(floorf(i * (float(in) / out))),
// in - 1) level pixel (y, x) is padding iff src_y(y) >= h or src_x(x) >= w, src is monotone, so a level's valid part is its first vh rows and
// vw columns and the masks' cumulative sums are closed forms:
//     y_embed = (x < vw) ? min(y + 1, vh) : 0        x_embed = (y < vh) ? min(x + 1, vw) : 0
// divided by (last row / column + 1e-6), i.e. by vh + 1e-6 / vw + 1e-6, or by 0 + 1e-6 where the numerator is 0 as well.
//
// The arithmetic is the reference's, operation by operation, in float32 with IEEE division (this library is built without fast-math; no
// expression below has a multiply feeding an add, so nothing can contract).  dim_t comes from the host (correctly rounded powf, a table in
// the kernel's arguments).  sin / cos of a channel pair share their argument and come from one sincosf.
//
// Launch: one workgroup of 256 threads per tile of kGeoTile consecutive pixels of one (image, level).  Each workgroup finds the valid
// counts of all L levels of its image itself (2 L binary searches over the src rule, one per lane), so there is no header kernel, no
// atomic and nothing read back.  The per-pixel outputs are written by the first lanes; pos_sine -- the only output with real bytes --
// by all of them: every lane stores 16 B (4 channels) of one pixel, consecutive lanes on consecutive addresses.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace msda {

constexpr int kGeoThreads = 256;
constexpr int kGeoTile = 32;             // pixels per workgroup
constexpr int kGeoMaxLevels = 8;
constexpr int kGeoMaxPosFeats = 256;     // channels per half: the dim_t tables travel in the kernel's arguments

struct GeoParams {
    int N, L, canvas_h, canvas_w, F;      // F = num_pos_feats
    long long S;
    int h[kGeoMaxLevels], w[kGeoMaxLevels];
    long long start[kGeoMaxLevels];       // first pixel of the level in S
    int tiles[kGeoMaxLevels];             // tiles per image of the level
    int first_block[kGeoMaxLevels + 1];   // first workgroup of the level (N * tiles each); [L] = the grid
    float dim_h[kGeoMaxPosFeats], dim_w[kGeoMaxPosFeats];
};

// the input pixel F.interpolate(mode="nearest") reads for output pixel i
__device__ __forceinline__ int geo_src(int i, float scale, int in)
{
    return min((int)floorf((float)i * scale), in - 1);
}

// how many of the `out` pixels of a level read an input pixel below `valid` (src is monotone: they are the first ones)
__device__ __forceinline__ int geo_valid_count(int out, int in, int valid)
{
    const float scale = (float)in / (float)out;
    int lo = 0, hi = out;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (geo_src(mid, scale, in) < valid) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float geo_unsigmoid(float p)
{
    return logf(p / (1.f - p));
}

__global__ __launch_bounds__(kGeoThreads) void batch_geometry_kernel(const GeoParams p, const int32_t *__restrict__ sizes,
                                                                     uint8_t *__restrict__ mask_flat, float *__restrict__ valid_ratios,
                                                                     float *__restrict__ ref, float *__restrict__ pos_sine,
                                                                     float *__restrict__ proposals, uint8_t *__restrict__ zeroed)
{
    __shared__ int cnt_s[2 * kGeoMaxLevels];                  // [2 k] = vh, [2 k + 1] = vw of level k
    __shared__ float dim_s[2 * kGeoMaxPosFeats];              // y half's dim_t, then the x half's
    __shared__ float arg_s[2 * kGeoTile];                     // [2 i] = the y half's argument of the tile's pixel i, [2 i + 1] = the x half's
    const int tid = threadIdx.x;
    int l = 0;
    while (l + 1 < p.L && (int)blockIdx.x >= p.first_block[l + 1]) ++l;
    const int r = (int)blockIdx.x - p.first_block[l];
    const int n = r / p.tiles[l], tile = r - n * p.tiles[l];
    const int hl = p.h[l], wl = p.w[l], hw = hl * wl;
    const int pix0 = tile * kGeoTile, npix = min(kGeoTile, hw - pix0);

    if (tid < 2 * p.L) {
        const int k = tid >> 1, is_w = tid & 1;
        const int canvas = is_w ? p.canvas_w : p.canvas_h;
        const int size = min(max(sizes[2 * n + is_w], 1), canvas);      // device data: clamped here
        cnt_s[tid] = geo_valid_count(is_w ? p.w[k] : p.h[k], canvas, size);
    }
    if (pos_sine)
        for (int i = tid; i < 2 * p.F; i += kGeoThreads) dim_s[i] = i < p.F ? p.dim_h[i] : p.dim_w[i - p.F];
    __syncthreads();

    const int vh = cnt_s[2 * l], vw = cnt_s[2 * l + 1];
    const long long row0 = (long long)n * p.S + p.start[l] + pix0;      // first row of the tile in (N * S)
    if (tile == 0 && tid == 0)
        reinterpret_cast<float2 *>(valid_ratios)[n * p.L + l] = make_float2((float)vw / (float)wl, (float)vh / (float)hl);

    if (tid < npix) {
        const int pix = pix0 + tid, y = pix / wl, x = pix - y * wl;
        const bool padded = y >= vh || x >= vw;
        mask_flat[row0 + tid] = padded ? 1 : 0;
        if (pos_sine) {
            const float eps = 1e-6f, scale = 6.283185307179586f;
            const float ye = x < vw ? (float)min(y + 1, vh) : 0.f, yl = x < vw ? (float)vh : 0.f;
            const float xe = y < vh ? (float)min(x + 1, vw) : 0.f, xl = y < vh ? (float)vw : 0.f;
            arg_s[2 * tid] = ye / (yl + eps) * scale;
            arg_s[2 * tid + 1] = xe / (xl + eps) * scale;
        }
        if (proposals) {
            const float px = ((float)x + 0.5f) / (float)vw, py = ((float)y + 0.5f) / (float)vh, wh = 0.05f * (float)(1 << l);
            const bool valid = px > 0.01f && px < 0.99f && py > 0.01f && py < 0.99f && wh > 0.01f && wh < 0.99f;
            const bool zero = padded || !valid;
            const float inf = __builtin_inff(), u = geo_unsigmoid(wh);
            reinterpret_cast<float4 *>(proposals)[row0 + tid] =
                zero ? make_float4(inf, inf, inf, inf) : make_float4(geo_unsigmoid(px), geo_unsigmoid(py), u, u);
            zeroed[row0 + tid] = zero ? 1 : 0;
        }
    }
    if (ref) {      // one (pixel, level k) pair per lane: 8 B each, consecutive lanes on consecutive addresses
        const float rw = (float)vw / (float)wl, rh = (float)vh / (float)hl;
        for (int e = tid; e < npix * p.L; e += kGeoThreads) {
            const int i = e / p.L, k = e - i * p.L;
            const int pix = pix0 + i, y = pix / wl, x = pix - y * wl;
            const float kw = (float)cnt_s[2 * k + 1] / (float)p.w[k], kh = (float)cnt_s[2 * k] / (float)p.h[k];
            const float rx = ((float)x + 0.5f) / (rw * (float)wl), ry = ((float)y + 0.5f) / (rh * (float)hl);
            reinterpret_cast<float2 *>(ref)[(row0 + i) * p.L + k] = make_float2(rx * kw, ry * kh);
        }
    }
    if (!pos_sine) return;
    __syncthreads();
    const int quads = p.F >> 1;      // 16-byte stores per pixel: 2 F channels / 4
    float4 *__restrict__ out = reinterpret_cast<float4 *>(pos_sine) + row0 * quads;
    for (int e = tid; e < npix * quads; e += kGeoThreads) {
        const int i = e / quads, c = (e - i * quads) * 4;      // channels c .. c + 3: two (sin, cos) pairs, each inside one half (F is even)
        float v[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ch = c + 2 * j, half = ch >= p.F ? 1 : 0;
            sincosf(arg_s[2 * i + half] / dim_s[ch], &v[2 * j], &v[2 * j + 1]);      // (dim_s[ch]: the x half's table follows the y half's)
        }
        out[e] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

}  // namespace msda
