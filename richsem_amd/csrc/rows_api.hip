// rows_api.hip -- C ABI of the rows around the operator (declared in include/richsem_msda.h): the matcher's cost blocks and the assignment
// solver, the attention-pool core, the criterion's focal / box-pair / federated / distillation kernels, the decoder's box refinement and sine embedding,
// the narrow linear backward, PostProcess (top-k over query x class, box decode, NMS), and the module-level helpers that are not the
// operator itself: the denoising indices and mask, per-row top-k, ROIAlign and the padding-mask rows.  A translation unit of its own so
// that the operator's kernels (msda_api.hip) are not rebuilt with it.  Error reporting: msda_host.h.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "msda_host.h"
#include "msda_attnpool.h"
#include "msda_matcher.h"
#include "msda_lsap.h"
#include "msda_postproc.h"
#include "msda_dn.h"
#include "msda_topk.h"
#include "msda_roi.h"
#include "msda_prep.h"      // (mask_rows_kernel)

namespace {

template <typename T, bool TM = false>
int matcher_cost_impl(const char *entry, const T *logits, const T *boxes, const int64_t *tgt_ids, const T *tgt_boxes, const int64_t *tgt_offsets, int B,
                      int Q, int C, int64_t n_targets, double w_class, double w_bbox, double w_giou, double alpha, T *cost,
                      msda_stream_t stream)
{
    if (!logits || !boxes || !tgt_offsets || !cost) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (B < 1 || Q < 0 || C < 1 || n_targets < 0) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (n_targets > 0 && (!tgt_ids || !tgt_boxes)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int64_t total = (int64_t)Q * n_targets;
    if (total == 0) return MSDA_OK;
    if (total >= ((int64_t)1 << 40)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    const int grid = (int)std::min<int64_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL((msda::matcher_cost_kernel<T, TM>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), logits, boxes, tgt_ids,
                       tgt_boxes, tgt_offsets, B, Q, C, (T)w_class, (T)w_bbox, (T)w_giou, (T)alpha, cost);
    return msda::launched(entry);
}

// the LDS a launch of the solver needs, or a negative error: the host knows Q and the total number of targets only
int lsap_sizes(int n_out, int B, int Q, int64_t n_targets, int *cols_cap, int *rows_cap, size_t *lds)
{
    if (n_out < 1 || B < 1 || Q < 0 || n_targets < 0) return MSDA_ERR_BAD_DIMS;
    if (Q > msda::kLsapMaxDim || n_targets > msda::kLsapMaxDim || (int64_t)n_out * B >= ((int64_t)1 << 30)) return MSDA_ERR_TOO_LARGE;
    *cols_cap = std::max(Q, (int)n_targets);
    *rows_cap = std::min(Q, (int)n_targets);
    *lds = msda::lsap_lds_bytes(*cols_cap, *rows_cap);
    return MSDA_OK;
}

template <typename T>
int lsap_impl(const char *entry, const T *cost, int target_major, const int64_t *tgt_offsets, int n_out, int B, int Q, int64_t n_targets,
              int64_t *query_of_target, int32_t *status, msda_stream_t stream)
{
    if (!tgt_offsets || !status || (n_targets > 0 && (!query_of_target || (Q > 0 && !cost)))) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    int cols_cap = 0, rows_cap = 0;
    size_t lds = 0;
    const int rc = lsap_sizes(n_out, B, Q, n_targets, &cols_cap, &rows_cap, &lds);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    if (lds > 64 * 1024) {      // beyond the default limit of dynamic LDS
        const hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(msda::lsap_kernel<T>), msda::lsap_lds_bytes(msda::kLsapMaxDim, msda::kLsapMaxDim));
        if (e != hipSuccess) return msda::hip_fail(e, entry);
    }
    hipLaunchKernelGGL(msda::lsap_kernel<T>, dim3(n_out * B), dim3(64), lds, static_cast<hipStream_t>(stream), cost, target_major, tgt_offsets, B, Q,
                       n_targets, cols_cap, rows_cap, query_of_target, status);
    return msda::launched(entry);
}

template <typename T>
int attnpool_core_impl(const char *entry, const T *u, const T *feat, const T *pos, const T *spos, int K, int H, int C, int Tn, int head_major, T *z,
                       msda_stream_t stream)
{
    if (!u || !feat || !pos || !spos || !z) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (K < 0 || H < 1 || C < 1 || Tn < 1 || Tn > msda::kAttnPoolMaxT) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (K == 0) return MSDA_OK;
    if ((int64_t)K * H >= ((int64_t)1 << 31) || (int64_t)K * C * Tn >= ((int64_t)1 << 40)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    const int waves = msda::kAttnPoolThreads / msda::kWave;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (H % 4 == 0) {
        const size_t lds = (size_t)4 * (waves + 1) * (Tn + 1) * sizeof(T);
        hipLaunchKernelGGL((msda::attnpool_core_kernel<T, 4>), dim3(K * (H / 4)), dim3(msda::kAttnPoolThreads), lds, st, u, feat, pos, spos, K,
                           H, C, Tn, head_major, z);
    } else {
        const size_t lds = (size_t)(waves + 1) * (Tn + 1) * sizeof(T);
        hipLaunchKernelGGL((msda::attnpool_core_kernel<T, 1>), dim3(K * H), dim3(msda::kAttnPoolThreads), lds, st, u, feat, pos, spos, K, H, C,
                           Tn, head_major, z);
    }
    return msda::launched(entry);
}

// gen_sineembed_for_position (models/richsem/utils.py:142-168): one thread per (token, pair of channels) writes sin | cos of
// coordinate * 2 pi / T^(2 i / pe_dim) as a packed pair of bf16
__global__ __launch_bounds__(256) void sine_embed_kernel(const float *__restrict__ boxes, int ld, int tokens, int dims, int pe_dim,
                                                         float log2_temperature, unsigned *__restrict__ out)
{
    const int half = pe_dim / 2, per_tok = dims * half;
    const long long n = (long long)tokens * per_tok;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const int t = (int)(i / per_tok), r = (int)(i - (long long)t * per_tok);
        const int part = r / half, k = r - part * half;                 // output block `part` = (y, x, w, h); channels 2k, 2k + 1
        const int src = part < 2 ? 1 - part : part;                      // ... of the box's (x, y, w, h)
        const float v = boxes[(long long)t * ld + src] * 6.283185307179586f;
        const float p = v * exp2f(-log2_temperature * (float)(2 * k) / (float)pe_dim);
        const __hip_bfloat16 a = __float2bfloat16(sinf(p)), b = __float2bfloat16(cosf(p));
        out[i] = (unsigned)__bfloat16_as_ushort(a) | (unsigned)__bfloat16_as_ushort(b) << 16;
    }
}

// the decoder's box update (deformable_transformer.py:779-804 / richsem.py:705-715): y = sigmoid(delta + inverse_sigmoid(ref)) with
// inverse_sigmoid(r) = log(max(clamp(r, 0, 1), eps) / max(1 - clamp(r, 0, 1), eps)) (util/misc.py:605-609); and its gradient w.r.t. delta
template <bool BF16>
__global__ __launch_bounds__(256) void box_refine_kernel(const void *__restrict__ delta, const float *__restrict__ ref, float eps, long long n,
                                                         float *__restrict__ out)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const float d = BF16 ? __bfloat162float(static_cast<const __hip_bfloat16 *>(delta)[i]) : static_cast<const float *>(delta)[i];
        const float r = fminf(fmaxf(ref[i], 0.f), 1.f);
        const float u = d + logf(fmaxf(r, eps) / fmaxf(1.f - r, eps));
        out[i] = 1.f / (1.f + expf(-u));
    }
}

// ... and, when `ref` carries a gradient too (the heads' boxes of decoder layers 1..5, richsem.py:705-715: the "look forward twice"
// reference is not detached there), w.r.t. ref: d inverse_sigmoid / d r = [r_c >= eps] / max(r_c, eps) + [1 - r_c >= eps] / max(1 - r_c, eps)
// inside [0, 1] (torch's clamp passes the gradient where the bound is not active, bounds included), 0 outside
template <bool BF16>
__global__ __launch_bounds__(256) void box_refine_grad_kernel(const float *__restrict__ gy, const float *__restrict__ y, long long n,
                                                              void *__restrict__ gdelta, const float *__restrict__ ref, float eps,
                                                              float *__restrict__ gref)
{
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        const float v = gy[i] * y[i] * (1.f - y[i]);
        if (BF16) static_cast<__hip_bfloat16 *>(gdelta)[i] = __float2bfloat16(v);
        else static_cast<float *>(gdelta)[i] = v;
        if (gref) {
            const float r0 = ref[i], r = fminf(fmaxf(r0, 0.f), 1.f);
            const float dr = (r >= eps ? 1.f / fmaxf(r, eps) : 0.f) + (1.f - r >= eps ? 1.f / fmaxf(1.f - r, eps) : 0.f);
            gref[i] = (r0 >= 0.f && r0 <= 1.f) ? v * dr : 0.f;
        }
    }
}

// Backward of a 256 -> n linear layer with n <= 8 (the box heads' last layer, 256 -> 4): the input gradient is an n-term sum per channel,
// the weight gradient n x 256 token sums -- streams of x / dx, not GEMMs (the library's GEMM takes 150 us for the 44646-token one, padded to 64).
__global__ __launch_bounds__(256) void narrow_linear_dx_kernel(const uint16_t *__restrict__ dy, const float *__restrict__ w, int T, int n,
                                                               uint16_t *__restrict__ dx)
{
    __shared__ float ws[8 * 256];
    for (int i = threadIdx.x; i < n * 256; i += 256) ws[i] = w[i];
    __syncthreads();
    const long long total = (long long)T * 32;      // a thread: one token, 8 channels
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += gridDim.x * 256ll) {
        const long long t = i >> 5;
        const int c0 = 8 * (int)(i & 31);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < n; ++j) {
            const float d = __uint_as_float((unsigned)dy[t * n + j] << 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(d, ws[j * 256 + c0 + e], acc[e]);
        }
        unsigned o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            o[e] = (unsigned)__bfloat16_as_ushort(__float2bfloat16(acc[2 * e])) | (unsigned)__bfloat16_as_ushort(__float2bfloat16(acc[2 * e + 1])) << 16;
        *reinterpret_cast<uint4 *>(dx + t * 256 + c0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// dw[j][c] += sum over the workgroup's tokens of dy[t][j] x[t][c] (thread = channel c), db[j] likewise (threads j < n).
// Eight tokens per trip with all of their loads issued before the first product (token index clamped, the surplus tokens weighted 0): as a
// plain loop over the tokens every trip waited for its own two loads -- 42.6 us for 2184 tokens (round 4: the composed step's twelve calls).
__global__ __launch_bounds__(256) void narrow_linear_dw_kernel(const uint16_t *__restrict__ dy, const uint16_t *__restrict__ x, int T, int n,
                                                               int chunk, float *__restrict__ dw, float *__restrict__ db)
{
    const int c = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * chunk, t1 = t0 + chunk < T ? t0 + chunk : T;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    const int cb = c < n ? c : 0;
    for (long long t = t0; t < t1; t += 8) {
        float xv[8], bv[8];
        unsigned short dv[8][8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long tt = t + u < t1 ? t + u : t1 - 1;
            xv[u] = __uint_as_float((unsigned)x[tt * 256 + c] << 16);
            bv[u] = __uint_as_float((unsigned)dy[tt * n + cb] << 16);
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[u][j] = dy[tt * n + (j < n ? j : 0)];      // (wave-uniform addresses: scalar loads)
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float live = t + u < t1 ? 1.f : 0.f;
            const float xs = xv[u] * live;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j < n) acc[j] = fmaf(__uint_as_float((unsigned)dv[u][j] << 16), xs, acc[j]);
            bsum += bv[u] * live;
        }
    }
    for (int j = 0; j < n; ++j) atomicAdd(dw + j * 256 + c, acc[j]);
    if (db && c < n) atomicAdd(db + c, bsum);
}

}  // namespace


// ---- the all-negative term of the sigmoid focal loss over a whole logit tensor (criterion plumbing) ------------
// sigmoid_focal_loss (reference models/richsem/utils.py / richsem.py:1124-1160) at a NEGATIVE entry is (1 - alpha) p^2 softplus(x), p = sigmoid(x);
// the criterion sums it over every (output, image, query, class) with a weight per ROW (1 / num_boxes for the matching queries, 1 / (num_boxes
// x groups) for the denoising queries' positive slots, 0 for the slots that carry no loss) and corrects the few positive entries separately.
// As PyTorch ops that is sigmoid, softplus, three products, a slice and a sum forward and as many kernels backward over 63 MB of logits; here one
// pass each way.   forward: partial[block] = sum_rows w[row] sum_c (1 - alpha) p^2 softplus(x)   (fp64 partials, summed by the caller)
//                  backward: grad_x = g w[row] (1 - alpha) p^2 (2 (1 - p) softplus(x) + p)
__device__ __forceinline__ float focal_neg(float x, float &dfdx)
{
    const float p = 1.f / (1.f + __expf(-x));
    const float sp = x > 20.f ? x : log1pf(__expf(x));      // softplus, as torch (threshold 20)
    const float pp = p * p;
    dfdx = pp * (2.f * (1.f - p) * sp + p);
    return pp * sp;
}

__global__ __launch_bounds__(256) void focal_neg_sum_kernel(const float *__restrict__ x, const float *__restrict__ w, long long rows, int C, float one_m_alpha,
                                                            double *__restrict__ partial)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float wr = w[r];
        if (wr == 0.f) continue;      // (block-uniform)
        float s = 0.f;
        for (int c = threadIdx.x; c < C; c += 256) {
            float d;
            s += focal_neg(x[r * C + c], d);
        }
        acc += (double)(s * wr);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] * (double)one_m_alpha;
}

__global__ __launch_bounds__(256) void focal_neg_grad_kernel(const float *__restrict__ x, const float *__restrict__ w, long long rows, int C, float one_m_alpha,
                                                             const float *__restrict__ gscale, float *__restrict__ gx)
{
    const float g = gscale[0] * one_m_alpha;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float wr = w[r] * g;
        for (int c = threadIdx.x; c < C; c += 256) {
            float d = 0.f;
            if (wr != 0.f) focal_neg(x[r * C + c], d);
            gx[r * C + c] = d * wr;
        }
    }
}

#include "msda_fed.h"      // (the federated loss: class sampler + the masked form of the two kernels above, which it shares focal_neg with)
#include "msda_distill.h"  // (the distillation term: KL of class distributions / L1 of unit vectors over gathered rows)
#include "msda_geometry.h" // (the batch-geometry tensors from the image sizes: masks, valid ratios, reference points, sine position, anchors)
#include "msda_dn_noise.h" // (the denoising queries from the target counts on the device: label / box noise, embedding, mask; the table's gradient)

namespace {

static_assert(MSDA_DISTILL_WORKSPACE_BYTES == sizeof(double) * msda::kDistillMaxGrid, "one f64 partial per workgroup");

// the checks the three distillation entry points share; MSDA_OK, or the code arg_fail has reported
int distill_check(const char *entry, const void *pred, int64_t pred_rows, const void *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                  const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                  int dynamic_weight, const double *workspace, const float *loss, const float *grad_rows, size_t pred_elem)
{
    if (!loss || (K > 0 && (!workspace || !pred_row || !tgt_row || !row_weight || !grad_rows || (pred_rows > 0 && !pred) || (tgt_rows > 0 && !tgt))))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    if (K < 0 || C < 1 || pred_rows < 0 || tgt_rows < 0 || groups < 0 || (dynamic_weight != 0 && dynamic_weight != 1) || (dynamic_weight && C < 2))
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, entry);
    if ((class_mask != nullptr) != (groups > 0)) return msda::arg_fail(groups > 0 ? MSDA_ERR_NULL_POINTER : MSDA_ERR_BAD_DIMS, entry);      // a mask without groups, groups without a mask
    if (class_mask && !row_group) return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    if (!class_mask && row_group) return msda::arg_fail(MSDA_ERR_BAD_DIMS, entry);
    if (!msda::aligned(pred_elem, {pred}) || !msda::aligned(4, {tgt, row_weight, row_group, class_mask, loss, grad_rows}) ||
        !msda::aligned(8, {pred_row, tgt_row, workspace}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, entry);
    return MSDA_OK;
}

// K == 0: loss = 0 and nothing else; otherwise the row kernel `launch(grid)` and, with more than one workgroup, the total of the partials
// the workgroups left in the caller's workspace
template <typename Launch>
int distill_run(const char *entry, int64_t K, double *partial, float *loss, hipStream_t stream, Launch launch)
{
    if (K == 0) {
        const hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), stream);
        return e == hipSuccess ? MSDA_OK : msda::hip_fail(e, entry, ": clearing the loss");
    }
    const int grid = (int)std::min<int64_t>(K, msda::kDistillMaxGrid);
    launch(grid);
    if (grid > 1)
        hipLaunchKernelGGL(msda::distill_total_kernel, dim3(1), dim3(msda::kDistillThreads), 0, stream, (const double *)partial, grid, loss);
    return msda::launched(entry);
}

template <typename TP>
int distill_kl_impl(const char *entry, const TP *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                    const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                    int dynamic_weight, double *workspace, float *loss, float *grad_rows, msda_stream_t stream)
{
    const int rc = distill_check(entry, pred, pred_rows, tgt, tgt_rows, C, pred_row, tgt_row, row_weight, K, row_group, class_mask, groups,
                                 dynamic_weight, workspace, loss, grad_rows, sizeof(TP));
    if (rc != MSDA_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return distill_run(entry, K, workspace, loss, s, [&](int grid) {
        hipLaunchKernelGGL(msda::distill_kl_kernel<TP>, dim3(grid), dim3(msda::kDistillThreads), 0, s, pred, (long long)pred_rows, tgt,
                           (long long)tgt_rows, C, pred_row, tgt_row, row_weight, (long long)K, row_group, class_mask, groups, dynamic_weight,
                           workspace, loss, grad_rows);
    });
}

}  // namespace

// ---- the criterion's per-pair tails as one kernel each (verdict item 3: "one kernel for the stacked focal + L1 + GIoU tails") -------------
// Box loss of K matched pairs (reference SetCriterion.loss_boxes, models/richsem/richsem.py:1162-1188 with util/box_ops.py:9-64 on the
// diagonal):   sum_k w[k] * ( c_l1 * |p_k - t_k|_1 + c_giou * (1 - GIoU(xyxy(p_k), xyxy(t_k))) ),   p, t = (cx, cy, w, h)
// and its gradient w.r.t. p, by forward-mode differentiation with four tangents per value (torch's conventions: |x|' = sign x, a maximum /
// minimum passes the gradient to the larger / smaller operand and halves it on a tie, clamp(min = 0) passes it where x >= 0).
struct Dual4 {
    float v, d[4];
};
__device__ __forceinline__ Dual4 d4_const(float v) { return Dual4{v, {0.f, 0.f, 0.f, 0.f}}; }
__device__ __forceinline__ Dual4 d4_var(float v, int i) { Dual4 r = d4_const(v); r.d[i] = 1.f; return r; }
__device__ __forceinline__ Dual4 operator+(Dual4 a, Dual4 b) { return Dual4{a.v + b.v, {a.d[0] + b.d[0], a.d[1] + b.d[1], a.d[2] + b.d[2], a.d[3] + b.d[3]}}; }
__device__ __forceinline__ Dual4 operator-(Dual4 a, Dual4 b) { return Dual4{a.v - b.v, {a.d[0] - b.d[0], a.d[1] - b.d[1], a.d[2] - b.d[2], a.d[3] - b.d[3]}}; }
__device__ __forceinline__ Dual4 operator*(Dual4 a, Dual4 b)
{
    return Dual4{a.v * b.v, {a.d[0] * b.v + a.v * b.d[0], a.d[1] * b.v + a.v * b.d[1], a.d[2] * b.v + a.v * b.d[2], a.d[3] * b.v + a.v * b.d[3]}};
}
__device__ __forceinline__ Dual4 operator/(Dual4 a, Dual4 b)
{
    const float q = a.v / b.v, ib = 1.f / b.v;
    return Dual4{q, {(a.d[0] - q * b.d[0]) * ib, (a.d[1] - q * b.d[1]) * ib, (a.d[2] - q * b.d[2]) * ib, (a.d[3] - q * b.d[3]) * ib}};
}
__device__ __forceinline__ Dual4 d4_scale(Dual4 a, float s) { return Dual4{a.v * s, {a.d[0] * s, a.d[1] * s, a.d[2] * s, a.d[3] * s}}; }
__device__ __forceinline__ Dual4 d4_max(Dual4 a, Dual4 b) { return a.v > b.v ? a : (b.v > a.v ? b : d4_scale(a + b, 0.5f)); }
__device__ __forceinline__ Dual4 d4_min(Dual4 a, Dual4 b) { return a.v < b.v ? a : (b.v < a.v ? b : d4_scale(a + b, 0.5f)); }
__device__ __forceinline__ Dual4 d4_relu(Dual4 a) { return a.v >= 0.f ? a : d4_const(0.f); }
__device__ __forceinline__ Dual4 d4_abs(Dual4 a) { return a.v > 0.f ? a : (a.v < 0.f ? d4_scale(a, -1.f) : d4_const(0.f)); }

__device__ __forceinline__ float block_sum_1024(float v, float *red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x < 64) {
        s = threadIdx.x < blockDim.x / 64 ? red[threadIdx.x] : 0.f;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    }
    return s;      // (valid in thread 0)
}

// one workgroup (K is thousands: the matched, two-stage and denoising pairs of a step): loss[0] and grad_p (K, 4) = d loss / d p
__global__ __launch_bounds__(1024) void box_pair_loss_kernel(const float *__restrict__ p, const float *__restrict__ t, const float *__restrict__ w, int K,
                                                             float c_l1, float c_giou, float *__restrict__ loss, float *__restrict__ grad_p)
{
    __shared__ float red[16];
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float4 pv = reinterpret_cast<const float4 *>(p)[k], tv = reinterpret_cast<const float4 *>(t)[k];
        const Dual4 cx = d4_var(pv.x, 0), cy = d4_var(pv.y, 1), pw = d4_var(pv.z, 2), ph = d4_var(pv.w, 3);
        const Dual4 l1 = d4_abs(cx - d4_const(tv.x)) + d4_abs(cy - d4_const(tv.y)) + d4_abs(pw - d4_const(tv.z)) + d4_abs(ph - d4_const(tv.w));
        const Dual4 half = d4_const(0.5f);
        const Dual4 ax0 = cx - half * pw, ay0 = cy - half * ph, ax1 = cx + half * pw, ay1 = cy + half * ph;
        const Dual4 bx0 = d4_const(tv.x - 0.5f * tv.z), by0 = d4_const(tv.y - 0.5f * tv.w), bx1 = d4_const(tv.x + 0.5f * tv.z), by1 = d4_const(tv.y + 0.5f * tv.w);
        const Dual4 area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
        const Dual4 iw = d4_relu(d4_min(ax1, bx1) - d4_max(ax0, bx0)), ih = d4_relu(d4_min(ay1, by1) - d4_max(ay0, by0));
        const Dual4 inter = iw * ih, uni = area_a + area_b - inter;
        const Dual4 iou = inter / (uni + d4_const(1e-6f));
        const Dual4 hw = d4_relu(d4_max(ax1, bx1) - d4_min(ax0, bx0)), hh = d4_relu(d4_max(ay1, by1) - d4_min(ay0, by0));
        const Dual4 hull = hw * hh;
        const Dual4 giou = iou - (hull - uni) / (hull + d4_const(1e-6f));
        const Dual4 l = d4_scale(l1, c_l1) + d4_scale(d4_const(1.f) - giou, c_giou);
        const float wk = w[k];
        acc += l.v * wk;
        reinterpret_cast<float4 *>(grad_p)[k] = make_float4(l.d[0] * wk, l.d[1] * wk, l.d[2] * wk, l.d[3] * wk);
    }
    const float s = block_sum_1024(acc, red);
    if (threadIdx.x == 0) loss[0] = s;
}

// What the positive entries of a sigmoid focal loss contribute INSTEAD of the all-negative term FocalNegativeSum has counted for them
// (sigmoid_focal_loss, models/richsem/richsem.py:1124-1160 with util: alpha (1 - q)^2 softplus(-x) for a positive, (1 - alpha) q^2
// softplus(x) for a negative, q = sigmoid(x)):   sum_k w[k] * ( alpha (1 - q_k)^2 softplus(-x_k) - (1 - alpha) q_k^2 softplus(x_k) )
__global__ __launch_bounds__(1024) void focal_pos_sum_kernel(const float *__restrict__ x, const float *__restrict__ w, int K, float alpha,
                                                             float *__restrict__ loss, float *__restrict__ grad_x)
{
    __shared__ float red[16];
    float acc = 0.f;
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const float v = x[k], q = 1.f / (1.f + expf(-v));
        const float sp_pos = v > 20.f ? v : log1pf(expf(v)), sp_neg = -v > 20.f ? -v : log1pf(expf(-v));      // softplus(x), softplus(-x) (torch's threshold 20)
        const float omq = 1.f - q;
        const float l = alpha * omq * omq * sp_neg - (1.f - alpha) * q * q * sp_pos;
        // d/dx: q' = q (1 - q); softplus(x)' = q; softplus(-x)' = -(1 - q)
        const float dl = alpha * (-2.f * omq * q * omq * sp_neg - omq * omq * omq) - (1.f - alpha) * (2.f * q * q * omq * sp_pos + q * q * q);
        const float wk = w[k];
        acc += l * wk;
        grad_x[k] = dl * wk;
    }
    const float s = block_sum_1024(acc, red);
    if (threadIdx.x == 0) loss[0] = s;
}

namespace {

// the checks, the grid rule and the launch of msda_focal_neg_sum_f32 (masked = false: no row groups, no class masks) and of its masked form
int focal_neg_sum_launch(const char *entry, bool masked, const float *logits, const float *row_weight, const int32_t *row_group,
                         const float *class_mask, int groups, int64_t rows, int C, float alpha, double *partial, int max_partial, int *n_partial,
                         msda_stream_t stream)
{
    if (!logits || !row_weight || !partial || !n_partial || (masked && (!row_group || !class_mask)))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    if (rows < 1 || C < 1 || max_partial < 1 || (masked && groups < 1)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, entry);
    const int grid = (int)std::min<int64_t>(std::min<int64_t>(rows, 4096), max_partial);
    *n_partial = grid;
    if (masked)
        hipLaunchKernelGGL(msda::focal_neg_sum_masked_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), logits, row_weight,
                           row_group, class_mask, groups, (long long)rows, C, 1.f - alpha, partial);
    else
        hipLaunchKernelGGL(focal_neg_sum_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), logits, row_weight, (long long)rows, C,
                           1.f - alpha, partial);
    return msda::launched(entry);
}

// the same for msda_focal_neg_grad_f32 and its masked form
int focal_neg_grad_launch(const char *entry, bool masked, const float *logits, const float *row_weight, const int32_t *row_group,
                          const float *class_mask, int groups, int64_t rows, int C, float alpha, const float *gscale, float *grad_logits,
                          msda_stream_t stream)
{
    if (!logits || !row_weight || !gscale || !grad_logits || (masked && (!row_group || !class_mask)))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    if (rows < 1 || C < 1 || (masked && groups < 1)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, entry);
    const int grid = (int)std::min<int64_t>(rows, 8192);
    if (masked)
        hipLaunchKernelGGL(msda::focal_neg_grad_masked_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), logits, row_weight,
                           row_group, class_mask, groups, (long long)rows, C, 1.f - alpha, gscale, grad_logits);
    else
        hipLaunchKernelGGL(focal_neg_grad_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), logits, row_weight, (long long)rows, C,
                           1.f - alpha, gscale, grad_logits);
    return msda::launched(entry);
}

}  // namespace

extern "C" {

/* msda_focal_neg_sum_f32: partial (grid doubles, grid = the value returned through n_partial) <- weighted all-negative focal sums; the caller adds
 * them up.  msda_focal_neg_grad_f32: grad_logits <- gscale[0] * d/dx of that sum (every element written). */
int msda_focal_neg_sum_f32(const float *logits, const float *row_weight, int64_t rows, int C, float alpha, double *partial, int max_partial,
                           int *n_partial, msda_stream_t stream)
{
    return focal_neg_sum_launch(__func__, false, logits, row_weight, nullptr, nullptr, 0, rows, C, alpha, partial, max_partial, n_partial, stream);
}
int msda_focal_neg_grad_f32(const float *logits, const float *row_weight, int64_t rows, int C, float alpha, const float *gscale,
                            float *grad_logits, msda_stream_t stream)
{
    return focal_neg_grad_launch(__func__, false, logits, row_weight, nullptr, nullptr, 0, rows, C, alpha, gscale, grad_logits, stream);
}

/* msda_fed_class_mask_f32: per group g, mask[g][c] = 1 for the classes among labels and for m = max(num_sample_cats - appeared, 0) more
 * drawn without replacement with probability proportional to class_weight (the exponential race, msda_fed.h), 0 elsewhere;
 * n_chosen[g] = appeared + min(m, eligible).  msda_focal_neg_{sum,grad}_masked_f32: msda_focal_neg_{sum,grad}_f32 with the classes of row r
 * restricted to class_mask[row_group[r]]. */
int msda_fed_class_mask_f32(const int64_t *labels, int64_t n_labels, const float *class_weight, const float *uniform, int groups, int C,
                            int num_sample_cats, float *mask, int32_t *n_chosen, msda_stream_t stream)
{
    if (!class_weight || !uniform || !mask || !n_chosen || (n_labels > 0 && !labels)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_labels < 0 || groups < 1 || C < 1 || C > msda::kFedMaxClasses || num_sample_cats < 0) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    int P2 = 1;
    while (P2 < C) P2 <<= 1;
    const int threads = std::min(msda::kFedThreads, std::max(64, P2 / 2));
    hipLaunchKernelGGL(msda::fed_class_mask_kernel, dim3(groups), dim3(threads), sizeof(unsigned long long) * P2, static_cast<hipStream_t>(stream),
                       labels, (long long)n_labels, class_weight, uniform, C, P2, num_sample_cats, mask, n_chosen);
    return msda::launched(__func__);
}
int msda_focal_neg_sum_masked_f32(const float *logits, const float *row_weight, const int32_t *row_group, const float *class_mask, int groups,
                                  int64_t rows, int C, float alpha, double *partial, int max_partial, int *n_partial, msda_stream_t stream)
{
    return focal_neg_sum_launch(__func__, true, logits, row_weight, row_group, class_mask, groups, rows, C, alpha, partial, max_partial, n_partial,
                                stream);
}
int msda_focal_neg_grad_masked_f32(const float *logits, const float *row_weight, const int32_t *row_group, const float *class_mask, int groups,
                                   int64_t rows, int C, float alpha, const float *gscale, float *grad_logits, msda_stream_t stream)
{
    return focal_neg_grad_launch(__func__, true, logits, row_weight, row_group, class_mask, groups, rows, C, alpha, gscale, grad_logits, stream);
}

/* The distillation term over K gathered rows (msda_distill.h; semantics in include/richsem_msda.h): loss[0] <- the sum of the row losses,
 * grad_rows (K, C) <- the gradient w.r.t. the gathered student rows, one launch for both (+ one small launch for the total of the f64
 * partials in the caller's workspace: the library owns no memory here). */
int msda_distill_kl_f32(const float *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                        const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                        int dynamic_weight, double *workspace, float *loss, float *grad_rows, msda_stream_t stream)
{
    return distill_kl_impl(__func__, pred, pred_rows, tgt, tgt_rows, C, pred_row, tgt_row, row_weight, K, row_group, class_mask, groups,
                           dynamic_weight, workspace, loss, grad_rows, stream);
}
int msda_distill_kl_bf16(const uint16_t *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                         const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                         int dynamic_weight, double *workspace, float *loss, float *grad_rows, msda_stream_t stream)
{
    return distill_kl_impl(__func__, reinterpret_cast<const msda::bf16_t *>(pred), pred_rows, tgt, tgt_rows, C, pred_row, tgt_row, row_weight, K,
                           row_group, class_mask, groups, dynamic_weight, workspace, loss, grad_rows, stream);
}
int msda_distill_l1_f32(const float *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int D, const int64_t *pred_row,
                        const int64_t *tgt_row, const float *row_weight, int64_t K, int normalize_target, double *workspace, float *loss,
                        float *grad_rows, msda_stream_t stream)
{
    if (normalize_target != 0 && normalize_target != 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    const int rc = distill_check(__func__, pred, pred_rows, tgt, tgt_rows, D, pred_row, tgt_row, row_weight, K, nullptr, nullptr, 0, 0, workspace,
                                 loss, grad_rows, sizeof(float));
    if (rc != MSDA_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return distill_run(__func__, K, workspace, loss, s, [&](int grid) {
        hipLaunchKernelGGL(msda::distill_l1_kernel, dim3(grid), dim3(msda::kDistillThreads), 0, s, pred, (long long)pred_rows, tgt,
                           (long long)tgt_rows, D, pred_row, tgt_row, row_weight, (long long)K, normalize_target, workspace, loss, grad_rows);
    });
}

/* The batch-geometry tensors from the image sizes, one launch (msda_geometry.h; semantics in include/richsem_msda.h).  `shapes` is read on
 * the host, `sizes` on the device only: nothing is read back and nothing allocated. */
int msda_batch_geometry_f32(const int32_t *sizes, int N, int canvas_h, int canvas_w, const int32_t *shapes, int L, int num_pos_feats,
                            float temperature_h, float temperature_w, uint8_t *mask_flat, float *valid_ratios, float *ref, float *pos_sine,
                            float *proposals, uint8_t *zeroed, msda_stream_t stream)
{
    if (!sizes || !shapes || !mask_flat || !valid_ratios || ((proposals != nullptr) != (zeroed != nullptr)))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (N < 1 || canvas_h < 1 || canvas_w < 1 || L < 1 || L > msda::kGeoMaxLevels || num_pos_feats < 2 || (num_pos_feats & 1) ||
        (2 * (int64_t)num_pos_feats) % 4 != 0 || num_pos_feats > msda::kGeoMaxPosFeats || !(temperature_h > 0.f) || !(temperature_w > 0.f))
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    msda::GeoParams p = {};
    p.N = N, p.L = L, p.canvas_h = canvas_h, p.canvas_w = canvas_w, p.F = num_pos_feats;
    int64_t S = 0, blocks = 0;
    for (int l = 0; l < L; ++l) {
        const int h = shapes[2 * l], w = shapes[2 * l + 1];
        if (h < 1 || w < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
        if ((int64_t)h * w >= ((int64_t)1 << 31)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
        const int64_t tiles = ((int64_t)h * w + msda::kGeoTile - 1) / msda::kGeoTile;
        p.h[l] = h, p.w[l] = w, p.start[l] = S, p.tiles[l] = (int)tiles, p.first_block[l] = (int)blocks;
        S += (int64_t)h * w;
        blocks += tiles * N;
        if (blocks >= ((int64_t)1 << 31) || S * N >= ((int64_t)1 << 31)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    }
    p.S = S;
    p.first_block[L] = (int)blocks;
    if (!msda::aligned(4, {sizes}) || !msda::aligned(8, {valid_ratios, ref}) || !msda::aligned(16, {pos_sine, proposals}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    // dim_t[i] = temperature ** (2 * (i // 2) / num_pos_feats): the exponent formed in float32 as the reference forms it, the power
    // correctly rounded
    for (int i = 0; i < num_pos_feats; ++i) {
        const float e = (2.f * (float)(i / 2)) / (float)num_pos_feats;
        p.dim_h[i] = (float)std::pow((double)temperature_h, (double)e);
        p.dim_w[i] = (float)std::pow((double)temperature_w, (double)e);
    }
    hipLaunchKernelGGL(msda::batch_geometry_kernel, dim3((unsigned)blocks), dim3(msda::kGeoThreads), 0, static_cast<hipStream_t>(stream), p, sizes,
                       mask_flat, valid_ratios, ref, pos_sine, proposals, zeroed);
    return msda::launched(__func__);
}

/* The denoising queries from the per-image target counts on the device, one launch (msda_dn_noise.h; semantics in include/richsem_msda.h):
 * nothing is read back and nothing allocated, every element of every output is written.  A buffer that has no elements may be null. */
int msda_dn_queries_f32(const int64_t *cum, const int64_t *labels, const float *boxes, int64_t target_cap, const float *uniform,
                        const float *table, int N, int pad_cap, int D, int V, int num_classes, int num_queries, int dn_number,
                        float label_noise_ratio, float box_noise_scale, int use_cdn, int add_gt, float *q_label, float *q_bbox,
                        int64_t *noised_label, float *noised_box, uint8_t *attn_mask, int64_t *meta, msda_stream_t stream)
{
    if (N < 1 || pad_cap < 0 || D < 4 || D % 4 != 0 || V < 1 || num_classes < 1 || num_queries < 0 || dn_number < 0 || target_cap < 0 ||
        (use_cdn != 0 && use_cdn != 1) || (add_gt != 0 && add_gt != 1) || !(label_noise_ratio >= 0.f) || !(box_noise_scale >= 0.f))
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    const int64_t rows = (int64_t)N * pad_cap, T = (int64_t)pad_cap + num_queries;
    if (!cum || !table || !meta || (target_cap > 0 && (!labels || !boxes)) || (rows > 0 && (!uniform || !q_label || !q_bbox || !noised_label)) ||
        (T > 0 && !attn_mask))
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int64_t row_blocks = (rows + msda::kDnRows - 1) / msda::kDnRows;
    const int64_t mask_blocks = (T * T + msda::kDnMaskBytes - 1) / msda::kDnMaskBytes;
    if (T >= ((int64_t)1 << 31) || rows >= ((int64_t)1 << 31) || rows * D >= ((int64_t)1 << 40) || (int64_t)V * D >= ((int64_t)1 << 40) ||
        row_blocks + mask_blocks >= ((int64_t)1 << 31))
        return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (!msda::aligned(16, {boxes, table, q_label, q_bbox, noised_box, attn_mask}) || !msda::aligned(8, {cum, labels, noised_label, meta}) ||
        !msda::aligned(4, {uniform}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    msda::DnParams p = {};
    p.N = N, p.pad_cap = pad_cap, p.D = D, p.V = V, p.num_classes = num_classes, p.num_queries = num_queries, p.dn_number = dn_number;
    p.use_cdn = use_cdn, p.add_gt = add_gt, p.target_cap = target_cap;
    p.label_thr = label_noise_ratio * 0.5f, p.box_noise_scale = box_noise_scale, p.row_blocks = (int)row_blocks;
    const int64_t grid = std::max<int64_t>(row_blocks + mask_blocks, 1);      // (the first workgroup also writes meta)
    hipLaunchKernelGGL(msda::dn_queries_kernel, dim3((unsigned)grid), dim3(msda::kDnThreads), 0, static_cast<hipStream_t>(stream), p, cum, labels,
                       boxes, uniform, table, q_label, q_bbox, noised_label, noised_box, attn_mask, meta);
    return msda::launched(__func__);
}

/* The embedding table's gradient of the call above: grad_table (V, D) <- per class the sum, in row order, of the rows of grad_q_label
 * (rows, D) whose noised_label is that class; every row of grad_table is written, zeros where no slot hits.  No atomic. */
int msda_dn_queries_backward_f32(const float *grad_q_label, const int64_t *noised_label, int64_t rows, int D, int V, float *grad_table,
                                 msda_stream_t stream)
{
    if (rows < 0 || D < 4 || D % 4 != 0 || V < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!grad_table || (rows > 0 && (!grad_q_label || !noised_label))) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (rows * D >= ((int64_t)1 << 40) || (int64_t)V * D >= ((int64_t)1 << 40)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (!msda::aligned(16, {grad_q_label, grad_table}) || !msda::aligned(8, {noised_label})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const int per = msda::kDnThreads / 64;
    hipLaunchKernelGGL(msda::dn_queries_backward_kernel, dim3((unsigned)((V + per - 1) / per)), dim3(msda::kDnThreads), 0,
                       static_cast<hipStream_t>(stream), grad_q_label, noised_label, (long long)rows, D, V, grad_table);
    return msda::launched(__func__);
}

/* The criterion's per-pair tails, one launch each (K pairs, float32, one workgroup): loss[0] <- the weighted sum, grad (K, 4) / (K) <- its
 * gradient w.r.t. the predictions (the caller multiplies by the incoming scalar gradient).
 * msda_box_pair_loss_f32: sum_k w[k] (c_l1 |p_k - t_k|_1 + c_giou (1 - GIoU(p_k, t_k))), boxes (cx, cy, w, h) (SetCriterion.loss_boxes);
 * msda_focal_pos_sum_f32: sum_k w[k] (alpha (1 - q)^2 softplus(-x_k) - (1 - alpha) q^2 softplus(x_k)), q = sigmoid(x_k): what a positive entry
 * contributes to the sigmoid focal loss instead of the all-negative term msda_focal_neg_sum_f32 counted for it. */
int msda_box_pair_loss_f32(const float *pred, const float *target, const float *weight, int K, float c_l1, float c_giou, float *loss, float *grad_pred,
                           msda_stream_t stream)
{
    if (!pred || !target || !weight || !loss || !grad_pred) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (K < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {pred, target, grad_pred})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipLaunchKernelGGL(box_pair_loss_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), pred, target, weight, K, c_l1, c_giou, loss, grad_pred);
    return msda::launched(__func__);
}
int msda_focal_pos_sum_f32(const float *x, const float *weight, int K, float alpha, float *loss, float *grad_x, msda_stream_t stream)
{
    if (!x || !weight || !loss || !grad_x) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (K < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    hipLaunchKernelGGL(focal_pos_sum_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), x, weight, K, alpha, loss, grad_x);
    return msda::launched(__func__);
}

/* Backward of y = x W^T + b for a 256 -> n layer, n <= 8: dy (T, n) bf16 contiguous, x (T, 256) bf16, w (n, 256) f32 -> dx (T, 256) bf16
 * (or NULL), dw (n, 256) f32 and db (n) f32 (or NULL), both overwritten */
int msda_narrow_linear_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *w, int T, int n, uint16_t *dx, float *dw, float *db,
                                     msda_stream_t stream)
{
    if (!dy || !x || !w || !dw) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (T < 1 || n < 1 || n > 8) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {dx, x})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(dw, 0, sizeof(float) * n * 256, st);
    if (e == hipSuccess && db) e = hipMemsetAsync(db, 0, sizeof(float) * n, st);
    if (e != hipSuccess) return msda::hip_fail(e, __func__);
    if (dx) {
        const long long total = (long long)T * 32;
        hipLaunchKernelGGL(narrow_linear_dx_kernel, dim3((unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096)), dim3(256), 0, st, dy,
                           w, T, n, dx);
    }
    const int chunk = T >= 65536 ? 256 : (T >= 8192 ? 128 : 32);
    hipLaunchKernelGGL(narrow_linear_dw_kernel, dim3((unsigned)((T + chunk - 1) / chunk)), dim3(256), 0, st, dy, x, T, n, chunk, dw, db);
    return msda::launched(__func__);
}

/* y = sigmoid(delta + inverse_sigmoid(ref)): delta (n) bf16 or f32, ref (n) f32, y (n) f32 */
int msda_box_refine_forward(const void *delta, int delta_is_bf16, const float *ref, float eps, int64_t n, float *y, msda_stream_t stream)
{
    if (!delta || !ref || !y) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    if (delta_is_bf16)
        hipLaunchKernelGGL(box_refine_kernel<true>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), delta, ref, eps, (long long)n, y);
    else
        hipLaunchKernelGGL(box_refine_kernel<false>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), delta, ref, eps, (long long)n, y);
    return msda::launched(__func__);
}

/* grad_delta = grad_y * y * (1 - y), written in delta's type */
int msda_box_refine_backward(const float *grad_y, const float *y, int64_t n, void *grad_delta, int delta_is_bf16, msda_stream_t stream)
{
    return msda_box_refine_backward_ref(grad_y, y, n, grad_delta, delta_is_bf16, nullptr, 0.f, nullptr, stream);
}

/* ... and grad_ref (n) f32 = grad_delta * d inverse_sigmoid(ref) / d ref (the clamps' gradients as torch takes them); ref, grad_ref may be NULL */
int msda_box_refine_backward_ref(const float *grad_y, const float *y, int64_t n, void *grad_delta, int delta_is_bf16, const float *ref, float eps,
                                 float *grad_ref, msda_stream_t stream)
{
    if (!grad_y || !y || !grad_delta || (grad_ref && !ref)) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    const int grid = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
    if (delta_is_bf16)
        hipLaunchKernelGGL(box_refine_grad_kernel<true>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), grad_y, y, (long long)n, grad_delta,
                           ref, eps, grad_ref);
    else
        hipLaunchKernelGGL(box_refine_grad_kernel<false>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), grad_y, y, (long long)n, grad_delta,
                           ref, eps, grad_ref);
    return msda::launched(__func__);
}

/* the decoder's positional query embedding: boxes (tokens, >= dims) f32 with row stride ld (floats), dims = 2 | 4 -> out (tokens,
 * dims * pe_dim) bf16 */
int msda_sine_embed_bf16(const float *boxes, int ld, int tokens, int dims, int pe_dim, float temperature, uint16_t *out, msda_stream_t stream)
{
    if (!boxes || !out) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (tokens < 1 || (dims != 2 && dims != 4) || ld < dims || pe_dim < 2 || (pe_dim & 1) || !(temperature > 0.f)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(4, {out})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const long long n = (long long)tokens * dims * (pe_dim / 2);
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(sine_embed_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), boxes, ld, tokens, dims, pe_dim,
                       log2f(temperature), reinterpret_cast<unsigned *>(out));
    return msda::launched(__func__);
}

int msda_attnpool_core_f32(const float *u, const float *feat, const float *pos, const float *spos, int K, int H, int C, int T,
                           int head_major, float *z, msda_stream_t stream)
{
    return attnpool_core_impl<float>(__func__, u, feat, pos, spos, K, H, C, T, head_major, z, stream);
}
int msda_attnpool_core_f64(const double *u, const double *feat, const double *pos, const double *spos, int K, int H, int C, int T,
                           int head_major, double *z, msda_stream_t stream)
{
    return attnpool_core_impl<double>(__func__, u, feat, pos, spos, K, H, C, T, head_major, z, stream);
}

int msda_matcher_cost_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_boxes,
                          const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                          double w_giou, double alpha, float *cost, msda_stream_t stream)
{
    return matcher_cost_impl<float>(__func__, logits, boxes, tgt_ids, tgt_boxes, tgt_offsets, B, Q, C, n_targets, w_class, w_bbox, w_giou, alpha,
                                    cost, stream);
}
int msda_matcher_cost_f64(const double *logits, const double *boxes, const int64_t *tgt_ids, const double *tgt_boxes,
                          const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                          double w_giou, double alpha, double *cost, msda_stream_t stream)
{
    return matcher_cost_impl<double>(__func__, logits, boxes, tgt_ids, tgt_boxes, tgt_offsets, B, Q, C, n_targets, w_class, w_bbox, w_giou, alpha,
                                     cost, stream);
}

int msda_matcher_cost_tm_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_boxes,
                             const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                             double w_giou, double alpha, float *cost, msda_stream_t stream)
{
    return matcher_cost_impl<float, true>(__func__, logits, boxes, tgt_ids, tgt_boxes, tgt_offsets, B, Q, C, n_targets, w_class, w_bbox, w_giou, alpha,
                                          cost, stream);
}
int msda_matcher_cost_tm_f64(const double *logits, const double *boxes, const int64_t *tgt_ids, const double *tgt_boxes,
                             const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                             double w_giou, double alpha, double *cost, msda_stream_t stream)
{
    return matcher_cost_impl<double, true>(__func__, logits, boxes, tgt_ids, tgt_boxes, tgt_offsets, B, Q, C, n_targets, w_class, w_bbox, w_giou, alpha,
                                           cost, stream);
}

int msda_lsap_workspace_bytes(int n_out, int B, int Q, int64_t n_targets, int64_t *bytes)
{
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    int cols_cap = 0, rows_cap = 0;
    size_t lds = 0;
    const int rc = lsap_sizes(n_out, B, Q, n_targets, &cols_cap, &rows_cap, &lds);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    *bytes = 0;      // every supported size keeps its state in LDS
    return MSDA_OK;
}
int msda_lsap_f32(const float *cost, int target_major, const int64_t *tgt_offsets, int n_out, int B, int Q, int64_t n_targets,
                  int64_t *query_of_target, int32_t *status, void *workspace, msda_stream_t stream)
{
    (void)workspace;
    return lsap_impl<float>(__func__, cost, target_major, tgt_offsets, n_out, B, Q, n_targets, query_of_target, status, stream);
}
int msda_lsap_f64(const double *cost, int target_major, const int64_t *tgt_offsets, int n_out, int B, int Q, int64_t n_targets,
                  int64_t *query_of_target, int32_t *status, void *workspace, msda_stream_t stream)
{
    (void)workspace;
    return lsap_impl<double>(__func__, cost, target_major, tgt_offsets, n_out, B, Q, n_targets, query_of_target, status, stream);
}

}  // extern "C"

/* ---- PostProcess on the device (csrc/msda_postproc.h; reference models/richsem/richsem.py:1309-1367) ------------------------------------ */
namespace {

// the argument checks msda_postprocess_workspace_bytes and msda_postprocess_select share
int postprocess_dims(int B, int Q, int C, int k)
{
    if (B < 1 || Q < 1 || C < 1 || k < 1 || k > msda::kPpMaxK) return MSDA_ERR_BAD_DIMS;
    if ((int64_t)Q * C >= ((int64_t)1 << 31)) return MSDA_ERR_TOO_LARGE;
    if (k > (int64_t)Q * C) return MSDA_ERR_BAD_DIMS;
    // the grid (a workgroup per chunk and image) and the words zeroed per call are counted in 32 bits
    const int64_t per_image = msda::pp_chunks((int64_t)Q * C) > msda::kPpZeroWords ? msda::pp_chunks((int64_t)Q * C) : msda::kPpZeroWords;
    if ((int64_t)B * per_image >= ((int64_t)1 << 31)) return MSDA_ERR_TOO_LARGE;
    return MSDA_OK;
}

template <bool BF16>
void postprocess_launch(const void *logits, const float *boxes, const float *sizes_hw, int B, int Q, int C, int k, int box_mode, float *scores,
                        int64_t *labels, float *out_boxes, int64_t *query_idx, unsigned *ws, hipStream_t st)
{
    const int n = Q * C, nchunks = msda::pp_chunks(n);
    unsigned *cand = ws + (size_t)B * msda::kPpZeroWords, *chunk_eq = cand + (size_t)B * 2 * msda::kPpMaxK;
    unsigned *eq_slots = chunk_eq + (size_t)B * nchunks;
    const dim3 grid(nchunks * B), block(msda::kPpThreads);      // (image-major: no limit of a grid's y extent on B)
    for (int round = 0; round < msda::kPpRounds; ++round)
        hipLaunchKernelGGL(msda::pp_hist_kernel<BF16>, grid, block, 0, st, logits, n, k, nchunks, round, ws);
    hipLaunchKernelGGL(msda::pp_compact_kernel<BF16>, grid, block, 0, st, logits, boxes, sizes_hw, Q, C, k, nchunks, box_mode, ws, cand, chunk_eq,
                       eq_slots, scores, labels, out_boxes, query_idx);
}

}  // namespace

extern "C" {

int msda_postprocess_workspace_bytes(int B, int Q, int C, int k, int64_t *bytes)
{
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int rc = postprocess_dims(B, Q, C, k);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    const int64_t words = (int64_t)B * (msda::kPpZeroWords + 2 * msda::kPpMaxK +
                                         (int64_t)(1 + msda::kPpEqSlots) * msda::pp_chunks((int64_t)Q * C));
    *bytes = (words * 4 + 15) & ~(int64_t)15;
    return MSDA_OK;
}

int msda_postprocess_select(const void *logits, int logits_is_bf16, const float *boxes, const float *sizes_hw, int B, int Q, int C, int k,
                            int box_mode, float *scores, int64_t *labels, float *out_boxes, int64_t *query_idx, void *workspace,
                            msda_stream_t stream)
{
    if (!logits || !boxes || !sizes_hw || !scores || !labels || !out_boxes || !query_idx || !workspace)
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int rc = postprocess_dims(B, Q, C, k);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    if (box_mode < 0 || box_mode > 2) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {logits, boxes, out_boxes, workspace})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // histograms, tickets and counters start every call at zero (a replayed graph or a second call on the same workspace starts clean)
    const int zero_words = B * msda::kPpZeroWords;
    hipLaunchKernelGGL(msda::pp_zero_kernel, dim3((zero_words + msda::kPpThreads - 1) / msda::kPpThreads), dim3(msda::kPpThreads), 0, st,
                       static_cast<unsigned *>(workspace), zero_words);
    if (logits_is_bf16)
        postprocess_launch<true>(logits, boxes, sizes_hw, B, Q, C, k, box_mode, scores, labels, out_boxes, query_idx, static_cast<unsigned *>(workspace), st);
    else
        postprocess_launch<false>(logits, boxes, sizes_hw, B, Q, C, k, box_mode, scores, labels, out_boxes, query_idx, static_cast<unsigned *>(workspace), st);
    return msda::launched(__func__);
}

int msda_nms_f32(const float *boxes_xyxy, const int64_t *labels_or_null, int B, int K, float iou_threshold, uint8_t *keep, int64_t *kept_idx,
                 int32_t *n_kept, msda_stream_t stream)
{
    if (!boxes_xyxy || !keep || !kept_idx || !n_kept) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (B < 1 || K < 1 || K > msda::kNmsMaxK) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(16, {boxes_xyxy})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const size_t lds = msda::nms_lds_bytes(K);
    if (lds > 64 * 1024) {      // beyond the default limit of dynamic LDS, as for the assignment solver
        const hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(msda::nms_kernel), msda::nms_lds_bytes(msda::kNmsMaxK));
        if (e != hipSuccess) return msda::hip_fail(e, __func__);
    }
    hipLaunchKernelGGL(msda::nms_kernel, dim3(B), dim3(msda::kNmsMaxK), lds, static_cast<hipStream_t>(stream), boxes_xyxy, labels_or_null, K,
                       iou_threshold, keep, kept_idx, n_kept);
    return msda::launched(__func__);
}

}  // extern "C"

/* ---- module-level helpers that are not the operator: denoising indices and mask (msda_dn.h), per-row top-k (msda_topk.h), ROIAlign
 * (msda_roi.h), padding-mask rows (msda_prep.h).  Their runtime failures read "<entry point>: launch of ...". ------------------------------ */
namespace {

template <typename T>
int roi_align_impl(const char *entry, const T *input, const T *rois, int K, int N, int C, int H, int W, int PH, int PW, double spatial_scale,
                   int sampling_ratio, int aligned, T *output, msda_stream_t stream)
{
    if (!input || !rois || !output) return msda::fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (K < 0 || N < 1 || C < 1 || H < 1 || W < 1 || PH < 1 || PW < 1 || sampling_ratio < 0 || sampling_ratio > msda::kRoiTgtMaxGrid ||
        !(spatial_scale > 0))
        return msda::fail(MSDA_ERR_BAD_DIMS, "bad ROIAlign dimensions");
    const int64_t n_out = (int64_t)K * C * PH * PW;
    if (n_out == 0) return MSDA_OK;
    if ((int64_t)N * C * H * W >= ((int64_t)1 << 40)) return msda::fail(MSDA_ERR_TOO_LARGE, "input too large");
    const int grid = (int)std::min<int64_t>((n_out + 255) / 256, 65536);
    hipLaunchKernelGGL(msda::roi_align_fwd_kernel<T>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), input, rois, n_out, N, C,
                       H, W, PH, PW, (T)spatial_scale, sampling_ratio, aligned, output);
    return msda::launched(entry, ": launch of the ROIAlign kernel");
}

template <typename T>
int mask_rows_impl(const char *entry, T *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream_)
{
    if (!x || !mask) return msda::fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (rows <= 0 || row_elems <= 0) return msda::fail(MSDA_ERR_BAD_DIMS, "non-positive dimension");
    const int grid = (int)std::min<int64_t>((rows + 255) / 256, 4096);
    hipLaunchKernelGGL(msda::mask_rows_kernel<T>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream_), x, mask, (long long)rows, row_elems);
    return msda::launched(entry, ": launch of the padding-mask kernel");
}

}  // namespace

extern "C" {

int msda_dn_indices_i64(const int64_t *cum, int batch, int64_t total, int groups2, int64_t single_pad, int64_t *known_bid,
                        int64_t *map_known_indice, msda_stream_t stream)
{
    if (!cum || !known_bid || !map_known_indice) return msda::fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (batch < 1 || total < 0 || groups2 < 0 || single_pad < 0) return msda::fail(MSDA_ERR_BAD_DIMS, "bad denoising dimensions");
    const int64_t n = total * groups2;
    if (n == 0) return MSDA_OK;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(msda::dn_indices_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), cum, batch, total, n, single_pad,
                       known_bid, map_known_indice);
    return msda::launched(__func__, ": launch of the denoising index kernel");
}

int msda_dn_attn_mask_u8(uint8_t *mask, int64_t tgt_size, int64_t pad_size, int64_t group_pad, msda_stream_t stream)
{
    if (!mask) return msda::fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (tgt_size < 0 || pad_size < 0 || pad_size > tgt_size || group_pad < 0) return msda::fail(MSDA_ERR_BAD_DIMS, "bad mask dimensions");
    if (tgt_size == 0) return MSDA_OK;
    const int64_t n = tgt_size * tgt_size;
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(msda::dn_attn_mask_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), mask, tgt_size, pad_size,
                       group_pad);
    return msda::launched(__func__, ": launch of the denoising mask kernel");
}

int msda_roi_align_forward_f32(const float *input, const float *rois, int K, int N, int C, int H, int W, int pooled_h, int pooled_w,
                               double spatial_scale, int sampling_ratio, int aligned, float *output, msda_stream_t stream)
{
    return roi_align_impl<float>(__func__, input, rois, K, N, C, H, W, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, output, stream);
}
int msda_roi_align_forward_f64(const double *input, const double *rois, int K, int N, int C, int H, int W, int pooled_h, int pooled_w,
                               double spatial_scale, int sampling_ratio, int aligned, double *output, msda_stream_t stream)
{
    return roi_align_impl<double>(__func__, input, rois, K, N, C, H, W, pooled_h, pooled_w, spatial_scale, sampling_ratio, aligned, output, stream);
}

int msda_topk_f32(const float *scores, int rows, int n, int k, int64_t *indices, float *values, msda_stream_t stream)
{
    if (!scores || !indices) return msda::fail(MSDA_ERR_NULL_POINTER, "null pointer argument");
    if (rows < 0 || n < 1 || k < 1 || k > n || k > msda::kTopkMaxK || n > msda::kTopkMaxN)
        return msda::fail(MSDA_ERR_BAD_DIMS, "top-k: 1 <= k <= min(n, %d), n <= %d (got n=%d, k=%d)", msda::kTopkMaxK, msda::kTopkMaxN, n, k);
    if (rows == 0) return MSDA_OK;
    const size_t lds = msda::topk_lds_bytes(n);
    const hipError_t e = msda::set_lds_limit(reinterpret_cast<const void *>(msda::topk_rows_kernel), lds);
    if (e != hipSuccess) return msda::hip_fail(e, __func__, ": LDS limit of the top-k kernel");
    hipLaunchKernelGGL(msda::topk_rows_kernel, dim3(rows), dim3(msda::kTopkThreads), lds, static_cast<hipStream_t>(stream), scores, n, k,
                       indices, values);
    return msda::launched(__func__, ": launch of the top-k kernel");
}

int msda_mask_rows_f32(float *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream)
{
    return mask_rows_impl<float>(__func__, x, mask, rows, row_elems, stream);
}
int msda_mask_rows_f64(double *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream)
{
    return mask_rows_impl<double>(__func__, x, mask, rows, row_elems, stream);
}
int msda_mask_rows_bf16(uint16_t *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream)
{
    return mask_rows_impl<uint16_t>(__func__, x, mask, rows, row_elems, stream);
}

}  // extern "C"
