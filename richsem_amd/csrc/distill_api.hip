// distill_api.hip -- the C ABI of the distillation term over capacity buffers (include/richsem_msda.h for the contract):
// msda_roi_align_targets_f32 (csrc/msda_roi_targets.h), msda_distill_pairs, msda_distill_scatter_f32 / _bf16 (csrc/msda_distill_pairs.h).
// A translation unit of its own: nothing the existing kernels are built from changes with it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "msda_host.h"
#include "msda_roi_targets.h"
#include "msda_distill_pairs.h"

namespace {

// the slot space of msda_distill_pairs; MSDA_OK or the code to report
int distill_pair_dims(int n_d, int N, int Q, int pad_cap, int64_t capacity)
{
    if (n_d < 1 || n_d > 63 || N < 1 || N > msda::kDistPairMaxImages || Q < 1 || pad_cap < 0 || capacity < 1) return MSDA_ERR_BAD_DIMS;
    const int64_t lim = (int64_t)1 << 31;      // rows and slots are counted in 32 bits by the launch geometry
    if (capacity >= ((int64_t)1 << 24) || (int64_t)n_d * N * ((int64_t)pad_cap + Q) >= lim || (int64_t)n_d * (capacity + (int64_t)N * pad_cap) >= lim)
        return MSDA_ERR_TOO_LARGE;
    return MSDA_OK;
}

template <typename TP>
int distill_scatter_impl(const char *entry, const float *grad_rows, const int64_t *pred_row, const int64_t *cum, const float *gscale, int n_d, int N,
                         int Q, int pad_cap, int64_t capacity, int C, TP *grad_pred, msda_stream_t stream)
{
    if (!grad_rows || !pred_row || !cum || !gscale || !grad_pred) return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    if (C < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, entry);
    const int rc = distill_pair_dims(n_d, N, Q, pad_cap, capacity);
    if (rc != MSDA_OK) return msda::arg_fail(rc, entry);
    if (!msda::aligned(8, {pred_row, cum}) || !msda::aligned(4, {grad_rows, gscale}) || !msda::aligned(sizeof(TP), {grad_pred}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, entry);
    const int64_t rows = (int64_t)n_d * N * ((int64_t)pad_cap + Q);
    const int grid = (int)std::min<int64_t>(rows, 16384);
    hipLaunchKernelGGL(msda::distill_scatter_kernel<TP>, dim3(grid), dim3(msda::kDistPairThreads), 0, static_cast<hipStream_t>(stream), grad_rows,
                       pred_row, cum, gscale, n_d, N, Q, pad_cap, capacity, C, grad_pred);
    return msda::launched(entry);
}

}  // namespace

extern "C" {

int msda_roi_align_targets_f32(const float *input, const int64_t *cum, const float *tgt_boxes, const int32_t *sizes, int N, int C, int H, int W,
                               int64_t capacity, int pooled_h, int pooled_w, double spatial_scale, int sampling_ratio, float *output,
                               int32_t *status, msda_stream_t stream)
{
    if (!input || !cum || !tgt_boxes || !sizes || !output || !status) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (N < 1 || N > msda::kRoiTgtMaxImages || C < 1 || H < 1 || W < 1 || capacity < 1 || pooled_h < 1 || pooled_w < 1 ||
        sampling_ratio > msda::kRoiTgtMaxGrid)
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    const int64_t lim = (int64_t)1 << 31;
    const int64_t chunks = (C + msda::kRoiTgtChunk - 1) / msda::kRoiTgtChunk;
    if (capacity >= ((int64_t)1 << 24) || (int64_t)pooled_h * pooled_w >= lim || (int64_t)H * W >= lim || capacity * chunks >= lim)
        return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (!msda::aligned(16, {tgt_boxes}) || !msda::aligned(8, {cum}) || !msda::aligned(4, {input, sizes, output, status}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    msda::RoiTgtArgs a;
    a.input = input; a.cum = cum; a.tgt_boxes = tgt_boxes; a.sizes = sizes;
    a.N = N; a.C = C; a.H = H; a.W = W; a.PH = pooled_h; a.PW = pooled_w; a.sampling_ratio = sampling_ratio;
    a.cap = capacity; a.spatial_scale = (float)spatial_scale;
    a.output = output; a.status = status;
    hipLaunchKernelGGL(msda::roi_align_targets_kernel, dim3((unsigned)(capacity * chunks)), dim3(msda::kRoiTgtThreads), 0,
                       static_cast<hipStream_t>(stream), a);
    return msda::launched(__func__);
}

int msda_distill_pairs(const int64_t *cum, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N, int Q,
                       int pad_cap, int64_t capacity, int64_t layer_mask, int objective, int64_t *pred_row, int64_t *tgt_row, float *row_weight,
                       int32_t *row_group, int32_t *status, msda_stream_t stream)
{
    if (!cum || !query_of_target || !pred_row || !tgt_row || !row_weight || !row_group || !status) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (nl < 1 || nl > 63 || layer_mask <= 0 || (layer_mask >> nl) != 0) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (objective != 0 && objective != 1) return msda::arg_fail(MSDA_ERR_BAD_OPTION, __func__);
    const int n_d = __builtin_popcountll((unsigned long long)layer_mask);
    const int rc = distill_pair_dims(n_d, N, Q, pad_cap, capacity);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    if (!msda::aligned(8, {cum, query_of_target, dn_meta, pred_row, tgt_row}) || !msda::aligned(4, {num_boxes, row_weight, row_group, status}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    msda::DistPairArgs a;
    a.cum = cum; a.qot = query_of_target; a.meta = dn_meta; a.num_boxes_in = num_boxes;
    a.nl = nl; a.N = N; a.Q = Q; a.pad_cap = pad_cap; a.n_d = n_d; a.objective = objective;
    a.cap = capacity; a.layer_mask = (unsigned long long)layer_mask;
    a.pred_row = pred_row; a.tgt_row = tgt_row; a.row_weight = row_weight; a.row_group = row_group; a.status = status;
    const int blocks_m = (int)((capacity + msda::kDistPairThreads - 1) / msda::kDistPairThreads);
    const int blocks_d = (int)(((int64_t)N * pad_cap + msda::kDistPairThreads - 1) / msda::kDistPairThreads);
    hipLaunchKernelGGL(msda::distill_pairs_kernel, dim3(n_d * (blocks_m + blocks_d)), dim3(msda::kDistPairThreads), 0,
                       static_cast<hipStream_t>(stream), a, blocks_m, blocks_d);
    return msda::launched(__func__);
}

int msda_distill_scatter_f32(const float *grad_rows, const int64_t *pred_row, const int64_t *cum, const float *gscale, int n_d, int N, int Q,
                             int pad_cap, int64_t capacity, int C, float *grad_pred, msda_stream_t stream)
{
    return distill_scatter_impl<float>(__func__, grad_rows, pred_row, cum, gscale, n_d, N, Q, pad_cap, capacity, C, grad_pred, stream);
}

int msda_distill_scatter_bf16(const float *grad_rows, const int64_t *pred_row, const int64_t *cum, const float *gscale, int n_d, int N, int Q,
                              int pad_cap, int64_t capacity, int C, uint16_t *grad_pred, msda_stream_t stream)
{
    return distill_scatter_impl<msda::bf16_t>(__func__, grad_rows, pred_row, cum, gscale, n_d, N, Q, pad_cap, capacity, C,
                                              reinterpret_cast<msda::bf16_t *>(grad_pred), stream);
}

}  // extern "C"
