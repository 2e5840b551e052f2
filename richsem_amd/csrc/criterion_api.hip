// criterion_api.hip -- the C ABI of the criterion over capacity buffers (csrc/msda_criterion.h; include/richsem_msda.h for the contract):
// msda_criterion_workspace_bytes, msda_criterion_pairs_f32, msda_criterion_pairs_ex_f32, msda_criterion_pairs_backward_f32 and the federated
// loss's class subsets from the same slot space (csrc/msda_fed_slots.h): msda_fed_class_mask_slots_f32.  A translation unit of its own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "msda_host.h"
#include "msda_criterion.h"
#include "msda_fed_slots.h"

extern "C" {

/* ---- the criterion over capacity buffers (csrc/msda_criterion.h; include/richsem_msda.h for the contract) ------------------------------- */
static int criterion_dims(int nl, int N, int Q, int Qi, int C, int64_t capacity, int pad_cap)
{
    if (nl < 1 || N < 1 || N > msda::kCritMaxImages || Q < 1 || Qi < 1 || C < 1 || capacity < 1 || pad_cap < 0) return MSDA_ERR_BAD_DIMS;
    // rows and slots are counted in 32 bits
    const int64_t lim = (int64_t)1 << 31;
    if (capacity >= ((int64_t)1 << 24) || (int64_t)nl * N * ((int64_t)pad_cap + Q) >= lim || (int64_t)N * Qi >= lim ||
        (int64_t)(nl + 1) * capacity + (int64_t)nl * N * pad_cap >= lim)
        return MSDA_ERR_TOO_LARGE;
    return MSDA_OK;
}
int msda_criterion_workspace_bytes(int nl, int N, int Q, int Qi, int64_t capacity, int pad_cap, int64_t *bytes)
{
    if (!bytes) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int rc = criterion_dims(nl, N, Q, Qi, 1, capacity, pad_cap);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    *bytes = (int64_t)msda::crit_layout(nl, N, Q, Qi, capacity, pad_cap).bytes;
    return MSDA_OK;
}
static int criterion_pairs_impl(const char *entry, const float *logits, const float *coords, const float *il, const float *ib, const int64_t *cum,
                                const int64_t *tgt_ids, const float *tgt_boxes, const int64_t *query_of_target, const int64_t *dn_meta,
                                const float *num_boxes, int nl, int N, int Q, int Qi, int C, int64_t capacity, int pad_cap, float alpha, float c_cls,
                                float c_l1, float c_giou, int flags, float *row_weight, float *row_weight_int, int32_t *row_group,
                                int32_t *row_group_int, float *terms, int32_t *status, void *workspace, msda_stream_t stream)
{
    if (!logits || !coords || !il || !ib || !cum || !tgt_ids || !tgt_boxes || !query_of_target || !row_weight || !row_weight_int || !terms ||
        !status || !workspace)
        return msda::arg_fail(MSDA_ERR_NULL_POINTER, entry);
    const int rc = criterion_dims(nl, N, Q, Qi, C, capacity, pad_cap);
    if (rc != MSDA_OK) return msda::arg_fail(rc, entry);
    if (!msda::aligned(16, {coords, ib, tgt_boxes, workspace}) || !msda::aligned(8, {cum, tgt_ids, query_of_target, dn_meta}) ||
        !msda::aligned(4, {logits, il, num_boxes, row_weight, row_weight_int, row_group, row_group_int, terms, status}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, entry);
    const msda::CritLayout L = msda::crit_layout(nl, N, Q, Qi, capacity, pad_cap);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    msda::CritArgs a;
    a.logits = logits; a.coords = coords; a.il = il; a.ib = ib;
    a.cum = cum; a.tgt_ids = tgt_ids; a.tgt_boxes = tgt_boxes; a.qot = query_of_target; a.meta = dn_meta; a.num_boxes_in = num_boxes;
    a.nl = nl; a.N = N; a.Q = Q; a.Qi = Qi; a.C = C; a.pad_cap = pad_cap; a.cap = capacity;
    a.alpha = alpha; a.c_cls = c_cls; a.c_l1 = c_l1; a.c_giou = c_giou;
    a.row_weight = row_weight; a.row_weight_int = row_weight_int;
    a.flags = flags; a.row_group = row_group; a.row_group_int = row_group_int;
    a.rec_gb = reinterpret_cast<float4 *>(ws + L.off_gb);
    a.rec_gx = reinterpret_cast<float *>(ws + L.off_gx);
    a.rec_row = reinterpret_cast<int32_t *>(ws + L.off_row);
    a.rec_label = reinterpret_cast<int32_t *>(ws + L.off_label);
    a.partial = reinterpret_cast<double *>(ws + L.off_partial);
    a.stat = reinterpret_cast<int32_t *>(ws + L.off_stat);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(msda::criterion_pairs_kernel, dim3(L.grid_pairs + L.blocks_r), dim3(msda::kCritThreads), 0, st, a, L);
    hipLaunchKernelGGL(msda::criterion_reduce_kernel, dim3(1), dim3(64), 0, st, (const double *)a.partial, (const int32_t *)a.stat, nl, L, terms, status);
    return msda::launched(entry);
}
int msda_criterion_pairs_f32(const float *logits, const float *coords, const float *il, const float *ib, const int64_t *cum, const int64_t *tgt_ids,
                             const float *tgt_boxes, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N,
                             int Q, int Qi, int C, int64_t capacity, int pad_cap, float alpha, float c_cls, float c_l1, float c_giou,
                             float *row_weight, float *row_weight_int, float *terms, int32_t *status, void *workspace, msda_stream_t stream)
{
    return criterion_pairs_impl(__func__, logits, coords, il, ib, cum, tgt_ids, tgt_boxes, query_of_target, dn_meta, num_boxes, nl, N, Q, Qi, C, capacity,
                                pad_cap, alpha, c_cls, c_l1, c_giou, 0, row_weight, row_weight_int, nullptr, nullptr, terms, status, workspace, stream);
}
int msda_criterion_pairs_ex_f32(const float *logits, const float *coords, const float *il, const float *ib, const int64_t *cum, const int64_t *tgt_ids,
                                const float *tgt_boxes, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N,
                                int Q, int Qi, int C, int64_t capacity, int pad_cap, float alpha, float c_cls, float c_l1, float c_giou, int flags,
                                float *row_weight, float *row_weight_int, int32_t *row_group, int32_t *row_group_int, float *terms, int32_t *status,
                                void *workspace, msda_stream_t stream)
{
    if (flags & ~1) return msda::arg_fail(MSDA_ERR_BAD_OPTION, __func__);
    return criterion_pairs_impl(__func__, logits, coords, il, ib, cum, tgt_ids, tgt_boxes, query_of_target, dn_meta, num_boxes, nl, N, Q, Qi, C, capacity,
                                pad_cap, alpha, c_cls, c_l1, c_giou, flags, row_weight, row_weight_int, row_group, row_group_int, terms, status,
                                workspace, stream);
}
int msda_criterion_pairs_backward_f32(const void *workspace, const int64_t *cum, const float *gscale, int nl, int N, int Q, int Qi, int C,
                                      int64_t capacity, int pad_cap, float *grad_logits, float *grad_il, float *grad_coords, float *grad_ib,
                                      msda_stream_t stream)
{
    if (!workspace || !cum || !gscale || !grad_logits || !grad_il || !grad_coords || !grad_ib) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    const int rc = criterion_dims(nl, N, Q, Qi, C, capacity, pad_cap);
    if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
    if (!msda::aligned(16, {workspace, grad_coords, grad_ib}) || !msda::aligned(8, {cum}) || !msda::aligned(4, {gscale, grad_logits, grad_il}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    const msda::CritLayout L = msda::crit_layout(nl, N, Q, Qi, capacity, pad_cap);
    const unsigned char *ws = static_cast<const unsigned char *>(workspace);
    msda::CritBackArgs a;
    a.rec_gb = reinterpret_cast<const float4 *>(ws + L.off_gb);
    a.rec_gx = reinterpret_cast<const float *>(ws + L.off_gx);
    a.rec_row = reinterpret_cast<const int32_t *>(ws + L.off_row);
    a.rec_label = reinterpret_cast<const int32_t *>(ws + L.off_label);
    a.cum = cum; a.gscale = gscale;
    a.nl = nl; a.N = N; a.Q = Q; a.Qi = Qi; a.C = C; a.pad_cap = pad_cap; a.cap = capacity;
    a.grad_logits = grad_logits; a.grad_il = grad_il;
    a.grad_coords = reinterpret_cast<float4 *>(grad_coords);
    a.grad_ib = reinterpret_cast<float4 *>(grad_ib);
    const int grid = (nl + 1) * N + (int)((L.slots_d + msda::kCritThreads - 1) / msda::kCritThreads);
    hipLaunchKernelGGL(msda::criterion_pairs_backward_kernel, dim3(grid), dim3(msda::kCritThreads), 0, static_cast<hipStream_t>(stream), a, L);
    return msda::launched(__func__);
}

/* msda_fed_class_mask_slots_f32 (csrc/msda_fed_slots.h; include/richsem_msda.h for the contract): one workgroup per get_loss call */
int msda_fed_class_mask_slots_f32(const int64_t *cum, const int64_t *tgt_ids, const int64_t *query_of_target, const int64_t *dn_meta,
                                  const float *class_weight, const float *uniform, int nl, int N, int Q, int Qi, int C, int64_t capacity,
                                  int num_sample_cats, int flags, float *mask, int32_t *n_chosen, msda_stream_t stream)
{
    if (!cum || !tgt_ids || !query_of_target || !class_weight || !uniform || !mask || !n_chosen) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (nl < 1 || N < 1 || N > msda::kCritMaxImages || Q < 1 || Qi < 1 || C < 1 || C > msda::kFedSlotsMaxClasses || capacity < 1 || num_sample_cats < 0)
        return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (capacity >= ((int64_t)1 << 24) || nl >= (1 << 20)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);
    if (flags & ~1) return msda::arg_fail(MSDA_ERR_BAD_OPTION, __func__);
    if (!msda::aligned(8, {cum, tgt_ids, query_of_target, dn_meta}) || !msda::aligned(4, {class_weight, uniform, mask, n_chosen}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    int P2 = 1;
    while (P2 < C) P2 <<= 1;
    const int threads = std::min(msda::kFedSlotsThreads, std::max(64, P2 / 2));
    msda::FedSlotsArgs a;
    a.cum = cum; a.tgt_ids = tgt_ids; a.qot = query_of_target; a.meta = dn_meta; a.weight = class_weight; a.uniform = uniform;
    a.nl = nl; a.N = N; a.Q = Q; a.Qi = Qi; a.C = C; a.P2 = P2; a.num_sample_cats = num_sample_cats; a.flags = flags; a.cap = capacity;
    a.mask = mask; a.n_chosen = n_chosen;
    hipLaunchKernelGGL(msda::fed_class_mask_slots_kernel, dim3(2 * nl + 1), dim3(threads), sizeof(unsigned long long) * P2,
                       static_cast<hipStream_t>(stream), a);
    return msda::launched(__func__);
}

}  // extern "C"
