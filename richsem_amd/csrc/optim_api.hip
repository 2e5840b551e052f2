// optim_api.hip -- the C ABI of the library optimizer (include/richsem_msda.h for the contract): msda_optim_plan (host only),
// msda_optim_sumsq, msda_optim_step, msda_optim_ema (csrc/msda_optim.h).
// A translation unit of its own: nothing the existing kernels are built from changes with it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "msda_host.h"
#include "msda_optim.h"

static_assert(sizeof(msda_optim_tensor) == 64 && sizeof(msda_optim_chunk) == 16 && sizeof(msda_optim_group) == 40 &&
                  sizeof(msda_optim_settings) == 24,
              "the table layouts are part of the ABI (richsem_amd/optim.py mirrors them)");

extern "C" {

int msda_optim_plan(const int64_t *numel, int n_tensors, msda_optim_chunk *chunks, int64_t capacity, int64_t *n_chunks)
{
    if (!numel || !n_chunks) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_tensors < 1 || (chunks && capacity < 1)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {numel, chunks, n_chunks})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    int64_t n = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
        n += (numel[t] + MSDA_OPTIM_CHUNK - 1) / MSDA_OPTIM_CHUNK;
        if (n >= ((int64_t)1 << 31)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);      // one workgroup per chunk: the grid
    }
    *n_chunks = n;
    if (!chunks) return MSDA_OK;
    if (n > capacity) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    int64_t c = 0;
    for (int t = 0; t < n_tensors; ++t)
        for (int64_t off = 0; off < numel[t]; off += MSDA_OPTIM_CHUNK, ++c) {
            const int64_t left = numel[t] - off;
            chunks[c].offset = off;
            chunks[c].tensor = t;
            chunks[c].count = (int32_t)(left < MSDA_OPTIM_CHUNK ? left : MSDA_OPTIM_CHUNK);
        }
    return MSDA_OK;
}

int msda_optim_sumsq(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, double *partials, msda_stream_t stream)
{
    if (!tensors || !chunks || !partials) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_chunks < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {tensors, chunks, partials})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipLaunchKernelGGL(msda::optim_sumsq_kernel, dim3((unsigned)n_chunks), dim3(msda::kOptimThreads), 0, static_cast<hipStream_t>(stream), tensors,
                       chunks, partials);
    return msda::launched(__func__);
}

int msda_optim_step(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, const double *partials,
                    const msda_optim_group *groups, const msda_optim_settings *settings, float *total_norm, msda_stream_t stream)
{
    if (!tensors || !chunks || !partials || !groups || !settings || !total_norm) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_chunks < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {tensors, chunks, partials, groups, settings}) || !msda::aligned(4, {total_norm}))
        return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipLaunchKernelGGL(msda::optim_step_kernel, dim3((unsigned)n_chunks), dim3(msda::kOptimThreads), 0, static_cast<hipStream_t>(stream), tensors,
                       chunks, n_chunks, partials, groups, settings, total_norm);
    return msda::launched(__func__);
}

int msda_optim_ema(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, const msda_optim_settings *settings,
                   msda_stream_t stream)
{
    if (!tensors || !chunks || !settings) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_chunks < 1) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {tensors, chunks, settings})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    hipLaunchKernelGGL(msda::optim_ema_kernel, dim3((unsigned)n_chunks), dim3(msda::kOptimThreads), 0, static_cast<hipStream_t>(stream), tensors,
                       chunks, settings);
    return msda::launched(__func__);
}

}  // extern "C"
