// repack_api.hip -- the C ABI of the grouped re-pack (include/richsem_msda.h for the contract): msda_repack_plan (host only) and
// msda_repack (csrc/msda_repack.h).
// A translation unit of its own: nothing the existing kernels are built from changes with it.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "msda_host.h"
#include "msda_repack.h"

static_assert(sizeof(msda_repack_job) == 160 && sizeof(msda_repack_chunk) == 16 && offsetof(msda_repack_job, seg_end) == 80 &&
                  offsetof(msda_repack_job, n_dst) == 112 && offsetof(msda_repack_job, dims) == 128,
              "the table layouts are part of the ABI (richsem_amd/repack.py mirrors them)");

namespace {

// MSDA_OK, or the class of error of one job of the HOST table
int check_job(const msda_repack_job &j)
{
    if (j.kind < MSDA_REPACK_CAST || j.kind > MSDA_REPACK_CONV_T) return MSDA_ERR_BAD_DIMS;
    if (j.n_segs < 1 || j.n_segs > MSDA_REPACK_MAX_SEGS || j.n_dst < 0) return MSDA_ERR_BAD_DIMS;
    if (j.n_dst >= ((int64_t)1 << 31)) return MSDA_ERR_TOO_LARGE;
    if (j.n_dst == 0) return MSDA_OK;      // an empty job: no chunk, nothing read or written
    if (!j.dst) return MSDA_ERR_NULL_POINTER;
    if (!msda::aligned(16, {j.dst})) return MSDA_ERR_MISALIGNED;
    int64_t prev = 0;
    for (int s = 0; s < j.n_segs; ++s) {
        if (!j.src[s]) return MSDA_ERR_NULL_POINTER;
        if (!msda::aligned(4, {j.src[s]})) return MSDA_ERR_MISALIGNED;
        if (j.seg_end[s] <= prev) return MSDA_ERR_BAD_DIMS;
        prev = j.seg_end[s];
    }
    const int64_t total = prev;
    const int32_t *d = j.dims;
    switch (j.kind) {
    case MSDA_REPACK_CAST:
    case MSDA_REPACK_COPY:
        return total <= j.n_dst ? MSDA_OK : MSDA_ERR_BAD_DIMS;
    case MSDA_REPACK_LIN256:
        return d[0] >= 64 && d[0] % 64 == 0 && j.n_dst == (int64_t)d[0] * 256 && total <= d[0] ? MSDA_OK : MSDA_ERR_BAD_DIMS;
    case MSDA_REPACK_LIN256_T:
        return d[0] >= 64 && d[0] % 64 == 0 && j.n_dst == (int64_t)d[0] * 256 && total == 256 ? MSDA_OK : MSDA_ERR_BAD_DIMS;
    case MSDA_REPACK_FFN_W2:
        return d[0] >= 1 && d[1] >= 32 && d[1] % 32 == 0 && j.n_dst == (int64_t)d[0] * d[1] && total == j.n_dst ? MSDA_OK : MSDA_ERR_BAD_DIMS;
    default: {
        const bool t = j.kind == MSDA_REPACK_CONV_T;
        if (j.n_segs != 1 || d[0] < 1 || d[1] < 1 || d[2] < 1 || d[3] < 1 || d[2] > 16 || d[3] > 16) return MSDA_ERR_BAD_DIMS;
        const int64_t rows = t ? d[1] : d[0], cin = t ? d[0] : d[1];
        const int64_t K = (int64_t)d[2] * d[3] * cin, kpad = (K + 31) / 32 * 32;
        if (rows < 16 || rows % 16 != 0 || (cin % 32 != 0 && K > 512)) return MSDA_ERR_BAD_DIMS;      // (msda_conv_packed_elems' rules)
        if (d[4] != kpad || j.n_dst != rows * kpad || total != (int64_t)d[0] * d[1] * d[2] * d[3]) return MSDA_ERR_BAD_DIMS;
        if (t && !j.scale) return MSDA_ERR_NULL_POINTER;
        if (t && !msda::aligned(4, {j.scale})) return MSDA_ERR_MISALIGNED;
        return MSDA_OK;
    }
    }
}

}  // namespace

extern "C" {

int msda_repack_plan(const msda_repack_job *jobs, int n_jobs, msda_repack_chunk *chunks, int64_t capacity, int64_t *n_chunks)
{
    if (!jobs || !n_chunks) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_jobs < 1 || (chunks && capacity < 1)) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {jobs, chunks, n_chunks})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    int64_t n = 0;
    for (int j = 0; j < n_jobs; ++j) {
        const int rc = check_job(jobs[j]);
        if (rc != MSDA_OK) return msda::arg_fail(rc, __func__);
        n += (jobs[j].n_dst + MSDA_REPACK_CHUNK - 1) / MSDA_REPACK_CHUNK;
        if (n >= ((int64_t)1 << 31)) return msda::arg_fail(MSDA_ERR_TOO_LARGE, __func__);      // one workgroup per chunk: the grid
    }
    *n_chunks = n;
    if (!chunks) return MSDA_OK;
    if (n > capacity) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    int64_t c = 0;
    for (int j = 0; j < n_jobs; ++j)
        for (int64_t off = 0; off < jobs[j].n_dst; off += MSDA_REPACK_CHUNK, ++c) {
            const int64_t left = jobs[j].n_dst - off;
            chunks[c].offset = off;
            chunks[c].job = j;
            chunks[c].count = (int32_t)(left < MSDA_REPACK_CHUNK ? left : MSDA_REPACK_CHUNK);
        }
    return MSDA_OK;
}

int msda_repack(const msda_repack_job *jobs, const msda_repack_chunk *chunks, int n_chunks, msda_stream_t stream)
{
    if (!jobs || !chunks) return msda::arg_fail(MSDA_ERR_NULL_POINTER, __func__);
    if (n_chunks < 0) return msda::arg_fail(MSDA_ERR_BAD_DIMS, __func__);
    if (!msda::aligned(8, {jobs, chunks})) return msda::arg_fail(MSDA_ERR_MISALIGNED, __func__);
    if (n_chunks == 0) return MSDA_OK;
    hipLaunchKernelGGL(msda::repack_kernel, dim3((unsigned)n_chunks), dim3(msda::kRepackThreads), 0, static_cast<hipStream_t>(stream), jobs,
                       chunks);
    return msda::launched(__func__);
}

}  // extern "C"
