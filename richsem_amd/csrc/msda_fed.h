// msda_fed.h -- the federated loss of the criterion (reference models/richsem/fed_loss.py:15-25, richsem.py:930-961 with use_fed_loss):
// a class subset per loss_labels call -- every class among the matched targets, topped up to num_sample_cats by weighted draws without
// replacement -- and the all-negative focal term restricted to it.  Included by rows_api.hip.
//
// The draw runs on the device with fixed shapes (no torch.unique, no len(), no host copy of the weights), so it can be captured into a graph:
// the uniforms come from the caller's RNG, a replay draws fresh ones.  It is the exponential race (Efraimidis-Spirakis): each eligible class
// c gets the key E_c / w_c, E_c = -log1p(-u_c) ~ Exp(1), and the m smallest keys are the draw.  The smallest of independent Exp(w_c) keys
// is class c with probability w_c / sum w, and by memorylessness the rest race on afresh: the sorted order is a sequence of weighted draws
// without replacement, which is what torch.multinomial(prob, m, replacement=False) samples.
// The focal kernels use focal_neg() of rows_api.hip, which includes this header after defining it.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace msda {

constexpr int kFedMaxClasses = 4096;      // the keys of one group sort in LDS: 4096 x 8 bytes
constexpr int kFedThreads = 1024;

// one workgroup per group g.  keys[] (dynamic LDS) holds P2 = the power of two >= C entries (float_bits(key) << 32) | c: the keys are
// non-negative, so their bit patterns sort like their values, and equal keys sort by the lower class index.  An ineligible class (appeared,
// or weight <= 0 / NaN) gets the high word 0xffffffff, above every float key including +inf, so the eligible classes always sort first.
__global__ __launch_bounds__(kFedThreads) void fed_class_mask_kernel(const int64_t *__restrict__ labels, long long n_labels,
                                                                     const float *__restrict__ weight, const float *__restrict__ uniform, int C,
                                                                     int P2, int num_sample_cats, float *__restrict__ mask,
                                                                     int32_t *__restrict__ n_chosen)
{
    extern __shared__ unsigned long long keys[];
    __shared__ unsigned seen[kFedMaxClasses / 32], taken[kFedMaxClasses / 32];
    __shared__ int n_seen, n_eligible;
    const int tid = threadIdx.x, nt = blockDim.x, g = blockIdx.x, words = (C + 31) >> 5;
    for (int i = tid; i < words; i += nt) seen[i] = taken[i] = 0u;
    if (tid == 0) n_seen = n_eligible = 0;
    __syncthreads();
    for (long long i = tid; i < n_labels; i += nt) {      // the appeared classes (repeats are one class; labels outside [0, C) are ignored)
        const long long l = labels[i];
        if (l >= 0 && l < C) atomicOr(&seen[l >> 5], 1u << (l & 31));
    }
    __syncthreads();
    for (int i = tid; i < words; i += nt) atomicAdd(&n_seen, __popc(seen[i]));
    const float *u = uniform + (long long)g * C;
    int elig = 0;
    for (int c = tid; c < P2; c += nt) {
        unsigned long long k = ~0ull;      // (the padding past C sorts last)
        if (c < C) {
            const float w = weight[c];
            unsigned hi = 0xffffffffu;
            if (!((seen[c >> 5] >> (c & 31)) & 1u) && w > 0.f) {
                const float key = -log1pf(-u[c]) / w;
                hi = key > 0.f ? __float_as_uint(key) : (key == 0.f ? 0u : 0x7f800000u);      // (-0 -> +0; a NaN key -- u outside [0, 1) -- counts as +inf)
                ++elig;
            }
            k = (unsigned long long)hi << 32 | (unsigned)c;
        }
        keys[c] = k;
    }
    if (elig) atomicAdd(&n_eligible, elig);
    __syncthreads();
    // bitonic sort of the P2 keys, ascending
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (P2 >> 1); i += nt) {
                const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    const int m = num_sample_cats - n_seen > 0 ? num_sample_cats - n_seen : 0;
    const int take = m < n_eligible ? m : n_eligible;      // (fewer eligible classes than m: every one of them; torch.multinomial raises)
    for (int i = tid; i < take; i += nt) {
        const unsigned c = (unsigned)(keys[i] & 0xffffffffu);
        atomicOr(&taken[c >> 5], 1u << (c & 31));
    }
    __syncthreads();
    float *out = mask + (long long)g * C;
    for (int c = tid; c < C; c += nt) out[c] = ((seen[c >> 5] | taken[c >> 5]) >> (c & 31)) & 1u ? 1.f : 0.f;
    if (tid == 0) n_chosen[g] = n_seen + take;
}

// the all-negative focal term of msda_focal_neg_sum_f32 / _grad_f32 (rows_api.hip) with a class selector per row: row r counts class c only
// where class_mask[row_group[r]][c] != 0 (a row whose group lies outside [0, groups) counts nothing).  The loops and the reduction are hand copies
// of the unmasked kernels', so that an all-ones mask gives the same bits: a change to either pair goes into both
// (tests/test_gpu_fed_loss.py compares them bit for bit at the grid caps and the column loop's edges).  One templated body for both was
// tried and left out: inlined into these shells it did not compile to the same instructions (profiles/r27_loss_host_layer.md).
__global__ __launch_bounds__(256) void focal_neg_sum_masked_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                   const int32_t *__restrict__ row_group, const float *__restrict__ class_mask,
                                                                   int groups, long long rows, int C, float one_m_alpha,
                                                                   double *__restrict__ partial)
{
    __shared__ double red[256];
    double acc = 0.0;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float wr = w[r];
        const int gr = row_group[r];
        if (wr == 0.f || gr < 0 || gr >= groups) continue;      // (block-uniform)
        const float *mr = class_mask + (long long)gr * C;
        float s = 0.f;
        for (int c = threadIdx.x; c < C; c += 256) {
            float d;
            if (mr[c] != 0.f) s += focal_neg(x[r * C + c], d);
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

__global__ __launch_bounds__(256) void focal_neg_grad_masked_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                    const int32_t *__restrict__ row_group, const float *__restrict__ class_mask,
                                                                    int groups, long long rows, int C, float one_m_alpha,
                                                                    const float *__restrict__ gscale, float *__restrict__ gx)
{
    const float g = gscale[0] * one_m_alpha;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int gr = row_group[r];
        const bool live = gr >= 0 && gr < groups;
        const float wr = live ? w[r] * g : 0.f;
        const float *mr = class_mask + (long long)(live ? gr : 0) * C;
        for (int c = threadIdx.x; c < C; c += 256) {
            float d = 0.f;
            if (wr != 0.f && mr[c] != 0.f) focal_neg(x[r * C + c], d);
            gx[r * C + c] = d * wr;
        }
    }
}

}  // namespace msda
