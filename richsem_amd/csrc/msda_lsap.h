// msda_lsap.h -- the Hungarian matcher's assignment on the device: an exact linear-sum-assignment solver, one wave per problem.
//
// What the reference hands to scipy.optimize.linear_sum_assignment on the host (models/richsem/matcher.py:76-78), solved where the
// cost blocks already are (msda_matcher.h).  Algorithm: shortest augmenting paths with dual variables (Jonker & Volgenant 1987; the
// form of Crouse, "On implementing 2D rectangular assignment algorithms", IEEE T-AES 2016, which scipy's rectangular_lsap follows):
// the smaller side of the block are the ROWS, augmented one at a time; the larger side the COLUMNS, scanned in every step of the path
// search.  Every reduction, dual variable and path length is float64 whatever the cost dtype, so that with the same cost values the
// optimum found is scipy's wherever it is unique; among equal-cost optima the choice is this kernel's own (DESIGN.md "ties").
//
// Shape: ONE wave64 = one workgroup per problem (output o, image b).  A scan step is a dependent update-then-argmin over the columns,
// bound by latency: lane l owns columns l, l + 64, ... and is the only lane that touches their state (shortest path cost, predecessor
// row, dual v, row of the column, scanned flag -- in LDS, 21 bytes per column), the argmin is a float64 xor-butterfly over the 64
// lanes + one ballot, and NO barrier is met inside the scan.  Barriers (of one wave: free) separate the three phases of an
// augmentation only: scan | dual update | path flip by lane 0.
//
// Termination: every loop has a trip count fixed by the block's size -- min(Q, T) augmentations of at most (rows assigned so far + 1)
// scan steps and as many flips; no exit depends on a floating-point comparison alone.  Non-finite costs never reach the solver: the
// block is scanned for them first (status 1, -1 written).  A scan step that finds no finite candidate (float64 overflow of finite
// costs) ends the problem with status 2.
#pragma once

#include <stdint.h>

#include "msda_common.h"

namespace msda {

constexpr int kLsapMaxDim = 4096;      // Q and the total number of targets, each: the state of 4096 columns + 4096 rows is 148 KB of LDS
constexpr int kLsapBatch = 8;          // columns per lane whose cost loads are issued before the first is used

// LDS bytes of a problem with `nc` columns and `nr` rows: columns {shortest f64, v f64, pred i32, row4col i32, scanned u8}, rows {u f64, col4row i32}
__host__ __device__ inline size_t lsap_lds_bytes(int nc, int nr)
{
    const size_t c8 = ((size_t)nc + 7) & ~(size_t)7, r8 = ((size_t)nr + 7) & ~(size_t)7;
    return c8 * (8 + 8 + 4 + 4 + 1) + r8 * (8 + 4);
}

__device__ __forceinline__ double lsap_wave_min(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o));
    return x;
}

// cost: n_out x (Q * Ttot) elements, output o's blocks as msda_matcher_cost_* lays them (image b's block at Q * tgt_offsets[b]), each
// block query-major (entry (q, t) at q * T_b + t) or, target_major != 0, target-major (t * Q + q).  cols_cap / rows_cap: what the LDS
// was sized for (the host knows Q and Ttot only).  Ttot is a capacity: with tgt_offsets[B] < Ttot the columns of query_of_target past
// tgt_offsets[B] are not written and the cost elements past Q * tgt_offsets[B] are not read.
template <typename T>
__global__ __launch_bounds__(64) void lsap_kernel(const T *__restrict__ cost, int target_major, const int64_t *__restrict__ tgt_offsets, int B,
                                                  int Q, int64_t Ttot, int cols_cap, int rows_cap, int64_t *__restrict__ query_of_target,
                                                  int32_t *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsap_smem[];
    const int lane = threadIdx.x;
    const int o = blockIdx.x / B, b = blockIdx.x - o * B;
    const int64_t t0 = tgt_offsets[b];
    const int64_t tb64 = tgt_offsets[b + 1] - t0;
    int64_t *out = query_of_target + (int64_t)o * Ttot + t0;
    int32_t *st = status + blockIdx.x;
    // offsets that do not describe this launch (negative counts, more targets than Ttot): nothing is read or written through them
    if (t0 < 0 || tb64 < 0 || t0 + tb64 > Ttot) {
        if (lane == 0) *st = 3;
        return;
    }
    const int Tb = (int)tb64;
    for (int t = lane; t < Tb; t += 64) out[t] = -1;
    if (Tb == 0 || Q == 0) {
        if (lane == 0) *st = 0;
        return;
    }
    const T *blk = cost + (int64_t)o * Q * Ttot + (int64_t)Q * t0;
    // ---- non-finite entries: found before anything is solved ------------------------------------------------------------------------
    const int64_t n = (int64_t)Q * Tb;
    bool bad = false;
    for (int64_t i = lane; i < n; i += 64) {
        const double c = (double)blk[i];
        bad |= !(fabs(c) <= 1.7976931348623157e308);
    }
    if (__ballot(bad) != 0ull) {
        if (lane == 0) *st = 1;
        return;
    }
    // ---- rows = the smaller side ------------------------------------------------------------------------------------------------------
    const bool rows_are_targets = Tb <= Q;
    const int nr = rows_are_targets ? Tb : Q, nc = rows_are_targets ? Q : Tb;
    if (nc > cols_cap || nr > rows_cap) {      // (cannot happen with the entry point's sizing: T_b <= Ttot)
        if (lane == 0) *st = 3;
        return;
    }
    // entry (row r, column c) at r * rs + c * cs
    const int64_t q_stride = target_major ? 1 : Tb, t_stride = target_major ? Q : 1;
    const int64_t rs = rows_are_targets ? t_stride : q_stride, cs = rows_are_targets ? q_stride : t_stride;

    const size_t c8 = ((size_t)cols_cap + 7) & ~(size_t)7, r8 = ((size_t)rows_cap + 7) & ~(size_t)7;
    double *shortest = reinterpret_cast<double *>(lsap_smem);
    double *v = shortest + c8;
    double *u = v + c8;
    int *pred = reinterpret_cast<int *>(u + r8);
    int *row4col = pred + c8;
    int *col4row = row4col + c8;
    unsigned char *scanned = reinterpret_cast<unsigned char *>(col4row + r8);

    for (int j = lane; j < nc; j += 64) {
        v[j] = 0.0;
        row4col[j] = -1;
    }
    for (int r = lane; r < nr; r += 64) {
        u[r] = 0.0;
        col4row[r] = -1;
    }
    __syncthreads();

    const double kInf = __longlong_as_double(0x7ff0000000000000ll);
    bool failed = false;
    for (int cur = 0; cur < nr; ++cur) {
        for (int j = lane; j < nc; j += 64) {
            shortest[j] = kInf;
            scanned[j] = 0;
        }
        double min_val = 0.0;
        int i = cur, sink = -1;
        // a step scans one more column, whose row is an assigned row or none (the sink): at most cur + 1 steps
        for (int step = 0; step <= cur && sink < 0; ++step) {
            const double ui = u[i];
            const T *row = blk + (int64_t)i * rs;
            double best = kInf;
            int best_j = -1;
            bool best_free = false;
            for (int j0 = lane; j0 < nc; j0 += 64 * kLsapBatch) {
                T c[kLsapBatch];
#pragma unroll
                for (int k = 0; k < kLsapBatch; ++k) {
                    const int j = j0 + 64 * k;
                    c[k] = j < nc ? row[(int64_t)j * cs] : (T)0;
                }
#pragma unroll
                for (int k = 0; k < kLsapBatch; ++k) {
                    const int j = j0 + 64 * k;
                    if (j < nc && !scanned[j]) {
                        const double r = min_val + (double)c[k] - ui - v[j];
                        double s = shortest[j];
                        if (r < s) {
                            s = r;
                            shortest[j] = r;
                            pred[j] = i;
                        }
                        const bool is_free = row4col[j] < 0;
                        if (s < best || (s == best && is_free && !best_free)) {
                            best = s;
                            best_j = j;
                            best_free = is_free;
                        }
                    }
                }
            }
            const double lowest = lsap_wave_min(best);
            if (!(lowest < kInf)) {      // (wave-uniform) no finite candidate: overflow of finite costs
                failed = true;
                break;
            }
            // the column: among the lanes at the minimum one whose column is free (a shorter path), else the first
            const unsigned long long at_min = __ballot(best == lowest && best_j >= 0);
            const unsigned long long at_min_free = __ballot(best == lowest && best_j >= 0 && best_free);
            const unsigned long long pick = at_min_free ? at_min_free : at_min;
            if (pick == 0ull) {          // (unreachable: lowest is some lane's best)
                failed = true;
                break;
            }
            const int winner = __ffsll((long long)pick) - 1;
            const int j = __shfl(best_j, winner);
            const int rj = __shfl(row4col[best_j < 0 ? 0 : best_j], winner);
            min_val = lowest;
            if (lane == winner) scanned[j] = 1;
            if (rj < 0) sink = j;
            else i = rj;
        }
        if (failed || sink < 0) {
            failed = true;
            break;
        }
        __syncthreads();
        // ---- dual variables: the scanned columns and the rows assigned to them (their rows are distinct: no two lanes write one u) ---------
        for (int j = lane; j < nc; j += 64) {
            if (scanned[j]) {
                const double d = min_val - shortest[j];
                v[j] -= d;
                const int r = row4col[j];
                if (r >= 0) u[r] += d;
            }
        }
        if (lane == 0) u[cur] += min_val;
        __syncthreads();
        // ---- flip the path from the sink back to the new row: at most cur + 1 columns ------------------------------------------------------
        if (lane == 0) {
            int j = sink;
            for (int hop = 0; hop <= cur; ++hop) {
                const int r = pred[j];
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    if (failed) {
        if (lane == 0) *st = 2;
        return;      // (out holds -1)
    }
    if (rows_are_targets) {
        for (int t = lane; t < Tb; t += 64) out[t] = col4row[t];
    } else {
        for (int t = lane; t < Tb; t += 64) out[t] = row4col[t];
    }
    if (lane == 0) *st = 0;
}

}  // namespace msda
