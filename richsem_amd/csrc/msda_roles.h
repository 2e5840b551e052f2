// msda_roles.h -- the decoder-shaped backward in ONE launch whose workgroups each do one of its two jobs (gfx950, fp32 compute).
//
// A decoder-shaped backward is two independent halves: grad_value from f64 LDS windows (msda_levelsum.h) and grad_sampling_loc /
// grad_attn_weight from the split kernel (msda_direct.h: no LDS but the level table).  Neither reads what the other writes.  Here a
// workgroup is EITHER a block of split items OR a level-sum entry, chosen from its block index alone.  The two bodies are the
// functions the two-launch kernels are made of, so the arithmetic is theirs.  No workgroup talks to another: nothing depends on
// placement or order.
//
// One launch has one block size, one register budget and one dynamic-LDS size:
//   * every workgroup reserves the level-sum window, so the windows are planned at kDdRolesLdsKb for two workgroups per CU;
//   * two 1024-thread workgroups per CU leave 64 registers: the split body with its point count known at run time (55; the
//     compile-time count of bwd_split_kernel<TV, 4> needs 76 and spills 60 B per lane here).
// Block order: the split workgroups FIRST, then the level-sum entries in the order of levelsum_grid().  A split workgroup holds a
// window-sized share of a CU's LDS like any other, so mixing the kinds buys no residency (spread evenly between the level-sum
// entries the launch is no faster than two launches on scattered locations); first, they are gone after one short round and the
// level-sum entries follow without a kernel boundary (profiles/r24_dd_roles.md).
#pragma once

#include "msda_direct.h"
#include "msda_levelsum.h"

namespace msda {

constexpr int kDdRolesThreads = 1024;
constexpr int kDdRolesLdsKb = 75;      // level-sum windows of this launch: two workgroups per CU

struct DdRoles {
    unsigned sp_blocks;      // split workgroups that have items
    unsigned sp_first;       // block index of the first level-sum entry: sp_blocks rounded up to whole rounds over the XCDs
};

template <int THREADS>
inline DdRoles plan_dd_roles(int64_t items)
{
    DdRoles r;
    r.sp_blocks = (unsigned)((items * 32 + THREADS - 1) / THREADS);
    r.sp_first = (r.sp_blocks + kXcds - 1) / kXcds * kXcds;      // (the level-sum order pins its pairs to XCDs by block index % kXcds)
    return r;
}

// LDS: [L x LevelGeom][window]
inline size_t dd_roles_lds_bytes(int L, size_t window_bytes) { return sizeof(LevelGeom) * L + window_bytes; }

template <typename TV, int THREADS>
__global__ __launch_bounds__(THREADS, 2 * THREADS / 256) void bwd_dd_roles_kernel(
    const TV *__restrict__ value, const int64_t *__restrict__ shapes, const int64_t *__restrict__ lsi,
    const float *__restrict__ loc, const float *__restrict__ aw, const TV *__restrict__ grad_out, TV *__restrict__ grad_value,
    float *__restrict__ grad_loc, float *__restrict__ grad_aw, const LevelSumGeom lg, const DirectGeom g, const DdRoles r)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (blockIdx.x < r.sp_first) {      // (block-uniform)
        if (blockIdx.x >= r.sp_blocks) return;
        LevelGeom *lv = reinterpret_cast<LevelGeom *>(smem);
        load_levels(lv, shapes, lsi, g.L);
        bwd_split_body<TV, 0, THREADS>(blockIdx.x, lv, value, loc, aw, grad_out, grad_loc, grad_aw, g);
    } else {
        double *win = reinterpret_cast<double *>(smem + sizeof(LevelGeom) * g.L);      // (16-byte records: the window stays aligned)
        levelsum_body<true, TV, THREADS>((int)(blockIdx.x - r.sp_first), win, loc, aw, grad_out, grad_value, lg);
    }
}

}  // namespace msda
