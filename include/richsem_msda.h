/*
 * richsem_msda.h -- C ABI of the MI355X (gfx950) multi-scale deformable attention library
 * (librichsem_msda.so, built from richsem_amd/csrc by hipcc --offload-arch=gfx950).
 *
 * This is the drop-in boundary for the reference's native extension
 * `MultiScaleDeformableAttention` (reference models/richsem/ops/src/vision.cpp:13-16):
 *
 *   reference (pybind11 / ATen)                                   this library (extern "C")
 *   ------------------------------------------------------------  ---------------------------
 *   ms_deform_attn_forward   src/ms_deform_attn.h:20-39            msda_forward_{f32,f64}
 *     -> ms_deform_attn_cuda_forward  src/cuda/ms_deform_attn_cuda.cu:20-80
 *   ms_deform_attn_backward  src/ms_deform_attn.h:41-61            msda_backward_{f32,f64}
 *     -> ms_deform_attn_cuda_backward src/cuda/ms_deform_attn_cuda.cu:83-153
 *
 * Plain pointers and sizes only; no torch / ATen types.  All data pointers are DEVICE pointers
 * to contiguous row-major tensors with the reference's layouts
 * (src/cuda/ms_deform_attn_cuda.cu:40-48):
 *
 *   value          (N, S, M, D)            S = sum_l H_l*W_l
 *   spatial_shapes (L, 2) int64            (H_l, W_l)                        [device]
 *   level_start    (L)    int64            start row of level l inside S     [device]
 *   sampling_loc   (N, Lq, M, L, P, 2)     (x, y) normalised to [0,1] over the padded map
 *   attn_weight    (N, Lq, M, L, P)
 *   out / grad_out (N, Lq, M*D)
 *   grad_value, grad_sampling_loc, grad_attn_weight: shaped like value / sampling_loc / attn_weight
 *
 * Differences from the reference binding, all on the ownership side:
 *   - outputs are caller-allocated; they need NOT be zero-filled (the reference allocates them
 *     with at::zeros, ms_deform_attn_cuda.cu:54,121-123; here the library zero-fills what its
 *     kernels accumulate into, on `stream`);
 *   - the HIP stream is an explicit argument (the reference takes the current stream,
 *     ms_deform_attn_cuda.cu:65,135); work is enqueued, never synchronised;
 *   - `shapes_host` / `level_start_host` are optional HOST mirrors of the two int64 tensors.
 *     The launch geometry and the argument checks need the level sizes on the host; when the
 *     mirrors are NULL the library copies them from the device, which synchronises `stream`
 *     (correct, slower; a training loop should pass the mirrors, as the Python shim does);
 *   - errors are returned (and described by msda_last_error()), never only printed as in
 *     ms_deform_im2col_cuda.cuh:948-952.
 *
 * `im2col_step` keeps the reference's contract (N % min(N, im2col_step) == 0, otherwise
 * MSDA_ERR_IM2COL_STEP; ms_deform_attn_cuda.cu:50-52).  Images are independent, so the
 * library processes the whole batch in one launch whatever the step is; results are identical.
 *
 * Thread safety: entry points keep no global mutable state except the option table set by
 * msda_set_option(); they may be called concurrently on different streams (forward thread
 * and autograd thread).
 */
#ifndef RICHSEM_MSDA_H
#define RICHSEM_MSDA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RICHSEM_MSDA_ABI_VERSION 13

/* Return codes: 0 = success; negative = argument error detected on the host (nothing was
 * launched); positive = hipError_t reported by the runtime. */
enum {
    MSDA_OK = 0,
    MSDA_ERR_NULL_POINTER = -1,
    MSDA_ERR_BAD_DIMS = -2,      /* non-positive dimension, sum H*W != S, bad level_start   */
    MSDA_ERR_IM2COL_STEP = -3,   /* N % min(N, im2col_step) != 0                            */
    MSDA_ERR_TOO_LARGE = -4,     /* a tensor has >= 2^31 elements (32-bit index math, as the */
                                 /* reference: ms_deform_im2col_cuda.cuh:255-263)           */
    MSDA_ERR_MISALIGNED = -5,    /* a data pointer is not aligned to its element size        */
    MSDA_ERR_NO_DEVICE = -6,     /* no gfx950 device / code object not loadable              */
    MSDA_ERR_BAD_OPTION = -7,
    MSDA_ERR_NOT_ON_CPU = -8     /* the host ("_cpu") variants: declared, as in the reference, and not implemented */
};

typedef void *msda_stream_t; /* hipStream_t; NULL = the default stream */

int msda_abi_version(void);

/* Text of the last error on the calling thread ("" if none). */
const char *msda_last_error(void);

/* Tuning / test hooks.  Keys:
 *   "fwd_variant"     0 = auto, 1 = direct gather kernel, 2 = LDS-window kernel (when applicable), 3 = split kernel (32 lanes per
 *                     (query, head), all gathers of a lane in flight at once: D = 32, L*P a multiple of 4 up to 32; automatic for
 *                     fp32 calls of fewer than 65536 (query, head) items: decoder-shaped calls)
 *   "bwd_variant"     0 = auto, 1 = direct kernel (level-sum windows / row atomics), 4 = routed pixel-stationary kernels
 *                     (sampling points routed to output tiles in ONE pass -- every query block lays its records out in a stretch of
 *                     its own and announces them to the tiles' bins --, then one workgroup per tile: every pixel of grad_value
 *                     written once with plain stores; cost independent of where the points fall; fp32 / bf16 storage, D = 32,
 *                     L <= 4, Lq <= 320 x 256 per (image, head): up to 320 x 128 queries -- E: 22323, the 1280 x 1280 mosaic
 *                     batches: 34000 -- with 8-wave route workgroups, beyond that with 16-wave ones; otherwise the call falls
 *                     back to 1); 5 = row-band kernel (msda_band.h: grad_value, grad_sampling_loc and grad_attn_weight of a
 *                     decoder-shaped call in ONE launch; a measured option -- 101 us against 88 us for 1 on the decoder call,
 *                     profiles/r05_dd_backward.md -- D = 32 only, else falls back to 1).  auto = routed for encoder-shaped calls
 *                     (Lq == S), direct for the rest
 *   "band_lds_kb"     row-band backward: window budget in KB (16..150, default 64 = two workgroups per CU)
 *   "band_hits"       row-band backward: expected listed points per workgroup above which a band is dealt over query slabs (default 400)
 *   "fwd_prep_fused"  1 (default) = msda_forward_prep_* runs decoder-shaped calls as one kernel, 0 = always two, 2 = encoder-shaped
 *                     calls too: the LDS-window kernel reads the raw projection itself (a measured option: 232 us against 139 us
 *                     for the two-kernel form on the encoder call, profiles/r05_f1_ab.txt)
 *   "locality_monitor"  1 (default) = in auto mode the window forward kernel counts the points that miss their window on the
 *                     first 2 calls of a (problem shape, sampling_loc buffer) and on every 64th after; the count comes back
 *                     by an asynchronous copy and is read on a later call (no call waits, nothing is probed during graph
 *                     capture, up to 8 probes in flight).  Share > 8 % -> direct forward (crossover measured on MI355X,
 *                     profiles/r02_locality.md).  0 = auto always takes the window forward kernel when it applies.  Setting
 *                     it forgets what was learnt.  "locality_share_ppm" (get only): last measured share in parts per
 *                     million, -1 = none.  (The backward needs no monitor.)
 *   "rps_tile"        routed backward: 4..15 = largest tile side + 1; 16 (default) = the planner's choice: rectangles of up to
 *                     30 pixels a side, tile + one row / column <= 312 pixels
 *   "rps_max_chunks"  routed backward: chunks of 1536 points one workgroup takes before a tile's points are dealt over
 *                     several workgroups (default 12)
 *   "rps_route_wgs"   routed backward: workgroups per CU of the route pass (default 2: what is resident)
 *   "rps_seg_shift"   routed backward: a pixel's list is walked in units of at most 2^n sampling points (3..11, default 4)
 *   "levelsum_lds_kb" level-sum window size in KB (8..150, default 150 = one workgroup per CU)
 *   "bwd_direct_cpl"  channels per lane of the direct backward kernel (0 = auto, 1, 2, 4)
 *   "tile_region"     side of an LDS-window region, in pixels of the finest level (default 20)
 *   "tile_margin"     window margin around a region, in pixels of the sampled level (default 6)
 *   "tile_grow"       1 (default) = a window grows into the LDS its phase leaves unused, coarsest level first (per-level
 *                     margins >= tile_margin); 0 = every level uses exactly tile_margin
 *   "bwd_levelsum"    1 (default) = direct backward, fp32: grad_value of whole levels (or row bands of a level) is summed
 *                     in an f64 LDS window by its own kernel and written once.  Calls with Lq*P <= 2^20 whose levels fit 16 windows
 *                     hand over ALL levels: no global atomics, no zero-fill, sums exact to fp32 rounding whatever the order.  Otherwise only
 *                     levels that fit LDS whole and receive >= 2 sampling points per pixel.  0 = off (row atomics only)
 *   "bwd_split"       1 (default) = when the level-sum kernel has produced all of grad_value, small calls (as "fwd_variant" 3) take
 *                     grad_sampling_loc / grad_attn_weight from the split kernel (32 lanes per (query, head)); 0 = the 8-lane kernel
 *   "bwd_dd_roles"    1 (default) = where "bwd_levelsum" hands over all levels and "bwd_split" applies, fp32 storage, P = 4 and
 *                     16-byte aligned sampling_loc / attn_weight: both jobs in ONE launch whose workgroups are either split items or
 *                     level-sum entries on 75-KB windows (msda_roles.h); 0 = the two launches.  "bwd_dd_roles_calls" (get only):
 *                     calls that took the one-launch path so far
 *   "profile_filter"  which calls msda_profile_enable brackets with its event pair: 0 (default) = every call; (kind + 1) * 16 + variant =
 *                     only those (kind 0 forward / 1 backward, variant as in msda_profile_record) -- an event pair costs a call ~4 us
 *   "tile_persist"    persistent workgroups walking the work items (default 512 = 2 per CU; 0 = one workgroup per item)
 * Unknown key or value out of range -> MSDA_ERR_BAD_OPTION.  Options change speed, never results. */
int msda_set_option(const char *key, int value);
int msda_get_option(const char *key, int *value);

/* Host-only: the launch plan the LDS-window kernels would use for a problem (no device access).
 * info[0] = 1 if the window kernels apply (fp32, D = 32, L <= 4, Lq == S, levels contiguous), else 0;
 * info[1], info[2] = region grid (rows, cols); info[3] = LDS phases; info[4] = LDS bytes per workgroup;
 * info[5] = workgroups; info[6] = margin; info[7] = largest number of queries in one region. */
int msda_tiled_plan(int N, int S, int M, int D, int L, int Lq, int P, const int64_t *shapes_host,
                    const int64_t *level_start_host, int info[8]);

/* Host-only: what the level-sum backward kernel (fp32 direct backward, option "bwd_levelsum") would take for a problem.
 * info[0] = bit mask of the levels handed over (0 = none; all L bits = no global atomics and no zero-fill at all);
 * info[1] = (level, row band) windows; info[2] = 4-channel slices; info[3] = LDS bytes per workgroup;
 * info[4] = workgroups; info[5] = most rows in one window; info[6..7] = 0. */
int msda_levelsum_plan(int N, int S, int M, int D, int L, int Lq, int P, const int64_t *shapes_host,
                       const int64_t *level_start_host, int info[8]);

/* Diagnostic: when `device_buffer` is non-NULL the LDS-window kernels write shader-clock stamps into it, 16 x 8 bytes
 * per workgroup (buffer >= workgroups x 128 bytes), one per kernel stage; NULL (default) switches it off. */
int msda_debug_stamps(void *device_buffer);

/* Diagnostic: when `device_counter` (one uint32, caller-zeroed) is non-NULL, the LDS-window FORWARD kernel adds to it
 * the number of sampling points that missed their window and took the general path, counted once per 16-channel half
 * (so a call adds at most 2 * N*Lq*M*L*P).  NULL (default) switches it off. */
int msda_debug_stats(void *device_counter);

/* ---- launch profiler (measurement aid; off by default) ------------------------------------
 * When enabled, every forward/backward call brackets its MAIN kernel (not the zero-fill) with
 * a pair of pre-created HIP events recorded on the stream the kernel is launched on.
 * msda_profile_collect() synchronises those events and returns one record per call, oldest
 * first, then clears the log.  No allocation happens on the launch path. */
typedef struct {
    int kind;        /* 0 = forward, 1 = backward                                  */
    int variant;     /* 1 = direct kernel, 2 = tiled kernel                        */
    int dtype_bytes; /* 4 or 8                                                     */
    int N, S, M, D, L, Lq, P;
    float kernel_ms; /* elapsed time of the main kernel                            */
} msda_profile_record;

int msda_profile_enable(int capacity);  /* capacity = max calls to log; 0 disables and frees   */
int msda_profile_collect(msda_profile_record *records, int max_records, int *n_records);

/* ---- forward:  replaces ms_deform_attn_forward (src/ms_deform_attn.h:20-39) ---------------- */
int msda_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const float *sampling_loc, const float *attn_weight,
                     int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                     float *out,
                     const int64_t *shapes_host, const int64_t *level_start_host,
                     msda_stream_t stream);

int msda_forward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const double *sampling_loc, const double *attn_weight,
                     int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                     double *out,
                     const int64_t *shapes_host, const int64_t *level_start_host,
                     msda_stream_t stream);

/* ---- backward: replaces ms_deform_attn_backward (src/ms_deform_attn.h:41-61) --------------- */
int msda_backward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const float *sampling_loc, const float *attn_weight, const float *grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                      float *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                      const int64_t *shapes_host, const int64_t *level_start_host,
                      msda_stream_t stream);

int msda_backward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const double *sampling_loc, const double *attn_weight, const double *grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                      double *grad_value, double *grad_sampling_loc, double *grad_attn_weight,
                      const int64_t *shapes_host, const int64_t *level_start_host,
                      msda_stream_t stream);

/* ---- host ("_cpu") variants of both (ABI v8).  The reference declares ms_deform_attn_cpu_forward / _backward
 * (src/cpu/ms_deform_attn_cpu.h:14-31) and implements neither: both bodies are AT_ERROR("Not implement on cpu")
 * (src/cpu/ms_deform_attn_cpu.cpp:17-41), and the dispatcher never reaches them (src/ms_deform_attn.h:38,60 raise
 * "Not implemented on the CPU" for a tensor that is not on the device).  These two do the same: they read no
 * argument, launch nothing, set msda_last_error() to the reference's text and return MSDA_ERR_NOT_ON_CPU.  This
 * library has no CPU implementation of the operator (the restatement under oracle/ is test infrastructure). */
int msda_forward_cpu(const void *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const void *sampling_loc, const void *attn_weight,
                     int N, int S, int M, int D, int L, int Lq, int P, int im2col_step, void *out);
int msda_backward_cpu(const void *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const void *sampling_loc, const void *attn_weight, const void *grad_out,
                      int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                      void *grad_value, void *grad_sampling_loc, void *grad_attn_weight);

/* ---- bf16 storage, fp32 compute (new capability: the reference dispatches float / double only,
 * src/cuda/ms_deform_attn_cuda.cu:64,134) -------------------------------------------------------
 * value, out, grad_out, grad_value are bfloat16 (raw 16-bit words, same layouts as above);
 * sampling_loc, attn_weight and their gradients stay float32.  Every sum is formed in fp32 (or in
 * f64 LDS windows) and rounded to bf16 ONCE: grad_value is never accumulated in bf16.  Where the
 * kernels accumulate grad_value with atomics, they do so in an fp32 scratch buffer owned by the
 * library (one per device and stream, allocated on first use -- not while the stream is being
 * captured -- and reused); decoder-shaped calls need no scratch.
 * value / out / grad_out / grad_value must be 8-byte aligned for the fast paths (2 bytes minimum).
 * Kernels are selected by the code that serves the f32 / f64 entry points; where bf16 storage is treated differently is listed
 * in one place, the comment block "kernel selection" of csrc/msda_api.hip. */
int msda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const float *sampling_loc, const float *attn_weight,
                      int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                      uint16_t *out,
                      const int64_t *shapes_host, const int64_t *level_start_host,
                      msda_stream_t stream);

int msda_backward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                       const float *sampling_loc, const float *attn_weight, const uint16_t *grad_out,
                       int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                       uint16_t *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                       const int64_t *shapes_host, const int64_t *level_start_host,
                       msda_stream_t stream);

/* ---- module-level element-wise work ------------------------------------------------
 * What reference models/richsem/ops/modules/ms_deform_attn.py:94-109 does with half a dozen PyTorch ops per call --
 * masked_fill of value, softmax over the L*P logits of a (query, head), offsets / normaliser (+ reference points) --
 * and what autograd replays backwards, as one kernel each way plus an in-place row mask.
 *
 *   offsets    raw output of the sampling_offsets projection: row (n, q) at offsets + (n*Lq + q)*off_stride, M*L*P*2 values
 *   logits     raw output of the attention_weights projection: row (n, q) at logits + (n*Lq + q)*log_stride, M*L*P values
 *              (strides in ELEMENTS: both may point into the output of ONE 256 -> 384 projection, stride 384)
 *   ref        reference points (N, Lq, L, ref_dim), ref_dim = 2 (x, y) or 4 (x, y, w, h), contiguous
 *   shapes_host  HOST copy of spatial_shapes (L, 2) int64 -- the offset normaliser (W_l, H_l) of ref_dim = 2
 *   loc, aw    outputs, contiguous: sampling_loc (N, Lq, M, L, P, 2), attn_weight (N, Lq, M, L, P) -- the operator's inputs
 * msda_prep_backward: grad_loc / grad_aw as returned by msda_backward_*, aw as produced by msda_prep_forward; writes
 *   grad_offsets / grad_logits (with their own row strides: they may be the two parts of ONE gradient tensor) and, when
 *   grad_ref is non-NULL, grad_reference_points (N, Lq, L, ref_dim); `offsets` is only read for ref_dim = 4 with grad_ref.
 * msda_mask_rows: x (rows, row_elems), zeroes IN PLACE every row whose mask byte is non-zero (value rows of padded
 *   pixels forward, grad_value rows backward).  Only masked rows cost memory traffic.
 * L <= 16, L*P <= 64.  float32 and float64 (the module's golden vectors are float64). */
int msda_prep_forward_f32(const float *offsets, int64_t off_stride, const float *logits, int64_t log_stride,
                          const float *ref, int ref_dim, const int64_t *shapes_host,
                          int N, int Lq, int M, int L, int P, float *loc, float *aw, msda_stream_t stream);
int msda_prep_forward_f64(const double *offsets, int64_t off_stride, const double *logits, int64_t log_stride,
                          const double *ref, int ref_dim, const int64_t *shapes_host,
                          int N, int Lq, int M, int L, int P, double *loc, double *aw, msda_stream_t stream);
int msda_prep_backward_f32(const float *grad_loc, const float *grad_aw, const float *aw,
                           const float *offsets, int64_t off_stride, const float *ref, int ref_dim,
                           const int64_t *shapes_host, int N, int Lq, int M, int L, int P,
                           float *grad_offsets, int64_t goff_stride, float *grad_logits, int64_t glog_stride,
                           float *grad_ref, msda_stream_t stream);
int msda_prep_backward_f64(const double *grad_loc, const double *grad_aw, const double *aw,
                           const double *offsets, int64_t off_stride, const double *ref, int ref_dim,
                           const int64_t *shapes_host, int N, int Lq, int M, int L, int P,
                           double *grad_offsets, int64_t goff_stride, double *grad_logits, int64_t glog_stride,
                           double *grad_ref, msda_stream_t stream);
/* the same with a bfloat16 projection: offsets / logits (and their gradients) are raw 16-bit bf16 words -- the output of a bf16
 * GEMM -- while locations, weights, reference points and their gradients are float32 and all arithmetic is fp32 */
int msda_prep_forward_bf16(const uint16_t *offsets, int64_t off_stride, const uint16_t *logits, int64_t log_stride,
                           const float *ref, int ref_dim, const int64_t *shapes_host, int N, int Lq, int M, int L, int P,
                           float *loc, float *aw, msda_stream_t stream);
int msda_prep_backward_bf16(const float *grad_loc, const float *grad_aw, const float *aw,
                            const uint16_t *offsets, int64_t off_stride, const float *ref, int ref_dim,
                            const int64_t *shapes_host, int N, int Lq, int M, int L, int P,
                            uint16_t *grad_offsets, int64_t goff_stride, uint16_t *grad_logits, int64_t glog_stride,
                            float *grad_ref, msda_stream_t stream);
/* msda_forward_prep_*: what msda_prep_forward_* followed by msda_forward_* compute, behind ONE entry point (SURVEY.md section 8f rank 1:
 * "softmax + location math fused into the gather kernel"; reference ops/modules/ms_deform_attn.py:97-114).  Arguments as those two;
 * sampling_loc / attn_weight are OUTPUTS (the module's backward needs them) and must not be NULL.  Decoder-shaped calls (Lq != S,
 * L*P <= 32) run as one kernel that resolves the sampling points from the raw projection and never re-reads sampling_loc; other calls
 * run the two kernels one after the other (the encoder-shaped forward keeps its LDS-window kernel and locality monitor).
 * msda_set_option("fwd_prep_fused", 0) forces the two-kernel form everywhere. */
int msda_forward_prep_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                          const float *offsets, int64_t off_stride, const float *logits, int64_t log_stride,
                          const float *ref, int ref_dim, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                          float *out, float *sampling_loc, float *attn_weight,
                          const int64_t *shapes_host, const int64_t *level_start_host, msda_stream_t stream);
int msda_forward_prep_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                          const double *offsets, int64_t off_stride, const double *logits, int64_t log_stride,
                          const double *ref, int ref_dim, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                          double *out, double *sampling_loc, double *attn_weight,
                          const int64_t *shapes_host, const int64_t *level_start_host, msda_stream_t stream);
int msda_forward_prep_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                           const uint16_t *offsets, int64_t off_stride, const uint16_t *logits, int64_t log_stride,
                           const float *ref, int ref_dim, int N, int S, int M, int D, int L, int Lq, int P, int im2col_step,
                           uint16_t *out, float *sampling_loc, float *attn_weight,
                           const int64_t *shapes_host, const int64_t *level_start_host, msda_stream_t stream);
int msda_mask_rows_f32(float *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream);
int msda_mask_rows_f64(double *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream);
int msda_mask_rows_bf16(uint16_t *x, const uint8_t *mask, int64_t rows, int row_elems, msda_stream_t stream);

/* ---- criterion plumbing: the all-negative term of the sigmoid focal loss, one pass each way -----------------
 * sigmoid_focal_loss at a negative entry is (1 - alpha) p^2 softplus(x) (reference models/richsem/richsem.py:1124-1160 through
 * sigmoid_focal_loss); the criterion sums it over whole logit tensors with one weight per row (query), and corrects the positive entries
 * separately.  logits (rows, C) float32 contiguous; row_weight (rows) float32 (0 = the row carries no loss).
 * msda_focal_neg_sum_f32 writes *n_partial <= max_partial fp64 partial sums (add them up); msda_focal_neg_grad_f32 writes
 * grad_logits = gscale[0] * d(sum)/d(logits) for every element (gscale: a device scalar, the upstream gradient). */
int msda_focal_neg_sum_f32(const float *logits, const float *row_weight, int64_t rows, int C, float alpha, double *partial, int max_partial,
                           int *n_partial, msda_stream_t stream);
int msda_focal_neg_grad_f32(const float *logits, const float *row_weight, int64_t rows, int C, float alpha, const float *gscale,
                            float *grad_logits, msda_stream_t stream);

/* ---- the federated loss (ABI v9; reference models/richsem/fed_loss.py:15-25 through SetCriterion.loss_labels, richsem.py:930-961 with
 * use_fed_loss): each loss_labels call takes the focal loss over a class subset only -- every class among the matched targets, topped up to
 * num_sample_cats classes drawn without replacement with probability proportional to a class weight (image_count ** 0.5, set_cats) -- with a
 * fresh draw per call.  Here the draw runs on the device with fixed shapes, so it can be captured into a graph and replayed.
 * msda_fed_class_mask_f32: labels (n_labels) int64 (the matched targets' classes, shared by every group; repeats and n_labels = 0 allowed,
 *   classes outside [0, C) ignored), class_weight (C) float32 (weight <= 0: never drawn), uniform (groups, C) float32 in [0, 1) (the caller's
 *   RNG; one independent draw per group) -> mask (groups, C) float32: 1 for every appeared class and for m = max(num_sample_cats - a, 0)
 *   more (a = distinct appeared classes), 0 elsewhere; n_chosen (groups) int32 = a + min(m, eligible).  The m classes of group g are those
 *   with the smallest keys -log1p(-u) / w (the exponential race: the distribution of m sequential weighted draws without replacement, that is
 *   of torch.multinomial(w, m, replacement=False)), ties to the lower class index.  Where fewer than m classes are eligible (weight > 0, not
 *   appeared) every eligible class is taken -- torch.multinomial raises there instead; n_chosen says so.  C <= 4096, one workgroup per group.
 * msda_focal_neg_sum_masked_f32 / msda_focal_neg_grad_masked_f32: msda_focal_neg_sum_f32 / _grad_f32 with row r counting class c only
 *   where class_mask[row_group[r]][c] != 0 (row_group (rows) int32; class_mask (groups, C) float32, a 0 / 1 selector; a row whose group lies
 *   outside [0, groups) counts nothing).  The gradient is written at every element and is exactly 0 where the mask is 0; an all-ones mask
 *   gives the bits of the unmasked functions. */
int msda_fed_class_mask_f32(const int64_t *labels, int64_t n_labels, const float *class_weight, const float *uniform, int groups, int C,
                            int num_sample_cats, float *mask, int32_t *n_chosen, msda_stream_t stream);
int msda_focal_neg_sum_masked_f32(const float *logits, const float *row_weight, const int32_t *row_group, const float *class_mask, int groups,
                                  int64_t rows, int C, float alpha, double *partial, int max_partial, int *n_partial, msda_stream_t stream);
int msda_focal_neg_grad_masked_f32(const float *logits, const float *row_weight, const int32_t *row_group, const float *class_mask, int groups,
                                   int64_t rows, int C, float alpha, const float *gscale, float *grad_logits, msda_stream_t stream);

/* ---- the distillation term (ABI v12; reference SetCriterion.loss_labels, models/richsem/richsem.py:967-1024): the detector's CLIP-space
 * outputs pulled toward the frozen CLIP teacher's, over K gathered rows.  Row k reads pred[pred_row[k]] and tgt[tgt_row[k]] (pred (pred_rows,
 * C), tgt (tgt_rows, C) contiguous; pred_row / tgt_row (K) int64 ON THE DEVICE -- the kernel guards them) with the weight row_weight[k]
 * (K float32).  loss[0] (float32) <- the sum of the row losses, accumulated in f64; grad_rows (K, C) float32 <- d loss / d (the gathered student
 * row), every element written; the teacher gets no gradient; the caller scatters the rows (rows that repeat in pred_row add) and multiplies
 * by the incoming scalar gradient.  Value and gradient come from one launch, the total from a second small one; fixed shapes, no host
 * synchronisation, no floating-point atomic: capturable, and the same inputs give the same bits.  K == 0 writes loss = 0 only.
 * workspace: MSDA_DISTILL_WORKSPACE_BYTES of device memory owned by the CALLER (8-byte aligned; needed when K > 0; contents do not matter
 * before and are garbage after): the workgroups' f64 partial sums.  The library keeps no memory for these calls, so a call -- eager,
 * captured, or replayed on any stream -- touches its arguments only; two calls that may run at the same time need a workspace each.
 * A row contributes loss 0 and a zero gradient row when row_weight[k] == 0, when pred_row[k] / tgt_row[k] lies outside [0, pred_rows) /
 * [0, tgt_rows), when row_group[k] lies outside [0, groups), or when its class subset is empty.
 * msda_distill_kl_f32 / msda_distill_kl_bf16 (distill_type 'clip_logits'): S_k = all C classes (row_group = class_mask = NULL, groups = 0),
 *   or the classes with class_mask[row_group[k]][c] != 0 (row_group (K) int32, class_mask (groups, C) float32: use_fed_on_kd);
 *     p = softmax(pred row over S_k),  t = softmax(tgt row over S_k),
 *     row_loss_k = w_k dw_k sum_{c in S_k} t_c (log t_c - log p_c),     grad_rows[k][c] = w_k dw_k (p_c - t_c) on S_k, exactly 0 elsewhere,
 *     dw_k = 1 (dynamic_weight = 0) or 2 H(softmax(tgt row over ALL C classes)) / ln C (dynamic_weight = 1: use_dynamic_distill_weight, formed
 *     before the subset is taken, as the reference does; needs C >= 2).
 *   log t and log p are formed analytically (x - max - log sum exp): an underflowed t_c = 0 contributes exactly 0 (F.kl_div's xlogy
 *   convention), in the entropy too -- where the reference's tgt_prob * tgt_prob.log() is NaN -- so no term is NaN for finite inputs.
 *   The bf16 entry point takes the student's logits in bf16 storage (the teacher's stay float32) and computes in f32 after the upcast: no
 *   float32 copy of the student's logit tensor is needed.
 * msda_distill_l1_f32 (distill_type 'clip_l1'; D >= 1 channels):  u = pred row / |pred row|_2,  v = tgt row (normalize_target = 0: objective
 *   'gt') or tgt row / |tgt row|_2 (1: 'pred', 'pred_all');  row_loss_k = w_k |u - v|_1;  grad_rows[k] = w_k (s - u (u . s)) / |pred row|_2 with
 *   s = sign(u - v), sign(0) = 0 (as torch differentiates |x|). */
#define MSDA_DISTILL_WORKSPACE_BYTES 16384
int msda_distill_kl_f32(const float *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                        const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                        int dynamic_weight, double *workspace, float *loss, float *grad_rows, msda_stream_t stream);
int msda_distill_kl_bf16(const uint16_t *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int C, const int64_t *pred_row,
                         const int64_t *tgt_row, const float *row_weight, int64_t K, const int32_t *row_group, const float *class_mask, int groups,
                         int dynamic_weight, double *workspace, float *loss, float *grad_rows, msda_stream_t stream);
int msda_distill_l1_f32(const float *pred, int64_t pred_rows, const float *tgt, int64_t tgt_rows, int D, const int64_t *pred_row,
                        const int64_t *tgt_row, const float *row_weight, int64_t K, int normalize_target, double *workspace, float *loss,
                        float *grad_rows, msda_stream_t stream);

/* ---- the batch-geometry tensors (ABI v13): everything the reference derives from the padding mask at the start of a forward -- the per-level
 * masks (F.interpolate of the image mask, models/richsem/richsem.py:593-612), get_valid_ratio (deformable_transformer.py:253-260), the
 * encoder's reference points (:513-525), PositionEmbeddingSineHW (position_encoding.py:46-92, normalize=True, scale 2 pi) and the geometry
 * half of gen_encoder_output_proposals (utils.py:10-65) -- from the image sizes, in ONE launch.  Every padding mask the reference builds is a
 * bottom / right rectangle (pixel (y, x) of image n is padding iff y >= h_n or x >= w_n), so all of it is a closed form of the sizes.
 *   sizes (N, 2) int32 ON THE DEVICE: (h_n, w_n), clamped there to [1, canvas_h] x [1, canvas_w]; shapes (L, 2) int32 ON THE HOST: (h_l, w_l)
 *   of the pyramid's levels, 1 <= L <= 8; S = sum_l h_l w_l.  A level's pixel (y, x) is padding iff src_y(y) >= h_n or src_x(x) >= w_n with
 *   src(i) = min(int(floorf(i * (float(in) / out))), in - 1), the nearest-neighbour rule of F.interpolate; vh_l / vw_l = the level's count of
 *   valid rows / columns under that rule.
 *   mask_flat (N, S) u8         1 = padding                                                                         (always written)
 *   valid_ratios (N, L, 2) f32  (float(vw_l) / w_l, float(vh_l) / h_l)                                              (always written)
 *   ref (N, S, L, 2) f32        [.., k, :] = ((x + 0.5) / (ratio_w_l * w_l) * ratio_w_k, (y + 0.5) / (ratio_h_l * h_l) * ratio_h_k)   (or NULL)
 *   pos_sine (N, S, 2 F) f32    F = num_pos_feats (even, <= 256); channels [0, F) from y_embed with temperature_h, [F, 2 F) from x_embed
 *                               with temperature_w: y_embed = (x < vw) ? min(y + 1, vh) : 0 over (vh or 0) + 1e-6, times 2 pi, over
 *                               dim_t[i] = temperature ** (2 * (i / 2) / F); even channels sin, odd channels cos                         (or NULL)
 *   proposals (N, S, 4) f32     log(p / (1 - p)) of p = ((x + 0.5) / vw, (y + 0.5) / vh, 0.05 * 2^l, 0.05 * 2^l); +inf in all four where
 *   zeroed (N, S) u8            the pixel is padding or one of the four lies outside (0.01, 0.99) -- 1 there        (both, or both NULL)
 * float32 arithmetic in the reference's operation order with IEEE division.  Alignment: valid_ratios and ref 8 bytes, pos_sine and proposals
 * 16 (MSDA_ERR_MISALIGNED).  N * S and the workgroup count (N * sum_l ceil(h_l w_l / 32)) below 2^31 (MSDA_ERR_TOO_LARGE).  A null required
 * pointer, proposals without zeroed or the reverse (MSDA_ERR_NULL_POINTER); N < 1, a canvas < 1, L outside 1..8, a non-positive shape,
 * num_pos_feats odd, < 2 or > 256, 2 * num_pos_feats not a multiple of 4, a temperature <= 0 (MSDA_ERR_BAD_DIMS): refused before any launch.
 * No host synchronisation, no allocation, no atomic: capturable; a replay follows the sizes tensor's current contents. */
int msda_batch_geometry_f32(const int32_t *sizes, int N, int canvas_h, int canvas_w, const int32_t *shapes, int L, int num_pos_feats,
                            float temperature_h, float temperature_w, uint8_t *mask_flat, float *valid_ratios, float *ref, float *pos_sine,
                            float *proposals, uint8_t *zeroed, msda_stream_t stream);

/* The criterion's per-pair tails, one launch each (K pairs, float32): loss[0] <- the weighted sum, grad <- its gradient w.r.t. the
 * predictions (multiply by the incoming scalar gradient).  msda_box_pair_loss_f32: sum_k w[k] (c_l1 |p_k - t_k|_1 + c_giou (1 - GIoU(p_k,
 * t_k))) for boxes (cx, cy, w, h) (SetCriterion.loss_boxes, models/richsem/richsem.py:1162-1188; util/box_ops.py:9-64 on the diagonal;
 * gradients with torch's conventions for |x|, max / min and clamp); msda_focal_pos_sum_f32: sum_k w[k] (alpha (1 - q)^2 softplus(-x_k) -
 * (1 - alpha) q^2 softplus(x_k)), q = sigmoid(x_k) -- a positive entry's share of the sigmoid focal loss (richsem.py:1124-1160) minus the
 * all-negative term that msda_focal_neg_sum_f32 counted for it. */
int msda_box_pair_loss_f32(const float *pred, const float *target, const float *weight, int K, float c_l1, float c_giou, float *loss, float *grad_pred,
                           msda_stream_t stream);
int msda_focal_pos_sum_f32(const float *x, const float *weight, int K, float alpha, float *loss, float *grad_x, msda_stream_t stream);

/* ---- the criterion's pair terms over CAPACITY buffers (csrc/msda_criterion.h; reference SetCriterion.forward, models/richsem/richsem.py:
 * 1124-1298 with prep_for_dn :1300-1306): which pairs carry a loss is read ON THE DEVICE, so a captured launch serves every batch that fits
 * the capacities.  The two per-pair formulas are those of the two entry points above.
 *   logits (nl, N, pad_cap + Q, C), coords (nl, N, pad_cap + Q, 4)   the nl decoder outputs: pad_cap denoising rows, then Q matching rows
 *   il (N, Qi, C), ib (N, Qi, 4)                                     the two-stage output
 *   cum (N + 1) int64             exclusive prefix of the per-image target counts; cum[N] <= capacity targets are live
 *   tgt_ids (capacity) int64, tgt_boxes (capacity, 4) cxcywh        rows past cum[N] are not read
 *   query_of_target (nl + 1, capacity) int64                        as msda_lsap_* writes it for the nl + 1 outputs; columns past cum[N] are not read
 *   dn_meta int64[5] or NULL      (single_pad, num_dn_group, pad_size, total, overflow) of msda_dn_queries_f32; NULL: no denoising part
 *   num_boxes float[1] or NULL    the normaliser; NULL: max(1, live pairs of the last decoder output), counted in the kernel
 * Matched slot (o, t): live iff t < cum[N] and 0 <= q = query_of_target[o][t] < Q (Qi for o == nl); prediction row pad_cap + q of the target's
 * image; weight 1 / num_boxes.  Denoising slot (l, b, s), s < pad_cap: stride = pad_size / num_dn_group; live iff overflow == 0, s < pad_size and
 * j = s % stride < T_b; target cum[b] + j; prediction row s; weight 1 / (num_boxes * num_dn_group).  Weights are formed in float64 and rounded once.
 * Outputs:
 *   row_weight (nl, N, pad_cap + Q), row_weight_int (N, Qi)   the row_weight of msda_focal_neg_*: denoising rows below pad_size 1 / (num_boxes *
 *                                 num_dn_group), rows in [pad_size, pad_cap) 0 (all of them 0 on overflow or without dn_meta), matching rows 1 / num_boxes
 *   terms (2 nl + 1, 3) f32       per get_loss call -- the matching part of layers 0..nl-1, their denoising parts, the two-stage output -- the sums
 *                                 of (the positive entries' focal correction, |p - t|_1, 1 - GIoU), each divided by the call's normaliser
 *   status int32[4]               [0] the denoising layout does not fit (overflow set, pad_size > pad_cap or not a multiple of num_dn_group): the
 *                                 denoising part is left out; [1] live targets without a query (-1, or outside the output's queries), over the
 *                                 nl + 1 outputs; [2] live targets with a label outside [0, C): their pairs are left out, nothing is read through
 *                                 the label; [3] cum does not start at 0, decreases or exceeds capacity: every pair is left out
 *   workspace                     msda_criterion_workspace_bytes() bytes, 16-byte aligned: the backward's per-slot records and the partial sums;
 *                                 contents irrelevant on entry, every byte the backward reads is written by this call
 * Sums: wave shuffles, one float64 partial per workgroup, added in workgroup order by a second small launch: no floating-point atomic, results
 * are bitwise reproducible.  No host synchronisation, no allocation: capturable.
 * msda_criterion_pairs_backward_f32 (after msda_criterion_pairs_f32 on the same workspace and cum): grad_coords (nl, N, pad_cap + Q, 4) and
 * grad_ib (N, Qi, 4) <- gscale[0] * d(c_l1 * L1 + c_giou * (1 - GIoU) terms) / d box, written whole (zero where no pair points);
 * grad_logits / grad_il += gscale[0] * c_cls * d(focal correction) / d logit at the positive entries -- ADDED to what msda_focal_neg_grad_f32
 * wrote there before on the same stream; every entry is touched by one slot, no atomic.
 * Limits: N <= 1024, capacity < 2^24, rows and slots below 2^31 (MSDA_ERR_TOO_LARGE); nl, N, Q, Qi, C, capacity >= 1, pad_cap >= 0
 * (MSDA_ERR_BAD_DIMS); boxes, box gradients and workspace 16-byte aligned, int64 inputs 8 (MSDA_ERR_MISALIGNED). */
int msda_criterion_workspace_bytes(int nl, int N, int Q, int Qi, int64_t capacity, int pad_cap, int64_t *bytes);
int msda_criterion_pairs_f32(const float *logits, const float *coords, const float *il, const float *ib, const int64_t *cum, const int64_t *tgt_ids,
                             const float *tgt_boxes, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N,
                             int Q, int Qi, int C, int64_t capacity, int pad_cap, float alpha, float c_cls, float c_l1, float c_giou,
                             float *row_weight, float *row_weight_int, float *terms, int32_t *status, void *workspace, msda_stream_t stream);
int msda_criterion_pairs_backward_f32(const void *workspace, const int64_t *cum, const float *gscale, int nl, int N, int Q, int Qi, int C,
                                      int64_t capacity, int pad_cap, float *grad_logits, float *grad_il, float *grad_coords, float *grad_ib,
                                      msda_stream_t stream);
/* msda_criterion_pairs_ex_f32: msda_criterion_pairs_f32 with options (that entry point is this one with flags = 0 and both row_group
 * pointers NULL: the same launches, the same bits).
 *   flags & 1                     enc_cls_agn (richsem.py:1249-1255): the slots of the two-stage output take label 0 instead of tgt_ids -- in the
 *                                 positive entry's focal correction, in the record the backward scatters from and in the range check (label 0 is
 *                                 always in range: such a slot is never left out for its label).  Other bits: MSDA_ERR_BAD_OPTION.
 *   row_group (nl, N, pad_cap + Q) int32, row_group_int (N, Qi) int32, each or NULL: the get_loss call of every row, written by the threads
 *                                 that write row_weight -- rows s < pad_cap of layer l: nl + l; rows s >= pad_cap: l; two-stage rows: 2 nl.  It
 *                                 is the row_group of msda_focal_neg_{sum,grad}_masked_f32 for a class_mask of 2 nl + 1 rows.
 * The backward is msda_criterion_pairs_backward_f32, unchanged: the record carries the class.
 *
 * msda_fed_class_mask_slots_f32 (csrc/msda_fed_slots.h): msda_fed_class_mask_f32 with the appeared classes of each group read from the slot
 * space above instead of a label list of exact length.  One workgroup per get_loss call g in 0 .. 2 nl, numbered as `terms`:
 *   g < nl            the labels tgt_ids[t] of the slots t < cum[N] with 0 <= query_of_target[g][t] < Q
 *   nl <= g < 2 nl    nothing if dn_meta is NULL, overflow != 0, pad_size == 0 (or num_dn_group < 1, or pad_size no multiple of it); else
 *                     tgt_ids[cum[b] + j] for every image b and j < min(T_b, pad_size / num_dn_group)
 *   g == 2 nl         as g < nl with row nl of query_of_target and Qi queries; with flags & 1 the label of every such slot is 0
 * Labels outside [0, C) appear nowhere; a cum that does not start at 0, decreases or exceeds capacity leaves every group empty.  So a class is
 * appeared in group g iff msda_criterion_pairs_ex_f32 (same arguments, same flags, dn_meta from msda_dn_queries_f32 run with the pair call's
 * pad_cap -- a layout that does not fit pad_cap has overflow set) counts a positive entry of that class in call g.
 *   class_weight (C), uniform (2 nl + 1, C), num_sample_cats -> mask (2 nl + 1, C), n_chosen (2 nl + 1): as msda_fed_class_mask_f32, and bit for
 *   bit what that function gives for group g's exact label list and uniform row g (same keys, same order of ties, same fewer-eligible rule).
 * No global atomic, no workspace, no host synchronisation: capturable.  Limits: 1 <= C <= 4096, N <= 1024, nl, Q, Qi, capacity >= 1,
 * num_sample_cats >= 0 (MSDA_ERR_BAD_DIMS); capacity < 2^24, nl < 2^20 (MSDA_ERR_TOO_LARGE); flags within bit 0 (MSDA_ERR_BAD_OPTION); int64
 * inputs 8-byte aligned (MSDA_ERR_MISALIGNED). */
int msda_criterion_pairs_ex_f32(const float *logits, const float *coords, const float *il, const float *ib, const int64_t *cum, const int64_t *tgt_ids,
                                const float *tgt_boxes, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N,
                                int Q, int Qi, int C, int64_t capacity, int pad_cap, float alpha, float c_cls, float c_l1, float c_giou, int flags,
                                float *row_weight, float *row_weight_int, int32_t *row_group, int32_t *row_group_int, float *terms, int32_t *status,
                                void *workspace, msda_stream_t stream);
int msda_fed_class_mask_slots_f32(const int64_t *cum, const int64_t *tgt_ids, const int64_t *query_of_target, const int64_t *dn_meta,
                                  const float *class_weight, const float *uniform, int nl, int N, int Q, int Qi, int C, int64_t capacity,
                                  int num_sample_cats, int flags, float *mask, int32_t *n_chosen, msda_stream_t stream);

/* ---- the distillation term over CAPACITY buffers (csrc/msda_roi_targets.h, csrc/msda_distill_pairs.h; reference models/richsem/richsem.py:
 * 745-761 for the teacher's box targets, :967-1024 with :1158-1180 for the term): the teacher's ROI rows, the (student row, teacher row)
 * pairs and the gradient's scatter, all shaped by the capacities and read ON THE DEVICE, so a captured launch serves every batch that fits.
 *
 * msda_roi_align_targets_f32: ROIAlign forward (aligned) of the target boxes.
 *   input (N, C, H, W) f32; cum (N + 1) int64; tgt_boxes (capacity, 4) cxcywh normalised f32; sizes (N, 2) int32 (h, w) of the images
 *   output (capacity, C, pooled_h, pooled_w) f32, every element written; status int32[4]: [3] = 1 when cum does not start at 0, decreases
 *   or exceeds capacity (every slot is then dead), [0..2] = 0
 * Slot t is live iff t < cum[N]; its image is the b with cum[b] <= t < cum[b + 1].  A dead slot is exact zeros and reads nothing through
 * its box.  The pixel box (x1, y1, x2, y2) = (w_b (cx - 0.5 w), h_b (cy - 0.5 h), w_b (cx + 0.5 w), h_b (cy + 0.5 h)) is formed in float32
 * with one rounding per operation and no contraction, as clip_box_targets forms it in torch; from there the algorithm of
 * msda_roi_align_forward_f32.  A live slot whose pixel box is not finite, or whose sampling grid would exceed 4096 per axis, is zeros.
 * Limits: N <= 1024, capacity < 2^24, the workgroup count capacity * ceil(C / 64) below 2^31 (MSDA_ERR_TOO_LARGE); N, C, H, W, capacity,
 * pooled_h, pooled_w >= 1, sampling_ratio <= 4096 (<= 0: adaptive) (MSDA_ERR_BAD_DIMS); tgt_boxes 16-byte aligned, cum 8 (MSDA_ERR_MISALIGNED).
 *
 * msda_distill_pairs: ONE launch that writes, for K = n_d * capacity + n_d * N * pad_cap slots, the arguments msda_distill_kl_f32 / _bf16 /
 * msda_distill_l1_f32 take -- those run unchanged over all K slots and skip the dead ones.  layer_mask: bit l set = decoder layer l is
 * distilled (0 < layer_mask < 2^nl); n_d = its popcount; the student tensor is (n_d, N, pad_cap + Q, C), the selected layers stacked in
 * increasing order.  cum, query_of_target (nl + 1, capacity), dn_meta, num_boxes: as for msda_criterion_pairs_f32.  objective 0 = 'gt', 1 = 'pred'.
 *   matched slot k = i * capacity + t: live iff t < cum[N] and 0 <= q = query_of_target[layer_i][t] < Q; pred_row = (i N + b)(pad_cap + Q) +
 *     pad_cap + q; tgt_row = t ('gt') or pred_row ('pred'); row_weight = 1 / num_boxes; row_group = i
 *   denoising slot k = n_d * capacity + (i N + b) pad_cap + s: live iff overflow == 0, s < pad_size and j = s % (pad_size / num_dn_group) < T_b;
 *     pred_row = (i N + b)(pad_cap + Q) + s; tgt_row = cum[b] + j or pred_row; row_weight = 1 / (num_boxes * num_dn_group); row_group = n_d + i
 *   a dead slot: pred_row = tgt_row = -1, row_weight = 0
 *   pred_row, tgt_row (K) int64; row_weight (K) f32 (formed in float64, rounded once); row_group (K) int32: the get_loss call of the slot,
 *   for a class_mask (2 n_d, C); num_boxes NULL: max(1, live pairs of the LAST decoder output), counted in the kernel
 *   status int32[4], the words of msda_criterion_pairs_f32: [0] the denoising layout does not fit, [1] live targets without a query over the
 *   n_d selected layers, [2] = 0, [3] bad cum: every slot dead
 * Integer results and single roundings: exact and reproducible.  No atomic, no workspace, no host synchronisation: capturable.
 *
 * msda_distill_scatter_f32 / _bf16 (the backward; after msda_distill_pairs and a row kernel on the same slots): grad_pred (n_d, N, pad_cap + Q,
 * C) f32 / bf16 <- gscale[0] * grad_rows[k] at row pred_row[k] for every live slot, written WHOLE (zeros elsewhere) with plain stores; dead
 * slots' gradient rows are not read.  The product is formed in float32 and, for bf16, rounded to nearest even once.  The assignment is
 * one-to-one per image and output, as msda_lsap_* writes it; if query_of_target sends two live targets of an image to one query, which of
 * their rows lands is unspecified.
 * Limits of both: nl <= 63, N <= 1024, capacity < 2^24, rows and slots below 2^31 (MSDA_ERR_TOO_LARGE); nl, N, Q, C, capacity >= 1,
 * pad_cap >= 0, layer_mask within (0, 2^nl) (MSDA_ERR_BAD_DIMS); objective not 0 / 1 (MSDA_ERR_BAD_OPTION); int64 arguments 8-byte aligned. */
int msda_roi_align_targets_f32(const float *input, const int64_t *cum, const float *tgt_boxes, const int32_t *sizes, int N, int C, int H, int W,
                               int64_t capacity, int pooled_h, int pooled_w, double spatial_scale, int sampling_ratio, float *output,
                               int32_t *status, msda_stream_t stream);
int msda_distill_pairs(const int64_t *cum, const int64_t *query_of_target, const int64_t *dn_meta, const float *num_boxes, int nl, int N, int Q,
                       int pad_cap, int64_t capacity, int64_t layer_mask, int objective, int64_t *pred_row, int64_t *tgt_row, float *row_weight,
                       int32_t *row_group, int32_t *status, msda_stream_t stream);
int msda_distill_scatter_f32(const float *grad_rows, const int64_t *pred_row, const int64_t *cum, const float *gscale, int n_d, int N, int Q,
                             int pad_cap, int64_t capacity, int C, float *grad_pred, msda_stream_t stream);
int msda_distill_scatter_bf16(const float *grad_rows, const int64_t *pred_row, const int64_t *cum, const float *gscale, int n_d, int N, int Q,
                              int pad_cap, int64_t capacity, int C, uint16_t *grad_pred, msda_stream_t stream);

/* ---- integer part of the contrastive-denoising set-up (reference
 * models/richsem/dn_components.py:42-71, 131-179): bit-exact int64 / bool results ---------------------------------
 * msda_dn_indices_i64: cum = exclusive prefix of the per-image box counts (batch + 1 int64 on the device), total = cum[batch],
 *   groups2 = 2 * dn_number.  Writes total * groups2 entries: known_bid[i] = image of box i % total,
 *   map_known_indice[i] = index of that box inside its image + single_pad * (i / total).
 * msda_dn_attn_mask_u8: (tgt_size x tgt_size) bytes, 1 = masked: columns < pad_size are hidden from rows >= pad_size, and
 *   from rows of another denoising group (group = index / group_pad). */
int msda_dn_indices_i64(const int64_t *cum, int batch, int64_t total, int groups2, int64_t single_pad, int64_t *known_bid,
                        int64_t *map_known_indice, msda_stream_t stream);
int msda_dn_attn_mask_u8(uint8_t *mask, int64_t tgt_size, int64_t pad_size, int64_t group_pad, msda_stream_t stream);

/* ---- the denoising queries from the target counts ON THE DEVICE (reference models/richsem/dn_components.py:11-193 with
 * check_pos_dn=False): the reference's input_query_label, input_query_bbox, attn_mask and dn_meta in ONE launch, into buffers of a fixed
 * capacity pad_cap, and the label table's gradient in one more.  (Additions within ABI v13: nothing existing changes.)
 *   cum (N + 1) int64     exclusive prefix of the per-image target counts (what msda_dn_indices_i64 takes; here read on the device)
 *   labels int64, boxes (., 4) f32 cxcywh: target_cap rows each (the caller's capacity; the first cum[N] are read)
 *   uniform (N, pad_cap, 10) f32 in [0, 1): per slot p, u_label, u_sign[4], u_part[4] -- the caller draws it, so a replay draws anew
 *   table (V, D) f32      what label_enc looks up (nn.Embedding, LabelEnc(weight), CLIPAlign.get_label_enc: a row lookup all three)
 * Layout: single_pad = the largest count; groups from dn_number, single_pad and add_gt as :27-41; pad_size = single_pad * 2 * groups,
 * halved when use_cdn = 0.  Slot s of image b: gi = s / single_pad, j = s % single_pad, group-half g2 = gi (use_cdn) or 2 gi (the positive
 * halves only); filled iff s < pad_size and j < count_b; its target is cum[b] + j.
 *   label: p < label_noise_ratio * 0.5 takes min(floor(u_label * num_classes), num_classes - 1), otherwise the target's label;
 *   box:   rand_part = (u_part + (g2 odd ? 1 : 0)) * (u_sign < 0.5 ? -1 : 1); xyxy + rand_part * (w/2, h/2, w/2, h/2) * box_noise_scale,
 *          clamped to [0, 1], back to cxcywh -- float32 operation by operation without contraction: equal to torch's bit for bit;
 *          box_noise_scale = 0 keeps the target's box (:73);
 *   add_gt: group-half 0 keeps label and box (:60-61, :86-87).
 *   q_label (N, pad_cap, D) f32       table[label] in a filled slot, zeros elsewhere (and for a label outside [0, V))
 *   q_bbox (N, pad_cap, 4) f32        inverse_sigmoid (eps 1e-3, util/misc.py:605-609) of the noised box; zeros in an empty slot
 *   noised_label (N, pad_cap) int64   -1 in an empty slot
 *   noised_box (N, pad_cap, 4) f32    the noised box before inverse_sigmoid; zeros in an empty slot                          (or NULL)
 *   attn_mask (T, T) u8, T = pad_cap + num_queries, 1 = masked: on rows / columns [0, pad_size) and [pad_cap, T) the reference's mask
 *          (:157-179); the tail columns [pad_size, pad_cap) are masked for every row; a tail row sees the matching queries only
 *   meta int64[5]                     single_pad, num_dn_group, pad_size, total = cum[N], overflow
 * Overflow (a graph cannot raise): if pad_size > pad_cap or cum[N] > target_cap, overflow = 1, pad_size = 0 and every slot is empty.
 * Every element of every output is written: no memset, no atomic, no host synchronisation, no allocation -- capturable; a replay follows
 * the current contents of cum, labels, boxes and uniform.  Alignment: boxes, table, q_label, q_bbox, noised_box, attn_mask 16 bytes, the
 * int64 arguments 8, uniform 4 (MSDA_ERR_MISALIGNED).  N < 1, pad_cap < 0, D < 4 or not a multiple of 4, V < 1, num_classes < 1, a negative
 * num_queries / dn_number / target_cap / ratio / scale, use_cdn or add_gt outside {0, 1} (MSDA_ERR_BAD_DIMS); a null pointer to a buffer
 * that has elements (MSDA_ERR_NULL_POINTER): refused before any launch.
 * msda_dn_queries_backward_f32: grad_table (V, D) <- per class v the sum over rows r = 0 .. rows - 1, in that order, of grad_q_label[r]
 *   where noised_label[r] == v; every row is written (zeros where no slot hits); no atomic, bitwise reproducible.  Labels, boxes and the
 *   uniforms get no gradient, as in the reference. */
int msda_dn_queries_f32(const int64_t *cum, const int64_t *labels, const float *boxes, int64_t target_cap, const float *uniform,
                        const float *table, int N, int pad_cap, int D, int V, int num_classes, int num_queries, int dn_number,
                        float label_noise_ratio, float box_noise_scale, int use_cdn, int add_gt, float *q_label, float *q_bbox,
                        int64_t *noised_label, float *noised_box, uint8_t *attn_mask, int64_t *meta, msda_stream_t stream);
int msda_dn_queries_backward_f32(const float *grad_q_label, const int64_t *noised_label, int64_t rows, int D, int V, float *grad_table,
                                 msda_stream_t stream);

/* Top-k query selection (reference models/richsem/deformable_transformer.py:370-372: torch.topk(scores, k, dim=1)[1]): for every
 * row of `scores` (rows x n, float32) the indices -- and, if `values` is non-NULL, the scores -- of its k largest elements in
 * descending order; equal scores lowest index first.  n <= 36864, k <= 1024 (one workgroup holds a row in LDS). */
int msda_topk_f32(const float *scores, int rows, int n, int k, int64_t *indices, float *values, msda_stream_t stream);

/* The decoder's positional query embedding, gen_sineembed_for_position (models/richsem/utils.py:142-168) in one launch (the reference:
 * ~15 element-wise ops per decoder layer): boxes (tokens, >= dims) f32 (x, y[, w, h]) with a row stride of ld floats; out (tokens,
 * dims * pe_dim) bf16 in the reference's order (y, x[, w, h]), channel 2k = sin, 2k + 1 = cos of coordinate * 2 pi /
 * temperature^(2k / pe_dim).  dims = 2 | 4, pe_dim even.  No gradient (the boxes it is applied to are detached, :779-804). */
/* Backward of a 256 -> n linear layer with n <= 8 (the last layer of the box heads, MLP(256, 256, 4, 3): models/richsem/utils.py:110-122,
 * deformable_transformer.py:779-804): dy (T, n) bf16 contiguous, x (T, 256) bf16, w (n, 256) f32 -> dx (T, 256) bf16 (or NULL), dw (n, 256)
 * f32, db (n) f32 (or NULL): two streaming kernels instead of three GEMMs with a 4-wide operand. */
int msda_narrow_linear_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *w, int T, int n, uint16_t *dx, float *dw, float *db,
                                     msda_stream_t stream);

/* The decoder's box update, y = sigmoid(delta + inverse_sigmoid(ref)) (models/richsem/deformable_transformer.py:779-804,
 * richsem.py:705-715; inverse_sigmoid of util/misc.py:605-609 with its eps) as one launch, and its gradient w.r.t. delta
 * (grad_y * y * (1 - y)) as one more: delta / grad_delta (n) bf16 or f32, ref, y, grad_y (n) f32.  ref is taken as a constant (the
 * reference detaches it between layers). */
int msda_box_refine_forward(const void *delta, int delta_is_bf16, const float *ref, float eps, int64_t n, float *y, msda_stream_t stream);
int msda_box_refine_backward(const float *grad_y, const float *y, int64_t n, void *grad_delta, int delta_is_bf16, msda_stream_t stream);
/* ... with the gradient w.r.t. ref as well (ref, grad_ref (n) f32; the heads' boxes of decoder layers 1..5, whose reference is not detached:
 * models/richsem/richsem.py:705-715): grad_ref = grad_delta * d inverse_sigmoid(ref) / d ref, the clamps' gradients as torch takes them */
int msda_box_refine_backward_ref(const float *grad_y, const float *y, int64_t n, void *grad_delta, int delta_is_bf16, const float *ref, float eps,
                                 float *grad_ref, msda_stream_t stream);

int msda_sine_embed_bf16(const float *boxes, int ld, int tokens, int dims, int pe_dim, float temperature, uint16_t *out, msda_stream_t stream);

/* ROIAlign forward (reference models/richsem/richsem.py:750, :878:
 * detectron2.layers.ROIAlign(output_size, spatial_scale, sampling_ratio = 0, aligned = True) on the frozen CLIP feature map).
 * input (N, C, H, W) contiguous; rois (K, 5) = (batch index, x1, y1, x2, y2) in input pixels; output (K, C, pooled_h, pooled_w).
 * detectron2's published algorithm (= torchvision.ops.roi_align); no gradient (the teacher is frozen).
 * Refusals: a ROI whose batch index is outside [0, N), whose coordinates are not finite, or whose adaptive sampling grid
 * (sampling_ratio = 0: ceil(roi / bins)) would exceed 4096 per axis is written as exact zeros, the other ROIs unaffected;
 * sampling_ratio > 4096 is MSDA_ERR_BAD_DIMS.  A ROI inside these limits is computed as the published algorithm does. */
int msda_roi_align_forward_f32(const float *input, const float *rois, int K, int N, int C, int H, int W, int pooled_h,
                               int pooled_w, double spatial_scale, int sampling_ratio, int aligned, float *output,
                               msda_stream_t stream);
int msda_roi_align_forward_f64(const double *input, const double *rois, int K, int N, int C, int H, int W, int pooled_h,
                               int pooled_w, double spatial_scale, int sampling_ratio, int aligned, double *output,
                               msda_stream_t stream);

/* ---- convolution forward on the matrix cores with the frozen-BatchNorm affine, residual add and ReLU in its epilogue (SURVEY.md
 * section 8a rows a10 / a11; reference clip/model.py:10-56, :94-167 -- the frozen CLIP teacher called at models/richsem/richsem.py:628 --
 * and models/richsem/backbone.py:20-56 around the ResNet-50 convolutions; csrc/conv_mfma.hip) -------------------------------------
 *     out[n, ho, wo, co] = act( scale[co] * sum_{kh, kw, ci} x[n, ho s + kh - p, wo s + kw - p, ci] w[co, ci, kh, kw] + shift[co]
 *                               (+ residual[n, ho, wo, co]) ),   act = relu or identity
 * Activations NHWC bf16, fp32 accumulation, fp32 scale / shift (BatchNorm folded: scale = w rsqrt(var + eps), shift = b - mean scale;
 * a plain bias is scale = 1, shift = bias).  C_out % 16 == 0; C_in % 32 == 0, or any C_in with KH KW C_in <= 512 (the 3-channel stems:
 * operand fragments gathered element by element); all pointers 16-byte aligned (x: 2-byte for few-channel inputs); residual may be NULL.
 * msda_conv_pack_weight: weight (C_out, C_in, KH, KW) fp32 (torch layout) -> msda_conv_packed_elems uint16 in MFMA fragment order
 * (repack when the weight changes).  msda_conv_set_tiling forces the per-wave tile (channel tiles in {1, 2, 4, 8, 16}, pixel tiles in
 * {1, 2, 3}; 0 = chosen per call so that the grid fills the chip) -- results do not depend on it beyond summation order. */
int msda_conv_set_tiling(int co_tiles, int pixel_tiles);
/* ... and msda_conv_set_ring the operand prefetch of the C_in % 64 == 0 kernels: both operands through LDS rings of `slots` iterations
 * (LDS DMA; csrc/conv_mfma.hip, conv_ring_kernel): -1 never, 0 chosen per call, 3 / 4 / 6 wherever that kernel applies.  Same results. */
int msda_conv_set_ring(int slots);
int msda_conv_packed_elems(int Cout, int Cin, int KH, int KW, int64_t *elems);
int msda_conv_pack_weight(const float *weight, int Cout, int Cin, int KH, int KW, uint16_t *packed, msda_stream_t stream);
int msda_conv_forward_bf16(const uint16_t *x, const uint16_t *packed_weight, const float *scale, const float *shift,
                           const uint16_t *residual, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                           uint16_t *out, msda_stream_t stream);

/* The same with a k split for problems that leave most of the chip idle (few output pixels, long k: ResNet-50's layer4 3 x 3 at batch 2,
 * the stride-2 projection of C5): msda_conv_forward_workspace_bytes reports how many bytes of ZEROED device memory (an fp32 image of the
 * output) the split needs -- 0 where the problem is not split --, msda_conv_forward_ws_bf16 takes them (or NULL: no split): the k
 * slices add their raw sums there and a second kernel applies the epilogue.  Results differ from the unsplit call by fp32 summation
 * order only. */
int msda_conv_forward_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int64_t *bytes);
int msda_conv_forward_ws_bf16(const uint16_t *x, const uint16_t *packed_weight, const float *scale, const float *shift,
                              const uint16_t *residual, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int relu,
                              uint16_t *out, void *workspace, msda_stream_t stream);

/* GroupNorm with 8 channels per group on NHWC bf16 (nn.GroupNorm(32, 256) of the input projections, models/richsem/richsem.py:301,
 * :307): x (N, HW, C) bf16 with C = 8 * groups; gamma, beta (C) f32; stats: N * (C / 8) * 2 doubles of device scratch; out_f32 and / or
 * out_bf16 (N, HW, C), either may be NULL.  Sums of x and x^2 in fp32 per thread, combined in fp64.  Forward only. */
int msda_groupnorm8_nhwc_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int N, int HW, int C, double *stats,
                              float *out_f32, uint16_t *out_bf16, msda_stream_t stream);
/* Its backward (the trainable input projections): x, dy (N, HW, C) bf16; stats as the forward left them; bstats: N * (C / 8) * 16 doubles
 * of device scratch; dx (N, HW, C) bf16; dgamma, dbeta (C) f32, either may be NULL.  Replaces autograd's GroupNorm backward on the
 * channels-first fp32 view (three permuting copies and five kernels per level). */
int msda_groupnorm8_backward_nhwc_bf16(const uint16_t *x, const uint16_t *dy, const float *gamma, float eps, int N, int HW, int C,
                                       const double *stats, double *bstats, uint16_t *dx, float *dgamma, float *dbeta, msda_stream_t stream);

/* Pooling on NHWC bf16 activations (nn.AvgPool2d(k) of the CLIP ResNet, clip/model.py:24, :36, :115; MaxPool2d(3, 2, 1) after
 * torchvision's ResNet stem): is_max = 0: mean over k x k windows at `stride`, pad must be 0; is_max = 1: maximum with implicit -inf
 * padding.  out (N, Ho, Wo, C) with Ho = (H + 2 pad - k) / stride + 1.  C % 8 == 0, 16-byte aligned pointers.  Forward only. */
int msda_pool_nhwc_bf16(const uint16_t *x, int N, int H, int W, int C, int k, int stride, int pad, int is_max, uint16_t *out,
                        msda_stream_t stream);

/* Gradient of msda_conv_forward_bf16 w.r.t. its input (for the backbone's trained stages), by the same kernel: a stride-1
 * convolution of the output gradient -- read as if zero-upsampled by `stride` -- with the flipped, transposed weight.
 * dy (N, Ho, Wo, Cout) bf16 (already multiplied by the ReLU mask); packed_weight_t = msda_conv_pack_weight(w_t, Cin, Cout, KH, KW) with
 * w_t[ci][co][kh][kw] = scale[co] * w[co][ci][KH-1-kh][KW-1-kw]; dx (N, H, W, Cin) bf16, every element written.  Square kernels,
 * Cout % 32 == 0, Cin % 16 == 0, pad <= KH - 1. */
int msda_conv_dgrad_bf16(const uint16_t *dy, const uint16_t *packed_weight_t, int N, int Ho, int Wo, int Cout, int Cin, int KH, int KW,
                         int stride, int pad, int H, int W, uint16_t *dx, msda_stream_t stream);

/* ... and its k-split form (see msda_conv_forward_ws_bf16; k = KH KW C_out here, the image is dx's) */
int msda_conv_dgrad_workspace_bytes(int N, int Ho, int Wo, int Cout, int Cin, int KH, int KW, int stride, int pad, int H, int W, int64_t *bytes);
int msda_conv_dgrad_ws_bf16(const uint16_t *dy, const uint16_t *packed_weight_t, int N, int Ho, int Wo, int Cout, int Cin, int KH, int KW,
                            int stride, int pad, int H, int W, uint16_t *dx, void *workspace, msda_stream_t stream);
/* ... with the element-wise work that follows an input gradient in a residual network in its epilogue: dx = mask(conv_dgrad(dy) + add).
 * add (N, H, W, Cin) bf16 or NULL: a second gradient of the same tensor (the identity branch of a bottleneck); relu_out (N, H, W, Cin)
 * bf16 or NULL: the tensor whose gradient this is, when it is the output of a ReLU -- dx is the gradient at that ReLU's INPUT: an element
 * is kept iff relu_out > 0 and is +0 otherwise.  The comparison is made on the bits: kept iff the bf16, read as a signed 16-bit integer,
 * is > 0.  For every non-NaN value (+-0, subnormals, +-inf included) that is relu_out > 0 and what aten::threshold_backward(dx, relu_out, 0)
 * gives; a NaN keeps the element when its sign bit is clear and zeroes it when set, where aten::threshold_backward keeps both
 * (msda_conv_forward_bf16's ReLU is fmaxf(y, 0), which never returns NaN, so a ReLU output of this library holds none). */
int msda_conv_dgrad_fused_bf16(const uint16_t *dy, const uint16_t *packed_weight_t, int N, int Ho, int Wo, int Cout, int Cin, int KH, int KW,
                               int stride, int pad, int H, int W, const uint16_t *add, const uint16_t *relu_out, uint16_t *dx,
                               void *workspace, msda_stream_t stream);

/* Gradient of msda_conv_forward_bf16 w.r.t. its weight (csrc/conv_wgrad.hip): dw[co][kh][kw][ci] = sum over output pixels of
 * dz[n, ho, wo, co] * x[n, ho stride + kh - pad, wo stride + kw - pad, ci].  dz (N, Ho, Wo, Cout) bf16 = gradient at the CONVOLUTION's
 * output (ReLU mask applied); x (N, H, W, Cin) bf16; dw (Cout, KH, KW, Cin) fp32, every element written.  The pixels are split into
 * chunks where the (tap, channel block) grid alone cannot fill the chip; the chunks' partial sums go through `workspace`
 * (msda_conv_wgrad_workspace_bytes; may be NULL when that is 0) and a second kernel.  dbias (Cout) fp32, optional (NULL: not wanted):
 * sum over the output pixels of dz, formed on the way.  scale (Cout) fp32, optional: dw[co] is multiplied by scale[co] (the frozen affine
 * that follows the convolution commutes with the pixel sum).  torch_layout != 0: dw is written as (Cout, Cin, KH, KW), nn.Conv2d's layout.
 * Cout % 128 == 0, Cin % 128 == 0. */
int msda_conv_wgrad_workspace_bytes(int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int64_t *bytes);
/* Tuning / tests: 1 (default) = operand stages prefetched three ahead through an LDS ring (LDS DMA), 0 = register-staged; same results */
int msda_conv_set_wgrad_ring(int on);
int msda_conv_wgrad_bf16(const uint16_t *dz, const uint16_t *x, int N, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                         int pad, float *dw, float *dbias, const float *scale, int torch_layout, void *workspace, msda_stream_t stream);

/* Several weight gradients in ONE launch of the product kernel and one of the reduction (a bottleneck block's three or four,
 * models/richsem/backbone.py:59-92 trains layer2-4): each problem is msda_conv_wgrad_bf16's, its result in nn.Conv2d's layout
 * (Cout, Cin, KH, KW), multiplied by scale[co] when scale is not NULL; dbias as msda_conv_wgrad_bf16's (optional).  The problems share the chip in proportion to
 * their work instead of each being cut into ~512 short workgroups.  n <= 8. */
typedef struct {
    const uint16_t *dz, *x;
    float *dw;
    const float *scale;
    float *dbias;      /* (Cout) fp32: sum over the pixels of dz, or NULL */
    int N, H, W, Cin, Cout, KH, KW, stride, pad;
} msda_wgrad_problem;
int msda_conv_wgrad_group_workspace_bytes(const msda_wgrad_problem *problems, int n, int64_t *bytes);
int msda_conv_wgrad_group_bf16(const msda_wgrad_problem *problems, int n, void *workspace, msda_stream_t stream);

/* ---- two-stage query selection: row maxima of the class logits without the logits (reference
 * models/richsem/deformable_transformer.py:368-372 with the CLIP-text classifier models/richsem/richsem.py:176-184 in its shipped
 * configuration: bias-free linear projection Wp (proj x 256), text embeddings t_c) ------------------------------------------------
 *     score[token] = max_c  exp(logit_scale) * (Wp x / |Wp x|) . (t_c / |t_c|)  =  scale * max_c (G x)_c / sqrt(x . (A x))
 * with G = T^ Wp (classes x 256) and A = Wp^T Wp (256 x 256), both formed by the caller in fp32 whenever the weights change
 * (csrc/cls_mfma.hip).  msda_cls_pack lays [G; A] out in MFMA fragment order as bf16 hi + lo parts (msda_cls_packed_elems uint16
 * elements); msda_cls_max_scores computes the scores of `tokens` rows of x (fp32, or bf16 when x_is_bf16) with bf16 MFMAs on the
 * split operands: parts = 2 keeps the weights' lo part (fp32-level accuracy with fp32 x), parts = 1 is a plain bf16 product.
 * d_model must be 256; classes <= 8192; x and packed 16-byte aligned.  Forward only (the selection carries no gradient). */
int msda_cls_packed_elems(int classes, int64_t *elems);
int msda_cls_pack(const float *G, int classes, const float *A, int d_model, uint16_t *packed, msda_stream_t stream);
int msda_cls_max_scores(const void *x, int x_is_bf16, const uint16_t *packed, int tokens, int d_model, int classes, float scale,
                        int parts, float *scores, msda_stream_t stream);

/* ---- class head: the CLIP-text logits themselves, forward and backward (reference models/richsem/richsem.py:182-205, CLIPAlign.forward /
 * forward_hs in the shipped configuration; csrc/cls_head_mfma.hip) -----------------------------------------------------------------
 *     n2 = x . (A x),   logits[row, c] = scale * (G x)_c / sqrt(n2)                        G, A as for msda_cls_pack
 *     dx = (scale / n) G^T g - (beta / n2) (A x),   beta = sum_c g_c logits_c,   n = sqrt(n2)
 *     dGA = [dG (classes x 256); dA (256 x 256)] = Y^T x,   Y = [ (scale / n) g | -(beta / (2 n2)) x ]   (the caller forms
 *     dWp = T^^T dG + Wp (dA + dA^T))
 * msda_cls_head_pack writes its own operand (msda_cls_head_packed_elems uint16 elements: A's tiles in front of G's, then G^T for the
 * backward); the layout of msda_cls_pack is a different one and is not accepted here.  x (tokens, 256) fp32, or bf16 when x_is_bf16;
 * logits, g (tokens, classes) fp32, dense; n2, beta (tokens) fp32; dx (tokens, 256) in x's type.  parts as for msda_cls_max_scores; in
 * the backward parts = 2 also splits g (hi + lo), parts = 1 rounds every operand to bf16 once.  msda_cls_head_backward_rows WRITES beta,
 * msda_cls_head_backward_weights READS it: rows first.  The weights call sums splits of 512 rows through `workspace`
 * (msda_cls_head_workspace_bytes) in a fixed order -- no atomics, the same bits on every run.  No call allocates or synchronises; all
 * can be captured into a graph.  d_model must be 256; 1 <= classes <= 8192; tokens >= 1; x, packed, dx, workspace and dGA 16-byte
 * aligned.  A row x = 0 yields NaN logits and NaN dx in that row only, and a NaN dGA (as the reference's f / |f| does). */
int msda_cls_head_packed_elems(int classes, int64_t *elems);
int msda_cls_head_pack(const float *G, int classes, const float *A, int d_model, uint16_t *packed, msda_stream_t stream);
int msda_cls_head_forward(const void *x, int x_is_bf16, const uint16_t *packed, int tokens, int d_model, int classes, float scale,
                          int parts, float *logits, float *n2, msda_stream_t stream);
int msda_cls_head_backward_rows(const float *g, const float *logits, const float *n2, const void *x, int x_is_bf16, const uint16_t *packed,
                                int tokens, int d_model, int classes, float scale, int parts, void *dx, float *beta, msda_stream_t stream);
int msda_cls_head_workspace_bytes(int tokens, int classes, int64_t *bytes);
int msda_cls_head_backward_weights(const float *g, const float *n2, const float *beta, const void *x, int x_is_bf16, int tokens, int d_model,
                                   int classes, float scale, int parts, void *workspace, float *dGA, msda_stream_t stream);

/* ---- Swin shifted-window attention, forward and backward (reference models/richsem/swin_transformer.py:108-139 inside :183-239, mask
 * of :353-369; csrc/swin_attn_mfma.hip) -- map layout in, map layout out: roll, window partition / reverse are index arithmetic ----------
 *     out = softmax(q k^T / sqrt(32) + bias + mask) v   per (image, window, head)
 * qkv (B, Hp, Wp, 3 channels) bf16 dense, last dimension ordered (3, heads, 32); table ((2 window - 1)^2, heads) fp32; out, dout
 * (B, Hp, Wp, channels) bf16; lse (B, Hp, Wp, heads) fp32, written by the forward and read by the backward; dqkv as qkv, dtable as table.
 * Window (wy, wx) holds rolled coordinates (wy window + i, wx window + j), token t = i window + j, living at ((py + shift) mod Hp,
 * (px + shift) mod Wp); bias of (t, t') = table[(i - i' + window - 1)(2 window - 1) + (j - j' + window - 1), head]; for shift > 0 pairs of
 * different regions (3 r(py, Hp) + r(px, Wp), r(c, n) = [c >= n - window] + [c >= n - shift]) get the reference's additive -100.
 * The backward writes every element of dqkv once (no pre-zeroed output) and sums dtable through `workspace`
 * (msda_swin_attn_workspace_bytes, contents irrelevant on entry) in a fixed order: no atomics, the same bits on every call.  No call
 * allocates or synchronises.  Limits: channels == 32 heads, window^2 <= 144, 0 <= shift < window, Hp and Wp multiples of window, B >= 1
 * (MSDA_ERR_BAD_DIMS); B Hp Wp < 2^31, heads <= 65535 (MSDA_ERR_TOO_LARGE); qkv, out, dout, dqkv 16-byte aligned, the fp32 buffers 4
 * (MSDA_ERR_MISALIGNED). */
int msda_swin_attn_workspace_bytes(int B, int Hp, int Wp, int channels, int heads, int window, int64_t *bytes);
int msda_swin_attn_forward_bf16(const uint16_t *qkv, const float *table, int B, int Hp, int Wp, int channels, int heads, int window,
                                int shift, uint16_t *out, float *lse, msda_stream_t stream);
int msda_swin_attn_backward_bf16(const uint16_t *qkv, const float *table, const uint16_t *out, const float *lse, const uint16_t *dout, int B,
                                 int Hp, int Wp, int channels, int heads, int window, int shift, uint16_t *dqkv, float *dtable,
                                 void *workspace, msda_stream_t stream);

/* ---- the rest of a Swin block: linear layers of general width with fused epilogues, LayerNorm of general width (reference
 * models/richsem/swin_transformer.py:27-44 Mlp, :108-139 qkv / proj, :183-239 norm1, norm2 and the residual adds;
 * csrc/swin_block_mfma.hip) -- bf16 storage, fp32 accumulation and element-wise arithmetic, one rounding per stored element ----------
 * msda_swin_linear_bf16:  acc = x (tokens, K) . w (N, K)^T, both bf16 row-major (no packed form: the input gradient is the same call on
 * the transposed weight); bias (N) fp32 or NULL; out (tokens, N) bf16.  `epilogue`:
 *   0  out = rnd(acc + bias)
 *   1  u = rnd(acc + bias) -> out2 (tokens, N) unless NULL;  out = rnd(gelu(u)) of the ROUNDED u, gelu(x) = x Phi(x) (the erf form)
 *   2  out = rnd(acc + bias + aux), aux (tokens, N) bf16
 *   3  out = rnd(acc gelu'(aux)), gelu'(x) = Phi(x) + x phi(x), aux = the u of epilogue 1;  out2 = rnd(gelu(aux)) unless NULL (bias unused)
 * msda_swin_layernorm_forward_bf16:  out = rnd((x - mean) rstd gamma + beta) per token over C channels, biased variance in fp32;
 * x, out (tokens, C) bf16, gamma, beta (C) fp32, mean, rstd (tokens) fp32 written unless NULL.
 * msda_swin_layernorm_backward_bf16:  with xhat = (x - mean) rstd recomputed and g = dy gamma,
 *   dx = rnd(add + rstd (g - mean_c(g) - xhat mean_c(g xhat))),  dgamma = sum_t dy xhat,  dbeta = sum_t dy
 * add (tokens, C) bf16 or NULL (the residual stream's gradient, fused so that the sum is rounded once); dgamma, dbeta (C) fp32, each may be
 * NULL; they are summed through `workspace` (msda_swin_layernorm_workspace_bytes, contents irrelevant on entry; may be NULL when both are)
 * in a fixed order.  No atomics, the same bits on every call; no call allocates or synchronises.
 * Limits: K, N multiples of 32 in [32, 8192], C a multiple of 32 in [32, 4096], tokens >= 1, epilogue in 0..3 (MSDA_ERR_BAD_DIMS);
 * tokens K, tokens N, tokens C < 2^31 (MSDA_ERR_TOO_LARGE); the bf16 buffers 16-byte aligned, the fp32 ones 4 (MSDA_ERR_MISALIGNED); aux
 * NULL for epilogue 2 or 3 is MSDA_ERR_NULL_POINTER.  Every check comes before any launch. */
int msda_swin_linear_bf16(const uint16_t *x, const uint16_t *w, const float *bias, const uint16_t *aux, int epilogue, int tokens, int K, int N,
                          uint16_t *out, uint16_t *out2, msda_stream_t stream);
int msda_swin_layernorm_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int tokens, int C, uint16_t *out,
                                     float *mean, float *rstd, msda_stream_t stream);
int msda_swin_layernorm_workspace_bytes(int tokens, int C, int64_t *bytes);
int msda_swin_layernorm_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma,
                                      const uint16_t *add, int tokens, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace,
                                      msda_stream_t stream);

/* ---- where the Swin backbone changes layout: the merging norm, the output norms to NCHW, the patch rows (reference
 * models/richsem/swin_transformer.py:242-277 PatchMerging, :399-434 PatchEmbed, :640-660 the output norms; csrc/swin_stage.hip) -- bf16
 * storage, fp32 statistics and arithmetic, one rounding per stored element; the formulas of msda_swin_layernorm_* operation for operation
 * (mean by a division, biased variance as the mean of squared deviations, dgamma / dbeta through the workspace of
 * msda_swin_layernorm_workspace_bytes in a fixed order): only where a row's elements live changes -------------------------------------
 * msda_swin_merge_norm_forward_bf16:  x (B, H, W, C) bf16, the map.  Rows (B H2 W2, 4 C), H2 = (H + 1) / 2, W2 = (W + 1) / 2: channel
 *   q C + c of row (b, i, j) is pixel (2 i + (q & 1), 2 j + (q >> 1)); a pixel outside the map reads as zero and takes part in the
 *   statistics as a zero.  out (B H2 W2, 4 C) = rnd((row - mean) rstd gamma + beta), gamma, beta (4 C) fp32; mean, rstd (B H2 W2) fp32
 *   written unless NULL.
 * msda_swin_merge_norm_backward_bf16:  dy (B H2 W2, 4 C), x the map, mean, rstd, gamma as above.  With xhat and g = dy gamma over the
 *   gathered row,  dx = rnd(rstd (g - mean_c(g) - xhat mean_c(g xhat)))  stored at the pixel the element came from: dx (B, H, W, C), every
 *   element written exactly once (nothing pre-zeroed); elements of quadrants outside the map are dropped.  dgamma = sum_rows dy xhat and
 *   dbeta = sum_rows dy, (4 C) fp32, each may be NULL; a padded element's xhat = (0 - mean) rstd counts in dgamma.  workspace:
 *   msda_swin_layernorm_workspace_bytes(B H2 W2, 4 C), may be NULL when both are.
 *   Limits: C a multiple of 32, 4 C <= 4096, B, H, W >= 1 (MSDA_ERR_BAD_DIMS); B H W C and B H2 W2 4 C < 2^31 (MSDA_ERR_TOO_LARGE).
 * msda_swin_norm_nchw_forward_bf16:  x (B, HW, C) tokens -> out (B, C, HW) = the LayerNorm of every token, stored transposed; mean, rstd
 *   (B HW) written unless NULL.  HW is arbitrary: a channel row of out may start on any 2-byte boundary (ragged ends are stored
 *   element by element, the 16-byte chunks of the buffer between them whole).
 * msda_swin_norm_nchw_backward_bf16:  dy (B, C, HW), x tokens -> dx (B, HW, C) tokens by the row formula above, dgamma, dbeta (C) (64-token
 *   parts of the B HW tokens, images back to back; workspace: msda_swin_layernorm_workspace_bytes(B HW, C)).
 *   Limits: C a multiple of 32 in [32, 4096], B, HW >= 1 (MSDA_ERR_BAD_DIMS); B HW C < 2^31 (MSDA_ERR_TOO_LARGE).
 * msda_swin_patch_rows_bf16:  img (B, Cin, H, W) bf16 -> rows (B Wh Ww, Kp), Wh = ceil(H / ph), Ww = ceil(W / pw), Kp = Cin ph pw rounded
 *   up to a multiple of 32; column (c ph + dy) pw + dx of row (b, i, j) = img[b, c, i ph + dy, j pw + dx] (the order of a convolution
 *   weight's flatten(1)); columns past Cin ph pw and pixels past the image are exact zeros.  Pure data movement: no rounding.
 * msda_swin_patch_rows_backward_bf16:  the inverse, drows (B Wh Ww, Kp) -> dimg (B, Cin, H, W), every element written once; the padding
 *   is dropped.   Limits: all extents >= 1, Kp <= 8192 (MSDA_ERR_BAD_DIMS); B Cin H W and B Wh Ww Kp < 2^31 (MSDA_ERR_TOO_LARGE).
 * Alignment (MSDA_ERR_MISALIGNED): the bf16 buffers 16 bytes (img and dimg: 2), the fp32 ones 4.  Every check comes before any launch; no
 * call allocates, synchronises or uses atomics; two calls give the same bits. */
int msda_swin_merge_norm_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int B, int H, int W, int C,
                                      uint16_t *out, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_merge_norm_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma, int B,
                                       int H, int W, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace, msda_stream_t stream);
int msda_swin_norm_nchw_forward_bf16(const uint16_t *x, const float *gamma, const float *beta, float eps, int B, int HW, int C, uint16_t *out,
                                     float *mean, float *rstd, msda_stream_t stream);
int msda_swin_norm_nchw_backward_bf16(const uint16_t *dy, const uint16_t *x, const float *mean, const float *rstd, const float *gamma, int B,
                                      int HW, int C, uint16_t *dx, float *dgamma, float *dbeta, void *workspace, msda_stream_t stream);
int msda_swin_patch_rows_bf16(const uint16_t *img, int B, int Cin, int H, int W, int ph, int pw, uint16_t *rows, msda_stream_t stream);
int msda_swin_patch_rows_backward_bf16(const uint16_t *drows, int B, int Cin, int H, int W, int ph, int pw, uint16_t *dimg, msda_stream_t stream);

/* ---- what a ConvNeXt block adds to the Swin kernels: depthwise 7 x 7 convolution and layer scale (reference
 * models/richsem/convnext.py:18-53 Block; csrc/convnext_dw.hip) -- the map is channels-last (B, H, W, C) bf16 ("map layout"), fp32
 * arithmetic and accumulation, one rounding per stored element --------------------------------------------------------------------------
 * msda_dwconv7_bf16:  out[b,y,x,c] = rnd(add[b,y,x,c] + bias[c] + sum_{ky,kx} w[t(ky,kx), c] x[b, y+ky-3, x+kx-3, c]),  ky, kx in 0..6;
 *   a pixel outside the image reads as zero, per image (a halo never reads the neighbouring image of the batch).  x, out, add (B, H, W, C)
 *   bf16, add may be NULL; w (49, C) fp32, tap-major; bias (C) fp32 or NULL.  t = 7 ky + kx for flip = 0, t = 7 (6 - ky) + (6 - kx) for
 *   flip = 1: with flip = 1, bias = NULL and add = the residual stream's gradient the call is the input gradient
 *   dinput = rnd(dout + dwconv^T(dy)), rounded once.
 * msda_dwconv7_wgrad_bf16:  dw[7 ky + kx, c] = sum_{b,y,x} dy[b,y,x,c] x[b, y+ky-3, x+kx-3, c], (49, C) fp32;  dbias[c] = sum_{b,y,x} dy,
 *   (C) fp32 or NULL.  Summed as per-workgroup partial rows in `workspace` (msda_dwconv7_workspace_bytes, contents irrelevant on entry),
 *   then one pass adds the parts in ascending order; the number of parts depends on the shape only.
 * msda_layer_scale_forward_bf16:  out = rnd(res + gamma[c] z);  z, res, out (tokens, C) bf16, gamma (C) fp32.
 * msda_layer_scale_backward_bf16:  dz = rnd(gamma[c] dout), (tokens, C) bf16;  dgamma[c] = sum_t dout z, (C) fp32 or NULL (then z and
 *   workspace may be NULL too), summed as parts of 64 k tokens (k = 1 up to 16384 tokens, then the smallest that keeps the parts at 256 or
 *   fewer) through `workspace` (msda_swin_layernorm_workspace_bytes(tokens, C), contents irrelevant on entry) in a fixed order.
 * Limits: C a multiple of 32 in [32, 4096], B, H, W, tokens >= 1, flip 0 or 1 (MSDA_ERR_BAD_DIMS); B H W C and tokens C < 2^31
 * (MSDA_ERR_TOO_LARGE); the bf16 buffers 16-byte aligned, the fp32 ones 4 (MSDA_ERR_MISALIGNED).  Every check comes before any launch; no
 * call allocates, synchronises or uses atomics; two calls give the same bits. */
int msda_dwconv7_bf16(const uint16_t *x, const float *w, const float *bias, const uint16_t *add, int flip, int B, int H, int W, int C,
                      uint16_t *out, msda_stream_t stream);
int msda_dwconv7_workspace_bytes(int B, int H, int W, int C, int64_t *bytes);
int msda_dwconv7_wgrad_bf16(const uint16_t *dy, const uint16_t *x, int B, int H, int W, int C, float *dw, float *dbias, void *workspace,
                            msda_stream_t stream);
int msda_layer_scale_forward_bf16(const uint16_t *z, const float *gamma, const uint16_t *res, int tokens, int C, uint16_t *out,
                                  msda_stream_t stream);
int msda_layer_scale_backward_bf16(const uint16_t *dout, const uint16_t *z, const float *gamma, int tokens, int C, uint16_t *dz, float *dgamma,
                                   void *workspace, msda_stream_t stream);

/* ---- the context aggregation of a FocalNet block (reference models/richsem/focal.py:84-110 FocalModulation.forward;
 * csrc/focalnet_ctx.hip, whose header holds the formulas and the rounding points) -- channels-last bf16 maps, fp32 arithmetic ----------------
 * L = focal level in 1..4, K_l = window + 2 l, every K_l in {3, 5, 7, 9}; s = 1 / (L + 1) with normalize = 1, else 1.  n = B H W C.
 * ctx0 (B, H, W, C) bf16 with ld0 elements per pixel and gates (B, H, W, L + 1) bf16 with ldg elements per pixel are read in place (the
 * output rows of the block's `f`); w fp32, tap-major (K_l K_l, C), level after level (sum K_l^2 rows); dw likewise.
 * msda_fmod_context_forward_bf16:  u (L, B, H, W, C) bf16: u_l = rnd(dwconv_{K_l}(ctx_{l-1})), ctx_l = GELU(u_l) of the stored u_l (as the
 *   input of the next convolution: rounded to bf16), zero padding per image;  mg (2, B, C) fp32: m = mean over the image of ctx_{L-1} and
 *   g = GELU(m);  A (B, H, W, C) bf16 = rnd(s (sum_{l<L} gate_l ctx_l + gate_L g)).
 * msda_fmod_context_backward_bf16:  from dA (B, H, W, C) bf16 and the forward's u, mg:  du (L, B, H, W, C) bf16, the gradients of the
 *   pre-activations;  dctx0 (ldd0 elements per pixel) and dgates (L + 1 per pixel, lddg elements per pixel) bf16, written in place into
 *   wider rows;  dw fp32 or NULL (then no weight gradient is formed).  Reductions run over per-workgroup parts in `workspace`, added in
 *   ascending order.
 * msda_fmod_workspace_bytes: the size of `workspace` for either call (contents irrelevant on entry).
 * msda_fmod_modulate_forward_bf16:  out = rnd(q mod);  q (tokens, C) with ldq elements per token, mod and out dense.
 * msda_fmod_modulate_backward_bf16:  dq = rnd(dout mod) (lddq elements per token), dmod = rnd(dout q).
 * Limits: C a multiple of 32 in [32, 4096], B, H, W, tokens >= 1, L and window as above, normalize 0 or 1, ld0, ldd0, ldq, lddq multiples
 * of 8 and >= C, ldg, lddg >= L + 1 (MSDA_ERR_BAD_DIMS); n and tokens C < 2^31 (MSDA_ERR_TOO_LARGE); the bf16 maps 16-byte aligned, gates
 * 2, the fp32 buffers 4 (MSDA_ERR_MISALIGNED).  Every check comes before any launch; no call allocates, synchronises or uses atomics; two
 * calls give the same bits. */
int msda_fmod_workspace_bytes(int B, int H, int W, int C, int64_t *bytes);
int msda_fmod_context_forward_bf16(const uint16_t *ctx0, int64_t ld0, const uint16_t *gates, int64_t ldg, const float *w, int B, int H, int W,
                                   int C, int L, int window, int normalize, uint16_t *u, float *mg, uint16_t *A, void *workspace,
                                   msda_stream_t stream);
int msda_fmod_context_backward_bf16(const uint16_t *dA, const uint16_t *ctx0, int64_t ld0, const uint16_t *gates, int64_t ldg, const float *w,
                                    const uint16_t *u, const float *mg, int B, int H, int W, int C, int L, int window, int normalize,
                                    uint16_t *du, uint16_t *dctx0, int64_t ldd0, uint16_t *dgates, int64_t lddg, float *dw, void *workspace,
                                    msda_stream_t stream);
int msda_fmod_modulate_forward_bf16(const uint16_t *q, int64_t ldq, const uint16_t *mod, int64_t tokens, int C, uint16_t *out,
                                    msda_stream_t stream);
int msda_fmod_modulate_backward_bf16(const uint16_t *dout, const uint16_t *q, int64_t ldq, const uint16_t *mod, int64_t tokens, int C,
                                     uint16_t *dq, int64_t lddq, uint16_t *dmod, msda_stream_t stream);

/* ---- the criterion's mask terms and the mask post-processor (csrc/mask_terms.hip; reference SetCriterion.loss_masks,
 * models/richsem/richsem.py:1073-1100 with dice_loss / sigmoid_focal_loss of segmentation.py:168-211, and PostProcessSegm.forward,
 * segmentation.py:214-242) ---------------------------------------------------------------------------------------------------------------
 * pred (N, Q, h, w) fp32 / bf16, read as stored;  target uint8 (cap, Hp, Wp), one padded canvas per target SLOT (the reference's
 * nested_tensor_from_tensor_list(masks): pixels outside a target's own mask are 0 and count in every mean and sum);  offsets (N + 1) int64
 * and query_of_target (cap) int64 ON THE DEVICE: slot s < offsets[N] with 0 <= query_of_target[s] < Q is a pair of the image whose offsets
 * bracket s; every other slot carries nothing;  num_boxes (1) fp32 on the device.  The resize is torch's bilinear interpolate with
 * align_corners = False (scale in / out, source max(0, (dst + 0.5) scale - 0.5), i1 = min(i0 + 1, in - 1), fp32 weights); gamma = 2; a
 * negative alpha switches the class weight off.
 * msda_mask_loss_forward_*:  pair_sums (cap, 4) fp32 = per slot (sum focal, sum p t, sum p, sum t) over the canvas, zeros where there is no
 *   pair;  losses (2) fp32 = loss_mask = sum_pairs (focal / (Hp Wp)) / num_boxes and loss_dice = sum_pairs (1 - (2 sum p t + 1) /
 *   (sum p + sum t + 1)) / num_boxes.  Per-workgroup partial sums in `workspace`, added in fp64 in ascending order.
 * msda_mask_loss_backward_*:  g (2) fp32 on the device = d / d loss_mask, d / d loss_dice;  grad_pred (N, Q, h, w) in pred's type, every
 *   element written exactly once: zeros for a query without a pair and for a source pixel no canvas pixel reads.
 * msda_mask_loss_workspace_bytes: the size of `workspace` for either call (contents irrelevant on entry).
 * msda_mask_postprocess_*:  per image n of N, HOST arrays: item_indices[n] (rows[n] int64 on the device: the rows of pred[n] to take) or
 *   item_indices == NULL (rows 0 .. rows[n] - 1), sizes[4 n ..] = (img_h, img_w, oh, ow), out[n] uint8 (rows[n], 1, oh, ow) on the device:
 *   out = sigmoid(x4[min(floor(oy ch / oh), ch - 1), min(floor(ox cw / ow), cw - 1)]) > threshold with (ch, cw) = (min(img_h, 4 h),
 *   min(img_w, 4 w)) and x4 the bilinear x4 map of the logits -- never materialised; the sigmoid is evaluated in fp32.
 * Limits: N, Q, h, w, Hp, cap >= 1, Wp a multiple of 16, rows >= 0, sizes >= 1 (MSDA_ERR_BAD_DIMS); w <= 1024, N Q h w < 2^31, the LDS
 * rows of a workgroup <= 64 KiB (MSDA_ERR_TOO_LARGE); target, workspace and out 16-byte aligned, the int64 buffers 8, fp32 4
 * (MSDA_ERR_MISALIGNED).  Every check comes before any launch; no call allocates, synchronises or uses atomics; two calls give the same bits. */
int msda_mask_loss_workspace_bytes(int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, int64_t *bytes);
int msda_mask_loss_forward_f32(const float *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                               const float *num_boxes, int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, float *losses,
                               float *pair_sums, void *workspace, msda_stream_t stream);
int msda_mask_loss_forward_bf16(const uint16_t *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                const float *num_boxes, int N, int Q, int h, int w, int Hp, int Wp, int64_t cap, float alpha, float *losses,
                                float *pair_sums, void *workspace, msda_stream_t stream);
int msda_mask_loss_backward_f32(const float *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                const float *num_boxes, const float *pair_sums, const float *g, int N, int Q, int h, int w, int Hp, int Wp,
                                int64_t cap, float alpha, float *grad_pred, void *workspace, msda_stream_t stream);
int msda_mask_loss_backward_bf16(const uint16_t *pred, const uint8_t *target, const int64_t *offsets, const int64_t *query_of_target,
                                 const float *num_boxes, const float *pair_sums, const float *g, int N, int Q, int h, int w, int Hp, int Wp,
                                 int64_t cap, float alpha, uint16_t *grad_pred, void *workspace, msda_stream_t stream);
int msda_mask_postprocess_f32(const float *pred, int N, int Q, int h, int w, const int64_t *const *item_indices, const int *rows, const int *sizes,
                              float threshold, uint8_t *const *out, msda_stream_t stream);
int msda_mask_postprocess_bf16(const uint16_t *pred, int N, int Q, int h, int w, const int64_t *const *item_indices, const int *rows,
                               const int *sizes, float threshold, uint8_t *const *out, msda_stream_t stream);

/* ---- the CondInst dynamic mask head (csrc/dynamic_masks.hip; reference MaskBranch.dynamic_mask_with_coords, models/richsem/cond_inst.py:
 * 337-435, with compute_locations, parse_dynamic_params and aligned_bilinear of the same file) ----------------------------------------------
 * feat (N, C, H, W), params (N, Q, P) and out (N, R, F H, F W) fp32 / bf16, read and written as stored;  ref (N, Q, 2) fp32 the normalised
 * reference point (x, y);  sizes (N, 2) fp32 the image size (h, w);  inst (N, R) int32 ON THE DEVICE: the query of output row r, a value
 * outside [0, Q) = no query.  C = 8 or 16, hidden width 8, F = `factor` = 2 (mask_out_stride 4) or 1 (mask_out_stride 8).  Per image n, row r
 * with query q and stride-8 pixel (y, x):
 *   in = [ref_x size_w - (8 x + 4), ref_y size_h - (8 y + 4), feat[n, :, y, x]]  (rel_coord = 0: the features alone; ref, sizes may be NULL)
 *   t  = w2 . relu(W1 relu(W0 in + b0) + b1) + b2,  a parameter row = W0 (8, Cin) row-major, W1 (8, 8), w2 (8), b0 (8), b1 (8), b2 (1),
 *        P = 8 Cin + 89 (169 / 233 with the coordinates)
 *   out[n, r] = aligned_bilinear(t, F): per axis F[0] = T[0], F[2 k + 1] = T[k], F[2 k] = (T[k - 1] + T[k]) / 2; a row without a query is zeros.
 * msda_dynmask_table: fills inst from `rows` (N, R) int64 (a value outside [0, Q): -1), else from offsets (N + 1) / query_of_target (cap), the
 *   operands of msda_mask_loss_* (R = Q; inst[n, q] = q where image n has a pair for q, else -1), else -- all three NULL -- the identity.
 * msda_dynmask_backward_*: grad_out (N, R, F H, F W) -> grad_params (N, Q, P) (every element written once; zeros for a query no row names;
 *   rows naming one query are added in ascending order), grad_feat (N, C, H, W), and, when non-NULL, grad_ref (N, Q, 2) fp32, the gradient for
 *   the normalised point.  The chain is recomputed; per-tile partial sums in `workspace`, added in ascending order.
 * Limits: N, H, W, Q, R >= 1, C in {8, 16}, factor in {1, 2}, rel_coord in {0, 1}, R = Q for the tables without `rows` (MSDA_ERR_BAD_DIMS);
 * N <= 65535, H, W <= 2^14, R <= 2^20, N R 4 H W < 2^40 (MSDA_ERR_TOO_LARGE); workspace 16-byte aligned, out `factor` elements, the others their
 * element (MSDA_ERR_MISALIGNED).  Every check comes before any launch; no call allocates, synchronises or uses atomics; two calls give the
 * same bits. */
int msda_dynmask_workspace_bytes(int N, int C, int H, int W, int Q, int R, int64_t *bytes);
int msda_dynmask_table(const int64_t *rows, const int64_t *offsets, const int64_t *query_of_target, int N, int R, int Q, int64_t cap, int *inst,
                       msda_stream_t stream);
int msda_dynmask_forward_f32(const float *feat, const float *params, const float *ref, const float *sizes, const int *inst, int N, int C, int H,
                             int W, int Q, int R, int rel_coord, int factor, float *out, msda_stream_t stream);
int msda_dynmask_forward_bf16(const uint16_t *feat, const uint16_t *params, const float *ref, const float *sizes, const int *inst, int N, int C,
                              int H, int W, int Q, int R, int rel_coord, int factor, uint16_t *out, msda_stream_t stream);
int msda_dynmask_backward_f32(const float *grad_out, const float *feat, const float *params, const float *ref, const float *sizes, const int *inst,
                              int N, int C, int H, int W, int Q, int R, int rel_coord, int factor, float *grad_params, float *grad_feat,
                              float *grad_ref, void *workspace, msda_stream_t stream);
int msda_dynmask_backward_bf16(const uint16_t *grad_out, const uint16_t *feat, const uint16_t *params, const float *ref, const float *sizes,
                               const int *inst, int N, int C, int H, int W, int Q, int R, int rel_coord, int factor, uint16_t *grad_params,
                               uint16_t *grad_feat, float *grad_ref, void *workspace, msda_stream_t stream);

/* ---- attention core of CLIP's AttentionPool2d for its single query token (reference
 * clip/model.py:58-91, called at models/richsem/richsem.py:753 on the ROIAlign output) -----------------------------------
 * With one query per head the key / value projections move to the other side of the attention (csrc/msda_attnpool.h): the caller
 * forms u[k, h, :] = head_dim^-1/2 * Wk_h^T q[k, h, :] with a library GEMM, this kernel computes per (ROI k, head h)
 *     x_0 = mean_t feat[k, :, t] + pos[0],  x_{t+1} = feat[k, :, t] + pos[t + 1]          (tokens, never materialised)
 *     a = softmax_t(u[k, h] . x_t),   z[k, h, :] = sum_t a_t x_t
 * and the caller finishes with Wv_h z[k, h] + bv_h and the output projection.
 * u, z (K, H, C), or (H, K, C) when head_major != 0; feat (K, C, T) as msda_roi_align_forward_* writes it; pos (T + 1, C);
 * spos = u . pos^T, rows as u, T + 1 columns (one library GEMM of the caller's); T <= 256. */
int msda_attnpool_core_f32(const float *u, const float *feat, const float *pos, const float *spos, int K, int H, int C, int T,
                           int head_major, float *z, msda_stream_t stream);
int msda_attnpool_core_f64(const double *u, const double *feat, const double *pos, const double *spos, int K, int H, int C, int T,
                           int head_major, double *z, msda_stream_t stream);

/* ---- the Hungarian matcher's cost blocks (reference models/richsem/matcher.py:49-78 with
 * util/box_ops.py:9-59) --------------------------------------------------------------------------------------------
 *     C[b][q][t] = w_bbox * |box_q - box_t|_1 + w_class * (focal-style class cost at label_t) + w_giou * (-GIoU(box_q, box_t))
 * for query q of image b against target t of THE SAME image only (the blocks the reference keeps, matcher.py:76-77), with the
 * reference's arithmetic in the reference's order.  logits (B, Q, C); boxes (B, Q, 4) cxcywh; tgt_ids (n_targets) int64;
 * tgt_boxes (n_targets, 4) cxcywh; tgt_offsets (B + 1) int64 ON THE DEVICE = exclusive prefix of the per-image target counts
 * (tgt_offsets[B] <= n_targets: n_targets is the CAPACITY of tgt_ids / tgt_boxes / cost, of which the first tgt_offsets[B] targets are
 * live; the kernel writes Q * tgt_offsets[B] elements and neither reads the target rows nor writes the cost elements past them).
 * cost: Q * n_targets elements; image b's (Q x T_b) row-major block starts at element Q * tgt_offsets[b].  Several decoder outputs are matched by calling this once per output into consecutive slices of one buffer
 * and copying that buffer to the host once.  A label outside [0, C) gives NaN in its column. */
int msda_matcher_cost_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_boxes,
                          const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                          double w_giou, double alpha, float *cost, msda_stream_t stream);
int msda_matcher_cost_f64(const double *logits, const double *boxes, const int64_t *tgt_ids, const double *tgt_boxes,
                          const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                          double w_giou, double alpha, double *cost, msda_stream_t stream);
/* The same entries with every block stored TARGET-major: entry (q, t) of image b at element Q * tgt_offsets[b] + t * Q + q.  The layout
 * msda_lsap_* scans with unit stride (target_major = 1); the value of every entry is msda_matcher_cost_*'s. */
int msda_matcher_cost_tm_f32(const float *logits, const float *boxes, const int64_t *tgt_ids, const float *tgt_boxes,
                             const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                             double w_giou, double alpha, float *cost, msda_stream_t stream);
int msda_matcher_cost_tm_f64(const double *logits, const double *boxes, const int64_t *tgt_ids, const double *tgt_boxes,
                             const int64_t *tgt_offsets, int B, int Q, int C, int64_t n_targets, double w_class, double w_bbox,
                             double w_giou, double alpha, double *cost, msda_stream_t stream);

/* ---- the Hungarian assignment on the device (csrc/msda_lsap.h; what the reference asks scipy.optimize.linear_sum_assignment for on
 * the host, models/richsem/matcher.py:76-78) ------------------------------------------------------------------------------------
 * Exact linear sum assignment of n_out * B cost blocks in ONE launch: shortest augmenting paths with dual variables (Jonker-Volgenant
 * as in Crouse 2016, the algorithm of scipy's rectangular_lsap), float64 arithmetic whatever the cost type, one wave per block.
 *   cost             n_out consecutive buffers of Q * n_targets elements, each as msda_matcher_cost_* (target_major = 0) or
 *                    msda_matcher_cost_tm_* (target_major = 1) writes it: image b's Q x T_b block at element Q * tgt_offsets[b]
 *   tgt_offsets      (B + 1) int64 ON THE DEVICE, tgt_offsets[B] <= n_targets (n_targets is the capacity of a cost buffer and of a row
 *                    of query_of_target).  The block sizes are read from it by the kernel: the launch depends on n_out, B, Q and n_targets
 *                    only, so a captured launch stays valid when the per-image counts AND their total change under the same capacity;
 *                    query_of_target[o][t] for t >= tgt_offsets[B] is not written
 *   query_of_target  (n_out, n_targets) int64: the query assigned to target t of output o, -1 for a target left without one (T_b > Q:
 *                    exactly Q targets of the block are assigned) and for every target of a block that was not solved
 *   status           (n_out, B) int32: 0 solved; 1 the block holds a non-finite cost (found by a scan before the solve; scipy raises
 *                    there); 2 no augmenting path of finite length (finite costs whose float64 sums overflow); 3 tgt_offsets does not
 *                    describe a block inside n_targets (nothing read or written for it)
 *   workspace        msda_lsap_workspace_bytes() bytes, 4-byte aligned; may be NULL when that is 0 (every size supported today keeps its
 *                    state in LDS and needs none)
 * Limits: Q <= 4096 and n_targets <= 4096, MSDA_ERR_TOO_LARGE beyond (from both entry points, nothing launched).  Among assignments of
 * equal total cost the choice is the kernel's own, not scipy's.  No allocation, no synchronisation. */
int msda_lsap_workspace_bytes(int n_out, int B, int Q, int64_t n_targets, int64_t *bytes);
int msda_lsap_f32(const float *cost, int target_major, const int64_t *tgt_offsets, int n_out, int B, int Q, int64_t n_targets,
                  int64_t *query_of_target, int32_t *status, void *workspace, msda_stream_t stream);
int msda_lsap_f64(const double *cost, int target_major, const int64_t *tgt_offsets, int n_out, int B, int Q, int64_t n_targets,
                  int64_t *query_of_target, int32_t *status, void *workspace, msda_stream_t stream);

/* ---- PostProcess on the device (csrc/msda_postproc.h; reference models/richsem/richsem.py:1309-1367) ----------------------------------
 * msda_postprocess_select: per image the k largest of the Q * C logits, in descending order, with what PostProcess makes of them:
 *   logits      (B, Q, C) f32, or bf16 when logits_is_bf16; boxes (B, Q, 4) f32 (cx, cy, w, h); sizes_hw (B, 2) f32 (height, width)
 *   scores      (B, k) f32 = sigmoid(logit) of the winners (from the f32 value of the logit)
 *   labels, query_idx (B, k) int64 = flat index % C, flat index / C
 *   out_boxes   (B, k, 4) f32: the winner's query box, box_mode 0 as it is (cx, cy, w, h), 1 as (x1, y1, x2, y2) = (cx - 0.5 w, cy - 0.5 h,
 *               cx + 0.5 w, cy + 0.5 h), 2 as (x1, y1, x2 - x1, y2 - y1); then times (width, height, width, height).  Every operation is
 *               rounded to float32 on its own, so the boxes are bit-equal to the reference's float32 tensor arithmetic.
 * The order is float comparison of the LOGITS with -0.0 == +0.0 and every NaN above +inf; equal logits are taken lowest flat index first,
 * so the result is determined by the input (exact for every input: all-equal rows, any number of elements equal to the k-th largest).
 * Limits: B >= 1, 1 <= k <= 1024, k <= Q * C (MSDA_ERR_BAD_DIMS), Q * C < 2^31, and B * max(6160, ceil((Q * C + 7) / 8192)) < 2^31 -- the
 * call's workgroups and zeroed words, some 348 000 images -- (MSDA_ERR_TOO_LARGE); logits, boxes, out_boxes and workspace 16-byte aligned
 * (MSDA_ERR_MISALIGNED).  workspace: msda_postprocess_workspace_bytes() bytes, contents irrelevant on entry
 * (the call zeroes what it counts in, on `stream`); it must not be shared by calls that may run concurrently.
 * msda_nms_f32: torchvision's nms of K <= 1024 boxes per image that are ALREADY in descending score order (as msda_postprocess_select
 * writes them): box i, unless suppressed itself, suppresses every later box j with inter / (area_i + area_j - inter) > iou_threshold in
 * float32, areas (x2 - x1) * (y2 - y1) (0 / 0 is NaN and suppresses nothing; a NaN coordinate suppresses nothing either for
 * iou_threshold >= 0, as in torchvision, though by another route: the clamp of the intersection's sides at 0 drops a NaN here and
 * propagates it there, and neither 0 nor NaN is above such a threshold); with labels (B, K) int64 only where the two labels are equal
 * (batched_nms).  keep (B, K) uint8; kept_idx (B, K) int64: the kept positions in ascending order (= descending score), then -1;
 * n_kept (B) int32.  boxes_xyxy 16-byte aligned.
 * None of these allocates, synchronises or reads device memory on the host: they can be captured into a graph. */
int msda_postprocess_workspace_bytes(int B, int Q, int C, int k, int64_t *bytes);
int msda_postprocess_select(const void *logits, int logits_is_bf16, const float *boxes, const float *sizes_hw,
                            int B, int Q, int C, int k, int box_mode,
                            float *scores, int64_t *labels, float *out_boxes, int64_t *query_idx,
                            void *workspace, msda_stream_t stream);
int msda_nms_f32(const float *boxes_xyxy, const int64_t *labels_or_null, int B, int K, float iou_threshold,
                 uint8_t *keep, int64_t *kept_idx, int32_t *n_kept, msda_stream_t stream);

/* ---- feed-forward block of the transformer layers on the matrix cores ----------
 *     out = LayerNorm(x + W2 . relu(W1 . x + b1) + b2)
 * reference: models/richsem/deformable_transformer.py:862-866 (encoder forward_ffn), :940-944 (decoder forward_ffn), with
 * activation = relu and the dropouts inactive (p = 0.0 in the shipped configs, or eval mode).  bf16 storage, fp32
 * accumulation; the hidden activation is rounded to bf16 once (as a bf16 nn.Linear would), everything after the second
 * product (bias, residual, LayerNorm) is fp32 and rounded once at the store.  New capability: the reference runs fp32.
 *   x, out       (tokens, d_model) bf16, row-major;  d_model must be 256
 *   w1           (d_ffn, d_model) bf16 = linear1.weight;  b1 (d_ffn) f32 = linear1.bias;  d_ffn % 32 == 0, <= 4096
 *   w2_packed    linear2.weight (d_model, d_ffn) bf16 after msda_ffn_pack_w2_bf16 (a fixed permutation of the hidden
 *                columns inside every group of 32: repack whenever the weight changes);  b2 (d_model) f32
 *   ln_weight, ln_bias (d_model) f32, eps as nn.LayerNorm.  All pointers 16-byte aligned. */
/* Training: the forward that also writes the LayerNorm's 1 / sqrt(var + eps) per token (rstd: `tokens` floats) and its normalised input
 * yhat = (y - mean) * rstd ((tokens, 256) bf16) -- either may be NULL -- and the first step of the backward: from dy (gradient of out),
 * yhat and rstd the gradient dz at the LayerNorm's input (= gradient of the residual x and of the second product's output, bf16) and the
 * token sums grad_ln_weight = sum dy * yhat, grad_ln_bias = sum dy, grad_b2 = sum dz (f32, 256 each, zeroed by the call).  The products
 * of the backward are msda_lin256_forward_bf16 (recomputed hidden activation, dH with the ReLU mask), msda_conv_wgrad_bf16 (weight
 * gradients) and one library GEMM (dx = dz + dHm W1), see richsem_amd/functions/ffn.py. */
int msda_ffn_forward_train_bf16(const uint16_t *x, const uint16_t *w1, const float *b1, const uint16_t *w2_packed, const float *b2,
                                const float *ln_weight, const float *ln_bias, float eps, int tokens, int d_model, int d_ffn,
                                uint16_t *out, float *rstd, uint16_t *yhat, msda_stream_t stream);
int msda_ffn_ln_backward_bf16(const uint16_t *dy, const uint16_t *yhat, const float *rstd, const float *ln_weight, int tokens, int d_model,
                              uint16_t *dz, float *grad_ln_weight, float *grad_ln_bias, float *grad_b2, msda_stream_t stream);
/* Residual add + LayerNorm of the transformer layers (reference deformable_transformer.py:876-877: src = norm1(src + dropout1(src2)),
 * with the dropout inactive): out = LayerNorm(a + b) over 256 channels; a, b (b may be NULL), out (tokens, 256) bf16; ln_weight, ln_bias
 * f32; rstd (tokens) f32 and yhat (tokens, 256) bf16 for the backward (either may be NULL), which is msda_ffn_ln_backward_bf16: its dz is
 * the gradient of a and of b. */
int msda_add_layernorm_forward_bf16(const uint16_t *a, const uint16_t *b, const float *ln_weight, const float *ln_bias, float eps, int tokens,
                                    int d_model, uint16_t *out, float *rstd, uint16_t *yhat, msda_stream_t stream);

/* out = act(x W^T + b) for in_features = 256 on the matrix cores (csrc/lin256_mfma.hip; bf16 storage, fp32 accumulation): the two
 * token-parallel products of the feed-forward block's backward.  msda_lin256_pack_bf16: W (out_features, 256) bf16 row-major -> the same
 * number of elements in MFMA fragment order (out_features % 64 == 0).  epilogue 0: acc + bias (bias may be NULL); 1: relu(acc + bias);
 * 2: acc where relu_mask > 0, else 0 (relu_mask (tokens, out_features) bf16: the forward's hidden activation); 3: acc + bias with the
 * rows of masked tokens zeroed (relu_mask then points to `tokens` bytes, non-zero = masked: MSDeformAttn's value projection with its
 * padding mask, ops/modules/ms_deform_attn.py:94-96).  16-byte aligned pointers (the byte mask of epilogue 3: any alignment). */
int msda_lin256_pack_bf16(const uint16_t *w, int out_features, int in_features, uint16_t *packed, msda_stream_t stream);
int msda_lin256_forward_bf16(const uint16_t *x, const uint16_t *packed_w, const float *bias, const uint16_t *relu_mask, int epilogue,
                             int tokens, int in_features, int out_features, uint16_t *out, msda_stream_t stream);
/* Several 256 -> 256 layers stacked into one product (out_features = 256 * layers, W and bias concatenated along the outputs): out is
 * `layers` separate contiguous (tokens, 256) matrices, one after the other; row_mask (tokens bytes, non-zero = zero that token's rows)
 * may be NULL.  The decoder's cross-attention value projections of all its layers: the memory is read once. */
int msda_lin256_forward_stacked_bf16(const uint16_t *x, const uint16_t *packed_w, const float *bias, const uint8_t *row_mask, int tokens,
                                     int in_features, int out_features, uint16_t *out, msda_stream_t stream);
/* Masked multi-head self-attention of the decoder's queries (csrc/attn_mfma.hip; reference: nn.MultiheadAttention of
 * DeformableTransformerDecoderLayer, models/richsem/deformable_transformer.py:907, :974-978): softmax(q k^T / sqrt(32) + mask) v per
 * (image, head), head dimension 32, bf16 storage, fp32 softmax -- new capability (the reference runs torch's fp32 attention).
 * Token (i, b) is row i * bs + b of q / k / v (sequence-first, batch_first = 0) or row b * nq + i (batch_first = 1), `ld*` elements
 * apart, a head's 32 channels at column 32 h; out / dout the same rows, heads * 32 wide, contiguous; lse (bs * heads, ceil32(nq)) f32: log2-sum-exp per query, written by the forward, read by
 * the backward; mask_bits (nq, ceil(nq / 32)) uint32: bit j of word (q, kb) set = query q must not attend to key 32 kb + j;
 * maskt_bits the same of the transposed mask (both NULL = no mask); workspace: msda_attn_workspace_bytes(nq, bs, heads) bytes.
 * 16-byte aligned pointers, ld* multiples of 8.  Every element of out / dq / dk / dv is written.  A query whose mask row allows no key
 * gets out = 0 and lse = +inf, its dq is 0 and it contributes nothing to dk / dv (torch's softmax gives NaN there); the entries
 * [nq, ceil32(nq)) of every lse row are +inf as well. */
int64_t msda_attn_workspace_bytes(int nq, int bs, int heads);
int msda_attn_forward_bf16(const uint16_t *q, int ldq, const uint16_t *k, int ldk, const uint16_t *v, int ldv, const uint32_t *mask_bits,
                           int nq, int bs, int batch_first, int heads, uint16_t *out, float *lse, void *workspace, msda_stream_t stream);
int msda_attn_backward_bf16(const uint16_t *q, int ldq, const uint16_t *k, int ldk, const uint16_t *v, int ldv, const uint16_t *out,
                            const uint16_t *dout, const float *lse, const uint32_t *mask_bits, const uint32_t *maskt_bits, int nq, int bs,
                            int batch_first, int heads, uint16_t *dq, int lddq, uint16_t *dk, int lddk, uint16_t *dv, int lddv, void *workspace,
                            msda_stream_t stream);
/* The same product for fp32 tensors at fp32-level accuracy (both operands split into bf16 hi + lo parts, three bf16 MFMAs per tile;
 * csrc/lin256_mfma.hip): out (tokens, out_features) f32 = x (tokens, 256) f32 . W^T + bias.  msda_lin256_pack_f32: W (out_features, 256)
 * f32 -> 2 * out_features * 256 uint16 (hi and lo parts in fragment order); out_features % 32 == 0.  The MSDeformAttn module's fp32
 * projections (reference ops/modules/ms_deform_attn.py:52-56). */
int msda_lin256_pack_f32(const float *w, int out_features, int in_features, uint16_t *packed, msda_stream_t stream);
int msda_lin256_forward_f32(const float *x, const uint16_t *packed_w, const float *bias, int tokens, int in_features, int out_features,
                            float *out, msda_stream_t stream);
/* Diagnostic: non-NULL = the kernel adds up the shader clocks wave 0 of every workgroup spends per loop stage (wait for the
 * weight tile, barrier, first product, relu + conversion, second product) into 8 x 8 bytes per workgroup; NULL = off. */
int msda_ffn_debug_stamps(void *device_buffer);
int msda_ffn_pack_w2_bf16(const uint16_t *w2, int d_model, int d_ffn, uint16_t *w2_packed, msda_stream_t stream);
int msda_ffn_forward_bf16(const uint16_t *x, const uint16_t *w1, const float *b1, const uint16_t *w2_packed, const float *b2,
                          const float *ln_weight, const float *ln_bias, float eps, int tokens, int d_model, int d_ffn,
                          uint16_t *out, msda_stream_t stream);

/* Gradient clipping + AdamW + EMA of the weights in two launches (csrc/msda_optim.h, csrc/optim_api.hip; reference engine.py:110-120:
 * clip_grad_norm_(max_norm), optimizer.step(), ema_m.update(model)).  float32 parameters, gradients and state.  The kernels read
 * everything from DEVICE-resident tables, so a captured step follows a learning-rate schedule without being captured again:
 *
 *   tensors   one msda_optim_tensor per tensor: device pointers (4-byte aligned, contiguous `numel` floats each), the group it belongs to
 *             and its step counter (a float, as torch.optim keeps it);
 *   chunks    msda_optim_chunk: chunk -> (tensor, offset, count), count <= MSDA_OPTIM_CHUNK, no chunk spans two tensors, a tensor's chunks
 *             in order -- filled by msda_optim_plan (host only) from the list of numel: one workgroup per chunk, so every workgroup gets
 *             a bounded, similar amount of work whatever the tensor sizes;
 *   groups    msda_optim_group per parameter group;   settings: msda_optim_settings, call-wide.
 *
 * msda_optim_sumsq: partials[c] = sum of grad^2 over chunk c (fixed order, plain stores), and every listed tensor's step += 1.
 * msda_optim_step:  every workgroup adds the partials in one fixed order; total_norm = sqrt(sum) (stored by workgroup 0),
 *                   coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 as torch.nn.utils.clip_grad_norm_ (max_norm <= 0: coef = 1, the
 *                   reference's `if max_norm > 0`), then torch's AdamW per element with g' = coef * g:
 *                   p *= 1 - lr wd;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),
 *                   bc = 1 - beta^step from the tensor's own counter (double, once per workgroup); where settings.ema_on and the tensor
 *                   has an `ema` pointer also ema = decay ema + (1 - decay) p_new (reference util/utils.py:396-397).
 *                   The gradient is READ, never written (clip_grad_norm_ scales p.grad in place; here coef * g exists only in registers).
 *                   Non-finite gradients behave as the torch sequence: an inf gives coef = 0 (NaN at that element, a zero-gradient update
 *                   elsewhere), a NaN gives NaN everywhere.
 * msda_optim_ema:   ema = decay ema + (1 - decay) param over a table whose tensors carry `ema` and `param` only.
 * Host checks (before any launch): null tables, n_chunks / n_tensors < 1, tables not aligned to 8 bytes (total_norm: 4). */
#define MSDA_OPTIM_CHUNK 16384
typedef struct msda_optim_tensor {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *ema;          /* NULL: no shadow */
    float *step;         /* one float on the device */
    int64_t numel;
    int32_t group;
    int32_t reserved;
} msda_optim_tensor;
typedef struct msda_optim_chunk {
    int64_t offset;      /* first element, a multiple of MSDA_OPTIM_CHUNK */
    int32_t tensor;
    int32_t count;
} msda_optim_chunk;
typedef struct msda_optim_group {
    double lr, beta1, beta2, eps, weight_decay;
} msda_optim_group;
typedef struct msda_optim_settings {
    double max_norm;     /* <= 0: no clipping */
    double ema_decay;
    int32_t ema_on;
    int32_t reserved;
} msda_optim_settings;
/* chunks may be NULL (count only); otherwise at most `capacity` entries are written and a larger need is MSDA_ERR_BAD_DIMS */
int msda_optim_plan(const int64_t *numel, int n_tensors, msda_optim_chunk *chunks, int64_t capacity, int64_t *n_chunks);
int msda_optim_sumsq(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, double *partials, msda_stream_t stream);
int msda_optim_step(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, const double *partials,
                    const msda_optim_group *groups, const msda_optim_settings *settings, float *total_norm, msda_stream_t stream);
int msda_optim_ema(const msda_optim_tensor *tensors, const msda_optim_chunk *chunks, int n_chunks, const msda_optim_settings *settings,
                   msda_stream_t stream);

/* Grouped re-pack: every derived form of the trained parameters (bf16 casts, lin256's fragment order, the feed-forward kernel's W2 order,
 * the convolutions' forward and input-gradient packs) rebuilt from the fp32 masters in ONE launch over a device-resident job table
 * (csrc/msda_repack.h, csrc/repack_api.hip).  Every form is a destination-indexed gather: an output element is one source element, at
 * most multiplied by one fp32 scale, rounded to bf16 (nearest even) -- bit-equal to what the single-form entry points
 * (msda_lin256_pack_bf16, msda_ffn_pack_w2_bf16, msda_conv_pack_weight) write from the same masters.
 *
 *   jobs      one msda_repack_job per destination tensor.  The source is the concatenation of `n_segs` fp32 segments (4-byte aligned,
 *             contiguous; a segment may be a row slice of a larger parameter); seg_end[s] is the cumulative end of segment s, counted in
 *             rows for the lin256 kinds and in elements for the flat kinds; the convolution kinds read src[0] only.
 *   chunks    msda_repack_chunk: chunk -> (job, offset, count) in destination elements, count <= MSDA_REPACK_CHUNK, no chunk spans two
 *             jobs -- filled by msda_repack_plan: one workgroup per chunk, 16 bytes of destination per thread and store.
 *
 * kinds (n_dst = destination elements; dims as listed, the rest 0):
 *   MSDA_REPACK_CAST      bf16 of the flat concatenation, zero from its end up to n_dst
 *   MSDA_REPACK_COPY      fp32 copy of the flat concatenation, zero from its end up to n_dst
 *   MSDA_REPACK_LIN256    dims[0] = N (a multiple of 64, n_dst = 256 N): msda_lin256_pack_bf16 of the (N x 256) row concatenation, rows
 *                         from its end up to N zero
 *   MSDA_REPACK_LIN256_T  dims[0] = N: msda_lin256_pack_bf16 of the transpose of the (256 x N) row concatenation
 *   MSDA_REPACK_FFN_W2    dims[0] = d_model, dims[1] = d_ffn (a multiple of 32, n_dst = d_model d_ffn): msda_ffn_pack_w2_bf16
 *   MSDA_REPACK_CONV      dims = Cout, Cin, KH, KW, Kpad (KH KW Cin rounded up to 32; n_dst = Cout Kpad): msda_conv_pack_weight
 *   MSDA_REPACK_CONV_T    dims = Cout, Cin, KH, KW of the SOURCE, Kpad (KH KW Cout rounded up to 32; n_dst = Cin Kpad): msda_conv_pack_weight
 *                         of w_t[ci][co][kh][kw] = w[co][ci][KH-1-kh][KW-1-kw] * scale[co], the product taken in fp32 (`scale`: Cout floats)
 *
 * msda_repack_plan (host only) checks the HOST copy of the job table -- null dst / src / scale (MSDA_ERR_NULL_POINTER), a dst not aligned
 * to 16 bytes or a src / scale not aligned to 4 (MSDA_ERR_MISALIGNED), an unknown kind, n_segs outside 1..MSDA_REPACK_MAX_SEGS, segment
 * ends that do not grow, dims and n_dst that do not fit the kind (MSDA_ERR_BAD_DIMS), n_dst or the chunk count >= 2^31
 * (MSDA_ERR_TOO_LARGE) -- and writes the chunk table; chunks may be NULL (count only), a need above `capacity` is MSDA_ERR_BAD_DIMS.  A
 * job with n_dst = 0 has no chunks, and only its kind and n_segs are checked.
 * msda_repack: one launch of n_chunks workgroups over DEVICE copies of both tables (8-byte aligned); n_chunks = 0 launches nothing,
 * n_chunks < 0 is MSDA_ERR_BAD_DIMS.  No host synchronisation; capturable. */
#define MSDA_REPACK_CHUNK 8192
#define MSDA_REPACK_MAX_SEGS 8
enum msda_repack_kind {
    MSDA_REPACK_CAST = 0,
    MSDA_REPACK_COPY = 1,
    MSDA_REPACK_LIN256 = 2,
    MSDA_REPACK_LIN256_T = 3,
    MSDA_REPACK_FFN_W2 = 4,
    MSDA_REPACK_CONV = 5,
    MSDA_REPACK_CONV_T = 6
};
typedef struct msda_repack_job {
    void *dst;                                 /* 16-byte aligned */
    const float *scale;                        /* MSDA_REPACK_CONV_T only, else NULL */
    const float *src[MSDA_REPACK_MAX_SEGS];
    int32_t seg_end[MSDA_REPACK_MAX_SEGS];     /* cumulative: rows (lin256 kinds) or elements (flat kinds) */
    int64_t n_dst;                             /* destination elements */
    int32_t kind;
    int32_t n_segs;
    int32_t dims[6];
    int32_t reserved[2];
} msda_repack_job;
typedef struct msda_repack_chunk {
    int64_t offset;      /* first destination element, a multiple of MSDA_REPACK_CHUNK */
    int32_t job;
    int32_t count;
} msda_repack_chunk;
int msda_repack_plan(const msda_repack_job *jobs, int n_jobs, msda_repack_chunk *chunks, int64_t capacity, int64_t *n_chunks);
int msda_repack(const msda_repack_job *jobs, const msda_repack_chunk *chunks, int n_chunks, msda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RICHSEM_MSDA_H */
