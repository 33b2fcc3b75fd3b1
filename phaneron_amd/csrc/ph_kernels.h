// ph_kernels.h - host-visible launchers of the gfx950 kernels (ph_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ph_formats.h"
#include "ph_lut.h"

namespace ph {

constexpr int kMaxLayers = 8;
// every kernel with a dynamic LDS array is allowed the CU's whole 160 KiB once and for all: the attribute is per-function state, and
// setting it to each launch's own size would let two launching threads undercut each other
constexpr int kMaxDynamicLds = 160 * 1024;

// 1 = f32 image outputs of the launches issued by this thread are streamed past the caches (ph_device.h store_image);
// set from the context's "stream_images" option before every launch (ph_api.cpp set_device)
extern thread_local uint32_t t_stream_images;  // 0 cached, 1 streamed, 2 by size
extern thread_local uint32_t t_stream_threshold_mb;
// the store policy of ONE image of `bytes` bytes written by the launch being issued
static inline uint32_t image_nt(size_t bytes) {
  return t_stream_images == 2 ? (bytes > ((size_t)t_stream_threshold_mb << 20) ? 1u : 0u) : t_stream_images;
}

struct FusedArgs {
  const void *layers[kMaxLayers];
  void *out;
  uint32_t quads_per_line_used;   // width / 6
  uint32_t quads_per_line_pitch;  // pitch bytes / 16
  uint32_t total_quads;           // quads_per_line_used * height
  const float *rd_cm, *rd_lut, *rd_gm, *wr_cm, *wr_lut;
  // widths that are not a multiple of 48 (the LDS kernel's TAIL instantiation only): total_quads counts the quad SLOTS of the
  // pitch, a line is quads_per_line_used whole quads, then - if tail_px (2 or 4) - the tail quad, then cleared slots
  uint32_t tail_px, magic_qpp;  // width % 6; ceil(2^32 / quads_per_line_pitch)
};

constexpr int kMaxBatch = 8;
// The lookup constants of one table (LutK of ph_ldslut.h) as the HOST finishes them: they are the same for every lane of every
// launch that uses the table, and the fused kernel used to rebuild both records from the LutViews in front of its first memory
// instruction.  fused_lut_k makes them with make_lut_k's float operations in make_lut_k's order (the LDS base is 0:
// ph_lut_register checks it), so the bits are the device's; tests/test_fused_args_cpu.py compares them for every layout.
struct FusedLutK {
  float a_scale, a_base, delta_scale, delta_base;
  uint32_t a_shift;
};
FusedLutK fused_lut_k(const LutView &v);  // ph_kernels_lds.hip (host code)

// blockIdx.x / wg_per_job of the fused kernel without a division: magic = ceil(2^31 / wg_per_job) (fused_wg_magic), and the
// high word of (2 * block + 1) * magic is the quotient - floor((block + 1/2) / d) == floor(block / d), and the half leaves room
// for the magic's rounding as long as (block + 1) * wg_per_job <= 2^30.  (ceil(2^32 / d) needs 33 bits at d = 1.)
static inline uint32_t fused_wg_magic(uint32_t wg_per_job) { return (uint32_t)(((1ull << 31) + wg_per_job - 1) / wg_per_job); }
static inline __host__ __device__ uint32_t fused_job_of(uint32_t block, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(2u * block + 1u, magic);
#else
  return (uint32_t)(((uint64_t)(2u * block + 1u) * magic) >> 32);
#endif
}

// The fused LDS kernel's arguments.  What the kernel needs in front of its first vector memory instruction - the job arithmetic,
// the reader table's place, the first layers - is the first 64-byte line; the rest of what its head reads fills the next two, and
// the kernel asks for all 192 bytes in one request and waits once (ph_kernels_lds.hip).  The listed fields take 168 bytes, so
// 128 cannot hold them.  The launcher fills `jobs` < 1 as 1, wg_per_job, per_wg and magic_wg.
struct alignas(64) FusedLdsArgs {
  // ---- bytes 0 .. 63
  const uint32_t *rd_blob;          // reader table (LutView of ph_lut.h): blob, LDS footprint, hole
  uint32_t rd_bytes, rd_hole;
  uint32_t total_quads;             // quads_per_line_used * height (ragged lines: quad slots of the pitch)
  // batched launch: `jobs` frames of identical geometry and colour parameters, each with its own
  // layers and output; workgroups [j * wg_per_job, (j + 1) * wg_per_job) work on job j
  uint32_t wg_per_job;
  uint32_t per_wg;                  // ceil(total_quads / wg_per_job): a workgroup's share
  uint32_t magic_wg;                // fused_wg_magic(wg_per_job)
  const void *layers[kMaxLayers];   // job 0 (bytes 32 .. 95)
  // ---- bytes 96 .. 127
  void *out;                        // job 0
  const float *rd_cm, *rd_gm, *wr_cm;
  // ---- bytes 128 .. 191
  FusedLutK rd_k, wr_k;
  uint32_t wr_bytes, wr_hole;       // writer table
  const uint32_t *wr_blob;
  uint32_t jobs;
  uint32_t quads_per_line_used;     // width / 6
  // ---- what the head does not read
  uint32_t quads_per_line_pitch;    // pitch bytes / 16
  // widths that are not a multiple of 48 (the TAIL instantiation only): see FusedArgs
  uint32_t tail_px, magic_qpp;
  // max |entry| over the reader table's finite entries (ph_lut_host.h lut_max_finite; the registry keeps it): what the kernel's
  // witness guard starts from (fused_witness_holds below).  Asked for behind the table DMA, like the colour coefficients.
  float rd_lmax;
  const void *more_layers[kMaxBatch - 1][kMaxLayers];
  void *more_out[kMaxBatch - 1];
};
constexpr size_t kFusedHeadBytes = 192;
static_assert(offsetof(FusedLdsArgs, rd_blob) == 0 && offsetof(FusedLdsArgs, rd_bytes) == 8 && offsetof(FusedLdsArgs, rd_hole) == 12 &&
              offsetof(FusedLdsArgs, total_quads) == 16 && offsetof(FusedLdsArgs, wg_per_job) == 20 && offsetof(FusedLdsArgs, per_wg) == 24 &&
              offsetof(FusedLdsArgs, magic_wg) == 28 && offsetof(FusedLdsArgs, layers) == 32,
              "line 0 of the fused kernel's head: ph_kernels_lds.hip reads it by offset");
static_assert(offsetof(FusedLdsArgs, out) == 96 && offsetof(FusedLdsArgs, rd_cm) == 104 && offsetof(FusedLdsArgs, rd_gm) == 112 &&
              offsetof(FusedLdsArgs, wr_cm) == 120, "the head's pointers end with the first 128 bytes");
static_assert(offsetof(FusedLdsArgs, rd_k) == 128 && offsetof(FusedLdsArgs, wr_k) == 148 && offsetof(FusedLdsArgs, wr_bytes) == 168 &&
              offsetof(FusedLdsArgs, wr_hole) == 172 && offsetof(FusedLdsArgs, wr_blob) == 176 && offsetof(FusedLdsArgs, jobs) == 184 &&
              offsetof(FusedLdsArgs, quads_per_line_used) == 188 && offsetof(FusedLdsArgs, quads_per_line_pitch) == kFusedHeadBytes,
              "line 2 of the fused kernel's head");
static_assert(offsetof(FusedLdsArgs, more_layers) >= kFusedHeadBytes, "the batch arrays lie behind the head");
// The fused kernel's witness guard (ph_kernels_lds.hip fused_layer_combine), uniform per launch: with every finite table entry
// at most lmax in magnitude, no product and no partial sum of a gamut row gm[3i .. 3i+2] . (r, g, b) of finite r, g, b exceeds
// lmax * (|g0| + |g1| + |g2|), so below 2^126 (a factor four under the largest float, for the roundings of the sums) nothing
// overflows and a lower layer's value is non-finite exactly where one of its three table entries is.  Every comparison is false
// for a NaN, and an Inf in gm makes a product Inf or (lmax = 0) NaN: any of them fails the guard.
static inline __host__ __device__ bool fused_witness_holds(float lmax, const float *gm) {
  const float bound = 8.5070591730234616e37f, half = 4.2535295865117308e37f;  // 2^126, 2^125
  bool ok = lmax < half;
  for (int i = 0; i < 3; ++i) {
    const float row = (__builtin_fabsf(gm[3 * i]) + __builtin_fabsf(gm[3 * i + 1])) + __builtin_fabsf(gm[3 * i + 2]);
    ok = ok & (lmax * row < bound);
  }
  return ok;
}
static_assert(offsetof(FusedLdsArgs, rd_lmax) == 204 && offsetof(FusedLdsArgs, more_layers) == 208, "rd_lmax fills a gap behind the head: no other field moves");
// the arguments of one frame (or of job 0 and what all jobs share) from the plain kernel's and the two tables; rd_lmax: the
// reader table's lut_max_finite
FusedLdsArgs fused_lds_args(const FusedArgs &f, const LutView &rd, const LutView &wr, float rd_lmax);  // ph_kernels_lds.hip

// Several consumers' frames of ONE plain-layer composite in one launch (ph_fused_v210_combine_multi; ph_kernels_fused_multi.hip): the
// headline kernel's phase 1, then the writer's phase once per distinct writer table - the quad's 18 table reads made once, every
// output of that table packing them with its own writer matrix.  width % 48 == 0 only: a line is quads_per_line whole quads, a planar
// pitch is the width.  The whole frame is composed; a field output stores the quads whose line has its parity (the field alone:
// launch_fused_v210_field_multi below).
// The launcher expects the outputs grouped by writer table.
constexpr int kMaxFusedOuts = 4;
struct FusedOut {
  uint32_t fmt;         // PH_FMT_* (one of fmt_chan_out)
  uint32_t takes;       // which lines are this output's: 0 all, 1 the even frame lines, 2 the odd ones
  uint32_t line_end;    // a field output: lines from here on are not its own (a field of a frame with an odd height)
  uint32_t field;       // 1: a field write (4:2:0: the written line of a pair gives the chroma)
  uint32_t half_pitch;  // launcher: chroma samples per chroma row
  uint32_t pad;
  const float *wr_cm;   // (unused for rgba8 / bgra8)
  void *plane[3];
  LutView wr;
};
struct FusedMultiArgs {
  const void *layers[kMaxLayers];
  uint32_t quads_per_line, total_quads;  // width / 6, quads_per_line * height
  uint32_t magic_qpl, need_line;         // launcher: ceil(2^32 / quads_per_line); 1: some output is a field or 4:2:0
  const float *rd_cm, *rd_gm;
  LutView rd;
  uint32_t n_out;
  FusedOut out[kMaxFusedOuts];
};
// named "fused_v210_combine_multi x<outputs>" in a route trace; n = 1..8 layers; one workgroup per CU, never more than slices and - a test
// and A/B hook, 0 = no cap - never more than max_wgs
hipError_t launch_fused_v210_combine_multi(hipStream_t s, int n, const FusedMultiArgs &a, uint32_t num_cus, uint32_t max_wgs);
// (the launcher's checks and planning, for the launchers of the single frame's kernels: ph_kernels_fused_multi.hip)
hipError_t fused_multi_plan(const FusedMultiArgs &a, uint32_t num_cus, uint32_t max_wgs, FusedMultiArgs &b, uint32_t &grid, uint32_t &lds);
// The same for `jobs` = 2..kMaxBatch frames of one geometry, layer count, reader recipe and output descriptors in one launch
// (ph_fused_v210_combine_multi_batch): the jobs differ in their layers and in their outputs' planes only.  m: what the jobs share
// (m.layers and m.out[k].plane are not read); layers[j] / plane[j][k]: job j's, k in m.out's order.
struct FusedMultiBatchArgs {
  FusedMultiArgs m;
  const void *layers[kMaxBatch][kMaxLayers];
  void *plane[kMaxBatch][kMaxFusedOuts][3];
};
// named "fused_v210_combine_multi x<outputs>j<jobs>"; max(1, num_cus / jobs) workgroups per job, never more than a job's slices and - 0 = no
// cap - never more than max_wgs; workgroups [j * per job, (j + 1) * per job) work on job j
hipError_t launch_fused_v210_combine_multi_batch(hipStream_t s, int n, uint32_t jobs, const FusedMultiBatchArgs &a, uint32_t num_cus, uint32_t max_wgs);
// The single frame's launch with layers in a TRANSITION (ph_fused_v210_transition_multi; ph_kernels_fused_trans.hip): a layer may bring a
// second v210 frame and, for a wipe, a mask - a v210 frame read like a layer (its red is the factor) or an f32 RGBA image (the red of
// pixel x, 16 bytes apart) - all of the output's size.  m: as launch_fused_v210_combine_multi takes it.
enum : uint32_t { kFusedCut = 0, kFusedDissolve = 1, kFusedWipeV210 = 2, kFusedWipeF32 = 3 };
struct FusedTransArgs {
  FusedMultiArgs m;
  const void *incoming[kMaxLayers];  // dissolve, wipe
  const void *mask[kMaxLayers];      // wipe
  uint32_t kind[kMaxLayers];         // kFused*
  float mix[kMaxLayers];             // dissolve
};
// named "fused_v210_trans_multi x<outputs>"; workgroups as launch_fused_v210_combine_multi
hipError_t launch_fused_v210_trans_multi(hipStream_t s, int n, const FusedTransArgs &a, uint32_t num_cus, uint32_t max_wgs);
// The single frame's launch with a ROUTED IMAGE among the layers and the combined image as an output (ph_fused_v210_route_multi;
// ph_kernels_fused_route.hip): a layer may be an f32 RGBA image of the output's size (16 bytes per pixel, rows unpadded) instead of a
// v210 frame, and image_out - or NULL - receives what ph_combine makes of the layers' images, to the bit.  m: as
// launch_fused_v210_combine_multi takes it, but m.n_out may be 0 with an image_out: the image alone, no writer table touched.
struct FusedRouteArgs {
  FusedMultiArgs m;
  uint32_t is_image[kMaxLayers];  // 1: m.layers[l] is an f32 RGBA image
  void *image_out;
  uint32_t nt;                    // launcher: image_out's store policy (image_nt)
};
// named "fused_v210_route_multi x<outputs>i<0|1>" (i1: the image is written); workgroups as launch_fused_v210_combine_multi
hipError_t launch_fused_v210_route_multi(hipStream_t s, int n, const FusedRouteArgs &a, uint32_t num_cus, uint32_t max_wgs);
// The single frame's and the batched launch for outputs that all take the SAME FIELD (context option "fused_fields";
// ph_kernels_fused_field.hip): only that field's lines are composed - first_line, first_line + 2, ... - and the workgroups' ranges,
// tiles and tails are counted in field quads (ph_fused_field.h).  m / b: as the whole-frame launchers take them, but total_quads is the
// FIELD's (quads_per_line * (height / 2)) and every output's takes is 0; their kernarg layout is the existing kernels', so the first
// line stands behind them.  interlace: the outputs' (1 or 3), for the trace name.
struct FusedFieldArgs {
  FusedMultiArgs m;
  uint32_t first_line;  // 0 (interlace 1) or 1 (interlace 3)
};
struct FusedFieldBatchArgs {
  FusedMultiBatchArgs b;
  uint32_t first_line;
};
// named "fused_v210_field_multi x<outputs>f<interlace>"; workgroups as launch_fused_v210_combine_multi, never more than the field's slices
hipError_t launch_fused_v210_field_multi(hipStream_t s, int n, const FusedFieldArgs &a, uint32_t interlace, uint32_t num_cus, uint32_t max_wgs);
// named "fused_v210_field_multi x<outputs>j<jobs>f<interlace>"; workgroups as launch_fused_v210_combine_multi_batch, of the field's slices
hipError_t launch_fused_v210_field_multi_batch(hipStream_t s, int n, uint32_t jobs, const FusedFieldBatchArgs &a, uint32_t interlace, uint32_t num_cus, uint32_t max_wgs);

struct ComposeArgs {
  const void *layers[kMaxLayers];
  const float *matrix[kMaxLayers];  // device 3x3 (transform) or NULL = the layer is used 1:1
  // optional wipe transition on a layer (transition.ts wipe): placed layer -> mix with `wipe_with` by `wipe_mask`.x,
  // both output-size RGBA images; NULL = none (ph_compose_wipe_write_v210)
  const void *wipe_with[kMaxLayers], *wipe_mask[kMaxLayers];
  int lw[kMaxLayers], lh[kMaxLayers];
  int n;
  void *out;
  uint32_t out_w, out_h, lines, first_line, line_step;
  const float *wr_cm;
  LutView wr;
};

// ph_kernels_chan.hip: the compositor that samples v210 sources directly
// planar YCbCr sources: 4:2:2 with 16-bit samples (yuv422p10le), 4:2:2 and 4:2:0 with 8-bit samples (yuv422p8, yuv420p), 4:2:0 with
// interleaved chroma (nv12); 4:2:0 with 16-bit samples, planar (yuv420p10le) or interleaved and MSB-aligned (p010le); ptr = the Y
// plane, ChanArgs::plane_u / plane_v the chroma planes (nv12, p010: plane_u holds CbCr pairs)
// and the packed 8-bit RGB formats of stills and graphics (rgba8, bgra8: four bytes per pixel, alpha included).
// The planar kinds are contiguous (kChanP10 .. kChanPlanarLast) and the packed-RGB ones come last: the kernels test ranges.
enum : uint32_t { kChanNone = 0, kChanV210 = 1, kChanRgba = 2, kChanP10 = 3, kChanP8x422 = 4, kChanP8x420 = 5, kChanNv12 = 6, kChanP10x420 = 7,
                  kChanP010 = 8, kChanRgba8 = 9, kChanBgra8 = 10, kChanPlanarLast = kChanP010 };
enum : uint32_t { kChanCut = 0, kChanDissolve = 1, kChanWipe = 2 };
struct ChanSrc {
  const void *ptr;
  uint32_t w, h, pitch;  // pixels, pixels, bytes per line
  uint32_t kind;         // kChanV210 / kChanRgba / a planar kind (kChanNone: absent)
  uint32_t sampled;      // 1 = through m (transform.ts:53-57), 0 = pixel for pixel
  uint32_t tail_from;    // v210: the first column of the line's tail, 6 * (w / 6) (== w when the width is a multiple of 6: no tail)
  float m[6];            // rows 0 and 1 of the 3x3 transform matrix
};
// The channel's frame as a flat program the kernel walks per pixel: one op per source to sample, with what to do with
// the sample.  A layer without a transition is one op (Layer); a dissolve is Hold (the layer's own source) + Dissolve (the
// incoming source); a wipe is Hold + Incoming + Wipe (the mask).  kChanActFirst marks the op that completes layer 0.
enum : uint32_t { kChanActLayer = 0, kChanActHold = 1, kChanActDissolve = 2, kChanActIncoming = 3, kChanActWipe = 4, kChanActFirst = 0x100,
                  // launcher: a v210 source shown at its own scale, unrotated - neighbouring lanes' taps are neighbouring columns, so a
                  // lane converts ONE column and takes the other from the lane beside it; bits 12..14: which halo table is the op's
                  kChanActShare = 0x200, kChanActShareShift = 12 };
constexpr int kMaxChanOps = 3 * kMaxLayers;
struct ChanOp {
  ChanSrc src;
  uint32_t action;
  float mix;
};
struct ChanArgs {
  ChanOp op[kMaxChanOps];
  int n_ops;
  uint32_t magic_cpr, magic_cpg;  // ceil(2^32 / chunks per row), ceil(2^32 / chunks per row group) (launcher)
  void *out;
  void *index;  // scratch: 8 bytes per output pixel (chan_index_bytes)
  uint32_t out_w, out_h, lines, first_line, line_step;
  const float *rd_cm, *rd_gm, *wr_cm;
  LutView rd, wr;
  // planar sources: the chroma planes of op k and, where the source has a Loader matrix of its own (8-bit code ranges), that
  // matrix (12 floats, device; NULL = rd_cm) - read by the planar instantiation of the kernel only
  const void *plane_u[kMaxChanOps], *plane_v[kMaxChanOps];
  const float *cm_op[kMaxChanOps];
  uint32_t planar;  // which instantiation the launch needs: 0 v210 / images on whole 48-pixel blocks, 1 v210 lines with tails, 2 planar / RGB sources
  // the packed frame the writer makes: 0 v210 (out), 1 yuv422p10 / 2 yuv422p8 (out = the Y plane, out_u, out_v; out_pitch = luma
  // samples per line), 5 rgba8 / 6 bgra8 (out; out_pitch = pixels per line) - PH_FMT_* numbering
  uint32_t out_fmt, out_pitch;
  void *out_u, *out_v;
  // v210 frames of any even width (1280: src/config.ts:43-54): quad slots per line by pitch, and the first column of the line's
  // tail (v210.ts:166-193; 0xFFFFFFFF when the width is a multiple of 6 or the frame is not v210)
  uint32_t out_qpitch, out_tail_from;
  // tap sharing (launcher): per sharing op and wave step of a workgroup, the converted LEFT column of the step's first lane
  // (3 rows x rgb = 36 bytes), made by a pass in front of phase 1 and kept in the LDS behind the table
  uint32_t halo_off, halo_steps;  // byte offset in the LDS; steps per op the area holds (0: no sharing in this launch)
  uint32_t any_cm;                // launcher: some op brings a Loader matrix of its own (cm_op): the whole launch takes the general dot products
  uint32_t images_only;           // launcher: every source is an f32 image (de-interlaced fields): nothing is looked up in the reader's table, it is not loaded
};

// Several consumers' frames of ONE composition in one launch (ph_chan_compose_multi): c describes the composition - the lines composed
// are the union of what the outputs need, c.out* / c.wr* are unused - and every output brings its format, planes and writer recipe.
// The launcher expects the outputs grouped by writer table.
constexpr int kMaxChanOuts = 4;
struct ChanOut {
  uint32_t fmt;    // PH_FMT_* (one of fmt_chan_out)
  uint32_t pitch;  // v210: quad slots per line; planar: luma samples per line; rgba8 / bgra8: pixels per line
  void *plane[3];
  uint32_t tail_from;  // v210: the first column of the line's tail (0xFFFFFFFF: none), as ChanArgs::out_tail_from
  uint32_t takes;      // which of the composed lines are this output's: 0 all, 1 the even frame lines, 2 the odd ones
  uint32_t line_end;   // lines from here on are not this output's (a field of a frame with an odd height)
  uint32_t field;      // 1: a field write (4:2:0: the written line of a pair gives the chroma)
  uint32_t round;      // 1: not v210, in a launch whose v210 output has a tail: tail pixels are parked truncated, with the rounding beside them
  const float *wr_cm;
  LutView wr;
};
struct ChanMultiArgs {
  ChanArgs c;
  uint32_t n_out;
  ChanOut out[kMaxChanOuts];
};
static_assert(sizeof(ChanMultiArgs) < 4096, "kernel arguments are limited to 4 KiB");

// Several channels' frames of ONE geometry and colour recipe in one launch (ph_chan_compose_batch) - what the reference runs: four
// channels of <= 1080p in one context through one queue (src/index.ts:45-71,156-160, clJobQueue.ts:114-141).  A workgroup takes its
// share of EVERY job, so the tables are loaded once and the wave steps of all jobs together are dealt to the waves in front of one
// barrier (ph_kernels_chan.hip).  Any source kind (round 6: planar / packed-RGB ones in an instantiation of their own), v210 out.
constexpr int kMaxChanJobs = 8;
constexpr int kMaxChanBatchOps = 40;  // the ops of all jobs of a launch (the argument block has to stay below 4 KiB)
struct ChanJob {
  void *out, *index;  // the v210 frame; this job's index frame (chan_index_bytes each)
  uint32_t first_op, n_ops, first_line, pad;
};
struct ChanBatchArgs {
  ChanOp op[kMaxChanBatchOps];
  ChanJob job[kMaxChanJobs];
  uint8_t op_job[kMaxChanBatchOps];  // the job an op belongs to (for the launcher)
  uint32_t share_op[8];              // launcher: the ops that share taps (ChanHalo), by halo table: op | its job << 8 | the job's first line << 16
  uint32_t jobs, n_ops, n_share;
  uint32_t magic_cpr, magic_cpg;     // as ChanArgs
  uint32_t steps;                    // wave steps per job of the workgroups that have the most chunks (launcher)
  uint32_t magic_spj, magic_qpj;     // ceil(2^32 / steps), ceil(2^32 / quads per job and workgroup = 64 * steps / 3)
  uint32_t out_w, out_h, lines, line_step;
  const float *rd_cm, *rd_gm, *wr_cm;
  LutView rd, wr;
  uint32_t tails;  // 1: lines may end in a tail (the TAILS instantiation)
  uint32_t out_qpitch, out_tail_from;
  uint32_t job_rot[kMaxChanJobs][4];  // per job and XCD (two 16-bit values per word): how far the job's share is rotated round the XCD's workgroups
  uint32_t sched_off;              // LDS byte offset of the jobs' tables behind the gamma table
  uint32_t halo_off, halo_steps;   // as ChanArgs; halo_steps = steps
  uint32_t images_only;            // as ChanArgs: every source of every job is an f32 image - the reader's table is not loaded
  // round 6: jobs with planar / packed-RGB sources (file playback with insets, graphics over clips) share launches too - the PLANAR
  // instantiation.  An op's chroma planes, and its Loader matrix as an index into a small table (0: the call's rd_cm; the argument
  // block has 4 KiB: forty pointers more would not fit)
  const void *plane_u[kMaxChanBatchOps], *plane_v[kMaxChanBatchOps];
  const float *cm_tab[8];
  uint8_t cm_idx[kMaxChanBatchOps];
  uint32_t planar;                 // 1: some op has a planar / packed-RGB source (launcher: the PLANAR instantiation)
  uint32_t any_cm;                 // some op brings a Loader matrix of its own: the general dot products throughout (as ChanArgs)
};
static_assert(sizeof(ChanBatchArgs) <= 4096, "kernel arguments are limited to 4 KiB");
// refuses (hipErrorInvalidValue) more than kMaxChanJobs jobs / kMaxChanBatchOps ops: callers split
// Route trace (ph_trace_begin / ph_trace_end, ph_api.cpp): while the calling thread traces, every launch is noted by name; returns
// true when the launch must NOT be made (a dry run).  `name` may be a launcher call's text ("ph::launch_xxx(...": noted as "xxx").
bool trace_launch(const char *name);
hipError_t launch_chan_compose_batch(hipStream_t s, const ChanBatchArgs &a, uint32_t num_cus);

// Several channels' frames for ANY consumer format, several consumers per channel, in one launch (ph_chan_compose_batch_out): the batch
// kernel's halo pass and phase 1 - the fields they read have ChanBatchArgs' names - and then the writer's phase per output on its job's
// index frame, as the several-outputs kernel runs it.  ChanBatchArgs has no room for output descriptors, so ops are traded for outputs:
// the reference's four channels, 24 ops, 8 outputs in all.  ONE writer table per launch (wr); an output brings its own writer matrix.
// All jobs of a launch compose the same lines (lines, line_step; a job's first_line is its own): a job's lines are the union of what
// its outputs want, as in ChanMultiArgs.
constexpr int kMaxChanOutJobs = 4;
constexpr int kMaxChanOutOps = 24;
constexpr int kMaxChanBatchOuts = 8;
struct ChanBatchOut {  // ChanOut without the table, with the job it belongs to
  uint32_t fmt, pitch;
  void *plane[3];
  uint32_t tail_from, takes, line_end, field, round;
  uint32_t job;
  const float *wr_cm;
};
static_assert(sizeof(ChanBatchOut) == 64, "an output descriptor is one 64-byte scalar load");
struct ChanBatchOutArgs {
  ChanOp op[kMaxChanOutOps];
  ChanJob job[kMaxChanOutJobs];  // (out is unused: the outputs name their planes)
  ChanBatchOut out[kMaxChanBatchOuts];  // grouped by job, in the jobs' order
  uint8_t op_job[kMaxChanOutOps];
  uint32_t share_op[8];
  uint32_t jobs, n_ops, n_share, n_out;
  uint32_t magic_cpr, magic_cpg;
  uint32_t steps;
  uint32_t magic_spj;
  uint32_t out_w, out_h, lines, line_step;
  const float *rd_cm, *rd_gm;
  LutView rd, wr;
  uint32_t tails;
  uint32_t out_tail_from;  // the first column of a v210 output's line tail (0xFFFFFFFF: no v210 output, or no tail): phase 1 parks those pixels truncated
  uint32_t job_rot[kMaxChanOutJobs][4];
  uint32_t sched_off;
  uint32_t halo_off, halo_steps;
  uint32_t images_only;
  const void *plane_u[kMaxChanOutOps], *plane_v[kMaxChanOutOps];
  const float *cm_tab[8];
  uint8_t cm_idx[kMaxChanOutOps];
  uint32_t planar;
  uint32_t any_cm;
};
static_assert(sizeof(ChanBatchOutArgs) <= 4096, "kernel arguments are limited to 4 KiB");
// refuses (hipErrorInvalidValue) more jobs, ops or outputs than the struct holds: callers split
hipError_t launch_chan_compose_batch_out(hipStream_t s, const ChanBatchOutArgs &a, uint32_t num_cus);

// ph_kernels_up.hip: the 2 x 2-block compositor for magnifying placements
struct UpLayer {
  const void *ptr;       // f32 RGBA (16 bytes per texel) or packed f32 RGB (12)
  uint32_t w, h, pitch;  // texels, texels, bytes per row
  uint32_t pad;
  float m[6];            // rows 0 and 1 of the 3x3 transform matrix
};
constexpr int kMaxUpJobs = 4;
struct UpArgs {
  UpLayer layer[kMaxLayers];
  int n;
  void *out;
  uint32_t out_w, out_h, lines, first_line, line_step;
  const float *wr_cm;
  LutView wr;
  uint32_t magic_upr, magic_upg;  // launcher
  uint32_t shared;                // launcher: all layers have one size and one placement
  // launcher: lines by pitch - quad slots per line; the columns the wave steps cover (out_w, or the whole pitch when lines end in a
  // tail quad and cleared slots: the TAILS instantiation writes those too)
  uint32_t out_qpitch, cover_w;
  // more jobs of the same shape in the same launch (both fields of a frame; several channels under one placement): their layers' data and
  // their outputs; jobs = 1 .. kMaxUpJobs
  const void *more_ptr[kMaxUpJobs - 1][kMaxLayers];
  void *more_out[kMaxUpJobs - 1];
  uint32_t jobs;
};
// Clips straight from their wire formats: reader and 2 x 2-block compositor in ONE launch (clip_up_write_v210_kernel).  A workgroup owns a
// tile of the output; with the reader's table resident it converts the source pixels its tile's taps fall on - once each - into a
// scratch rectangle of its own (packed f32 RGB, or RGBA when a source carries alpha; it stays in the XCD's L2), swaps the writer's
// table in and composes from there.
struct ClipSrc {
  const void *p0, *p1, *p2;  // the planes (v210 / packed RGB: p0)
  const float *cm;           // the source's YCbCr -> RGB matrix (device, 12 floats; unused for packed RGB)
  uint32_t fmt;              // PH_FMT_*
  uint32_t pitch;            // line pitch in luma samples / pixels; v210: in 16-byte quads
};
struct ClipUpArgs {
  UpArgs up;                 // layer[l].w / h / m: the clip's size and placement (ptr / pitch are the kernel's: the scratch rectangle)
  ClipSrc src[kMaxLayers];
  const float *rd_gm;
  LutView rd;
  char *scratch;             // grid * wg_bytes
  uint32_t wg_bytes;
  uint32_t rect_off[kMaxLayers], rect_cap[kMaxLayers];  // a layer's rectangle inside the workgroup's scratch: offset, bytes reserved
  uint32_t tcu, trp, gx;     // a tile: wave-step columns x row pairs; tiles per row of tiles
  // several frames of ONE shape in one launch (up.jobs = 2 .. kMaxUpJobs; single-layer frames only: several channels' file playback):
  // job j's clip is src[j] (layer[0] has the shape of all), its frame up.out / up.more_out[j - 1]; gy: rows of tiles per job
  uint32_t gy;
  uint32_t info_off;         // LDS offset of the per-layer rectangle descriptors (behind the larger table)
};
// picks the tiling and fills rect_off / rect_cap / wg_bytes / tcu / trp / gx / info_off; returns the number of workgroups (0: not for this kernel)
// (v210_tails == false: for clip_up_multi_kernel, which writes no v210 line tails - its wave steps cover the frame's columns, not the pitch)
uint32_t clip_up_plan(ClipUpArgs &a, bool rgb12, uint32_t num_cus, bool v210_tails = true);
hipError_t launch_clip_up_write_v210(hipStream_t s, const ClipUpArgs &a, bool rgb12, uint32_t grid);
bool compose_up_eligible(const UpArgs &a);
hipError_t launch_compose_up_write_v210(hipStream_t s, const UpArgs &a, bool rgb12, uint32_t num_cus);
// Several consumers' frames of ONE enlarged composition in one launch (ph_compose_up_write_multi): up describes the composition - the
// lines composed are the union of what the outputs need, up.out / up.more_out / up.wr_cm are unused, up.wr is the ONE writer table of
// the launch - and every output brings its format, its planes per job and its writer matrix.  A v210 output's lines end on a 48-pixel
// block here (the caller sends a v210 frame with a tail through launch_compose_up_write_v210).
// The bound on jobs x outputs is the argument block's: kMaxUpJobs x kMaxUpOuts x 3 plane pointers are 384 of its 4096 bytes.
constexpr int kMaxUpOuts = 4;
struct UpOut {
  uint32_t fmt;       // PH_FMT_* (one of fmt_chan_out)
  uint32_t pitch;     // v210: quad slots per line; planar: luma samples per line; rgba8 / bgra8: pixels per line
  uint32_t takes;     // which of the composed lines are this output's: 0 all, 1 the even frame lines, 2 the odd ones
  uint32_t line_end;  // lines from here on are not this output's (a field of a frame with an odd height)
  uint32_t field;     // 1: a field write (4:2:0: the written line of a pair gives the chroma)
  uint32_t pad;
  const float *wr_cm;  // (unused for rgba8 / bgra8)
  void *plane[kMaxUpJobs][3];
};
struct UpMultiArgs {
  UpArgs up;
  uint32_t n_out;
  UpOut out[kMaxUpOuts];
};
static_assert(sizeof(UpMultiArgs) < 4096, "kernel arguments are limited to 4 KiB");
// v210_tails (context option "up_v210_tails"): a v210 output whose lines end in a tail quad stays in the launch - compose_up_multi_t<..>
hipError_t launch_compose_up_multi(hipStream_t s, const UpMultiArgs &m, bool rgb12, uint32_t num_cus, bool v210_tails = false);
// Clips straight from their wire formats for ANY consumer, up to kMaxUpOuts per launch (ph_clip_compose_multi, clip_up_multi_kernel):
// clip describes the composition as for clip_up_write_v210_kernel - clip.up.out / more_out / wr_cm are unused, clip.up.wr is the ONE
// writer table of the launch - and every output brings its format, its planes per job and its writer matrix, as in UpMultiArgs.  A v210
// output's lines end on a 48-pixel block.  clip.up.jobs = 2 .. kMaxUpJobs (ph_clip_compose_batch_out): single-layer frames of one shape,
// job j's clip in clip.src[j] and its planes in out[k].plane[j], as ClipUpArgs says for the v210 kernel.
struct ClipUpMultiArgs {
  ClipUpArgs clip;
  uint32_t n_out;
  UpOut out[kMaxUpOuts];
};
static_assert(sizeof(ClipUpMultiArgs) < 4096, "kernel arguments are limited to 4 KiB");
// grid: clip_up_plan(clip, rgb12, num_cus, false); named clip_up_multi<rgb|rgba>x<outputs> in a route trace, with several jobs
// clip_up_multi<rgb|rgba>x<outputs>j<jobs>
// v210_tails (context option "up_v210_tails"): a v210 output whose lines end in a tail quad stays in the launch - grid is then
// clip_up_plan(clip, rgb12, num_cus, true), the name clip_up_multi_t<..>
hipError_t launch_clip_up_multi(hipStream_t s, const ClipUpMultiArgs &m, bool rgb12, uint32_t grid, bool v210_tails = false);
// ONE wire-format clip in a TRANSITION for any consumer (ph_clip_compose_transition_multi, clip_up_trans_kernel): a playlist's MIX or WIPE
// from one file to the next.  multi is the frame as for clip_up_multi_kernel with a single layer and a single job - multi.clip.up.layer[0]
// and multi.clip.src[0] are the layer's `src` - and the transition brings the incoming clip (dissolve, wipe) and the mask clip (wipe), each
// with a size and a placement of its own.  A workgroup converts up to three rectangles per tile: slot 0 src, slot 1 incoming, slot 2 mask;
// multi.clip.rect_off / rect_cap are indexed by slot.
struct ClipUpTransArgs {
  ClipUpMultiArgs multi;
  UpLayer partner[2];        // [0: incoming, 1: mask]: size and placement (ptr / pitch are the kernel's)
  ClipSrc partner_src[2];
  uint32_t kind;             // PH_TRANSITION_DISSOLVE or PH_TRANSITION_WIPE
  uint32_t same;             // bit 0: the incoming clip has the layer's size and placement, bit 1: the mask has
  float mix;                 // dissolve
};
static_assert(sizeof(ClipUpTransArgs) < 4096, "kernel arguments are limited to 4 KiB");
// plans the launch as a clip of three "layers" (clip_up_plan: tiling, a rectangle bound per slot from that image's own size and placement);
// returns the number of workgroups (0: not for this kernel)
uint32_t clip_up_trans_plan(ClipUpTransArgs &t, bool rgb12, uint32_t num_cus);
// named clip_up_trans<rgb|rgba>x<outputs> in a route trace.  Refuses what launch_clip_up_multi refuses, several jobs or layers, and a cut
hipError_t launch_clip_up_trans(hipStream_t s, const ClipUpTransArgs &t, bool rgb12, uint32_t grid);
// The same with layers in a transition (ph_compose_up_transition_multi, compose_up_trans_kernel): a layer may bring an incoming image
// (dissolve, wipe) and a mask (wipe), each with a size and a placement of its own.  multi.up.layer[l] is the layer's `src`; job j > 0
// differs in the images' data, the outputs' planes and the mix values.  multi.up.shared is not used: geometry is per layer, and a
// partner shares its layer's only where `same` says it has the layer's size and placement.
// Every field is sized for kMaxUpJobs jobs and kMaxLayers layers: 2.6 of the argument block's 4 KiB, so the bound on jobs stays kMaxUpJobs.
struct UpTransArgs {
  UpMultiArgs multi;
  UpLayer partner[kMaxLayers][2];                            // [layer][0: incoming, 1: mask]; ptr: job 0's
  const void *more_partner[kMaxUpJobs - 1][kMaxLayers][2];   // the further jobs' partner images
  float mix[kMaxUpJobs][kMaxLayers];                         // dissolve: per job (the two fields of a tick pass the Transitioner one after the other)
  uint32_t kind[kMaxLayers];                                 // PH_TRANSITION_*
  uint32_t same[kMaxLayers];                                 // bit 0: the incoming image has the layer's size and placement, bit 1: the mask has
};
static_assert(sizeof(UpTransArgs) < 4096, "kernel arguments are limited to 4 KiB: kMaxUpJobs jobs of kMaxLayers layers with two partners each must fit");
hipError_t launch_compose_up_trans(hipStream_t s, const UpTransArgs &t, bool rgb12, uint32_t num_cus);
// A ROUTED channel's file playback (ph_clip_compose_route_multi): the frames as above and the COMBINED IMAGE itself - f32 RGBA, out_w x
// out_h, rows unpadded - which another channel takes as a layer.  The whole frame is composed (up.first_line 0, line_step 1, lines out_h);
// the block's four pixels are made as values with their filtered alpha (ph_combine's arithmetic, alpha included) and stored before the
// writers' table reads.  n_out may be 0: the image alone, no writer table loaded (up.wr is not looked at).  One job.
struct ClipUpRouteArgs {  // clip_up_route_kernel: ONE clip in its wire format, one launch
  ClipUpMultiArgs multi;
  void *image;
  uint32_t nt;            // launcher: the image's store policy (image_nt)
};
static_assert(sizeof(ClipUpRouteArgs) < 4096, "kernel arguments are limited to 4 KiB");
// grid: clip_up_plan(multi.clip, rgb12, num_cus, false); named clip_up_route<rgb|rgba>x<outputs> in a route trace
hipError_t launch_clip_up_route(hipStream_t s, const ClipUpRouteArgs &r, bool rgb12, uint32_t grid);
struct UpRouteArgs {  // compose_up_route_kernel: f32 RGBA images (the readers' scratch images, routed images), any number of layers
  UpMultiArgs multi;
  void *image;
  uint32_t nt;
};
static_assert(sizeof(UpRouteArgs) < 4096, "kernel arguments are limited to 4 KiB");
// named compose_up_route<rgba>x<outputs>j1 in a route trace
hipError_t launch_compose_up_route(hipStream_t s, const UpRouteArgs &r, uint32_t num_cus);

struct DeintArgs {  // ph_kernels_deint.hip
  const uint4 *prev[kMaxLayers], *cur[kMaxLayers], *next[kMaxLayers];  // v210 frames, width x height
  float4 *out0[kMaxLayers], *out1[kMaxLayers];                         // RGBA f32: yadif parity 0 / parity 1
  int n, skip;
  uint32_t width, height, quads_pitch;
  uint32_t rows_per_strip, strips, col_blocks, nt;  // filled in by the launcher; nt (image_nt) is the RGBA outputs' store policy only
  uint32_t rgb12;  // 1: the outputs are packed f32 RGB (12 bytes per pixel, the reader's alpha == 1 left out); always stored plainly, nt or not
  const float *cm, *gm;
  LutView lut;
  // the windows' PH_FMT_* (one the fused reader takes: fmt_deint); planar frames: prev / cur / next are the Y planes, these the
  // chroma planes (read by the planar instantiations only)
  uint32_t pack;
  const void *prev_u[kMaxLayers], *prev_v[kMaxLayers], *cur_u[kMaxLayers], *cur_v[kMaxLayers], *next_u[kMaxLayers], *next_v[kMaxLayers];
};

struct CombineArgs {
  const void *layers[kMaxLayers];
  void *out;
  size_t npx;
  uint32_t nt;  // filled in by the launcher
};

hipError_t launch_v210_read(hipStream_t s, const void *in, void *out, uint32_t width, uint32_t height,
                            const void *cm, const void *lut, const void *gm);
hipError_t launch_v210_write(hipStream_t s, const void *in, void *out, uint32_t width, uint32_t height,
                             uint32_t interlace, const void *cm, const void *lut);
hipError_t launch_fused_v210_combine(hipStream_t s, int n, const FusedArgs &a);
// LDS-LUT variants (ph_kernels_lds.hip): one 1024-lane workgroup per CU
hipError_t launch_fused_v210_combine_lds(hipStream_t s, int n, const FusedLdsArgs &a, uint32_t num_cus);
hipError_t launch_lds_base_probe(hipStream_t s, uint32_t *out_dev);  // writes the LDS address of g_lds (expected: 0)
hipError_t launch_v210_read_lds(hipStream_t s, const void *in, void *out, uint32_t width, uint32_t height,
                                const void *cm, const void *gm, const LutView &lut, uint32_t num_cus);
hipError_t launch_v210_read_lds_batch(hipStream_t s, int n, const void *const *ins, void *const *outs, uint32_t width,
                                      uint32_t height, const void *cm, const void *gm, const LutView &lut, uint32_t num_cus);
hipError_t launch_v210_write_lds(hipStream_t s, const void *in, void *out, uint32_t width, uint32_t height,
                                 uint32_t interlace, const void *cm, const LutView &lut, uint32_t num_cus);
// the other pack formats (ph_kernels_fmt.hip); lv == NULL selects the global-gather form
hipError_t launch_pack_read(hipStream_t s, int fmt, const void *const planes[3], void *out, uint32_t width,
                            uint32_t height, const void *cm, const void *table, const void *gm, const LutView *lv,
                            uint32_t num_cus);
hipError_t launch_pack_read_batch(hipStream_t s, int fmt, int n, const void *const (*planes)[3], void *const *outs, uint32_t width, uint32_t height,
                                  const void *cm, const void *gm, const LutView &lv, uint32_t num_cus);
hipError_t launch_pack_write(hipStream_t s, int fmt, const void *in, void *const planes[3], uint32_t width,
                             uint32_t height, uint32_t interlace, const void *cm, const void *table, const LutView *lv,
                             uint32_t num_cus);
// One f32 RGBA image packed for several consumers in one launch (ph_pack_write_multi; ph_kernels_fmt.hip): every pixel is loaded once and
// looked up once in the ONE writer table of the launch (wr, in its LDS form); every output brings its format - any PH_FMT_* - its planes
// and its writer matrix.  The launch reads the lines first_line + i * line_step, i < lines: the field every output wants, or the whole
// frame, of which a field output takes the lines of its parity.  A planar output needs width % 8 == 0, a v210 output width % 48 == 0
// (the caller sends the others through launch_pack_write / launch_v210_write_lds: their line tails round differently).
constexpr int kMaxPackOuts = 4;
struct PackOut {
  uint32_t fmt;       // PH_FMT_*
  uint32_t pitch;     // v210: quad slots per line; planar: luma samples per line; rgba8 / bgra8: pixels per line
  uint32_t takes;     // which of the launch's lines are this output's: 0 all, 1 the even frame lines, 2 the odd ones
  uint32_t line_end;  // lines from here on are not this output's (a field of an odd height; a 4:2:0 frame's unpaired last line)
  uint32_t field;     // 1: a field write (4:2:0: the written line of a pair gives the chroma; a frame write: the pair's upper line)
  uint32_t pad;
  const float *wr_cm;  // (unused for rgba8 / bgra8)
  void *plane[3];
  uint64_t pad2;
};
static_assert(sizeof(PackOut) == 64, "an output descriptor is one 64-byte scalar load");
struct PackMultiArgs {
  const void *in;  // width x height f32 RGBA
  uint32_t width, lines, first_line, line_step;
  uint32_t n_out;
  uint32_t units_per_line;  // launcher: a lane's work unit is an octet of pixels
  LutView wr;
  PackOut out[kMaxPackOuts];
};
// named "pack_write_multi x<outputs>" in a route trace
hipError_t launch_pack_write_multi(hipStream_t s, const PackMultiArgs &a, uint32_t num_cus);
hipError_t launch_compose_write_v210(hipStream_t s, const ComposeArgs &a, uint32_t num_cus);
size_t chan_index_bytes(uint32_t out_w, uint32_t lines);
hipError_t launch_chan_compose_v210(hipStream_t s, const ChanArgs &a, uint32_t num_cus);
hipError_t launch_chan_compose_multi(hipStream_t s, const ChanMultiArgs &a, uint32_t num_cus);
bool compose_can_wipe(const ComposeArgs &a);  // the buffer-addressed compositor serves this job (needed for wipe layers)
hipError_t launch_v210_yadif_pair(hipStream_t s, DeintArgs a, int tff, uint32_t num_cus);
hipError_t launch_yadif(hipStream_t s, const void *prev, const void *cur, const void *next, int w, int h, int parity,
                        int tff, int skip, void *out);
hipError_t launch_yadif_pair(hipStream_t s, const void *prev, const void *cur, const void *next, int w, int h, int tff,
                             int skip, void *out0, void *out1);
hipError_t launch_transform(hipStream_t s, const void *in, int iw, int ih, const void *m9, void *out, int ow, int oh);
hipError_t launch_resize(hipStream_t s, const void *in, int iw, int ih, float scale, float ox, float oy,
                         const void *flip4, void *out, int ow, int oh);
hipError_t launch_combine(hipStream_t s, int n, const CombineArgs &a);
hipError_t launch_dissolve(hipStream_t s, const void *in0, const void *in1, float mix, int w, int h, void *out);
hipError_t launch_twipe(hipStream_t s, const void *in0, const void *in1, const void *mask, int w, int h, void *out);
hipError_t launch_wipe(hipStream_t s, const void *in0, const void *in1, float wipe, int w, int h, void *out);
hipError_t launch_rgb_unpack(hipStream_t s, const void *packed, void *rgba, size_t npx);

}  // namespace ph
