// ph_kernels_fused_multi.hip - the headline kernel ([v210 read] x N -> combine_N -> write, ph_kernels_lds.hip
// fused_v210_combine_lds_kernel) with up to four consumers' frames per launch, any format the channel kernel writes.
//
// A translation unit of its own: the shipped kernel's instantiations are compiled from the text they always had.
//
// Phase 1 is the shipped kernel's non-TAIL form with P = 6, operation for operation: the prefetch chain through layers and
// slices, the rolled layer loop, the three-operand v_fma_f32 combine, lds_lut_index_unit and the packed, pinned st[p][9].
// Between the phases a quad is its 18 writer-table indices in registers; they stay there while phase 2 runs once per
// distinct writer table of the launch: barrier, table load, barrier, then per slice the 18 indices are expanded, the 18
// table reads are made ONCE, and every output of that table packs the same 18 values with its own writer matrix.
//
// Two kernels of one body (ph_kernels_fused_multi_body.h): a single frame's, and the batched launch's - several channels' frames for
// the same list of consumers side by side, each workgroup on one job's layers and planes (ph_fused_v210_combine_multi_batch).
#include "ph_device.h"
#include "ph_kernels.h"
#include "ph_ldslut.h"

#include <cstdio>
#include <type_traits>

#pragma clang fp contract(off)

namespace ph {

namespace {

// as ph_kernels_lds.hip PH_BALANCE: a wave lowers its priority as it advances through its slices, so the waves of a SIMD
// reach the phase barrier together (s_setprio takes an immediate: the switch folds once the slice loop is unrolled)
__device__ __forceinline__ void fm_set_wave_priority(int level) {
  switch (level) {
    case 3: __builtin_amdgcn_s_setprio(3); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(0); break;
  }
}
#define PH_FM_BALANCE(p) fm_set_wave_priority(3 - ((p) * 4) / P)

typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_stream8(uint2 *p, const uint2 v) {
#if PH_NT_STORE
  __builtin_nontemporal_store(ph_u2v{v.x, v.y}, reinterpret_cast<ph_u2v *>(p));
#else
  *p = v;
#endif
}

// One output's share of one quad: the six pixels' table values g[3 j + c] packed with the output's own writer matrix and stored.
// f: the flat quad index (width % 48 == 0: a line is a whole number of quads and of octets, a planar pitch is the width), so
// luma starts at sample 6 f, 4:2:2 chroma at 3 f, packed RGB at pixel 6 f, v210 at quad f.  line / g (the quad's line and its
// place in it) are computed by the caller, and only read, where the launch has a field or a 4:2:0 output.
// Everything about the output is uniform: scalar branches.  A lane's share of an 8-bit plane is 6 or 3 bytes at an offset that
// is only 2-byte (luma, nv12 chroma) or 1-byte (4:2:2 / 4:2:0 chroma) aligned: short and byte stores through the cache, which
// merges a wave's 384 / 192 contiguous bytes before they leave for memory.
// pl: the output's planes - its descriptor's own, or (a batched launch) those of the workgroup's job.
template <class O, class Pl>
__device__ __forceinline__ void fused_out_store(const O &o, const Pl pl, const float (&g)[18], uint32_t f, uint32_t line, uint32_t col) {
  // a field output: the lines of its parity, height / 2 of them (per lane: a wave may span lines)
  if (o.takes && ((line & 1u) + 1u != o.takes || line >= o.line_end)) return;
  if (fmt_rgb8((int)o.fmt)) {  // rgba8.ts:69-101, alpha 255
    // bgra8 is rgba8 with red and blue exchanged (uniform selects).  A pixel pair at a time, the pairs kept apart: eighteen bytes
    // being rounded at once want registers this kernel does not have
    const bool bgr = o.fmt == PH_FMT_BGRA8;
    uint2 *const dst = reinterpret_cast<uint2 *>(pl[0]) + (size_t)f * 3u;  // 24 bytes per quad: 8-byte pieces
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      uint32_t px[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = 3 * (2 * pr + j);
        px[j] = rgb8_pack<PH_FMT_RGBA8>(bgr ? g[c + 2] : g[c], g[c + 1], bgr ? g[c] : g[c + 2]);
      }
      store_stream8(dst + pr, make_uint2(px[0], px[1]));
      __builtin_amdgcn_sched_barrier(0);
    }
    return;
  }
  const WriteK wk = load_write_k(o.wr_cm);
  uint32_t y[6], u[3], v[3];
#pragma unroll
  for (int j = 0; j < 6; ++j) {  // chroma from the even pixel of a pair (v210.ts:159-162, yuv422p10.ts:140-189)
    y[j] = ycbcr_code(g[3 * j], g[3 * j + 1], g[3 * j + 2], wk.y);
    if ((j & 1) == 0) u[j >> 1] = ycbcr_code(g[3 * j], g[3 * j + 1], g[3 * j + 2], wk.u), v[j >> 1] = ycbcr_code(g[3 * j], g[3 * j + 1], g[3 * j + 2], wk.v);
  }
  if (o.fmt == PH_FMT_V210) {
    store_stream(reinterpret_cast<uint4 *>(pl[0]) + f, pack_quad(y, u, v));
    return;
  }
  if (o.fmt == PH_FMT_YUV422P10) {  // 16-bit samples: 12 bytes of luma (4-byte aligned), 6 + 6 of chroma (2-byte aligned)
    uint32_t *const py = reinterpret_cast<uint32_t *>(pl[0]) + (size_t)f * 3u;
    py[0] = (y[0] & 0xffffu) | y[1] << 16, py[1] = (y[2] & 0xffffu) | y[3] << 16, py[2] = (y[4] & 0xffffu) | y[5] << 16;
    uint16_t *const pu = reinterpret_cast<uint16_t *>(pl[1]) + (size_t)f * 3u;
    uint16_t *const pv = reinterpret_cast<uint16_t *>(pl[2]) + (size_t)f * 3u;
#pragma unroll
    for (int j = 0; j < 3; ++j) pu[j] = (uint16_t)u[j], pv[j] = (uint16_t)v[j];
    return;
  }
  // the 8-bit planar formats: uchar = (uchar)ushort keeps the low 8 bits (yuv422p8.ts:166-168)
  uint16_t *const py = reinterpret_cast<uint16_t *>(pl[0]) + (size_t)f * 3u;
#pragma unroll
  for (int j = 0; j < 3; ++j) py[j] = (uint16_t)((y[2 * j] & 0xffu) | (y[2 * j + 1] & 0xffu) << 8);
  size_t c = (size_t)f * 3u;  // 4:2:2: the chroma planes' pitch is half the width = 3 per quad
  if (fmt_v420((int)o.fmt)) {
    // 4:2:0 (yuv420p.ts:150-216, nv12.ts:139-196): chroma row line >> 1 from the pair's upper line - or from the one line of the
    // pair that a field writes
    if (!o.field && (line & 1u)) return;
    c = (size_t)(line >> 1) * (o.half_pitch) + 3u * col;
  }
  if (o.fmt == PH_FMT_NV12) {  // Cb, Cr interleaved: 6 bytes at a 2-byte aligned offset
    uint16_t *const pc = reinterpret_cast<uint16_t *>(pl[1]) + c;
#pragma unroll
    for (int j = 0; j < 3; ++j) pc[j] = (uint16_t)((u[j] & 0xffu) | (v[j] & 0xffu) << 8);
    return;
  }
  uint8_t *const pu = reinterpret_cast<uint8_t *>(pl[1]) + c, *const pv = reinterpret_cast<uint8_t *>(pl[2]) + c;
#pragma unroll
  for (int j = 0; j < 3; ++j) pu[j] = (uint8_t)u[j], pv[j] = (uint8_t)v[j];
}

}  // namespace

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_combine_multi_kernel(FusedMultiArgs a) {
#define PH_FM_BATCH 0
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
}

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_combine_multi_batch_kernel(FusedMultiBatchArgs args) {
  const FusedMultiArgs &a = args.m;
#define PH_FM_BATCH 1
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
}

template <int N>
static hipError_t launch_fused_multi_n(hipStream_t s, const FusedMultiArgs &a, uint32_t grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_combine_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_combine_multi_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_fused_v210_combine_multi(hipStream_t s, int n, const FusedMultiArgs &a, uint32_t num_cus, uint32_t max_wgs) {
  if (!a.total_quads) return hipSuccess;
  if (a.n_out < 1 || a.n_out > (uint32_t)kMaxFusedOuts || !a.quads_per_line || a.quads_per_line % 8u || a.total_quads % a.quads_per_line) return hipErrorInvalidValue;
  if ((uint64_t)a.total_quads * a.quads_per_line >= (1ull << 32)) return hipErrorInvalidValue;  // the line by reciprocal
  uint32_t lds = a.rd.bytes;
  for (uint32_t k = 0; k < a.n_out; ++k) {
    if (!fmt_chan_out((int)a.out[k].fmt) || !a.out[k].wr.bytes) return hipErrorInvalidValue;
    lds = a.out[k].wr.bytes > lds ? a.out[k].wr.bytes : lds;
  }
  char name[40];
  snprintf(name, sizeof name, "fused_v210_combine_multi x%u", a.n_out);
  if (trace_launch(name)) return hipSuccess;
  FusedMultiArgs b = a;
  b.magic_qpl = (uint32_t)(((1ull << 32) + a.quads_per_line - 1) / a.quads_per_line);
  b.need_line = 0;
  for (uint32_t k = 0; k < b.n_out; ++k) {
    b.need_line |= (b.out[k].takes || fmt_v420((int)b.out[k].fmt)) ? 1u : 0u;
    b.out[k].half_pitch = 3u * a.quads_per_line;  // chroma samples (nv12: CbCr pairs) per chroma row: half the width
  }
  // one workgroup per CU, never more than slices (as the shipped kernel's launcher), capped by the caller
  const uint32_t slices = (a.total_quads + kLdsBlock - 1) / kLdsBlock;
  uint32_t grid = num_cus ? num_cus : 1;
  if (grid > slices) grid = slices;
  if (max_wgs && grid > max_wgs) grid = max_wgs;
  switch (n) {
    case 1: return launch_fused_multi_n<1>(s, b, grid, lds);
    case 2: return launch_fused_multi_n<2>(s, b, grid, lds);
    case 3: return launch_fused_multi_n<3>(s, b, grid, lds);
    case 4: return launch_fused_multi_n<4>(s, b, grid, lds);
    case 5: return launch_fused_multi_n<5>(s, b, grid, lds);
    case 6: return launch_fused_multi_n<6>(s, b, grid, lds);
    case 7: return launch_fused_multi_n<7>(s, b, grid, lds);
    case 8: return launch_fused_multi_n<8>(s, b, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

template <int N>
static hipError_t launch_fused_multi_batch_n(hipStream_t s, const FusedMultiBatchArgs &a, dim3 grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_combine_multi_batch_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_combine_multi_batch_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_fused_v210_combine_multi_batch(hipStream_t s, int n, uint32_t jobs, const FusedMultiBatchArgs &a, uint32_t num_cus, uint32_t max_wgs) {
  static_assert(sizeof(FusedMultiBatchArgs) <= 4096, "the argument block of a batched launch stays within 4 KiB");
  const FusedMultiArgs &m = a.m;
  if (!m.total_quads) return hipSuccess;
  if (jobs < 2 || jobs > (uint32_t)kMaxBatch || n < 1 || n > kMaxLayers) return hipErrorInvalidValue;
  if (m.n_out < 1 || m.n_out > (uint32_t)kMaxFusedOuts || !m.quads_per_line || m.quads_per_line % 8u || m.total_quads % m.quads_per_line) return hipErrorInvalidValue;
  if ((uint64_t)m.total_quads * m.quads_per_line >= (1ull << 32)) return hipErrorInvalidValue;  // the line by reciprocal
  uint32_t lds = m.rd.bytes;
  for (uint32_t k = 0; k < m.n_out; ++k) {
    if (!fmt_chan_out((int)m.out[k].fmt) || !m.out[k].wr.bytes) return hipErrorInvalidValue;
    lds = m.out[k].wr.bytes > lds ? m.out[k].wr.bytes : lds;
  }
  for (uint32_t j = 0; j < jobs; ++j) {  // every pointer the kernel will follow is there
    for (int l = 0; l < n; ++l)
      if (!a.layers[j][l]) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < m.n_out; ++k)
      for (int p = 0; p < fmt_planes((int)m.out[k].fmt); ++p)
        if (!a.plane[j][k][p]) return hipErrorInvalidValue;
  }
  char name[48];
  snprintf(name, sizeof name, "fused_v210_combine_multi x%uj%u", m.n_out, jobs);
  if (trace_launch(name)) return hipSuccess;
  FusedMultiBatchArgs b = a;
  b.m.magic_qpl = (uint32_t)(((1ull << 32) + m.quads_per_line - 1) / m.quads_per_line);
  b.m.need_line = 0;
  for (uint32_t k = 0; k < m.n_out; ++k) {
    b.m.need_line |= (m.out[k].takes || fmt_v420((int)m.out[k].fmt)) ? 1u : 0u;
    b.m.out[k].half_pitch = 3u * m.quads_per_line;
  }
  // the CUs divided among the jobs (as the shipped kernel's batch): never more workgroups than a job has slices, the caller's cap per job
  const uint32_t slices = (m.total_quads + kLdsBlock - 1) / kLdsBlock;
  uint32_t wg_per_job = num_cus / jobs ? num_cus / jobs : 1;
  if (wg_per_job > slices) wg_per_job = slices;
  if (max_wgs && wg_per_job > max_wgs) wg_per_job = max_wgs;
  const dim3 grid(wg_per_job, jobs);
  switch (n) {
    case 1: return launch_fused_multi_batch_n<1>(s, b, grid, lds);
    case 2: return launch_fused_multi_batch_n<2>(s, b, grid, lds);
    case 3: return launch_fused_multi_batch_n<3>(s, b, grid, lds);
    case 4: return launch_fused_multi_batch_n<4>(s, b, grid, lds);
    case 5: return launch_fused_multi_batch_n<5>(s, b, grid, lds);
    case 6: return launch_fused_multi_batch_n<6>(s, b, grid, lds);
    case 7: return launch_fused_multi_batch_n<7>(s, b, grid, lds);
    case 8: return launch_fused_multi_batch_n<8>(s, b, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ph
