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

// the wave-priority ladder (PH_FM_BALANCE) and one output's share of one quad (fused_out_store): shared with ph_kernels_fused_trans.hip
#include "ph_kernels_fused_out.h"

}  // namespace

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_combine_multi_kernel(FusedMultiArgs a) {
#define PH_FM_BATCH 0
#define PH_FM_TRANS 0
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
}

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_combine_multi_batch_kernel(FusedMultiBatchArgs args) {
  const FusedMultiArgs &a = args.m;
#define PH_FM_BATCH 1
#define PH_FM_TRANS 0
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
}

template <int N>
static hipError_t launch_fused_multi_n(hipStream_t s, const FusedMultiArgs &a, uint32_t grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_combine_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_combine_multi_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

// what a single frame's launch needs beside its kernel - the checks, the launcher's own fields of the arguments (b), the LDS bytes and the
// grid: shared with launch_fused_v210_trans_multi (ph_kernels_fused_trans.hip)
hipError_t fused_multi_plan(const FusedMultiArgs &a, uint32_t num_cus, uint32_t max_wgs, FusedMultiArgs &b, uint32_t &grid, uint32_t &lds) {
  if (a.n_out < 1 || a.n_out > (uint32_t)kMaxFusedOuts || !a.quads_per_line || a.quads_per_line % 8u || a.total_quads % a.quads_per_line) return hipErrorInvalidValue;
  if ((uint64_t)a.total_quads * a.quads_per_line >= (1ull << 32)) return hipErrorInvalidValue;  // the line by reciprocal
  lds = a.rd.bytes;
  for (uint32_t k = 0; k < a.n_out; ++k) {
    if (!fmt_chan_out((int)a.out[k].fmt) || !a.out[k].wr.bytes) return hipErrorInvalidValue;
    lds = a.out[k].wr.bytes > lds ? a.out[k].wr.bytes : lds;
  }
  b = a;
  b.magic_qpl = (uint32_t)(((1ull << 32) + a.quads_per_line - 1) / a.quads_per_line);
  b.need_line = 0;
  for (uint32_t k = 0; k < b.n_out; ++k) {
    b.need_line |= (b.out[k].takes || fmt_v420((int)b.out[k].fmt)) ? 1u : 0u;
    b.out[k].half_pitch = 3u * a.quads_per_line;  // chroma samples (nv12: CbCr pairs) per chroma row: half the width
  }
  // one workgroup per CU, never more than slices (as the shipped kernel's launcher), capped by the caller
  const uint32_t slices = (a.total_quads + kLdsBlock - 1) / kLdsBlock;
  grid = num_cus ? num_cus : 1;
  if (grid > slices) grid = slices;
  if (max_wgs && grid > max_wgs) grid = max_wgs;
  return hipSuccess;
}

hipError_t launch_fused_v210_combine_multi(hipStream_t s, int n, const FusedMultiArgs &a, uint32_t num_cus, uint32_t max_wgs) {
  if (!a.total_quads) return hipSuccess;
  FusedMultiArgs b;
  uint32_t grid, lds;
  const hipError_t e = fused_multi_plan(a, num_cus, max_wgs, b, grid, lds);
  if (e != hipSuccess) return e;
  char name[40];
  snprintf(name, sizeof name, "fused_v210_combine_multi x%u", a.n_out);
  if (trace_launch(name)) return hipSuccess;
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
