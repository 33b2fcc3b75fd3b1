// ph_kernels_fused_field.hip - the plain-layer composite for up to four consumers (ph_kernels_fused_multi.hip), single frame and batch,
// for consumers that all take the SAME FIELD of the frame (1080i: SDI's v210, an interlaced encoder's planes): only that field's lines
// are read, combined and looked up - half the frame's work (context option "fused_fields"; ph_fused_v210_combine_multi and
// ph_fused_v210_combine_multi_batch).
//
// A translation unit of its own: ph_kernels_fused_multi.hip's, ph_kernels_fused_trans.hip's and ph_kernels_fused_route.hip's kernels are
// compiled from the text they always had (profiles/fused_field_resources.txt).
//
// The kernels are the shared body (ph_kernels_fused_multi_body.h, PH_FM_FIELD 1) counted in FIELD quads: a workgroup's contiguous range,
// the tiles of BS * P quads, the slices a wave skips and the tail lanes that recompute the range's last quad are all the field's.  A
// field quad's place in the frame (ph_fused_field.h: one division by reciprocal, a multiply, two adds) is made where a slice loads and
// again where it stores, so no register holds it between the phases.  Per quad the arithmetic, its order, the prefetch chain, the
// packed st[p][9], the table swap and the once-per-table phase 2 are the body's.
#include "ph_device.h"
#include "ph_fused_field.h"
#include "ph_kernels.h"
#include "ph_ldslut.h"

#include <cstdio>
#include <type_traits>

#pragma clang fp contract(off)

namespace ph {

namespace {

#include "ph_kernels_fused_out.h"

}  // namespace

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_field_multi_kernel(FusedFieldArgs args) {
  const FusedMultiArgs &a = args.m;
  const uint32_t first_line = args.first_line;
#define PH_FM_BATCH 0
#define PH_FM_TRANS 0
#define PH_FM_ROUTE 0
#define PH_FM_FIELD 1
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
#undef PH_FM_ROUTE
#undef PH_FM_FIELD
}

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_field_multi_batch_kernel(FusedFieldBatchArgs args) {
  const FusedMultiArgs &a = args.b.m;
  const uint32_t first_line = args.first_line;
#define PH_FM_BATCH 1
#define PH_FM_TRANS 0
#define PH_FM_ROUTE 0
#define PH_FM_FIELD 1
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
#undef PH_FM_ROUTE
#undef PH_FM_FIELD
}

template <int N>
static hipError_t launch_fused_field_n(hipStream_t s, const FusedFieldArgs &a, uint32_t grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_field_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_field_multi_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

// the field's last quad lies in front of frame quad 2 * total_quads: the plan's bound on the field (total_quads * quads_per_line < 2^32,
// the division by reciprocal) is asked of twice as much, for the frame's flat quad the kernel makes of it
static bool field_frame_fits(const FusedMultiArgs &m) { return 2ull * m.total_quads * m.quads_per_line < (1ull << 32); }

hipError_t launch_fused_v210_field_multi(hipStream_t s, int n, const FusedFieldArgs &a, uint32_t interlace, uint32_t num_cus, uint32_t max_wgs) {
  static_assert(offsetof(FusedFieldArgs, m) == 0, "the kernel reads the whole-frame kernel's arguments at the start of its own");
  if (!a.m.total_quads) return hipSuccess;
  if ((interlace != 1 && interlace != 3) || a.first_line != (interlace == 3 ? 1u : 0u) || !field_frame_fits(a.m)) return hipErrorInvalidValue;
  FusedFieldArgs b = a;
  uint32_t grid, lds;
  const hipError_t e = fused_multi_plan(a.m, num_cus, max_wgs, b.m, grid, lds);  // (total_quads is the field's: so are the slices)
  if (e != hipSuccess) return e;
  for (uint32_t k = 0; k < a.m.n_out; ++k)
    if (a.m.out[k].takes) return hipErrorInvalidValue;  // every line composed is every output's
  char name[48];
  snprintf(name, sizeof name, "fused_v210_field_multi x%uf%u", a.m.n_out, interlace);
  if (trace_launch(name)) return hipSuccess;
  switch (n) {
    case 1: return launch_fused_field_n<1>(s, b, grid, lds);
    case 2: return launch_fused_field_n<2>(s, b, grid, lds);
    case 3: return launch_fused_field_n<3>(s, b, grid, lds);
    case 4: return launch_fused_field_n<4>(s, b, grid, lds);
    case 5: return launch_fused_field_n<5>(s, b, grid, lds);
    case 6: return launch_fused_field_n<6>(s, b, grid, lds);
    case 7: return launch_fused_field_n<7>(s, b, grid, lds);
    case 8: return launch_fused_field_n<8>(s, b, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

template <int N>
static hipError_t launch_fused_field_batch_n(hipStream_t s, const FusedFieldBatchArgs &a, dim3 grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_field_multi_batch_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_field_multi_batch_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_fused_v210_field_multi_batch(hipStream_t s, int n, uint32_t jobs, const FusedFieldBatchArgs &a, uint32_t interlace, uint32_t num_cus, uint32_t max_wgs) {
  static_assert(sizeof(FusedFieldBatchArgs) <= 4096, "the argument block of a batched launch stays within 4 KiB");
  static_assert(offsetof(FusedFieldBatchArgs, b) == 0 && offsetof(FusedMultiBatchArgs, m) == 0, "the kernel reads the whole-frame kernel's arguments at the start of its own");
  const FusedMultiArgs &m = a.b.m;
  if (!m.total_quads) return hipSuccess;
  if (jobs < 2 || jobs > (uint32_t)kMaxBatch || n < 1 || n > kMaxLayers) return hipErrorInvalidValue;
  if ((interlace != 1 && interlace != 3) || a.first_line != (interlace == 3 ? 1u : 0u) || !field_frame_fits(m)) return hipErrorInvalidValue;
  FusedFieldBatchArgs b = a;
  // the plan's checks and fields; its grid for a job's share of the CUs: max(1, num_cus / jobs) workgroups, never more than the field's
  // slices or the caller's cap
  uint32_t wg_per_job, lds;
  const hipError_t e = fused_multi_plan(m, num_cus / jobs ? num_cus / jobs : 1, max_wgs, b.b.m, wg_per_job, lds);
  if (e != hipSuccess) return e;
  for (uint32_t k = 0; k < m.n_out; ++k)
    if (m.out[k].takes) return hipErrorInvalidValue;
  for (uint32_t j = 0; j < jobs; ++j) {  // every pointer the kernel will follow is there
    for (int l = 0; l < n; ++l)
      if (!a.b.layers[j][l]) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < m.n_out; ++k)
      for (int p = 0; p < fmt_planes((int)m.out[k].fmt); ++p)
        if (!a.b.plane[j][k][p]) return hipErrorInvalidValue;
  }
  char name[56];
  snprintf(name, sizeof name, "fused_v210_field_multi x%uj%uf%u", m.n_out, jobs, interlace);
  if (trace_launch(name)) return hipSuccess;
  const dim3 grid(wg_per_job, jobs);
  switch (n) {
    case 1: return launch_fused_field_batch_n<1>(s, b, grid, lds);
    case 2: return launch_fused_field_batch_n<2>(s, b, grid, lds);
    case 3: return launch_fused_field_batch_n<3>(s, b, grid, lds);
    case 4: return launch_fused_field_batch_n<4>(s, b, grid, lds);
    case 5: return launch_fused_field_batch_n<5>(s, b, grid, lds);
    case 6: return launch_fused_field_batch_n<6>(s, b, grid, lds);
    case 7: return launch_fused_field_batch_n<7>(s, b, grid, lds);
    case 8: return launch_fused_field_batch_n<8>(s, b, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ph
