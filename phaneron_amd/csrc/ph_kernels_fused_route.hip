// ph_kernels_fused_route.hip - the plain-layer composite for up to four consumers (ph_kernels_fused_multi.hip) for a ROUTED channel: a
// layer may be a finished f32 RGBA image - another channel's combined frame - and the combined image is an output beside the consumers'
// packed frames: [v210 read | image] x N -> combine_N -> image_out, write x n_out (ph_fused_v210_route_multi).
//
// A translation unit of its own: ph_kernels_fused_multi.hip's and ph_kernels_fused_trans.hip's kernels are compiled from the text they
// always had (profiles/fused_route_resources.txt).
//
// The kernel is the single frame's body (ph_kernels_fused_multi_body.h, PH_FM_ROUTE 1): flat quad ranges and tiles, the one-deep
// prefetch of the v210 layers' words, the rolled layer loop, the packed st[p][9], the table swap and the once-per-table phase 2 with
// fused_out_store.  A layer's kind is uniform - a scalar load from the argument block - so an image layer branches out of the loop's
// plain path into fm_route_image_layer below and comes back for the next layer.
//
// What the image makes visible, the body's plain combine does not give: it starts from acc = 0 - fma(0, k, t) loses the bottom layer's
// -0 and is NaN under an image whose alpha is Inf - and it carries no alpha.  Here the combine is ph_combine's (combine_kernel,
// ph_kernels.hip; combine.ts:45-65): the bottom layer is ASSIGNED; above it k = 1 - l.a, rgb = fma(acc, k, l), a = fma(acc.a, 0, l.a).
// The alphas are six more accumulators, carried in the IMG instantiations only: v210 layers alone have alpha 1 throughout.
#include "ph_device.h"
#include "ph_kernels.h"
#include "ph_ldslut.h"

#include <cstdio>
#include <type_traits>

#pragma clang fp contract(off)

namespace ph {

namespace {

#include "ph_kernels_fused_out.h"

// one texel of an image layer combined into pixel J's accumulators
template <int J>
__device__ __forceinline__ void fm_route_px(float (&acc)[18], float (&al)[6], const float4 t, int l) {
  if (l == 0) {  // uniform: the bottom layer as it is - its -0, its alpha
    acc[3 * J] = t.x, acc[3 * J + 1] = t.y, acc[3 * J + 2] = t.z, al[J] = t.w;
    return;
  }
  const float kk = 1.0f - t.w;
  al[J] = fma_rn(al[J], 0.0f, t.w);  // a value of its own: NaN above a pixel whose alpha is Inf or NaN
  asm volatile("v_fma_f32 %0, %0, %3, %4\n\tv_fma_f32 %1, %1, %3, %5\n\tv_fma_f32 %2, %2, %3, %6"
               : "+v"(acc[3 * J]), "+v"(acc[3 * J + 1]), "+v"(acc[3 * J + 2])
               : "v"(kk), "v"(t.x), "v"(t.y), "v"(t.z));
}

// One image layer, for the quad f: its six texels are 96 contiguous bytes at (size_t)f * 96 - f < total_quads < 2^29 (the launcher's
// bound), so the 64-bit offset is right for every frame the launcher takes.  They are asked for here, with the streaming load, a pair
// at a time and the next pair in front of the first one's combine: they do not join the prefetch chain, which would keep their
// registers alive through the layer in front (fm_trans_layer, ph_kernels_fused_trans.hip, says the same of its partners), and all six
// at once are 24 registers this kernel does not have.  Tail lanes come with the last quad of the range in f, for this pointer too.
// A: 6 in the IMG instantiations; the others never get here (their call folds away).
template <int A>
__device__ __forceinline__ void fm_route_image_layer(float (&acc)[18], float (&al)[A], const void *layer, int l, uint32_t f) {
  if constexpr (A == 6) {
    const float4 *const p = reinterpret_cast<const float4 *>(layer) + (size_t)f * 6u;
    const float4 t0 = load_stream(p), t1 = load_stream(p + 1);
    const float4 t2 = load_stream(p + 2), t3 = load_stream(p + 3);
    __builtin_amdgcn_sched_barrier(0);
    fm_route_px<0>(acc, al, t0, l);
    fm_route_px<1>(acc, al, t1, l);
    const float4 t4 = load_stream(p + 4), t5 = load_stream(p + 5);
    __builtin_amdgcn_sched_barrier(0);
    fm_route_px<2>(acc, al, t2, l);
    fm_route_px<3>(acc, al, t3, l);
    __builtin_amdgcn_sched_barrier(0);
    fm_route_px<4>(acc, al, t4, l);
    fm_route_px<5>(acc, al, t5, l);
  }
}

}  // namespace

// slices per tile: the shared body's six; five with an image layer, whose six alphas and texels in flight stand beside the tile's
// packed indices - with six slices three to four vector registers spill (profiles/fused_route_resources.txt)
#define PH_FM_ROUTE_P (IMG ? 5 : 6)

template <int N, bool IMG>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_route_multi_kernel(FusedRouteArgs args) {
  const FusedMultiArgs &a = args.m;
#define PH_FM_BATCH 0
#define PH_FM_TRANS 0
#define PH_FM_ROUTE 1
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
#undef PH_FM_ROUTE
}

template <int N, bool IMG>
static hipError_t launch_fused_route_n(hipStream_t s, const FusedRouteArgs &a, uint32_t grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_route_multi_kernel<N, IMG>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_route_multi_kernel<N, IMG><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}
template <int N>
static hipError_t launch_fused_route_img(hipStream_t s, const FusedRouteArgs &a, bool img, uint32_t grid, uint32_t lds) {
  return img ? launch_fused_route_n<N, true>(s, a, grid, lds) : launch_fused_route_n<N, false>(s, a, grid, lds);
}

hipError_t launch_fused_v210_route_multi(hipStream_t s, int n, const FusedRouteArgs &a, uint32_t num_cus, uint32_t max_wgs) {
  static_assert(sizeof(FusedRouteArgs) <= 4096, "the argument block stays within 4 KiB");
  const FusedMultiArgs &m = a.m;
  if (!m.total_quads) return hipSuccess;
  if (n < 1 || n > kMaxLayers || (!a.image_out && !m.n_out)) return hipErrorInvalidValue;
  bool img = false;
  for (int l = 0; l < n; ++l) {  // every pointer the kernel will follow is there
    if (!m.layers[l] || a.is_image[l] > 1u) return hipErrorInvalidValue;
    img = img || a.is_image[l];
  }
  FusedRouteArgs b = a;
  uint32_t grid, lds;
  if (m.n_out) {
    // (the frame bound of the plan - total_quads * quads_per_line < 2^32 - is the bound the image's addresses are written for)
    const hipError_t e = fused_multi_plan(m, num_cus, max_wgs, b.m, grid, lds);
    if (e != hipSuccess) return e;
  } else {  // the image alone: the plan's checks and grid without its outputs; the reader's table is the only one in the LDS
    if (!m.quads_per_line || m.quads_per_line % 8u || m.total_quads % m.quads_per_line) return hipErrorInvalidValue;
    if ((uint64_t)m.total_quads * m.quads_per_line >= (1ull << 32)) return hipErrorInvalidValue;
    lds = m.rd.bytes;
    b.m.magic_qpl = (uint32_t)(((1ull << 32) + m.quads_per_line - 1) / m.quads_per_line);
    b.m.need_line = 0;
    const uint32_t slices = (m.total_quads + kLdsBlock - 1) / kLdsBlock;
    grid = num_cus ? num_cus : 1;
    if (grid > slices) grid = slices;
    if (max_wgs && grid > max_wgs) grid = max_wgs;
  }
  b.nt = image_nt((size_t)m.total_quads * 96u);
  char name[48];
  snprintf(name, sizeof name, "fused_v210_route_multi x%ui%d", m.n_out, a.image_out ? 1 : 0);
  if (trace_launch(name)) return hipSuccess;
  switch (n) {
    case 1: return launch_fused_route_img<1>(s, b, img, grid, lds);
    case 2: return launch_fused_route_img<2>(s, b, img, grid, lds);
    case 3: return launch_fused_route_img<3>(s, b, img, grid, lds);
    case 4: return launch_fused_route_img<4>(s, b, img, grid, lds);
    case 5: return launch_fused_route_img<5>(s, b, img, grid, lds);
    case 6: return launch_fused_route_img<6>(s, b, img, grid, lds);
    case 7: return launch_fused_route_img<7>(s, b, img, grid, lds);
    case 8: return launch_fused_route_img<8>(s, b, img, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ph
