// ph_kernels_fused_trans.hip - the plain-layer composite for up to four consumers (ph_kernels_fused_multi.hip) with layers that may be
// in a TRANSITION: [v210 read] x (N + partners) -> dissolve / wipe -> combine_N -> write (ph_fused_v210_transition_multi).
//
// A translation unit of its own: ph_kernels_fused_multi.hip's kernels are compiled from the text they always had.
//
// The kernel is the single frame's body (ph_kernels_fused_multi_body.h, PH_FM_TRANS 1): flat quad ranges and tiles, the one-deep
// prefetch of the layers' own words, the rolled layer loop, the packed st[p][9], the table swap and the once-per-table phase 2 with
// fused_out_store.  A layer's kind is uniform - a scalar load from the argument block - so a layer in a transition branches out of the
// loop's plain path into fm_trans_layer below and comes back for the next layer.
#include "ph_device.h"
#include "ph_kernels.h"
#include "ph_ldslut.h"

#include <cstdio>
#include <type_traits>

#pragma clang fp contract(off)

namespace ph {

namespace {

#include "ph_kernels_fused_out.h"

// pixel J of a word quad as unpack_quad gives it (v210.ts:58-63): the fields are taken where the pixel is used, pixel by pixel -
// unpacked up front, three quads' 36 values stand beside the accumulators and the tile's packed indices, and registers spill
struct Yuv1f {
  float y, cb, cr;
};
template <int J>
__device__ __forceinline__ Yuv1f unpack_px(const uint4 w) {
  const uint32_t ys = J == 0 ? w.x >> 10 : J == 1 ? w.y : J == 2 ? w.y >> 20 : J == 3 ? w.z >> 10 : J == 4 ? w.w : w.w >> 20;
  const uint32_t cbs = J < 2 ? w.x : J < 4 ? w.y >> 10 : w.z >> 20;
  const uint32_t crs = J < 2 ? w.x >> 20 : J < 4 ? w.z : w.w >> 10;
  return Yuv1f{(float)(ys & 0x3ff), (float)(cbs & 0x3ff), (float)(crs & 0x3ff)};
}
template <bool STD, int J>
__device__ __forceinline__ float4 read_word_px(const uint4 w, const ReadK &rk, const LutK &rlut) {
  const Yuv1f c = unpack_px<J>(w);
  return read_px_lds<STD>(c.y, c.cb, c.cr, rk, rlut, 1.0f);
}

// one pixel of a layer in a transition: mixed and combined (see fm_trans_layer)
template <bool STD, int J>
__device__ __forceinline__ void fm_trans_px(float (&acc)[18], const uint4 wx, const uint4 wy, const uint32_t (&mk)[6], float mix, uint32_t kind, int l,
                                            const ReadK &rk, const LutK &rlut) {
  const float4 x = read_word_px<STD, J>(wx, rk, rlut), y = read_word_px<STD, J>(wy, rk, rlut);
  float m = mix;
  if (kind == kFusedWipeV210) m = read_word_px<STD, J>(make_uint4(mk[0], mk[1], mk[2], mk[3]), rk, rlut).x;  // through the reader like a layer; its red
  if (kind == kFusedWipeF32) m = __uint_as_float(mk[J]);
  const float rm = 1.0f - m;
  const float tx = fma_rn(x.x, m, y.x * rm), ty = fma_rn(x.y, m, y.y * rm), tz = fma_rn(x.z, m, y.z * rm);
  const float tw = fma_rn(x.w, m, y.w * rm);
  const float kk = l ? 1.0f - tw : 0.0f;
  asm volatile("v_fma_f32 %0, %0, %3, %4\n\tv_fma_f32 %1, %1, %3, %5\n\tv_fma_f32 %2, %2, %3, %6"
               : "+v"(acc[3 * J]), "+v"(acc[3 * J + 1]), "+v"(acc[3 * J + 2])
               : "v"(kk), "v"(tx), "v"(ty), "v"(tz));
}

// One layer in a dissolve or a wipe, for the quad f: its own word w is there (the prefetch chain's); the incoming frame's word and the
// mask are asked for here, with the streaming load - they do not join the chain, which would keep eight more registers alive through
// the layer in front (profiles/fused_trans_resources.txt: the kernel stands at 127 - 128 VGPRs with 1024 lanes as it is).  The mix is made
// pixel by pixel (fm_trans_px) - both sides' read_px_lds, the factor, four fma - so a pixel's eight values stand beside acc[18], not a
// second accumulator; a scheduling barrier between the pixels keeps one pixel's lookups in flight at a time.
//   dissolve: t = fma(src, mix, incoming * (1 - mix))        (transition.ts:58-64)
//   wipe:     t = fma(incoming, m, src * (1 - m))            (transition.ts:66-77), m = the mask's red at the pixel
// One text for both: x is the side under the fma, y the side under the product (uniform selects of the two words).  Alpha is a value:
// both sides' is 1, so t.a = fma(1, m, 1 * (1 - m)), which is not always 1 (mix = 1/3) and is NaN where a mask holds Inf.
// The combine takes the bottom layer as it is: there k is 0 whatever t.a says, and fma(0, 0, t) is t (but for the sign of a zero,
// which no table index sees); above it k = 1 - t.a, acc = fma(acc, k, t) (combine.ts:45-65).
// Addresses: f < total_quads < 2^29 (the launcher's bound with at least 8 quads per line); the words are indexed as 16-byte
// elements through a 64-bit offset, the f32 mask's pixel 6 f + j as (size_t)f * 24 + 4 j floats - correct for every frame the
// launcher takes.  Tail lanes come with the last quad of the range in f, for every pointer.
template <bool STD, class K>
__device__ __forceinline__ void fm_trans_layer(float (&acc)[18], const uint4 w, const K karg, int l, uint32_t f, const ReadK &rk, const LutK &rlut) {
  const uint32_t kind = karg->kind[l];  // uniform
  const uint4 wi = load_stream(reinterpret_cast<const uint4 *>(karg->incoming[l]) + f);
  // the mask as it is loaded, in one set of six registers whichever kind it is - a v210 mask's four words (the factor is made where its
  // pixel is, not six factors up front) or the six reds of an f32 RGBA image, 16 bytes apart
  uint32_t mk[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  const float mix = karg->mix[l];
  if (kind == kFusedWipeV210) {
    const uint4 wm = load_stream(reinterpret_cast<const uint4 *>(karg->mask[l]) + f);
    mk[0] = wm.x, mk[1] = wm.y, mk[2] = wm.z, mk[3] = wm.w;
  } else if (kind == kFusedWipeF32) {
    const float *const pm = reinterpret_cast<const float *>(karg->mask[l]) + (size_t)f * 24u;
#pragma unroll
    for (int j = 0; j < 6; ++j) mk[j] = __float_as_uint(__builtin_nontemporal_load(pm + 4 * j));
  }
  const bool wipe = kind != kFusedDissolve;
  const uint4 wx = make_uint4(wipe ? wi.x : w.x, wipe ? wi.y : w.y, wipe ? wi.z : w.z, wipe ? wi.w : w.w);
  const uint4 wy = make_uint4(wipe ? w.x : wi.x, wipe ? w.y : wi.y, wipe ? w.z : wi.z, wipe ? w.w : wi.w);
  fm_trans_px<STD, 0>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
  __builtin_amdgcn_sched_barrier(0);
  fm_trans_px<STD, 1>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
  __builtin_amdgcn_sched_barrier(0);
  fm_trans_px<STD, 2>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
  __builtin_amdgcn_sched_barrier(0);
  fm_trans_px<STD, 3>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
  __builtin_amdgcn_sched_barrier(0);
  fm_trans_px<STD, 4>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
  __builtin_amdgcn_sched_barrier(0);
  fm_trans_px<STD, 5>(acc, wx, wy, mk, mix, kind, l, rk, rlut);
}

}  // namespace

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_trans_multi_kernel(FusedTransArgs args) {
  const FusedMultiArgs &a = args.m;
#define PH_FM_BATCH 0
#define PH_FM_TRANS 1
#include "ph_kernels_fused_multi_body.h"
#undef PH_FM_BATCH
#undef PH_FM_TRANS
}

template <int N>
static hipError_t launch_fused_trans_n(hipStream_t s, const FusedTransArgs &a, uint32_t grid, uint32_t lds) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fused_v210_trans_multi_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  fused_v210_trans_multi_kernel<N><<<grid, kLdsBlock, lds, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_fused_v210_trans_multi(hipStream_t s, int n, const FusedTransArgs &a, uint32_t num_cus, uint32_t max_wgs) {
  static_assert(sizeof(FusedTransArgs) <= 4096, "the argument block stays within 4 KiB");
  if (!a.m.total_quads) return hipSuccess;
  if (n < 1 || n > kMaxLayers) return hipErrorInvalidValue;
  for (int l = 0; l < n; ++l) {  // every pointer the kernel will follow is there
    if (a.kind[l] > kFusedWipeF32 || !a.m.layers[l]) return hipErrorInvalidValue;
    if (a.kind[l] != kFusedCut && !a.incoming[l]) return hipErrorInvalidValue;
    if (a.kind[l] >= kFusedWipeV210 && !a.mask[l]) return hipErrorInvalidValue;
  }
  FusedTransArgs b = a;
  uint32_t grid, lds;
  // (the frame bound of the plan - total_quads * quads_per_line < 2^32 - is the bound fm_trans_layer's addresses are written for)
  const hipError_t e = fused_multi_plan(a.m, num_cus, max_wgs, b.m, grid, lds);
  if (e != hipSuccess) return e;
  char name[40];
  snprintf(name, sizeof name, "fused_v210_trans_multi x%u", a.m.n_out);
  if (trace_launch(name)) return hipSuccess;
  switch (n) {
    case 1: return launch_fused_trans_n<1>(s, b, grid, lds);
    case 2: return launch_fused_trans_n<2>(s, b, grid, lds);
    case 3: return launch_fused_trans_n<3>(s, b, grid, lds);
    case 4: return launch_fused_trans_n<4>(s, b, grid, lds);
    case 5: return launch_fused_trans_n<5>(s, b, grid, lds);
    case 6: return launch_fused_trans_n<6>(s, b, grid, lds);
    case 7: return launch_fused_trans_n<7>(s, b, grid, lds);
    case 8: return launch_fused_trans_n<8>(s, b, grid, lds);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace ph
