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
template <class O>
__device__ __forceinline__ void fused_out_store(const O &o, const float (&g)[18], uint32_t f, uint32_t line, uint32_t col) {
  // a field output: the lines of its parity, height / 2 of them (per lane: a wave may span lines)
  if (o.takes && ((line & 1u) + 1u != o.takes || line >= o.line_end)) return;
  if (fmt_rgb8((int)o.fmt)) {  // rgba8.ts:69-101, alpha 255
    // bgra8 is rgba8 with red and blue exchanged (uniform selects).  A pixel pair at a time, the pairs kept apart: eighteen bytes
    // being rounded at once want registers this kernel does not have
    const bool bgr = o.fmt == PH_FMT_BGRA8;
    uint2 *const dst = reinterpret_cast<uint2 *>(o.plane[0]) + (size_t)f * 3u;  // 24 bytes per quad: 8-byte pieces
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
    store_stream(reinterpret_cast<uint4 *>(o.plane[0]) + f, pack_quad(y, u, v));
    return;
  }
  if (o.fmt == PH_FMT_YUV422P10) {  // 16-bit samples: 12 bytes of luma (4-byte aligned), 6 + 6 of chroma (2-byte aligned)
    uint32_t *const py = reinterpret_cast<uint32_t *>(o.plane[0]) + (size_t)f * 3u;
    py[0] = (y[0] & 0xffffu) | y[1] << 16, py[1] = (y[2] & 0xffffu) | y[3] << 16, py[2] = (y[4] & 0xffffu) | y[5] << 16;
    uint16_t *const pu = reinterpret_cast<uint16_t *>(o.plane[1]) + (size_t)f * 3u;
    uint16_t *const pv = reinterpret_cast<uint16_t *>(o.plane[2]) + (size_t)f * 3u;
#pragma unroll
    for (int j = 0; j < 3; ++j) pu[j] = (uint16_t)u[j], pv[j] = (uint16_t)v[j];
    return;
  }
  // the 8-bit planar formats: uchar = (uchar)ushort keeps the low 8 bits (yuv422p8.ts:166-168)
  uint16_t *const py = reinterpret_cast<uint16_t *>(o.plane[0]) + (size_t)f * 3u;
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
    uint16_t *const pc = reinterpret_cast<uint16_t *>(o.plane[1]) + c;
#pragma unroll
    for (int j = 0; j < 3; ++j) pc[j] = (uint16_t)((u[j] & 0xffu) | (v[j] & 0xffu) << 8);
    return;
  }
  uint8_t *const pu = reinterpret_cast<uint8_t *>(o.plane[1]) + c, *const pv = reinterpret_cast<uint8_t *>(o.plane[2]) + c;
#pragma unroll
  for (int j = 0; j < 3; ++j) pu[j] = (uint8_t)u[j], pv[j] = (uint8_t)v[j];
}

}  // namespace

template <int N>
__global__ __launch_bounds__(kLdsBlock) void fused_v210_combine_multi_kernel(FusedMultiArgs a) {
  constexpr int P = 6, BS = kLdsBlock;
  // The output descriptors are walked by run-time index (table groups, the outputs of a group).  Read through the argument struct
  // that would put a private copy of all of it in scratch; read where they are - the explicit arguments lie at the start of the
  // kernel-argument segment - they stay scalar loads at a computed offset.
  typedef const __attribute__((address_space(4))) FusedMultiArgs *fm_kernarg_ptr;
  const auto *const outs = ((fm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr())->out;
  const ReadK rk = load_read_k(a.rd_cm, a.rd_gm);
  const LutK rlut = make_lut_k(a.rd);
  const bool std_matrix = ycbcr_matrix_is_standard(rk);  // uniform
  auto layer_ptr = [&](int l) { return reinterpret_cast<const uint4 *>(a.layers[l]); };
  // every workgroup owns one contiguous, equally sized range of quads - it begins and ends wherever that falls, in mid-line too -
  // and walks it in tiles of BS * P quads; only the last tile of a range is partially filled
  const uint32_t per_wg = (a.total_quads + gridDim.x - 1) / gridDim.x;
  const uint32_t wg_begin = blockIdx.x * per_wg;
  const uint32_t wg_end = wg_begin + per_wg < a.total_quads ? wg_begin + per_wg : a.total_quads;
  const uint32_t tile_quads = BS * P;
  for (uint32_t tile_begin = wg_begin; tile_begin < wg_end; tile_begin += tile_quads) {
    uint32_t st[P][9];
    // (pinned per tile, like the reader table's place below: what the lanes derive from them is made in the tile, not kept in
    // registers through it for a next tile that a frame-sized share does not have)
    uint32_t last_quad = wg_end - 1;
    asm volatile("" : "+s"(last_quad));
    auto quad_of = [&](int p) {
      const uint32_t f = tile_begin + p * BS + threadIdx.x;  // width % 48 == 0: flat index == offset
      return f < wg_end ? f : last_quad;                      // tail lanes recompute the last quad
    };
    // one-deep prefetch through layers and slices; the very first word is requested before the table load
    uint4 w = load_stream(layer_ptr(0) + quad_of(0));
    auto phase1_slice = [&](auto tag, uint4 w, uint32_t f, uint32_t f_next, bool more, uint32_t(&st)[9]) -> uint4 {
      float acc[18];
#pragma unroll
      for (int i = 0; i < 18; ++i) acc[i] = 0.0f;
#pragma unroll 1  // rolled: one copy of the per-layer code whatever N is
      for (int l = 0; l < N; ++l) {
        uint4 nxt = w;
        if (l + 1 < N) nxt = load_stream(layer_ptr(l + 1) + f);
        else if (more) nxt = load_stream(layer_ptr(0) + f_next);
        const Yuv6 q = unpack_quad(w);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float4 t = read_px_lds<decltype(tag)::value>(q.y[j], q.cb[j >> 1], q.cr[j >> 1], rk, rlut, 1.0f);
          const float kk = 1.0f - t.w;
          // acc = fma(acc, kk, t), acc as destination (combine.ts:45-65; layer 0: fma(0, k, t) == t)
          asm volatile("v_fma_f32 %0, %0, %3, %4\n\tv_fma_f32 %1, %1, %3, %5\n\tv_fma_f32 %2, %2, %3, %6"
                       : "+v"(acc[3 * j]), "+v"(acc[3 * j + 1]), "+v"(acc[3 * j + 2])
                       : "v"(kk), "v"(t.x), "v"(t.y), "v"(t.z));
        }
        w = nxt;
      }
#pragma unroll
      for (int i = 0; i < 9; ++i) {  // the writers' first step needs no table: the 16-bit indices, two per register
        const uint32_t lo = __float_as_uint(lds_lut_index_unit(acc[2 * i]));
        const uint32_t hi = __float_as_uint(lds_lut_index_unit(acc[2 * i + 1]));
        st[i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        asm volatile("" : "+v"(st[i]));  // pinned: keeps phase 1's arithmetic in front of the barrier
      }
      return w;
    };
    {
      LutView rd = a.rd;
      asm volatile("" : "+s"(rd.blob), "+s"(rd.hole));
      lds_lut_load<BS>(rd);
    }
    __syncthreads();
    // a slice is skipped per WAVE: only the waves that hold quads of a partly filled slice run it
    const uint32_t wave_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x & ~63u));
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const uint32_t f = quad_of(p);
      if (p * BS + wave_first < wg_end - tile_begin) {
        PH_FM_BALANCE(p);
        const bool more = (p + 1 < P) && ((p + 1) * BS + wave_first < wg_end - tile_begin);
        const uint32_t f_next = more ? quad_of(p + 1) : f;
        if (std_matrix) w = phase1_slice(std::true_type{}, w, f, f_next, more, st[p]);
        else w = phase1_slice(std::false_type{}, w, f, f_next, more, st[p]);
      }
    }
    // phase 2, once per distinct writer table (the outputs arrive grouped by table)
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < a.n_out;) {
      const LutView wr{outs[k0].wr.blob, outs[k0].wr.bytes, outs[k0].wr.hole, outs[k0].wr.bias, outs[k0].wr.shift, outs[k0].wr.a_scale, outs[k0].wr.delta_scale, outs[k0].wr.delta_base};
      uint32_t k1 = k0 + 1;
      while (k1 < a.n_out && outs[k1].wr.blob == wr.blob) ++k1;  // uniform
      __syncthreads();  // nobody reads the table in the LDS any more
      lds_lut_load<BS>(wr);
      __syncthreads();
      const LutK wlut = make_lut_k(wr);
      uint32_t lane_quad = tile_begin + threadIdx.x;
      asm volatile("" : "+v"(lane_quad));  // (pinned: every slice's quad, line and column are made here, not kept from in front of the loop)
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const uint32_t f = lane_quad + p * BS;
        if (p * BS + wave_first < wg_end - tile_begin) {
          PH_FM_BALANCE(p);
          float g[18];
#pragma unroll
          for (int i = 0; i < 9; ++i) {  // M + idx: the index ORed into the mantissa of 1.5 * 2^23
            // (pinned: the expansion does not depend on the table, and left alone all 108 expanded indices of the tile are made
            // in front of the loop over the tables and kept through it - twice the registers the packed ones take)
            asm volatile("" : "+v"(st[p][i]));
            g[2 * i] = lds_lut_fetch(wlut, __uint_as_float((st[p][i] & 0xFFFFu) | 0x4B400000u));
            g[2 * i + 1] = lds_lut_fetch(wlut, __uint_as_float((st[p][i] >> 16) | 0x4B400000u));
            // two pixels' twelve LDS reads in flight at a time: all thirty-six at once would want registers this kernel does not have
            if (i % 3 == 2) __builtin_amdgcn_sched_barrier(0);
          }
          if (f < wg_end) {
            uint32_t line = 0, col = 0;
            if (a.need_line) {  // uniform: some output is a field or 4:2:0
              line = __umulhi(f, a.magic_qpl);
              col = f - line * a.quads_per_line;
            }
#pragma unroll 1
            for (uint32_t k = k0; k < k1; ++k) fused_out_store(outs[k], g, f, line, col);
          }
        }
      }
      k0 = k1;
    }
    __syncthreads();  // the next tile loads the reader's table
  }
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

}  // namespace ph
