// ph_kernels_fmt.hip - the reference's other packed formats:
//   yuv422p10le (yuv422p10.ts), yuv422p8 (yuv422p8.ts), yuv420p (yuv420p.ts), nv12 (nv12.ts),
//   rgba8 (rgba8.ts), bgra8 (bgra8.ts) - read (-> linear f32 RGBA) and write (<- f32 RGBA) - and the 10-bit 4:2:0 decoder frames
//   yuv420p10le and p010le, which the reference has no kernel for: defined as its yuv422p10 Reader / Writer on the 4:2:2 frame whose
//   chroma line r is the 4:2:0 frame's line r >> 1 (read), whose upper line of a pair gives the chroma (write) - DESIGN.md 2.
//
// Readers: one PIXEL per lane (coalesced float4 stores; the sample loads of a wave are 64-128
// contiguous bytes).  Writers: one group of 8 pixels per lane (8-16 byte plane stores), the
// 4:2:0 writers handle the line pair of their group.  Every kernel exists in two forms chosen at
// launch: gamma LUT in LDS (persistent 1024-lane workgroups) or plain table in global memory.
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "ph_kernels.h"
#include "ph_ldslut.h"

#pragma clang fp contract(off)

namespace ph {

constexpr int kFmtBlock = 256;

template <typename LUT>
__device__ __forceinline__ float4 yuv_to_rgba(float y, float u, float v, const ReadK &k, const LUT &lut) {
  const float r = lut.at_unit(dot4(y, u, v, 1.0f, k.r));  // e.g. yuv422p10.ts:74-78
  const float g = lut.at_unit(dot4(y, u, v, 1.0f, k.g));
  const float b = lut.at_unit(dot4(y, u, v, 1.0f, k.b));
  return make_float4(dot3(r, g, b, k.gm[0], k.gm[1], k.gm[2]), dot3(r, g, b, k.gm[3], k.gm[4], k.gm[5]),
                     dot3(r, g, b, k.gm[6], k.gm[7], k.gm[8]), 1.0f);
}

struct FmtReadArgs {
  const void *p0, *p1, *p2;
  float4 *out;
  uint32_t width, lines, pitch;  // pitch in luma samples (RGBA: pixels)
  const float *cm, *gm;
  uint32_t nt;  // stream the image output past the caches (ph_device.h store_image)
};

// FMT is a template parameter: plane layout and sample width are compile-time
template <int FMT, typename LUT, bool PERSISTENT>
__device__ __forceinline__ void fmt_read_body(const FmtReadArgs &a, const LUT &lut, uint32_t block = blockIdx.x, uint32_t blocks = gridDim.x) {
  ReadK k;
  if (fmt_rgb8(FMT)) {  // the RGB formats carry no YCbCr matrix: gamut only (9 floats, never more)
#pragma unroll
    for (int i = 0; i < 9; ++i) k.gm[i] = a.gm[i];
  } else {
    k = load_read_k(a.cm, a.gm);
  }
  const uint32_t total = a.width * a.lines;
  const uint32_t stride = PERSISTENT ? blocks * blockDim.x : total;
  for (uint32_t p = block * blockDim.x + threadIdx.x; p < total; p += stride) {
    const uint32_t line = p / a.width, x = p - line * a.width;
    float4 o;
    if (fmt_rgb8(FMT)) {
      const uchar4 px = __builtin_bit_cast(uchar4, fmt_fetch<FMT>(a.p0, a.p1, a.p2, a.pitch, x, line).x);
      constexpr bool RGBA = FMT == PH_FMT_RGBA8;
      o = rgb8_to_rgba((float)(RGBA ? px.x : px.z), (float)px.y, (float)(RGBA ? px.z : px.x), (float)px.w, k, lut);
    } else {
      const float4 c = fmt_fetch<FMT, float4>(a.p0, a.p1, a.p2, a.pitch, x, line);
      o = yuv_to_rgba(c.x, c.y, c.z, k, lut);
    }
    store_image(a.out + p, o, a.nt);
  }
}

template <int FMT>
__global__ __launch_bounds__(kLdsBlock) void fmt_read_lds_kernel(FmtReadArgs a, LutView lv) {
  const LutInLds lut{make_lut_k(lv)};
  lds_lut_load(lv);
  __syncthreads();
  fmt_read_body<FMT, LutInLds, true>(a, lut);
}
// several frames of one format, size and Loader recipe in one launch (several channels' clips of a tick: ph_pack_read_batch): the
// workgroups go round the frames (uniform per workgroup: the frame's pointers are scalar loads), the table is loaded once per workgroup as ever
struct FmtReadBatchArgs {
  const void *p0[kMaxLayers], *p1[kMaxLayers], *p2[kMaxLayers];
  float4 *out[kMaxLayers];
  uint32_t jobs;
  uint32_t width, lines, pitch;
  const float *cm, *gm;
  uint32_t nt;
};
template <int FMT>
__global__ __launch_bounds__(kLdsBlock) void fmt_read_lds_batch_kernel(FmtReadBatchArgs b, LutView lv) {
  const LutInLds lut{make_lut_k(lv)};
  lds_lut_load(lv);
  __syncthreads();
  const uint32_t per_job = gridDim.x / b.jobs, job = blockIdx.x / per_job;  // (the launcher makes the grid a multiple of jobs)
  const FmtReadArgs a{b.p0[job], b.p1[job], b.p2[job], b.out[job], b.width, b.lines, b.pitch, b.cm, b.gm, b.nt};
  fmt_read_body<FMT, LutInLds, true>(a, lut, blockIdx.x - job * per_job, per_job);
}
template <int FMT>
__global__ __launch_bounds__(kFmtBlock) void fmt_read_gather_kernel(FmtReadArgs a, const float *__restrict__ table) {
  const LutInGlobal lut{table};
  fmt_read_body<FMT, LutInGlobal, false>(a, lut);
}

// ------------------------------------------------------------------------------------------
// writers
// ------------------------------------------------------------------------------------------
struct FmtWriteArgs {
  const float4 *in;
  void *p0, *p1, *p2;
  uint32_t width, pitch;          // pitch in luma samples
  uint32_t groups;                // work groups of the reference: lines, or line pairs for 4:2:0
  uint32_t interlace;
  const float *cm;
};

template <typename LUT>
__device__ __forceinline__ void px_codes(const float4 px, const WriteK &k, const LUT &lut, bool tail, uint32_t &y,
                                         uint32_t &u, uint32_t &v) {
  const float gr = lut.at_unit(px.x), gg = lut.at_unit(px.y), gb = lut.at_unit(px.z);
  float ty = dot4(gr, gg, gb, 1.0f, k.y), tu = dot4(gr, gg, gb, 1.0f, k.u), tv = dot4(gr, gg, gb, 1.0f, k.v);
  if (tail) ty = __builtin_roundf(ty), tu = __builtin_roundf(tu), tv = __builtin_roundf(tv);  // :186-188
  y = sat_u16_rte(ty), u = sat_u16_rte(tu), v = sat_u16_rte(tv);
}

template <int FMT, typename LUT, bool PERSISTENT>
__device__ __forceinline__ void fmt_write_body(const FmtWriteArgs &a, const LUT &lut) {
  if (fmt_rgb8(FMT)) {  // rgba8.ts:69-101: one pixel per lane
    const uint32_t total = a.width * a.groups;
    const uint32_t stride = PERSISTENT ? gridDim.x * blockDim.x : total;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += stride) {
      const uint32_t g = p / a.width, x = p - g * a.width;
      const uint32_t line = g * (a.interlace ? 2 : 1) + ((3 == a.interlace) ? 1 : 0);
      const float4 px = a.in[(size_t)line * a.width + x];
      const float r = lut.at_unit(px.x), gg = lut.at_unit(px.y), b = lut.at_unit(px.z);
      const uint32_t r8 = sat_u8_rte(r * 255.0f);
      const uint32_t g8 = sat_u8_rte(gg * 255.0f);
      const uint32_t b8 = sat_u8_rte(b * 255.0f);
      const uint32_t w = FMT == PH_FMT_RGBA8 ? (r8 | g8 << 8 | b8 << 16 | 0xff000000u) : (b8 | g8 << 8 | r8 << 16 | 0xff000000u);
      reinterpret_cast<uint32_t *>(a.p0)[(size_t)line * a.pitch + x] = w;
    }
    return;
  }
  constexpr bool V420 = fmt_v420(FMT), WIDE = fmt_wide(FMT);
  constexpr uint32_t MSB = fmt_msb(FMT);  // p010: the code in the word's upper bits
  const WriteK k = load_write_k(a.cm);
  const uint32_t full = a.width / 8, remain = a.width % 8, octets = full + (remain ? 1 : 0);
  const uint32_t total = octets * a.groups;
  const uint32_t stride = PERSISTENT ? gridDim.x * blockDim.x : total;
  for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < total; f += stride) {
    const uint32_t g = f / octets, o8 = f - g * octets;
    const bool tail = (o8 == full);
    const uint32_t n = tail ? (remain < 6 ? remain : 6) : 8;
    // 4:2:2: one line per group (yuv422p10.ts:140-141); 4:2:0: line pair, or one field line of it
    const uint32_t first = V420 ? g * 2 + ((3 == a.interlace) ? 1 : 0)
                                : g * (a.interlace ? 2 : 1) + ((3 == a.interlace) ? 1 : 0);
    const uint32_t nlines = V420 ? (a.interlace ? 1 : 2) : 1;
    const uint32_t crow = V420 ? g : first;
    for (uint32_t l = 0; l < nlines; ++l) {
      const uint32_t line = first + l;
      const float4 *px = a.in + (size_t)line * a.width + 8 * o8;
      uint32_t y[8], u[4], v[4];
#pragma unroll
      for (int p = 0; p < 8; ++p) y[p] = WIDE ? 64u : 16u;  // tail defaults (:191-193)
#pragma unroll
      for (int p = 0; p < 4; ++p) u[p] = v[p] = WIDE ? 512u : 128u;
      if (!tail) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          uint32_t cy, cu, cv;
          px_codes(px[p], k, lut, false, cy, cu, cv);
          y[p] = cy;
          if (!(p & 1)) u[p >> 1] = cu, v[p >> 1] = cv;
        }
      } else {  // yuv422p10.ts:190-217 / yuv420p.ts:213-251
        uint32_t cy[6] = {0, 0, 0, 0, 0, 0}, cu[6] = {0, 0, 0, 0, 0, 0}, cv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int p = 0; p < 6; ++p)
          if ((uint32_t)p < n) px_codes(px[p], k, lut, true, cy[p], cu[p], cv[p]);
        y[0] = cy[0], y[1] = cy[1], u[0] = cu[0], v[0] = cv[0];
        if (remain > 2) {
          y[2] = cy[2], y[3] = cy[3], u[1] = cu[2], v[1] = cv[2];
          if (remain > 4) {
            y[4] = cy[4], y[5] = cy[5];
            if (V420 && !WIDE) u[2] = cu[4], v[2] = cv[4];
            else u[1] = cu[4], v[1] = cv[4];  // the 4:2:2 writers overwrite slot 1 (yuv422p10.ts:209-210) - so do the 10-bit 4:2:0 ones defined by them
          }
        }
      }
      if (WIDE) {
        uint4 w;
        w.x = ((y[0] << MSB) & 0xffff) | y[1] << (16 + MSB), w.y = ((y[2] << MSB) & 0xffff) | y[3] << (16 + MSB);
        w.z = ((y[4] << MSB) & 0xffff) | y[5] << (16 + MSB), w.w = ((y[6] << MSB) & 0xffff) | y[7] << (16 + MSB);
        reinterpret_cast<uint4 *>(a.p0)[((size_t)line * a.pitch >> 3) + o8] = w;
      } else {  // uchar = (uchar)ushort keeps the low 8 bits (yuv422p8.ts:166-168)
        uint2 w;
        w.x = (y[0] & 0xff) | (y[1] & 0xff) << 8 | (y[2] & 0xff) << 16 | y[3] << 24;
        w.y = (y[4] & 0xff) | (y[5] & 0xff) << 8 | (y[6] & 0xff) << 16 | y[7] << 24;
        reinterpret_cast<uint2 *>(a.p0)[((size_t)line * a.pitch >> 3) + o8] = w;
      }
      if (l == 0) {
        if (fmt_cbcr(FMT) && !WIDE) {  // nv12
          uint2 w;
          w.x = (u[0] & 0xff) | (v[0] & 0xff) << 8 | (u[1] & 0xff) << 16 | v[1] << 24;
          w.y = (u[2] & 0xff) | (v[2] & 0xff) << 8 | (u[3] & 0xff) << 16 | v[3] << 24;
          reinterpret_cast<uint2 *>(a.p1)[((size_t)crow * a.pitch >> 3) + o8] = w;
        } else if (fmt_cbcr(FMT)) {  // p010: Cb, Cr words interleaved - 16 bytes per group, the luma line's pitch
          uint4 w;
          w.x = ((u[0] << MSB) & 0xffff) | v[0] << (16 + MSB), w.y = ((u[1] << MSB) & 0xffff) | v[1] << (16 + MSB);
          w.z = ((u[2] << MSB) & 0xffff) | v[2] << (16 + MSB), w.w = ((u[3] << MSB) & 0xffff) | v[3] << (16 + MSB);
          reinterpret_cast<uint4 *>(a.p1)[((size_t)crow * a.pitch >> 3) + o8] = w;
        } else if (WIDE) {
          uint2 wu, wv;
          wu.x = (u[0] & 0xffff) | u[1] << 16, wu.y = (u[2] & 0xffff) | u[3] << 16;
          wv.x = (v[0] & 0xffff) | v[1] << 16, wv.y = (v[2] & 0xffff) | v[3] << 16;
          reinterpret_cast<uint2 *>(a.p1)[((size_t)crow * a.pitch >> 3) + o8] = wu;
          reinterpret_cast<uint2 *>(a.p2)[((size_t)crow * a.pitch >> 3) + o8] = wv;
        } else {
          const uint32_t wu = (u[0] & 0xff) | (u[1] & 0xff) << 8 | (u[2] & 0xff) << 16 | u[3] << 24;
          const uint32_t wv = (v[0] & 0xff) | (v[1] & 0xff) << 8 | (v[2] & 0xff) << 16 | v[3] << 24;
          reinterpret_cast<uint32_t *>(a.p1)[((size_t)crow * a.pitch >> 3) + o8] = wu;
          reinterpret_cast<uint32_t *>(a.p2)[((size_t)crow * a.pitch >> 3) + o8] = wv;
        }
      }
    }
  }
}

template <int FMT>
__global__ __launch_bounds__(kLdsBlock) void fmt_write_lds_kernel(FmtWriteArgs a, LutView lv) {
  const LutInLds lut{make_lut_k(lv)};
  lds_lut_load(lv);
  __syncthreads();
  fmt_write_body<FMT, LutInLds, true>(a, lut);
}
template <int FMT>
__global__ __launch_bounds__(kFmtBlock) void fmt_write_gather_kernel(FmtWriteArgs a, const float *__restrict__ table) {
  const LutInGlobal lut{table};
  fmt_write_body<FMT, LutInGlobal, false>(a, lut);
}

// One group of 8 pixels of a planar frame, from its code values: the words packed and stored as the format lays them out - the Y
// words on `line` (luma), the chroma words on chroma row `crow` (chroma).  STREAM: non-temporal stores (ph_device.h store_stream).
// fmt_write_body's own packing and stores, word for word (a copy: called from fmt_write_body it changed the one-output kernels'
// register allocation, and those stay the parent's instruction for instruction - profiles/pack_write_multi_resources.txt).
template <bool STREAM>
__device__ __forceinline__ void fmt_store(uint32_t *p, const uint32_t v) {
  // (through a pointer that says "global memory": a flat one lets the optimiser merge this store with a store to a lane-private array
  // behind one pointer, and the array then lives in scratch)
  if (STREAM) __builtin_nontemporal_store(v, (__attribute__((address_space(1))) uint32_t *)p);
  else *p = v;
}
template <bool STREAM>
__device__ __forceinline__ void fmt_store(uint2 *p, const uint2 v) {
  typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
  if (STREAM && PH_NT_STORE) __builtin_nontemporal_store(ph_u2v{v.x, v.y}, reinterpret_cast<ph_u2v *>(p));
  else *p = v;
}
template <bool STREAM>
__device__ __forceinline__ void fmt_store(uint4 *p, const uint4 v) {
  if (STREAM) store_stream(p, v);
  else *p = v;
}
template <int FMT, bool STREAM>
__device__ __forceinline__ void fmt_store_octet(void *p0, void *p1, void *p2, uint32_t pitch, uint32_t line, uint32_t crow, uint32_t o8,
                                                const uint32_t (&y)[8], const uint32_t (&u)[4], const uint32_t (&v)[4], bool luma, bool chroma) {
  constexpr bool WIDE = fmt_wide(FMT);
  constexpr uint32_t MSB = fmt_msb(FMT);  // p010: the code in the word's upper bits
  if (luma) {
    if (WIDE) {
      uint4 w;
      w.x = ((y[0] << MSB) & 0xffff) | y[1] << (16 + MSB), w.y = ((y[2] << MSB) & 0xffff) | y[3] << (16 + MSB);
      w.z = ((y[4] << MSB) & 0xffff) | y[5] << (16 + MSB), w.w = ((y[6] << MSB) & 0xffff) | y[7] << (16 + MSB);
      fmt_store<STREAM>(reinterpret_cast<uint4 *>(p0) + (((size_t)line * pitch >> 3) + o8), w);
    } else {  // uchar = (uchar)ushort keeps the low 8 bits (yuv422p8.ts:166-168)
      uint2 w;
      w.x = (y[0] & 0xff) | (y[1] & 0xff) << 8 | (y[2] & 0xff) << 16 | y[3] << 24;
      w.y = (y[4] & 0xff) | (y[5] & 0xff) << 8 | (y[6] & 0xff) << 16 | y[7] << 24;
      fmt_store<STREAM>(reinterpret_cast<uint2 *>(p0) + (((size_t)line * pitch >> 3) + o8), w);
    }
  }
  if (chroma) {
    if (fmt_cbcr(FMT) && !WIDE) {  // nv12
      uint2 w;
      w.x = (u[0] & 0xff) | (v[0] & 0xff) << 8 | (u[1] & 0xff) << 16 | v[1] << 24;
      w.y = (u[2] & 0xff) | (v[2] & 0xff) << 8 | (u[3] & 0xff) << 16 | v[3] << 24;
      fmt_store<STREAM>(reinterpret_cast<uint2 *>(p1) + (((size_t)crow * pitch >> 3) + o8), w);
    } else if (fmt_cbcr(FMT)) {  // p010: Cb, Cr words interleaved - 16 bytes per group, the luma line's pitch
      uint4 w;
      w.x = ((u[0] << MSB) & 0xffff) | v[0] << (16 + MSB), w.y = ((u[1] << MSB) & 0xffff) | v[1] << (16 + MSB);
      w.z = ((u[2] << MSB) & 0xffff) | v[2] << (16 + MSB), w.w = ((u[3] << MSB) & 0xffff) | v[3] << (16 + MSB);
      fmt_store<STREAM>(reinterpret_cast<uint4 *>(p1) + (((size_t)crow * pitch >> 3) + o8), w);
    } else if (WIDE) {
      uint2 wu, wv;
      wu.x = (u[0] & 0xffff) | u[1] << 16, wu.y = (u[2] & 0xffff) | u[3] << 16;
      wv.x = (v[0] & 0xffff) | v[1] << 16, wv.y = (v[2] & 0xffff) | v[3] << 16;
      fmt_store<STREAM>(reinterpret_cast<uint2 *>(p1) + (((size_t)crow * pitch >> 3) + o8), wu);
      fmt_store<STREAM>(reinterpret_cast<uint2 *>(p2) + (((size_t)crow * pitch >> 3) + o8), wv);
    } else {
      const uint32_t wu = (u[0] & 0xff) | (u[1] & 0xff) << 8 | (u[2] & 0xff) << 16 | u[3] << 24;
      const uint32_t wv = (v[0] & 0xff) | (v[1] & 0xff) << 8 | (v[2] & 0xff) << 16 | v[3] << 24;
      fmt_store<STREAM>(reinterpret_cast<uint32_t *>(p1) + (((size_t)crow * pitch >> 3) + o8), wu);
      fmt_store<STREAM>(reinterpret_cast<uint32_t *>(p2) + (((size_t)crow * pitch >> 3) + o8), wv);
    }
  }
}

// ------------------------------------------------------------------------------------------
// one image, several consumers (ph_pack_write_multi): every pixel loaded once and looked up once, then packed per output
// ------------------------------------------------------------------------------------------
// A lane's work unit is an OCTET: 8 consecutive pixels of a line, 128 contiguous bytes, loaded as fmt_write_body loads them and looked
// up at once - the 24 table values take the registers the 32 floats came in.  Then the outputs pack the octet in turn, one output's
// code words live at a time: a planar octet is stored from its sixteen codes, rgba8 / bgra8 as two 16-byte groups.  A v210 quad is 6
// pixels, so with a v210 output (HAS_V210) three neighbouring lanes hold the 24 pixels of four quads - a wave step is 63 octets, lane
// 63 idles, and a lane's role is lane % 3 = octet % 3 (a line is a multiple of 48 pixels here) - and trade the two pixel PAIRS (even
// pixel: Y, Cb, Cr; odd pixel: Y - two words a pair) that straddle their borders: role 0 packs quad 0 from its pairs 0..2 and hands pair 3
// to role 1, which packs quads 1 and 2 with role 2's pair 0; role 2 packs quad 3 from its pairs 1..3.
// (24 pixels a lane, tried first, left a 1080p frame with 85 workgroups' worth of units and ran at half the separate launches' speed.)
// An output's format is uniform and dispatched at run time; what is packed and how is the one-output kernels' own code (ycbcr_code /
// pack_quad / rgb8_pack, fmt_store_octet).
template <int FMT>
__device__ __forceinline__ void pack_octet_planar(const PackOut &o, const WriteK &wk, const float (&t)[8][3], uint32_t line, uint32_t o8, bool on) {
  uint32_t y[8], u[4], v[4];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    y[p] = ycbcr_code(t[p][0], t[p][1], t[p][2], wk.y);
    if (!(p & 1)) u[p >> 1] = ycbcr_code(t[p][0], t[p][1], t[p][2], wk.u), v[p >> 1] = ycbcr_code(t[p][0], t[p][1], t[p][2], wk.v);  // chroma from the even pixel
  }
  if (!on) return;
  // 4:2:0: chroma row line >> 1 from the pair's upper line, or from the one line of the pair that a field writes (fmt_write_body's crow)
  const bool chroma = !fmt_v420(FMT) || o.field || !(line & 1u);
  fmt_store_octet<FMT, true>(o.plane[0], o.plane[1], o.plane[2], o.pitch, line, fmt_v420(FMT) ? line >> 1 : line, o8, y, u, v, true, chroma);
}
__device__ __forceinline__ uint4 pack_quad_pairs(uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1, uint32_t a2, uint32_t b2) {
  const uint32_t y[6] = {a0 & 0xffffu, a0 >> 16, a1 & 0xffffu, a1 >> 16, a2 & 0xffffu, a2 >> 16};
  const uint32_t u[3] = {b0 & 0xffffu, b1 & 0xffffu, b2 & 0xffffu}, v[3] = {b0 >> 16, b1 >> 16, b2 >> 16};
  return pack_quad(y, u, v);
}
// octet o8 of `line` (t: its pixels' table values) into output o.  Every lane of the wave comes here (the v210 trade is a wave operation);
// on: the lane stores
template <bool HAS_V210>
__device__ __forceinline__ void pack_octet(const PackOut &o, const WriteK &wk, const float (&t)[8][3], uint32_t o8, uint32_t width, uint32_t line, bool on,
                                           uint32_t role) {
  const uint32_t x = 8u * o8;
  if (o.fmt == PH_FMT_RGBA8 || o.fmt == PH_FMT_BGRA8) {  // uniform
    const bool rgba = o.fmt == PH_FMT_RGBA8;
    uint32_t w[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) w[p] = rgba ? rgb8_pack<PH_FMT_RGBA8>(t[p][0], t[p][1], t[p][2]) : rgb8_pack<PH_FMT_BGRA8>(t[p][0], t[p][1], t[p][2]);
    uint32_t *const row = reinterpret_cast<uint32_t *>(o.plane[0]) + (size_t)line * o.pitch;
    if (width % 4u) {  // uniform: the lines do not start on 16 bytes - pixel by pixel, the line's last octet up to the width
#pragma unroll
      for (int p = 0; p < 8; ++p)
        if (on && x + (uint32_t)p < width) fmt_store<true>(row + x + (uint32_t)p, w[p]);
      return;
    }
    if (on && x < width) fmt_store<true>(reinterpret_cast<uint4 *>(row + x), make_uint4(w[0], w[1], w[2], w[3]));
    if (on && x + 4u < width) fmt_store<true>(reinterpret_cast<uint4 *>(row + x + 4u), make_uint4(w[4], w[5], w[6], w[7]));
    return;
  }
  if (HAS_V210 && o.fmt == PH_FMT_V210) {  // uniform
    uint32_t a[4], b[4];  // the octet's pairs: Y | Y << 16, Cb | Cr << 16
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float(&e)[3] = t[2 * p], (&d)[3] = t[2 * p + 1];
      a[p] = ycbcr_code(e[0], e[1], e[2], wk.y) | ycbcr_code(d[0], d[1], d[2], wk.y) << 16;
      b[p] = ycbcr_code(e[0], e[1], e[2], wk.u) | ycbcr_code(e[0], e[1], e[2], wk.v) << 16;
    }
    // role 1 takes pair 3 of the lane below and pair 0 of the lane above
    const uint32_t a_lo = (uint32_t)__shfl_up((int)a[3], 1), b_lo = (uint32_t)__shfl_up((int)b[3], 1);
    const uint32_t a_hi = (uint32_t)__shfl_down((int)a[0], 1), b_hi = (uint32_t)__shfl_down((int)b[0], 1);
    if (!on) return;
    uint4 *const q = reinterpret_cast<uint4 *>(o.plane[0]) + ((size_t)line * o.pitch + (o8 / 3u) * 4u);
    if (role == 0u) {
      store_stream(q, pack_quad_pairs(a[0], b[0], a[1], b[1], a[2], b[2]));
    } else if (role == 1u) {
      store_stream(q + 1, pack_quad_pairs(a_lo, b_lo, a[0], b[0], a[1], b[1]));
      store_stream(q + 2, pack_quad_pairs(a[2], b[2], a[3], b[3], a_hi, b_hi));
    } else {
      store_stream(q + 3, pack_quad_pairs(a[1], b[1], a[2], b[2], a[3], b[3]));
    }
    return;
  }
  switch (o.fmt) {  // uniform
    case PH_FMT_YUV422P10: pack_octet_planar<PH_FMT_YUV422P10>(o, wk, t, line, o8, on); break;
    case PH_FMT_YUV422P8: pack_octet_planar<PH_FMT_YUV422P8>(o, wk, t, line, o8, on); break;
    case PH_FMT_YUV420P: pack_octet_planar<PH_FMT_YUV420P>(o, wk, t, line, o8, on); break;
    case PH_FMT_NV12: pack_octet_planar<PH_FMT_NV12>(o, wk, t, line, o8, on); break;
    case PH_FMT_YUV420P10: pack_octet_planar<PH_FMT_YUV420P10>(o, wk, t, line, o8, on); break;
    case PH_FMT_P010: pack_octet_planar<PH_FMT_P010>(o, wk, t, line, o8, on); break;
  }
}
template <bool HAS_V210>
__global__ __launch_bounds__(kLdsBlock) void pack_write_multi_kernel(PackMultiArgs a) {
  WriteK wk[kMaxPackOuts];  // (read before the table load: behind its memory clobber these would be vector loads into 48 VGPRs, not scalar ones)
#pragma unroll
  for (int k = 0; k < kMaxPackOuts; ++k) {
    wk[k].y = wk[k].u = wk[k].v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((uint32_t)k < a.n_out && a.out[k].wr_cm) wk[k] = load_write_k(a.out[k].wr_cm);  // (rgba8 / bgra8: none)
  }
  const LutInLds lut{make_lut_k(a.wr)};
  lds_lut_load(a.wr);
  __syncthreads();
  constexpr uint32_t STEP = HAS_V210 ? 63u : 64u;  // octets a wave takes at a time
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u, role = lane % 3u;
  const uint32_t total = a.units_per_line * a.lines, waves = kLdsBlock / 64u;
  for (uint32_t base = (blockIdx.x * waves + wave) * STEP; base < total; base += gridDim.x * waves * STEP) {  // uniform per wave
    const bool live = lane < STEP && base + lane < total;
    const uint32_t f = live ? base + lane : total - 1u;
    const uint32_t li = f / a.units_per_line, o8 = f - li * a.units_per_line;
    const uint32_t line = a.first_line + li * a.line_step;
    const float4 *row = reinterpret_cast<const float4 *>(a.in) + (size_t)line * a.width;
    float4 px[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      uint32_t x = 8u * o8 + (uint32_t)p;
      if (!HAS_V210) x = x < a.width ? x : a.width - 1u;  // (the last octet of a line whose width is no multiple of 8 - rgba8 / bgra8 outputs only: never stored)
      px[p] = row[x];
    }
    float t[8][3];
#pragma unroll
    for (int p = 0; p < 8; ++p) t[p][0] = lut.at_unit(px[p].x), t[p][1] = lut.at_unit(px[p].y), t[p][2] = lut.at_unit(px[p].z);
#pragma unroll
    for (int k = 0; k < kMaxPackOuts; ++k) {
      const PackOut &o = a.out[k];  // (an output past n_out: line_end == 0, and its format is v210's number - so the break)
      if ((uint32_t)k >= a.n_out) break;  // uniform
      const bool on = live && line < o.line_end && (!o.takes || (line & 1u) == o.takes - 1u);
      pack_octet<HAS_V210>(o, wk[k], t, o8, a.width, line, on, role);
    }
  }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
// f(std::integral_constant<int, FMT>{}) for the pack format fmt (v210 has kernels of its own: ph_kernels_lds.hip)
template <typename F>
static hipError_t for_fmt(int fmt, F &&f) {
  switch (fmt) {
    case PH_FMT_YUV422P10: return f(std::integral_constant<int, PH_FMT_YUV422P10>{});
    case PH_FMT_YUV422P8: return f(std::integral_constant<int, PH_FMT_YUV422P8>{});
    case PH_FMT_YUV420P: return f(std::integral_constant<int, PH_FMT_YUV420P>{});
    case PH_FMT_NV12: return f(std::integral_constant<int, PH_FMT_NV12>{});
    case PH_FMT_RGBA8: return f(std::integral_constant<int, PH_FMT_RGBA8>{});
    case PH_FMT_BGRA8: return f(std::integral_constant<int, PH_FMT_BGRA8>{});
    case PH_FMT_YUV420P10: return f(std::integral_constant<int, PH_FMT_YUV420P10>{});
    case PH_FMT_P010: return f(std::integral_constant<int, PH_FMT_P010>{});
  }
  return hipErrorInvalidValue;
}

template <int FMT>
static hipError_t launch_read_fmt(hipStream_t s, const FmtReadArgs &a, const float *table, const LutView *lv,
                                  uint32_t num_cus) {
  const uint32_t total = a.width * a.lines;
  if (!total) return hipSuccess;
  if (lv) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fmt_read_lds_kernel<FMT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    const uint32_t want = (total + kLdsBlock - 1) / kLdsBlock;
    fmt_read_lds_kernel<FMT><<<want < num_cus ? want : num_cus, kLdsBlock, lv->bytes, s>>>(a, *lv);
  } else {
    fmt_read_gather_kernel<FMT><<<(total + kFmtBlock - 1) / kFmtBlock, kFmtBlock, 0, s>>>(a, table);
  }
  return hipGetLastError();
}

hipError_t launch_pack_read(hipStream_t s, int fmt, const void *const planes[3], void *out, uint32_t width,
                            uint32_t height, const void *cm, const void *table, const void *gm, const LutView *lv,
                            uint32_t num_cus) {
  const bool v420 = fmt_v420(fmt);
  FmtReadArgs a{planes[0], planes[1], planes[2], (float4 *)out, width, v420 ? (height / 2) * 2 : height,
                pack_pitch(fmt, width), (const float *)cm, (const float *)gm, image_nt((size_t)width * height * 16)};
  return for_fmt(fmt, [&](auto f) { return launch_read_fmt<decltype(f)::value>(s, a, (const float *)table, lv, num_cus); });
}

template <int FMT>
static hipError_t launch_read_batch_fmt(hipStream_t s, const FmtReadBatchArgs &b, const LutView &lv, uint32_t num_cus) {
  const uint32_t total = b.width * b.lines;
  if (!total) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fmt_read_lds_batch_kernel<FMT>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  const uint32_t want = (total + kLdsBlock - 1) / kLdsBlock, share = num_cus / b.jobs ? num_cus / b.jobs : 1u, per_job = want < share ? want : share;
  fmt_read_lds_batch_kernel<FMT><<<per_job * b.jobs, kLdsBlock, lv.bytes, s>>>(b, lv);
  return hipGetLastError();
}
// n frames (1 .. kMaxLayers) of one format, size and Loader recipe; the table in its LDS form
hipError_t launch_pack_read_batch(hipStream_t s, int fmt, int n, const void *const (*planes)[3], void *const *outs, uint32_t width, uint32_t height,
                                  const void *cm, const void *gm, const LutView &lv, uint32_t num_cus) {
  const bool v420 = fmt_v420(fmt);
  FmtReadBatchArgs b{};
  for (int i = 0; i < n; ++i) b.p0[i] = planes[i][0], b.p1[i] = planes[i][1], b.p2[i] = planes[i][2], b.out[i] = (float4 *)outs[i];
  b.jobs = (uint32_t)n, b.width = width, b.lines = v420 ? (height / 2) * 2 : height, b.pitch = pack_pitch(fmt, width);
  b.cm = (const float *)cm, b.gm = (const float *)gm, b.nt = image_nt((size_t)width * height * 16);
  return for_fmt(fmt, [&](auto f) { return launch_read_batch_fmt<decltype(f)::value>(s, b, lv, num_cus); });
}

template <int FMT>
static hipError_t launch_write_fmt(hipStream_t s, const FmtWriteArgs &a, const float *table, const LutView *lv,
                                   uint32_t num_cus) {
  const bool rgb = fmt_rgb8(FMT);
  const uint32_t total = rgb ? a.width * a.groups : ((a.width + 7) / 8) * a.groups;
  if (!total) return hipSuccess;
  if (lv) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(fmt_write_lds_kernel<FMT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    const uint32_t want = (total + kLdsBlock - 1) / kLdsBlock;
    fmt_write_lds_kernel<FMT><<<want < num_cus ? want : num_cus, kLdsBlock, lv->bytes, s>>>(a, *lv);
  } else {
    fmt_write_gather_kernel<FMT><<<(total + kFmtBlock - 1) / kFmtBlock, kFmtBlock, 0, s>>>(a, table);
  }
  return hipGetLastError();
}

hipError_t launch_pack_write(hipStream_t s, int fmt, const void *in, void *const planes[3], uint32_t width,
                             uint32_t height, uint32_t interlace, const void *cm, const void *table, const LutView *lv,
                             uint32_t num_cus) {
  const bool v420 = fmt_v420(fmt);
  const uint32_t groups = v420 ? height / 2 : (interlace ? height / 2 : height);  // e.g. yuv422p10.ts:328, yuv420p.ts:381
  FmtWriteArgs a{(const float4 *)in, planes[0], planes[1], planes[2], width, pack_pitch(fmt, width), groups, interlace,
                 (const float *)cm};
  return for_fmt(fmt, [&](auto f) { return launch_write_fmt<decltype(f)::value>(s, a, (const float *)table, lv, num_cus); });
}

hipError_t launch_pack_write_multi(hipStream_t s, const PackMultiArgs &a, uint32_t num_cus) {
  if (!a.lines || !a.width) return hipSuccess;
  if (a.n_out < 1 || a.n_out > (uint32_t)kMaxPackOuts) return hipErrorInvalidValue;
  bool v210 = false;
  for (uint32_t k = 0; k < a.n_out; ++k) {
    const int fmt = (int)a.out[k].fmt;
    if (!fmt_known(fmt) || (fmt == PH_FMT_V210 && a.width % 48u) || (fmt_planar(fmt) && a.width % 8u)) return hipErrorInvalidValue;
    v210 = v210 || fmt == PH_FMT_V210;
  }
  char name[32];
  snprintf(name, sizeof name, "pack_write_multi x%u", a.n_out);
  if (trace_launch(name)) return hipSuccess;
  PackMultiArgs b = a;
  b.units_per_line = (a.width + 7u) / 8u;
  const uint32_t per_wg = (kLdsBlock / 64u) * (v210 ? 63u : 64u);  // octets a workgroup takes at a time
  const uint32_t total = b.units_per_line * b.lines, want = (total + per_wg - 1) / per_wg, grid = want < num_cus ? want : num_cus;
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kLdsBlock, b.wr.bytes, s>>>(b);
    return hipGetLastError();
  };
  return v210 ? go(pack_write_multi_kernel<true>) : go(pack_write_multi_kernel<false>);
}

}  // namespace ph
