// ph_kernels_up.hip - the compositor for MAGNIFYING placements: [transform] x N -> combine_N -> v210 write as one kernel,
// each lane producing a 2 x 2 block of output pixels.
//
// The pixel-per-lane compositor (ph_kernels_lds.hip) loads four 16-byte taps per layer and output pixel; for BASELINE
// config 3 (four 1080 sources shown at 2160) that is 256 bytes through the texture addressers per output pixel, and
// they - not HBM, not the VALU - were what the kernel waited for.  When a layer is magnified without rotation
// (Mixer's default fill of an HD source on a UHD channel: producer/mixer.ts:209-223, transform.ts:36-59), neighbouring
// output pixels share their taps: the four pixels (x, x + 1) x (y, y + 1) with x, y even draw all sixteen taps from a
// 3 x 3 patch of the source.  A lane owns such a block, loads the nine texels once per layer and picks each pixel's
// 2 x 2 sub-patch with selects (columns, per lane) and a uniform branch (rows): 2.25 taps per pixel instead of 4, and with
// sources stored as packed RGB (12 bytes per texel: alpha == 1 is implied for a de-interlaced v210 source,
// ph_v210_yadif_pair_fmt) 27 bytes per layer and pixel instead of 64.  Arithmetic and its order are those of
// transform.ts / combine.ts / v210.ts, pixel by pixel: results are bit-identical to the separate kernels.
//
// Shape: only the writer's table is needed (one phase); one 1024-lane workgroup per CU, persistent.  A wave step is
// 126 columns x 2 rows: 63 lanes x (2 x 2) - 21 v210 quads per row, three lanes to a quad.  The lanes of a quad hand
// their code values to each other with two DPP moves per row (no LDS staging): lane A (pixels 0, 1) and lane C (4, 5)
// each store half of the packed quad, lane B (2, 3) only gives.
#include "ph_device.h"
#include "ph_kernels.h"
#include "ph_ldslut.h"

#include <cstdlib>
#include <type_traits>

#pragma clang fp contract(off)

#ifndef PH_UP_GROUP_ROWS
#define PH_UP_GROUP_ROWS 16
#endif

namespace ph {

#ifndef PH_UP_BLOCK
#define PH_UP_BLOCK 1024
#endif
// lanes per workgroup (one workgroup per CU: the table fills the LDS).  Measured at 2160p x 4 layers: 1024 lanes 64.7 us, 768 lanes
// (three waves per SIMD, 168 registers each) 65.7 us, 512 lanes 78 us; with the next layer's patch requested before this layer's is
// filtered (two patches in flight) 768 lanes 69 us, 512 lanes 72.5 us, 1024 lanes 92 us (31 spilled registers): not a kernel that waits for its loads
constexpr int kUpBlock = PH_UP_BLOCK;
constexpr uint32_t kUpCols = 126;              // output columns of a wave step
constexpr uint32_t kUpOutside = 0x40000000u;   // offsets of texels outside the image: beyond any num_records (images < 1 GiB)

typedef uint32_t ph_u32x3 __attribute__((ext_vector_type(3)));
typedef uint32_t ph_u32x4 __attribute__((ext_vector_type(4)));

struct UpTexel {
  float r, g, b, a;
};
template <bool RGB12>
__device__ __forceinline__ UpTexel up_load(__amdgpu_buffer_rsrc_t img, uint32_t off) {  // outside: 0 = the border colour
  if (RGB12) {
    const ph_u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(img, (int)off, 0, 0);
    UpTexel t;  // .a is not part of a packed-RGB texel (UpPend::cin / rin)
    t.r = __uint_as_float(v.x), t.g = __uint_as_float(v.y), t.b = __uint_as_float(v.z);
    return t;
  }
  const ph_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(img, (int)off, 0, 0);
  return UpTexel{__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
}
__device__ __forceinline__ UpTexel up_pick(bool second, const UpTexel &t0, const UpTexel &t1) {
  return UpTexel{second ? t1.r : t0.r, second ? t1.g : t0.g, second ? t1.b : t0.b, second ? t1.a : t0.a};
}

struct UpShare {  // as ChanShare (ph_kernels_chan.hip): units dealt XCD-aware in groups of output rows, divisions by reciprocal
  uint32_t units, upg, upr, xcd, v0, vstep, vend, slots;
  bool banded;
};
// COLS: the output columns of a wave step - 126 (63 lanes: 21 v210 quads), or 128 (all 64 lanes) in launches without a v210 output
// BLOCK: the lanes of the kernel's workgroup (compose_up_trans_kernel has fewer than the others)
template <uint32_t COLS = kUpCols, uint32_t BLOCK = (uint32_t)kUpBlock>
__device__ __forceinline__ UpShare up_share(const UpArgs &a) {
  UpShare s;
  s.upr = (a.cover_w + COLS - 1u) / COLS;  // wave steps per row pair
  s.units = s.upr * ((a.lines + 1u) / 2u) * a.jobs;  // a further job's row pairs follow the one before's
  s.upg = (uint32_t)(PH_UP_GROUP_ROWS / 2) * s.upr;
  s.banded = (gridDim.x & 7u) == 0;
  s.xcd = 0, s.v0 = blockIdx.x * (BLOCK / 64), s.vstep = gridDim.x * (BLOCK / 64), s.vend = s.units;
  if (s.banded) {
    s.xcd = blockIdx.x & 7u;
    const uint32_t groups = (s.units + s.upg - 1u) / s.upg, mine = (groups + 7u - s.xcd) / 8u;
    s.v0 = (blockIdx.x >> 3) * (BLOCK / 64), s.vstep = (gridDim.x >> 3) * (BLOCK / 64), s.vend = mine * s.upg;
  }
  return s;
}
__device__ __forceinline__ uint32_t up_unit(const UpArgs &a, const UpShare &s, uint32_t v) {
  if (!s.banded) return v < s.units ? v : ~0u;
  const uint32_t gi = __umulhi(v, a.magic_upg);  // v / upg
  const uint32_t unit = (gi * 8u + s.xcd) * s.upg + (v - gi * s.upg);
  return unit < s.units ? unit : ~0u;
}

// one output pixel of a layer: the sampler's filter on its 2 x 2 sub-patch with the four weights of OpenCL 1.2 8.2 as DESIGN.md
// section 2 fixes them (w00 = (1 - a)(1 - b), w10 = a (1 - b), w01 = (1 - a) b, w11 = a b), then combine.ts:45-65 into the pixel's accumulator
struct UpAcc {
  float r, g, b;
};
struct UpWeights {
  float w00, w10, w01, w11;
};
__device__ __forceinline__ UpWeights up_weights(float wa, float wb) {
  const float oma = 1.0f - wa, omb = 1.0f - wb;
  return UpWeights{oma * omb, wa * omb, oma * wb, wa * wb};
}
// `INSIDE` (packed RGB, every texel of every lane's patch inside the image): each texel's alpha is exactly 1, so the filtered alpha
// is the sum of the four weights and 1 - alpha depends on the block's geometry only (UpGeo::kk, computed with it).
// A pixel of a layer in two steps: its filtered colour with what it leaves of the layers below (kk = 1 - alpha) ...
struct UpColour {
  float r, g, b, kk;
};
template <bool RGB12, bool INSIDE, bool FIRST>
__device__ __forceinline__ UpColour up_blend(const UpTexel &t00, const UpTexel &t10, const UpTexel &t01, const UpTexel &t11, const UpWeights &w,
                                             float kk_inside) {
  UpColour c;
  c.r = ((w.w00 * t00.r + w.w10 * t10.r) + w.w01 * t01.r) + w.w11 * t11.r;
  c.g = ((w.w00 * t00.g + w.w10 * t10.g) + w.w01 * t01.g) + w.w11 * t11.g;
  c.b = ((w.w00 * t00.b + w.w10 * t10.b) + w.w01 * t01.b) + w.w11 * t11.b;
  c.kk = kk_inside;  // (the result's alpha is never used by the writer)
  if (!FIRST && !INSIDE) c.kk = 1.0f - (((w.w00 * t00.a + w.w10 * t10.a) + w.w01 * t01.a) + w.w11 * t11.a);
  return c;
}
// ... then combine.ts:45-65 into the pixel's accumulator.  The bottom layer is taken as it is (the kernel peels it off the layer loop);
// above it acc = fma(acc, kk, colour) is the three-operand v_fma_f32 with the accumulator as destination, issued once per pixel
// outside any branch: the accumulators stay in their registers over the layer loop (LLVM's v_fmac into the fresh colour costs a
// v_mov per accumulator and layer, an accumulator merged from two paths another one)
template <bool FIRST>
__device__ __forceinline__ void up_over(const UpColour &c, UpAcc &acc) {
  if (FIRST) {
    acc.r = c.r, acc.g = c.g, acc.b = c.b;
  } else {
    asm volatile("v_fma_f32 %0, %0, %3, %4\n\tv_fma_f32 %1, %1, %3, %5\n\tv_fma_f32 %2, %2, %3, %6"
                 : "+v"(acc.r), "+v"(acc.g), "+v"(acc.b)
                 : "v"(c.kk), "v"(c.r), "v"(c.g), "v"(c.b));
  }
}

// where a wave step lies: 126 columns x 2 rows; the lane's block starts at (x0, line[0])
static_assert(kMaxUpJobs == 4, "up_step finds a row pair's job by three comparisons");
struct UpStep {
  uint32_t job;  // uniform: which of the launch's jobs the row pair belongs to
  uint32_t x0, li[2], line[2];
  float px[2], py[2];
  bool live;
};
// A wave's steps: round k of the share's units is [k * vstep, (k + 1) * vstep), the wave's place in a round v0 + wave.  The LAST round is
// usually partial (2160p: 8.2 rounds) and its units are dealt one per SIMD instead - workgroup first, wave second (the waves of a
// workgroup go round its four SIMDs) - so that the tail runs as single waves on otherwise idle SIMDs all over the chip, not as a few
// CUs with sixteen waves each doing a ninth step.
template <uint32_t COLS = kUpCols, uint32_t BLOCK = (uint32_t)kUpBlock>
__device__ __forceinline__ bool up_step(const UpArgs &a, const UpShare &sh, uint32_t &base, uint32_t wave, uint32_t lane, UpStep &st) {
  while (base < sh.vend) {
    const uint32_t left = sh.vend - base, nwg = sh.vstep / (BLOCK / 64), wg = sh.v0 / (BLOCK / 64);
    const uint32_t pos = left >= sh.vstep ? sh.v0 + wave : wg + nwg * wave;
    const uint32_t v = base + pos;
    base += sh.vstep;
    if (pos >= left) continue;  // uniform
    const uint32_t unit = up_unit(a, sh, v);
    if (unit == ~0u) continue;  // uniform
    uint32_t rp = sh.upr == 1u ? unit : __umulhi(unit, a.magic_upr);  // unit / upr
    const uint32_t col_unit = unit - rp * sh.upr, rp_per_job = (a.lines + 1u) / 2u;
    st.job = (rp >= rp_per_job ? 1u : 0u) + (rp >= 2u * rp_per_job ? 1u : 0u) + (rp >= 3u * rp_per_job ? 1u : 0u);  // kMaxUpJobs == 4
    rp -= st.job * rp_per_job;
    st.x0 = col_unit * COLS + 2u * lane;  // even
    st.live = (COLS == 128u || lane < 63u) && st.x0 < a.out_w;  // lane 63 has no quad; the row's last step may be short
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      st.li[dy] = 2u * rp + (uint32_t)dy < a.lines ? 2u * rp + (uint32_t)dy : 2u * rp;  // an odd field's last row is its own partner
      st.line[dy] = a.first_line + st.li[dy] * a.line_step;
      st.py[dy] = (float)(int)st.line[dy] / (float)(int)a.out_h - 0.5f;  // transform.ts:53
    }
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) st.px[dx] = (float)(int)(st.x0 + (uint32_t)dx) / (float)(int)a.out_w - 0.5f;
    return true;
  }
  return false;
}

// Where a layer's 3 x 3 patch lies for the lane's block and how each of the four pixels weighs its 2 x 2 sub-patch: everything
// that depends on the placement and the source's SIZE but not on its pixels.  Layers of one size under one placement (the
// four full-frame HD sources of a UHD channel) share it: computed for the first, reused for the rest.
struct UpGeo {
  uint32_t coff[3];  // per lane: byte offsets of the patch's columns inside a row, or kUpOutside
  uint32_t roff[3];  // uniform: byte offsets of its rows, or kUpOutside
  UpWeights w[2][2];  // [output row][output column]
  float kk[2][2];    // packed RGB with every texel inside: 1 - (the filtered alpha = the sum of the weights, each times exactly 1)
  bool d1;           // per lane: the right pixel's first tap is one texel further than the left pixel's
  bool dj;           // uniform: likewise the lower row's
  bool all_inside;   // uniform (packed RGB): every texel of every lane's patch is inside the image
  uint32_t cin;      // packed RGB, per lane: bit c = patch column c is inside the image
  uint32_t rin;      // packed RGB, uniform: bit r = patch row r is inside
};
template <bool RGB12>
__device__ __forceinline__ UpGeo up_geo(const UpLayer &L, const UpStep &st) {
  constexpr uint32_t kTexel = RGB12 ? 12u : 16u;
  UpGeo g;
  // columns (per lane): transform.ts:53-57 with m1 == 0 (host-checked): fma(py, 0, px * m0) == px * m0 for every finite py
  uint32_t i0[2];
  float wa[2], wb[2];
#pragma unroll
  for (int dx = 0; dx < 2; ++dx) {
    const float sx = dot3(L.m[0], L.m[1], L.m[2], st.px[dx], st.py[0], 1.0f) + 0.5f;
    const float fu = sx * (float)(int)L.w - 0.5f, flu = __builtin_floorf(fu);
    i0[dx] = (uint32_t)(int)flu, wa[dx] = fu - flu;
  }
  // rows (the same for every lane: m3 == 0, host-checked; computed on the lane's own operands, read from one lane)
  uint32_t j0[2];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const float sy = dot3(L.m[3], L.m[4], L.m[5], st.px[0], st.py[dy], 1.0f) + 0.5f;
    const float fv = sy * (float)(int)L.h - 0.5f, flv = __builtin_floorf(fv);
    j0[dy] = (uint32_t)__builtin_amdgcn_readfirstlane((int)flv);
    wb[dy] = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(fv - flv)));
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      g.w[dy][dx] = up_weights(wa[dx], wb[dy]);
      const UpWeights &q = g.w[dy][dx];
      g.kk[dy][dx] = RGB12 ? 1.0f - (((q.w00 + q.w10) + q.w01) + q.w11) : 0.0f;
    }
  // the 3 x 3 patch: columns i0[0] .. + 2 (i0[1] - i0[0] is 0 or 1 for a magnification of 2 or more), rows j0[0] .. + 2
  g.d1 = i0[1] != i0[0];
  g.dj = j0[1] != j0[0];
  bool cin[3], rin[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t col = i0[0] + (uint32_t)c;
    cin[c] = col < L.w;
    g.coff[c] = cin[c] ? __umul24(col, kTexel) : kUpOutside;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const uint32_t row = j0[0] + (uint32_t)r;
    rin[r] = row < L.h;
    g.roff[r] = rin[r] ? row * L.pitch : kUpOutside;  // uniform
  }
  g.all_inside = false, g.cin = 0, g.rin = 0;
  if (RGB12) {  // alpha of a packed-RGB texel: 1 inside the image, 0 (the border colour) outside - made when the patch is filtered
    const bool mine = cin[0] && cin[1] && cin[2];
    g.all_inside = rin[0] && rin[1] && rin[2] && __builtin_amdgcn_ballot_w64(!mine) == 0;  // uniform
    g.cin = (cin[0] ? 1u : 0u) | (cin[1] ? 2u : 0u) | (cin[2] ? 4u : 0u);
    g.rin = (rin[0] ? 1u : 0u) | (rin[1] ? 2u : 0u) | (rin[2] ? 4u : 0u);
  }
  return g;
}
// one layer in two halves: its nine texels are requested, then the four pixels are filtered and combined
struct UpPatch {
  UpTexel P[3][3];
};
template <bool RGB12>
__device__ __forceinline__ void up_fetch(const UpLayer &L, const UpGeo &g, UpPatch &p) {
  const __amdgpu_buffer_rsrc_t img = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(L.ptr), 0, (int)(L.pad ? L.pad : L.pitch * L.h), 0x00020000);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) p.P[r][c] = up_load<RGB12>(img, g.roff[r] + g.coff[c]);
}
// PH_UP_PRICE_INDEX builds (tools/config3_price.py; timing only, WRONG pixels, never shipped): what it would cost this kernel if the
// fields' KEPT lines - half of a field's lines are copies of the source frame's - arrived as three 16-bit reader-table indices
// instead of three floats (first candidate): every such texel then needs the reader's three table lookups and its
// gamut matrix here.  Five of a patch's nine texels get that arithmetic (on average 4.5 lie on kept lines).
#ifndef PH_UP_PRICE_INDEX
#define PH_UP_PRICE_INDEX 0
#endif
template <bool RGB12, bool INSIDE, bool FIRST>
__device__ __forceinline__ void up_filter(const UpPatch &p, const UpGeo &g, UpAcc (&acc)[2][2], const LutK &price_lut) {
  UpTexel P[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P[r][c] = p.P[r][c];
#if PH_UP_PRICE_INDEX
      if (r == 0 || (r == 2 && c < 2)) {
        const float lr = lds_lut_at_unit(price_lut, P[r][c].r), lg = lds_lut_at_unit(price_lut, P[r][c].g), lb = lds_lut_at_unit(price_lut, P[r][c].b);
        P[r][c].r = dot3(lr, lg, lb, 0.6274f, 0.3293f, 0.0433f), P[r][c].g = dot3(lr, lg, lb, 0.0691f, 0.9195f, 0.0114f);
        P[r][c].b = dot3(lr, lg, lb, 0.0164f, 0.0880f, 0.8956f);
      }
#endif
      if (RGB12) P[r][c].a = (!INSIDE && ((g.rin >> r) & 1u) && ((g.cin >> c) & 1u)) ? 1.0f : 0.0f;  // unused when all are inside
    }
  const bool d1 = g.d1;
  // upper output row: patch rows 0, 1; left pixel: columns 0, 1; right pixel: columns d1, d1 + 1
  up_over<FIRST>(up_blend<RGB12, INSIDE, FIRST>(P[0][0], P[0][1], P[1][0], P[1][1], g.w[0][0], g.kk[0][0]), acc[0][0]);
  up_over<FIRST>(up_blend<RGB12, INSIDE, FIRST>(up_pick(d1, P[0][0], P[0][1]), up_pick(d1, P[0][1], P[0][2]), up_pick(d1, P[1][0], P[1][1]),
                                                up_pick(d1, P[1][1], P[1][2]), g.w[0][1], g.kk[0][1]), acc[0][1]);
  // lower output row: patch rows dj, dj + 1 (a uniform branch: no selects)
  UpColour lo0, lo1;
  if (g.dj) {
    lo0 = up_blend<RGB12, INSIDE, FIRST>(P[1][0], P[1][1], P[2][0], P[2][1], g.w[1][0], g.kk[1][0]);
    lo1 = up_blend<RGB12, INSIDE, FIRST>(up_pick(d1, P[1][0], P[1][1]), up_pick(d1, P[1][1], P[1][2]), up_pick(d1, P[2][0], P[2][1]),
                                         up_pick(d1, P[2][1], P[2][2]), g.w[1][1], g.kk[1][1]);
  } else {
    lo0 = up_blend<RGB12, INSIDE, FIRST>(P[0][0], P[0][1], P[1][0], P[1][1], g.w[1][0], g.kk[1][0]);
    lo1 = up_blend<RGB12, INSIDE, FIRST>(up_pick(d1, P[0][0], P[0][1]), up_pick(d1, P[0][1], P[0][2]), up_pick(d1, P[1][0], P[1][1]),
                                         up_pick(d1, P[1][1], P[1][2]), g.w[1][1], g.kk[1][1]);
  }
  up_over<FIRST>(lo0, acc[1][0]);
  up_over<FIRST>(lo1, acc[1][1]);
}

// The half of a packed quad that lane A (role 0: w0, w1) or lane C (role 2: w2, w3) stores, from the lane's own four code values and
// lane B's gifts: to A (the lane before it) Cb2 << 10 | Y2 << 20, to C (the lane after it) Cr2 | Y3 << 10.  Every lane of the wave calls it.
__device__ __forceinline__ uint2 up_v210_half(uint32_t ey, uint32_t eu, uint32_t ev, uint32_t y1, uint32_t role) {
  const uint32_t to_prev = eu << 10 | ey << 20, to_next = ev | y1 << 10;
  const uint32_t from_next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)to_prev, 0x130 /* wave_shl:1: lane i reads lane i + 1 */, 0xf, 0xf, false);
  const uint32_t from_prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)to_next, 0x138 /* wave_shr:1: lane i reads lane i - 1 */, 0xf, 0xf, false);
  if (role == 0u) return make_uint2(ev << 20 | ey << 10 | eu, from_next | y1);  // w0, w1
  return make_uint2(eu << 20 | from_prev, y1 << 20 | ev << 10 | ey);            // w2, w3 (lane C)
}

// writer (v210.ts:145-162) of the lane's block: the even pixel gives Y, Cb, Cr, the odd one Y; then the quad's three lanes trade halves
// TAILS: lines that do not end on a 48-pixel block (1280: src/config.ts:43-54) - `full` whole quads, the tail quad of out_w % 6 = 2 or 4
// pixels with the reference's tail arithmetic (table indices truncated, code values through round() and a truncating convert, the words
// it does not set 0: v210.ts:166-193), then the slots it clears up to the pitch (:131-136).  A lane beyond the line's pixels contributes
// zero code values, so the same hand-overs and stores make the tail quad's unset words and the cleared slots.
template <bool TAILS>
__device__ __forceinline__ void up_write(const UpArgs &a, const UpStep &st, const UpAcc (&acc)[2][2], uint32_t role, const WriteK &wk, const LutK &lk,
                                         void *frame = nullptr) {  // frame: the step's output frame, where the caller knows it (else by st.job)
  const uint32_t qpl = TAILS ? a.out_qpitch : a.out_w / 6u;
  const uint32_t quad = st.x0 / 6u, full = a.out_w / 6u;
  const bool in_tail = TAILS && quad == full, beyond = TAILS && st.x0 >= a.out_w;  // (a tail's pixels are inside: beyond is false for them)
  // the twelve table reads of the block's four pixels are started together
  PxPending pend[2][2];
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      auto index_of = [&](float t) __attribute__((always_inline)) { return TAILS ? lds_lut_index_unit_tail(t, in_tail) : lds_lut_index_unit(t); };
      pend[dy][dx] = write_px_issue(index_of(acc[dy][dx].r), index_of(acc[dy][dx].g), index_of(acc[dy][dx].b), lk);
    }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const float er = lds_lut_finish(pend[dy][0].r), eg = lds_lut_finish(pend[dy][0].g), eb = lds_lut_finish(pend[dy][0].b);
    const float orr = lds_lut_finish(pend[dy][1].r), og = lds_lut_finish(pend[dy][1].g), ob = lds_lut_finish(pend[dy][1].b);
    auto code = [&](float v) __attribute__((always_inline)) {
      if (!TAILS) return sat_u16_rte(v);
      const uint32_t c = in_tail ? sat_u16_trunc(__builtin_roundf(v)) : sat_u16_rte(v);
      return beyond ? 0u : c;
    };
    const uint32_t ey = code(dot4(er, eg, eb, 1.0f, wk.y)), eu = code(dot4(er, eg, eb, 1.0f, wk.u)), ev = code(dot4(er, eg, eb, 1.0f, wk.v));
    const uint32_t y1 = code(dot4(orr, og, ob, 1.0f, wk.y));
    const uint2 half = up_v210_half(ey, eu, ev, y1, role);
    // (TAILS: every quad slot of the pitch is written - the tail quad's unset words and the cleared slots come out of the zero lanes)
    const bool store = (TAILS ? (threadIdx.x & 63u) < 63u && quad < qpl : st.live) && role != 1u && (dy == 0 || st.li[1] != st.li[0]);
    if (store) {
      // ONE eight-byte store per lane: the wave's lanes A and C then cover their row segment without a gap, every 32-byte sector
      // written whole and once.  (As two dword stores each instruction wrote every other dword and each sector went out twice,
      // half filled: WRITE_SIZE 36.7 MB for a 22.1 MB frame, profiles/r03_pmc_up.txt.)
      typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
      ph_u2v *dst = reinterpret_cast<ph_u2v *>(reinterpret_cast<uint4 *>(frame ? frame : st.job ? a.more_out[st.job - 1u] : a.out) + (size_t)st.line[dy] * qpl + st.x0 / 6u) + (role == 2u ? 1 : 0);
      __builtin_nontemporal_store(ph_u2v{half.x, half.y}, dst);
    }
  }
}

template <bool RGB12, bool TAILS = false>
__global__ __launch_bounds__(kUpBlock) void compose_up_write_v210_kernel(UpArgs a) {
  const WriteK wk = load_write_k(a.wr_cm);
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kUpBlock>(a.wr);
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const UpShare sh = up_share(a);
  const uint32_t role = lane - 3u * (lane / 3u);  // 0: pixels 0, 1 of the quad, 1: pixels 2, 3, 2: pixels 4, 5
  UpStep st;
  for (uint32_t base = 0; up_step(a, sh, base, wave, lane, st);) {
    // (lowering a wave's priority as it advances, which helps the two-phase kernels reach their barrier together, measured neutral here)
    UpAcc acc[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) acc[dy][dx] = UpAcc{0.0f, 0.0f, 0.0f};
    // (up_layers below is a copy of this loop for compose_up_multi_kernel: keep the two in step)
    // one layer at a time.  Variants built and measured slower at 2160p x 4 layers: layers in pairs with both patches in
    // flight (76 against 70 us; again with the shared geometry: 84 against 68 us, 128 registers and spills) and a patch
    // carried in flight across loop turns (85 us) - two patches plus the writer's temporaries do not fit 128 registers
    // The bottom layer is peeled off the loop (it is taken as it is; above it the accumulators are updated in place), and the loop
    // exists three times - shared geometry with every texel inside (packed RGB: no alpha arithmetic at all), shared geometry, a
    // geometry per layer - so that inside a loop nothing about an accumulator is decided by a branch
    UpGeo geo;
    auto layers = [&](auto inside_tag, auto shared_tag) __attribute__((always_inline)) {
      constexpr bool INSIDE = decltype(inside_tag)::value, SHARED = decltype(shared_tag)::value;
      {
        UpLayer L = a.layer[0];  // one 48-byte scalar load
        if (st.job) L.ptr = a.more_ptr[st.job - 1u][0];
        if (!SHARED) geo = up_geo<RGB12>(L, st);
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, true>(p, geo, acc, lk);
      }
#pragma unroll 1
      for (int l = 1; l < a.n; ++l) {
        UpLayer L = a.layer[l];
        if (st.job) L.ptr = a.more_ptr[st.job - 1u][l];
        if (!SHARED) geo = up_geo<RGB12>(L, st);
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, false>(p, geo, acc, lk);
      }
    };
    if (a.shared) {  // uniform
      geo = up_geo<RGB12>(a.layer[0], st);
      if (RGB12 && geo.all_inside) layers(std::true_type{}, std::true_type{});  // uniform
      else layers(std::false_type{}, std::true_type{});
    } else {
      layers(std::false_type{}, std::false_type{});
    }
    up_write<TAILS>(a, st, acc, role, wk, lk);
  }
}

// ---- several consumers' frames of ONE enlarged composition per launch ---------------------------------------------------------------
// A channel's consumers each run their own FromRGBA on the one combined image (channel.ts:64-88: v210 for SDI, rgba8 for the screen,
// yuv422p8 for an encoder).  The writers differ only AFTER the table lookups (ph_kernels_chan.hip chan_phase2_other: same indices, same
// table, another matrix and packing), and the block's four pixels are in registers when the writer is reached: the twelve table reads
// are made once, then every output packs the same twelve values with its own matrix.  A block with even x and y is one 4:2:0 chroma site.
// Every output of a launch names the launch's ONE table (the kernel is persistent and single-phase: no point at which all waves could
// swap it), and rounds its indices - a v210 output whose lines end in a tail quad, which truncates them there, is launched on its own
// by the caller (compose_up_write_v210_kernel<RGB12, true>) - or, with the context option "up_v210_tails", stays in the kernels' TAILS
// form (up_write_outs_tails below).
//
// Stores.  rgba8 / bgra8 store 8 bytes per lane and row - a wave's row segment without a gap, as the v210 halves; the planar writers
// store the lane's two luma samples (2 or 4 bytes) and its one chroma site per plane (1 or 2 bytes), again contiguous over the wave's
// lanes, through the cache.  With the v210 writer's 126-column step (63 lanes, three to a quad) two neighbouring wave steps share the
// sector at every step boundary - 126 is no multiple of 32 - so launches WITHOUT a v210 output take a 128-column step (COLS = 128, all
// 64 lanes): a wave's store instruction then covers 128 or 256 contiguous bytes of luma and 64 or 128 of a chroma plane, which are
// whole, aligned 32-byte sectors where the row pitch is a multiple of 32 luma samples (64 for the 8-bit 4:2:0 chroma planes) - 1920 and
// 3840 are; the entry asks for a multiple of 8 only, and other widths share a sector between rows as any writer's would.
// Of the two ways to whole sectors this one was built; trading samples by DPP into 8-byte stores (which would also serve launches that
// have a v210 output) was not.  Measured, four packed-RGB 1080p images, one output
// (tools/up_out_bench.py, two processes; the separate side agrees to 0.4 us between them): 128 against 126 columns - yuv420p 27.8 against
// 28.0 us, yuv422p8 28.4 against 28.4, rgba8 27.5 against 27.5 (profiles/up_out_bench.jsonl, profiles/up_out_bench_step126.jsonl): the
// 128-column step is never slower and 0.2 us (0.8 %, three times the spread) faster for the 4:2:0 writer - it is the one taken.
//
// The writer matrices are loaded per output and wave step (load_write_k: twelve scalar loads from the scalar cache).  Loading all four
// outputs' matrices once per wave in front of the step loop was built and dropped on the compiler's own figures: 48 more values live over
// the loop take the kernel from 110 / 114 to 128 vector registers with 35 - 38 of them spilled (160 - 176 bytes of scratch per lane)
// at 1024 lanes - the scalar file is full (106) either way (profiles/up_out_resources.txt).
__device__ __forceinline__ bool up_out_takes(const UpOut &o, uint32_t line) { return line < o.line_end && (o.takes == 0u || (line & 1u) + 1u == o.takes); }

// A wave step's layers, bottom to top, into the block's four accumulators (zero on entry): the layer loop of compose_up_write_v210_kernel,
// which keeps its own copy - called from here that kernel's registers are allocated differently, and its code is pinned
// (profiles/up_out_resources.txt)
template <bool RGB12>
__device__ __forceinline__ void up_layers(const UpArgs &a, const UpStep &st, UpAcc (&acc)[2][2], const LutK &lk) {
  // one layer at a time.  Variants built and measured slower at 2160p x 4 layers: layers in pairs with both patches in
  // flight (76 against 70 us; again with the shared geometry: 84 against 68 us, 128 registers and spills) and a patch
  // carried in flight across loop turns (85 us) - two patches plus the writer's temporaries do not fit 128 registers
  // The bottom layer is peeled off the loop (it is taken as it is; above it the accumulators are updated in place), and the loop
  // exists three times - shared geometry with every texel inside (packed RGB: no alpha arithmetic at all), shared geometry, a
  // geometry per layer - so that inside a loop nothing about an accumulator is decided by a branch
  UpGeo geo;
  auto layers = [&](auto inside_tag, auto shared_tag) __attribute__((always_inline)) {
    constexpr bool INSIDE = decltype(inside_tag)::value, SHARED = decltype(shared_tag)::value;
    {
      UpLayer L = a.layer[0];  // one 48-byte scalar load
      if (st.job) L.ptr = a.more_ptr[st.job - 1u][0];
      if (!SHARED) geo = up_geo<RGB12>(L, st);
      UpPatch p;
      up_fetch<RGB12>(L, geo, p);
      up_filter<RGB12, INSIDE, true>(p, geo, acc, lk);
    }
#pragma unroll 1
    for (int l = 1; l < a.n; ++l) {
      UpLayer L = a.layer[l];
      if (st.job) L.ptr = a.more_ptr[st.job - 1u][l];
      if (!SHARED) geo = up_geo<RGB12>(L, st);
      UpPatch p;
      up_fetch<RGB12>(L, geo, p);
      up_filter<RGB12, INSIDE, false>(p, geo, acc, lk);
    }
  };
  if (a.shared) {  // uniform
    geo = up_geo<RGB12>(a.layer[0], st);
    if (RGB12 && geo.all_inside) layers(std::true_type{}, std::true_type{});  // uniform
    else layers(std::false_type{}, std::true_type{});
  } else {
    layers(std::false_type{}, std::false_type{});
  }
}

// TAILS (a v210 output of a launch whose lines end in a tail quad and cleared slots - the TAILS forms of the several-outputs kernels, whose
// wave steps cover the pitch): up_write<true>'s line ends.  `t` holds the tail quad's lanes' values from TRUNCATED indices (the caller's
// second set); their codes go through round() and the truncating convert, a lane beyond the line's pixels contributes zero code values, and
// lanes A and C of every quad slot of the pitch store (o.pitch: the pitch in quad slots).  The other writers of such a launch are called as
// ever: a lane beyond the line is not live and stores nothing for them.
template <int OUT, bool TAILS = false>
__device__ __forceinline__ void up_write_out(const UpOut &o, const UpStep &st, const float (&t)[2][2][3], uint32_t role, uint32_t out_w = 0) {
  constexpr bool WIDE = fmt_wide(OUT), V420 = fmt_v420(OUT), NV12 = fmt_cbcr(OUT);
  char *const p0 = static_cast<char *>(o.plane[st.job][0]);
  WriteK wk;
  if (!fmt_rgb8(OUT)) wk = load_write_k(o.wr_cm);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const uint32_t line = st.line[dy];
    if (!((dy == 0 || st.li[1] != st.li[0]) && up_out_takes(o, line))) continue;  // uniform
    const float *const e = t[dy][0], *const d = t[dy][1];  // the even pixel, the odd one
    if (fmt_rgb8(OUT)) {  // rgba8.ts:69-101
      typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
      const ph_u2v px{rgb8_pack<OUT>(e[0], e[1], e[2]), rgb8_pack<OUT>(d[0], d[1], d[2])};
      if (st.live) __builtin_nontemporal_store(px, reinterpret_cast<ph_u2v *>(p0 + ((size_t)line * o.pitch + st.x0) * 4u));
      continue;
    }
    if (TAILS && OUT == PH_FMT_V210) {  // up_write<true>: the tail quad's codes, zeros beyond the line, every quad slot of the pitch stored
      typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
      const uint32_t quad = st.x0 / 6u;
      const bool in_tail = quad == out_w / 6u, beyond = st.x0 >= out_w;
      auto code = [&](const float *px, const float4 row) __attribute__((always_inline)) {
        const float v = dot4(px[0], px[1], px[2], 1.0f, row);
        const uint32_t c = in_tail ? sat_u16_trunc(__builtin_roundf(v)) : sat_u16_rte(v);
        return beyond ? 0u : c;
      };
      const uint2 half = up_v210_half(code(e, wk.y), code(e, wk.u), code(e, wk.v), code(d, wk.y), role);
      ph_u2v *dst = reinterpret_cast<ph_u2v *>(reinterpret_cast<uint4 *>(p0) + (size_t)line * o.pitch + quad) + (role == 2u ? 1 : 0);
      if ((threadIdx.x & 63u) < 63u && quad < o.pitch && role != 1u) __builtin_nontemporal_store(ph_u2v{half.x, half.y}, dst);
      continue;
    }
    // chroma from the even pixel (v210.ts:145-162 and every planar writer)
    const uint32_t ey = ycbcr_code(e[0], e[1], e[2], wk.y), eu = ycbcr_code(e[0], e[1], e[2], wk.u), ev = ycbcr_code(e[0], e[1], e[2], wk.v);
    const uint32_t y1 = ycbcr_code(d[0], d[1], d[2], wk.y);
    if (OUT == PH_FMT_V210) {  // (every lane trades, then lanes A and C store: up_write)
      typedef uint32_t ph_u2v __attribute__((ext_vector_type(2)));
      const uint2 half = up_v210_half(ey, eu, ev, y1, role);
      ph_u2v *dst = reinterpret_cast<ph_u2v *>(reinterpret_cast<uint4 *>(p0) + (size_t)line * o.pitch + st.x0 / 6u) + (role == 2u ? 1 : 0);
      if (st.live && role != 1u) __builtin_nontemporal_store(ph_u2v{half.x, half.y}, dst);
      continue;
    }
    if (!st.live) continue;
    // planar (yuv422p10.ts:140-189, yuv422p8.ts:166-168, yuv420p.ts:150-216, nv12.ts:139-196): codes cut to the sample width on store
    const size_t at = (size_t)line * o.pitch + st.x0;  // in luma samples; even
    if (WIDE) *reinterpret_cast<uint32_t *>(p0 + at * 2u) = ey | y1 << 16;
    else *reinterpret_cast<uint16_t *>(p0 + at) = (uint16_t)((ey & 0xffu) | (y1 & 0xffu) << 8);
    char *const p1 = static_cast<char *>(o.plane[st.job][1]), *const p2 = static_cast<char *>(o.plane[st.job][2]);
    if (V420) {  // a chroma line serves a line pair: from the pair's upper line, or from the one line of the pair that a field writes
      if (!(o.field || !(line & 1u))) continue;  // uniform
      const size_t cat = (size_t)(line >> 1) * o.pitch + st.x0;
      if (NV12) *reinterpret_cast<uint16_t *>(p1 + cat) = (uint16_t)((eu & 0xffu) | (ev & 0xffu) << 8);
      else p1[cat >> 1] = (char)(eu & 0xffu), p2[cat >> 1] = (char)(ev & 0xffu);
    } else if (WIDE) {
      *reinterpret_cast<uint16_t *>(p1 + at) = (uint16_t)eu, *reinterpret_cast<uint16_t *>(p2 + at) = (uint16_t)ev;
    } else {
      p1[at >> 1] = (char)(eu & 0xffu), p2[at >> 1] = (char)(ev & 0xffu);
    }
  }
}

// The writers of a wave step in the TAILS forms of compose_up_multi_kernel and clip_up_multi_kernel (context option "up_v210_tails"): a v210
// output whose lines end in a tail quad (out_w % 48 != 0; 1280: src/config.ts:43-54) beside the rounding writers of its table.  The twelve
// table reads are made once for all outputs as ever.  In the ONE wave step of a row pair that holds the tail quad's pixels (a wave-uniform
// test: every other step runs the reads above and nothing more) twelve more reads give the v210 outputs their second set - the tail quad's
// lanes from truncated indices (v210.ts:176-178), every other lane its rounded values again.  (The channel kernel's way - the rounded index
// is the truncated one plus 0 or 1, ph_kernels_chan.hip - saves those reads in a kernel that waits for the LDS; this one does not, and the
// step is one of ten or more per row pair.)
__device__ __forceinline__ void up_write_outs_tails(uint32_t out_w, const UpStep &st, const UpAcc (&acc)[2][2], uint32_t n_out, const UpOut *out, uint32_t role,
                                                    const LutK &lk) {
  float t[2][2][3], tv[2][2][3];
  {
    PxPending pend[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        pend[dy][dx] = write_px_issue(lds_lut_index_unit(acc[dy][dx].r), lds_lut_index_unit(acc[dy][dx].g), lds_lut_index_unit(acc[dy][dx].b), lk);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
  }
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) tv[dy][dx][ch] = t[dy][dx][ch];
  const bool in_tail = st.x0 / 6u == out_w / 6u && st.x0 < out_w;  // the lane's block belongs to the tail quad (none where out_w % 6 == 0)
  if (__builtin_amdgcn_ballot_w64(in_tail) != 0) {  // uniform: the step that holds the tail quad
    PxPending pend[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        pend[dy][dx] = write_px_issue(lds_lut_index_unit_tail(acc[dy][dx].r, in_tail), lds_lut_index_unit_tail(acc[dy][dx].g, in_tail),
                                      lds_lut_index_unit_tail(acc[dy][dx].b, in_tail), lk);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        tv[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), tv[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), tv[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
  }
  // (left to the compiler whether to unroll: with the pragma of the kernels' own copies of this loop it answers "loop not unrolled" here)
  for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
    if (k >= n_out) break;  // uniform
    const UpOut &o = out[k];
    switch (o.fmt) {  // uniform
      case PH_FMT_V210: up_write_out<PH_FMT_V210, true>(o, st, tv, role, out_w); break;
      case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
      case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
      case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
      case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
      case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
      case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
    }
  }
}

// TAILS: a v210 output's lines end in a tail quad and cleared slots (an instantiation of its own, 126 columns: the existing forms keep
// their text and their registers, profiles/up_tails_resources.txt).  The wave steps cover the pitch (up_plan), a lane beyond the line's
// pixels composes whatever its taps give (loads are bounded by the buffer's records) and up_write_outs_tails lets none of it out.
template <bool RGB12, uint32_t COLS, bool TAILS = false>
__global__ __launch_bounds__(kUpBlock) void compose_up_multi_kernel(UpMultiArgs m) {
  const UpArgs &a = m.up;
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kUpBlock>(a.wr);
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const UpShare sh = up_share<COLS>(a);
  const uint32_t role = lane - 3u * (lane / 3u);
  UpStep st;
  for (uint32_t base = 0; up_step<COLS>(a, sh, base, wave, lane, st);) {
    UpAcc acc[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) acc[dy][dx] = UpAcc{0.0f, 0.0f, 0.0f};
    up_layers<RGB12>(a, st, acc, lk);
    if (TAILS) {
      up_write_outs_tails(a.out_w, st, acc, m.n_out, m.out, role, lk);
      continue;
    }
    // the twelve table reads of the block's four pixels, started together - once for all outputs
    float t[2][2][3];
    {
      PxPending pend[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          pend[dy][dx] = write_px_issue(lds_lut_index_unit(acc[dy][dx].r), lds_lut_index_unit(acc[dy][dx].g), lds_lut_index_unit(acc[dy][dx].b), lk);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
      if (k >= m.n_out) break;  // uniform
      const UpOut &o = m.out[k];
      switch (o.fmt) {  // uniform
        case PH_FMT_V210: up_write_out<PH_FMT_V210>(o, st, t, role); break;
        case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
        case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
        case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
        case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
        case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
        case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
      }
    }
  }
}

// ---- layers in a TRANSITION: [transform -> dissolve | wipe against a second source] x N -> combine_N -> the writers, one launch --------
// The Transitioner (transitioner.ts:165-176) puts transition.ts's dissolve or wipe between a layer's transform and the Combiner, with
// the incoming source - and a wipe's mask - transformed by matrices of their own.  Here a layer's four block pixels are made as VALUES
// (r, g, b and the filtered alpha: a transition mixes alpha like any channel, so the INSIDE shortcut of up_blend holds for no layer
// that has one), the partner images are filtered one after the other into the same sixteen registers - one patch in flight at any time -
// and the result goes over the accumulators as any layer's does.  Arithmetic and order are transition.ts's:
//   dissolve  v = fma(src, mix, incoming * (1 - mix))           wipe  v = fma(incoming, m, src * (1 - m)),  m = the mask's red
// with (1 - mix), (1 - m) and the products beside the fma each rounded once.  A wipe's mask is filtered BEFORE its incoming image (the
// order of the loads is nobody's business): src * (1 - m) then replaces src, and only those sixteen values and the four m wait for the
// incoming patch - with the incoming image first, thirty-two values would.
template <bool RGB12, typename F>
__device__ __forceinline__ void up_values(const UpPatch &p, const UpGeo &g, F each) {
  UpTexel P[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P[r][c] = p.P[r][c];
      if (RGB12) P[r][c].a = (((g.rin >> r) & 1u) && ((g.cin >> c) & 1u)) ? 1.0f : 0.0f;  // packed RGB: alpha 1 inside, the border's 0 outside
    }
  auto value = [](const UpTexel &t00, const UpTexel &t10, const UpTexel &t01, const UpTexel &t11, const UpWeights &w) __attribute__((always_inline)) {
    UpTexel v;
    v.r = ((w.w00 * t00.r + w.w10 * t10.r) + w.w01 * t01.r) + w.w11 * t11.r;
    v.g = ((w.w00 * t00.g + w.w10 * t10.g) + w.w01 * t01.g) + w.w11 * t11.g;
    v.b = ((w.w00 * t00.b + w.w10 * t10.b) + w.w01 * t01.b) + w.w11 * t11.b;
    v.a = ((w.w00 * t00.a + w.w10 * t10.a) + w.w01 * t01.a) + w.w11 * t11.a;
    return v;
  };
  const bool d1 = g.d1;
  each(0, 0, value(P[0][0], P[0][1], P[1][0], P[1][1], g.w[0][0]));
  each(0, 1, value(up_pick(d1, P[0][0], P[0][1]), up_pick(d1, P[0][1], P[0][2]), up_pick(d1, P[1][0], P[1][1]), up_pick(d1, P[1][1], P[1][2]), g.w[0][1]));
  UpTexel lo0, lo1;
  if (g.dj) {  // uniform, as up_filter
    lo0 = value(P[1][0], P[1][1], P[2][0], P[2][1], g.w[1][0]);
    lo1 = value(up_pick(d1, P[1][0], P[1][1]), up_pick(d1, P[1][1], P[1][2]), up_pick(d1, P[2][0], P[2][1]), up_pick(d1, P[2][1], P[2][2]), g.w[1][1]);
  } else {
    lo0 = value(P[0][0], P[0][1], P[1][0], P[1][1], g.w[1][0]);
    lo1 = value(up_pick(d1, P[0][0], P[0][1]), up_pick(d1, P[0][1], P[0][2]), up_pick(d1, P[1][0], P[1][1]), up_pick(d1, P[1][1], P[1][2]), g.w[1][1]);
  }
  each(1, 0, lo0);
  each(1, 1, lo1);
}

// layer l of the step's job as the Combiner gets it: the block's four pixels after transform and transition
template <bool RGB12>
__device__ __forceinline__ void up_trans_layer(const UpTransArgs &m, const UpStep &st, int l, UpTexel (&v)[2][2]) {
  const UpArgs &a = m.multi.up;
  UpLayer L = a.layer[l];
  if (st.job) L.ptr = a.more_ptr[st.job - 1u][l];
  UpGeo geo = up_geo<RGB12>(L, st);
  {
    UpPatch p;
    up_fetch<RGB12>(L, geo, p);
    up_values<RGB12>(p, geo, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) { v[dy][dx] = t; });
  }
  const uint32_t kind = m.kind[l], same = m.same[l];  // uniform
  if (kind == PH_TRANSITION_CUT) return;
  // a partner of the layer's size and placement is filtered with the layer's geometry; any other brings its own, which takes the
  // layer's place (the layer is filtered by then) - and is replaced in its turn if the next partner is like the layer again
  bool geo_is_layers = true;
  auto partner = [&](int which, auto each) __attribute__((always_inline)) {
    UpLayer P = m.partner[l][which];
    if (st.job) P.ptr = m.more_partner[st.job - 1u][l][which];
    const bool like_layer = (same >> which) & 1u;
    if (!(like_layer && geo_is_layers)) geo = up_geo<RGB12>(P, st);  // uniform
    geo_is_layers = like_layer;
    UpPatch p;
    up_fetch<RGB12>(P, geo, p);
    up_values<RGB12>(p, geo, each);
  };
  if (kind == PH_TRANSITION_WIPE) {
    float mr[2][2];
    partner(1, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
      const float mk = t.r, rm = 1.0f - mk;
      UpTexel &s = v[dy][dx];
      mr[dy][dx] = mk, s.r = s.r * rm, s.g = s.g * rm, s.b = s.b * rm, s.a = s.a * rm;
    });
    partner(0, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
      const float mk = mr[dy][dx];
      UpTexel &s = v[dy][dx];
      s.r = fma_rn(t.r, mk, s.r), s.g = fma_rn(t.g, mk, s.g), s.b = fma_rn(t.b, mk, s.b), s.a = fma_rn(t.a, mk, s.a);
    });
  } else {
    const float mix = m.mix[st.job][l], rmix = 1.0f - mix;  // uniform
    partner(0, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
      UpTexel &s = v[dy][dx];
      s.r = fma_rn(s.r, mix, t.r * rmix), s.g = fma_rn(s.g, mix, t.g * rmix), s.b = fma_rn(s.b, mix, t.b * rmix), s.a = fma_rn(s.a, mix, t.a * rmix);
    });
  }
}

// compose_up_multi_kernel with up_trans_layer's layers; everything behind the layer loop is that kernel's, kept in step by hand (its
// code is pinned - profiles/up_trans_resources.txt - so the two do not share a function that it would have to be rebuilt around)
//
// Lanes.  A transitioning layer's sixteen values (and a wipe's four mask values) live beside the accumulators while the partner's patch
// is fetched and filtered: at 1024 lanes (128 vector registers) 52 - 56 of them are spilled, 288 - 316 bytes of scratch per lane; at
// 768 lanes (three waves per SIMD, 168 registers) 7 - 10 and 124 - 144 bytes (profiles/up_trans_resources.txt).  Timed, four packed 1080p
// fields with a dissolve and a wipe on a 1080p channel: 1024 lanes 81.1 us, 768 lanes 54.2 us, 512 lanes (no spills, two waves per
// SIMD) 65.7 us; both fields of a tick 140.9 / 100.9 / 116.4; config 3's 2160p frame with one dissolve 120.9 / 122.5 / 148.9
// (profiles/up_transition_lanes.jsonl): 768 lanes it is.
#ifndef PH_UP_TRANS_BLOCK
#define PH_UP_TRANS_BLOCK 768
#endif
constexpr int kUpTransBlock = PH_UP_TRANS_BLOCK;
template <bool RGB12, uint32_t COLS>
__global__ __launch_bounds__(kUpTransBlock) void compose_up_trans_kernel(UpTransArgs tr) {
  const UpMultiArgs &m = tr.multi;
  const UpArgs &a = m.up;
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kUpTransBlock>(a.wr);
  __syncthreads();
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const UpShare sh = up_share<COLS, (uint32_t)kUpTransBlock>(a);
  const uint32_t role = lane - 3u * (lane / 3u);
  UpStep st;
  for (uint32_t base = 0; up_step<COLS, (uint32_t)kUpTransBlock>(a, sh, base, wave, lane, st);) {
    UpAcc acc[2][2];
    {  // the bottom layer is taken as it is - with a transition: the transition's value as it is
      UpTexel v[2][2];
      up_trans_layer<RGB12>(tr, st, 0, v);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) acc[dy][dx] = UpAcc{v[dy][dx].r, v[dy][dx].g, v[dy][dx].b};
    }
#pragma unroll 1
    for (int l = 1; l < a.n; ++l) {
      UpTexel v[2][2];
      up_trans_layer<RGB12>(tr, st, l, v);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) up_over<false>(UpColour{v[dy][dx].r, v[dy][dx].g, v[dy][dx].b, 1.0f - v[dy][dx].a}, acc[dy][dx]);  // combine.ts:45-65
    }
    float t[2][2][3];
    {
      PxPending pend[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          pend[dy][dx] = write_px_issue(lds_lut_index_unit(acc[dy][dx].r), lds_lut_index_unit(acc[dy][dx].g), lds_lut_index_unit(acc[dy][dx].b), lk);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
      if (k >= m.n_out) break;  // uniform
      const UpOut &o = m.out[k];
      switch (o.fmt) {  // uniform
        case PH_FMT_V210: up_write_out<PH_FMT_V210>(o, st, t, role); break;
        case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
        case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
        case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
        case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
        case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
        case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Clips straight from their wire formats: [read] x N -> [transform] x N -> combine_N -> v210 write as ONE launch.
// The two-launch route (reader of the format into an f32 image, then the kernel above) sends every clip's image out of the chip and
// back - 6 x the frame's compulsory bytes for a 720p clip on a 1080p channel - and pays launch, table load and drain twice for two
// kernels of ten microseconds each.  Here a workgroup owns a TILE of the output (tcu wave-step columns x trp row pairs).  Phase 1, the
// reader's table in the LDS: the source pixels the tile's taps fall on are converted once each (v210.ts:58-78 / yuv420p.ts ... the
// reader's own arithmetic, a wave per source row) into a rectangle of the workgroup's own scratch, which never leaves the XCD's L2.
// Phase 2, the writer's table swapped in: the kernel above, its nine-texel patches taken from the rectangle.
// ------------------------------------------------------------------------------------------------------------------------------------
// PH_CLIP_ABLATE builds (timing experiments, never shipped): bit 0 = stop after phase 1, bit 1 = phase 1 converts nothing, bit 2 = no phase 2 work
#ifndef PH_CLIP_ABLATE
#define PH_CLIP_ABLATE 0
#endif
// one source pixel as the reader of its format makes it (ph_kernels_fmt.hip fmt_read_body, ph_kernels_lds.hip v210_read_lds_kernel), in two
// halves: its samples requested, then converted - a lane requests the samples of all its pixels of a round before it converts the first
// (a rectangle is a handful of pixels per lane: one at a time, every pixel would wait out its own trip to HBM)
struct ClipRaw {
  uint4 w;  // v210: the pixel's word quad; the other formats: fmt_fetch's codes
};
template <int FMT>
__device__ __forceinline__ ClipRaw clip_fetch(const ClipSrc &S, uint32_t x, uint32_t line) {
  ClipRaw r;
  if (FMT == PH_FMT_V210) r.w = reinterpret_cast<const uint4 *>(S.p0)[(size_t)line * S.pitch + x / 6u];
  else r.w = fmt_fetch<FMT>(S.p0, S.p1, S.p2, S.pitch, x, line);
  return r;
}
template <int FMT>
__device__ __forceinline__ float4 clip_finish(const ClipRaw &raw, uint32_t width, uint32_t x, const ReadK &k, const LutK &lk) {
  if (FMT == PH_FMT_V210) {
    const uint4 w = raw.w;
    const uint32_t g = x / 6u, j = x - 6u * g, pr = j >> 1;
    const uint32_t wy = (j == 0) ? w.x : (j < 3) ? w.y : (j == 3) ? w.z : w.w;  // v210.ts:58-63, as v210_read_lds_kernel
    const uint32_t sy = (j == 0 || j == 3) ? 10u : (j == 1 || j == 4) ? 0u : 20u;
    const uint32_t wcb = pr == 0 ? w.x : pr == 1 ? w.y : w.z;
    const uint32_t wcr = pr == 0 ? w.x : pr == 1 ? w.z : w.w;
    const uint32_t scr = pr == 0 ? 20u : pr == 1 ? 0u : 10u;
    const float yf = (float)((wy >> sy) & 0x3ff), cbf = (float)((wcb >> (10u * pr)) & 0x3ff), crf = (float)((wcr >> scr) & 0x3ff);
    return read_px_lds(yf, cbf, crf, k, lk, x < width - width % 6u ? 1.0f : 0.0f);  // (a line's tail: v210.ts:88-93)
  }
  if (fmt_rgb8(FMT)) {
    const uint32_t p = raw.w.x;
    const float c0 = (float)(p & 0xffu), gf = (float)((p >> 8) & 0xffu), c2 = (float)((p >> 16) & 0xffu), af = (float)(p >> 24);
    return rgb8_to_rgba(FMT == PH_FMT_RGBA8 ? c0 : c2, gf, FMT == PH_FMT_RGBA8 ? c2 : c0, af, k, LutInLds{lk});
  }
  // (yuv422p10.ts:74-78: dot4 with the offset column, table, gamut - the v210 reader's arithmetic)
  return read_px_lds((float)raw.w.x, (float)raw.w.y, (float)raw.w.z, k, lk, 1.0f);
}

// The first tap (column / row) of an output pixel, exactly as up_geo computes it: monotone in the pixel's position (every step is a
// correctly rounded monotone operation), so a tile's first and last pixels bound the taps of everything between them.
__device__ __forceinline__ int clip_tap_col(const UpLayer &L, uint32_t x, uint32_t out_w) {
  const float px = (float)(int)x / (float)(int)out_w - 0.5f;
  const float sx = dot3(L.m[0], L.m[1], L.m[2], px, 0.0f, 1.0f) + 0.5f;
  return (int)__builtin_floorf(sx * (float)(int)L.w - 0.5f);
}
__device__ __forceinline__ int clip_tap_row(const UpLayer &L, uint32_t line, uint32_t out_h) {
  const float py = (float)(int)line / (float)(int)out_h - 0.5f;
  const float sy = dot3(L.m[3], L.m[4], L.m[5], 0.0f, py, 1.0f) + 0.5f;
  return (int)__builtin_floorf(sy * (float)(int)L.h - 0.5f);
}
struct ClipRect {  // uniform: the source rectangle of a tile, inside the image (w == 0: nothing of the image under this tile)
  uint32_t c0, r0, w, h;
};

// FIRST: the launch's first rectangle.  Its first round of samples is requested BEFORE the reader's table is loaded (the table load and the
// samples' trip to HBM overlap), and the table load + barrier happen in here.  Within a rectangle a round's samples are requested before
// the round before it is converted.
// BLOCK: the lanes of the kernel's workgroup (clip_up_trans_kernel is built with fewer too)
template <int FMT, bool RGB12, bool FIRST, int BLOCK = kUpBlock>
__device__ __forceinline__ void clip_convert(const ClipSrc &S, const UpLayer &L, const ClipRect &R, char *dst, uint32_t ppitch, const float *rd_gm, const LutK &rlk,
                                             const LutView &rd_view) {
  // the rectangle's pixels row by row over all the workgroup's lanes, kClipRound of them per lane and round
  constexpr int kClipRound = FMT == PH_FMT_V210 ? 4 : 6;  // (a 720p clip on a 1080p channel: 4.3 K pixels per workgroup - one round)
  const uint32_t total = R.w * R.h;  // (< 2^24: exact as a float)
  const float inv_w = 1.0f / (float)(R.w ? R.w : 1u);
  struct Round {
    ClipRaw raw[kClipRound];
    uint32_t col[kClipRound], row[kClipRound];
  };
  auto request = [&](uint32_t base, Round &q) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < kClipRound; ++i) {
      const uint32_t idx = base + (uint32_t)i * BLOCK < total ? base + (uint32_t)i * BLOCK : total - 1u;  // (lanes past the end redo the last pixel)
      uint32_t r = (uint32_t)((float)idx * inv_w);  // idx / R.w, off by one at most
      r -= r * R.w > idx ? 1u : 0u;
      r += (r + 1u) * R.w <= idx ? 1u : 0u;
      q.row[i] = r, q.col[i] = idx - r * R.w;
      q.raw[i] = clip_fetch<FMT>(S, R.c0 + q.col[i], R.r0 + r);
    }
  };
  Round cur;
  if (total) request(threadIdx.x, cur);  // (uniform)
  if (FIRST) {
    lds_lut_load<BLOCK>(rd_view);
    __syncthreads();
  }
  ReadK k;
  if (fmt_rgb8(FMT)) {
#pragma unroll
    for (int i = 0; i < 9; ++i) k.gm[i] = rd_gm[i];
  } else {
    k = load_read_k(S.cm, rd_gm);
  }
  for (uint32_t base = threadIdx.x; base < total; base += kClipRound * BLOCK) {
    Round nxt = cur;
    const uint32_t next_base = base + kClipRound * BLOCK;
    if (next_base - threadIdx.x < total) request(next_base < total ? next_base : total - 1u, nxt);  // (uniform test: the whole workgroup takes the round or not)
#pragma unroll
    for (int i = 0; i < kClipRound; ++i) {
      const float4 t = clip_finish<FMT>(cur.raw[i], L.w, R.c0 + cur.col[i], k, rlk);
      char *at = dst + (size_t)cur.row[i] * ppitch + (size_t)cur.col[i] * (RGB12 ? 12u : 16u);
      if (RGB12) *reinterpret_cast<ph_u32x3 *>(at) = ph_u32x3{__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z)};
      else *reinterpret_cast<float4 *>(at) = t;
    }
    cur = nxt;
  }
}

// a wave step of a tile: as up_step makes it for (col_unit, row pair) of job 0
__device__ __forceinline__ void clip_step(const UpArgs &a, uint32_t job, uint32_t col_unit, uint32_t rp, uint32_t lane, UpStep &st) {
  st.job = job;
  st.x0 = col_unit * kUpCols + 2u * lane;
  st.live = lane < 63u && st.x0 < a.out_w;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    st.li[dy] = 2u * rp + (uint32_t)dy < a.lines ? 2u * rp + (uint32_t)dy : 2u * rp;
    st.line[dy] = a.first_line + st.li[dy] * a.line_step;
    st.py[dy] = (float)(int)st.line[dy] / (float)(int)a.out_h - 0.5f;
  }
#pragma unroll
  for (int dx = 0; dx < 2; ++dx) st.px[dx] = (float)(int)(st.x0 + (uint32_t)dx) / (float)(int)a.out_w - 0.5f;
}

// MULTI: several frames of one shape in the launch (an instantiation of its own: a job index alive through both phases costs the
// one-frame kernel eight spilled registers and 1.3 us, measured)
template <bool RGB12, bool TAILS, bool MULTI = false>
__global__ __launch_bounds__(kUpBlock) void clip_up_write_v210_kernel(ClipUpArgs c) {
  const UpArgs &a = c.up;
  constexpr uint32_t kTexel = RGB12 ? 12u : 16u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // the tile
  const uint32_t upr = (a.cover_w + kUpCols - 1u) / kUpCols, rps = (a.lines + 1u) / 2u;
  const uint32_t tyj = blockIdx.x / c.gx, tx = blockIdx.x - tyj * c.gx;
  const uint32_t job = MULTI ? tyj / c.gy : 0u, ty = tyj - job * c.gy;  // (uniform) several frames of one shape: rows of tiles job after job
  const uint32_t cu0 = tx * c.tcu, rp0 = ty * c.trp;
  const uint32_t ncu = cu0 + c.tcu <= upr ? c.tcu : upr - cu0, nrp = rp0 + c.trp <= rps ? c.trp : rps - rp0;
  char *const mine = c.scratch + (size_t)blockIdx.x * c.wg_bytes;
  // ---- phase 1: the reader's table; every layer's rectangle converted
  const LutK rlk = make_lut_k(c.rd);
  uint4 *const info = reinterpret_cast<uint4 *>(g_lds + c.info_off);
#pragma unroll 1
  for (int l = 0; l < a.n; ++l) {
    const UpLayer L = a.layer[l];
    const ClipSrc S = c.src[MULTI ? job : (uint32_t)l];  // (several jobs: single-layer frames, job j's clip in src[j])
    // the tile's first and last pixels (inside the frame: columns past out_w - the padding of a line with a tail - have no taps that count)
    const uint32_t x_first = cu0 * kUpCols, x_end = (cu0 + ncu) * kUpCols < a.out_w ? (cu0 + ncu) * kUpCols : a.out_w;
    const uint32_t li_last = 2u * (rp0 + nrp) < a.lines ? 2u * (rp0 + nrp) - 1u : a.lines - 1u;
    ClipRect R{0, 0, 0, 0};
    if (x_first < x_end) {
      int c_lo = clip_tap_col(L, x_first, a.out_w), c_hi = clip_tap_col(L, x_end - 1u, a.out_w) + 2;  // (a block's patch: three columns from its left pixel's first tap)
      int r_lo = clip_tap_row(L, a.first_line + 2u * rp0 * a.line_step, a.out_h), r_hi = clip_tap_row(L, a.first_line + li_last * a.line_step, a.out_h) + 2;
      c_lo = c_lo < 0 ? 0 : c_lo, r_lo = r_lo < 0 ? 0 : r_lo;
      c_hi = c_hi >= (int)L.w ? (int)L.w - 1 : c_hi, r_hi = r_hi >= (int)L.h ? (int)L.h - 1 : r_hi;
      if (c_hi >= c_lo && r_hi >= r_lo) R = ClipRect{(uint32_t)c_lo, (uint32_t)r_lo, (uint32_t)(c_hi - c_lo + 1), (uint32_t)(r_hi - r_lo + 1)};
    }
    R.c0 = __builtin_amdgcn_readfirstlane(R.c0), R.r0 = __builtin_amdgcn_readfirstlane(R.r0);
    R.w = __builtin_amdgcn_readfirstlane(R.w), R.h = __builtin_amdgcn_readfirstlane(R.h);
    const uint32_t ppitch = R.w * kTexel;
    if (ppitch && R.h * ppitch > c.rect_cap[l]) R.h = c.rect_cap[l] / ppitch;  // (the launcher's bound holds: never taken)
    char *const dst = mine + c.rect_off[l];
#if PH_CLIP_ABLATE & 2  // timing experiment only (wrong pixels): nothing converted
    R.h = 0;
#endif
#define PH_CLIP_CASE(F)                                                                                   \
  case F:                                                                                                  \
    if (l == 0) clip_convert<F, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                    \
    else clip_convert<F, RGB12, false>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                          \
    break;
    switch (S.fmt) {  // uniform
      PH_CLIP_CASE(PH_FMT_V210)
      PH_CLIP_CASE(PH_FMT_YUV422P10)
      PH_CLIP_CASE(PH_FMT_YUV422P8)
      PH_CLIP_CASE(PH_FMT_YUV420P)
      PH_CLIP_CASE(PH_FMT_NV12)
      PH_CLIP_CASE(PH_FMT_YUV420P10)
      PH_CLIP_CASE(PH_FMT_P010)
      PH_CLIP_CASE(PH_FMT_RGBA8)
      default:
        if (l == 0) clip_convert<PH_FMT_BGRA8, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        else clip_convert<PH_FMT_BGRA8, RGB12, false>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        break;
    }
#undef PH_CLIP_CASE
    // the layer as phase 2 sees it: texel (col, row) of the IMAGE at base + row * ppitch + col * kTexel (only texels of the rectangle are ever
    // taken: everything else of a patch is outside the image, an offset beyond the buffer's records)
    if (threadIdx.x == 0) {
      const uint64_t base = (uint64_t)(uintptr_t)dst - ((uint64_t)R.r0 * ppitch + (uint64_t)R.c0 * kTexel);
      info[l] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), ppitch ? ppitch : kTexel, 0u);
    }
  }
#if PH_CLIP_ABLATE & 1  // timing experiment only: phase 1 alone
  return;
#endif
  // ---- the swap: every wave's rectangle rows are in L2 (a workgroup's stores are visible to its own later loads), the writer's table comes in
  __threadfence_block();
  __syncthreads();
  const WriteK wk = load_write_k(a.wr_cm);
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kUpBlock>(a.wr);
  __syncthreads();
  // ---- phase 2: the 2 x 2-block compositor on the tile's wave steps
  const uint32_t role = lane - 3u * (lane / 3u);
  auto layer_of = [&](int l) __attribute__((always_inline)) {
    UpLayer L = a.layer[l];
    const uint4 d = info[l];  // uniform address: one broadcast read
    const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.y) << 32;
    L.ptr = reinterpret_cast<const void *>((uintptr_t)base);
    L.pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.z);
    L.pad = kUpOutside - 16u;  // the buffer's records: rows are ppitch apart but columns count from the IMAGE's left edge, so pitch * h is no bound here
    return L;
  };
#if PH_CLIP_ABLATE & 4
  const uint32_t units = 0;
#else
  const uint32_t units = ncu * nrp;
#endif
  void *const frame = MULTI && job ? a.more_out[job - 1u] : a.out;  // (uniform: the tile's frame)
  for (uint32_t u = wave; u < units; u += kUpBlock / 64) {
    const uint32_t rp_in = ncu == 1u ? u : u / ncu, cu_in = u - rp_in * ncu;
    UpStep st;
    clip_step(a, 0u, cu0 + cu_in, rp0 + rp_in, lane, st);
    UpAcc acc[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) acc[dy][dx] = UpAcc{0.0f, 0.0f, 0.0f};
    UpGeo geo;
    auto layers = [&](auto inside_tag, auto shared_tag) __attribute__((always_inline)) {
      constexpr bool INSIDE = decltype(inside_tag)::value, SHARED = decltype(shared_tag)::value;
      {
        const UpLayer L = layer_of(0);
        if (!SHARED) geo = up_geo<RGB12>(L, st);  // (shared: layers of one size and placement have rectangles of one shape, their bases aside)
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, true>(p, geo, acc, lk);
      }
#pragma unroll 1
      for (int l = 1; l < a.n; ++l) {
        const UpLayer L = layer_of(l);
        if (!SHARED) geo = up_geo<RGB12>(L, st);
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, false>(p, geo, acc, lk);
      }
    };
    if (a.shared) {  // uniform
      geo = up_geo<RGB12>(layer_of(0), st);
      if (RGB12 && geo.all_inside) layers(std::true_type{}, std::true_type{});
      else layers(std::false_type{}, std::true_type{});
    } else {
      layers(std::false_type{}, std::false_type{});
    }
    up_write<TAILS>(a, st, acc, role, wk, lk, frame);
  }
}

// ---- the same clips for ANY consumer, up to four per launch -----------------------------------------------------------------------------
// File playback that feeds an encoder or the screen beside SDI (or instead of it): clip_up_write_v210_kernel's phase 1 and table swap,
// its wave-step loop up to the block's four accumulators, and from there compose_up_multi_kernel's tail - the twelve writer-table reads
// made once, then every output packing the same twelve values with its own matrix (up_write_out).  Both kernels keep their own text
// (their code is pinned: profiles/up_out_resources.txt, profiles/clip_multi_resources.txt), so the two halves are copies kept in step by
// hand.  One frame per launch unless MULTI (job 0's planes of every output: clip_step's job is 0); the wave step is the clip kernel's 126 columns for
// every launch, a v210 output or not, so the tiling and the rectangle bounds of clip_up_plan hold as they are.  A v210 output's lines end
// on a 48-pixel block here (the caller sends the others through the one-output routes: their tail quads truncate table indices) -
// unless TAILS.
// MULTI: several frames of one shape in the launch, as clip_up_write_v210_kernel's MULTI - rows of tiles job after job, job j's clip in
// src[j], its planes o.plane[j] of every output (an instantiation of its own: the one-frame forms keep their text and their registers,
// profiles/clip_multi_batch_resources.txt)
// TAILS: a v210 output's lines end in a tail quad and cleared slots (instantiations of their own, as compose_up_multi_kernel's): the tiles
// cover the pitch (clip_up_plan with v210_tails), the rectangle bounds clamp to the line's pixels as clip_up_write_v210_kernel<.., TAILS>'s
// do, and up_write_outs_tails is the writer.
template <bool RGB12, bool MULTI = false, bool TAILS = false>
__global__ __launch_bounds__(kUpBlock) void clip_up_multi_kernel(ClipUpMultiArgs cm) {
  const ClipUpArgs &c = cm.clip;
  const UpArgs &a = c.up;
  constexpr uint32_t kTexel = RGB12 ? 12u : 16u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // the tile
  const uint32_t upr = (a.cover_w + kUpCols - 1u) / kUpCols, rps = (a.lines + 1u) / 2u;
  const uint32_t tyj = blockIdx.x / c.gx, tx = blockIdx.x - tyj * c.gx;
  const uint32_t job = MULTI ? tyj / c.gy : 0u, ty = tyj - job * c.gy;  // (uniform) several frames of one shape: rows of tiles job after job
  const uint32_t cu0 = tx * c.tcu, rp0 = ty * c.trp;
  const uint32_t ncu = cu0 + c.tcu <= upr ? c.tcu : upr - cu0, nrp = rp0 + c.trp <= rps ? c.trp : rps - rp0;
  char *const mine = c.scratch + (size_t)blockIdx.x * c.wg_bytes;
  // ---- phase 1: the reader's table; every layer's rectangle converted
  const LutK rlk = make_lut_k(c.rd);
  uint4 *const info = reinterpret_cast<uint4 *>(g_lds + c.info_off);
#pragma unroll 1
  for (int l = 0; l < a.n; ++l) {
    const UpLayer L = a.layer[l];
    const ClipSrc S = c.src[MULTI ? job : (uint32_t)l];  // (several jobs: single-layer frames, job j's clip in src[j])
    const uint32_t x_first = cu0 * kUpCols, x_end = (cu0 + ncu) * kUpCols < a.out_w ? (cu0 + ncu) * kUpCols : a.out_w;
    const uint32_t li_last = 2u * (rp0 + nrp) < a.lines ? 2u * (rp0 + nrp) - 1u : a.lines - 1u;
    ClipRect R{0, 0, 0, 0};
    if (x_first < x_end) {
      int c_lo = clip_tap_col(L, x_first, a.out_w), c_hi = clip_tap_col(L, x_end - 1u, a.out_w) + 2;
      int r_lo = clip_tap_row(L, a.first_line + 2u * rp0 * a.line_step, a.out_h), r_hi = clip_tap_row(L, a.first_line + li_last * a.line_step, a.out_h) + 2;
      c_lo = c_lo < 0 ? 0 : c_lo, r_lo = r_lo < 0 ? 0 : r_lo;
      c_hi = c_hi >= (int)L.w ? (int)L.w - 1 : c_hi, r_hi = r_hi >= (int)L.h ? (int)L.h - 1 : r_hi;
      if (c_hi >= c_lo && r_hi >= r_lo) R = ClipRect{(uint32_t)c_lo, (uint32_t)r_lo, (uint32_t)(c_hi - c_lo + 1), (uint32_t)(r_hi - r_lo + 1)};
    }
    R.c0 = __builtin_amdgcn_readfirstlane(R.c0), R.r0 = __builtin_amdgcn_readfirstlane(R.r0);
    R.w = __builtin_amdgcn_readfirstlane(R.w), R.h = __builtin_amdgcn_readfirstlane(R.h);
    const uint32_t ppitch = R.w * kTexel;
    if (ppitch && R.h * ppitch > c.rect_cap[l]) R.h = c.rect_cap[l] / ppitch;  // (the launcher's bound holds: never taken)
    char *const dst = mine + c.rect_off[l];
#define PH_CLIP_CASE(F)                                                                                   \
  case F:                                                                                                  \
    if (l == 0) clip_convert<F, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                    \
    else clip_convert<F, RGB12, false>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                          \
    break;
    switch (S.fmt) {  // uniform
      PH_CLIP_CASE(PH_FMT_V210)
      PH_CLIP_CASE(PH_FMT_YUV422P10)
      PH_CLIP_CASE(PH_FMT_YUV422P8)
      PH_CLIP_CASE(PH_FMT_YUV420P)
      PH_CLIP_CASE(PH_FMT_NV12)
      PH_CLIP_CASE(PH_FMT_YUV420P10)
      PH_CLIP_CASE(PH_FMT_P010)
      PH_CLIP_CASE(PH_FMT_RGBA8)
      default:
        if (l == 0) clip_convert<PH_FMT_BGRA8, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        else clip_convert<PH_FMT_BGRA8, RGB12, false>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        break;
    }
#undef PH_CLIP_CASE
    if (threadIdx.x == 0) {  // the layer as phase 2 sees it (clip_up_write_v210_kernel)
      const uint64_t base = (uint64_t)(uintptr_t)dst - ((uint64_t)R.r0 * ppitch + (uint64_t)R.c0 * kTexel);
      info[l] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), ppitch ? ppitch : kTexel, 0u);
    }
  }
  // ---- the swap: every wave's rectangle rows are in L2, the writer's table comes in
  __threadfence_block();
  __syncthreads();
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kUpBlock>(a.wr);
  __syncthreads();
  // ---- phase 2: the 2 x 2-block compositor on the tile's wave steps, every output's writer behind it
  const uint32_t role = lane - 3u * (lane / 3u);
  auto layer_of = [&](int l) __attribute__((always_inline)) {
    UpLayer L = a.layer[l];
    const uint4 d = info[l];  // uniform address: one broadcast read
    const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.y) << 32;
    L.ptr = reinterpret_cast<const void *>((uintptr_t)base);
    L.pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.z);
    L.pad = kUpOutside - 16u;
    return L;
  };
  const uint32_t units = ncu * nrp;
  for (uint32_t u = wave; u < units; u += kUpBlock / 64) {
    const uint32_t rp_in = ncu == 1u ? u : u / ncu, cu_in = u - rp_in * ncu;
    UpStep st;
    clip_step(a, job, cu0 + cu_in, rp0 + rp_in, lane, st);  // (up_write_out writes o.plane[st.job])
    UpAcc acc[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) acc[dy][dx] = UpAcc{0.0f, 0.0f, 0.0f};
    UpGeo geo;
    auto layers = [&](auto inside_tag, auto shared_tag) __attribute__((always_inline)) {
      constexpr bool INSIDE = decltype(inside_tag)::value, SHARED = decltype(shared_tag)::value;
      {
        const UpLayer L = layer_of(0);
        if (!SHARED) geo = up_geo<RGB12>(L, st);
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, true>(p, geo, acc, lk);
      }
#pragma unroll 1
      for (int l = 1; l < a.n; ++l) {
        const UpLayer L = layer_of(l);
        if (!SHARED) geo = up_geo<RGB12>(L, st);
        UpPatch p;
        up_fetch<RGB12>(L, geo, p);
        up_filter<RGB12, INSIDE, false>(p, geo, acc, lk);
      }
    };
    if (a.shared) {  // uniform
      geo = up_geo<RGB12>(layer_of(0), st);
      if (RGB12 && geo.all_inside) layers(std::true_type{}, std::true_type{});
      else layers(std::false_type{}, std::true_type{});
    } else {
      layers(std::false_type{}, std::false_type{});
    }
    if (TAILS) {
      up_write_outs_tails(a.out_w, st, acc, cm.n_out, cm.out, role, lk);
      continue;
    }
    // the twelve table reads of the block's four pixels, started together - once for all outputs (compose_up_multi_kernel)
    float t[2][2][3];
    {
      PxPending pend[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          pend[dy][dx] = write_px_issue(lds_lut_index_unit(acc[dy][dx].r), lds_lut_index_unit(acc[dy][dx].g), lds_lut_index_unit(acc[dy][dx].b), lk);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
      if (k >= cm.n_out) break;  // uniform
      const UpOut &o = cm.out[k];
      switch (o.fmt) {  // uniform
        case PH_FMT_V210: up_write_out<PH_FMT_V210>(o, st, t, role); break;
        case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
        case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
        case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
        case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
        case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
        case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
      }
    }
  }
}

// ---- ONE clip in a TRANSITION, for any consumer: a playlist's MIX or WIPE from one file to the next -------------------------------------
// The Transitioner's frame of file playback (transitioner.ts:165-176): one layer whose `src` clip dissolves or wipes into an `incoming` clip,
// a wipe through a mask clip - two or three decoders' frames, each with a size and a placement of its own.  Phase 1 is clip_up_multi_kernel's
// with up to three rectangles per tile - slot 0 src, slot 1 incoming, slot 2 the mask - each bounded by its own image's taps and converted by
// its own format's reader, all in front of the one table swap; phase 2 is up_trans_layer's arithmetic (compose_up_trans_kernel) on patches
// taken from the rectangles, then compose_up_multi_kernel's twelve table reads and every output's up_write_out.  This is a THIRD copy of
// those texts, kept in step by hand: the kernels it copies from are pinned (profiles/clip_multi_resources.txt, profiles/up_trans_resources.txt)
// and are not rebuilt around shared functions.
// A frame of one layer: what the transition leaves IS the frame, and no writer reads its alpha - the alpha arithmetic of up_values and of the
// mixes below is written out as transition.ts has it and dropped by the compiler.
//
// Lanes.  compose_up_trans_kernel runs 768 lanes because a transitioning layer's sixteen values spill at 1024; here only twelve are alive
// (no alpha) and neither 1024 lanes (119 vector registers of 128) nor 768 (125 of 168) spills one or uses scratch
// (profiles/clip_trans_resources.txt).  Timed on the one-launch route, 1024 against 768 lanes: two 1080p yuv420p files dissolving on a
// 1080p channel -> nv12 33.4 / 36.3 us, -> v210 + rgba8 35.2 / 38.6; a 720p file into a 1080p one 30.3 / 34.3; two 1080p p010 files on
// 2160p -> yuv422p10 65.8 / 76.7; a wipe through a 960 x 540 v210 mask 40.6 / 43.6 (profiles/clip_transition_lanes.jsonl; spreads up to
// 1.2 us): 1024 lanes it is, the clip kernels' kUpBlock - clip_up_plan's tiling counts rounds of sixteen waves.
#ifndef PH_CLIP_TRANS_BLOCK
#define PH_CLIP_TRANS_BLOCK 1024
#endif
constexpr int kClipTransBlock = PH_CLIP_TRANS_BLOCK;
static_assert(kMaxLayers >= 3, "clip_up_trans_plan plans the three slots as three layers");
template <bool RGB12>
__global__ __launch_bounds__(kClipTransBlock) void clip_up_trans_kernel(ClipUpTransArgs tr) {
  const ClipUpMultiArgs &cm = tr.multi;
  const ClipUpArgs &c = cm.clip;
  const UpArgs &a = c.up;
  constexpr uint32_t kTexel = RGB12 ? 12u : 16u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // the tile
  const uint32_t upr = (a.cover_w + kUpCols - 1u) / kUpCols, rps = (a.lines + 1u) / 2u;
  const uint32_t ty = blockIdx.x / c.gx, tx = blockIdx.x - ty * c.gx;
  const uint32_t cu0 = tx * c.tcu, rp0 = ty * c.trp;
  const uint32_t ncu = cu0 + c.tcu <= upr ? c.tcu : upr - cu0, nrp = rp0 + c.trp <= rps ? c.trp : rps - rp0;
  char *const mine = c.scratch + (size_t)blockIdx.x * c.wg_bytes;
  const int slots = tr.kind == (uint32_t)PH_TRANSITION_WIPE ? 3 : 2;  // uniform
  // ---- phase 1: the reader's table; every present image's rectangle converted
  const LutK rlk = make_lut_k(c.rd);
  uint4 *const info = reinterpret_cast<uint4 *>(g_lds + c.info_off);
#pragma unroll 1
  for (int s = 0; s < slots; ++s) {
    const UpLayer L = s ? tr.partner[s - 1] : a.layer[0];
    const ClipSrc S = s ? tr.partner_src[s - 1] : c.src[0];
    const uint32_t x_first = cu0 * kUpCols, x_end = (cu0 + ncu) * kUpCols < a.out_w ? (cu0 + ncu) * kUpCols : a.out_w;
    const uint32_t li_last = 2u * (rp0 + nrp) < a.lines ? 2u * (rp0 + nrp) - 1u : a.lines - 1u;
    ClipRect R{0, 0, 0, 0};
    if (x_first < x_end) {
      int c_lo = clip_tap_col(L, x_first, a.out_w), c_hi = clip_tap_col(L, x_end - 1u, a.out_w) + 2;
      int r_lo = clip_tap_row(L, a.first_line + 2u * rp0 * a.line_step, a.out_h), r_hi = clip_tap_row(L, a.first_line + li_last * a.line_step, a.out_h) + 2;
      c_lo = c_lo < 0 ? 0 : c_lo, r_lo = r_lo < 0 ? 0 : r_lo;
      c_hi = c_hi >= (int)L.w ? (int)L.w - 1 : c_hi, r_hi = r_hi >= (int)L.h ? (int)L.h - 1 : r_hi;
      if (c_hi >= c_lo && r_hi >= r_lo) R = ClipRect{(uint32_t)c_lo, (uint32_t)r_lo, (uint32_t)(c_hi - c_lo + 1), (uint32_t)(r_hi - r_lo + 1)};
    }
    R.c0 = __builtin_amdgcn_readfirstlane(R.c0), R.r0 = __builtin_amdgcn_readfirstlane(R.r0);
    R.w = __builtin_amdgcn_readfirstlane(R.w), R.h = __builtin_amdgcn_readfirstlane(R.h);
    const uint32_t ppitch = R.w * kTexel;
    if (ppitch && R.h * ppitch > c.rect_cap[s]) R.h = c.rect_cap[s] / ppitch;  // (the launcher's bound holds: never taken)
    char *const dst = mine + c.rect_off[s];
#define PH_CLIP_CASE(F)                                                                                                   \
  case F:                                                                                                                  \
    if (s == 0) clip_convert<F, RGB12, true, kClipTransBlock>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                   \
    else clip_convert<F, RGB12, false, kClipTransBlock>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);                         \
    break;
    switch (S.fmt) {  // uniform
      PH_CLIP_CASE(PH_FMT_V210)
      PH_CLIP_CASE(PH_FMT_YUV422P10)
      PH_CLIP_CASE(PH_FMT_YUV422P8)
      PH_CLIP_CASE(PH_FMT_YUV420P)
      PH_CLIP_CASE(PH_FMT_NV12)
      PH_CLIP_CASE(PH_FMT_YUV420P10)
      PH_CLIP_CASE(PH_FMT_P010)
      PH_CLIP_CASE(PH_FMT_RGBA8)
      default:
        if (s == 0) clip_convert<PH_FMT_BGRA8, RGB12, true, kClipTransBlock>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        else clip_convert<PH_FMT_BGRA8, RGB12, false, kClipTransBlock>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd);
        break;
    }
#undef PH_CLIP_CASE
    if (threadIdx.x == 0) {  // the image as phase 2 sees it (clip_up_write_v210_kernel)
      const uint64_t base = (uint64_t)(uintptr_t)dst - ((uint64_t)R.r0 * ppitch + (uint64_t)R.c0 * kTexel);
      info[s] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), ppitch ? ppitch : kTexel, 0u);
    }
  }
  // ---- the swap: every wave's rectangle rows are in L2, the writer's table comes in
  __threadfence_block();
  __syncthreads();
  const LutK lk = make_lut_k(a.wr);
  lds_lut_load<kClipTransBlock>(a.wr);
  __syncthreads();
  // ---- phase 2: the layer's four block pixels after transform and transition, every output's writer behind them
  const uint32_t role = lane - 3u * (lane / 3u);
  auto image_of = [&](int s) __attribute__((always_inline)) {
    UpLayer L = s ? tr.partner[s - 1] : a.layer[0];
    const uint4 d = info[s];  // uniform address: one broadcast read
    const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.y) << 32;
    L.ptr = reinterpret_cast<const void *>((uintptr_t)base);
    L.pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.z);
    L.pad = kUpOutside - 16u;
    return L;
  };
  const uint32_t kind = tr.kind, same = tr.same;  // uniform
  const uint32_t units = ncu * nrp;
  for (uint32_t u = wave; u < units; u += kClipTransBlock / 64) {
    const uint32_t rp_in = ncu == 1u ? u : u / ncu, cu_in = u - rp_in * ncu;
    UpStep st;
    clip_step(a, 0u, cu0 + cu_in, rp0 + rp_in, lane, st);
    // (up_trans_layer, on the rectangles)
    UpTexel v[2][2];
    UpGeo geo;
    {
      const UpLayer L = image_of(0);
      geo = up_geo<RGB12>(L, st);
      UpPatch p;
      up_fetch<RGB12>(L, geo, p);
      up_values<RGB12>(p, geo, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) { v[dy][dx] = t; });
    }
    // a partner of the layer's size and placement has a rectangle of the layer's shape (its base aside) and is filtered with the layer's
    // geometry; any other brings its own, which takes the layer's place - and is replaced in its turn if the next partner is like the layer again
    bool geo_is_layers = true;
    auto partner = [&](int which, auto each) __attribute__((always_inline)) {
      const UpLayer P = image_of(1 + which);
      const bool like_layer = (same >> which) & 1u;
      if (!(like_layer && geo_is_layers)) geo = up_geo<RGB12>(P, st);  // uniform
      geo_is_layers = like_layer;
      UpPatch p;
      up_fetch<RGB12>(P, geo, p);
      up_values<RGB12>(p, geo, each);
    };
    if (kind == (uint32_t)PH_TRANSITION_WIPE) {  // the mask before the incoming image, as up_trans_layer
      float mr[2][2];
      partner(1, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
        const float mk = t.r, rm = 1.0f - mk;
        UpTexel &s = v[dy][dx];
        mr[dy][dx] = mk, s.r = s.r * rm, s.g = s.g * rm, s.b = s.b * rm, s.a = s.a * rm;
      });
      partner(0, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
        const float mk = mr[dy][dx];
        UpTexel &s = v[dy][dx];
        s.r = fma_rn(t.r, mk, s.r), s.g = fma_rn(t.g, mk, s.g), s.b = fma_rn(t.b, mk, s.b), s.a = fma_rn(t.a, mk, s.a);
      });
    } else {
      const float mix = tr.mix, rmix = 1.0f - mix;  // uniform
      partner(0, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
        UpTexel &s = v[dy][dx];
        s.r = fma_rn(s.r, mix, t.r * rmix), s.g = fma_rn(s.g, mix, t.g * rmix), s.b = fma_rn(s.b, mix, t.b * rmix), s.a = fma_rn(s.a, mix, t.a * rmix);
      });
    }
    // the twelve table reads of the block's four pixels, started together - once for all outputs (compose_up_multi_kernel)
    float t[2][2][3];
    {
      PxPending pend[2][2];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          pend[dy][dx] = write_px_issue(lds_lut_index_unit(v[dy][dx].r), lds_lut_index_unit(v[dy][dx].g), lds_lut_index_unit(v[dy][dx].b), lk);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx)
          t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
    }
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
      if (k >= cm.n_out) break;  // uniform
      const UpOut &o = cm.out[k];
      switch (o.fmt) {  // uniform
        case PH_FMT_V210: up_write_out<PH_FMT_V210>(o, st, t, role); break;
        case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
        case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
        case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
        case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
        case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
        case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
      }
    }
  }
}

// ---- a ROUTED channel's file playback: the combined IMAGE beside (or instead of) the consumers' frames ------------------------------------
// A ROUTE (routeProducer.ts:63-126, combiner.ts:219-254) hands another channel this channel's combined image - f32 RGBA, the channel's
// size.  The read-once kernels above hold the block's four combined pixels in registers right before the writers' table reads; the two
// kernels below are their texts again (clip_up_multi_kernel's phase 1 and table swap, compose_up_multi_kernel's front: both pinned,
// profiles/clip_route_resources.txt) with a phase 2 that makes every layer's four pixels as VALUES (up_values: the filtered alpha computed
// - 1 inside a clip without alpha, the border's 0 outside - never taken from the geometry), carries four alpha accumulators through
// ph_combine's arithmetic (combine_kernel: the bottom layer as it is, above it k = 1 - l.a, rgb = fma(acc, k, l), a = fma(acc.a, 0, l.a)),
// stores the block - two rows of two pixels, 32 bytes each, streamed or cached by `nt` as ph_combine stores its image - and then runs the
// twelve table reads and every output's writer on the very values it stored.  With no output there is no table: the image alone.
// one layer over the block's accumulators (FIRST: the bottom layer - or the Combiner's passthrough of a single one)
template <bool RGB12, bool FIRST>
__device__ __forceinline__ void up_route_layer(const UpLayer &L, const UpGeo &geo, UpTexel (&v)[2][2]) {
  UpPatch p;
  up_fetch<RGB12>(L, geo, p);
  up_values<RGB12>(p, geo, [&](int dy, int dx, const UpTexel &t) __attribute__((always_inline)) {
    UpTexel &s = v[dy][dx];
    if (FIRST) {
      s = t;
    } else {  // combine.ts:45-65, as combine_kernel has it
      const float k = 1.0f - t.a;
      s.r = fma_rn(s.r, k, t.r), s.g = fma_rn(s.g, k, t.g), s.b = fma_rn(s.b, k, t.b), s.a = fma_rn(s.a, 0.0f, t.a);
    }
  });
}
// the block into the image, then - where the launch has outputs - compose_up_multi_kernel's tail
__device__ __forceinline__ void up_route_tail(void *image, uint32_t nt, uint32_t out_w, const UpStep &st, const UpTexel (&v)[2][2], uint32_t n_out,
                                              const UpOut (&out)[kMaxUpOuts], uint32_t role, const LutK &lk) {
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    if (!(st.live && (dy == 0 || st.li[1] != st.li[0]))) continue;  // (x0 is even and so is out_w: both pixels of a live lane are inside)
    float4 *const at = static_cast<float4 *>(image) + (size_t)st.line[dy] * out_w + st.x0;
    store_image(at, make_float4(v[dy][0].r, v[dy][0].g, v[dy][0].b, v[dy][0].a), nt);
    store_image(at + 1, make_float4(v[dy][1].r, v[dy][1].g, v[dy][1].b, v[dy][1].a), nt);
  }
  if (!n_out) return;  // uniform
  float t[2][2][3];
  {
    PxPending pend[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        pend[dy][dx] = write_px_issue(lds_lut_index_unit(v[dy][dx].r), lds_lut_index_unit(v[dy][dx].g), lds_lut_index_unit(v[dy][dx].b), lk);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx)
        t[dy][dx][0] = lds_lut_finish(pend[dy][dx].r), t[dy][dx][1] = lds_lut_finish(pend[dy][dx].g), t[dy][dx][2] = lds_lut_finish(pend[dy][dx].b);
  }
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)kMaxUpOuts; ++k) {
    if (k >= n_out) break;  // uniform
    const UpOut &o = out[k];
    switch (o.fmt) {  // uniform
      case PH_FMT_V210: up_write_out<PH_FMT_V210>(o, st, t, role); break;
      case PH_FMT_YUV422P10: up_write_out<PH_FMT_YUV422P10>(o, st, t, role); break;
      case PH_FMT_YUV422P8: up_write_out<PH_FMT_YUV422P8>(o, st, t, role); break;
      case PH_FMT_YUV420P: up_write_out<PH_FMT_YUV420P>(o, st, t, role); break;
      case PH_FMT_NV12: up_write_out<PH_FMT_NV12>(o, st, t, role); break;
      case PH_FMT_RGBA8: up_write_out<PH_FMT_RGBA8>(o, st, t, role); break;
      case PH_FMT_BGRA8: up_write_out<PH_FMT_BGRA8>(o, st, t, role); break;
    }
  }
}

// ONE clip in its wire format: phase 1 and the swap are clip_up_multi_kernel's (one frame, one layer: the launcher refuses the rest)
template <bool RGB12>
__global__ __launch_bounds__(kUpBlock) void clip_up_route_kernel(ClipUpRouteArgs rt) {
  const ClipUpMultiArgs &cm = rt.multi;
  const ClipUpArgs &c = cm.clip;
  const UpArgs &a = c.up;
  constexpr uint32_t kTexel = RGB12 ? 12u : 16u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // the tile
  const uint32_t upr = (a.cover_w + kUpCols - 1u) / kUpCols, rps = (a.lines + 1u) / 2u;
  const uint32_t ty = blockIdx.x / c.gx, tx = blockIdx.x - ty * c.gx;
  const uint32_t cu0 = tx * c.tcu, rp0 = ty * c.trp;
  const uint32_t ncu = cu0 + c.tcu <= upr ? c.tcu : upr - cu0, nrp = rp0 + c.trp <= rps ? c.trp : rps - rp0;
  char *const mine = c.scratch + (size_t)blockIdx.x * c.wg_bytes;
  // ---- phase 1: the reader's table; the clip's rectangle converted
  const LutK rlk = make_lut_k(c.rd);
  uint4 *const info = reinterpret_cast<uint4 *>(g_lds + c.info_off);
  {
    const UpLayer L = a.layer[0];
    const ClipSrc S = c.src[0];
    const uint32_t x_first = cu0 * kUpCols, x_end = (cu0 + ncu) * kUpCols < a.out_w ? (cu0 + ncu) * kUpCols : a.out_w;
    const uint32_t li_last = 2u * (rp0 + nrp) < a.lines ? 2u * (rp0 + nrp) - 1u : a.lines - 1u;
    ClipRect R{0, 0, 0, 0};
    if (x_first < x_end) {
      int c_lo = clip_tap_col(L, x_first, a.out_w), c_hi = clip_tap_col(L, x_end - 1u, a.out_w) + 2;
      int r_lo = clip_tap_row(L, a.first_line + 2u * rp0 * a.line_step, a.out_h), r_hi = clip_tap_row(L, a.first_line + li_last * a.line_step, a.out_h) + 2;
      c_lo = c_lo < 0 ? 0 : c_lo, r_lo = r_lo < 0 ? 0 : r_lo;
      c_hi = c_hi >= (int)L.w ? (int)L.w - 1 : c_hi, r_hi = r_hi >= (int)L.h ? (int)L.h - 1 : r_hi;
      if (c_hi >= c_lo && r_hi >= r_lo) R = ClipRect{(uint32_t)c_lo, (uint32_t)r_lo, (uint32_t)(c_hi - c_lo + 1), (uint32_t)(r_hi - r_lo + 1)};
    }
    R.c0 = __builtin_amdgcn_readfirstlane(R.c0), R.r0 = __builtin_amdgcn_readfirstlane(R.r0);
    R.w = __builtin_amdgcn_readfirstlane(R.w), R.h = __builtin_amdgcn_readfirstlane(R.h);
    const uint32_t ppitch = R.w * kTexel;
    if (ppitch && R.h * ppitch > c.rect_cap[0]) R.h = c.rect_cap[0] / ppitch;  // (the launcher's bound holds: never taken)
    char *const dst = mine + c.rect_off[0];
#define PH_CLIP_CASE(F)                                                                 \
  case F: clip_convert<F, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd); break;
    switch (S.fmt) {  // uniform
      PH_CLIP_CASE(PH_FMT_V210)
      PH_CLIP_CASE(PH_FMT_YUV422P10)
      PH_CLIP_CASE(PH_FMT_YUV422P8)
      PH_CLIP_CASE(PH_FMT_YUV420P)
      PH_CLIP_CASE(PH_FMT_NV12)
      PH_CLIP_CASE(PH_FMT_YUV420P10)
      PH_CLIP_CASE(PH_FMT_P010)
      PH_CLIP_CASE(PH_FMT_RGBA8)
      default: clip_convert<PH_FMT_BGRA8, RGB12, true>(S, L, R, dst, ppitch, c.rd_gm, rlk, c.rd); break;
    }
#undef PH_CLIP_CASE
    if (threadIdx.x == 0) {  // the layer as phase 2 sees it (clip_up_write_v210_kernel)
      const uint64_t base = (uint64_t)(uintptr_t)dst - ((uint64_t)R.r0 * ppitch + (uint64_t)R.c0 * kTexel);
      info[0] = make_uint4((uint32_t)base, (uint32_t)(base >> 32), ppitch ? ppitch : kTexel, 0u);
    }
  }
  // ---- the swap: every wave's rectangle rows are in L2; the writer's table comes in where there is an output
  __threadfence_block();
  __syncthreads();
  const LutK lk = make_lut_k(a.wr);
  if (cm.n_out) {  // uniform
    lds_lut_load<kUpBlock>(a.wr);
    __syncthreads();
  }
  // ---- phase 2: the transformed clip as values - the image -, every output's writer behind it
  const uint32_t role = lane - 3u * (lane / 3u);
  UpLayer L = a.layer[0];
  {
    const uint4 d = info[0];  // uniform address: one broadcast read
    const uint64_t base = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.x) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)d.y) << 32;
    L.ptr = reinterpret_cast<const void *>((uintptr_t)base);
    L.pitch = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.z);
    L.pad = kUpOutside - 16u;
  }
  const uint32_t units = ncu * nrp;
  for (uint32_t u = wave; u < units; u += kUpBlock / 64) {
    const uint32_t rp_in = ncu == 1u ? u : u / ncu, cu_in = u - rp_in * ncu;
    UpStep st;
    clip_step(a, 0u, cu0 + cu_in, rp0 + rp_in, lane, st);
    UpTexel v[2][2];
    up_route_layer<RGB12, true>(L, up_geo<RGB12>(L, st), v);
    up_route_tail(rt.image, rt.nt, a.out_w, st, v, cm.n_out, cm.out, role, lk);
  }
}

// f32 RGBA images, any number of layers: compose_up_multi_kernel's front (COLS: 126 with a v210 output, else 128)
template <uint32_t COLS>
__global__ __launch_bounds__(kUpBlock) void compose_up_route_kernel(UpRouteArgs rt) {
  const UpMultiArgs &m = rt.multi;
  const UpArgs &a = m.up;
  const LutK lk = make_lut_k(a.wr);
  if (m.n_out) {  // uniform
    lds_lut_load<kUpBlock>(a.wr);
    __syncthreads();
  }
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const UpShare sh = up_share<COLS>(a);
  const uint32_t role = lane - 3u * (lane / 3u);
  UpStep st;
  for (uint32_t base = 0; up_step<COLS>(a, sh, base, wave, lane, st);) {
    UpTexel v[2][2];
    UpGeo geo = up_geo<false>(a.layer[0], st);
    up_route_layer<false, true>(a.layer[0], geo, v);
#pragma unroll 1
    for (int l = 1; l < a.n; ++l) {
      const UpLayer L = a.layer[l];
      if (!a.shared) geo = up_geo<false>(L, st);  // uniform
      up_route_layer<false, false>(L, geo, v);
    }
    up_route_tail(rt.image, rt.nt, a.out_w, st, v, m.n_out, m.out, role, lk);
  }
}

// The tiling: tiles of tcu wave-step columns x trp row pairs, one per workgroup, as even as the frame allows (a workgroup's sixteen waves
// share its tile's wave steps); then every layer's rectangle bound - the taps of (tcu * 126) columns x (2 * trp) written rows span that
// many source texels times the magnification, + the patch's third column / row, + one for the rounding of the coordinates.
// v210_tails: the launch's kernel writes a v210 line's tail quad and cleared slots (clip_up_write_v210_kernel<.., TAILS>), so the wave
// steps cover the whole pitch; clip_up_multi_kernel has no such output and covers the frame's columns.
uint32_t clip_up_plan(ClipUpArgs &c, bool rgb12, uint32_t num_cus, bool v210_tails) {
  UpArgs &a = c.up;
  if (!a.lines || !a.n || !num_cus) return 0;
  if (!a.jobs) a.jobs = 1;
  if (a.jobs > (uint32_t)kMaxUpJobs || (a.jobs > 1u && a.n != 1)) return 0;
  const bool tails = v210_tails && a.out_w % 48u != 0;
  a.out_qpitch = v210_pitch_bytes(a.out_w) / 16u;
  a.cover_w = tails ? a.out_qpitch * 6u : a.out_w;
  a.shared = 1;
  for (int l = 1; l < a.n; ++l) {
    a.shared = a.shared && a.layer[l].w == a.layer[0].w && a.layer[l].h == a.layer[0].h;
    for (int k = 0; k < 6; ++k) a.shared = a.shared && a.layer[l].m[k] == a.layer[0].m[k];
  }
  const uint32_t upr = (a.cover_w + kUpCols - 1u) / kUpCols, rps = (a.lines + 1u) / 2u, cus_per_job = num_cus / a.jobs ? num_cus / a.jobs : 1u;
  uint32_t best = ~0u, tcu = 0, trp = 0;
  for (uint32_t cx = 1; cx <= 32u && cx <= upr && cx <= cus_per_job; cx *= 2u) {
    const uint32_t ry = cus_per_job / cx < rps ? cus_per_job / cx : rps;  // rows of tiles per job (a tile belongs to one job)
    const uint32_t t_cu = (upr + cx - 1u) / cx, t_rp = (rps + ry - 1u) / ry;
    // wave steps of the fullest workgroup, in rounds of its sixteen waves (what phase 2 takes), + its rectangle's rim (what phase 1 converts twice)
    const uint32_t rounds = (t_cu * t_rp + kUpBlock / 64 - 1u) / (kUpBlock / 64);
    const uint32_t cost = rounds * 1024u + t_cu + t_rp;
    if (cost < best) best = cost, tcu = t_cu, trp = t_rp;
  }
  c.tcu = tcu, c.trp = trp, c.gx = (upr + tcu - 1u) / tcu, c.gy = (rps + trp - 1u) / trp;
  const uint32_t grid = c.gx * c.gy * a.jobs;
  const uint32_t texel = rgb12 ? 12u : 16u;
  uint32_t off = 0;
  for (int l = 0; l < a.n; ++l) {
    const UpLayer &L = a.layer[l];
    const double sx = (double)L.m[0] * L.w / a.out_w, sy = (double)L.m[4] * L.h / a.out_h * a.line_step;
    uint32_t rw = (uint32_t)((tcu * kUpCols - 1u) * sx) + 6u, rh = (uint32_t)((2u * trp - 1u) * sy) + 6u;
    rw = rw < L.w ? rw : L.w, rh = rh < L.h ? rh : L.h;
    c.rect_off[l] = off, c.rect_cap[l] = (rw * rh * texel + 255u) & ~255u;
    off += c.rect_cap[l] + 256u;  // (+ a rim: dead lanes' patches read a few texels past a rectangle's last row)
  }
  c.wg_bytes = off;
  const uint32_t lds = c.rd.bytes > a.wr.bytes ? c.rd.bytes : a.wr.bytes;
  c.info_off = (lds + 15u) & ~15u;
  if (c.info_off + 16u * (uint32_t)a.n > (uint32_t)kMaxDynamicLds) return 0;
  return grid;
}

hipError_t launch_clip_up_write_v210(hipStream_t s, const ClipUpArgs &c, bool rgb12, uint32_t grid) {
  if (!grid) return hipErrorInvalidValue;
  char name[48];
  if (c.up.jobs > 1u) snprintf(name, sizeof name, "clip_up_write_v210<%s>x%u", rgb12 ? "rgb" : "rgba", c.up.jobs);
  else snprintf(name, sizeof name, "clip_up_write_v210<%s>", rgb12 ? "rgb" : "rgba");
  if (trace_launch(name)) return hipSuccess;
  const bool tails = c.up.out_w % 48u != 0, multi = c.up.jobs > 1u;
  const uint32_t lds = c.info_off + 16u * (uint32_t)c.up.n;
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpBlock, lds, s>>>(c);
    return hipGetLastError();
  };
  if (multi) {
    if (tails) return rgb12 ? go(clip_up_write_v210_kernel<true, true, true>) : go(clip_up_write_v210_kernel<false, true, true>);
    return rgb12 ? go(clip_up_write_v210_kernel<true, false, true>) : go(clip_up_write_v210_kernel<false, false, true>);
  }
  if (tails) return rgb12 ? go(clip_up_write_v210_kernel<true, true, false>) : go(clip_up_write_v210_kernel<false, true, false>);
  return rgb12 ? go(clip_up_write_v210_kernel<true, false, false>) : go(clip_up_write_v210_kernel<false, false, false>);
}

// Several outputs of one clip composition: named clip_up_multi<rgb|rgba>x<outputs> in a route trace.  grid: clip_up_plan's, asked with
// v210_tails == false.  Refuses what launch_compose_up_multi refuses.  Several jobs (single-layer frames of one shape, job j's clip in
// clip.src[j] and its planes in out[k].plane[j]): named clip_up_multi<rgb|rgba>x<outputs>j<jobs>, the MULTI instantiation.
// v210_tails (context option "up_v210_tails"): a v210 output whose lines end in a tail quad is taken - grid is then clip_up_plan's asked
// with v210_tails == true (the tiles cover the pitch), the launch is named clip_up_multi_t<..> and runs the TAILS instantiations.
hipError_t launch_clip_up_multi(hipStream_t s, const ClipUpMultiArgs &m, bool rgb12, uint32_t grid, bool v210_tails) {
  const UpArgs &a = m.clip.up;
  if (!grid || m.n_out < 1 || m.n_out > (uint32_t)kMaxUpOuts || a.jobs < 1u || a.jobs > (uint32_t)kMaxUpJobs || a.n < 1 || a.n > kMaxLayers) return hipErrorInvalidValue;
  bool tails = false;
  for (uint32_t k = 0; k < m.n_out; ++k) tails = tails || (v210_tails && m.out[k].fmt == PH_FMT_V210 && a.out_w % 48u);
  if (a.cover_w != (tails ? a.out_qpitch * 6u : a.out_w)) return hipErrorInvalidValue;
  const bool multi = a.jobs > 1u;
  if (multi && (a.n != 1 || !m.clip.gy || grid != m.clip.gx * m.clip.gy * a.jobs)) return hipErrorInvalidValue;  // (a tile's job is its row of tiles / gy: within jobs)
  for (uint32_t k = 0; k < m.n_out; ++k)
    if (!fmt_chan_out((int)m.out[k].fmt) || (m.out[k].fmt == PH_FMT_V210 && a.out_w % 48u && !tails)) return hipErrorInvalidValue;
  char name[48];
  if (multi) snprintf(name, sizeof name, "clip_up_multi%s<%s>x%uj%u", tails ? "_t" : "", rgb12 ? "rgb" : "rgba", m.n_out, a.jobs);
  else snprintf(name, sizeof name, "clip_up_multi%s<%s>x%u", tails ? "_t" : "", rgb12 ? "rgb" : "rgba", m.n_out);
  if (trace_launch(name)) return hipSuccess;
  const uint32_t lds = m.clip.info_off + 16u * (uint32_t)a.n;
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpBlock, lds, s>>>(m);
    return hipGetLastError();
  };
  if (tails) {  // a v210 output's line pitch: every quad slot of it is written
    ClipUpMultiArgs b = m;
    for (uint32_t k = 0; k < b.n_out; ++k)
      if (b.out[k].fmt == PH_FMT_V210) b.out[k].pitch = a.out_qpitch;
    auto go_tails = [&](auto kernel) -> hipError_t {
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
      if (e != hipSuccess) return e;
      kernel<<<grid, kUpBlock, lds, s>>>(b);
      return hipGetLastError();
    };
    if (multi) return rgb12 ? go_tails(clip_up_multi_kernel<true, true, true>) : go_tails(clip_up_multi_kernel<false, true, true>);
    return rgb12 ? go_tails(clip_up_multi_kernel<true, false, true>) : go_tails(clip_up_multi_kernel<false, false, true>);
  }
  if (multi) return rgb12 ? go(clip_up_multi_kernel<true, true>) : go(clip_up_multi_kernel<false, true>);
  return rgb12 ? go(clip_up_multi_kernel<true>) : go(clip_up_multi_kernel<false>);
}

// One clip in a transition: the launch planned as a clip of three "layers" - src, incoming, mask (a dissolve: two) - so that clip_up_plan's
// tiling, its rectangle bound per slot (from that image's OWN size and placement: a partner placed differently from the layer gets the
// bound of its own taps) and its scratch size hold as they are.  The composition itself stays one layer.
uint32_t clip_up_trans_plan(ClipUpTransArgs &t, bool rgb12, uint32_t num_cus) {
  ClipUpArgs &c = t.multi.clip;
  if (c.up.n != 1 || c.up.jobs > 1u || (t.kind != (uint32_t)PH_TRANSITION_DISSOLVE && t.kind != (uint32_t)PH_TRANSITION_WIPE)) return 0;
  const int slots = t.kind == (uint32_t)PH_TRANSITION_WIPE ? 3 : 2;
  ClipUpArgs p = c;
  p.up.n = slots;
  for (int s = 1; s < slots; ++s) p.up.layer[s] = t.partner[s - 1];
  const uint32_t grid = clip_up_plan(p, rgb12, num_cus, false);
  if (!grid || p.info_off + 16u * 3u > (uint32_t)kMaxDynamicLds) return 0;  // (the launch reserves three descriptors, a dissolve's third unused)
  c.up.jobs = 1, c.up.out_qpitch = p.up.out_qpitch, c.up.cover_w = p.up.cover_w, c.up.shared = 0;
  c.tcu = p.tcu, c.trp = p.trp, c.gx = p.gx, c.gy = p.gy, c.wg_bytes = p.wg_bytes, c.info_off = p.info_off;
  for (int s = 0; s < slots; ++s) c.rect_off[s] = p.rect_off[s], c.rect_cap[s] = p.rect_cap[s];
  return grid;
}

hipError_t launch_clip_up_trans(hipStream_t s, const ClipUpTransArgs &t, bool rgb12, uint32_t grid) {
  const ClipUpMultiArgs &m = t.multi;
  const UpArgs &a = m.clip.up;
  if (!grid || m.n_out < 1 || m.n_out > (uint32_t)kMaxUpOuts || a.jobs != 1u || a.n != 1 || a.cover_w != a.out_w || grid != m.clip.gx * m.clip.gy)
    return hipErrorInvalidValue;
  if (t.kind != (uint32_t)PH_TRANSITION_DISSOLVE && t.kind != (uint32_t)PH_TRANSITION_WIPE) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < m.n_out; ++k)
    if (!fmt_chan_out((int)m.out[k].fmt) || (m.out[k].fmt == PH_FMT_V210 && a.out_w % 48u)) return hipErrorInvalidValue;
  char name[48];
  snprintf(name, sizeof name, "clip_up_trans<%s>x%u", rgb12 ? "rgb" : "rgba", m.n_out);
  if (trace_launch(name)) return hipSuccess;
  const uint32_t lds = m.clip.info_off + 16u * 3u;
  if (lds > (uint32_t)kMaxDynamicLds) return hipErrorInvalidValue;
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kClipTransBlock, lds, s>>>(t);
    return hipGetLastError();
  };
  return rgb12 ? go(clip_up_trans_kernel<true>) : go(clip_up_trans_kernel<false>);
}

// Does the 2 x 2 block scheme apply?  Unrotated, unmirrored, MAGNIFIED in both directions (then the first taps of the two
// pixels of a block are at most one texel apart, rounding noise included, and the block's taps lie in a 3 x 3 patch), images
// below 1 GiB.
bool compose_up_eligible(const UpArgs &a) {
  if (a.out_w % 2u || !a.n) return false;  // (any even width: lines with a tail take the TAILS instantiation)
  for (int l = 0; l < a.n; ++l) {
    const UpLayer &L = a.layer[l];
    if (L.m[1] != 0.0f || L.m[3] != 0.0f || !(L.m[0] > 0.0f) || !(L.m[4] > 0.0f)) return false;
    // source texels per output pixel: d(u)/dx = m0 * w / out_w; per WRITTEN row: d(v)/dy = m4 * h / out_h * line_step (a field
    // write takes every other line).  Below one texel by a margin far above the f32 noise of the coordinates (1e-4 texels at
    // 1920 columns): then the first taps of the block's two columns / rows are 0 or 1 apart; at a whole texel between them
    // the noise could make it 2.
    // ... or EXACTLY one: a source of the frame's size under the Mixer's default fill (the identity, a frame write).  Its taps sit half a
    // texel off the pixel centres (transform.ts:53 samples at x / w, not (x + 0.5) / w: fu = x - 0.5), as far from a flip as can be:
    // neighbouring pixels' first taps are exactly 1 apart
    const bool fill = L.w == a.out_w && L.h == a.out_h && a.line_step == 1u && L.m[0] == 1.0f && L.m[4] == 1.0f && L.m[2] == 0.0f && L.m[5] == 0.0f;
    if (!fill && ((double)L.m[0] * L.w > 0.99 * a.out_w || (double)L.m[4] * L.h * a.line_step > 0.99 * a.out_h)) return false;
    if ((uint64_t)L.pitch * L.h >= (1ull << 30) || L.w >= (1u << 22)) return false;
  }
  return true;
}

// what the launcher adds to a launch's arguments; returns the number of workgroups
static uint32_t up_plan(UpArgs &b, bool tails, uint32_t num_cus, uint32_t cols = kUpCols, uint32_t block = (uint32_t)kUpBlock) {
  if (!b.jobs) b.jobs = 1;
  b.out_qpitch = v210_pitch_bytes(b.out_w) / 16u;
  b.cover_w = tails ? b.out_qpitch * 6u : b.out_w;
  b.shared = 1;  // every layer has the size and the placement of the first: the patch geometry and the weights are computed once per block
  for (int l = 1; l < b.n; ++l) {
    b.shared = b.shared && b.layer[l].w == b.layer[0].w && b.layer[l].h == b.layer[0].h && b.layer[l].pitch == b.layer[0].pitch;
    for (int k = 0; k < 6; ++k) b.shared = b.shared && b.layer[l].m[k] == b.layer[0].m[k];
  }
  const uint32_t upr = (b.cover_w + cols - 1u) / cols, upg = (uint32_t)(PH_UP_GROUP_ROWS / 2) * upr;
  const uint32_t units = upr * ((b.lines + 1u) / 2u) * b.jobs;
  // reciprocals for the kernel's uniform divisions: umulhi(v, ceil(2^32 / d)) == v / d while v * d < 2^32
  b.magic_upr = upr > 1 ? (uint32_t)(((1ull << 32) + upr - 1) / upr) : 0u;
  b.magic_upg = (uint32_t)(((1ull << 32) + upg - 1) / upg);
  const uint32_t want = (units + block / 64 - 1) / (block / 64);
  return want < num_cus ? want : num_cus;
}

hipError_t launch_compose_up_write_v210(hipStream_t s, const UpArgs &a, bool rgb12, uint32_t num_cus) {
  if (!a.lines) return hipSuccess;
  const bool tails = a.out_w % 48u != 0;  // lines that end in a tail quad and / or cleared slots: an instantiation of its own
  const void *fn = tails ? (rgb12 ? reinterpret_cast<const void *>(compose_up_write_v210_kernel<true, true>)
                                  : reinterpret_cast<const void *>(compose_up_write_v210_kernel<false, true>))
                         : (rgb12 ? reinterpret_cast<const void *>(compose_up_write_v210_kernel<true>)
                                  : reinterpret_cast<const void *>(compose_up_write_v210_kernel<false>));
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
  if (e != hipSuccess) return e;
  UpArgs b = a;
  const uint32_t grid = up_plan(b, tails, num_cus);
  if (tails && rgb12) compose_up_write_v210_kernel<true, true><<<grid, kUpBlock, a.wr.bytes, s>>>(b);
  else if (tails) compose_up_write_v210_kernel<false, true><<<grid, kUpBlock, a.wr.bytes, s>>>(b);
  else if (rgb12) compose_up_write_v210_kernel<true><<<grid, kUpBlock, a.wr.bytes, s>>>(b);
  else compose_up_write_v210_kernel<false><<<grid, kUpBlock, a.wr.bytes, s>>>(b);
  return hipGetLastError();
}

// Several outputs of one composition: named compose_up_multi<rgb|rgba>x<outputs>j<jobs> in a route trace
// v210_tails (context option "up_v210_tails"): a v210 output whose lines end in a tail quad is taken - the launch is named
// compose_up_multi_t<..> and runs the TAILS instantiation, its wave steps over the pitch.
hipError_t launch_compose_up_multi(hipStream_t s, const UpMultiArgs &m, bool rgb12, uint32_t num_cus, bool v210_tails) {
  if (!m.up.lines) return hipSuccess;
  if (m.n_out < 1 || m.n_out > (uint32_t)kMaxUpOuts || m.up.jobs < 1 || m.up.jobs > (uint32_t)kMaxUpJobs) return hipErrorInvalidValue;
  bool tails = false;
  for (uint32_t k = 0; k < m.n_out; ++k) tails = tails || (v210_tails && m.out[k].fmt == PH_FMT_V210 && m.up.out_w % 48u);
  for (uint32_t k = 0; k < m.n_out; ++k)
    if (!fmt_chan_out((int)m.out[k].fmt) || (m.out[k].fmt == PH_FMT_V210 && m.up.out_w % 48u && !tails)) return hipErrorInvalidValue;
  char name[48];
  snprintf(name, sizeof name, "compose_up_multi%s<%s>x%uj%u", tails ? "_t" : "", rgb12 ? "rgb" : "rgba", m.n_out, m.up.jobs);
  if (trace_launch(name)) return hipSuccess;
  // the wave step: 126 columns with a v210 output (its quads), else 128 - every store instruction of a wave then covers whole 32-byte
  // sectors of its row where the pitch allows (see compose_up_multi_kernel).  PH_UP_OUT_STEP=126 in the environment keeps 126 for every
  // launch: the A/B that tools/up_out_bench.py step=126 recorded in profiles/up_out_bench_step126.jsonl
  static const bool narrow_always = [] { const char *e = getenv("PH_UP_OUT_STEP"); return e && atoi(e) == 126; }();
  bool v210 = false;
  for (uint32_t k = 0; k < m.n_out; ++k) v210 = v210 || m.out[k].fmt == PH_FMT_V210;
  const bool wide = !v210 && !narrow_always;
  UpMultiArgs b = m;
  const uint32_t grid = up_plan(b.up, tails, num_cus, wide ? 128u : kUpCols);
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpBlock, b.up.wr.bytes, s>>>(b);
    return hipGetLastError();
  };
  if (tails) {  // (a v210 output: 126 columns) - its line pitch, every quad slot of which is written
    for (uint32_t k = 0; k < b.n_out; ++k)
      if (b.out[k].fmt == PH_FMT_V210) b.out[k].pitch = b.up.out_qpitch;
    return rgb12 ? go(compose_up_multi_kernel<true, kUpCols, true>) : go(compose_up_multi_kernel<false, kUpCols, true>);
  }
  if (wide) return rgb12 ? go(compose_up_multi_kernel<true, 128u>) : go(compose_up_multi_kernel<false, 128u>);
  return rgb12 ? go(compose_up_multi_kernel<true, kUpCols>) : go(compose_up_multi_kernel<false, kUpCols>);
}

// The same with layers in a transition: named compose_up_trans<rgb|rgba>x<outputs>j<jobs> in a route trace.  A v210 output's lines end on
// a 48-pixel block (the caller refuses the others: no TAILS instantiation here)
hipError_t launch_compose_up_trans(hipStream_t s, const UpTransArgs &t, bool rgb12, uint32_t num_cus) {
  const UpMultiArgs &m = t.multi;
  if (!m.up.lines) return hipSuccess;
  if (m.n_out < 1 || m.n_out > (uint32_t)kMaxUpOuts || m.up.jobs < 1 || m.up.jobs > (uint32_t)kMaxUpJobs || m.up.n < 1 || m.up.n > kMaxLayers) return hipErrorInvalidValue;
  for (uint32_t k = 0; k < m.n_out; ++k)
    if (!fmt_chan_out((int)m.out[k].fmt) || (m.out[k].fmt == PH_FMT_V210 && m.up.out_w % 48u)) return hipErrorInvalidValue;
  for (int l = 0; l < m.up.n; ++l)
    if (t.kind[l] > (uint32_t)PH_TRANSITION_WIPE) return hipErrorInvalidValue;
  char name[48];
  snprintf(name, sizeof name, "compose_up_trans<%s>x%uj%u", rgb12 ? "rgb" : "rgba", m.n_out, m.up.jobs);
  if (trace_launch(name)) return hipSuccess;
  bool v210 = false;
  for (uint32_t k = 0; k < m.n_out; ++k) v210 = v210 || m.out[k].fmt == PH_FMT_V210;
  UpTransArgs b = t;
  const uint32_t grid = up_plan(b.multi.up, false, num_cus, v210 ? kUpCols : 128u, (uint32_t)kUpTransBlock);
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpTransBlock, b.multi.up.wr.bytes, s>>>(b);
    return hipGetLastError();
  };
  if (!v210) return rgb12 ? go(compose_up_trans_kernel<true, 128u>) : go(compose_up_trans_kernel<false, 128u>);
  return rgb12 ? go(compose_up_trans_kernel<true, kUpCols>) : go(compose_up_trans_kernel<false, kUpCols>);
}

// what both route launches refuse: no image, more than one job, lines other than the whole frame, an output the writers do not make
static bool up_route_refused(const UpArgs &a, const void *image, uint32_t n_out, const UpOut *out) {
  if (!image || n_out > (uint32_t)kMaxUpOuts || a.jobs > 1u || a.n < 1 || a.n > kMaxLayers) return true;
  if (a.out_w % 2u || a.first_line != 0u || a.line_step != 1u || a.lines != a.out_h) return true;  // (the image is the whole frame)
  for (uint32_t k = 0; k < n_out; ++k)
    if (!fmt_chan_out((int)out[k].fmt) || (out[k].fmt == PH_FMT_V210 && a.out_w % 48u)) return true;
  return false;
}

// One clip, the image and its frames: named clip_up_route<rgb|rgba>x<outputs> in a route trace.  grid: clip_up_plan's, asked with
// v210_tails == false
hipError_t launch_clip_up_route(hipStream_t s, const ClipUpRouteArgs &r, bool rgb12, uint32_t grid) {
  const ClipUpMultiArgs &m = r.multi;
  const UpArgs &a = m.clip.up;
  if (!grid || up_route_refused(a, r.image, m.n_out, m.out) || a.n != 1 || a.cover_w != a.out_w || grid != m.clip.gx * m.clip.gy) return hipErrorInvalidValue;
  char name[48];
  snprintf(name, sizeof name, "clip_up_route<%s>x%u", rgb12 ? "rgb" : "rgba", m.n_out);
  if (trace_launch(name)) return hipSuccess;
  const uint32_t lds = m.clip.info_off + 16u;
  if (lds > (uint32_t)kMaxDynamicLds) return hipErrorInvalidValue;
  ClipUpRouteArgs b = r;
  b.nt = image_nt((size_t)a.out_w * a.out_h * 16u);
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpBlock, lds, s>>>(b);
    return hipGetLastError();
  };
  return rgb12 ? go(clip_up_route_kernel<true>) : go(clip_up_route_kernel<false>);
}

// f32 RGBA images, the image and its frames: named compose_up_route<rgba>x<outputs>j1 in a route trace
hipError_t launch_compose_up_route(hipStream_t s, const UpRouteArgs &r, uint32_t num_cus) {
  const UpMultiArgs &m = r.multi;
  if (!m.up.lines) return hipSuccess;
  if (up_route_refused(m.up, r.image, m.n_out, m.out)) return hipErrorInvalidValue;
  char name[48];
  snprintf(name, sizeof name, "compose_up_route<rgba>x%uj1", m.n_out);
  if (trace_launch(name)) return hipSuccess;
  bool v210 = false;
  for (uint32_t k = 0; k < m.n_out; ++k) v210 = v210 || m.out[k].fmt == PH_FMT_V210;
  UpRouteArgs b = r;
  b.multi.up.jobs = 1;
  const uint32_t grid = up_plan(b.multi.up, false, num_cus, v210 ? kUpCols : 128u);
  b.nt = image_nt((size_t)m.up.out_w * m.up.out_h * 16u);
  auto go = [&](auto kernel) -> hipError_t {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynamicLds);
    if (e != hipSuccess) return e;
    kernel<<<grid, kUpBlock, m.n_out ? b.multi.up.wr.bytes : 0u, s>>>(b);
    return hipGetLastError();
  };
  return v210 ? go(compose_up_route_kernel<kUpCols>) : go(compose_up_route_kernel<128u>);
}

}  // namespace ph
