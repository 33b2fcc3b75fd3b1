// ph_kernels_fused_out.h - what the kernels of ph_kernels_fused_multi_body.h share beside the body itself: the wave-priority ladder
// the table load of the kernels with more in their layer loop, and one output's share of one quad.  Included by
// ph_kernels_fused_multi.hip, ph_kernels_fused_trans.hip and ph_kernels_fused_route.hip, each inside its own unnamed namespace; the
// text is the one ph_kernels_fused_multi.hip always had, and its kernels compile to the same assembly, instruction for instruction
// (profiles/fused_trans_resources.txt, profiles/fused_route_resources.txt).

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

// lds_lut_load (ph_ldslut.h: its text, its s_waitcnt included) with the lane's place in the copy made at the load, from a pinned copy of
// threadIdx.x.  Made from threadIdx.x as it stands, the wave's and the lane's offsets are loop invariants that the compiler carries
// through both phases of every tile - in registers the kernels with more in their layer loop (ph_kernels_fused_trans.hip,
// ph_kernels_fused_route.hip) do not have: four vector spills (profiles/fused_trans_resources.txt).
template <int BS>
__device__ __forceinline__ void fm_lut_load(const LutView &v) {
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const uint32_t n = (v.bytes - v.hole) / 16;
  unsigned char *const dst = g_lds + v.hole;
  const uint32_t wave = tid >> 6, lane = tid & 63;
  const uint4 *src = reinterpret_cast<const uint4 *>(v.blob);
  for (uint32_t base = wave * 64; base < n; base += BS) {
    const uint32_t i = base + lane;
    if (i < n)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i),
                                       (__attribute__((address_space(3))) void *)(dst + 16 * base), 16, 0, 0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
