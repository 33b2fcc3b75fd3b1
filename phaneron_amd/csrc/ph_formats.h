// ph_formats.h - the pack formats described once, for the host code and every kernel.  constexpr only: no HIP runtime calls.
//
// A format is its PH_FMT_* value (include/phaneron_hip.h), the index of its row in kFmts.  The kernels' compile-time branches, the
// entry points' checks, the plane geometry and the program names all ask the traits below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/phaneron_hip.h"

namespace ph {

struct FmtDesc {
  int id;            // PH_FMT_*
  const char *name;  // program tag "phaneron:<name>", kernel ids "<name>_read" / "<name>_write" (ph_program.cpp)
  int src;           // the PH_SRC_* of a channel source in this format (ph_chan_source)
  int planes;        // 1: v210, packed RGB; 2: Y + interleaved CbCr (nv12, p010); 3: Y, Cb, Cr
  bool rgb8;         // packed 8-bit RGB, four bytes per pixel (rgba8.ts)
  bool v420;         // 4:2:0: chroma line r >> 1 serves line r
  bool wide;         // 16-bit samples
  uint32_t msb;      // the sample's shift inside its 16-bit word: p010 holds it in bits 6..15
  bool even_size;    // defined for even widths and heights only (the 10-bit 4:2:0 frames)
  bool deint;        // the fused de-interlacing reader takes it (ph_yadif_pair_packed)
  bool chan_out;     // the channel kernel writes it (ph_chan_compose)
};
constexpr FmtDesc kFmts[] = {
    // id              name         src               planes rgb8   v420   wide   msb even   deint  chan_out
    {PH_FMT_V210,      "v210",      PH_SRC_V210,      1,     false, false, false, 0, false, true,  true},
    {PH_FMT_YUV422P10, "yuv422p10", PH_SRC_YUV422P10, 3,     false, false, true,  0, false, true,  true},
    {PH_FMT_YUV422P8,  "yuv422p8",  PH_SRC_YUV422P8,  3,     false, false, false, 0, false, true,  true},
    {PH_FMT_YUV420P,   "yuv420p",   PH_SRC_YUV420P,   3,     false, true,  false, 0, false, true,  true},
    {PH_FMT_NV12,      "nv12",      PH_SRC_NV12,      2,     false, true,  false, 0, false, true,  true},
    {PH_FMT_RGBA8,     "rgba8",     PH_SRC_RGBA8,     1,     true,  false, false, 0, false, false, true},
    {PH_FMT_BGRA8,     "bgra8",     PH_SRC_BGRA8,     1,     true,  false, false, 0, false, false, true},
    {PH_FMT_YUV420P10, "yuv420p10", PH_SRC_YUV420P10, 3,     false, true,  true,  0, true,  false, false},
    {PH_FMT_P010,      "p010",      PH_SRC_P010,      2,     false, true,  true,  6, true,  false, false},
};
constexpr int kFmtCount = (int)(sizeof kFmts / sizeof kFmts[0]);
constexpr bool fmt_rows_in_order() {
  for (int f = 0; f < kFmtCount; ++f)
    if (kFmts[f].id != f) return false;
  return true;
}
static_assert(fmt_rows_in_order(), "kFmts holds one row per PH_FMT_* value, in their order");

constexpr bool fmt_known(int f) { return f >= 0 && f < kFmtCount; }
constexpr const char *fmt_name(int f) { return fmt_known(f) ? kFmts[f].name : nullptr; }
constexpr int fmt_planes(int f) { return fmt_known(f) ? kFmts[f].planes : -1; }
constexpr bool fmt_planar(int f) { return fmt_planes(f) > 1; }  // YCbCr in planes: neither v210 nor packed RGB
constexpr bool fmt_cbcr(int f) { return fmt_planes(f) == 2; }   // Cb and Cr interleaved in one plane
constexpr bool fmt_rgb8(int f) { return fmt_known(f) && kFmts[f].rgb8; }
constexpr bool fmt_v420(int f) { return fmt_known(f) && kFmts[f].v420; }
constexpr bool fmt_wide(int f) { return fmt_known(f) && kFmts[f].wide; }
constexpr uint32_t fmt_msb(int f) { return fmt_known(f) ? kFmts[f].msb : 0u; }
constexpr bool fmt_even_size(int f) { return fmt_known(f) && kFmts[f].even_size; }
constexpr bool fmt_deint(int f) { return fmt_known(f) && kFmts[f].deint; }
constexpr bool fmt_chan_out(int f) { return fmt_known(f) && kFmts[f].chan_out; }

// a channel source's wire format: PH_SRC_* -> PH_FMT_* (-1: an f32 image, PH_SRC_NONE or no PH_SRC_* value), and back
constexpr int fmt_of_src(int src) {
  for (int f = 0; f < kFmtCount; ++f)
    if (kFmts[f].src == src) return f;
  return -1;
}
constexpr int src_of_fmt(int f) { return fmt_known(f) ? kFmts[f].src : PH_SRC_NONE; }
static_assert(fmt_of_src(PH_SRC_NONE) < 0 && fmt_of_src(PH_SRC_RGBA_F32) < 0, "f32 images have no wire format");

// ---- geometry: the planes as the reference's Readers / Writers lay them out (packer.ts:30-83) ------------------------------------
// v210: a line is the width rounded up to 48 pixels, 16 bytes per 6 (v210.ts:198-204)
constexpr uint32_t v210_pitch_bytes(uint32_t width) { return (width + 47 - ((width - 1) % 48)) * 8 / 3; }
// a line of the first plane in its samples (packed RGB: pixels)
constexpr uint32_t pack_pitch(int fmt, uint32_t width) {
  if (fmt_rgb8(fmt)) return width;  // rgba8.ts:103-105
  if (fmt == PH_FMT_V210) return width + 47 - ((width - 1) % 48);
  return width + 7 - ((width - 1) % 8);  // yuv422p10.ts:221
}
// bytes per sample of the first plane (packed RGB: per pixel; v210 lines are v210_pitch_bytes)
constexpr uint32_t fmt_sample_bytes(int f) { return fmt_rgb8(f) ? 4u : fmt_wide(f) ? 2u : 1u; }
// the plane sizes of a width x height frame; returns the number of planes (-1: not a PH_FMT_*).  A chroma plane has half the bytes of
// a Y line per line (4:2:2), on every other line (4:2:0); an interleaved CbCr plane holds both halves
constexpr int pack_plane_bytes(int fmt, uint32_t width, uint32_t height, size_t bytes[3]) {
  bytes[0] = bytes[1] = bytes[2] = 0;
  if (!fmt_known(fmt)) return -1;
  bytes[0] = fmt == PH_FMT_V210 ? (size_t)v210_pitch_bytes(width) * height : (size_t)pack_pitch(fmt, width) * fmt_sample_bytes(fmt) * height;
  const int shift = (fmt_v420(fmt) ? 1 : 0) + (fmt_cbcr(fmt) ? 0 : 1);
  for (int i = 1; i < fmt_planes(fmt); ++i) bytes[i] = bytes[0] >> shift;
  return fmt_planes(fmt);
}

}  // namespace ph
