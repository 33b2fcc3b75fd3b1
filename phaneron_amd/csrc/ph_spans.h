// ph_spans.h - the byte ranges a job reads and writes, and the one test that decides whether two jobs may sit in one launch.  Host
// only: plain C++17, no HIP.  The jobs of a shared launch are made side by side, so a job that reads what an earlier job of its
// launch writes (RAW), writes what one reads (WAR) or writes what one writes (WAW) starts the next launch: call order holds
// (include/phaneron_hip.h).  Every planner of shared launches - ph_run_programs' groups, ph_chan_compose_batch_out,
// ph_clip_compose_batch_out - builds a Footprint per job with the builders below and asks clashes(); sizes decide where launches end,
// so each site says at its call which sizes it takes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/phaneron_hip.h"
#include "ph_formats.h"

#pragma GCC visibility push(hidden)  // nothing here is exported: the C ABI is include/phaneron_hip.h
namespace ph {

struct Span {  // bytes a job reads or writes; for an output's planes also what lets two fields of one frame share a launch
  const char *p;
  size_t n;
  int fmt;             // an output's PH_FMT_* (-1: a source)
  uint32_t interlace;
};
// (the only comparison of two address ranges in the library; an empty span meets nothing)
inline bool spans_meet(const Span &a, const Span &b) { return a.n && b.n && a.p < b.p + b.n && b.p < a.p + a.n; }
// two outputs that may be written side by side although their bytes meet: the two fields of one frame (not 4:2:0: both fields of a
// line pair write the pair's chroma line, and the later call has to win)
inline bool spans_interleave(const Span &a, const Span &b) {
  return a.p == b.p && a.fmt >= 0 && a.fmt == b.fmt && !fmt_v420(a.fmt) && a.interlace && b.interlace && a.interlace != b.interlace;
}

// The limits the storage below is sized by (ph_internal.h holds them against ph_kernels.h's): a job has at most kSpanLayers layers of
// three images (src, incoming, mask) of three planes each - a compose_up pair's second field's images come to less - and at most
// kSpanOuts outputs of three planes.
constexpr int kSpanLayers = 8, kSpanOuts = 4;
struct Footprint {  // a job's reads and writes, held in place: planning allocates nothing per job
  int n_reads = 0, n_writes = 0;
  Span writes[kSpanOuts * 3], reads[kSpanLayers * 3 * 3];  // (the few writes first: a job of few ranges keeps to the struct's first cache lines)
  Footprint() {}  // (user-provided: an empty footprint is its two counts, the spans are not cleared)
};
enum : unsigned { kRAW = 1, kWAR = 2, kWAW = 4, kAllHazards = kRAW | kWAR | kWAW };
// May `later` not share a launch with `earlier`?  hazards: which of the three are asked; fields_interleave: two fields of one frame
// may be written side by side (spans_interleave) - the only exception there is, on WAW.
inline bool clashes(const Footprint &later, const Footprint &earlier, unsigned hazards, bool fields_interleave) {
  if (hazards & kRAW)
    for (int r = 0; r < later.n_reads; ++r)
      for (int w = 0; w < earlier.n_writes; ++w)
        if (spans_meet(later.reads[r], earlier.writes[w])) return true;
  for (int w = 0; w < later.n_writes; ++w) {
    if (hazards & kWAR)
      for (int r = 0; r < earlier.n_reads; ++r)
        if (spans_meet(later.writes[w], earlier.reads[r])) return true;
    if (hazards & kWAW)
      for (int v = 0; v < earlier.n_writes; ++v)
        if (spans_meet(later.writes[w], earlier.writes[v]) && !(fields_interleave && spans_interleave(later.writes[w], earlier.writes[v]))) return true;
  }
  return false;
}

// ---- builders: one per kind of range ---------------------------------------------------------------------------------------------
// a plain (pointer, bytes); a NULL pointer or no bytes is no range
inline void span_read(Footprint &f, const void *p, size_t bytes) {
  if (p && bytes) f.reads[f.n_reads++] = Span{(const char *)p, bytes, -1, 0u};
}
inline void span_write(Footprint &f, const void *p, size_t bytes, int fmt = -1, uint32_t interlace = 0u) {
  if (p && bytes) f.writes[f.n_writes++] = Span{(const char *)p, bytes, fmt, interlace};
}
// a ph_chan_source by its format: the bytes its planes hold - an f32 image 16 per pixel, a wire-format frame what its format's planes
// take (a range taken wider than that runs into whatever buffer lies behind the plane, and where the launches of a call end would
// depend on where its buffers were allocated).  A frame whose planes have no size of their own (odd dims, which the launch refuses)
// counts as the widest any format takes.  at_least: what a plane of no bytes is widened to (0: it is no range).
inline void span_read_source(Footprint &f, const ph_chan_source &s, size_t at_least) {
  if (!s.data) return;
  size_t pb[3];
  const int fmt = fmt_of_src(s.format);
  if (fmt < 0 || ((s.width | s.height) & 1) || pack_plane_bytes(fmt, (uint32_t)s.width, (uint32_t)s.height, pb) < 0)
    pb[0] = (size_t)s.width * s.height * 16u, pb[1] = pb[2] = (size_t)s.width * s.height * 2u;
  const void *const planes[3] = {s.data, s.data_u, s.data_v};
  for (int i = 0; i < 3; ++i) span_read(f, planes[i], pb[i] ? pb[i] : at_least);
}
// a source as the channel kernel's op list holds it (ChanSrc: ptr, pitch in bytes, h lines) with its chroma planes, sized as the kernel
// sizes them (ph_kernels_chan.hip planes_of): v420 - chroma on every other line; cbcr - one interleaved plane of the Y pitch
inline void span_read_planes(Footprint &f, const void *ptr, uint32_t pitch, uint32_t h, bool v420, bool cbcr, const void *plane_u, const void *plane_v) {
  span_read(f, ptr, (size_t)pitch * h);
  const size_t chroma = (size_t)(cbcr ? pitch : pitch >> 1) * (v420 ? (h + 1u) >> 1 : h);
  span_read(f, plane_u, chroma);
  span_read(f, plane_v, chroma);
}
// a ph_chan_output's planes at (w, h), as pack_plane_bytes sizes them (every plane of a 4:2:2 or packed frame has a row per line:
// fields interleave in all of them).  no_sizes: what plane 0 of a format without plane sizes counts as
inline void span_write_output(Footprint &f, const ph_chan_output &o, uint32_t w, uint32_t h, size_t no_sizes = 0) {
  size_t bytes[3];
  if (pack_plane_bytes(o.format, w, h, bytes) < 0) bytes[0] = no_sizes;
  for (int i = 0; i < 3; ++i) span_write(f, o.planes[i], bytes[i], o.format, o.interlace);
}

}  // namespace ph
#pragma GCC visibility pop
