// ph_fused_field.h - a FIELD quad's place in the frame, for the plain-layer launches that compose one field only
// (ph_kernels_fused_field.hip; context option "fused_fields") and for the host, which tests it (ph_debug_fused_field_quad).
//
// A field of a frame of `quads_per_line` quads per line (width % 48 == 0: a line is whole quads) is the lines first_line, first_line + 2,
// ...: field_lines = height / 2 of them.  Its quads are numbered g = 0 .. quads_per_line * field_lines - 1 in raster order, and the
// kernels divide, tile and bound their work in these.  What they load and store at is the frame's:
//   fl   = g / quads_per_line       the field line, by the reciprocal magic_qpl = ceil(2^32 / quads_per_line) - exact while
//                                   g * quads_per_line < 2^32, which the launchers' frame bound (total_quads * quads_per_line < 2^32) gives
//   col  = g - fl * quads_per_line  the quad's place in its line
//   line = 2 * fl + first_line      the frame line
//   f    = g + (fl + first_line) * quads_per_line == line * quads_per_line + col: the frame's flat quad
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ph {

struct FieldQuad {
  uint32_t f, line, col;
};

static inline __host__ __device__ FieldQuad fused_field_quad(uint32_t g, uint32_t quads_per_line, uint32_t magic_qpl, uint32_t first_line) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t fl = __umulhi(g, magic_qpl);
#else
  const uint32_t fl = (uint32_t)(((uint64_t)g * magic_qpl) >> 32);
#endif
  FieldQuad q;
  q.col = g - fl * quads_per_line;
  q.line = 2u * fl + first_line;
  q.f = g + (fl + first_line) * quads_per_line;
  return q;
}

}  // namespace ph
