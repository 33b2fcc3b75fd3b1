// spans_check.cpp - phaneron_amd/csrc/ph_spans.h on its own: the byte ranges of a job and the one hazard test the planners of shared
// launches ask.  Host only, no HIP: tests/test_spans_cpu.py compiles this file with the host compiler and runs it; it prints one line
// per failed check and exits 1 if there was any.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../phaneron_amd/csrc/ph_spans.h"

using namespace ph;

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("line %d: %s\n", __LINE__, #cond);                  \
      ++failures;                                                \
    }                                                            \
  } while (0)

static char arena[64 * 1024];  // addresses only: nothing is read or written through a span

static Footprint job(std::initializer_list<Span> reads, std::initializer_list<Span> writes) {
  Footprint f;
  for (const Span &r : reads) span_read(f, r.p, r.n);
  for (const Span &w : writes) span_write(f, w.p, w.n, w.fmt, w.interlace);
  return f;
}

static void check_spans_meet() {
  const Span a{arena, 8, -1, 0}, next{arena + 8, 8, -1, 0}, into{arena + 7, 8, -1, 0}, none{arena + 2, 0, -1, 0}, inside{arena + 2, 1, -1, 0};
  CHECK(!spans_meet(a, next) && !spans_meet(next, a));  // adjacent
  CHECK(spans_meet(a, into) && spans_meet(into, a));    // one byte in common
  CHECK(spans_meet(a, inside) && spans_meet(inside, a));
  CHECK(spans_meet(a, a));
  CHECK(!spans_meet(a, none) && !spans_meet(none, a) && !spans_meet(none, none));  // an empty span meets nothing
}

static void check_each_hazard_alone() {
  const Span x{arena, 16, -1, 0}, y{arena + 100, 16, -1, 0}, z{arena + 200, 16, -1, 0}, u{arena + 300, 16, -1, 0};
  const Footprint earlier = job({x}, {y});
  const Footprint raw = job({y}, {z}), war = job({z}, {x}), waw = job({z}, {y}), clear = job({x, z}, {u});
  for (unsigned mask = 0; mask <= kAllHazards; ++mask) {
    CHECK(clashes(raw, earlier, mask, false) == ((mask & kRAW) != 0));
    CHECK(clashes(war, earlier, mask, false) == ((mask & kWAR) != 0));
    CHECK(clashes(waw, earlier, mask, false) == ((mask & kWAW) != 0));
    CHECK(!clashes(clear, earlier, mask, false));  // (reading what another job reads is no hazard)
  }
}

static void check_field_exception() {
  // every pair of (first byte, format, interlace) against the rule in words: the same first byte, the same format, not 4:2:0, one the
  // upper field and the other the lower
  const int fmts[] = {-1, PH_FMT_V210, PH_FMT_YUV422P10, PH_FMT_YUV422P8, PH_FMT_YUV420P, PH_FMT_NV12, PH_FMT_RGBA8, PH_FMT_BGRA8, PH_FMT_YUV420P10, PH_FMT_P010};
  const uint32_t modes[] = {0, 1, 3};
  for (int pa = 0; pa < 2; ++pa)
    for (int fa : fmts)
      for (int fb : fmts)
        for (uint32_t ia : modes)
          for (uint32_t ib : modes) {
            const Span a{arena + 64 * pa, 4096, fa, ia}, b{arena, 4096, fb, ib};
            const bool v420 = fa == PH_FMT_YUV420P || fa == PH_FMT_NV12 || fa == PH_FMT_YUV420P10 || fa == PH_FMT_P010;
            const bool fields = pa == 0 && fa >= 0 && fa == fb && !v420 && ((ia == 1 && ib == 3) || (ia == 3 && ib == 1));
            CHECK(spans_interleave(a, b) == fields);
            const Footprint later = job({}, {a}), earlier = job({}, {b});
            CHECK(clashes(later, earlier, kWAW, /*fields_interleave*/ true) == !fields);
            CHECK(clashes(later, earlier, kWAW, /*fields_interleave*/ false));  // (the bytes meet in every pair)
          }
  // the exception is on WAW only: a job that READS a frame whose other field an earlier job writes starts the next launch
  const Span upper{arena, 4096, PH_FMT_YUV422P8, 1}, lower{arena, 4096, PH_FMT_YUV422P8, 3};
  CHECK(clashes(job({lower}, {}), job({}, {upper}), kAllHazards, true));
  CHECK(clashes(job({}, {lower}), job({upper}, {}), kAllHazards, true));
}

static void check_output_builder() {
  // the formats the channel kernel writes, at 48 x 4: their planes' bytes (v210: 128 bytes per line of 48 pixels)
  struct Case { int fmt; int planes; size_t bytes[3]; };
  const Case cases[] = {{PH_FMT_V210, 1, {512, 0, 0}},     {PH_FMT_YUV422P10, 3, {384, 192, 192}}, {PH_FMT_YUV422P8, 3, {192, 96, 96}}, {PH_FMT_YUV420P, 3, {192, 48, 48}},
                        {PH_FMT_NV12, 2, {192, 96, 0}},    {PH_FMT_RGBA8, 1, {768, 0, 0}},         {PH_FMT_BGRA8, 1, {768, 0, 0}}};
  int chan_out = 0;
  for (int f = 0; f < kFmtCount; ++f) chan_out += fmt_chan_out(f) ? 1 : 0;
  CHECK(chan_out == (int)(sizeof cases / sizeof cases[0]));  // (a format the channel kernel learns to write gets its row here)
  for (const Case &c : cases) {
    CHECK(fmt_chan_out(c.fmt));
    ph_chan_output o{};
    o.format = c.fmt, o.interlace = 3;
    for (int i = 0; i < 3; ++i) o.planes[i] = arena + 4096 * i;  // (a plane the format does not have is not looked at)
    Footprint f;
    span_write_output(f, o, 48, 4);
    size_t want[3];
    CHECK(pack_plane_bytes(c.fmt, 48, 4, want) == c.planes);
    CHECK(f.n_writes == c.planes && f.n_reads == 0);
    for (int i = 0; i < f.n_writes && i < 3; ++i) {
      CHECK(f.writes[i].p == arena + 4096 * i && f.writes[i].n == c.bytes[i] && f.writes[i].n == want[i]);
      CHECK(f.writes[i].fmt == c.fmt && f.writes[i].interlace == 3);
    }
  }
  // a format without plane sizes: nothing, or plane 0 at what the caller says it counts as
  ph_chan_output o{};
  o.format = 99, o.planes[0] = arena, o.planes[1] = arena + 4096;
  Footprint none, first;
  span_write_output(none, o, 48, 4);
  span_write_output(first, o, 48, 4, 512);
  CHECK(none.n_writes == 0);
  CHECK(first.n_writes == 1 && first.writes[0].p == arena && first.writes[0].n == 512);
  // a missing plane is no range
  o.format = PH_FMT_YUV422P8, o.planes[1] = nullptr, o.planes[2] = arena + 8192;
  Footprint two;
  span_write_output(two, o, 48, 4);
  CHECK(two.n_writes == 2 && two.writes[1].p == arena + 8192);
}

static void check_source_builders() {
  ph_chan_source s{};
  s.data = arena, s.data_u = arena + 8192, s.data_v = arena + 16384;
  auto sizes = [&](int format, int w, int h, size_t at_least, size_t n0, size_t n1, size_t n2, int line) {
    s.format = format, s.width = w, s.height = h;
    Footprint f;
    span_read_source(f, s, at_least);
    const size_t want[3] = {n0, n1, n2};
    int at = 0;
    for (int i = 0; i < 3; ++i)
      if (want[i]) {
        const void *const planes[3] = {s.data, s.data_u, s.data_v};
        if (at >= f.n_reads || f.reads[at].p != planes[i] || f.reads[at].n != want[i]) printf("line %d: plane %d\n", line, i), ++failures;
        ++at;
      }
    if (at != f.n_reads) printf("line %d: %d ranges, not %d\n", line, f.n_reads, at), ++failures;
  };
  sizes(PH_SRC_RGBA_F32, 10, 3, 0, 480, 60, 60, __LINE__);    // an f32 image: 16 bytes per pixel (chroma pointers, if any: the fallback's 2)
  sizes(PH_SRC_YUV420P, 16, 4, 0, 64, 16, 16, __LINE__);      // a frame: its format's planes
  sizes(PH_SRC_YUV420P, 15, 5, 0, 1200, 150, 150, __LINE__);  // odd 4:2:0 dims: the widest any format takes
  sizes(PH_SRC_NV12, 16, 4, 0, 64, 32, 0, __LINE__);
  sizes(PH_SRC_YUV422P10, 16, 4, 0, 128, 64, 64, __LINE__);
  sizes(PH_SRC_V210, 48, 4, 0, 512, 0, 0, __LINE__);          // a plane of no bytes: no range ...
  sizes(PH_SRC_V210, 48, 4, 1, 512, 1, 1, __LINE__);          // ... or widened to one byte
  sizes(PH_SRC_V210, 48, 0, 1, 1, 1, 1, __LINE__);
  s.data_u = s.data_v = nullptr;
  sizes(PH_SRC_V210, 48, 4, 1, 512, 0, 0, __LINE__);          // (a NULL plane stays no range)
  s.data = nullptr, s.data_u = arena + 8192;
  sizes(PH_SRC_V210, 48, 4, 1, 0, 0, 0, __LINE__);            // no source at all
  // the channel kernel's op list: pitch in bytes, h lines, the chroma planes as the kernel sizes them
  for (int fmt : {PH_FMT_YUV422P10, PH_FMT_YUV422P8, PH_FMT_YUV420P, PH_FMT_NV12, PH_FMT_YUV420P10, PH_FMT_P010}) {
    size_t want[3];
    const int planes = pack_plane_bytes(fmt, 64, 6, want);
    const uint32_t pitch = pack_pitch(fmt, 64) * fmt_sample_bytes(fmt);
    Footprint f;
    span_read_planes(f, arena, pitch, 6, fmt_v420(fmt), fmt_cbcr(fmt), arena + 8192, planes == 3 ? arena + 16384 : nullptr);
    CHECK(f.n_reads == planes);
    for (int i = 0; i < f.n_reads && i < 3; ++i) CHECK(f.reads[i].n == want[i] && f.reads[i].p == arena + 8192 * i);
  }
  Footprint odd, packed;
  span_read_planes(odd, arena, 64, 5, true, false, arena + 8192, arena + 16384);  // 4:2:0 of an odd height: the last line has its chroma line
  CHECK(odd.n_reads == 3 && odd.reads[0].n == 320 && odd.reads[1].n == 96 && odd.reads[2].n == 96);
  span_read_planes(packed, arena, 128, 4, false, false, nullptr, nullptr);
  CHECK(packed.n_reads == 1 && packed.reads[0].n == 512);
}

// a seeded brute force over a 64-byte address space against a model that marks bytes
static uint64_t bytes_of(const Span *s, int n) {
  uint64_t m = 0;
  for (int i = 0; i < n; ++i)
    for (size_t b = 0; b < s[i].n; ++b) m |= 1ull << (size_t)(s[i].p - arena + b);
  return m;
}
static void check_brute_force() {
  uint32_t seed = 20240611u;
  auto rnd = [&](uint32_t n) { return ((seed = seed * 1664525u + 1013904223u) >> 16) % n; };
  int clashed = 0, clear = 0;
  for (int round = 0; round < 5000; ++round) {
    Footprint f[2];
    for (Footprint &fp : f) {
      for (uint32_t r = rnd(4); r; --r) { const uint32_t at = rnd(56); span_read(fp, arena + at, rnd(9)); }
      for (uint32_t w = rnd(3); w; --w) { const uint32_t at = rnd(56); span_write(fp, arena + at, rnd(9)); }
    }
    const uint64_t r1 = bytes_of(f[0].reads, f[0].n_reads), w1 = bytes_of(f[0].writes, f[0].n_writes);
    const uint64_t r0 = bytes_of(f[1].reads, f[1].n_reads), w0 = bytes_of(f[1].writes, f[1].n_writes);
    for (unsigned mask = 0; mask <= kAllHazards; ++mask) {
      const bool model = ((mask & kRAW) && (r1 & w0)) || ((mask & kWAR) && (w1 & r0)) || ((mask & kWAW) && (w1 & w0));
      CHECK(clashes(f[0], f[1], mask, false) == model);
      CHECK(clashes(f[0], f[1], mask, true) == model);  // (sources and plain ranges carry no format: no exception applies)
      clashed += model ? 1 : 0, clear += model ? 0 : 1;
    }
  }
  CHECK(clashed > 1000 && clear > 1000);  // (the rounds exercise both answers)
}

int main() {
  check_spans_meet();
  check_each_hazard_alone();
  check_field_exception();
  check_output_builder();
  check_source_builders();
  check_brute_force();
  printf("%d failed checks\n", failures);
  return failures ? 1 : 0;
}
