// ph_run.cpp - programs and their by-name jobs: the nodencl `runProgram` contract the reference's clJobQueue drives.  A job is a
// program (a kernel chosen by name: ph_program.cpp) and a list of NAMED arguments; ph_run_program, ph_check_program and
// ph_run_programs turn it into one of the typed calls of include/phaneron_hip.h - the only way this file reaches a kernel.
// How an argument is found, type-checked, size-checked and reported is decided in one place: struct Args.
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ph_internal.h"

using namespace ph;  // K_* kernel ids, the fmt_* traits

namespace {

// the Loader's triple and the Saver's pair of a job, as the buffers the job names (the parts a program does not take stay null):
// jobs that share one launch have to name the same ones
struct Recipe {
  ph_buf *rd_cm = nullptr, *rd_lut = nullptr, *rd_gm = nullptr, *wr_cm = nullptr, *wr_lut = nullptr;
  bool operator==(const Recipe &o) const { return rd_cm == o.rd_cm && rd_lut == o.rd_lut && rd_gm == o.rd_gm && wr_cm == o.wr_cm && wr_lut == o.wr_lut; }
};
const void *dptr(const ph_buf *b) { return b ? b->dptr : nullptr; }

ph_buf *const g_no_buf = new ph_buf{nullptr, nullptr, nullptr, SIZE_MAX, 0, 0, {0}, false, false, false, ""};  // what a read hands out once the job has failed (never freed)

// The reader of a job's named arguments.  The FIRST defect found is the job's error (rc, and ph_last_error's text): every read after
// it does nothing and hands out a harmless value - a number's default, g_no_buf - so a parser reads its arguments in a straight
// line and asks once, at the end, whether there is anything to launch (done()).  Names are printf formats: "l%dIn", i.
struct Args {
  ph_ctx *ctx;
  const ph_program *prog;
  const ph_arg *args;
  int n;
  bool check_only;  // everything up to the launch - names, kinds, buffer sizes, geometry - and nothing on the device (ph_check_program)
  int rc = PH_OK;
  const char *name = "";  // the argument read last
  char built[48];

#define PH_ARG_NAME(fmt)     \
  do {                       \
    va_list ap_;             \
    va_start(ap_, fmt);      \
    set_name(fmt, ap_);      \
    va_end(ap_);             \
  } while (0)
  void set_name(const char *fmt, va_list ap) {
    name = fmt;
    if (!strchr(fmt, '%')) return;
    vsnprintf(built, sizeof built, fmt, ap);
    name = built;
  }
  Args &named(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    PH_ARG_NAME(fmt);
    return *this;
  }

  int fail(int code, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
    if (rc) return rc;
    char text[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    return rc = ::fail(code, "%s", text);
  }
  bool done() const { return rc != PH_OK || check_only; }  // nothing (more) to do: return rc

  // ---- the argument called `name` ----
  const ph_arg *find_arg() const {
    for (int i = 0; i < n; ++i)
      if (args[i].name && 0 == strcmp(args[i].name, name)) return &args[i];
    return nullptr;
  }
  ph_buf *need_buf(size_t min_bytes) {
    if (rc) return g_no_buf;
    const ph_arg *a = find_arg();
    if (!a || a->kind != PH_ARG_BUF || !a->v.buf) return fail(PH_E_INVALID, "kernel argument '%s' (buffer) missing", name), g_no_buf;
    if (a->v.buf->bytes < min_bytes)
      return fail(PH_E_RANGE, "kernel argument '%s': buffer of %zu bytes, %zu needed", name, a->v.buf->bytes, min_bytes), g_no_buf;
    return a->v.buf;
  }
  double need_num(double otherwise) {
    if (rc) return otherwise;
    const ph_arg *a = find_arg();
    if (!a || a->kind == PH_ARG_BUF) return fail(PH_E_INVALID, "kernel argument '%s' (number) missing", name), otherwise;
    return a->kind == PH_ARG_F32 ? (double)a->v.f32 : a->kind == PH_ARG_I32 ? (double)a->v.i32 : (double)a->v.u32;
  }
  // b's dims, b being an image buffer (createBuffer with imageDims)
  void need_image(const ph_buf *b, int *w, int *h) {
    *w = *h = 0;
    if (rc) return;
    if (b->width <= 0 || b->height <= 0) return (void)fail(PH_E_INVALID, "kernel argument '%s' is not an image buffer", name);
    if (b->bytes < (size_t)b->width * b->height * 16) return (void)fail(PH_E_RANGE, "image '%s' smaller than its dims", name);
    *w = b->width, *h = b->height;
  }

  // ---- what the parsers ask for ----
  bool has(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    PH_ARG_NAME(fmt);
    return find_arg() != nullptr;
  }
  ph_buf *buf(size_t min_bytes, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {
    PH_ARG_NAME(fmt);
    return need_buf(min_bytes);
  }
  ph_buf *buf_or_null(size_t min_bytes, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {  // an optional buffer
    PH_ARG_NAME(fmt);
    return find_arg() ? need_buf(min_bytes) : nullptr;
  }
  double num(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    PH_ARG_NAME(fmt);
    return need_num(0);
  }
  double num_or(double otherwise, const char *fmt, ...) __attribute__((format(printf, 3, 4))) {  // an optional number
    PH_ARG_NAME(fmt);
    return find_arg() ? need_num(otherwise) : otherwise;
  }
  ph_buf *image(int *w, int *h, const char *fmt, ...) __attribute__((format(printf, 4, 5))) {
    PH_ARG_NAME(fmt);
    ph_buf *b = need_buf(0);
    need_image(b, w, h);
    return b;
  }
  // a 65536-entry f32 table; a launch takes the LDS form of what its host mirror holds now
  ph_buf *table(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
    PH_ARG_NAME(fmt);
    ph_buf *b = need_buf(65536 * 4);
    if (!done()) refresh_buf_lut(ctx, b);
    return b;
  }
  // a placement: a buffer whose HOST mirror holds the nine floats (Transform writes it through hostAccess: transform.ts:84-89)
  const float *host_matrix(const ph_buf *m) {
    if (!rc && !m->hptr) fail(PH_E_INVALID, "kernel argument '%s': the matrix must have been written through hostAccess (its host copy is what the launch reads)", name);
    return (const float *)m->hptr;
  }
  // colMatrix / gammaLut / gamutMatrix: the Loader's (a Writer of one format names its own two the same way)
  void loader(Recipe *r, bool col_matrix = true, bool gamut = true) {
    if (col_matrix) r->rd_cm = buf(48, "colMatrix");
    r->rd_lut = table("gammaLut");
    if (gamut) r->rd_gm = buf(36, "gamutMatrix");
  }
  // outColMatrix / outGammaLut: the Saver's
  void saver(Recipe *r, bool col_matrix = true) {
    if (col_matrix) r->wr_cm = buf(48, "outColMatrix");
    r->wr_lut = table("outGammaLut");
  }
  // the frame a 2-D program makes: globalWorkItems
  void frame(uint32_t *width, uint32_t *height) {
    *width = prog->global[0], *height = prog->global[1];
    if (!*width || !*height) fail(PH_E_INVALID, "%s: globalWorkItems must be [width, height]", prog->kernel.c_str());
  }
  // the plane sizes of a frame (the format's pack_plane_bytes); the number of planes, < 0 where the format has no such frame
  int plane_bytes(int fmt, uint32_t width, uint32_t height, size_t pb[3]) {
    pb[0] = pb[1] = pb[2] = 0;
    return rc ? -1 : ph_pack_plane_bytes(fmt, width, height, pb);
  }
  // the planes of a frame: <prefix> where the format has one, else <prefix><y>, <prefix>C (nv12.ts:374) or <prefix><y>, <prefix>U, <prefix>V
  int planes(int fmt, uint32_t width, uint32_t height, const char *prefix, const char *y, void *out[3]) {
    size_t pb[3];
    const int np = plane_bytes(fmt, width, height, pb);
    for (int i = 0; i < np; ++i) out[i] = buf(pb[i], "%s%s", prefix, np == 1 ? "" : i == 0 ? y : np == 2 ? "C" : i == 1 ? "U" : "V")->dptr;
    return np;
  }
#undef PH_ARG_NAME
};

size_t v210_bytes(uint32_t width, uint32_t height) { return (size_t)ph_v210_pitch_bytes(width) * height; }
size_t image_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * 16; }

}  // namespace

extern "C" {

// ---- programs ---------------------------------------------------------------------------------
int ph_program_resolve(const char *src, const char *name, char *kernel_id, size_t kernel_id_len, int *format, int *how) {
  ph::ProgramChoice c;
  std::string err;
  const int rc = ph::resolve_program(src, name, c, err);
  if (rc != PH_OK) return fail(rc, "%s", err.c_str());
  if (kernel_id && kernel_id_len) snprintf(kernel_id, kernel_id_len, "%s", c.kernel.c_str());
  if (format) *format = (c.id <= K_V210_WRITE) ? c.format : -1;
  if (how) *how = c.how;
  return PH_OK;
}

int ph_program_create(ph_ctx *ctx, const char *src, const char *name, const uint32_t *gwi, int n_dims, uint32_t wipg,
                      ph_program **out) {
  if (!ctx || !name || !out) return fail(PH_E_INVALID, "ph_program_create: NULL argument");
  ph::ProgramChoice c;
  std::string err;
  const int rc = ph::resolve_program(src, name, c, err);
  if (rc != PH_OK) return fail(rc, "%s", err.c_str());
  ph_program p{ctx, c.id, c.n_layers, c.format, c.kernel, {0, 0}, wipg};
  for (int i = 0; i < n_dims && i < 2; ++i) p.global[i] = gwi ? gwi[i] : 0;
  if (ctx->closed.load()) return closed_error("ph_program_create");
  *out = new ph_program(p);
  ctx_ref(ctx);
  return PH_OK;
}

int ph_program_destroy(ph_program *p) {
  if (!p) return PH_OK;
  ph_ctx *ctx = p->ctx;
  delete p;
  ctx_unref(ctx);
  return PH_OK;
}

const char *ph_program_kernel(const ph_program *p) { return p ? p->kernel.c_str() : ""; }

// nodencl lets a caller map a buffer for writing (hostAccess('writeonly')), fill it and launch
// without an explicit unmap (loadSave.ts:76-99): flush such mirrors on the launch queue first.
static int flush_dirty_args(ph_ctx *ctx, const ph_arg *args, int n, int queue) {
  for (int i = 0; i < n; ++i) {
    if (args[i].kind != PH_ARG_BUF || !args[i].v.buf) continue;
    ph_buf *b = args[i].v.buf;
    if (b->host_dirty && b->hptr) {
      hipStream_t s = stream_of(ctx, queue);
      PH_HIP(hipMemcpyAsync(b->dptr, b->hptr, b->bytes, hipMemcpyHostToDevice, s));
      mirror_mark(b, s);
      b->host_dirty = false;
      b->lut_dirty = b->lut_dirty || b->bytes >= 65536 * 4;
    }
  }
  return PH_OK;
}

// A channel's frame as the by-name program chan_compose_v210_<n> describes it (dispatch K_CHAN_COMPOSE; ph_run_programs puts several
// such calls into one launch): the arguments checked and turned into ph_chan_compose's own.
struct ChanCall {
  ph_chan_layer layers[ph::kMaxLayers];
  int n_layers, out_format;
  uint32_t width, height, interlace;
  void *out_planes[3];
  Recipe r;
  // chan_compose_multi_<n>: every output as ph_chan_compose_multi takes it (outs[0]: the one above)
  bool multi;  // the program is chan_compose_multi_<n> - or clip_compose_multi_<n>, which names its arguments the same
  bool clip;   // the program is clip_compose_multi_<n>: ph_clip_compose_multi, a launch of its own in its turn (option "clip_batch": grouped, ph_clip_compose_batch_out)
  bool clip_trans;  // the program is clip_compose_trans_<n>: ph_clip_compose_transition_multi, always a launch of its own in its turn
  // the program is clip_compose_route_<n>: ph_clip_compose_route_multi, always a launch of its own in its turn.  image_out: the optional
  // buffer imageOut, the combined f32 RGBA image; `output` may be absent only where imageOut is there (n_out == 0: the image alone)
  bool clip_route;
  void *image_out;
  int n_out;
  ph_chan_output outs[ph::kMaxChanOuts];
};
// l<i>In: a layer's source - a v210 frame (l<i>Width / l<i>Height: its size, default the output's) or an RGBA image buffer;
// l<i>Matrix (optional): its placement, a buffer whose host mirror holds the nine floats (Transform writes it through
// hostAccess: transform.ts:84-89), absent = 1:1; l<i>Transition: 0 cut / 1 dissolve / 2 wipe; l<i>Mix; l<i>Incoming(In|Matrix|
// Width|Height) and l<i>Mask(...): the transition's other sources; output: v210; colMatrix / gammaLut / gamutMatrix: the
// Loader's, outColMatrix / outGammaLut: the Saver's; interlace as 'write'
static void chan_source_parse(Args &a, int i, const char *role, uint32_t width, uint32_t height, ph_chan_source *s) {
  const ph_buf *x = a.buf(0, "l%d%sIn", i, role);
  double sw = width, sh = height;
  s->data = x->dptr;
  if (x->width > 0 && x->height > 0) {  // an image buffer (createBuffer with imageDims): f32 RGBA
    s->format = PH_SRC_RGBA_F32, sw = x->width, sh = x->height;
  } else {
    s->format = PH_SRC_V210;
    // another wire format: l<i>Packing = its PH_FMT_* (1 yuv422p10, 2 yuv422p8, 3 yuv420p, 4 nv12, 7 yuv420p10, 8 p010: l<i>In the Y plane,
    // l<i>InU / l<i>InV the chroma planes (nv12, p010: l<i>InU the CbCr plane), l<i>ColMatrix (optional) its own Loader matrix; 5 rgba8,
    // 6 bgra8: l<i>In the frame)
    const double packing = a.num_or(0, "l%d%sPacking", i, role);
    if (packing != 0) {
      if (packing < PH_FMT_YUV422P10 || packing >= kFmtCount) return (void)a.fail(PH_E_INVALID, "kernel argument '%s': %g is not a pack format other than v210", a.name, packing);
      s->format = src_of_fmt((int)packing);  // (PH_FMT_V210 is 0: every value from 1 on is another format)
    }
    sw = a.num_or(sw, "l%d%sWidth", i, role);
    sh = a.num_or(sh, "l%d%sHeight", i, role);
    const int fmt = fmt_of_src(s->format);
    if (fmt_rgb8(fmt)) {
      if (sw > 0 && sh > 0 && x->bytes < (size_t)sw * (size_t)sh * 4) return (void)a.fail(PH_E_RANGE, "kernel argument 'l%d%sIn': buffer of %zu bytes is smaller than a %gx%g frame of 4 bytes per pixel", i, role, x->bytes, sw, sh);
    } else if (fmt_planar(fmt)) {
      size_t pb[3];
      if (sw > 0 && sh > 0) a.plane_bytes(fmt, (uint32_t)sw, (uint32_t)sh, pb);
      else pb[0] = pb[1] = pb[2] = 0;
      s->data_u = a.buf(pb[1], "l%d%sInU", i, role)->dptr;
      if (fmt_planes(fmt) == 3) s->data_v = a.buf(pb[2], "l%d%sInV", i, role)->dptr;
      s->col_matrix12 = dptr(a.buf_or_null(48, "l%d%sColMatrix", i, role));
      if (x->bytes < pb[0]) return (void)a.fail(PH_E_RANGE, "kernel argument 'l%d%sIn': buffer of %zu bytes is smaller than the Y plane of a %gx%g frame", i, role, x->bytes, sw, sh);
    } else if (sw > 0 && sh > 0 && x->bytes < (size_t)ph_v210_pitch_bytes((uint32_t)sw) * (size_t)sh)
      return (void)a.fail(PH_E_RANGE, "kernel argument 'l%d%sIn': buffer of %zu bytes is smaller than a %gx%g v210 frame", i, role, x->bytes, sw, sh);
  }
  s->width = (int)sw, s->height = (int)sh;
  if (const ph_buf *m = a.buf_or_null(36, "l%d%sMatrix", i, role)) s->matrix9_host = a.host_matrix(m);
}
// One output of a channel's frame.  Output 0 is named as chan_compose_v210_<n> names its only one (outPacking, output, outputU / V / C,
// outColMatrix, outGammaLut, interlace); output k = 1..3 of chan_compose_multi_<n> puts its number behind the first word (out<k>Packing,
// output<k>, output<k>U ..., out<k>ColMatrix, out<k>GammaLut, interlace<k>).  The same reads, checks and texts for all of them.
// any_format: the program writes every pack format (pack_write_multi_<n>), not only those the channel kernel does
static int chan_output_parse(Args &a, int k, uint32_t width, uint32_t height, ph_chan_output *o, ph_buf **wr_cm, ph_buf **wr_lut, Recipe *loader = nullptr,
                             bool any_format = false) {
  char num[4] = "", packing_arg[48], refused[80], prefix[16];
  if (k) snprintf(num, sizeof num, "%d", k);
  snprintf(packing_arg, sizeof packing_arg, "out%sPacking", num);
  snprintf(prefix, sizeof prefix, "output%s", num);
  // the packed frame - v210, or with outPacking = PH_FMT_* another wire format: 1 yuv422p10 / 2 yuv422p8 / 3 yuv420p (output = the Y
  // plane, outputU, outputV), 4 nv12 (output, outputC), 5 rgba8 / 6 bgra8 (no outColMatrix)
  const double out_packing = a.num_or(0, "%s", packing_arg);
  const int ofmt = (int)out_packing;
  if (!fmt_known(ofmt)) return a.fail(PH_E_INVALID, "kernel argument '%s': %g is not a pack format", packing_arg, out_packing);
  snprintf(refused, sizeof refused, "kernel argument '%s'", packing_arg);
  if (!a.rc && !any_format && !fmt_chan_out(ofmt)) return a.rc = chan_out_refused(refused, ofmt);
  o->planes[0] = o->planes[1] = o->planes[2] = nullptr;
  if (a.planes(ofmt, width, height, prefix, "", o->planes) < 0) return a.fail(PH_E_INVALID, "kernel argument '%s': %g is not a pack format", packing_arg, out_packing);
  if (loader) a.loader(loader);  // (output 0: the Loader's triple is read here, between the frame and the Saver's pair, as it always was)
  *wr_cm = fmt_rgb8(ofmt) ? nullptr : a.buf(48, "out%sColMatrix", num);
  *wr_lut = a.table("out%sGammaLut", num);
  o->format = ofmt, o->interlace = (uint32_t)a.num_or(0, "interlace%s", num);
  o->wr_col_matrix12 = dptr(*wr_cm), o->wr_gamma_lut = (*wr_lut)->dptr;
  return a.rc;
}
static int chan_call_parse(Args &a, ChanCall *call) {
  const int n_layers = a.prog->n_layers;
  uint32_t width, height;
  a.frame(&width, &height);
  memset(call->layers, 0, sizeof call->layers);
  for (int i = 0; i < n_layers; ++i) {
    ph_chan_layer &l = call->layers[i];
    chan_source_parse(a, i, "", width, height, &l.src);
    l.transition = (int)a.num_or(0, "l%dTransition", i), l.mix = (float)a.num_or(0, "l%dMix", i);
    if (l.transition != PH_TRANSITION_CUT) chan_source_parse(a, i, "Incoming", width, height, &l.incoming);
    if (l.transition == PH_TRANSITION_WIPE) chan_source_parse(a, i, "Mask", width, height, &l.mask);
  }
  call->r = Recipe();
  call->clip = a.prog->kernel.compare(0, 19, "clip_compose_multi_") == 0;
  call->clip_trans = a.prog->kernel.compare(0, 19, "clip_compose_trans_") == 0;
  call->clip_route = a.prog->kernel.compare(0, 19, "clip_compose_route_") == 0;
  call->multi = call->clip || call->clip_trans || call->clip_route || a.prog->kernel.compare(0, 19, "chan_compose_multi_") == 0;
  call->image_out = nullptr;
  if (call->clip_route)
    if (const ph_buf *image = a.buf_or_null(image_bytes(width, height), "imageOut")) call->image_out = image->dptr;
  if (call->image_out && !a.has("output")) {  // the image alone: no packed frame at all
    call->outs[0] = ph_chan_output{};
    call->n_out = 0;
    a.loader(&call->r);
  } else {
    chan_output_parse(a, 0, width, height, &call->outs[0], &call->r.wr_cm, &call->r.wr_lut, &call->r);
    call->n_out = 1;
  }
  if (call->multi && call->n_out) {  // the outputs named, in turn
    ph_buf *wr_cm, *wr_lut;
    for (int k = 1; k < ph::kMaxChanOuts && !a.rc && a.has("output%d", k); ++k) chan_output_parse(a, k, width, height, &call->outs[call->n_out++], &wr_cm, &wr_lut);
  }
  const int ofmt = call->outs[0].format;
  for (int p = 0; p < 3; ++p) call->out_planes[p] = call->outs[0].planes[p];
  call->interlace = call->outs[0].interlace;
  call->n_layers = n_layers, call->out_format = ofmt, call->width = width, call->height = height;
  return a.rc;
}

// fused_v210_combine_<n> (dispatch K_FUSED_V210; ph_run_programs puts several such calls of one shape into one launch):
// l<i>In: v210 sources; colMatrix / gammaLut / gamutMatrix: the Loader's; outColMatrix / outGammaLut: the Saver's
struct FusedCall {
  const void *layers[ph::kMaxLayers];
  int n;
  void *out;
  uint32_t width, height;
  size_t frame_bytes;
  Recipe r;
};
static int fused_call_parse(Args &a, FusedCall *call) {
  call->n = a.prog->n_layers;
  a.frame(&call->width, &call->height);
  call->frame_bytes = v210_bytes(call->width, call->height);
  for (int i = 0; i < call->n; ++i) call->layers[i] = a.buf(call->frame_bytes, "l%dIn", i)->dptr;
  call->out = a.buf(call->frame_bytes, "output")->dptr;
  call->r = Recipe();
  a.loader(&call->r);
  a.saver(&call->r);
  return a.rc;
}

// fused_v210_combine_multi_<n> (K_FUSED_V210, told apart by its name): l<i>In and the Loader's triple as fused_v210_combine_<n> names them; the
// outputs as chan_compose_multi_<n> names them (chan_output_parse: outPacking, output, outputU / V / C, outColMatrix, outGammaLut, interlace,
// then out<k>Packing, output<k>[U|V|C], out<k>ColMatrix, out<k>GammaLut, interlace<k> while output<k> is there, k = 1..3)
static bool fused_is_multi(const ph_program *prog) { return prog->kernel.compare(0, 25, "fused_v210_combine_multi_") == 0; }
// (ph_run_programs, with the context option "fused_multi_batch", puts several such calls of one shape into one launch)
struct FusedMultiCall {
  int n, n_out;
  const void *layers[ph::kMaxLayers];
  ph_chan_output outs[ph::kMaxFusedOuts];
  uint32_t width, height;
  Recipe r;  // (the Loader's triple; the Saver's pair of output 0)
  // fused_v210_route_<n>: which layers are f32 RGBA images, and the combined image's buffer (or NULL)
  int format[ph::kMaxLayers];
  void *image_out;
};
// route: the program is fused_v210_route_<n> - l<i>Image, imageOut, and no `output` at all where imageOut is there
static int fused_multi_parse(Args &a, FusedMultiCall *call, bool route = false) {
  const int n = call->n = a.prog->n_layers;
  uint32_t &width = call->width, &height = call->height;
  a.frame(&width, &height);
  const void **layers = call->layers;
  for (int i = 0; i < n; ++i) {
    const double image = route ? a.num_or(0, "l%dImage", i) : 0;
    if (image != 0 && image != 1) return a.fail(PH_E_INVALID, "kernel argument 'l%dImage': %g (0: l%dIn is a v210 frame, 1: an f32 RGBA image)", i, image, i);
    call->format[i] = image != 0 ? PH_SRC_RGBA_F32 : PH_SRC_V210;
    layers[i] = a.buf(image != 0 ? image_bytes(width, height) : v210_bytes(width, height), "l%dIn", i)->dptr;
  }
  Recipe &r = call->r = Recipe();
  ph_chan_output *outs = call->outs;
  int &n_out = call->n_out = 1;
  call->image_out = nullptr;
  if (route) {
    if (const ph_buf *image = a.buf_or_null(image_bytes(width, height), "imageOut")) call->image_out = image->dptr;
    for (int i = 0; i < n && !a.rc && call->image_out; ++i)
      if (layers[i] == call->image_out) return a.fail(PH_E_INVALID, "kernel argument 'imageOut': the buffer is layer %d's too", i);
  }
  if (call->image_out && !a.has("output")) {  // the image alone
    n_out = 0;
    a.loader(&r);
    return a.rc;
  }
  chan_output_parse(a, 0, width, height, &outs[0], &r.wr_cm, &r.wr_lut, &r);
  for (int k = 1; k < ph::kMaxFusedOuts && !a.rc && a.has("output%d", k); ++k) {
    ph_buf *wr_cm, *wr_lut;
    chan_output_parse(a, k, width, height, &outs[n_out++], &wr_cm, &wr_lut);
  }
  // what the typed call refuses about the outputs together, so that a check answers as a launch does
  for (int k = 0; k < n_out && !a.rc; ++k) {
    char num[4] = "";
    if (k) snprintf(num, sizeof num, "%d", k);
    if (outs[k].interlace != 0 && outs[k].interlace != 1 && outs[k].interlace != 3) return a.fail(PH_E_INVALID, "kernel argument 'interlace%s': must be 0, 1 or 3", num);
    if (fmt_v420(outs[k].format) && (height & 1)) return a.fail(PH_E_INVALID, "kernel argument 'out%sPacking': a 4:2:0 frame needs an even height (%u)", num, height);
    for (int j = 0; j < k; ++j)
      if (outs[j].planes[0] == outs[k].planes[0]) return a.fail(PH_E_INVALID, "kernel argument 'output%d': the buffer is another output's too", k);
    if (call->image_out && outs[k].planes[0] == call->image_out) return a.fail(PH_E_INVALID, "kernel argument 'imageOut': the buffer is output %d's too", k);
  }
  return a.rc;
}
static int fused_multi_job(Args &a, int queue) {
  FusedMultiCall c;
  if (const int rc = fused_multi_parse(a, &c)) return rc;
  return a.done() ? a.rc : ph_fused_v210_combine_multi(a.ctx, queue, c.n, c.layers, c.n_out, c.outs, c.width, c.height, c.r.rd_cm->dptr, c.r.rd_lut->dptr, c.r.rd_gm->dptr);
}
// fused_v210_trans_<n> (K_FUSED_V210, told apart by its name; ph_fused_v210_transition_multi): fused_v210_combine_multi_<n>'s arguments and,
// per layer, the keys compose_up_trans_<n> has for a transition - l<i>Transition (0 cut / 1 dissolve / 2 wipe, default 0), l<i>Mix,
// l<i>IncomingIn: a v210 frame of the output's size; a wipe's l<i>MaskIn with l<i>MaskPacking: 0 (PH_FMT_V210) a v210 frame, absent an f32
// RGBA image of the output's size.  A launch of its own, in its turn (ph_run_programs does not group it).
static bool fused_is_trans(const ph_program *prog) { return prog->kernel.compare(0, 17, "fused_v210_trans_") == 0; }
static int fused_trans_job(Args &a, int queue) {
  FusedMultiCall c;
  if (const int rc = fused_multi_parse(a, &c)) return rc;
  ph_fused_layer layers[ph::kMaxLayers];
  for (int i = 0; i < c.n; ++i) {
    ph_fused_layer &L = layers[i] = ph_fused_layer{};
    L.v210 = c.layers[i];
    const double kind = a.num_or(0, "l%dTransition", i);
    if (kind != PH_TRANSITION_CUT && kind != PH_TRANSITION_DISSOLVE && kind != PH_TRANSITION_WIPE)
      return a.fail(PH_E_INVALID, "kernel argument 'l%dTransition': %g (0 cut, 1 dissolve, 2 wipe)", i, kind);
    L.transition = (int)kind;
    L.mix = (float)a.num_or(0, "l%dMix", i);
    if (L.transition != PH_TRANSITION_CUT) L.incoming_v210 = a.buf(v210_bytes(c.width, c.height), "l%dIncomingIn", i)->dptr;
    if (L.transition != PH_TRANSITION_WIPE) continue;
    if (a.has("l%dMaskPacking", i)) {
      const double packing = a.num("l%dMaskPacking", i);
      if (packing != PH_FMT_V210) return a.fail(PH_E_INVALID, "kernel argument 'l%dMaskPacking': %g (0: a v210 frame; absent: an f32 RGBA image)", i, packing);
      L.mask = a.buf(v210_bytes(c.width, c.height), "l%dMaskIn", i)->dptr, L.mask_format = PH_SRC_V210;
    } else {
      L.mask = a.buf(image_bytes(c.width, c.height), "l%dMaskIn", i)->dptr, L.mask_format = PH_SRC_RGBA_F32;
    }
  }
  return a.done() ? a.rc : ph_fused_v210_transition_multi(a.ctx, queue, c.n, layers, c.n_out, c.outs, c.width, c.height, c.r.rd_cm->dptr, c.r.rd_lut->dptr, c.r.rd_gm->dptr);
}
// fused_v210_route_<n> (K_FUSED_V210, told apart by its name; ph_fused_v210_route_multi): fused_v210_combine_multi_<n>'s arguments and
// l<i>Image: 1 marks l<i>In as an f32 RGBA image of width x height x 16 bytes (absent or 0: a v210 frame); imageOut (optional): the
// buffer that receives the combined image; `output` may be absent only when imageOut is there - no packed frame at all.  A launch of
// its own, in its turn (ph_run_programs does not group it).
static bool fused_is_route(const ph_program *prog) { return prog->kernel.compare(0, 17, "fused_v210_route_") == 0; }
static int fused_route_job(Args &a, int queue) {
  FusedMultiCall c;
  if (const int rc = fused_multi_parse(a, &c, true)) return rc;
  ph_route_layer layers[ph::kMaxLayers];
  for (int i = 0; i < c.n; ++i) layers[i] = ph_route_layer{c.layers[i], c.format[i]};
  return a.done() ? a.rc
                  : ph_fused_v210_route_multi(a.ctx, queue, c.n, layers, c.image_out, c.n_out, c.outs, c.width, c.height, c.r.rd_cm->dptr, c.r.rd_lut->dptr, c.r.rd_gm->dptr);
}

// a compose_up_write_v210_<n> job's arguments (ph_run_program and ph_run_programs, which puts like jobs into one launch)
struct UpCall {
  int n;
  bool rgb, pair;
  ph_image_layer layers[ph::kMaxLayers], layers2[ph::kMaxLayers];
  ph_buf *o, *o2;
  Recipe r;  // (the Saver's pair)
  uint32_t width, height, interlace;
  // compose_up_multi_<n>: every output as ph_compose_up_write_multi takes it, job-major (outs[1]: the twin's)
  bool multi;  // the program is compose_up_multi_<n> or compose_up_trans_<n>
  int n_out;
  ph_chan_output outs[2][ph::kMaxUpOuts];
  // compose_up_trans_<n>: the layers as ph_compose_up_transition_multi takes them (tlayers[1]: the twin's; their src: layers / layers2)
  bool trans;  // the program is compose_up_trans_<n>
  ph_image_trans_layer tlayers[2][ph::kMaxLayers];
};
// a partner image of a compose_up_trans_<n> layer: l<i><Role>In, l<i><Role>Matrix, with packedRgb l<i><Role>Width / Height, the twin's l<i><Role>In2
static void up_partner_parse(Args &a, int i, const char *role, bool rgb, bool pair, ph_image_layer *first, ph_image_layer *twin) {
  const ph_buf *x = a.buf(0, "l%d%sIn", i, role);
  double w = 0, h = 0;
  if (rgb) {
    w = a.num("l%d%sWidth", i, role), h = a.num("l%d%sHeight", i, role);
    if (w <= 0 || h <= 0 || x->bytes < (size_t)w * (size_t)h * 12) return (void)a.fail(PH_E_RANGE, "kernel argument 'l%d%sIn': smaller than its %gx%g packed-RGB image", i, role, w, h);
  } else {
    int iw, ih;
    a.named("l%d%sIn", i, role).need_image(x, &iw, &ih);
    w = iw, h = ih;
  }
  first->data = x->dptr, first->format = rgb ? PH_IMG_RGB_F32 : PH_IMG_RGBA_F32, first->width = (int)w, first->height = (int)h;
  first->matrix9_host = a.host_matrix(a.buf(36, "l%d%sMatrix", i, role));
  *twin = *first;
  if (!pair) return;
  const ph_buf *x2 = a.buf(x->bytes, "l%d%sIn2", i, role);
  if (!rgb) {
    int w2, h2;
    a.need_image(x2, &w2, &h2);
    if (!a.rc && (w2 != (int)w || h2 != (int)h)) return (void)a.fail(PH_E_INVALID, "kernel argument '%s': the second job's image is %dx%d, the first's %gx%g", a.name, w2, h2, w, h);
  }
  twin->data = x2->dptr;
}
static int up_call_parse(Args &a, UpCall *u) {
  // l<i>In: the layer's image - an RGBA image buffer, or with packedRgb = 1 a buffer of packed f32 RGB (l<i>Width / l<i>Height:
  // its size); l<i>Matrix: its placement (host mirror, as above); output: v210; outColMatrix / outGammaLut; interlace
  a.frame(&u->width, &u->height);
  u->n = a.prog->n_layers, u->rgb = a.num_or(0, "packedRgb") != 0;
  // output2 + l<i>In2 (optional): a second job of the same shape in the same launch - the other field of a de-interlaced frame
  // (ph_compose_up_write_v210_pair): same sizes, formats and placements, other data
  // compose_up_multi_<n>: the same layers; the outputs as chan_compose_multi_<n> names them (chan_output_parse: output, outPacking,
  // outputU / V / C, outColMatrix, outGammaLut, interlace, then out<k>Packing, output<k>[U|V|C], out<k>ColMatrix, out<k>GammaLut,
  // interlace<k>, k = 1..3).  There `output2` is output 2's frame, so the twin is announced by l0In2 and its planes are the first
  // job's names behind the word twin: twinOutput, twinOutputU / V / C, twinOutput<k>, twinOutput<k>U / V / C.
  // compose_up_trans_<n>: compose_up_multi_<n>'s arguments and, per layer, the keys chan_compose_v210_<n> has for a transition:
  // l<i>Transition (0 cut / 1 dissolve / 2 wipe), l<i>Mix, l<i>Incoming(In|Matrix|Width|Height), l<i>Mask(...); the twin's
  // l<i>IncomingIn2, l<i>MaskIn2 and l<i>Mix2 (default l<i>Mix)
  u->trans = a.prog->kernel.compare(0, 17, "compose_up_trans_") == 0;
  u->multi = u->trans || a.prog->kernel.compare(0, 17, "compose_up_multi_") == 0;
  u->n_out = 0;
  u->pair = u->multi ? a.has("l0In2") : a.has("output2");
  for (int i = 0; i < u->n; ++i) {
    const ph_buf *x = a.buf(0, "l%dIn", i), *x2 = nullptr;
    double lw = 0, lh = 0;
    if (u->pair) {
      x2 = a.buf(x->bytes, "l%dIn2", i);
      if (!u->rgb) {
        int w2, h2, w1, h1;
        a.need_image(x2, &w2, &h2);
        a.need_image(x, &w1, &h1);
        if (w1 != w2 || h1 != h2) return a.fail(PH_E_INVALID, "kernel argument '%s': the second job's image is %dx%d, the first's %dx%d", a.name, w2, h2, w1, h1);
      }
    }
    if (u->rgb) {
      lw = a.num("l%dWidth", i), lh = a.num("l%dHeight", i);
      if (lw <= 0 || lh <= 0 || x->bytes < (size_t)lw * (size_t)lh * 12) return a.fail(PH_E_RANGE, "kernel argument 'l%dIn': smaller than its %gx%g packed-RGB image", i, lw, lh);
    } else {
      int iw, ih;
      a.named("l%dIn", i).need_image(x, &iw, &ih);
      lw = iw, lh = ih;
    }
    const float *placement = a.host_matrix(a.buf(36, "l%dMatrix", i));
    u->layers[i].data = x->dptr, u->layers[i].format = u->rgb ? PH_IMG_RGB_F32 : PH_IMG_RGBA_F32;
    u->layers[i].width = (int)lw, u->layers[i].height = (int)lh, u->layers[i].matrix9_host = placement;
    u->layers2[i] = u->layers[i];
    if (u->pair) u->layers2[i].data = x2->dptr;
    if (!u->trans) continue;
    ph_image_trans_layer &t = u->tlayers[0][i], &t2 = u->tlayers[1][i];
    t = t2 = ph_image_trans_layer{};
    t.src = u->layers[i], t2.src = u->layers2[i];
    const double kind = a.num_or(0, "l%dTransition", i);
    if (kind != PH_TRANSITION_CUT && kind != PH_TRANSITION_DISSOLVE && kind != PH_TRANSITION_WIPE)
      return a.fail(PH_E_INVALID, "kernel argument 'l%dTransition': %g (0 cut, 1 dissolve, 2 wipe)", i, kind);
    t.transition = t2.transition = (int)kind;
    t.mix = (float)a.num_or(0, "l%dMix", i), t2.mix = (float)a.num_or(t.mix, "l%dMix2", i);
    if (t.transition != PH_TRANSITION_CUT) up_partner_parse(a, i, "Incoming", u->rgb, u->pair, &t.incoming, &t2.incoming);
    if (t.transition == PH_TRANSITION_WIPE) up_partner_parse(a, i, "Mask", u->rgb, u->pair, &t.mask, &t2.mask);
  }
  if (u->multi) {
    u->o = u->o2 = nullptr, u->r = Recipe(), u->interlace = 0;
    for (int k = 0; k < ph::kMaxUpOuts && !a.rc && (k == 0 || a.has("output%d", k)); ++k) {
      ph_buf *wr_cm, *wr_lut;
      ph_chan_output &o = u->outs[0][u->n_out++];
      if (chan_output_parse(a, k, u->width, u->height, &o, &wr_cm, &wr_lut)) break;
      for (int j = 0; j < k; ++j)
        if (u->outs[0][j].planes[0] == o.planes[0]) return a.fail(PH_E_INVALID, "kernel argument 'output%d': the buffer is another output's too", k);
      if (!u->pair) continue;
      char prefix[24];
      if (k) snprintf(prefix, sizeof prefix, "twinOutput%d", k);
      else snprintf(prefix, sizeof prefix, "twinOutput");
      ph_chan_output &t = u->outs[1][k];
      t = o, t.planes[0] = t.planes[1] = t.planes[2] = nullptr;
      a.planes(o.format, u->width, u->height, prefix, "", t.planes);
      for (int j = 0; j <= k && !a.rc; ++j)
        if (u->outs[0][j].planes[0] == t.planes[0] || (j < k && u->outs[1][j].planes[0] == t.planes[0]))
          return a.fail(PH_E_INVALID, "kernel argument '%s': the buffer is another output's too", prefix);
    }
    // the outputs are numbered without a gap: an output<k> behind a missing one would be ignored without a word (`output2` alone is
    // what compose_up_write_v210_<n> calls its twin: here the twin is l0In2 / twinOutput)
    for (int k = u->n_out + 1; k < ph::kMaxUpOuts && !a.rc; ++k)
      if (a.has("output%d", k)) return a.fail(PH_E_INVALID, "kernel argument 'output%d': there is no output%d (outputs are numbered without a gap; the twin's frame is twinOutput)", k, u->n_out);
    return a.rc;
  }
  u->o = a.buf(v210_bytes(u->width, u->height), "output");
  u->o2 = u->pair ? a.buf(v210_bytes(u->width, u->height), "output2") : nullptr;
  u->r = Recipe();
  a.saver(&u->r);
  u->interlace = (uint32_t)a.num_or(0, "interlace");
  return a.rc;
}

// a compose_up_multi_<n> / compose_up_trans_<n> job as the typed call
static int up_call_multi(ph_ctx *ctx, int queue, const UpCall &u) {
  const ph_image_layer *sets[2] = {u.layers, u.layers2};
  ph_chan_output outs[2 * ph::kMaxUpOuts];
  const int jobs = u.pair ? 2 : 1;
  for (int j = 0; j < jobs; ++j)
    for (int k = 0; k < u.n_out; ++k) outs[j * u.n_out + k] = u.outs[j][k];
  if (u.trans) {
    const ph_image_trans_layer *tsets[2] = {u.tlayers[0], u.tlayers[1]};
    return ph_compose_up_transition_multi(ctx, queue, jobs, u.n, tsets, u.n_out, outs, u.width, u.height);
  }
  return ph_compose_up_write_multi(ctx, queue, jobs, u.n, sets, u.n_out, outs, u.width, u.height);
}

// pack_write_multi_<n> (K_PACK_WRITE, told apart by its name): input: the f32 RGBA image; width (globalWorkItems [width, height]); the n outputs as
// chan_compose_multi_<n> names them (chan_output_parse: outPacking - any pack format here - output, outputU / V / C, outColMatrix, outGammaLut,
// interlace, then out<k>Packing, output<k>[U|V|C], out<k>ColMatrix, out<k>GammaLut, interlace<k>, k = 1..n-1)
static int pack_write_multi_job(Args &a, int queue) {
  ph_ctx *ctx = a.ctx;
  const ph_program *prog = a.prog;
  uint32_t gw, height;
  a.frame(&gw, &height);
  const uint32_t width = (uint32_t)a.num("width");
  if (!a.rc && width != gw) return a.fail(PH_E_INVALID, "%s: globalWorkItems must be [width, height] (width %u, globalWorkItems[0] %u)", prog->kernel.c_str(), width, gw);
  const ph_buf *image = a.buf(image_bytes(width, height), "input");
  ph_chan_output outs[ph::kMaxPackOuts];
  for (int k = 0; k < prog->n_layers && !a.rc; ++k) {
    ph_buf *wr_cm, *wr_lut;
    if (chan_output_parse(a, k, width, height, &outs[k], &wr_cm, &wr_lut, nullptr, true)) break;
    for (int j = 0; j < k; ++j)
      if (outs[j].planes[0] == outs[k].planes[0]) return a.fail(PH_E_INVALID, "kernel argument 'output%d': the buffer is another output's too", k);
  }
  return a.done() ? a.rc : ph_pack_write_multi(ctx, queue, image->dptr, prog->n_layers, outs, width, height);
}

// ph_run_program's argument marshalling, one function per kernel family: each checks the job's named arguments against the frame geometry
// (everything ph_check_program reports) and, unless check_only, makes the typed call.
// the wire formats: v210 / pack readers and writers (v210.ts, yuv422p10.ts ... bgra8.ts; Reader / Writer geometry packer.ts:30-83)
static int dispatch_wire(Args &a, int queue) {
  ph_ctx *ctx = a.ctx;
  const ph_program *prog = a.prog;
  Recipe r;
  switch (prog->id) {
    case K_PACK_READ:
    case K_PACK_WRITE: {
      if (prog->id == K_PACK_WRITE && prog->kernel.compare(0, 17, "pack_write_multi_") == 0) return pack_write_multi_job(a, queue);
      const bool rd = prog->id == K_PACK_READ;
      const int fmt = prog->format;
      const uint32_t width = (uint32_t)a.num("width"), interlace = rd ? 0 : (uint32_t)a.num("interlace");
      if (!prog->local || !width) return a.fail(PH_E_INVALID, "%s: width / workItemsPerGroup not set", prog->kernel.c_str());
      // Readers: global = wipg*height (4:2:0: /2).  Writers: /2 when interlaced, 4:2:0 always /2
      uint32_t height = prog->global[0] / prog->local;
      if (fmt_v420(fmt)) height *= 2;
      else if (!rd && interlace) height *= 2;
      void *planes[3] = {nullptr, nullptr, nullptr};
      a.planes(fmt, width, height, rd ? "input" : "output", "Y", planes);
      const ph_buf *image = a.buf(image_bytes(width, height), rd ? "output" : "input");
      a.loader(&r, !fmt_rgb8(fmt), rd);
      if (a.done()) return a.rc;
      if (rd) return ph_pack_read(ctx, queue, fmt, planes, image->dptr, width, height, dptr(r.rd_cm), r.rd_lut->dptr, r.rd_gm->dptr);
      return ph_pack_write(ctx, queue, fmt, image->dptr, planes, width, height, interlace, dptr(r.rd_cm), r.rd_lut->dptr);
    }
    case K_V210_READ: {
      const uint32_t width = (uint32_t)a.num("width");
      if (!prog->local || !width) return a.fail(PH_E_INVALID, "v210 read: width / workItemsPerGroup not set");
      const uint32_t height = prog->global[0] / prog->local;  // Reader: global = wipg * height (v210.ts:293-294)
      const ph_buf *in = a.buf(v210_bytes(width, height), "input"), *out = a.buf(image_bytes(width, height), "output");
      a.loader(&r);
      return a.done() ? a.rc : ph_v210_read(ctx, queue, in->dptr, out->dptr, width, height, r.rd_cm->dptr, r.rd_lut->dptr, r.rd_gm->dptr);
    }
    case K_V210_WRITE: {
      const uint32_t width = (uint32_t)a.num("width"), interlace = (uint32_t)a.num("interlace");
      if (!prog->local || !width) return a.fail(PH_E_INVALID, "v210 write: width / workItemsPerGroup not set");
      // Writer: global = wipg * height / (interlaced ? 2 : 1) (v210.ts:322-323)
      const uint32_t height = prog->global[0] / prog->local * (interlace ? 2 : 1);
      const ph_buf *in = a.buf(image_bytes(width, height), "input"), *out = a.buf(v210_bytes(width, height), "output");
      a.loader(&r, true, false);
      return a.done() ? a.rc : ph_v210_write(ctx, queue, in->dptr, out->dptr, width, height, interlace, r.rd_cm->dptr, r.rd_lut->dptr);
    }
    case K_V210_READ_BATCH: {  // l<i>In: v210 frames; l<i>Out: RGBA images; colMatrix / gammaLut / gamutMatrix: the Loader's
      uint32_t width, height;
      a.frame(&width, &height);
      const void *ins[ph::kMaxLayers];
      void *outs[ph::kMaxLayers];
      for (int i = 0; i < prog->n_layers; ++i) {
        ins[i] = a.buf(v210_bytes(width, height), "l%dIn", i)->dptr;
        outs[i] = a.buf(image_bytes(width, height), "l%dOut", i)->dptr;
      }
      a.loader(&r);
      return a.done() ? a.rc : ph_v210_read_batch(ctx, queue, prog->n_layers, ins, outs, width, height, r.rd_cm->dptr, r.rd_lut->dptr, r.rd_gm->dptr);
    }
    default: break;
  }
  return fail(PH_E_UNKNOWN_KERNEL, "unhandled kernel id");
}
// de-interlacing: yadif, both parities in one launch, and the reader fused with it (yadifCl.ts, yadif.ts:88-145)
static int dispatch_deint(Args &a, int queue) {
  ph_ctx *ctx = a.ctx;
  const ph_program *prog = a.prog;
  int w, h;
  switch (prog->id) {
    case K_YADIF: {
      const ph_buf *out = a.image(&w, &h, "output");
      const size_t img = image_bytes(w, h);
      const ph_buf *prev = a.buf(img, "prev"), *cur = a.buf(img, "cur"), *next = a.buf(img, "next");
      const int parity = (int)a.num("parity"), tff = (int)a.num("tff"), skip = (int)a.num("skipSpatial");
      return a.done() ? a.rc : ph_yadif(ctx, queue, prev->dptr, cur->dptr, next->dptr, w, h, parity, tff, skip, out->dptr);
    }
    case K_YADIF_PAIR: {  // output0 / output1: what 'yadif' writes with parity 0 / 1
      const ph_buf *out0 = a.image(&w, &h, "output0");
      const size_t img = image_bytes(w, h);
      const ph_buf *out1 = a.buf(img, "output1"), *prev = a.buf(img, "prev"), *cur = a.buf(img, "cur"), *next = a.buf(img, "next");
      const int tff = (int)a.num("tff"), skip = (int)a.num("skipSpatial");
      return a.done() ? a.rc : ph_yadif_pair(ctx, queue, prev->dptr, cur->dptr, next->dptr, w, h, tff, skip, out0->dptr, out1->dptr);
    }
    case K_V210_YADIF_PAIR: {
      // l<i>Prev / l<i>Cur / l<i>Next: v210 window; l<i>Out0 / l<i>Out1: RGBA; colMatrix / gammaLut / gamutMatrix: the Loader's
      uint32_t width, height;
      a.frame(&width, &height);
      // packedRgb (optional): 1 = the outputs are packed f32 RGB (12 bytes per pixel) for compose_up_write_v210_<n>
      const bool rgb = a.num_or(0, "packedRgb") != 0;
      // packing (optional): 1 yuv422p10 / 2 yuv422p8 / 3 yuv420p / 4 nv12 - the windows are planar frames: l<i>Prev / Cur / Next their Y planes,
      // l<i>PrevU, l<i>PrevV, l<i>CurU ... their chroma planes
      const double packing = a.num_or(0, "packing");
      const int pfmt = (int)packing;
      if (!fmt_deint(pfmt)) return a.fail(PH_E_INVALID, "kernel argument 'packing': %g (0 v210, 1 yuv422p10, 2 yuv422p8, 3 yuv420p, 4 nv12)", packing);
      size_t pb[3];
      a.plane_bytes(pfmt, width, height, pb);
      const size_t img = (size_t)width * height * (rgb ? 12 : 16);
      ph_deint_source src[ph::kMaxLayers];
      memset(src, 0, sizeof src);
      for (int i = 0; i < prog->n_layers; ++i) {
        static const char *const which[3] = {"Prev", "Cur", "Next"};
        const void **slots[3][3] = {{&src[i].prev, &src[i].prev_u, &src[i].prev_v}, {&src[i].cur, &src[i].cur_u, &src[i].cur_v}, {&src[i].next, &src[i].next_u, &src[i].next_v}};
        for (int f = 0; f < 3; ++f)
          for (int c = 1; c < fmt_planes(pfmt); ++c)  // (nv12: l<i>PrevU ... are the interleaved CbCr planes)
            *slots[f][c] = a.buf(pb[c], "l%d%s%c", i, which[f], c == 1 ? 'U' : 'V')->dptr;
        for (int f = 0; f < 3; ++f) *slots[f][0] = a.buf(pb[0], "l%d%s", i, which[f])->dptr;
        src[i].out_parity0 = a.buf(img, "l%dOut0", i)->dptr;
        src[i].out_parity1 = a.buf(img, "l%dOut1", i)->dptr;
      }
      Recipe r;
      a.loader(&r);
      const int tff = (int)a.num("tff"), skip = (int)a.num("skipSpatial");
      return a.done() ? a.rc : ph_yadif_pair_packed(ctx, queue, prog->n_layers, src, pfmt, width, height, tff, skip, rgb ? PH_IMG_RGB_F32 : PH_IMG_RGBA_F32,
                                                    r.rd_cm->dptr, r.rd_lut->dptr, r.rd_gm->dptr);
    }
    default: break;
  }
  return fail(PH_E_UNKNOWN_KERNEL, "unhandled kernel id");
}
// the compositors: a channel's frame, enlarged layers, the buffer-addressed compositor, the headline kernel, combine_N (combine.ts, mixer.ts:189-228)
static int dispatch_compose(Args &a, int queue) {
  ph_ctx *ctx = a.ctx;
  const ph_program *prog = a.prog;
  switch (prog->id) {
    case K_CHAN_COMPOSE: {
      ChanCall call;
      chan_call_parse(a, &call);
      if (call.clip_route && !a.rc && a.check_only)  // (a check answers as the launch does: the typed call's own refusals)
        return clip_compose_route_check(queue, call.n_layers, call.layers, call.image_out, call.n_out, call.outs, call.width, call.height, call.r.rd_cm->dptr,
                                        call.r.rd_lut->dptr, call.r.rd_gm->dptr);
      if (a.done()) return a.rc;
      if (call.clip)  // clip_compose_multi_<n>: chan_compose_multi_<n>'s arguments, name for name
        return ph_clip_compose_multi(ctx, queue, call.n_layers, call.layers, call.n_out, call.outs, call.width, call.height, call.r.rd_cm->dptr, call.r.rd_lut->dptr,
                                     call.r.rd_gm->dptr);
      if (call.clip_trans)  // clip_compose_trans_<n>: the same arguments, the transition's included
        return ph_clip_compose_transition_multi(ctx, queue, call.n_layers, call.layers, call.n_out, call.outs, call.width, call.height, call.r.rd_cm->dptr,
                                                call.r.rd_lut->dptr, call.r.rd_gm->dptr);
      if (call.clip_route)  // clip_compose_route_<n>: the same arguments and the optional imageOut
        return ph_clip_compose_route_multi(ctx, queue, call.n_layers, call.layers, call.image_out, call.n_out, call.outs, call.width, call.height,
                                           call.r.rd_cm->dptr, call.r.rd_lut->dptr, call.r.rd_gm->dptr);
      if (call.multi)  // chan_compose_multi_<n>: chan_compose_v210_<n>'s arguments (output 0) and up to three more outputs (chan_output_parse)
        return ph_chan_compose_multi(ctx, queue, call.n_layers, call.layers, call.n_out, call.outs, call.width, call.height, call.r.rd_cm->dptr, call.r.rd_lut->dptr,
                                     call.r.rd_gm->dptr);
      return ph_chan_compose(ctx, queue, call.n_layers, call.layers, call.out_format, call.out_planes, call.width, call.height, call.interlace,
                             call.r.rd_cm->dptr, call.r.rd_lut->dptr, call.r.rd_gm->dptr, dptr(call.r.wr_cm), call.r.wr_lut->dptr);
    }
    case K_COMPOSE_UP: {
      UpCall u;
      up_call_parse(a, &u);
      if (a.done()) return a.rc;
      if (u.multi) return up_call_multi(ctx, queue, u);
      if (u.pair)
        return ph_compose_up_write_v210_pair(ctx, queue, u.n, u.layers, u.layers2, u.o->dptr, u.o2->dptr, u.width, u.height, u.interlace, u.r.wr_cm->dptr, u.r.wr_lut->dptr);
      return ph_compose_up_write_v210(ctx, queue, u.n, u.layers, u.o->dptr, u.width, u.height, u.interlace, u.r.wr_cm->dptr, u.r.wr_lut->dptr);
    }
    case K_COMPOSE_V210: {
      // l<i>In: RGBA image; l<i>Matrix (optional): its 3x3 placement, absent = taken 1:1; l<i>WipeIn + l<i>WipeMask (optional):
      // a wipe transition on the placed layer; output: v210; outColMatrix / outGammaLut: the Saver's; interlace as 'write'
      uint32_t width, height;
      a.frame(&width, &height);
      ph_layer layers[ph::kMaxLayers];
      ph_layer_wipe wipes[ph::kMaxLayers];
      bool any_wipe = false;
      for (int i = 0; i < prog->n_layers; ++i) {
        layers[i].rgba = a.image(&layers[i].width, &layers[i].height, "l%dIn", i)->dptr;
        layers[i].matrix9 = dptr(a.buf_or_null(36, "l%dMatrix", i));
        wipes[i].incoming_rgba = wipes[i].mask_rgba = nullptr;
        if (const ph_buf *incoming = a.buf_or_null(image_bytes(width, height), "l%dWipeIn", i)) {
          wipes[i].incoming_rgba = incoming->dptr;
          wipes[i].mask_rgba = a.buf(image_bytes(width, height), "l%dWipeMask", i)->dptr;
          any_wipe = true;
        }
      }
      const ph_buf *out = a.buf(v210_bytes(width, height), "output");
      Recipe r;
      a.saver(&r);
      const uint32_t interlace = (uint32_t)a.num_or(0, "interlace");
      if (a.done()) return a.rc;
      if (any_wipe) return ph_compose_wipe_write_v210(ctx, queue, prog->n_layers, layers, wipes, out->dptr, width, height, interlace, r.wr_cm->dptr, r.wr_lut->dptr);
      return ph_compose_write_v210(ctx, queue, prog->n_layers, layers, out->dptr, width, height, interlace, r.wr_cm->dptr, r.wr_lut->dptr);
    }
    case K_COMBINE: {
      const void *layers[ph::kMaxLayers];
      int w, h;
      const ph_buf *out = a.image(&w, &h, "output");
      for (int i = 0; i < prog->n_layers; ++i) layers[i] = a.buf(image_bytes(w, h), "l%dIn", i)->dptr;
      return a.done() ? a.rc : ph_combine(ctx, queue, prog->n_layers, layers, w, h, out->dptr);
    }
    case K_FUSED_V210: {
      if (fused_is_trans(prog)) return fused_trans_job(a, queue);
      if (fused_is_route(prog)) return fused_route_job(a, queue);
      if (fused_is_multi(prog)) return fused_multi_job(a, queue);
      FusedCall f;
      fused_call_parse(a, &f);
      return a.done() ? a.rc : ph_fused_v210_combine(ctx, queue, f.n, f.layers, f.out, f.width, f.height, f.r.rd_cm->dptr, f.r.rd_lut->dptr, f.r.rd_gm->dptr,
                                                     f.r.wr_cm->dptr, f.r.wr_lut->dptr);
    }
    default: break;
  }
  return fail(PH_E_UNKNOWN_KERNEL, "unhandled kernel id");
}
// the f32 image operators: transform, resize, dissolve / mixer / wipe, transition_wipe (transform.ts, resize.ts, transition.ts, mix.ts, wipe.ts)
static int dispatch_image(Args &a, int queue) {
  ph_ctx *ctx = a.ctx;
  const ph_program *prog = a.prog;
  int w, h, iw, ih;
  switch (prog->id) {
    case K_TRANSFORM: {
      const ph_buf *in = a.image(&iw, &ih, "input"), *out = a.image(&w, &h, "output"), *matrix = a.buf(32, "transformMatrix");
      return a.done() ? a.rc : ph_transform(ctx, queue, in->dptr, iw, ih, matrix->dptr, out->dptr, w, h);
    }
    case K_RESIZE: {
      const ph_buf *in = a.image(&iw, &ih, "input"), *out = a.image(&w, &h, "output"), *flip = a.buf(16, "flip");
      const float scale = (float)a.num("scale"), ox = (float)a.num("offsetX"), oy = (float)a.num("offsetY");
      return a.done() ? a.rc : ph_resize(ctx, queue, in->dptr, iw, ih, scale, ox, oy, flip->dptr, out->dptr, w, h);
    }
    case K_DISSOLVE:
    case K_MIXER:
    case K_WIPE: {
      const ph_buf *out = a.image(&w, &h, "output"), *in0 = a.buf(image_bytes(w, h), "input0"), *in1 = a.buf(image_bytes(w, h), "input1");
      const float mix = (float)a.num(prog->id == K_WIPE ? "wipe" : "mix");
      if (a.done()) return a.rc;
      if (prog->id == K_WIPE) return ph_wipe(ctx, queue, in0->dptr, in1->dptr, mix, w, h, out->dptr);
      if (prog->id == K_MIXER) return ph_mixer(ctx, queue, in0->dptr, in1->dptr, mix, w, h, out->dptr);
      return ph_transition_dissolve(ctx, queue, in0->dptr, in1->dptr, mix, w, h, out->dptr);
    }
    case K_RGB_UNPACK: {  // image: an f32 RGBA image buffer whose first width * height * 12 bytes hold packed f32 RGB - expanded in place
      const ph_buf *image = a.image(&w, &h, "image");
      return a.done() ? a.rc : ph_image_unpack_rgb(ctx, queue, image->dptr, w, h);
    }
    case K_TWIPE: {
      const ph_buf *out = a.image(&w, &h, "output"), *in0 = a.buf(image_bytes(w, h), "input0"), *in1 = a.buf(image_bytes(w, h), "input1");
      const ph_buf *mask = a.buf(image_bytes(w, h), "maskIn");
      return a.done() ? a.rc : ph_transition_wipe(ctx, queue, in0->dptr, in1->dptr, mask->dptr, w, h, out->dptr);
    }
    default: break;
  }
  return fail(PH_E_UNKNOWN_KERNEL, "unhandled kernel id");
}
// (injection_asked: the caller has put this launch to the "fail_launches" fault injection itself)
static int dispatch(ph_ctx *ctx, ph_program *prog, const ph_arg *args, int n, int queue, bool check_only = false, bool injection_asked = false) {
  if (!check_only && !injection_asked && inject_failure(ctx)) return fail(PH_E_HIP, "%s: launch failed: injected (context option fail_launches)", prog->kernel.c_str());
  Args a{ctx, prog, args, n, check_only};
  switch (prog->id) {
    case K_PACK_READ:
    case K_PACK_WRITE:
    case K_V210_READ:
    case K_V210_WRITE:
    case K_V210_READ_BATCH:
      return dispatch_wire(a, queue);
    case K_YADIF:
    case K_YADIF_PAIR:
    case K_V210_YADIF_PAIR:
      return dispatch_deint(a, queue);
    case K_CHAN_COMPOSE:
    case K_COMPOSE_UP:
    case K_COMPOSE_V210:
    case K_COMBINE:
    case K_FUSED_V210:
      return dispatch_compose(a, queue);
    case K_TRANSFORM:
    case K_RESIZE:
    case K_DISSOLVE:
    case K_MIXER:
    case K_WIPE:
    case K_TWIPE:
    case K_RGB_UNPACK:
      return dispatch_image(a, queue);
  }
  return fail(PH_E_UNKNOWN_KERNEL, "unhandled kernel id");
}

int ph_run_program(ph_ctx *ctx, ph_program *prog, const ph_arg *args, int n_args, int queue, ph_run_timings *t) {
  if (!ctx || !prog || (n_args > 0 && !args)) return fail(PH_E_INVALID, "ph_run_program: NULL argument");
  PH_QUEUE("ph_run_program", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  rc = flush_dirty_args(ctx, args, n_args, queue);
  if (rc) return rc;
  if (!t) return dispatch(ctx, prog, args, n_args, queue);
  hipStream_t s = stream_of(ctx, queue);
  const auto t0 = std::chrono::steady_clock::now();
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // per call: timed runs may come from several threads
  PH_HIP(hipEventCreate(&ev0));
  if (hipEventCreate(&ev1) != hipSuccess) {
    hipEventDestroy(ev0);
    return fail(PH_E_HIP, "ph_run_program: hipEventCreate failed");
  }
  hipError_t te = hipEventRecord(ev0, s);
  rc = te == hipSuccess ? dispatch(ctx, prog, args, n_args, queue) : fail(PH_E_HIP, "hipEventRecord: %s", hipGetErrorString(te));
  float ms = 0.f;
  if (rc == PH_OK) {
    te = hipEventRecord(ev1, s);
    if (te == hipSuccess) te = hipEventSynchronize(ev1);
    if (te == hipSuccess) te = hipEventElapsedTime(&ms, ev0, ev1);
    if (te != hipSuccess) rc = fail(PH_E_HIP, "ph_run_program: timing failed: %s", hipGetErrorString(te));
  }
  hipEventDestroy(ev0);
  hipEventDestroy(ev1);
  if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  t->data_to_kernel = 0;  // arguments are device-resident: nothing moves at launch
  t->kernel_exec = (uint32_t)(ms * 1000.0f + 0.5f);
  t->total_time = (uint32_t)std::chrono::duration_cast<std::chrono::microseconds>(t1 - t0).count();
  return PH_OK;
}

int ph_check_program(ph_ctx *ctx, ph_program *prog, const ph_arg *args, int n_args, int queue) {
  if (!ctx || !prog || (n_args > 0 && !args)) return fail(PH_E_INVALID, "ph_check_program: NULL argument");
  PH_QUEUE("ph_check_program", queue);
  return dispatch(ctx, prog, args, n_args, queue, true);
}

/* Several recorded jobs handed over in one call (a binding that records jobs and launches them later: node/defer.js).  Exactly the
 * ph_run_program calls in the order given - with the channel frames among them (chan_compose_v210_<n> programs of one geometry that name
 * the SAME Loader / Saver buffers and make v210 frames) put into launches together (ph_chan_compose_batch), likewise consecutive
 * fused_v210_combine_<n> frames; a job that reads or writes what an earlier job of its group writes (or writes what one reads) is
 * detected here and starts the next launch, so call order holds (include/phaneron_hip.h).  A chan_compose_multi_<n> job runs in its turn
 * as a launch of its own - it ends the group in front of it, so whatever that group writes is there for it, and all its outputs for what follows.
 * So does a pack_write_multi_<n> job (ph_pack_write_multi), and a fused_v210_combine_multi_<n> job (ph_fused_v210_combine_multi) - unless
 * the context option "fused_multi_batch" = 1 (default 0) lets consecutive such jobs of one shape and output list share launches
 * (ph_fused_v210_combine_multi_batch), under the same call-order rule.
 * With the context option "chan_batch_outs" = 1 (default 0) consecutive chan_compose_multi_<n> jobs and chan_compose_v210_<n> jobs that
 * make another format than v210 (outPacking) share launches as well (ph_chan_compose_batch_out).  A clip_compose_multi_<n> job
 * (ph_clip_compose_multi) is a launch of its own in its turn too - unless the context option "clip_batch" = 1 (default 0) lets consecutive
 * such jobs of one geometry and Loader recipe go down in one ph_clip_compose_batch_out call, under the same call-order rule.  A call that fails after its checks
 * (a launch refused) has made the launches of the jobs before the failing group: ph_run_programs_progress says how many. */
namespace {
thread_local int g_programs_done = 0;  // jobs of the calling thread's last ph_run_programs call whose launches were made
}
// What a job of each grouped kind reads and writes (ph_spans.h), by byte range.
// fused_v210_combine_<n>: every layer and the frame are frame_bytes long
static void fused_footprint(const FusedCall &f, Footprint &fp) {
  for (int l = 0; l < f.n; ++l) span_read(fp, f.layers[l], f.frame_bytes);
  span_write(fp, f.out, f.frame_bytes);
}
// fused_v210_combine_multi_<n>: a layer is any v210_bytes, a plane what its format gives it at the height rounded up to even
static void fused_multi_footprint(const FusedMultiCall &m, Footprint &fp) {
  const size_t frame_bytes = v210_bytes(m.width, m.height);
  for (int l = 0; l < m.n; ++l) span_read(fp, m.layers[l], frame_bytes);
  // (a format without plane sizes is one the typed call refuses: the job goes down alone and is answered there)
  for (int o = 0; o < m.n_out; ++o) span_write_output(fp, m.outs[o], m.width, m.height + (m.height & 1u), frame_bytes);
}
// compose_up_write_v210_<n>: a layer image - either field's - is any buffer of w * h * 16 bytes (packedRgb: 12), a frame any buffer of
// v210_bytes; a pair writes two
static void up_footprint(const UpCall &u, Footprint &fp) {
  const size_t frame_bytes = v210_bytes(u.width, u.height);
  for (int l = 0; l < u.n; ++l) {
    const size_t bytes = (size_t)u.layers[l].width * (size_t)u.layers[l].height * (u.rgb ? 12u : 16u);
    span_read(fp, u.layers[l].data, bytes);
    if (u.pair) span_read(fp, u.layers2[l].data, bytes);
  }
  span_write(fp, u.o->dptr, frame_bytes);
  if (u.pair) span_write(fp, u.o2->dptr, frame_bytes);
}
// chan_compose_v210_<n>: the sources by their formats, a plane of no bytes widened to one; the frame pitch * height
static void chan_footprint(const ChanCall &c, Footprint &fp) {
  for (int l = 0; l < c.n_layers; ++l)
    for (const ph_chan_source *s : {&c.layers[l].src, &c.layers[l].incoming, &c.layers[l].mask}) span_read_source(fp, *s, 1);
  span_write(fp, c.out_planes[0], (size_t)ph_v210_pitch_bytes(c.width) * c.height);
}
int ph_run_programs_progress(int *jobs_done) {
  if (!jobs_done) return fail(PH_E_INVALID, "ph_run_programs_progress: NULL argument");
  *jobs_done = g_programs_done;
  return PH_OK;
}
int ph_run_programs(ph_ctx *ctx, int n_jobs, ph_program *const *progs, const ph_arg *const *args, const int *n_args, int queue) {
  g_programs_done = 0;  // first of all: a call refused by ANY check has made nothing, and must not leave the call before it standing
  if (!ctx || n_jobs < 1 || !progs || !args || !n_args) return fail(PH_E_INVALID, "ph_run_programs: NULL argument");
  PH_QUEUE("ph_run_programs", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  if (ctx->fail_launches.load() > 0) return fail(PH_E_HIP, "ph_run_programs: launch failed: injected (context option fail_launches)");
  std::vector<ChanCall> calls((size_t)n_jobs);
  std::vector<FusedCall> fused((size_t)n_jobs);
  std::vector<UpCall> ups;  // (sized when the first compose_up job shows up: most calls have none)
  std::vector<FusedMultiCall> multis;  // (likewise)
  // 1: a v210 frame from the channel kernel, 2: fused_v210_combine, 3: compose_up_write_v210, 4: a channel's frame for other consumers
  // (option "chan_batch_outs"), 5: fused_v210_combine_multi (option "fused_multi_batch"), 6: clip_compose_multi (option "clip_batch"),
  // 0: whatever else, launched as it is
  std::vector<char> kind((size_t)n_jobs, 0);
  // the footprints of the group being collected, the candidate's last: does it keep clear of every job already in the group?
  // (the calling thread's, kept from call to call: a call allocates none)
  static thread_local std::vector<Footprint> kept;
  std::vector<Footprint> &prints = kept;
  auto joins = [&](unsigned hazards) {
    for (size_t e = 0; e + 1 < prints.size(); ++e)
      if (clashes(prints.back(), prints[e], hazards, false)) return false;
    return true;
  };
  for (int j = 0; j < n_jobs; ++j) {  // every job is checked before anything is launched: a bad one refuses the call as a whole
    if (!progs[j] || (n_args[j] > 0 && !args[j])) return fail(PH_E_INVALID, "ph_run_programs: job %d: NULL argument", j);
    if ((rc = flush_dirty_args(ctx, args[j], n_args[j], queue))) return rc;
    Args job{ctx, progs[j], args[j], n_args[j], false};
    if (progs[j]->id == K_CHAN_COMPOSE) {
      if ((rc = chan_call_parse(job, &calls[(size_t)j]))) return rc;
      if (const ChanCall &c = calls[(size_t)j]; c.clip_route && (rc = clip_compose_route_check(queue, c.n_layers, c.layers, c.image_out, c.n_out, c.outs, c.width, c.height,
                                                                                            c.r.rd_cm->dptr, c.r.rd_lut->dptr, c.r.rd_gm->dptr)))
        return rc;
      // (a frame for another consumer, or a chan_compose_multi_<n> job: a launch of its own, in its turn - unless the context option
      // "chan_batch_outs" lets such jobs share launches too: ph_chan_compose_batch_out)
      // (a clip_compose_multi_<n> job: a launch of its own, in its turn - unless the context option "clip_batch" lets such jobs share
      // launches: ph_clip_compose_batch_out)
      // (a clip_compose_trans_<n> job: a launch of its own, in its turn - never grouped.  So is a clip_compose_route_<n> job: no group
      // reaches across it, so the image it writes - which the entry itself holds against the job's own sources and planes by byte range,
      // ph_spans.h - is written before any later job of the call reads it, and after every earlier job has read or written its bytes)
      kind[(size_t)j] = calls[(size_t)j].clip_trans || calls[(size_t)j].clip_route ? 0 : calls[(size_t)j].clip ? (ctx->clip_batch ? 6 : 0) : calls[(size_t)j].out_format == PH_FMT_V210 && !calls[(size_t)j].multi ? 1 : ctx->chan_batch_outs ? 4 : 0;
    } else if (progs[j]->id == K_FUSED_V210 && !fused_is_multi(progs[j]) && !fused_is_trans(progs[j]) && !fused_is_route(progs[j])) {
      if ((rc = fused_call_parse(job, &fused[(size_t)j]))) return rc;
      kind[(size_t)j] = 2;
    } else if (progs[j]->id == K_FUSED_V210 && ctx->fused_multi_batch && !fused_is_trans(progs[j]) && !fused_is_route(progs[j])) {  // (a fused_v210_trans_<n> or fused_v210_route_<n> job: a launch of its own, in its turn)
      // (a fused_v210_combine_multi_<n> job: a launch of its own, in its turn - unless the context option "fused_multi_batch" lets such
      // jobs share launches: ph_fused_v210_combine_multi_batch)
      if (multis.empty()) multis.resize((size_t)n_jobs);
      if ((rc = fused_multi_parse(job, &multis[(size_t)j]))) return rc;
      kind[(size_t)j] = 5;
    } else if (progs[j]->id == K_COMPOSE_UP) {
      if (ups.empty()) ups.resize((size_t)n_jobs);
      if ((rc = up_call_parse(job, &ups[(size_t)j]))) return rc;
      kind[(size_t)j] = ups[(size_t)j].multi ? 0 : 3;  // (a compose_up_multi_<n> job: a launch of its own, in its turn)
    } else if ((rc = dispatch(ctx, progs[j], args[j], n_args[j], queue, true))) {
      return rc;
    }
  }
  for (int j = 0; j < n_jobs;) {
    if (!kind[(size_t)j]) {
      if ((rc = dispatch(ctx, progs[j], args[j], n_args[j], queue))) return rc;
      g_programs_done = ++j;
      continue;
    }
    int k = j;
    if (inject_failure(ctx)) return fail(PH_E_HIP, "ph_run_programs: launch failed: injected (context option fail_launches)");
    if (kind[(size_t)j] == 2) {
      // frames of one size, layer count and recipe: one launch of the headline kernel (ph_fused_v210_combine_batch).  A frame that reads
      // what an earlier frame of the run writes (or writes what one reads or writes) starts the next launch: call order is kept.
      const FusedCall &f0 = fused[(size_t)j];
      std::vector<const void *> layers;
      std::vector<void *> outs;
      prints.clear();
      for (; k < n_jobs && kind[(size_t)k] == 2 && k - j < ph::kMaxBatch; ++k) {
        const FusedCall &f = fused[(size_t)k];
        if (f.n != f0.n || f.width != f0.width || f.height != f0.height || !(f.r == f0.r)) break;
        fused_footprint(f, prints.emplace_back());
        if (!joins(kAllHazards)) break;
        layers.insert(layers.end(), f.layers, f.layers + f.n);
        outs.push_back(f.out);
      }
      rc = ph_fused_v210_combine_batch(ctx, queue, (int)outs.size(), f0.n, layers.data(), outs.data(), f0.width, f0.height, f0.r.rd_cm->dptr, f0.r.rd_lut->dptr,
                                       f0.r.rd_gm->dptr, f0.r.wr_cm->dptr, f0.r.wr_lut->dptr);
      if (rc) return rc;
      g_programs_done = j = k;
      continue;
    }
    if (kind[(size_t)j] == 5) {
      // plain-layer composites for one list of consumers - one size, layer count, Loader recipe and, output by output, format, field mode,
      // writer matrix and table - in one launch of up to kMaxBatch jobs (ph_fused_v210_combine_multi_batch).  The jobs of a launch are made
      // side by side, so a job one of whose layers overlaps a plane an earlier job of the group writes, or one of whose planes overlaps a
      // layer an earlier job reads or a plane it writes, starts the next launch: call order is kept.  By byte range, as the headline
      // kernel's groups: a layer is any v210_bytes, a plane what its format gives it.
      const FusedMultiCall &m0 = multis[(size_t)j];
      std::vector<const void *> layers;
      std::vector<ph_chan_output> outs;
      prints.clear();
      for (; k < n_jobs && kind[(size_t)k] == 5 && k - j < ph::kMaxBatch; ++k) {
        const FusedMultiCall &m = multis[(size_t)k];
        bool same = m.n == m0.n && m.width == m0.width && m.height == m0.height && m.n_out == m0.n_out && m.r.rd_cm == m0.r.rd_cm && m.r.rd_lut == m0.r.rd_lut &&
                    m.r.rd_gm == m0.r.rd_gm;
        for (int o = 0; o < m0.n_out && same; ++o)
          same = m.outs[o].format == m0.outs[o].format && m.outs[o].interlace == m0.outs[o].interlace && m.outs[o].wr_col_matrix12 == m0.outs[o].wr_col_matrix12 &&
                 m.outs[o].wr_gamma_lut == m0.outs[o].wr_gamma_lut;
        if (!same) break;
        fused_multi_footprint(m, prints.emplace_back());
        if (!joins(kAllHazards)) break;
        layers.insert(layers.end(), m.layers, m.layers + m.n);
        outs.insert(outs.end(), m.outs, m.outs + m.n_out);
      }
      rc = ph_fused_v210_combine_multi_batch(ctx, queue, k - j, m0.n, layers.data(), m0.n_out, outs.data(), m0.width, m0.height, m0.r.rd_cm->dptr, m0.r.rd_lut->dptr,
                                             m0.r.rd_gm->dptr);
      if (rc) return rc;
      g_programs_done = j = k;
      continue;
    }
    if (kind[(size_t)j] == 3) {
      // frames of the 2 x 2-block compositor of ONE shape (layer count, image format and sizes, placements, output size, field mode, Saver) -
      // several channels' frames from de-interlaced fields, each job one frame or a frame's two fields - in one launch of up to
      // kMaxUpJobs frames (ph_compose_up_write_v210_batch).  The frames of one launch are made side by side, so a job that writes a frame an
      // earlier one of the group writes, whose layer images (either field's) overlap a frame an earlier one writes, or whose frame overlaps
      // an earlier one's layer images starts the next launch: call order is kept.  By byte range, as the headline kernel's groups - a
      // layer image is any buffer of w * h * 16 bytes (packedRgb: 12), a frame any buffer of v210_bytes.
      const UpCall &u0 = ups[(size_t)j];
      const ph_image_layer *sets[ph::kMaxUpJobs];
      void *outs[ph::kMaxUpJobs];
      int frames = 0;
      prints.clear();
      for (; k < n_jobs && kind[(size_t)k] == 3; ++k) {
        const UpCall &u = ups[(size_t)k];
        bool same = u.n == u0.n && u.rgb == u0.rgb && u.width == u0.width && u.height == u0.height && u.interlace == u0.interlace && u.r == u0.r;
        for (int l = 0; l < u.n && same; ++l) {
          same = u.layers[l].width == u0.layers[l].width && u.layers[l].height == u0.layers[l].height;
          for (int e = 0; e < 9 && same; ++e) same = u.layers[l].matrix9_host[e] == u0.layers[l].matrix9_host[e];
        }
        if (!same || frames + (u.pair ? 2 : 1) > ph::kMaxUpJobs) break;
        Footprint &fp = prints.emplace_back();
        up_footprint(u, fp);
        // written twice - by the job's own pair, or by an earlier job -, read here after it is written there, or written here after it is read there
        if ((fp.n_writes == 2 && spans_meet(fp.writes[0], fp.writes[1])) || !joins(kAllHazards)) break;
        sets[frames] = u.layers, outs[frames++] = u.o->dptr;
        if (u.pair) sets[frames] = u.layers2, outs[frames++] = u.o2->dptr;
      }
      if (k == j) {  // (the first job does not fit a group of its own making - a pair writing one buffer twice: as it is, for its own error)
        if ((rc = dispatch(ctx, progs[j], args[j], n_args[j], queue, false, true))) return rc;  // (the injection was asked above, once per launch)
        g_programs_done = ++j;
        continue;
      }
      rc = ph_compose_up_write_v210_batch(ctx, queue, frames, u0.n, sets, outs, u0.width, u0.height, u0.interlace, u0.r.wr_cm->dptr, u0.r.wr_lut->dptr);
      if (rc) return rc;
      g_programs_done = j = k;
      continue;
    }
    if (kind[(size_t)j] == 4 || kind[(size_t)j] == 6) {
      // channels' frames for consumers other than SDI, or for several consumers, of one geometry and one Loader recipe: one call of
      // ph_chan_compose_batch_out, which itself starts the next launch where a job reads or writes what an earlier one writes, and runs
      // the jobs that name another Saver table in their turn.  6: the same for clip_compose_multi_<n> jobs (file playback) through
      // ph_clip_compose_batch_out, which runs whatever its shared launch does not take through ph_clip_compose_multi in its turn
      const ChanCall &c0 = calls[(size_t)j];
      const char group = kind[(size_t)j];
      std::vector<ph_chan_job_out> batch;
      for (; k < n_jobs && kind[(size_t)k] == group; ++k) {
        const ChanCall &c = calls[(size_t)k];
        if (c.width != c0.width || c.height != c0.height || c.r.rd_cm != c0.r.rd_cm || c.r.rd_lut != c0.r.rd_lut || c.r.rd_gm != c0.r.rd_gm) break;
        batch.push_back(ph_chan_job_out{c.n_layers, c.layers, c.n_out, c.outs});
      }
      rc = (group == 6 ? ph_clip_compose_batch_out : ph_chan_compose_batch_out)(ctx, queue, (int)batch.size(), batch.data(), c0.width, c0.height, c0.r.rd_cm->dptr,
                                                                                 c0.r.rd_lut->dptr, c0.r.rd_gm->dptr);
      if (rc) return rc;
      g_programs_done = j = k;
      continue;
    }
    const ChanCall &c0 = calls[(size_t)j];
    std::vector<ph_chan_job> batch;
    // a frame that reads what an earlier frame of the group writes (a channel routed into another), or writes what one reads, starts the next
    // call of ph_chan_compose_batch: the jobs of one such call may share launches, and call order has to hold
    prints.clear();
    for (; k < n_jobs && kind[(size_t)k] == 1; ++k) {
      const ChanCall &c = calls[(size_t)k];
      if (c.width != c0.width || c.height != c0.height || !(c.r == c0.r)) break;
      chan_footprint(c, prints.emplace_back());
      // (WAW is not asked here: ph_chan_compose_batch sees to the jobs that name one frame, and keeps the two fields of a frame in one launch)
      if (!joins(kRAW | kWAR)) break;
      batch.push_back(ph_chan_job{c.n_layers, c.layers, c.out_planes[0], c.interlace});
    }
    rc = ph_chan_compose_batch(ctx, queue, (int)batch.size(), batch.data(), c0.width, c0.height, c0.r.rd_cm->dptr, c0.r.rd_lut->dptr, c0.r.rd_gm->dptr,
                               c0.r.wr_cm->dptr, c0.r.wr_lut->dptr);
    if (rc) return rc;
    g_programs_done = j = k;
  }
  return PH_OK;
}

}  // extern "C"
