// ph_api.cpp - the C ABI of libphaneron_hip.so (include/phaneron_hip.h): context, ref-counted
// pooled device buffers, queues and the typed entry points.  Programs and their by-name jobs (the nodencl
// `runProgram` contract the reference's clJobQueue drives) are ph_run.cpp, which calls the typed entry points.
//
// No CPU path exists here: every entry point that does work needs a HIP device.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/phaneron_hip.h"
#include "ph_fused_field.h"
#include "ph_internal.h"
#include "ph_kernels.h"
#include "ph_lut_host.h"

using ph::KernelId;
using namespace ph;  // K_* kernel ids

namespace {
thread_local std::string g_err;
}  // namespace

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

namespace {

// the formats defined for even sizes only (fmt_even_size: a line pair per chroma line, a sample pair per chroma sample)
int even_dims(const char *fn, int f, uint32_t w, uint32_t h) {
  if (fmt_even_size(f) && ((w & 1) || (h & 1)))
    return fail(PH_E_INVALID, "%s: a %s frame needs an even width and height (%ux%u)", fn, fmt_name(f), w, h);
  return PH_OK;
}

}  // namespace

// ---- route trace: which kernels made it ------------------------------------------------------------------------------------------
// Which of the library's routes makes a frame is decided here and in the launchers (headline kernel / channel kernel and its
// instantiations / batch kernel / read + 2 x 2-block compositor / pair launch ...), so a caller - and a test - can ASK: between
// ph_trace_begin and ph_trace_end every launch of the calling thread is noted by kernel name, and in a dry run that is all that happens.
namespace {
thread_local bool g_trace_on = false, g_trace_dry = false;
thread_local std::string g_trace;
}  // namespace
namespace ph {
bool trace_launch(const char *name) {
  if (!g_trace_on) return false;
  if (const char *p = strstr(name, "launch_")) name = p + 7;
  if (!g_trace.empty()) g_trace += '+';
  g_trace.append(name, strcspn(name, "("));
  return g_trace_dry;
}
}  // namespace ph

int set_device(ph_ctx *ctx) {
  if (ctx->closed.load()) return fail(PH_E_INVALID, "the context has been destroyed");
  PH_HIP(hipSetDevice(ctx->device));
  ph::t_stream_images = (uint32_t)ctx->stream_images;  // the launch that follows on this thread takes the context's store policy
  ph::t_stream_threshold_mb = (uint32_t)ctx->stream_threshold_mb;
  return PH_OK;
}

namespace {

void order_queues_after_routes(ph_ctx *ctx);  // below, with ph_route

int pool_alloc(ph_ctx *ctx, size_t bytes, void **out) {
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    auto it = ctx->pool.find(bytes);
    if (it != ctx->pool.end()) {
      *out = it->second;
      ctx->pool.erase(it);
      ctx->pooled_bytes -= bytes;
      // the block's previous owner may have released it right after ph_route_send: RCCL could still be reading it on
      // the communication stream, which the three queues know nothing about
      order_queues_after_routes(ctx);
      return PH_OK;
    }
  }
  PH_HIP(hipMalloc(out, bytes ? bytes : 1));
  return PH_OK;
}

void pool_free(ph_ctx *ctx, size_t bytes, void *p) {
  // Recycling is stream-safe because all kernels touching a buffer were enqueued (in order)
  // before its last release, and the next user enqueues after it on the same in-order queues;
  // cross-queue users call ph_wait_finish first, exactly as the reference does (io.ts, clJobQueue.ts:131).
  // ROUTE transfers run on a fourth stream: pool_alloc orders the queues behind them before a block is reused.
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->pool.emplace(bytes, p);
  ctx->pooled_bytes += bytes;
}

}  // namespace

void ctx_ref(ph_ctx *ctx) { ctx->refs.fetch_add(1); }

namespace {

// contexts that exist: ph_ctx_destroy on a pointer that is no longer (or never was) a context is refused instead of
// touching freed storage (a second destroy after the last handle went)
std::mutex g_live_mu;
std::vector<ph_ctx *> g_live;
bool ctx_is_live(ph_ctx *ctx) {
  std::lock_guard<std::mutex> lock(g_live_mu);
  for (ph_ctx *c : g_live)
    if (c == ctx) return true;
  return false;
}

}  // namespace

// drops one reference; the last one frees the device state (streams, pool, LUT blobs)
void ctx_unref(ph_ctx *ctx) {
  if (ctx->refs.fetch_sub(1) != 1) return;
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    for (size_t i = 0; i < g_live.size(); ++i)
      if (g_live[i] == ctx) {
        g_live.erase(g_live.begin() + (long)i);
        break;
      }
  }
  hipSetDevice(ctx->device);
  for (int i = 0; i < 3; ++i)
    if (ctx->streams[i]) {
      hipStreamSynchronize(ctx->streams[i]);
      hipStreamDestroy(ctx->streams[i]);
    }
  for (auto &kv : ctx->pool) hipFree(kv.second);
  for (auto &kv : ctx->host_pool) {
    hipHostFree(kv.second.p);
    if (kv.second.busy) hipEventDestroy(kv.second.busy);
  }
  for (auto &kv : ctx->luts)
    if (kv.second.blob_dev) hipFree(kv.second.blob_dev);
  for (int i = 0; i < 3; ++i)
    if (ctx->chan_index[i]) hipFree(ctx->chan_index[i]);
  delete ctx;
}

int closed_error(const char *fn) { return fail(PH_E_INVALID, "%s: the context has been destroyed", fn); }

extern "C" {

int ph_abi_version(void) { return PH_ABI_VERSION; }

const char *ph_last_error(ph_ctx *) { return g_err.c_str(); }

int ph_trace_begin(int dry_run) {
  g_trace_on = true, g_trace_dry = dry_run != 0;
  g_trace.clear();
  return PH_OK;
}
int ph_trace_end(char *route, size_t len) {
  const bool was_on = g_trace_on;
  g_trace_on = g_trace_dry = false;
  if (!was_on) return fail(PH_E_INVALID, "ph_trace_end: no ph_trace_begin on this thread");
  if (!route || len <= g_trace.size()) return fail(PH_E_RANGE, "ph_trace_end: the route takes %zu bytes", g_trace.size() + 1);
  memcpy(route, g_trace.c_str(), g_trace.size() + 1);
  return PH_OK;
}

int ph_ctx_create(int device_index, ph_ctx **out) {
  if (!out) return fail(PH_E_INVALID, "ph_ctx_create: out is NULL");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(PH_E_NO_DEVICE, "no HIP device available (%s); libphaneron_hip has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device_index < 0 || device_index >= count) return fail(PH_E_INVALID, "device index %d out of range (%d devices)", device_index, count);
  ph_ctx *ctx = new ph_ctx();
  ctx->device = device_index;
  PH_HIP(hipSetDevice(device_index));
  PH_HIP(hipGetDeviceProperties(&ctx->props, device_index));
  for (int i = 0; i < 3; ++i) PH_HIP(hipStreamCreateWithFlags(&ctx->streams[i], hipStreamNonBlocking));
  {
    std::lock_guard<std::mutex> lock(g_live_mu);
    g_live.push_back(ctx);
  }
  *out = ctx;
  return PH_OK;
}

int ph_ctx_destroy(ph_ctx *ctx) {
  if (!ctx) return PH_OK;
  if (!ctx_is_live(ctx)) return PH_OK;  // destroyed before and every handle gone since: the storage no longer exists
  if (ctx->closed.exchange(true)) return PH_OK;  // second destroy: the creator's reference is already gone
  hipSetDevice(ctx->device);
  for (int i = 0; i < 3; ++i)
    if (ctx->streams[i]) hipStreamSynchronize(ctx->streams[i]);
  ctx_unref(ctx);  // handles still alive keep the storage they point into; the last one tears down
  return PH_OK;
}

int ph_ctx_info(ph_ctx *ctx, char *vendor, size_t vlen, char *device, size_t dlen) {
  if (!ctx) return fail(PH_E_INVALID, "ph_ctx_info: ctx is NULL");
  if (vendor && vlen) snprintf(vendor, vlen, "Advanced Micro Devices, Inc.");
  if (device && dlen) snprintf(device, dlen, "%s (%s)", ctx->props.name, ctx->props.gcnArchName);
  return PH_OK;
}

void *ph_ctx_stream(ph_ctx *ctx, int queue) { return ctx && queue_ok(queue) ? (void *)ctx->streams[queue] : nullptr; }

int ph_wait_finish(ph_ctx *ctx, int queue) {
  if (!ctx) return fail(PH_E_INVALID, "ph_wait_finish: ctx is NULL");
  if (ctx->closed.load()) return closed_error("ph_wait_finish");
  PH_QUEUE("ph_wait_finish", queue);
  PH_HIP(hipStreamSynchronize(stream_of(ctx, queue)));
  return PH_OK;
}

// ---- buffers -------------------------------------------------------------------------------
int ph_buf_create(ph_ctx *ctx, size_t bytes, int access, int svm_type, int width, int height, const char *owner,
                  ph_buf **out) {
  (void)access;
  (void)svm_type;  // OpenCL SVM hints have no HIP counterpart: device memory + pinned mirror
  if (!ctx || !out) return fail(PH_E_INVALID, "ph_buf_create: NULL argument");
  if (width > 0 && height > 0 && bytes < (size_t)width * height * 16)
    return fail(PH_E_RANGE, "ph_buf_create: %zu bytes cannot hold a %dx%d RGBA f32 image", bytes, width, height);
  int rc = set_device(ctx);
  if (rc) return rc;
  void *d = nullptr;
  rc = pool_alloc(ctx, bytes, &d);
  if (rc) return rc;
  ph_buf *b = new ph_buf{ctx, d, nullptr, bytes, width > 0 ? width : 0, height > 0 ? height : 0, {1}, true, false,
                         false, owner ? owner : ""};
  ctx_ref(ctx);
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->live_buffers++;
    ctx->live_bytes += bytes;
  }
  *out = b;
  return PH_OK;
}

int ph_buf_wrap(ph_ctx *ctx, void *device_ptr, size_t bytes, int width, int height, ph_buf **out) {
  if (!ctx || !out || !device_ptr) return fail(PH_E_INVALID, "ph_buf_wrap: NULL argument");
  if (ctx->closed.load()) return closed_error("ph_buf_wrap");
  *out = new ph_buf{ctx, device_ptr, nullptr, bytes, width > 0 ? width : 0, height > 0 ? height : 0, {1}, false, false,
                    false, "wrapped"};
  ctx_ref(ctx);
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->live_buffers++;
  }
  return PH_OK;
}

int ph_buf_addref(ph_buf *b) {
  if (!b) return fail(PH_E_INVALID, "ph_buf_addref: NULL buffer");
  return b->refs.fetch_add(1), PH_OK;
}

int ph_buf_release(ph_buf *b) {
  if (!b) return fail(PH_E_INVALID, "ph_buf_release: NULL buffer");
  if (b->refs.fetch_sub(1) > 1) return PH_OK;
  ph_ctx *ctx = b->ctx;
  hipSetDevice(ctx->device);
  ph_lut_unregister(ctx, b->dptr);  // the storage goes back to the pool: forget any LUT form of it
  if (b->owned) pool_free(ctx, b->bytes, b->dptr);
  if (b->hptr) {
    // The mirror goes to the pool WITH the event behind its last asynchronous copy (the next owner waits for it).  Over budget the
    // OLDEST blocks make room - after a format change the pool would otherwise fill with sizes nobody asks for any more and every
    // new size pay hipHostMalloc / hipHostFree again (~40 ms for a 2160p image); a block larger than the whole budget is freed.
    std::vector<ph_ctx::HostBlock> victims;
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      const size_t fixed = (size_t)ctx->host_pool_mb << 20;
      const size_t budget = ctx->host_pool_mb && ctx->host_peak_bytes > fixed ? ctx->host_peak_bytes : fixed;  // (0: no pool at all)
      ctx->host_live_bytes -= b->bytes;
      if (b->bytes > budget) {
        victims.push_back(ph_ctx::HostBlock{b->hptr, b->mirror_busy, 0});
      } else {
        while (ctx->host_pooled_bytes + b->bytes > budget && !ctx->host_pool.empty()) {
          auto oldest = ctx->host_pool.begin();
          for (auto it = ctx->host_pool.begin(); it != ctx->host_pool.end(); ++it)
            if (it->second.seq < oldest->second.seq) oldest = it;
          victims.push_back(oldest->second);
          ctx->host_pooled_bytes -= oldest->first;
          ctx->host_pool.erase(oldest);
        }
        ctx->host_pool.emplace(b->bytes, ph_ctx::HostBlock{b->hptr, b->mirror_busy, ctx->host_pool_seq++});
        ctx->host_pooled_bytes += b->bytes;
      }
    }
    for (auto &v : victims) {
      hipHostFree(v.p);  // (waits for copies in flight)
      if (v.busy) hipEventDestroy(v.busy);
    }
  } else if (b->mirror_busy) {
    hipEventDestroy(b->mirror_busy);
  }
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (b->owned) ctx->live_bytes -= b->bytes;
    ctx->live_buffers--;
  }
  delete b;
  ctx_unref(ctx);
  return PH_OK;
}

int ph_buf_refcount(const ph_buf *b) { return b ? b->refs.load() : 0; }
size_t ph_buf_bytes(const ph_buf *b) { return b ? b->bytes : 0; }
void *ph_buf_device_ptr(ph_buf *b) { return b ? b->dptr : nullptr; }
int ph_buf_dims(const ph_buf *b, int *w, int *h) {
  if (!b) return fail(PH_E_INVALID, "ph_buf_dims: NULL buffer");
  if (w) *w = b->width;
  if (h) *h = b->height;
  return PH_OK;
}

// an asynchronous copy into or out of b's mirror has just been enqueued on `s`
extern "C++" void mirror_mark(ph_buf *b, hipStream_t s) {
  if (!b->mirror_busy && hipEventCreateWithFlags(&b->mirror_busy, hipEventDisableTiming) != hipSuccess) {
    b->mirror_busy = nullptr;
    hipStreamSynchronize(s);  // no event to carry: wait here rather than let the mirror go back to the pool under the copy
    return;
  }
  // ONE event stands for every copy of this mirror still in flight: a copy on another queue than the last one's (an upload on LOAD,
  // then a downloadAsync on UNLOAD) is ordered behind it first, so that the event recorded now covers both
  if (b->mirror_stream && b->mirror_stream != s) hipStreamWaitEvent(s, b->mirror_busy, 0);
  b->mirror_stream = s;
  hipEventRecord(b->mirror_busy, s);
}

void *ph_buf_host_ptr(ph_buf *b) {
  if (!b) return nullptr;
  if (!b->hptr) {
    {
      std::unique_lock<std::mutex> lock(b->ctx->mu);
      auto it = b->ctx->host_pool.find(b->bytes);
      if (it != b->ctx->host_pool.end()) {
        b->hptr = it->second.p;
        b->mirror_busy = it->second.busy;
        b->ctx->host_pool.erase(it);
        b->ctx->host_pooled_bytes -= b->bytes;
        b->ctx->host_live_bytes += b->bytes;
        if (b->ctx->host_live_bytes > b->ctx->host_peak_bytes) b->ctx->host_peak_bytes = b->ctx->host_live_bytes;
        lock.unlock();
        // the previous owner may have released the buffer with a download or an upload of this block still in flight
        // (release after downloadAsync, before its waitFinish: ADVICE r3); normally the event completed long ago
        if (b->mirror_busy) hipEventSynchronize(b->mirror_busy);
        return b->hptr;
      }
    }
    hipSetDevice(b->ctx->device);
    if (hipHostMalloc(&b->hptr, b->bytes ? b->bytes : 1, hipHostMallocDefault) != hipSuccess) {
      fail(PH_E_HIP, "hipHostMalloc(%zu) failed", b->bytes);
      b->hptr = nullptr;
    } else {
      std::lock_guard<std::mutex> lock(b->ctx->mu);
      b->ctx->host_pins++;
      b->ctx->host_live_bytes += b->bytes;
      if (b->ctx->host_live_bytes > b->ctx->host_peak_bytes) b->ctx->host_peak_bytes = b->ctx->host_live_bytes;
    }
  }
  return b->hptr;
}

/* A binding that keeps released buffers of its own (node/index.js parks frames and images whole: handle, device block, pinned mirror)
 * calls this when one of them gets its next owner: what ph_buf_release + ph_buf_create would have seen to - an asynchronous copy into
 * or out of the mirror still in flight (release after downloadAsync, before its waitFinish), a ROUTE transfer still reading or writing
 * the device block on the communication stream, and the previous owner's pending host data (a mirror filled but never handed back). */
int ph_buf_reuse(ph_buf *b) {
  if (!b || b->refs.load() <= 0) return fail(PH_E_INVALID, "ph_buf_reuse: NULL or released buffer");
  if (b->mirror_busy && hipEventSynchronize(b->mirror_busy) != hipSuccess) (void)hipGetLastError();
  {
    std::lock_guard<std::mutex> lock(b->ctx->mu);
    order_queues_after_routes(b->ctx);
  }
  b->host_dirty = false;
  b->lut_dirty = false;
  return PH_OK;
}

int ph_buf_host_access(ph_buf *b, int dir, int queue, const void *src, size_t bytes) {
  if (!b) return fail(PH_E_INVALID, "ph_buf_host_access: NULL buffer");
  PH_QUEUE("ph_buf_host_access", queue);
  int rc = set_device(b->ctx);
  if (rc) return rc;
  hipStream_t s = stream_of(b->ctx, queue);
  if (!ph_buf_host_ptr(b)) return PH_E_HIP;
  switch (dir) {
    case PH_HOST_WRITEONLY:
      if (src) {
        if (bytes > b->bytes) return fail(PH_E_RANGE, "hostAccess: %zu source bytes into a %zu byte buffer", bytes, b->bytes);
        // previous async upload from the mirror must have drained before it is overwritten
        PH_HIP(hipStreamSynchronize(s));
        memcpy(b->hptr, src, bytes);
        PH_HIP(hipMemcpyAsync(b->dptr, b->hptr, bytes, hipMemcpyHostToDevice, s));
        mirror_mark(b, s);
        b->host_dirty = false;
        b->lut_dirty = b->lut_dirty || b->bytes >= 65536 * 4;
      } else {
        b->host_dirty = true;  // caller fills the mirror, then calls hostAccess('none')
      }
      return PH_OK;
    case PH_HOST_NONE:
      if (b->host_dirty) {
        PH_HIP(hipMemcpyAsync(b->dptr, b->hptr, b->bytes, hipMemcpyHostToDevice, s));
        mirror_mark(b, s);
        b->host_dirty = false;
        b->lut_dirty = b->lut_dirty || b->bytes >= 65536 * 4;
      }
      return PH_OK;
    case PH_HOST_READONLY:
      PH_HIP(hipMemcpyAsync(b->hptr, b->dptr, b->bytes, hipMemcpyDeviceToHost, s));
      PH_HIP(hipStreamSynchronize(s));
      return PH_OK;
    default:
      return fail(PH_E_INVALID, "hostAccess: unknown direction %d", dir);
  }
}

int ph_queue_query(ph_ctx *ctx, int queue) {
  if (!ctx) return fail(PH_E_INVALID, "ph_queue_query: ctx is NULL");
  PH_QUEUE("ph_queue_query", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  hipError_t e = hipStreamQuery(stream_of(ctx, queue));
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(PH_E_HIP, "ph_queue_query: %s", hipGetErrorString(e));
}

int ph_queue_wait_queue(ph_ctx *ctx, int waiter_queue, int signal_queue) {
  if (!ctx) return fail(PH_E_INVALID, "ph_queue_wait_queue: ctx is NULL");
  if (waiter_queue < 0 || waiter_queue > 2 || signal_queue < 0 || signal_queue > 2)
    return fail(PH_E_INVALID, "ph_queue_wait_queue: queues are 0..2");
  if (waiter_queue == signal_queue) return PH_OK;  // in-order already
  int rc = set_device(ctx);
  if (rc) return rc;
  hipEvent_t ev;
  PH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, ctx->streams[signal_queue]);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->streams[waiter_queue], ev, 0);
  hipEventDestroy(ev);  // released by the runtime once the recorded work has completed
  if (e != hipSuccess) return fail(PH_E_HIP, "ph_queue_wait_queue: %s", hipGetErrorString(e));
  return PH_OK;
}

int ph_buf_download_async(ph_buf *b, int queue) {
  if (!b) return fail(PH_E_INVALID, "ph_buf_download_async: NULL buffer");
  PH_QUEUE("ph_buf_download_async", queue);
  int rc = set_device(b->ctx);
  if (rc) return rc;
  if (!ph_buf_host_ptr(b)) return PH_E_HIP;
  hipStream_t s = stream_of(b->ctx, queue);
  PH_HIP(hipMemcpyAsync(b->hptr, b->dptr, b->bytes, hipMemcpyDeviceToHost, s));
  mirror_mark(b, s);
  return PH_OK;
}

struct ph_event {
  ph_ctx *ctx;
  hipEvent_t ev;
};

int ph_event_record(ph_ctx *ctx, int queue, ph_event **out) {
  if (!ctx || !out) return fail(PH_E_INVALID, "ph_event_record: NULL argument");
  PH_QUEUE("ph_event_record", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  hipEvent_t ev;
  PH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, stream_of(ctx, queue));
  if (e != hipSuccess) {
    hipEventDestroy(ev);
    return fail(PH_E_HIP, "ph_event_record: %s", hipGetErrorString(e));
  }
  *out = new ph_event{ctx, ev};
  ctx_ref(ctx);
  return PH_OK;
}

/* a point in `queue` that can be timed against another (ph_event_elapsed_us): RunTimings of a recording binding's fused launches */
int ph_event_record_timed(ph_ctx *ctx, int queue, ph_event **out) {
  if (!ctx || !out) return fail(PH_E_INVALID, "ph_event_record_timed: NULL argument");
  PH_QUEUE("ph_event_record_timed", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  hipEvent_t ev;
  PH_HIP(hipEventCreate(&ev));
  hipError_t e = hipEventRecord(ev, stream_of(ctx, queue));
  if (e != hipSuccess) {
    hipEventDestroy(ev);
    return fail(PH_E_HIP, "ph_event_record_timed: %s", hipGetErrorString(e));
  }
  *out = new ph_event{ctx, ev};
  ctx_ref(ctx);
  return PH_OK;
}

int ph_event_elapsed_us(ph_event *from, ph_event *to, uint32_t *us) {
  if (!from || !to || !us) return fail(PH_E_INVALID, "ph_event_elapsed_us: NULL argument");
  float ms = 0.f;
  hipError_t e = hipEventElapsedTime(&ms, from->ev, to->ev);  // both finished, both recorded with timing (ph_event_record_timed)
  if (e != hipSuccess) return fail(PH_E_HIP, "ph_event_elapsed_us: %s", hipGetErrorString(e));
  *us = (uint32_t)(ms * 1000.0f + 0.5f);
  return PH_OK;
}

int ph_event_wait(ph_event *ev) {
  if (!ev) return fail(PH_E_INVALID, "ph_event_wait: NULL event");
  int rc = set_device(ev->ctx);
  if (rc) return rc;
  PH_HIP(hipEventSynchronize(ev->ev));
  return PH_OK;
}

int ph_event_query(ph_event *ev) {
  if (!ev) return fail(PH_E_INVALID, "ph_event_query: NULL event");
  hipError_t e = hipEventQuery(ev->ev);
  if (e == hipSuccess) return 1;
  if (e == hipErrorNotReady) return 0;
  return fail(PH_E_HIP, "ph_event_query: %s", hipGetErrorString(e));
}

int ph_event_destroy(ph_event *ev) {
  if (!ev) return PH_OK;
  ph_ctx *ctx = ev->ctx;
  hipEventDestroy(ev->ev);
  delete ev;
  ctx_unref(ctx);
  return PH_OK;
}

struct ph_graph {
  ph_ctx *ctx;
  hipGraph_t graph;
  hipGraphExec_t exec;
};

int ph_graph_begin(ph_ctx *ctx, int queue) {
  if (!ctx) return fail(PH_E_INVALID, "ph_graph_begin: ctx is NULL");
  PH_QUEUE("ph_graph_begin", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  // relaxed: other threads (the libuv pool of the node addon) may keep calling into HIP meanwhile
  PH_HIP(hipStreamBeginCapture(stream_of(ctx, queue), hipStreamCaptureModeRelaxed));
  return PH_OK;
}

int ph_graph_end(ph_ctx *ctx, int queue, ph_graph **out) {
  if (!ctx || !out) return fail(PH_E_INVALID, "ph_graph_end: NULL argument");
  PH_QUEUE("ph_graph_end", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  hipGraph_t g = nullptr;
  PH_HIP(hipStreamEndCapture(stream_of(ctx, queue), &g));
  if (!g) return fail(PH_E_HIP, "ph_graph_end: nothing was recorded");
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    hipGraphDestroy(g);
    return fail(PH_E_HIP, "ph_graph_end: hipGraphInstantiate: %s", hipGetErrorString(e));
  }
  *out = new ph_graph{ctx, g, exec};
  ctx_ref(ctx);
  return PH_OK;
}

int ph_graph_launch(ph_graph *g, int queue) {
  if (!g) return fail(PH_E_INVALID, "ph_graph_launch: NULL graph");
  PH_QUEUE("ph_graph_launch", queue);
  int rc = set_device(g->ctx);
  if (rc) return rc;
  PH_HIP(hipGraphLaunch(g->exec, stream_of(g->ctx, queue)));
  return PH_OK;
}

int ph_graph_destroy(ph_graph *g) {
  if (!g) return PH_OK;
  ph_ctx *ctx = g->ctx;
  hipGraphExecDestroy(g->exec);
  hipGraphDestroy(g->graph);
  delete g;
  ctx_unref(ctx);
  return PH_OK;
}

// ---- ROUTE: RCCL point-to-point on a communication stream of its own ----------------------------------
// RCCL is loaded with dlopen(RTLD_LOCAL): the library has no link-time dependency on it, and a host process
// that already carries another copy (PyTorch ships one) keeps the two apart.
struct Id128 {  // ncclUniqueId, passed to ncclCommInitRank by value
  char bytes[128];
};
namespace {
struct Rccl {
  void *handle = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  int (*CommInitRank)(void **, int, Id128, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::mutex g_rccl_mu;
const int kNcclUint32 = 3;  // ncclUint32 (rccl.h ncclDataType_t)

int load_rccl() {
  std::lock_guard<std::mutex> lock(g_rccl_mu);
  if (g_rccl.handle) return PH_OK;
  const char *names[] = {getenv("PH_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *h = nullptr;
  for (const char *n : names)
    if (n && *n && (h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
  if (!h) return fail(PH_E_HIP, "ROUTE needs RCCL and librccl.so could not be loaded (%s)", dlerror());
#define PH_SYM(field, name)                                                              \
  if (!(*(void **)(&g_rccl.field) = dlsym(h, name))) {                                    \
    dlclose(h);                                                                          \
    return fail(PH_E_HIP, "librccl.so lacks %s", name);                                  \
  }
  PH_SYM(GetUniqueId, "ncclGetUniqueId")
  PH_SYM(CommInitRank, "ncclCommInitRank")
  PH_SYM(CommDestroy, "ncclCommDestroy")
  PH_SYM(Send, "ncclSend")
  PH_SYM(Recv, "ncclRecv")
  PH_SYM(GroupStart, "ncclGroupStart")
  PH_SYM(GroupEnd, "ncclGroupEnd")
  PH_SYM(CommCount, "ncclCommCount")
  PH_SYM(GetErrorString, "ncclGetErrorString")
#undef PH_SYM
  g_rccl.handle = h;
  return PH_OK;
}
#define PH_NCCL(call)                                                                               \
  do {                                                                                              \
    int r_ = (call);                                                                                \
    if (r_ != 0) return fail(PH_E_HIP, "%s failed: %s", #call, g_rccl.GetErrorString(r_));          \
  } while (0)
}  // namespace

struct ph_route {
  ph_ctx *ctx;
  void *comm;
  hipStream_t stream;
  int rank, world;
  hipEvent_t last = nullptr;         // recorded behind the latest transfer enqueued on `stream`
  bool in_group = false;
  std::atomic<bool> busy{false};     // `last` may not have completed yet
};

extern "C++" {
namespace {
// Buffer lifetime against ROUTE (the source rank's `send(frame); frame.release()`): the pool hands a recycled block out
// only after the three queues have been ordered behind every transfer enqueued so far.  Device-side waits only, and
// only while a transfer is really in flight (hipEventQuery).  Called with ctx->mu held.
// `busy` and `last` change only under ctx->mu (route_mark takes it too): a pool thread that found the old record complete
// cannot clear the flag after another thread has recorded a new transfer.  A queue that is being captured
// (ph_graph_begin) is left alone - an event recorded outside the capture cannot be waited for inside it; if a wait cannot
// be enqueued the host waits for the transfer instead, so a recycled block is never handed out under RCCL's read.
void order_queues_after_routes(ph_ctx *ctx) {
  for (ph_route *r : ctx->routes) {
    if (!r->busy.load() || !r->last) continue;
    if (hipEventQuery(r->last) == hipSuccess) {
      r->busy.store(false);
      continue;
    }
    for (int q = 0; q < 3; ++q) {
      hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(ctx->streams[q], &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone) continue;
      if (hipStreamWaitEvent(ctx->streams[q], r->last, 0) != hipSuccess) {
        (void)hipGetLastError();
        hipEventSynchronize(r->last);
        r->busy.store(false);
        break;
      }
    }
  }
}
int route_mark(ph_route *r) {  // a transfer has just been enqueued on the communication stream
  std::lock_guard<std::mutex> lock(r->ctx->mu);
  PH_HIP(hipEventRecord(r->last, r->stream));
  r->busy.store(true);
  return PH_OK;
}
}  // namespace
}  // extern "C++"

int ph_route_unique_id(void *id128) {
  if (!id128) return fail(PH_E_INVALID, "ph_route_unique_id: NULL argument");
  int rc = load_rccl();
  if (rc) return rc;
  static_assert(PH_ROUTE_ID_BYTES == sizeof(Id128), "ncclUniqueId is 128 bytes");
  PH_NCCL(g_rccl.GetUniqueId(id128));
  return PH_OK;
}

int ph_route_init(ph_ctx *ctx, const void *id128, int rank, int world, ph_route **out) {
  if (!ctx || !id128 || !out) return fail(PH_E_INVALID, "ph_route_init: NULL argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(PH_E_INVALID, "ph_route_init: rank %d of %d", rank, world);
  int rc = set_device(ctx);
  if (rc) return rc;
  rc = load_rccl();
  if (rc) return rc;
  Id128 id;
  memcpy(id.bytes, id128, sizeof id.bytes);
  void *comm = nullptr;
  PH_NCCL(g_rccl.CommInitRank(&comm, world, id, rank));
  hipStream_t s = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  if (e != hipSuccess) {
    g_rccl.CommDestroy(comm);
    return fail(PH_E_HIP, "ph_route_init: hipStreamCreate: %s", hipGetErrorString(e));
  }
  hipEvent_t ev = nullptr;
  e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (e != hipSuccess) {
    g_rccl.CommDestroy(comm);
    hipStreamDestroy(s);
    return fail(PH_E_HIP, "ph_route_init: hipEventCreate: %s", hipGetErrorString(e));
  }
  ph_route *r = new ph_route{ctx, comm, s, rank, world};
  r->last = ev;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->routes.push_back(r);
  }
  *out = r;
  ctx_ref(ctx);
  return PH_OK;
}

int ph_route_destroy(ph_route *r) {
  if (!r) return PH_OK;
  hipSetDevice(r->ctx->device);
  hipStreamSynchronize(r->stream);
  ph_ctx *ctx = r->ctx;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    for (size_t i = 0; i < ctx->routes.size(); ++i)
      if (ctx->routes[i] == r) {
        ctx->routes.erase(ctx->routes.begin() + (long)i);
        break;
      }
  }
  g_rccl.CommDestroy(r->comm);
  hipStreamDestroy(r->stream);
  if (r->last) hipEventDestroy(r->last);
  delete r;
  ctx_unref(ctx);
  return PH_OK;
}

int ph_route_group_begin(ph_route *r) {
  if (!r) return fail(PH_E_INVALID, "ph_route_group_begin: NULL route");
  PH_NCCL(g_rccl.GroupStart());
  r->in_group = true;
  return PH_OK;
}
int ph_route_group_end(ph_route *r) {
  if (!r) return fail(PH_E_INVALID, "ph_route_group_end: NULL route");
  int rc = set_device(r->ctx);
  if (rc) return rc;
  PH_NCCL(g_rccl.GroupEnd());
  r->in_group = false;
  return route_mark(r);  // the group's transfers are on the stream now
}

static int route_args(ph_route *r, const void *p, size_t bytes, int peer, const char *fn) {
  if (!r || !p) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (bytes % 4) return fail(PH_E_INVALID, "%s: %zu bytes is not a multiple of 4", fn, bytes);
  if (peer < 0 || peer >= r->world) return fail(PH_E_INVALID, "%s: peer %d of %d ranks", fn, peer, r->world);
  return set_device(r->ctx);
}
int ph_route_send(ph_route *r, const void *src, size_t bytes, int peer) {
  int rc = route_args(r, src, bytes, peer, "ph_route_send");
  if (rc) return rc;
  PH_NCCL(g_rccl.Send(src, bytes / 4, kNcclUint32, peer, r->comm, r->stream));
  return r->in_group ? PH_OK : route_mark(r);
}
int ph_route_recv(ph_route *r, void *dst, size_t bytes, int peer) {
  int rc = route_args(r, dst, bytes, peer, "ph_route_recv");
  if (rc) return rc;
  PH_NCCL(g_rccl.Recv(dst, bytes / 4, kNcclUint32, peer, r->comm, r->stream));
  return r->in_group ? PH_OK : route_mark(r);
}

static int order_streams(ph_ctx *ctx, hipStream_t waiter, hipStream_t signal, const char *fn) {
  int rc = set_device(ctx);
  if (rc) return rc;
  hipEvent_t ev;
  PH_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, signal);
  if (e == hipSuccess) e = hipStreamWaitEvent(waiter, ev, 0);
  hipEventDestroy(ev);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: %s", fn, hipGetErrorString(e));
  return PH_OK;
}
int ph_route_after_queue(ph_route *r, int queue) {
  if (!r || queue < 0 || queue > 2) return fail(PH_E_INVALID, "ph_route_after_queue: bad argument");
  return order_streams(r->ctx, r->stream, r->ctx->streams[queue], "ph_route_after_queue");
}
int ph_queue_after_route(ph_route *r, int queue) {
  if (!r || queue < 0 || queue > 2) return fail(PH_E_INVALID, "ph_queue_after_route: bad argument");
  return order_streams(r->ctx, r->ctx->streams[queue], r->stream, "ph_queue_after_route");
}
int ph_route_wait(ph_route *r) {
  if (!r) return fail(PH_E_INVALID, "ph_route_wait: NULL route");
  int rc = set_device(r->ctx);
  if (rc) return rc;
  PH_HIP(hipStreamSynchronize(r->stream));
  return PH_OK;
}
void *ph_route_stream(ph_route *r) { return r ? (void *)r->stream : nullptr; }
int ph_route_comm_count(ph_route *r, int *count) {
  if (!r || !count) return fail(PH_E_INVALID, "ph_route_comm_count: NULL argument");
  PH_NCCL(g_rccl.CommCount(r->comm, count));
  return PH_OK;
}

int ph_ctx_buffer_stats(ph_ctx *ctx, size_t *live_buffers, size_t *live_bytes, size_t *pooled_bytes) {
  if (!ctx) return fail(PH_E_INVALID, "ph_ctx_buffer_stats: ctx is NULL");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (live_buffers) *live_buffers = ctx->live_buffers;
  if (live_bytes) *live_bytes = ctx->live_bytes;
  if (pooled_bytes) *pooled_bytes = ctx->pooled_bytes;
  return PH_OK;
}

int ph_ctx_host_pool_stats(ph_ctx *ctx, size_t *in_use_bytes, size_t *pooled_bytes, size_t *peak_in_use_bytes, uint64_t *pins) {
  if (!ctx) return fail(PH_E_INVALID, "ph_ctx_host_pool_stats: ctx is NULL");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (in_use_bytes) *in_use_bytes = ctx->host_live_bytes;
  if (pooled_bytes) *pooled_bytes = ctx->host_pooled_bytes;
  if (peak_in_use_bytes) *peak_in_use_bytes = ctx->host_peak_bytes;
  if (pins) *pins = ctx->host_pins;
  return PH_OK;
}

// ---- gamma LUT registry ------------------------------------------------------------------------
int ph_lut_unregister(ph_ctx *ctx, const void *dev) {
  if (!ctx) return fail(PH_E_INVALID, "ph_lut_unregister: ctx is NULL");
  void *blob = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    auto it = ctx->luts.find(dev);
    if (it == ctx->luts.end()) return PH_OK;
    blob = it->second.blob_dev;
    ctx->luts.erase(it);
  }
  if (blob) {
    // kernels already enqueued may still read the blob: drain before freeing
    for (int q = 0; q < 3; ++q) hipStreamSynchronize(ctx->streams[q]);
    hipFree(blob);
  }
  return PH_OK;
}

int ph_lut_register(ph_ctx *ctx, const void *dev, const float *host) {
  if (!ctx || !dev || !host) return fail(PH_E_INVALID, "ph_lut_register: NULL argument");
  int rc = set_device(ctx);
  if (rc) return rc;
  ph_lut_unregister(ctx, dev);
  std::vector<uint32_t> blob;
  ph::LutHostInfo info;
  LutEntry e;
  if (ph::lut_compress(host, ph::kLutMaxLdsBytes, blob, info)) {
    if (!ctx->lds_base_checked.load()) {  // the lookups address the table absolutely: the kernels' dynamic shared array must start at LDS 0
      uint32_t *probe = nullptr, base = ~0u;
      PH_HIP(hipMalloc(&probe, 4));
      hipError_t pe = ph::launch_lds_base_probe(ctx->streams[0], probe);
      if (pe == hipSuccess) pe = hipStreamSynchronize(ctx->streams[0]);
      if (pe == hipSuccess) pe = hipMemcpy(&base, probe, 4, hipMemcpyDeviceToHost);
      hipFree(probe);
      if (pe != hipSuccess) return fail(PH_E_HIP, "ph_lut_register: LDS base probe: %s", hipGetErrorString(pe));
      if (base != 0) return fail(PH_E_HIP, "ph_lut_register: dynamic shared memory starts at LDS address %u, not 0: the table kernels cannot run", base);
      ctx->lds_base_checked.store(true);
    }
    const size_t blob_bytes = blob.size() * sizeof(uint32_t);  // info.bytes is the LDS footprint: the hole in front of the blob included
    PH_HIP(hipMalloc(&e.blob_dev, blob_bytes));
    PH_HIP(hipMemcpy(e.blob_dev, blob.data(), blob_bytes, hipMemcpyHostToDevice));
    e.view = ph::lut_view(info, e.blob_dev);
    e.max_finite = ph::lut_max_finite(host);
  }
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    ctx->luts[dev] = e;
  }
  return e.view.bytes ? 1 : 0;
}

int ph_lut_layout_of(const float *host, ph_lut_layout *layout, void *lds_image, size_t capacity) {
  if (!host || !layout) return fail(PH_E_INVALID, "ph_lut_layout_of: NULL argument");
  std::vector<uint32_t> blob;
  ph::LutHostInfo info;
  memset(layout, 0, sizeof(*layout));
  if (!ph::lut_compress(host, ph::kLutMaxLdsBytes, blob, info)) return 0;
  const ph::LutView v = ph::lut_view(info, nullptr);
  layout->lds_bytes = info.bytes, layout->hole = info.hole, layout->delta_off = info.delta_off, layout->shift = info.shift;
  layout->index_bias = (uint32_t)info.bias, layout->a_scale = v.a_scale;
  if (lds_image) {
    if (capacity < info.bytes) return fail(PH_E_INVALID, "ph_lut_layout_of: the image needs %u bytes, %zu given", info.bytes, capacity);
    memset(lds_image, 0, info.hole);
    memcpy(static_cast<char *>(lds_image) + info.hole, blob.data(), info.bytes - info.hole);
  }
  return (int)info.bytes;
}

// What the host computes for the fused kernel once per launch (ph_kernels.h: fused_lut_k, fused_wg_magic, fused_job_of), device-free,
// for tests/test_fused_args_cpu.py.  k5: the bit patterns of a_scale, a_base, delta_scale, delta_base, then a_shift; returns the
// table's LDS footprint as ph_lut_layout_of does (0: the table stays plain).
int ph_debug_fused_lut_k(const float *host, uint32_t k5[5]) {
  if (!host || !k5) return fail(PH_E_INVALID, "ph_debug_fused_lut_k: NULL argument");
  std::vector<uint32_t> blob;
  ph::LutHostInfo info;
  if (!ph::lut_compress(host, ph::kLutMaxLdsBytes, blob, info)) return 0;
  const ph::FusedLutK k = ph::fused_lut_k(ph::lut_view(info, nullptr));
  memcpy(k5, &k, 5 * sizeof(uint32_t));
  return (int)info.bytes;
}
// The fused kernel's witness guard as a launch gets it, device-free (tests/test_fused_witness_cpu.py): lmax = what ph_lut_register
// keeps of the reader table and fused_lds_args passes on, holds = the kernel's own expression (ph_kernels.h fused_witness_holds)
// of lmax and the nine gamut coefficients.
int ph_debug_fused_witness(const float *host, const float *gm9, float *lmax, int *holds) {
  if (!host || !gm9 || !lmax || !holds) return fail(PH_E_INVALID, "ph_debug_fused_witness: NULL argument");
  const ph::FusedLdsArgs a = ph::fused_lds_args(ph::FusedArgs{}, ph::LutView{}, ph::LutView{}, ph::lut_max_finite(host));
  *lmax = a.rd_lmax;
  *holds = ph::fused_witness_holds(a.rd_lmax, gm9) ? 1 : 0;
  return PH_OK;
}
// block / wg_per_job as the kernel takes it: the high word of (2 * block + 1) * magic
uint32_t ph_debug_fused_job_of(uint32_t wg_per_job, uint32_t block) {
  return wg_per_job ? ph::fused_job_of(block, ph::fused_wg_magic(wg_per_job)) : 0;
}
// Field quad g's place in the frame as the field launches' kernels make it (ph_fused_field.h, the function they inline), under the bounds
// the entries and launchers ask of a frame before those kernels see it
int ph_debug_fused_field_quad(uint32_t width, uint32_t height, int interlace, uint32_t g, uint32_t *f, uint32_t *line, uint32_t *col) {
  if (!width || width % 48) return fail(PH_E_INVALID, "ph_debug_fused_field_quad: width %u (the field launches take width %% 48 == 0)", width);
  if (interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "ph_debug_fused_field_quad: interlace %d (a field: 1 or 3)", interlace);
  const uint32_t qpl = width / 6;
  if ((uint64_t)qpl * height * qpl >= (1ull << 32)) return fail(PH_E_INVALID, "ph_debug_fused_field_quad: %u x %u is beyond the kernels' division by reciprocal", width, height);
  if (g >= qpl * (height / 2u)) return fail(PH_E_INVALID, "ph_debug_fused_field_quad: quad %u is outside the field (%u quads)", g, qpl * (height / 2u));
  const ph::FieldQuad q = ph::fused_field_quad(g, qpl, (uint32_t)(((1ull << 32) + qpl - 1) / qpl), interlace == 3 ? 1u : 0u);
  if (f) *f = q.f;
  if (line) *line = q.line;
  if (col) *col = q.col;
  return PH_OK;
}
// The store policy (ph_kernels.h image_nt) a launch issued next on the calling thread for `ctx` would be given for an image of `bytes`
// bytes: the context's "stream_images" / "stream_threshold_mb" as set_device hands them to the launchers.  0 cached, 1 streamed.
int ph_debug_image_nt(ph_ctx *ctx, size_t bytes) {
  if (!ctx) return fail(PH_E_INVALID, "ph_debug_image_nt: ctx is NULL");
  if (int rc = set_device(ctx)) return rc;
  return (int)ph::image_nt(bytes);
}

int ph_lut_query(ph_ctx *ctx, const void *dev, uint32_t *lds_bytes, uint32_t *toe, uint32_t *shift) {
  if (!ctx) return fail(PH_E_INVALID, "ph_lut_query: ctx is NULL");
  std::lock_guard<std::mutex> lock(ctx->mu);
  auto it = ctx->luts.find(dev);
  const bool have = it != ctx->luts.end();
  if (lds_bytes) *lds_bytes = have ? it->second.view.bytes : 0;
  if (toe) *toe = have ? (uint32_t)it->second.view.bias : 0;
  if (shift) *shift = have ? 23 - it->second.view.shift : 0;
  return PH_OK;
}

int ph_ctx_set_option(ph_ctx *ctx, const char *name, int value) {
  if (!ctx || !name) return fail(PH_E_INVALID, "ph_ctx_set_option: NULL argument");
  if (0 == strcmp(name, "lds_lut")) return ctx->use_lds_lut = (value != 0), PH_OK;
  if (0 == strcmp(name, "stream_images")) {
    if (value < 0 || value > 2) return fail(PH_E_INVALID, "stream_images: 0 (cached), 1 (streamed) or 2 (by size)");
    return ctx->stream_images = value, PH_OK;
  }
  if (0 == strcmp(name, "stream_threshold_mb")) {
    if (value < 0) return fail(PH_E_INVALID, "stream_threshold_mb: a size in MiB");
    return ctx->stream_threshold_mb = value, PH_OK;
  }
  if (0 == strcmp(name, "fail_launches")) return ctx->fail_launches.store(value), PH_OK;
  if (0 == strcmp(name, "chan_enlarged")) return ctx->chan_enlarged = (value < 0 || value > 2 ? 1 : value), PH_OK;  // 2: never the one-launch form (A/B, tests)
  if (0 == strcmp(name, "chan_batch_outs")) {
    if (value != 0 && value != 1) return fail(PH_E_INVALID, "chan_batch_outs: 0 (a launch per such job) or 1 (shared launches)");
    return ctx->chan_batch_outs = value, PH_OK;
  }
  if (0 == strcmp(name, "clip_batch")) {
    if (value != 0 && value != 1) return fail(PH_E_INVALID, "clip_batch: 0 (a launch per such job) or 1 (shared launches)");
    return ctx->clip_batch = value, PH_OK;
  }
  if (0 == strcmp(name, "up_v210_tails")) {
    if (value != 0 && value != 1) return fail(PH_E_INVALID, "up_v210_tails: 0 (a v210 output at width %% 48 != 0 is made on its own) or 1 (it stays in its table's launch)");
    return ctx->up_v210_tails = value, PH_OK;
  }
  if (0 == strcmp(name, "fused_multi_wgs")) {
    if (value < 0) return fail(PH_E_INVALID, "fused_multi_wgs: a number of workgroups, or 0 for no cap");
    return ctx->fused_multi_wgs = value, PH_OK;
  }
  if (0 == strcmp(name, "fused_multi_batch")) {
    if (value != 0 && value != 1) return fail(PH_E_INVALID, "fused_multi_batch: 0 (a launch per such job) or 1 (shared launches)");
    return ctx->fused_multi_batch = value, PH_OK;
  }
  if (0 == strcmp(name, "fused_fields")) {
    if (value != 0 && value != 1) return fail(PH_E_INVALID, "fused_fields: 0 (the plain-layer launches compose the whole frame) or 1 (only the field, where every output takes the same one)");
    return ctx->fused_fields = value, PH_OK;
  }
  if (0 == strcmp(name, "host_pool_mb")) {
    if (value < 0) return fail(PH_E_INVALID, "host_pool_mb: a size in MiB");
    std::vector<ph_ctx::HostBlock> drop;
    {
      std::lock_guard<std::mutex> lock(ctx->mu);
      ctx->host_pool_mb = value;
      ctx->host_peak_bytes = ctx->host_live_bytes;  // the working set is measured afresh from here (a burst long ago no longer sizes the pool)
      while (ctx->host_pooled_bytes > (size_t)value << 20 && !ctx->host_pool.empty()) {
        auto it = std::prev(ctx->host_pool.end());
        ctx->host_pooled_bytes -= it->first;
        drop.push_back(it->second);
        ctx->host_pool.erase(it);
      }
    }
    for (auto &v : drop) {
      hipHostFree(v.p);
      if (v.busy) hipEventDestroy(v.busy);
    }
    return PH_OK;
  }
  return fail(PH_E_INVALID, "unknown option '%s'", name);
}

// The compressed form of a device LUT pointer (unknown / plain / LDS path switched off: none).  A COPY, by value: the registry entry
// may be replaced by another thread once the lock is dropped, and a caller may hold its copy across any number of further look-ups
// (until round 6 this handed out slots of a 16-entry per-thread ring; a later launch once got the writer's table as its reader's).
struct LutRef {
  ph::LutView view{};
  bool found = false;
  float max_finite = __builtin_inff();  // (LutEntry's)
  const ph::LutView *get() const { return found ? &view : nullptr; }
};
static LutRef lds_view(ph_ctx *ctx, const void *dev) {
  LutRef r;
  if (!ctx || !ctx->use_lds_lut) return r;
  std::lock_guard<std::mutex> lock(ctx->mu);
  auto it = ctx->luts.find(dev);
  if (it == ctx->luts.end() || !it->second.view.bytes) return r;
  r.view = it->second.view, r.max_finite = it->second.max_finite, r.found = true;
  return r;
}

// a ph_buf used as `gammaLut`: (re)compress from its host mirror if new data went in
extern "C++" void refresh_buf_lut(ph_ctx *ctx, ph_buf *b) {
  if (b->lut_dirty && b->hptr && b->bytes >= 65536 * 4) {
    hipStreamSynchronize(ctx->streams[PH_QUEUE_LOAD]);  // the mirror must be stable
    ph_lut_register(ctx, b->dptr, (const float *)b->hptr);
    b->lut_dirty = false;
  }
}

// a format the channel kernel does not write (fmt_chan_out): the same answer from ph_chan_compose and from a program's outPacking
extern "C++" int chan_out_refused(const char *fn, int fmt) {
  return fail(PH_E_INVALID, "%s: the channel kernel does not write %s frames - run the separate kernels: the channel's frame as an image, then the format's writer (ph_pack_write)", fn,
              fmt_name(fmt));
}

// the "fail_launches" fault injection (tests of a binding's error paths: node/test/soak_run.js, tests/test_boundary_gpu.py): does this launch fail?
extern "C++" bool inject_failure(ph_ctx *ctx) {
  const int v = ctx->fail_launches.load();
  if (v > 0) return true;
  if (v < 0 && ctx->fail_launches.fetch_add(1) == -1) ctx->fail_launches.store(1);  // the last one that goes through
  return false;
}

// ---- typed entry points ------------------------------------------------------------------------
uint32_t ph_v210_pitch_bytes(uint32_t width) { return width ? ph::v210_pitch_bytes(width) : 0; }

#define PH_LAUNCH(expr)                                                                         \
  do {                                                                                          \
    if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", __func__);                           \
    PH_QUEUE(__func__, queue);                                                                  \
    int rc_ = set_device(ctx);                                                                  \
    if (rc_) return rc_;                                                                        \
    hipError_t e_ = ph::trace_launch(#expr) ? hipSuccess : (expr);                              \
    if (e_ != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", __func__, hipGetErrorString(e_)); \
    return PH_OK;                                                                               \
  } while (0)

int ph_v210_read(ph_ctx *ctx, int queue, const void *in, void *out, uint32_t width, uint32_t height, const void *cm,
                 const void *lut, const void *gm) {
  if (!in || !out || !cm || !lut || !gm || !width) return fail(PH_E_INVALID, "ph_v210_read: NULL/zero argument");
  if (!height) return PH_OK;
  if (ctx && width % 2 == 0) {  // (a tail of 2 or 4 pixels is the reference's: v210.ts:84-110; other widths: the general kernel)
    const LutRef lref = lds_view(ctx, lut);
    if (const ph::LutView *v = lref.get())
      PH_LAUNCH(ph::launch_v210_read_lds(stream_of(ctx, queue), in, out, width, height, cm, gm, *v,
                                         (uint32_t)ctx->props.multiProcessorCount));
  }
  PH_LAUNCH(ph::launch_v210_read(stream_of(ctx, queue), in, out, width, height, cm, lut, gm));
}

int ph_v210_read_batch(ph_ctx *ctx, int queue, int n, const void *const *ins, void *const *outs, uint32_t width,
                       uint32_t height, const void *cm, const void *lut, const void *gm) {
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_v210_read_batch: 1..%d frames", ph::kMaxLayers);
  if (!ins || !outs || !cm || !lut || !gm || !width) return fail(PH_E_INVALID, "ph_v210_read_batch: NULL/zero argument");
  for (int i = 0; i < n; ++i)
    if (!ins[i] || !outs[i]) return fail(PH_E_INVALID, "ph_v210_read_batch: frame %d is NULL", i);
  if (!height) return PH_OK;
  if (ctx && width % 2 == 0) {
    const LutRef lref = lds_view(ctx, lut);
    if (const ph::LutView *v = lref.get())
      PH_LAUNCH(ph::launch_v210_read_lds_batch(stream_of(ctx, queue), n, ins, outs, width, height, cm, gm, *v,
                                               (uint32_t)ctx->props.multiProcessorCount));
  }
  for (int i = 0; i < n; ++i) {  // table not LDS-resident / ragged width: one gather-kernel launch per frame
    const int rc = ph_v210_read(ctx, queue, ins[i], outs[i], width, height, cm, lut, gm);
    if (rc) return rc;
  }
  return PH_OK;
}

int ph_v210_write(ph_ctx *ctx, int queue, const void *in, void *out, uint32_t width, uint32_t height,
                  uint32_t interlace, const void *cm, const void *lut) {
  if (!in || !out || !cm || !lut || !width) return fail(PH_E_INVALID, "ph_v210_write: NULL/zero argument");
  if (interlace != 0 && interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "ph_v210_write: interlace must be 0, 1 or 3");
  if (!height) return PH_OK;
  if (ctx && width % 2 == 0) {
    const LutRef lref = lds_view(ctx, lut);
    if (const ph::LutView *v = lref.get())
      PH_LAUNCH(ph::launch_v210_write_lds(stream_of(ctx, queue), in, out, width, height, interlace, cm, *v,
                                          (uint32_t)ctx->props.multiProcessorCount));
  }
  PH_LAUNCH(ph::launch_v210_write(stream_of(ctx, queue), in, out, width, height, interlace, cm, lut));
}

int ph_fused_v210_combine(ph_ctx *ctx, int queue, int n, const void *const *layers, void *out, uint32_t width,
                          uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm,
                          const void *wr_cm, const void *wr_lut) {
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_fused_v210_combine: 1..%d layers", ph::kMaxLayers);
  if (!layers || !out || !rd_cm || !rd_lut || !rd_gm || !wr_cm || !wr_lut || !width)
    return fail(PH_E_INVALID, "ph_fused_v210_combine: NULL/zero argument");
  // (a width that is not a multiple of 48 - 1280 x 720, src/config.ts:43-54 - has lines that end in a tail quad and cleared slots:
  // the LDS kernel's TAIL instantiation; the reference's kernels serve tails of 2 or 4 pixels, v210.ts:84-110,166-193)
  const bool ragged = width % 48 != 0;
  if (width & 1) return fail(PH_E_INVALID, "ph_fused_v210_combine: width %u is odd; run the separate kernels", width);
  if (!height) return PH_OK;
  ph::FusedArgs a{};
  for (int i = 0; i < n; ++i) {
    if (!layers[i]) return fail(PH_E_INVALID, "ph_fused_v210_combine: layer %d is NULL", i);
    a.layers[i] = layers[i];
  }
  a.out = out;
  a.quads_per_line_used = width / 6;
  a.quads_per_line_pitch = ph::v210_pitch_bytes(width) / 16;
  a.total_quads = (ragged ? a.quads_per_line_pitch : a.quads_per_line_used) * height;
  a.tail_px = width % 6, a.magic_qpp = (uint32_t)(((1ull << 32) + a.quads_per_line_pitch - 1) / a.quads_per_line_pitch);
  if (ragged && (uint64_t)a.total_quads * a.quads_per_line_pitch >= (1ull << 32))  // the kernel's slot -> column division by reciprocal
    return fail(PH_E_INVALID, "ph_fused_v210_combine: a %u x %u frame with ragged lines is too large; run the separate kernels", width, height);
  a.rd_cm = (const float *)rd_cm, a.rd_lut = (const float *)rd_lut, a.rd_gm = (const float *)rd_gm;
  a.wr_cm = (const float *)wr_cm, a.wr_lut = (const float *)wr_lut;
  if (ctx) {
    const LutRef rref = lds_view(ctx, rd_lut), wref = lds_view(ctx, wr_lut);
    const ph::LutView *rv = rref.get(), *wv = wref.get();
    if (rv && wv) {
      const ph::FusedLdsArgs la = ph::fused_lds_args(a, *rv, *wv, rref.max_finite);
      PH_LAUNCH(ph::launch_fused_v210_combine_lds(stream_of(ctx, queue), n, la, (uint32_t)ctx->props.multiProcessorCount));
    }
  }
  PH_LAUNCH(ph::launch_fused_v210_combine(stream_of(ctx, queue), n, a));
}

int ph_pack_plane_bytes(int format, uint32_t width, uint32_t height, size_t bytes[3]) {
  if (!bytes || !width) return fail(PH_E_INVALID, "ph_pack_plane_bytes: NULL/zero argument");
  if (const int rc = even_dims("ph_pack_plane_bytes", format, width, height)) return rc;
  const int n = ph::pack_plane_bytes(format, width, height, bytes);
  return n < 0 ? fail(PH_E_INVALID, "ph_pack_plane_bytes: unknown format %d", format) : n;
}

int ph_fused_v210_combine_batch(ph_ctx *ctx, int queue, int jobs, int n, const void *const *layers, void *const *outs,
                                uint32_t width, uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm,
                                const void *wr_cm, const void *wr_lut) {
  if (jobs < 1 || jobs > ph::kMaxBatch) return fail(PH_E_INVALID, "ph_fused_v210_combine_batch: 1..%d jobs", ph::kMaxBatch);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_fused_v210_combine_batch: 1..%d layers", ph::kMaxLayers);
  if (!layers || !outs || !rd_cm || !rd_lut || !rd_gm || !wr_cm || !wr_lut)
    return fail(PH_E_INVALID, "ph_fused_v210_combine_batch: NULL argument");
  for (int j = 0; j < jobs; ++j) {
    if (!outs[j]) return fail(PH_E_INVALID, "ph_fused_v210_combine_batch: output %d is NULL", j);
    for (int l = 0; l < n; ++l)
      if (!layers[j * n + l]) return fail(PH_E_INVALID, "ph_fused_v210_combine_batch: job %d layer %d is NULL", j, l);
  }
  const LutRef rref = lds_view(ctx, rd_lut), wref = lds_view(ctx, wr_lut);  // (a NULL context has no tables)
  const ph::LutView *rv = rref.get(), *wv = wref.get();
  if (jobs == 1 || !rv || !wv || !width || width % 48 || !height) {
    // one job, or no LDS form of the tables: the plain entry point per job (same results)
    for (int j = 0; j < jobs; ++j) {
      int rc = ph_fused_v210_combine(ctx, queue, n, layers + (size_t)j * n, outs[j], width, height, rd_cm, rd_lut, rd_gm,
                                     wr_cm, wr_lut);
      if (rc != PH_OK) return rc;
    }
    return PH_OK;
  }
  ph::FusedArgs f{};
  for (int l = 0; l < n; ++l) f.layers[l] = layers[l];
  f.out = outs[0];
  f.quads_per_line_used = width / 6;
  f.quads_per_line_pitch = ph::v210_pitch_bytes(width) / 16;
  f.total_quads = f.quads_per_line_used * height;
  f.rd_cm = (const float *)rd_cm, f.rd_lut = (const float *)rd_lut, f.rd_gm = (const float *)rd_gm;
  f.wr_cm = (const float *)wr_cm, f.wr_lut = (const float *)wr_lut;
  ph::FusedLdsArgs la = ph::fused_lds_args(f, *rv, *wv, rref.max_finite);
  la.jobs = (uint32_t)jobs;
  for (int j = 1; j < jobs; ++j) {
    for (int l = 0; l < n; ++l) la.more_layers[j - 1][l] = layers[(size_t)j * n + l];
    la.more_out[j - 1] = outs[j];
  }
  PH_LAUNCH(ph::launch_fused_v210_combine_lds(stream_of(ctx, queue), n, la, (uint32_t)ctx->props.multiProcessorCount));
}

int ph_pack_read(ph_ctx *ctx, int queue, int format, const void *const planes[3], void *out, uint32_t width,
                 uint32_t height, const void *cm, const void *lut, const void *gm) {
  if (!ctx || !planes || !out || !lut || !gm || !width) return fail(PH_E_INVALID, "ph_pack_read: NULL/zero argument");
  if (format == PH_FMT_V210) return ph_v210_read(ctx, queue, planes[0], out, width, height, cm, lut, gm);
  if (const int rc = even_dims("ph_pack_read", format, width, height)) return rc;
  size_t pb[3];
  const int np = ph::pack_plane_bytes(format, width, height, pb);
  if (np < 0) return fail(PH_E_INVALID, "ph_pack_read: unknown format %d", format);
  for (int i = 0; i < np; ++i)
    if (!planes[i]) return fail(PH_E_INVALID, "ph_pack_read: plane %d is NULL", i);
  if (!fmt_rgb8(format) && !cm) return fail(PH_E_INVALID, "ph_pack_read: YCbCr formats need a colMatrix");
  if (!height) return PH_OK;
  PH_LAUNCH(ph::launch_pack_read(stream_of(ctx, queue), format, planes, out, width, height, cm, lut, gm, lds_view(ctx, lut).get(),
                                 (uint32_t)ctx->props.multiProcessorCount));
}

int ph_pack_read_batch(ph_ctx *ctx, int queue, int format, int n, const void *const (*planes)[3], void *const *outs, uint32_t width, uint32_t height,
                       const void *cm, const void *lut, const void *gm) {
  if (!ctx || !planes || !outs || !lut || !gm || !width) return fail(PH_E_INVALID, "ph_pack_read_batch: NULL/zero argument");
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_pack_read_batch: 1..%d frames", ph::kMaxLayers);
  if (const int rc = even_dims("ph_pack_read_batch", format, width, height)) return rc;
  const LutRef lref = lds_view(ctx, lut);
  const ph::LutView *v = format == PH_FMT_V210 ? nullptr : lref.get();
  if (n == 1 || !v) {  // one frame, v210 (its own batch call), or no LDS form of the table: frame by frame
    if (format == PH_FMT_V210) {
      const void *ins[ph::kMaxLayers];
      for (int i = 0; i < n; ++i) ins[i] = planes[i][0];
      return ph_v210_read_batch(ctx, queue, n, ins, outs, width, height, cm, lut, gm);
    }
    for (int i = 0; i < n; ++i) {
      const int rc = ph_pack_read(ctx, queue, format, planes[i], outs[i], width, height, cm, lut, gm);
      if (rc) return rc;
    }
    return PH_OK;
  }
  size_t pb[3];
  const int np = ph::pack_plane_bytes(format, width, height, pb);
  if (np < 0) return fail(PH_E_INVALID, "ph_pack_read_batch: unknown format %d", format);
  for (int i = 0; i < n; ++i) {
    if (!outs[i]) return fail(PH_E_INVALID, "ph_pack_read_batch: output %d is NULL", i);
    for (int k = 0; k < np; ++k)
      if (!planes[i][k]) return fail(PH_E_INVALID, "ph_pack_read_batch: frame %d: plane %d is NULL", i, k);
  }
  if (!fmt_rgb8(format) && !cm) return fail(PH_E_INVALID, "ph_pack_read_batch: YCbCr formats need a colMatrix");
  if (!height) return PH_OK;
  PH_LAUNCH(ph::launch_pack_read_batch(stream_of(ctx, queue), format, n, planes, outs, width, height, cm, gm, *v, (uint32_t)ctx->props.multiProcessorCount));
}

int ph_pack_write(ph_ctx *ctx, int queue, int format, const void *in, void *const planes[3], uint32_t width,
                  uint32_t height, uint32_t interlace, const void *cm, const void *lut) {
  if (!ctx || !planes || !in || !lut || !width) return fail(PH_E_INVALID, "ph_pack_write: NULL/zero argument");
  if (interlace != 0 && interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "ph_pack_write: interlace must be 0, 1 or 3");
  if (format == PH_FMT_V210) return ph_v210_write(ctx, queue, in, planes[0], width, height, interlace, cm, lut);
  if (const int rc = even_dims("ph_pack_write", format, width, height)) return rc;
  size_t pb[3];
  const int np = ph::pack_plane_bytes(format, width, height, pb);
  if (np < 0) return fail(PH_E_INVALID, "ph_pack_write: unknown format %d", format);
  for (int i = 0; i < np; ++i)
    if (!planes[i]) return fail(PH_E_INVALID, "ph_pack_write: plane %d is NULL", i);
  if (!fmt_rgb8(format) && !cm) return fail(PH_E_INVALID, "ph_pack_write: YCbCr formats need a colMatrix");
  if (!height) return PH_OK;
  PH_LAUNCH(ph::launch_pack_write(stream_of(ctx, queue), format, in, planes, width, height, interlace, cm, lut,
                                  lds_view(ctx, lut).get(), (uint32_t)ctx->props.multiProcessorCount));
}

// The outputs grouped by writer table, in the order the tables first appear - THE walk every several-outputs entry makes.  order (n_out
// entries): the outputs' indices group by group, a group's members in the call's order; group g is order[start[g]] .. order[start[g + 1] - 1]
// (start: n_out + 1 entries), and its first member is the first output that names its table.  Answers the number of groups
static int writer_table_groups(int n_out, const ph_chan_output *outs, int *order, int *start) {
  int placed = 0, groups = 0;
  for (int k = 0; k < n_out; ++k) {
    bool seen = false;
    for (int j = 0; j < k; ++j) seen = seen || outs[j].wr_gamma_lut == outs[k].wr_gamma_lut;
    if (seen) continue;
    start[groups++] = placed;
    for (int j = k; j < n_out; ++j)
      if (outs[j].wr_gamma_lut == outs[k].wr_gamma_lut) order[placed++] = j;
  }
  start[groups] = placed;
  return groups;
}

/* One image packed for several consumers: see include/phaneron_hip.h.  Every check is ph_pack_write's, per output, and is made - and every
 * launch of the call planned - before anything is launched. */
int ph_pack_write_multi(ph_ctx *ctx, int queue, const void *in, int n_out, const ph_chan_output *outs, uint32_t width, uint32_t height) {
  const char *const fn = "ph_pack_write_multi";
  if (!ctx || !in || !outs || !width) return fail(PH_E_INVALID, "%s: NULL/zero argument", fn);
  if (n_out < 1 || n_out > ph::kMaxPackOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxPackOuts, n_out);
  if (n_out == 1)
    return ph_pack_write(ctx, queue, outs[0].format, in, outs[0].planes, width, height, outs[0].interlace, outs[0].wr_col_matrix12, outs[0].wr_gamma_lut);
  PH_QUEUE(fn, queue);
  for (int k = 0; k < n_out; ++k) {
    const ph_chan_output &o = outs[k];
    if (!o.wr_gamma_lut) return fail(PH_E_INVALID, "%s: output %d: the writer's gamma LUT is missing", fn, k);
    if (!fmt_known(o.format)) return fail(PH_E_INVALID, "%s: output %d: unknown format %d", fn, k, o.format);
    if (o.interlace != 0 && o.interlace != 1 && o.interlace != 3) return fail(PH_E_INVALID, "%s: output %d: interlace must be 0, 1 or 3", fn, k);
    if (const int rc = even_dims(fn, o.format, width, height)) return rc;
    for (int i = 0; i < fmt_planes(o.format); ++i)
      if (!o.planes[i]) return fail(PH_E_INVALID, "%s: output %d: plane %d is NULL", fn, k, i);
    if (!fmt_rgb8(o.format) && !o.wr_col_matrix12) return fail(PH_E_INVALID, "%s: output %d: YCbCr formats need a colMatrix", fn, k);
    for (int j = 0; j < k; ++j)
      if (outs[j].planes[0] == o.planes[0]) return fail(PH_E_INVALID, "%s: outputs %d and %d name the same plane", fn, j, k);
  }
  if (!height) return PH_OK;
  // the launches: per writer table, in the order the tables first appear - the outputs the shared kernel does not take (and an output that
  // would be alone in it) through ph_pack_write, in their order, then the others as one shared launch
  struct Launch {
    int solo;  // >= 0: outs[solo] through ph_pack_write
    ph::PackMultiArgs m;
  };
  std::vector<Launch> launches;
  int order[ph::kMaxPackOuts], start[ph::kMaxPackOuts + 1];
  const int groups = writer_table_groups(n_out, outs, order, start);
  for (int t = 0; t < groups; ++t) {
    const int *const group = order + start[t], members = start[t + 1] - start[t];
    const LutRef wref = lds_view(ctx, outs[group[0]].wr_gamma_lut);
    int share = 0;
    bool shared_ok[ph::kMaxPackOuts];
    for (int g = 0; g < members; ++g) {
      const int f = outs[group[g]].format;
      shared_ok[g] = wref.get() && !(f == PH_FMT_V210 && width % 48) && !(fmt_planar(f) && width % 8);
      share += shared_ok[g] ? 1 : 0;
    }
    Launch shared{};
    shared.solo = -1;
    for (int g = 0; g < members; ++g) {
      const ph_chan_output &o = outs[group[g]];
      if (!shared_ok[g] || share < 2) {
        Launch own{};
        own.solo = group[g];
        launches.push_back(own);
        continue;
      }
      ph::PackOut &d = shared.m.out[shared.m.n_out++];
      d.fmt = (uint32_t)o.format;
      d.pitch = o.format == PH_FMT_V210 ? width / 6u : ph::pack_pitch(o.format, width);  // (v210 here: a multiple of 48, no padding)
      d.wr_cm = fmt_rgb8(o.format) ? nullptr : (const float *)o.wr_col_matrix12;
      for (int i = 0; i < 3; ++i) d.plane[i] = i < fmt_planes(o.format) ? o.planes[i] : nullptr;
      d.takes = o.interlace;  // (settled below, once the launch's lines are known)
    }
    if (!shared.m.n_out) continue;
    ph::PackMultiArgs &m = shared.m;
    const uint32_t first_il = m.out[0].takes;
    bool same_lines = true;
    for (uint32_t i = 0; i < m.n_out; ++i) same_lines = same_lines && m.out[i].takes == first_il;
    const uint32_t il = same_lines ? first_il : 0u;
    m.in = in, m.width = width, m.wr = *wref.get();
    m.line_step = il ? 2 : 1, m.first_line = il == 3 ? 1 : 0, m.lines = il ? height / 2 : height;
    for (uint32_t i = 0; i < m.n_out; ++i) {
      ph::PackOut &d = m.out[i];
      const uint32_t oil = d.takes;
      d.takes = same_lines || !oil ? 0u : oil == 1 ? 1u : 2u;
      // a field: height / 2 lines; a 4:2:0 frame: its line pairs (an odd height leaves the last line alone, as ph_pack_write does)
      d.line_end = oil || fmt_v420((int)d.fmt) ? 2u * (height / 2u) : height;
      d.field = oil ? 1u : 0u;
    }
    launches.push_back(shared);
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  for (const Launch &l : launches) {
    if (l.solo >= 0) {
      const ph_chan_output &o = outs[l.solo];
      if ((rc = ph_pack_write(ctx, queue, o.format, in, o.planes, width, height, o.interlace, o.wr_col_matrix12, o.wr_gamma_lut))) return rc;
      continue;
    }
    const hipError_t e = ph::launch_pack_write_multi(stream_of(ctx, queue), l.m, (uint32_t)ctx->props.multiProcessorCount);
    if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  }
  return PH_OK;
}

static int compose_write(ph_ctx *ctx, int queue, int n, const ph_layer *layers, const ph_layer_wipe *wipes, void *out, uint32_t out_w,
                         uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut);

int ph_compose_write_v210(ph_ctx *ctx, int queue, int n, const ph_layer *layers, void *out, uint32_t out_w,
                          uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  return compose_write(ctx, queue, n, layers, nullptr, out, out_w, out_h, interlace, wr_cm, wr_lut);
}

int ph_compose_wipe_write_v210(ph_ctx *ctx, int queue, int n, const ph_layer *layers, const ph_layer_wipe *wipes, void *out,
                               uint32_t out_w, uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  if (!wipes) return fail(PH_E_INVALID, "ph_compose_wipe_write_v210: NULL argument");
  return compose_write(ctx, queue, n, layers, wipes, out, out_w, out_h, interlace, wr_cm, wr_lut);
}

static int compose_write(ph_ctx *ctx, int queue, int n, const ph_layer *layers, const ph_layer_wipe *wipes, void *out, uint32_t out_w,
                         uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  if (!ctx || !layers || !out || !wr_cm || !wr_lut) return fail(PH_E_INVALID, "ph_compose_write_v210: NULL argument");
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_compose_write_v210: 1..%d layers", ph::kMaxLayers);
  // (a width that is not a multiple of 48 - 1280 x 720 - goes to the quad-per-lane kernel, which writes the reference's tail quad
  // and cleared slots, v210.ts:131-136,166-193; the reference's writer serves tails of 2 or 4 pixels)
  if (!out_w || (out_w & 1)) return fail(PH_E_INVALID, "ph_compose_write_v210: width %u is zero or odd; run the separate kernels", out_w);
  if (interlace != 0 && interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "ph_compose_write_v210: interlace must be 0, 1 or 3");
  const LutRef wref = lds_view(ctx, wr_lut);
  const ph::LutView *wv = wref.get();
  if (!wv) return fail(PH_E_INVALID, "ph_compose_write_v210: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)");
  ph::ComposeArgs a{};
  a.n = n;
  for (int i = 0; i < n; ++i) {
    if (!layers[i].rgba || layers[i].width <= 0 || layers[i].height <= 0)
      return fail(PH_E_INVALID, "ph_compose_write_v210: layer %d is empty", i);
    if (!layers[i].matrix9 && ((uint32_t)layers[i].width != out_w || (uint32_t)layers[i].height != out_h))
      return fail(PH_E_INVALID, "ph_compose_write_v210: layer %d has no transform but is %dx%d, not the output size", i,
                  layers[i].width, layers[i].height);
    a.layers[i] = layers[i].rgba, a.matrix[i] = (const float *)layers[i].matrix9;
    a.lw[i] = layers[i].width, a.lh[i] = layers[i].height;
    if (wipes && (wipes[i].incoming_rgba || wipes[i].mask_rgba)) {
      if (!wipes[i].incoming_rgba || !wipes[i].mask_rgba)
        return fail(PH_E_INVALID, "ph_compose_wipe_write_v210: layer %d needs both the incoming image and the mask", i);
      a.wipe_with[i] = wipes[i].incoming_rgba, a.wipe_mask[i] = wipes[i].mask_rgba;
    }
  }
  a.out = out, a.out_w = out_w, a.out_h = out_h;
  a.wr = *wv;  // the path choice depends on the table's size
  bool any_wipe = false;  // a wipes array without a single entry set is the plain compositor (the header: such entries leave the layer alone)
  for (int i = 0; i < n; ++i) any_wipe = any_wipe || a.wipe_with[i] != nullptr;
  if (any_wipe && !ph::compose_can_wipe(a))
    return fail(PH_E_INVALID, "ph_compose_wipe_write_v210: needs out_width %% 192 == 0, source images below 2 GiB and a writer table that leaves "
                              "the staging area free in LDS; run the separate kernels");
  a.line_step = interlace ? 2 : 1, a.first_line = (interlace == 3) ? 1 : 0;
  a.lines = interlace ? out_h / 2 : out_h;
  a.wr_cm = (const float *)wr_cm, a.wr = *wv;
  if (!a.lines) return PH_OK;
  PH_LAUNCH(ph::launch_compose_write_v210(stream_of(ctx, queue), a, (uint32_t)ctx->props.multiProcessorCount));
}

static int chan_source(const ph_chan_source &s, const char *what, int layer, uint32_t out_w, uint32_t out_h, ph::ChanSrc *o, const void **pu,
                       const void **pv, const float **cm, uint32_t *planar) {
  if (!s.data || s.width <= 0 || s.height <= 0)
    return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s is empty", layer, what);
  const int fmt = fmt_of_src(s.format);
  const bool is_planar = fmt_planar(fmt), is_rgb8 = fmt_rgb8(fmt);
  if (fmt < 0 && s.format != PH_SRC_RGBA_F32)
    return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s has format %d (not a PH_SRC_*)", layer, what, s.format);
  *pu = *pv = nullptr, *cm = nullptr;
  if (is_rgb8) *planar = 2;  // (served by the kernel's wire-format instantiation)
  if (is_planar) {
    if (!s.data_u || (fmt_planes(fmt) == 3 && !s.data_v) || (s.width & 1) || (fmt_v420(fmt) && (s.height & 1)))
      return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s is a %s frame (planar): it needs its chroma plane(s), an even width and, for 4:2:0, an even height (%dx%d)", layer,
                  what, fmt_name(fmt), s.width, s.height);
    *pu = s.data_u, *pv = s.data_v, *cm = (const float *)s.col_matrix12, *planar = 2;
  }
  // (the reference's v210 reader serves tails of 2 or 4 pixels: v210.ts:84-110)
  if (s.format == PH_SRC_V210 && (s.width & 1))
    return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s is a v210 frame %d wide, an odd width; run the separate kernels", layer, what, s.width);
  if (s.format == PH_SRC_V210 && s.width % 6 && *planar < 1) *planar = 1;  // a line with a tail: the kernel's instantiation for those
  if (!s.matrix9_host && ((uint32_t)s.width != out_w || (uint32_t)s.height != out_h))
    return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s has no transform but is %dx%d, not the output size", layer, what, s.width, s.height);
  o->ptr = s.data, o->w = (uint32_t)s.width, o->h = (uint32_t)s.height;
  static const uint32_t kinds[] = {ph::kChanNone, ph::kChanV210,  ph::kChanRgba,  ph::kChanP10,     ph::kChanP8x422, ph::kChanP8x420,
                                   ph::kChanNv12, ph::kChanRgba8, ph::kChanBgra8, ph::kChanP10x420, ph::kChanP010};  // [PH_SRC_*]
  o->kind = kinds[s.format];
  // the line of the frame's first plane (planar: the Y plane), or of an f32 image
  o->pitch = s.format == PH_SRC_V210 ? ph_v210_pitch_bytes((uint32_t)s.width)
             : fmt >= 0 ? pack_pitch(fmt, (uint32_t)s.width) * fmt_sample_bytes(fmt) : (uint32_t)s.width * 16u;
  if ((uint64_t)o->pitch * o->h >= (1ull << 30))
    return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: the %s is 1 GiB or larger; run the separate kernels", layer, what);
  o->sampled = s.matrix9_host ? 1u : 0u;
  o->tail_from = (uint32_t)s.width - (uint32_t)s.width % 6u;
  for (int i = 0; i < 6; ++i) o->m[i] = s.matrix9_host ? s.matrix9_host[i] : 0.0f;
  return PH_OK;
}

// PH_CHAN_BATCH=0: every job of a batch call through the one-job kernel (A/B runs, tools/chan_bench.py)
static bool chan_batch_on() {
  static const bool on = !(getenv("PH_CHAN_BATCH") && getenv("PH_CHAN_BATCH")[0] == '0');
  return on;
}
// the index frames between the phases: one area per queue (launches on one queue are in order), grown on demand (ctx->mu held)
static int chan_index_reserve(ph_ctx *ctx, int queue, size_t need) {
  if (ctx->chan_index_bytes[queue] >= need) return PH_OK;
  if (ctx->chan_index[queue]) {
    hipStreamSynchronize(ctx->streams[queue]);
    hipFree(ctx->chan_index[queue]);
    ctx->chan_index[queue] = nullptr, ctx->chan_index_bytes[queue] = 0;
  }
  PH_HIP(hipMalloc(&ctx->chan_index[queue], need));
  ctx->chan_index_bytes[queue] = need;
  return PH_OK;
}
// One launch that uses the queue's area: the area is held until the launch is enqueued, so the launches of two calls on one queue do not
// interleave around it.  launch(stream, area) enqueues; what it answers is fn's "launch failed"
extern "C++" template <class Launch>
static int with_scratch(const char *fn, ph_ctx *ctx, int queue, size_t bytes, Launch launch) {
  const hipStream_t s = stream_of(ctx, queue);
  std::lock_guard<std::mutex> scratch(ctx->chan_scratch_mu[queue]);
  void *area = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (const int rc = chan_index_reserve(ctx, queue, bytes)) return rc;
    area = ctx->chan_index[queue];
  }
  const hipError_t e = launch(s, area);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return PH_OK;
}
// one launch of the batch kernel: b holds the jobs and their ops, g the geometry, colour recipe and tables (set_device done)
static int chan_batch_launch(ph_ctx *ctx, int queue, ph::ChanBatchArgs &b, const ph::ChanArgs &g) {
  b.out_w = g.out_w, b.out_h = g.out_h, b.lines = g.lines, b.line_step = g.line_step;
  b.rd_cm = g.rd_cm, b.rd_gm = g.rd_gm, b.wr_cm = g.wr_cm, b.rd = g.rd, b.wr = g.wr;
  b.tails = g.planar >= 1 ? 1u : 0u, b.planar = g.planar == 2 ? 1u : 0u, b.out_qpitch = g.out_qpitch, b.out_tail_from = g.out_tail_from;
  const size_t each = (ph::chan_index_bytes(g.out_w, g.lines) + 255u) & ~(size_t)255u;
  return with_scratch("ph_chan_compose_batch", ctx, queue, each * b.jobs, [&](hipStream_t s, void *area) {
    for (uint32_t j = 0; j < b.jobs; ++j) b.job[j].index = (char *)area + each * j;
    return ph::launch_chan_compose_batch(s, b, (uint32_t)ctx->props.multiProcessorCount);
  });
}

// a channel's layers as the kernel's flat program: one op per source to sample (ph_kernels.h ChanOp)
static int chan_ops(int n, const ph_chan_layer *layers, uint32_t out_w, uint32_t out_h, ph::ChanOp *op, const void **plane_u, const void **plane_v,
                    const float **cm_op, uint32_t *planar, int *n_ops) {
  int k = 0;
  for (int i = 0; i < n; ++i) {
    const ph_chan_layer &L = layers[i];
    const uint32_t first = i == 0 ? ph::kChanActFirst : 0u;
    int rc = chan_source(L.src, "source", i, out_w, out_h, &op[k].src, &plane_u[k], &plane_v[k], &cm_op[k], planar);
    if (rc) return rc;
    if (L.transition == PH_TRANSITION_CUT) {
      op[k++].action = ph::kChanActLayer | first;
    } else if (L.transition == PH_TRANSITION_DISSOLVE || L.transition == PH_TRANSITION_WIPE) {
      op[k++].action = ph::kChanActHold;
      rc = chan_source(L.incoming, "transition's incoming source", i, out_w, out_h, &op[k].src, &plane_u[k], &plane_v[k], &cm_op[k], planar);
      if (rc) return rc;
      if (L.transition == PH_TRANSITION_DISSOLVE) {
        op[k].mix = L.mix;
        op[k++].action = ph::kChanActDissolve | first;
      } else {
        op[k++].action = ph::kChanActIncoming;
        rc = chan_source(L.mask, "wipe's mask", i, out_w, out_h, &op[k].src, &plane_u[k], &plane_v[k], &cm_op[k], planar);
        if (rc) return rc;
        op[k++].action = ph::kChanActWipe | first;
      }
    } else {
      return fail(PH_E_INVALID, "ph_chan_compose_v210: layer %d: transition %d", i, L.transition);
    }
  }
  *n_ops = k;
  return PH_OK;
}

// ---- a frame of ENLARGED clips: read once, then the 2 x 2-block compositor --------------------------------------------------------------
// The reference uploads a clip at its own size and lets the Mixer's transform fill the channel (src/producer/ffmpegProducer.ts:395-442,
// mixer.ts:189-228): a 720p or SD clip on a 1080 channel, an HD clip on a 2160p one.  The channel kernel converts every TAP - four
// conversions per output pixel - where an enlarged clip has fewer pixels than the frame it fills.  When every layer of a frame is such a
// clip (v210 or a decoder's planar / packed-RGB frame, no transition, placed without rotation or mirroring, under 0.99 source texels per output pixel and written row: what
// ph_compose_up_write_v210 takes), the frame is made by the kernels that exist for exactly this: ph_v210_read(_batch) / ph_pack_read into scratch images,
// one conversion per SOURCE pixel, then ph_compose_up_write_v210 on them.  Same arithmetic, same bits (tests/test_chan_gpu.py checks both
// routes against the chain of the reference's operators); 1280 x 720 -> 1920 x 1080: 26.4 -> 17.7 us, 1080p -> 2160p: 82 -> 38 us (tools/enlarge_bench.py).
// Context option "chan_enlarged" = 0 (or PH_CHAN_ENLARGED=0): such frames through the channel kernel like any other (A/B runs, tests of that path).
// v210_fill: v210 frames under the default fill count too - only worth it when several channels' frames of one shape share the launches
// (one alone: 22.3 us by the channel kernel against 23.5; four to a call 18.7 against 15.6): ph_chan_compose_batch asks that way
// one image - a layer's src, or a transition's incoming image or mask (ph_clip_compose_transition_multi asks per image)
static bool chan_image_enlarged(const ph_chan_source &S, uint32_t out_w, uint32_t out_h, uint32_t interlace, bool v210_fill) {
  const float *m = S.matrix9_host;
  // (v210 frames, a file decoder's planar frames, packed 8-bit RGB: whatever has a reader of its own - ph_v210_read, ph_pack_read)
  // - and finished f32 images, which the compositor takes as they are
  const int fmt = fmt_of_src(S.format);
  if ((fmt < 0 && S.format != PH_SRC_RGBA_F32) || !m || S.width <= 0 || S.height <= 0 || ((S.width & 1) && !fmt_rgb8(fmt) && S.format != PH_SRC_RGBA_F32))
    return false;
  if (m[1] != 0.0f || m[3] != 0.0f || !(m[0] > 0.0f) || !(m[4] > 0.0f)) return false;                      // (ph_kernels_up.hip compose_up_eligible)
  // ... or a decoder's frame of the channel's size under the Mixer's default fill (the compositor takes exactly that placement beside the
  // enlargements: compose_up_eligible): a 1080p yuv420p clip 26.1 -> 22.6 us, under a bgra8 graphic 45.2 -> 40.2.  Not v210 frames: the channel
  // kernel's shared taps serve those better (22.3 against 23.2 us)
  const bool fill = (v210_fill || S.format != PH_SRC_V210) && !interlace && (uint32_t)S.width == out_w && (uint32_t)S.height == out_h && m[0] == 1.0f && m[4] == 1.0f &&
                    m[2] == 0.0f && m[5] == 0.0f;
  if (!fill && ((double)m[0] * S.width > 0.99 * out_w || (double)m[4] * S.height * (interlace ? 2 : 1) > 0.99 * out_h)) return false;
  if ((uint64_t)S.width * 16u * (uint64_t)S.height >= (1ull << 30) || S.width >= (1 << 22)) return false;
  return true;
}
static bool chan_layers_enlarged(int n, const ph_chan_layer *layers, uint32_t out_w, uint32_t out_h, uint32_t interlace, bool v210_fill = false) {
  if (out_w % 2u) return false;
  for (int i = 0; i < n; ++i)
    if (layers[i].transition != PH_TRANSITION_CUT || !chan_image_enlarged(layers[i].src, out_w, out_h, interlace, v210_fill)) return false;
  return true;
}
// two such frames of one shape (layer count, clip sizes, placements): one launch of the compositor can make both
static bool chan_enlarged_same_shape(int n, const ph_chan_layer *a, const ph_chan_layer *b) {
  for (int i = 0; i < n; ++i) {
    if (a[i].src.width != b[i].src.width || a[i].src.height != b[i].src.height) return false;
    for (int k = 0; k < 9; ++k)
      if (a[i].src.matrix9_host[k] != b[i].src.matrix9_host[k]) return false;
  }
  return true;
}
// The reading half of the two-stage route, for `jobs` frames of one shape: every clip through its format's reader - as few launches as
// their sizes allow - into the queue's scratch images (finished f32 images are taken as they are).  The caller holds
// ctx->chan_scratch_mu[queue], and keeps it until its compositor launch is enqueued.
// The images are given as a flat list, srcs[j * n + i]: image i of job j (n: up to kMaxUpJobs * kMaxLayers / jobs - a frame in a transition
// brings its partners as further images); imgs[j * n + i]: where the compositor finds it.
static int chan_images_read(ph_ctx *ctx, int queue, int jobs, int n, const ph_chan_source *const *srcs, const void *rd_cm, const void *rd_lut, const void *rd_gm,
                            void **imgs) {
  // the images live in the channel compositor's scratch area of the queue (launches on one queue are in order)
  size_t off[ph::kMaxUpJobs * ph::kMaxLayers], per_job = 0;
  bool one_size = true;
  for (int i = 0; i < n; ++i) {
    off[i] = per_job;
    per_job += ((size_t)srcs[i]->width * srcs[i]->height * 16u + 255u) & ~(size_t)255u;
    one_size = one_size && srcs[i]->width == srcs[0]->width && srcs[i]->height == srcs[0]->height;
  }
  const size_t total = per_job * (size_t)jobs;
  // Three sets of images taken in turn: a frame's read kernel overwriting the very lines the previous frame's compositor has just read
  // (still cached, in several XCDs' L2s) measured 11.7 us against 7.9 us into lines nobody holds (tools/enlarge_bench.py, PH_ENLARGE_RING)
  // - while the sets together stay inside the 256 MB of last-level cache: four 1080p images (132 MB) in three sets measured 109 us per
  // 2160p frame against 94 in one set that stays cached
  const unsigned kTurns = total <= ((size_t)64 << 20) ? 3u : 1u;
  char *base;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    int rc = chan_index_reserve(ctx, queue, total * kTurns);
    if (rc) return rc;
    base = (char *)ctx->chan_index[queue] + total * (ctx->chan_scratch_turn[queue]++ % kTurns);
  }
  const void *ins[ph::kMaxUpJobs * ph::kMaxLayers];
  for (int j = 0; j < jobs; ++j) {
    for (int i = 0; i < n; ++i) {
      const ph_chan_source &S = *srcs[j * n + i];
      ins[j * n + i] = S.data, imgs[j * n + i] = S.format == PH_SRC_RGBA_F32 ? const_cast<void *>(S.data) : base + per_job * (size_t)j + off[i];
    }
  }
  int rc = PH_OK;
  const int frames = jobs * n;
  bool all_v210 = true;
  for (int f = 0; f < frames; ++f) all_v210 = all_v210 && srcs[f]->format == PH_SRC_V210;
  bool one_reader = !all_v210 && one_size && frames > 1;  // every frame a decoder's frame of ONE format, size and Loader matrix: one launch reads them all
  for (int f = 0; f < frames && one_reader; ++f) {
    const ph_chan_source &S = *srcs[f], &S0 = *srcs[0];
    one_reader = S.format == S0.format && fmt_of_src(S.format) > PH_FMT_V210 && S.col_matrix12 == S0.col_matrix12;
  }
  if (one_reader) {
    const void *planes[ph::kMaxUpJobs * ph::kMaxLayers][3];
    for (int f = 0; f < frames; ++f) {
      const ph_chan_source &S = *srcs[f];
      planes[f][0] = S.data, planes[f][1] = S.data_u, planes[f][2] = S.data_v;
    }
    const ph_chan_source &S0 = *srcs[0];
    for (int f = 0; f < frames && rc == PH_OK; f += ph::kMaxLayers)
      rc = ph_pack_read_batch(ctx, queue, fmt_of_src(S0.format), frames - f < ph::kMaxLayers ? frames - f : ph::kMaxLayers, planes + f, imgs + f,
                              (uint32_t)S0.width, (uint32_t)S0.height, S0.col_matrix12 ? S0.col_matrix12 : rd_cm, rd_lut, rd_gm);
  } else if (!all_v210) {  // each clip through the reader of its format (a source with code ranges of its own brings its Loader matrix)
    for (int f = 0; f < frames && rc == PH_OK; ++f) {
      const ph_chan_source &S = *srcs[f];
      if (S.format == PH_SRC_RGBA_F32) continue;  // an image: nothing to read
      if (S.format == PH_SRC_V210) {
        rc = ph_v210_read(ctx, queue, S.data, imgs[f], (uint32_t)S.width, (uint32_t)S.height, rd_cm, rd_lut, rd_gm);
      } else {
        const void *planes[3] = {S.data, S.data_u, S.data_v};
        rc = ph_pack_read(ctx, queue, fmt_of_src(S.format), planes, imgs[f], (uint32_t)S.width, (uint32_t)S.height,
                          S.col_matrix12 ? S.col_matrix12 : rd_cm, rd_lut, rd_gm);
      }
    }
  } else if (one_size && frames > 1) {
    for (int f = 0; f < frames && rc == PH_OK; f += ph::kMaxLayers)
      rc = ph_v210_read_batch(ctx, queue, frames - f < ph::kMaxLayers ? frames - f : ph::kMaxLayers, ins + f, imgs + f, (uint32_t)srcs[0]->width,
                              (uint32_t)srcs[0]->height, rd_cm, rd_lut, rd_gm);
  } else {
    for (int f = 0; f < frames && rc == PH_OK; ++f)
      rc = ph_v210_read(ctx, queue, ins[f], imgs[f], (uint32_t)srcs[f]->width, (uint32_t)srcs[f]->height, rd_cm, rd_lut, rd_gm);
  }
  return rc;
}
// every layer's src of `jobs` frames of one shape; il / sets: the images as the 2 x 2-block compositor's entries take them
static int chan_enlarged_read(ph_ctx *ctx, int queue, int jobs, int n, const ph_chan_layer *const *layers, const void *rd_cm, const void *rd_lut, const void *rd_gm,
                              ph_image_layer (*il)[ph::kMaxLayers], const ph_image_layer **sets) {
  const ph_chan_source *srcs[ph::kMaxUpJobs * ph::kMaxLayers];
  void *imgs[ph::kMaxUpJobs * ph::kMaxLayers];
  for (int j = 0; j < jobs; ++j)
    for (int i = 0; i < n; ++i) srcs[j * n + i] = &layers[j][i].src;
  const int rc = chan_images_read(ctx, queue, jobs, n, srcs, rd_cm, rd_lut, rd_gm, imgs);
  if (rc) return rc;
  for (int j = 0; j < jobs; ++j) {
    for (int i = 0; i < n; ++i) {
      const ph_chan_source &S = layers[j][i].src;
      il[j][i] = ph_image_layer{imgs[j * n + i], PH_IMG_RGBA_F32, S.width, S.height, S.matrix9_host};
    }
    sets[j] = il[j];
  }
  return PH_OK;
}
// `jobs` frames of one shape and field mode (1 .. kMaxUpJobs, different outputs): the clips read - as few launches as their sizes allow -
// and ONE compositor launch (ph_compose_up_write_v210_batch)
static int chan_compose_enlarged(ph_ctx *ctx, int queue, int jobs, int n, const ph_chan_layer *const *layers, void *const *outs, uint32_t out_w, uint32_t out_h,
                                 uint32_t interlace, const void *rd_cm, const void *rd_lut, const void *rd_gm, const void *wr_cm, const void *wr_lut) {
  // ONE frame whose layers are all clips in their wire formats: reader and compositor in one launch (ph_kernels_up.hip clip_up_write_v210_kernel) -
  // no image leaves the chip.  (Several frames of one shape: the batched reads + one compositor launch below.)
  // Measured (tools/enlarge_bench.py, profiles/r06_clip_up.txt): one decoder's frame 22.5 -> 19.3 us (1080p yuv420p under the default fill), 18.0 -> 17.3
  // (720p filling 1080p); a v210 clip and frames of several layers are not faster this way (two layers 23.7 -> 24.1 us, four 1080 layers on
  // 2160p 95 -> 110: the conversions of a tile's rim are done twice) and keep the two launches.
  // (several frames of one shape - several channels' file playback - share the launch: a tile belongs to one frame)
  if (jobs <= ph::kMaxUpJobs && n == 1 && ctx->chan_enlarged == 1) {
    bool wire = true, alpha = false;
    for (int j = 0; j < jobs && wire; ++j) {
      const ph_chan_source &S = layers[j][0].src;
      const int fmt = fmt_of_src(S.format);
      wire = fmt >= 0 && fmt != PH_FMT_V210 && !(fmt_v420(fmt) && (S.height & 1));
      alpha = alpha || fmt_rgb8(fmt);
    }
    const LutRef rref = lds_view(ctx, rd_lut), wref = lds_view(ctx, wr_lut);
    if (wire && rref.found && wref.found) {
      ph::ClipUpArgs c{};
      ph::UpArgs &a = c.up;
      a.n = 1, a.jobs = (uint32_t)jobs, a.out = outs[0], a.out_w = out_w, a.out_h = out_h;
      for (int j = 1; j < jobs; ++j) a.more_out[j - 1] = outs[j];
      a.line_step = interlace ? 2 : 1, a.first_line = (interlace == 3) ? 1 : 0, a.lines = interlace ? out_h / 2 : out_h;
      a.wr_cm = (const float *)wr_cm, a.wr = wref.view;
      c.rd = rref.view, c.rd_gm = (const float *)rd_gm;
      {
        const ph_chan_source &S = layers[0][0].src;  // (every job's clip has this size and placement: chan_enlarged_same_shape)
        a.layer[0].w = (uint32_t)S.width, a.layer[0].h = (uint32_t)S.height, a.layer[0].pitch = (uint32_t)S.width * 16u;
        for (int k = 0; k < 6; ++k) a.layer[0].m[k] = S.matrix9_host[k];
      }
      for (int j = 0; j < jobs; ++j) {
        const ph_chan_source &S = layers[j][0].src;
        const int fmt = fmt_of_src(S.format);
        c.src[j] = ph::ClipSrc{S.data, S.data_u, S.data_v, (const float *)(S.col_matrix12 ? S.col_matrix12 : rd_cm), (uint32_t)fmt, ph::pack_pitch(fmt, (uint32_t)S.width)};
      }
      if (a.lines && ph::compose_up_eligible(a)) {
        const uint32_t grid = ph::clip_up_plan(c, !alpha, (uint32_t)ctx->props.multiProcessorCount);
        if (grid) {
          return with_scratch("ph_chan_compose_v210", ctx, queue, (size_t)c.wg_bytes * grid + 4096u, [&](hipStream_t s, void *area) {
            c.scratch = (char *)area;
            return ph::launch_clip_up_write_v210(s, c, !alpha, grid);
          });
        }
      }
    }
  }
  ph_image_layer il[ph::kMaxUpJobs][ph::kMaxLayers];
  const ph_image_layer *sets[ph::kMaxUpJobs];
  std::lock_guard<std::mutex> scratch(ctx->chan_scratch_mu[queue]);  // until the compositor's launch is enqueued
  const int rc = chan_enlarged_read(ctx, queue, jobs, n, layers, rd_cm, rd_lut, rd_gm, il, sets);
  if (rc) return rc;
  return ph_compose_up_write_v210_batch(ctx, queue, jobs, n, sets, outs, out_w, out_h, interlace, wr_cm, wr_lut);
}

int ph_chan_compose_v210(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, void *out, uint32_t out_w, uint32_t out_h,
                         uint32_t interlace, const void *rd_cm, const void *rd_lut, const void *rd_gm, const void *wr_cm,
                         const void *wr_lut) {
  void *planes[3] = {out, nullptr, nullptr};
  return ph_chan_compose(ctx, queue, n, layers, PH_FMT_V210, planes, out_w, out_h, interlace, rd_cm, rd_lut, rd_gm, wr_cm, wr_lut);
}

int ph_chan_compose(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int out_format, void *const out_planes[3], uint32_t out_w,
                    uint32_t out_h, uint32_t interlace, const void *rd_cm, const void *rd_lut, const void *rd_gm, const void *wr_cm,
                    const void *wr_lut) {
  if (!ctx || !layers || !out_planes || !out_planes[0] || !rd_cm || !rd_lut || !rd_gm || !wr_lut) return fail(PH_E_INVALID, "ph_chan_compose_v210: NULL argument");
  void *const out = out_planes[0];
  if (!fmt_known(out_format)) return fail(PH_E_INVALID, "ph_chan_compose_v210: output format %d is not a PH_FMT_*", out_format);
  if (!fmt_chan_out(out_format)) return chan_out_refused("ph_chan_compose_v210", out_format);
  const bool out_planar = fmt_planar(out_format);
  if (!fmt_rgb8(out_format) && !wr_cm) return fail(PH_E_INVALID, "ph_chan_compose_v210: the writer's RGB -> YCbCr matrix is missing");
  if (out_planar && (!out_planes[1] || (fmt_planes(out_format) == 3 && !out_planes[2])))
    return fail(PH_E_INVALID, "ph_chan_compose_v210: a planar output needs its three planes (nv12: Y and the interleaved CbCr plane)");
  if (fmt_v420(out_format) && (out_h & 1)) return fail(PH_E_INVALID, "ph_chan_compose_v210: a 4:2:0 frame needs an even height (%u)", out_h);
  PH_QUEUE("ph_chan_compose_v210", queue);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_chan_compose_v210: 1..%d layers", ph::kMaxLayers);
  // A v210 line of a width that is not a multiple of 48 (1280 x 720, src/config.ts:43-54) ends in a padded block: whole quads, the
  // tail quad with the reference's tail arithmetic (v210.ts:166-193), cleared slots - lines addressed by pitch.
  // The planar writers here take whole groups of eight pixels; rgba8 / bgra8 any width.
  if (!out_w || (out_format == PH_FMT_V210 && (out_w & 1)) || (out_planar && out_w % 8))
    return fail(PH_E_INVALID, "ph_chan_compose_v210: width %u (a v210 frame needs an even width, a planar one a multiple of 8); run the separate kernels", out_w);
  if (interlace != 0 && interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "ph_chan_compose_v210: interlace must be 0, 1 or 3");
  const LutRef rref = lds_view(ctx, rd_lut), wref = lds_view(ctx, wr_lut);
  const ph::LutView *rv = rref.get(), *wv = wref.get();
  if (!rv || !wv)
    return fail(PH_E_INVALID, "ph_chan_compose_v210: the %s gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", rv ? "writer" : "reader");
  ph::ChanArgs a{};
  int k = 0;
  int rc_ops = chan_ops(n, layers, out_w, out_h, a.op, a.plane_u, a.plane_v, a.cm_op, &a.planar, &k);
  if (rc_ops) return rc_ops;
  a.n_ops = k;
  a.out = out, a.out_w = out_w, a.out_h = out_h;
  a.line_step = interlace ? 2 : 1, a.first_line = (interlace == 3) ? 1 : 0;
  a.lines = interlace ? out_h / 2 : out_h;
  a.rd_cm = (const float *)rd_cm, a.rd_gm = (const float *)rd_gm, a.wr_cm = (const float *)(wr_cm ? wr_cm : rd_cm), a.rd = *rv, a.wr = *wv;
  a.out_fmt = (uint32_t)out_format, a.out_u = out_planes[1], a.out_v = out_planes[2];
  a.out_pitch = out_w;  // planar: width rounded up to 8 samples (yuv422p10.ts:221) - widths here are multiples of 8; rgba8: no padding
  a.out_qpitch = ph_v210_pitch_bytes(out_w) / 16u;
  a.out_tail_from = 0xFFFFFFFFu;
  if (out_format == PH_FMT_V210 && out_w % 48) {
    if (a.planar < 1) a.planar = 1;  // the tail instantiation writes lines that end in a tail / cleared slots
    if (out_w % 6) a.out_tail_from = out_w - out_w % 6u;
  }
  if (!a.lines) return PH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  if (out_format == PH_FMT_V210 && wr_cm && ctx->chan_enlarged && chan_layers_enlarged(n, layers, out_w, out_h, interlace))
    return chan_compose_enlarged(ctx, queue, 1, n, &layers, &out, out_w, out_h, interlace, rd_cm, rd_lut, rd_gm, wr_cm, wr_lut);
  // the index frame between the phases: one per queue (launches on one queue are in order), grown on demand
  return with_scratch("ph_chan_compose_v210", ctx, queue, ph::chan_index_bytes(out_w, a.lines), [&](hipStream_t s, void *area) {
    a.index = area;
    return ph::launch_chan_compose_v210(s, a, (uint32_t)ctx->props.multiProcessorCount);
  });
}

// One output of a several-outputs call, checked as ph_chan_compose checks its only one.  where: "" or "job <j>: " (ph_chan_compose_batch_out)
static int chan_output_check(const char *fn, const char *where, int k, const ph_chan_output &o, uint32_t out_w, uint32_t out_h) {
  if (!o.planes[0] || !o.wr_gamma_lut) return fail(PH_E_INVALID, "%s: %soutput %d: NULL argument", fn, where, k);
  if (!fmt_known(o.format)) return fail(PH_E_INVALID, "%s: %soutput %d: format %d is not a PH_FMT_*", fn, where, k, o.format);
  if (!fmt_chan_out(o.format)) return chan_out_refused(fn, o.format);
  if (!fmt_rgb8(o.format) && !o.wr_col_matrix12) return fail(PH_E_INVALID, "%s: %soutput %d: the writer's RGB -> YCbCr matrix is missing", fn, where, k);
  if (fmt_planar(o.format) && (!o.planes[1] || (fmt_planes(o.format) == 3 && !o.planes[2])))
    return fail(PH_E_INVALID, "%s: %soutput %d: a planar output needs its three planes (nv12: Y and the interleaved CbCr plane)", fn, where, k);
  if (fmt_v420(o.format) && (out_h & 1)) return fail(PH_E_INVALID, "%s: %soutput %d: a 4:2:0 frame needs an even height (%u)", fn, where, k, out_h);
  if ((o.format == PH_FMT_V210 && (out_w & 1)) || (fmt_planar(o.format) && out_w % 8))
    return fail(PH_E_INVALID, "%s: %soutput %d: width %u (a v210 frame needs an even width, a planar one a multiple of 8); run the separate kernels", fn, where, k, out_w);
  if (o.interlace != 0 && o.interlace != 1 && o.interlace != 3) return fail(PH_E_INVALID, "%s: %soutput %d: interlace must be 0, 1 or 3", fn, where, k);
  return PH_OK;
}

// An output's field mode as the several-outputs kernels take it (d: a ChanOut, ChanBatchOut, FusedOut or UpOut).  same_lines: the launch
// composes just the lines every output wants; else it composes the whole frame, and a field output takes the lines of its parity
extern "C++" template <class Out>
static void out_lines(const ph_chan_output &o, bool same_lines, uint32_t out_h, Out &d) {
  d.takes = same_lines || !o.interlace ? 0u : o.interlace == 1 ? 1u : 2u;
  d.line_end = o.interlace ? 2u * (out_h / 2u) : out_h;  // (a field of an odd height: out_h / 2 lines, as ph_chan_compose writes it)
  d.field = o.interlace ? 1u : 0u;
}
// the outputs grouped by writer table (writer_table_groups): the order alone, for a launch that takes every group
static void by_writer_table(int n_out, const ph_chan_output *outs, int *order) {
  int start[(ph::kMaxChanOuts > ph::kMaxFusedOuts ? ph::kMaxChanOuts : ph::kMaxFusedOuts) + 1];
  writer_table_groups(n_out, outs, order, start);
}

/* Several consumers' frames of one composition in one launch: see include/phaneron_hip.h.  Every check is made before anything is
 * launched; the checks and their texts are ph_chan_compose's, per output. */
int ph_chan_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w,
                          uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  if (!ctx || !layers || !outs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "ph_chan_compose_multi: NULL argument");
  if (n_out < 1 || n_out > ph::kMaxChanOuts) return fail(PH_E_INVALID, "ph_chan_compose_multi: 1..%d outputs (%d)", ph::kMaxChanOuts, n_out);
  if (n_out == 1)
    return ph_chan_compose(ctx, queue, n, layers, outs[0].format, outs[0].planes, out_w, out_h, outs[0].interlace, rd_cm, rd_lut, rd_gm, outs[0].wr_col_matrix12,
                           outs[0].wr_gamma_lut);
  PH_QUEUE("ph_chan_compose_multi", queue);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_chan_compose_multi: 1..%d layers", ph::kMaxLayers);
  if (!out_w) return fail(PH_E_INVALID, "ph_chan_compose_multi: width 0");
  bool any_v210 = false, same_lines = true;
  for (int k = 0; k < n_out; ++k) {
    const ph_chan_output &o = outs[k];
    if (const int bad = chan_output_check("ph_chan_compose_multi", "", k, o, out_w, out_h)) return bad;
    for (int j = 0; j < k; ++j)
      if (outs[j].planes[0] == o.planes[0]) return fail(PH_E_INVALID, "ph_chan_compose_multi: outputs %d and %d name the same plane", j, k);
    any_v210 = any_v210 || o.format == PH_FMT_V210;
    same_lines = same_lines && o.interlace == outs[0].interlace;
  }
  const LutRef rref = lds_view(ctx, rd_lut);
  if (!rref.get()) return fail(PH_E_INVALID, "ph_chan_compose_multi: the reader gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)");
  LutRef wref[ph::kMaxChanOuts];
  for (int k = 0; k < n_out; ++k) {
    wref[k] = lds_view(ctx, outs[k].wr_gamma_lut);
    if (!wref[k].get())
      return fail(PH_E_INVALID, "ph_chan_compose_multi: output %d: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", k);
  }
  ph::ChanMultiArgs m{};
  ph::ChanArgs &a = m.c;
  int n_ops = 0;
  int rc = chan_ops(n, layers, out_w, out_h, a.op, a.plane_u, a.plane_v, a.cm_op, &a.planar, &n_ops);
  if (rc) return rc;
  a.n_ops = n_ops;
  a.out_w = out_w, a.out_h = out_h;
  // the lines composed: the field every output wants, or the whole frame (a field output then takes the index rows of its parity)
  const uint32_t interlace = same_lines ? outs[0].interlace : 0u;
  a.line_step = interlace ? 2 : 1, a.first_line = (interlace == 3) ? 1 : 0;
  a.lines = interlace ? out_h / 2 : out_h;
  a.rd_cm = (const float *)rd_cm, a.rd_gm = (const float *)rd_gm, a.rd = *rref.get();
  a.out_tail_from = 0xFFFFFFFFu;
  if (any_v210 && out_w % 48) {  // as ph_chan_compose: the tail instantiation writes lines that end in a tail / cleared slots
    if (a.planar < 1) a.planar = 1;
    if (out_w % 6) a.out_tail_from = out_w - out_w % 6u;
  }
  int order[ph::kMaxChanOuts];
  by_writer_table(n_out, outs, order);
  m.n_out = (uint32_t)n_out;
  for (int i = 0; i < n_out; ++i) {
    const ph_chan_output &o = outs[order[i]];
    ph::ChanOut &d = m.out[i];
    d.fmt = (uint32_t)o.format;
    d.pitch = o.format == PH_FMT_V210 ? ph_v210_pitch_bytes(out_w) / 16u : out_w;
    d.plane[0] = o.planes[0], d.plane[1] = o.planes[1], d.plane[2] = o.planes[2];
    d.tail_from = o.format == PH_FMT_V210 ? a.out_tail_from : 0xFFFFFFFFu;
    out_lines(o, same_lines, out_h, d);
    d.round = o.format != PH_FMT_V210 && a.out_tail_from != 0xFFFFFFFFu ? 1u : 0u;
    d.wr_cm = (const float *)(o.wr_col_matrix12 ? o.wr_col_matrix12 : rd_cm);
    d.wr = *wref[order[i]].get();
  }
  a.wr = m.out[0].wr, a.wr_cm = m.out[0].wr_cm;
  if (!a.lines) return PH_OK;
  rc = set_device(ctx);
  if (rc) return rc;
  return with_scratch("ph_chan_compose_multi", ctx, queue, ph::chan_index_bytes(out_w, a.lines), [&](hipStream_t s, void *area) {
    a.index = area;
    return ph::launch_chan_compose_multi(s, m, (uint32_t)ctx->props.multiProcessorCount);
  });
}

// The field (interlace 1 or 3) of which alone ph_fused_v210_combine_multi and its batch compose the lines: every output takes it and the context
// asks for it (option "fused_fields") - or 0: the whole frame is composed.  (A field of a frame of height h is h / 2 lines: out_lines.)
static uint32_t fused_field_of(const ph_ctx *ctx, int n_out, const ph_chan_output *outs) {
  if (!ctx->fused_fields) return 0;
  for (int k = 0; k < n_out; ++k)
    if (!outs[k].interlace || outs[k].interlace != outs[0].interlace) return 0;
  return (uint32_t)outs[0].interlace;
}
// What ph_fused_v210_combine_multi and ph_fused_v210_transition_multi refuse about their outputs and geometry - everything but the layers and
// the context, which each entry sees to itself
static int fused_multi_outputs_check(const char *fn, int queue, int n_out, const ph_chan_output *outs, uint32_t width, uint32_t height) {
  PH_QUEUE(fn, queue);
  if (!width) return fail(PH_E_INVALID, "%s: width 0", fn);
  for (int k = 0; k < n_out; ++k) {
    if (const int bad = chan_output_check(fn, "", k, outs[k], width, height)) return bad;
    for (int j = 0; j < k; ++j)
      if (outs[j].planes[0] == outs[k].planes[0]) return fail(PH_E_INVALID, "%s: outputs %d and %d name the same plane", fn, j, k);
  }
  return PH_OK;
}
// The shared launch's arguments but for the layers - or false: the call does not qualify.  It needs lines of whole 48-pixel blocks, every
// table in its LDS form (none is with the option "lds_lut" = 0), a frame small enough for the kernel's quad -> line division by reciprocal.
// order (kMaxFusedOuts entries, or NULL): m.out[i] is outs[order[i]]
// field (fused_field_of): 0, or the field every output takes - the arguments are then the field launch's: its quads, every composed line every output's
static bool fused_multi_shared(ph_ctx *ctx, int n_out, const ph_chan_output *outs, uint32_t width, uint32_t height, const void *rd_cm, const void *rd_lut,
                               const void *rd_gm, ph::FusedMultiArgs &m, int *order = nullptr, uint32_t field = 0) {
  const LutRef rref = lds_view(ctx, rd_lut);
  LutRef wref[ph::kMaxFusedOuts];
  bool shared = width % 48 == 0 && rref.get() && (uint64_t)(width / 6) * height * (width / 6) < (1ull << 32);
  for (int k = 0; k < n_out && shared; ++k) {
    wref[k] = lds_view(ctx, outs[k].wr_gamma_lut);
    shared = wref[k].get() != nullptr;
  }
  if (!shared) return false;
  m.quads_per_line = width / 6, m.total_quads = m.quads_per_line * (field ? height / 2u : height);
  m.rd_cm = (const float *)rd_cm, m.rd_gm = (const float *)rd_gm, m.rd = *rref.get();
  int own[ph::kMaxFusedOuts];
  if (!order) order = own;
  by_writer_table(n_out, outs, order);
  m.n_out = (uint32_t)n_out;
  for (int i = 0; i < n_out; ++i) {
    const ph_chan_output &o = outs[order[i]];
    ph::FusedOut &d = m.out[i];
    d.fmt = (uint32_t)o.format;
    out_lines(o, /*same_lines*/ field != 0, height, d);  // the whole frame is composed: a field output takes the lines of its parity - or only the field all take
    d.wr_cm = (const float *)(o.wr_col_matrix12 ? o.wr_col_matrix12 : rd_cm);
    d.plane[0] = o.planes[0], d.plane[1] = o.planes[1], d.plane[2] = o.planes[2];
    d.wr = *wref[order[i]].get();
  }
  return true;
}
// a frame of the channel's size taken 1:1, as a cut layer of ph_chan_compose_multi: what the fused entries hand a call on with
static ph_chan_layer plain_chan_layer(const void *data, int format, uint32_t width, uint32_t height) {
  ph_chan_layer c;
  memset(&c, 0, sizeof c);
  c.src.data = data, c.src.format = format, c.src.width = (int)width, c.src.height = (int)height;
  c.transition = PH_TRANSITION_CUT;
  return c;
}

/* The plain-layer composite for several consumers: see include/phaneron_hip.h.  The call IS the n_out calls of ph_chan_compose on the layers
 * taken 1:1; every check is made before anything is launched, with ph_chan_compose_multi's texts per output.  A call the shared kernel
 * does not take runs ph_chan_compose_multi on those layers, which answers for everything else. */
int ph_fused_v210_combine_multi(ph_ctx *ctx, int queue, int n, const void *const *layers, int n_out, const ph_chan_output *outs, uint32_t width,
                                uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = "ph_fused_v210_combine_multi";
  if (!ctx || !layers || !outs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  if (n_out < 1 || n_out > ph::kMaxFusedOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxFusedOuts, n_out);
  for (int i = 0; i < n; ++i)
    if (!layers[i]) return fail(PH_E_INVALID, "%s: layer %d is NULL", fn, i);
  if (const int bad = fused_multi_outputs_check(fn, queue, n_out, outs, width, height)) return bad;
  // one v210 frame: the headline kernel itself, same route
  if (n_out == 1 && outs[0].format == PH_FMT_V210 && outs[0].interlace == 0)
    return ph_fused_v210_combine(ctx, queue, n, layers, outs[0].planes[0], width, height, rd_cm, rd_lut, rd_gm, outs[0].wr_col_matrix12, outs[0].wr_gamma_lut);
  const uint32_t field = fused_field_of(ctx, n_out, outs);
  ph::FusedFieldArgs fa{};  // (the whole-frame launch takes its m alone)
  ph::FusedMultiArgs &m = fa.m;
  if (!fused_multi_shared(ctx, n_out, outs, width, height, rd_cm, rd_lut, rd_gm, m, nullptr, field)) {
    ph_chan_layer cl[ph::kMaxLayers];
    for (int i = 0; i < n; ++i) cl[i] = plain_chan_layer(layers[i], PH_SRC_V210, width, height);
    return ph_chan_compose_multi(ctx, queue, n, cl, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  }
  if (!m.total_quads) return PH_OK;  // height 0 - or a field of a frame of one line
  for (int i = 0; i < n; ++i) m.layers[i] = layers[i];
  const int rc = set_device(ctx);
  if (rc) return rc;
  fa.first_line = field == 3 ? 1u : 0u;
  const uint32_t cus = (uint32_t)ctx->props.multiProcessorCount, cap = (uint32_t)ctx->fused_multi_wgs;
  const hipError_t e = field ? ph::launch_fused_v210_field_multi(stream_of(ctx, queue), n, fa, field, cus, cap)
                             : ph::launch_fused_v210_combine_multi(stream_of(ctx, queue), n, m, cus, cap);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return PH_OK;
}

/* The same with layers in a dissolve or a wipe: see include/phaneron_hip.h.  What the arguments alone decide is decided first - the context is
 * looked at last, so a caller without a device learns of its mistakes too. */
int ph_fused_v210_transition_multi(ph_ctx *ctx, int queue, int n, const ph_fused_layer *layers, int n_out, const ph_chan_output *outs, uint32_t width,
                                   uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = "ph_fused_v210_transition_multi";
  if (!layers || !outs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  if (n_out < 1 || n_out > ph::kMaxFusedOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxFusedOuts, n_out);
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const ph_fused_layer &L = layers[i];
    if (!L.v210) return fail(PH_E_INVALID, "%s: layer %d is NULL", fn, i);
    if (L.transition != PH_TRANSITION_CUT && L.transition != PH_TRANSITION_DISSOLVE && L.transition != PH_TRANSITION_WIPE)
      return fail(PH_E_INVALID, "%s: layer %d: transition %d is not a PH_TRANSITION_*", fn, i, L.transition);
    if (L.transition == PH_TRANSITION_CUT) continue;
    any = true;
    if (!L.incoming_v210) return fail(PH_E_INVALID, "%s: layer %d: a layer in a transition needs its incoming frame", fn, i);
    if (L.transition != PH_TRANSITION_WIPE) continue;
    if (!L.mask) return fail(PH_E_INVALID, "%s: layer %d: a wipe needs its mask", fn, i);
    if (L.mask_format != PH_SRC_V210 && L.mask_format != PH_SRC_RGBA_F32)
      return fail(PH_E_INVALID, "%s: layer %d: mask format %d (a v210 frame, PH_SRC_V210, or an f32 RGBA image, PH_SRC_RGBA_F32)", fn, i, L.mask_format);
  }
  if (const int bad = fused_multi_outputs_check(fn, queue, n_out, outs, width, height)) return bad;
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  if (!any) {  // every layer a cut: ph_fused_v210_combine_multi on the layers' frames
    const void *plain[ph::kMaxLayers];
    for (int i = 0; i < n; ++i) plain[i] = layers[i].v210;
    return ph_fused_v210_combine_multi(ctx, queue, n, plain, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  }
  ph::FusedTransArgs t{};
  if (!fused_multi_shared(ctx, n_out, outs, width, height, rd_cm, rd_lut, rd_gm, t.m)) {
    ph_chan_layer cl[ph::kMaxLayers];
    for (int i = 0; i < n; ++i) {
      const ph_fused_layer &L = layers[i];
      cl[i] = plain_chan_layer(L.v210, PH_SRC_V210, width, height);
      cl[i].transition = L.transition, cl[i].mix = L.mix;
      if (L.transition != PH_TRANSITION_CUT) cl[i].incoming = plain_chan_layer(L.incoming_v210, PH_SRC_V210, width, height).src;
      if (L.transition == PH_TRANSITION_WIPE) cl[i].mask = plain_chan_layer(L.mask, L.mask_format, width, height).src;
    }
    return ph_chan_compose_multi(ctx, queue, n, cl, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  }
  if (!height) return PH_OK;
  for (int i = 0; i < n; ++i) {
    const ph_fused_layer &L = layers[i];
    t.m.layers[i] = L.v210;
    if (L.transition == PH_TRANSITION_CUT) continue;  // (kFusedCut: what a cut layer says beside its frame is not looked at)
    t.incoming[i] = L.incoming_v210;
    if (L.transition == PH_TRANSITION_DISSOLVE) {
      t.kind[i] = ph::kFusedDissolve, t.mix[i] = L.mix;
    } else {
      t.kind[i] = L.mask_format == PH_SRC_V210 ? ph::kFusedWipeV210 : ph::kFusedWipeF32, t.mask[i] = L.mask;
    }
  }
  const int rc = set_device(ctx);
  if (rc) return rc;
  const hipError_t e = ph::launch_fused_v210_trans_multi(stream_of(ctx, queue), n, t, (uint32_t)ctx->props.multiProcessorCount, (uint32_t)ctx->fused_multi_wgs);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return PH_OK;
}

/* The same for a routed channel - an f32 RGBA image among the layers, the combined image among the outputs: see include/phaneron_hip.h.
 * What the arguments alone decide is decided first; the context is looked at last. */
int ph_fused_v210_route_multi(ph_ctx *ctx, int queue, int n, const ph_route_layer *layers, void *image_out, int n_out, const ph_chan_output *outs,
                              uint32_t width, uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = "ph_fused_v210_route_multi";
  if (n_out < 0 || n_out > ph::kMaxFusedOuts) return fail(PH_E_INVALID, "%s: 0..%d outputs (%d)", fn, ph::kMaxFusedOuts, n_out);
  if (!layers || (n_out && !outs) || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  if (!n_out && !image_out) return fail(PH_E_INVALID, "%s: nothing to make: no output and image_out is NULL", fn);
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const ph_route_layer &L = layers[i];
    if (!L.data) return fail(PH_E_INVALID, "%s: layer %d is NULL", fn, i);
    if (L.format != PH_SRC_V210 && L.format != PH_SRC_RGBA_F32)
      return fail(PH_E_INVALID, "%s: layer %d: format %d (a v210 frame, PH_SRC_V210, or an f32 RGBA image, PH_SRC_RGBA_F32)", fn, i, L.format);
    any = any || L.format == PH_SRC_RGBA_F32;
    // (tail lanes recompute the last quad of a range: they would read what another lane has just written)
    if (L.data == image_out) return fail(PH_E_INVALID, "%s: image_out is layer %d's data", fn, i);
  }
  if (const int bad = fused_multi_outputs_check(fn, queue, n_out, outs, width, height)) return bad;
  for (int k = 0; k < n_out; ++k)
    if (image_out && outs[k].planes[0] == image_out) return fail(PH_E_INVALID, "%s: image_out is output %d's first plane", fn, k);
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  if (!any && !image_out) {  // plain layers, packed frames only: ph_fused_v210_combine_multi on the layers' frames
    const void *plain[ph::kMaxLayers];
    for (int i = 0; i < n; ++i) plain[i] = layers[i].data;
    return ph_fused_v210_combine_multi(ctx, queue, n, plain, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  }
  ph::FusedRouteArgs t{};
  if (!fused_multi_shared(ctx, n_out, outs, width, height, rd_cm, rd_lut, rd_gm, t.m)) {
    if (image_out)
      return fail(PH_E_INVALID,
                  "%s: the one-launch route does not take this frame (it needs width %% 48 == 0, the reader's and every writer's table registered, \"lds_lut\" = 1 and a "
                  "frame within the kernel's division by reciprocal) and nothing else makes image_out: run ph_v210_read, ph_combine and ph_pack_write_multi",
                  fn);
    ph_chan_layer cl[ph::kMaxLayers];
    for (int i = 0; i < n; ++i) cl[i] = plain_chan_layer(layers[i].data, layers[i].format, width, height);
    return ph_chan_compose_multi(ctx, queue, n, cl, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  }
  if (!height) return PH_OK;
  for (int i = 0; i < n; ++i) t.m.layers[i] = layers[i].data, t.is_image[i] = layers[i].format == PH_SRC_RGBA_F32 ? 1u : 0u;
  t.image_out = image_out;
  const int rc = set_device(ctx);
  if (rc) return rc;
  const hipError_t e = ph::launch_fused_v210_route_multi(stream_of(ctx, queue), n, t, (uint32_t)ctx->props.multiProcessorCount, (uint32_t)ctx->fused_multi_wgs);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return PH_OK;
}

/* Several channels' plain-layer composites, each for the same consumers, in one launch: see include/phaneron_hip.h.  The call IS the `jobs`
 * calls of ph_fused_v210_combine_multi in order; every check - those calls' own, per job and output - is made before anything is launched. */
int ph_fused_v210_combine_multi_batch(ph_ctx *ctx, int queue, int jobs, int n, const void *const *layers, int n_out, const ph_chan_output *outs,
                                      uint32_t width, uint32_t height, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = "ph_fused_v210_combine_multi_batch";
  if (!ctx || !layers || !outs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (jobs < 1 || jobs > ph::kMaxBatch) return fail(PH_E_INVALID, "%s: 1..%d jobs (%d)", fn, ph::kMaxBatch, jobs);
  if (jobs == 1) return ph_fused_v210_combine_multi(ctx, queue, n, layers, n_out, outs, width, height, rd_cm, rd_lut, rd_gm);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  if (n_out < 1 || n_out > ph::kMaxFusedOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxFusedOuts, n_out);
  for (int j = 0; j < jobs; ++j)
    for (int i = 0; i < n; ++i)
      if (!layers[(size_t)j * n + i]) return fail(PH_E_INVALID, "%s: job %d: layer %d is NULL", fn, j, i);
  PH_QUEUE(fn, queue);
  if (!width) return fail(PH_E_INVALID, "%s: width 0", fn);
  bool frames_only = n_out == 1;
  for (int j = 0; j < jobs; ++j) {
    char where[16];
    snprintf(where, sizeof where, "job %d: ", j);
    for (int k = 0; k < n_out; ++k) {
      const ph_chan_output &o = outs[(size_t)j * n_out + k], &o0 = outs[k];
      if (const int bad = chan_output_check(fn, where, k, o, width, height)) return bad;
      if (o.format != o0.format || o.interlace != o0.interlace || o.wr_col_matrix12 != o0.wr_col_matrix12 || o.wr_gamma_lut != o0.wr_gamma_lut)
        return fail(PH_E_INVALID, "%s: job %d: output %d differs from job 0's in more than its planes (format, interlace, writer matrix, writer table)", fn, j, k);
      for (int e = 0; e < j * n_out + k; ++e)
        if (outs[e].planes[0] == o.planes[0])
          return fail(PH_E_INVALID, "%s: job %d output %d and job %d output %d name the same plane", fn, e / n_out, e % n_out, j, k);
      frames_only = frames_only && o.format == PH_FMT_V210 && o.interlace == 0;
    }
  }
  if (frames_only) {  // every job one v210 frame: the headline kernel's own batch, same route
    void *frames[ph::kMaxBatch];
    for (int j = 0; j < jobs; ++j) frames[j] = outs[j].planes[0];
    return ph_fused_v210_combine_batch(ctx, queue, jobs, n, layers, frames, width, height, rd_cm, rd_lut, rd_gm, outs[0].wr_col_matrix12, outs[0].wr_gamma_lut);
  }
  // the shared launch: what ph_fused_v210_combine_multi's own asks for, with its arguments (every job's output list is job 0's: one order for all)
  const uint32_t field = fused_field_of(ctx, n_out, outs);
  ph::FusedFieldBatchArgs fb{};  // (the whole-frame launch takes its b alone)
  ph::FusedMultiBatchArgs &b = fb.b;
  int order[ph::kMaxFusedOuts];
  if (!fused_multi_shared(ctx, n_out, outs, width, height, rd_cm, rd_lut, rd_gm, b.m, order, field)) {
    for (int j = 0; j < jobs; ++j)
      if (const int rc = ph_fused_v210_combine_multi(ctx, queue, n, layers + (size_t)j * n, n_out, outs + (size_t)j * n_out, width, height, rd_cm, rd_lut, rd_gm)) return rc;
    return PH_OK;
  }
  if (!b.m.total_quads) return PH_OK;  // height 0 - or a field of a frame of one line
  for (int j = 0; j < jobs; ++j) {  // (b.m.out[i].plane, job 0's, is not read: each job's planes are b.plane's)
    for (int i = 0; i < n; ++i) b.layers[j][i] = layers[(size_t)j * n + i];
    for (int i = 0; i < n_out; ++i)
      for (int p = 0; p < 3; ++p) b.plane[j][i][p] = outs[(size_t)j * n_out + order[i]].planes[p];
  }
  const int rc = set_device(ctx);
  if (rc) return rc;
  fb.first_line = field == 3 ? 1u : 0u;
  const uint32_t cus = (uint32_t)ctx->props.multiProcessorCount, cap = (uint32_t)ctx->fused_multi_wgs;
  const hipError_t e = field ? ph::launch_fused_v210_field_multi_batch(stream_of(ctx, queue), n, (uint32_t)jobs, fb, field, cus, cap)
                             : ph::launch_fused_v210_combine_multi_batch(stream_of(ctx, queue), n, (uint32_t)jobs, b, cus, cap);
  if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  return PH_OK;
}

// A job's Loader matrices as indices into a launch's small table: cm_of[i] = 1 .. 8, or 0 for the call's own matrix.  tab: the launch's
// table with the job's matrices in it - those already there are found again, new ones appended in the order they first appear - for
// the caller to make the launch's if the job joins it.  false: the table does not hold them all
static bool place_cms(int n_ops, const float *const *cm_op, const void *rd_cm, const float *const *launch_tab, const float **tab, uint8_t *cm_of) {
  for (int t = 0; t < 8; ++t) tab[t] = launch_tab[t];
  for (int i = 0; i < n_ops; ++i) {
    cm_of[i] = 0;
    const float *cm = cm_op[i];
    if (!cm || cm == (const float *)rd_cm) continue;
    int at = 0;
    while (at < 8 && tab[at] && tab[at] != cm) ++at;
    if (at == 8) return false;
    tab[at] = cm, cm_of[i] = (uint8_t)(at + 1);
  }
  return true;
}

/* Several channels' frames in one launch: see include/phaneron_hip.h.  Jobs the batch kernel does not take (planar / packed-RGB sources,
 * more ops or wave steps than one launch holds) run through ph_chan_compose_v210 in their turn, so the call as a whole is always the
 * `n_jobs` separate calls it stands for. */
int ph_chan_compose_batch(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job *jobs, uint32_t out_w, uint32_t out_h, const void *rd_cm,
                          const void *rd_lut, const void *rd_gm, const void *wr_cm, const void *wr_lut) {
  if (!ctx || !jobs || !rd_cm || !rd_lut || !rd_gm || !wr_cm || !wr_lut) return fail(PH_E_INVALID, "ph_chan_compose_batch: NULL argument");
  PH_QUEUE("ph_chan_compose_batch", queue);
  if (n_jobs < 1) return fail(PH_E_INVALID, "ph_chan_compose_batch: no jobs");
  if (!out_w || (out_w & 1)) return fail(PH_E_INVALID, "ph_chan_compose_batch: width %u (a v210 frame needs an even width)", out_w);
  const LutRef rref = lds_view(ctx, rd_lut), wref = lds_view(ctx, wr_lut);
  const ph::LutView *rv = rref.get(), *wv = wref.get();
  if (!rv || !wv)
    return fail(PH_E_INVALID, "ph_chan_compose_batch: the %s gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", rv ? "writer" : "reader");
  for (int j = 0; j < n_jobs; ++j) {
    const ph_chan_job &J = jobs[j];
    if (!J.layers || !J.out || J.n < 1 || J.n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_chan_compose_batch: job %d: 1..%d layers and an output", j, ph::kMaxLayers);
    if (J.interlace != 0 && J.interlace != 1 && J.interlace != 3) return fail(PH_E_INVALID, "ph_chan_compose_batch: job %d: interlace must be 0, 1 or 3", j);
  }
  const ph::LutView &rview = rref.view, &wview = wref.view;
  int rc = set_device(ctx);
  if (rc) return rc;
  // the common part of a launch's arguments (ChanArgs carries it to chan_batch_launch)
  auto common = [&](uint32_t interlace) {
    ph::ChanArgs a{};
    a.out_w = out_w, a.out_h = out_h;
    a.line_step = interlace ? 2 : 1, a.lines = interlace ? out_h / 2 : out_h;
    a.rd_cm = (const float *)rd_cm, a.rd_gm = (const float *)rd_gm, a.wr_cm = (const float *)wr_cm, a.rd = rview, a.wr = wview;
    a.out_qpitch = ph_v210_pitch_bytes(out_w) / 16u;
    a.out_tail_from = out_w % 6 ? out_w - out_w % 6u : 0xFFFFFFFFu;
    a.planar = out_w % 48 ? 1u : 0u;
    return a;
  };
  // How many jobs a launch should take so that the launches come out even (eight jobs of six ops are 4 + 4, not 6 + 2: a launch of
  // two is a poor one): by the jobs and ops of the call as a whole - a plan, the limits below still hold for every launch
  uint32_t plan_jobs = 0, plan_ops = 0;
  for (int j = 0; j < n_jobs; ++j) {
    uint32_t ops = 0;  // (planar / packed-RGB sources share launches too since round 6: the batch kernel's PLANAR instantiation)
    for (int l = 0; l < jobs[j].n; ++l) {
      const ph_chan_layer &L = jobs[j].layers[l];
      ops += L.transition == PH_TRANSITION_WIPE ? 3u : L.transition == PH_TRANSITION_DISSOLVE ? 2u : 1u;
    }
    if (ops <= (uint32_t)ph::kMaxChanBatchOps && !(ctx->chan_enlarged && chan_layers_enlarged(jobs[j].n, jobs[j].layers, out_w, out_h, jobs[j].interlace)))
      ++plan_jobs, plan_ops += ops;
  }
  const uint32_t by_jobs = (plan_jobs + (uint32_t)ph::kMaxChanJobs - 1u) / (uint32_t)ph::kMaxChanJobs;
  const uint32_t by_ops = (plan_ops + (uint32_t)ph::kMaxChanBatchOps - 1u) / (uint32_t)ph::kMaxChanBatchOps;
  const uint32_t launches = by_jobs > by_ops ? by_jobs : by_ops;
  const uint32_t jobs_per_launch = launches ? (plan_jobs + launches - 1u) / launches : 1u;
  ph::ChanBatchArgs b{};
  ph::ChanArgs a = common(0);
  bool fields = false;
  int first_job = 0;  // of the launch being collected
  // frames of enlarged clips among the jobs (chan_compose_enlarged): those of one shape and field mode, one after the other, are made together
  const ph_chan_layer *enl_layers[ph::kMaxUpJobs];
  void *enl_outs[ph::kMaxUpJobs];
  int enl = 0, enl_n = 0;
  uint32_t enl_interlace = 0;
  auto flush_enlarged = [&]() -> int {
    if (!enl) return PH_OK;
    const int r = chan_compose_enlarged(ctx, queue, enl, enl_n, enl_layers, enl_outs, out_w, out_h, enl_interlace, rd_cm, rd_lut, rd_gm, wr_cm, wr_lut);
    enl = 0;
    return r;
  };
  auto flush = [&]() -> int {
    if (!b.jobs) return PH_OK;
    int r;
    if (b.jobs == 1) {  // nothing to share: the one-job kernel
      const ph_chan_job &J = jobs[first_job];
      r = ph_chan_compose_v210(ctx, queue, J.n, J.layers, J.out, out_w, out_h, J.interlace, rd_cm, rd_lut, rd_gm, wr_cm, wr_lut);
    } else {
      r = chan_batch_launch(ctx, queue, b, a);
    }
    b = ph::ChanBatchArgs{};
    return r;
  };
  for (int j = 0; j < n_jobs; ++j) {
    const ph_chan_job &J = jobs[j];
    ph::ChanArgs one{};  // this job's program, checked as the single call checks it
    int k = 0;
    rc = chan_ops(J.n, J.layers, out_w, out_h, one.op, one.plane_u, one.plane_v, one.cm_op, &one.planar, &k);
    if (rc) return rc;
    const bool is_field = J.interlace != 0;
    const uint32_t lines = is_field ? out_h / 2 : out_h;
    const uint32_t fit = chan_batch_on() ? jobs_per_launch : 0u;
    bool routed = lines && ctx->chan_enlarged && chan_layers_enlarged(J.n, J.layers, out_w, out_h, J.interlace);  // read + 2 x 2-block compositor, in its turn
    bool fits = false;
    auto fits_group = [&]() {
      bool f = enl > 0 && enl < ph::kMaxUpJobs && J.n == enl_n && J.interlace == enl_interlace && chan_enlarged_same_shape(J.n, enl_layers[0], J.layers);
      for (int e = 0; e < enl && f; ++e) f = enl_outs[e] != J.out;
      return f;
    };
    // (frames of v210 clips ONLY: with a packed-RGB graphic on top the images carry alpha and the route loses to the channel kernel - 42 against 34 us)
    bool all_v210 = true;
    for (int l = 0; l < J.n; ++l) all_v210 = all_v210 && J.layers[l].src.format == PH_SRC_V210;
    if (!routed && all_v210 && lines && ctx->chan_enlarged && chan_layers_enlarged(J.n, J.layers, out_w, out_h, J.interlace, true)) {
      // v210 frames under the default fill: by the route if they share its launches with a neighbour of their shape, else the batch kernel's
      const bool with_next = j + 1 < n_jobs && jobs[j + 1].n == J.n && jobs[j + 1].interlace == J.interlace && jobs[j + 1].out != J.out && jobs[j + 1].layers &&
                             chan_layers_enlarged(jobs[j + 1].n, jobs[j + 1].layers, out_w, out_h, jobs[j + 1].interlace, true) &&
                             chan_enlarged_same_shape(J.n, J.layers, jobs[j + 1].layers);
      routed = fits_group() || with_next;
    }
    if (routed) {
      if ((rc = flush())) return rc;
      fits = fits_group();
      if (!fits && (rc = flush_enlarged())) return rc;
      enl_layers[enl] = J.layers, enl_outs[enl] = J.out, enl_n = J.n, enl_interlace = J.interlace, ++enl;
      continue;
    }
    if ((rc = flush_enlarged())) return rc;
    // a planar job's Loader matrices against the launch's table as it stands: a job they do not fit runs on its own
    uint8_t cm_of[ph::kMaxChanOps];
    const float *tab[8];
    const bool cm_fits = one.planar != 2 || place_cms(k, one.cm_op, rd_cm, b.cm_tab, tab, cm_of);
    if (!cm_fits || k > ph::kMaxChanBatchOps || fit < 1 || !lines) {  // not for the batch kernel: in its turn, on its own
      if ((rc = flush())) return rc;
      if ((rc = ph_chan_compose_v210(ctx, queue, J.n, J.layers, J.out, out_w, out_h, J.interlace, rd_cm, rd_lut, rd_gm, wr_cm, wr_lut))) return rc;
      continue;
    }
    // a launch holds jobs of one kind (frames or fields: the same lines), no two of which write the same lines of one frame
    bool clash = false;
    for (uint32_t i = 0; i < b.jobs; ++i)
      clash = clash || (b.job[i].out == J.out && (!is_field || b.job[i].first_line == (J.interlace == 3 ? 1u : 0u)));
    if (b.jobs && (fields != is_field || clash || b.jobs >= fit || b.n_ops + (uint32_t)k > (uint32_t)ph::kMaxChanBatchOps))
      if ((rc = flush())) return rc;
    if (!b.jobs) a = common(J.interlace), fields = is_field, first_job = j;
    if (one.planar > a.planar) a.planar = one.planar;  // a source whose lines end in a tail
    ph::ChanJob &jb = b.job[b.jobs];
    jb.out = J.out, jb.first_op = b.n_ops, jb.n_ops = (uint32_t)k, jb.first_line = J.interlace == 3 ? 1u : 0u;
    for (int i = 0; i < k; ++i) b.op[b.n_ops + i] = one.op[i], b.op_job[b.n_ops + i] = (uint8_t)b.jobs;
    if (one.planar == 2) {
      // (a flush above has emptied the launch: the table then starts again, and what fitted the old one fits an empty one)
      place_cms(k, one.cm_op, rd_cm, b.cm_tab, tab, cm_of);
      for (int t = 0; t < 8; ++t) b.cm_tab[t] = tab[t];
      for (int i = 0; i < k; ++i) {
        b.plane_u[b.n_ops + i] = one.plane_u[i], b.plane_v[b.n_ops + i] = one.plane_v[i], b.cm_idx[b.n_ops + i] = cm_of[i];
        b.any_cm |= cm_of[i] ? 1u : 0u;
      }
    }
    b.n_ops += (uint32_t)k, ++b.jobs;
  }
  if ((rc = flush_enlarged())) return rc;
  return flush();
}

/* Several channels' frames for any consumers in one launch: see include/phaneron_hip.h.  Every check of every job is made before anything
 * is launched.  Jobs the shared launch does not take run through ph_chan_compose_multi in their turn; a launch that ends up with one job
 * is that call too, so a job on its own keeps the routes it has today. */
namespace {
struct ChanJobPlan {  // what ph_chan_compose_batch_out and ph_clip_compose_batch_out learn of a job while they check it
  ph::ChanArgs one{};  // the job's program (op, plane_u / plane_v, cm_op, planar)
  int n_ops = 0;
  uint32_t interlace = 0;  // the lines the job composes: the field every output wants, or the frame
  bool same_lines = true, any_v210 = false, joins = false;
  const void *table = nullptr;  // the writer table all its outputs name (NULL: they name several)
  Footprint print;              // what it reads and writes
  ChanJobPlan() {}              // (user-provided, as Footprint's: a vector of plans does not clear the spans)
};
}  // namespace
// One job of those two entries, checked as ph_chan_compose_multi checks its call, fault by fault in that order, and described in P.
// max_outs: the entry's limit; ctx: where an output's writer table is looked up between that output's checks and the next output's
// (NULL: the caller looks the tables up later, after every check of the arguments)
static int chan_job_check(const char *fn, int j, const ph_chan_job_out &J, int max_outs, ph_ctx *ctx, uint32_t out_w, uint32_t out_h, ChanJobPlan &P) {
  char where[24];
  snprintf(where, sizeof where, "job %d: ", j);
  if (!J.layers || !J.outs) return fail(PH_E_INVALID, "%s: %sNULL argument", fn, where);
  if (J.n_out < 1 || J.n_out > max_outs) return fail(PH_E_INVALID, "%s: %s1..%d outputs (%d)", fn, where, max_outs, J.n_out);
  if (J.n < 1 || J.n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: %s1..%d layers", fn, where, ph::kMaxLayers);
  P.table = J.outs[0].wr_gamma_lut;
  for (int k = 0; k < J.n_out; ++k) {
    const ph_chan_output &o = J.outs[k];
    if (const int bad = chan_output_check(fn, where, k, o, out_w, out_h)) return bad;
    for (int i = 0; i < k; ++i)
      if (J.outs[i].planes[0] == o.planes[0]) return fail(PH_E_INVALID, "%s: %soutputs %d and %d name the same plane", fn, where, i, k);
    if (ctx && !lds_view(ctx, o.wr_gamma_lut).found)
      return fail(PH_E_INVALID, "%s: %soutput %d: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn, where, k);
    P.any_v210 = P.any_v210 || o.format == PH_FMT_V210;
    P.same_lines = P.same_lines && o.interlace == J.outs[0].interlace;
    if (o.wr_gamma_lut != P.table) P.table = nullptr;
    span_write_output(P.print, o, out_w, out_h);
  }
  P.interlace = P.same_lines ? J.outs[0].interlace : 0u;
  // the layers, as the channel kernel's entries check them (their texts); what the job reads
  if (const int bad = chan_ops(J.n, J.layers, out_w, out_h, P.one.op, P.one.plane_u, P.one.plane_v, P.one.cm_op, &P.one.planar, &P.n_ops)) return bad;
  for (int i = 0; i < P.n_ops; ++i) {
    const ph::ChanSrc &src = P.one.op[i].src;
    const bool v420 = src.kind == ph::kChanP8x420 || src.kind == ph::kChanNv12 || src.kind == ph::kChanP10x420 || src.kind == ph::kChanP010;
    span_read_planes(P.print, src.ptr, src.pitch, src.h, v420, /*cbcr*/ src.kind == ph::kChanNv12 || src.kind == ph::kChanP010, P.one.plane_u[i], P.one.plane_v[i]);
  }
  return PH_OK;
}

int ph_chan_compose_batch_out(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job_out *jobs, uint32_t out_w, uint32_t out_h, const void *rd_cm,
                              const void *rd_lut, const void *rd_gm) {
  static const char *const fn = "ph_chan_compose_batch_out";
  if (!ctx) {  // (a caller whose ph_ctx_create found no device gets that answer here too: there is no CPU path)
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(PH_E_NO_DEVICE, "%s: no HIP device available; libphaneron_hip has no CPU path", fn);
  }
  if (!ctx || !jobs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  PH_QUEUE(fn, queue);
  if (n_jobs < 1) return fail(PH_E_INVALID, "%s: no jobs", fn);
  if (!out_w) return fail(PH_E_INVALID, "%s: width 0", fn);
  const LutRef rref = lds_view(ctx, rd_lut);
  if (!rref.get()) return fail(PH_E_INVALID, "%s: the reader gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn);
  std::vector<ChanJobPlan> plan((size_t)n_jobs);
  uint32_t plan_jobs = 0, plan_ops = 0, plan_outs = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const ph_chan_job_out &J = jobs[j];
    ChanJobPlan &P = plan[(size_t)j];
    if (const int bad = chan_job_check(fn, j, J, ph::kMaxChanOuts, ctx, out_w, out_h, P)) return bad;
    // what the shared launch takes: one writer table, a program and outputs that fit, lines to compose - and not the one v210 frame
    // that the enlarged-clip routes make better (ph_chan_compose takes them; with several outputs nobody does)
    const ph_chan_output &o0 = J.outs[0];
    const bool enlarged = J.n_out == 1 && o0.format == PH_FMT_V210 && o0.wr_col_matrix12 && ctx->chan_enlarged &&
                          chan_layers_enlarged(J.n, J.layers, out_w, out_h, o0.interlace);
    uint32_t own_cms = 0;  // (an over-estimate: the same matrix named twice counts twice)
    for (int i = 0; i < P.n_ops; ++i) own_cms += P.one.cm_op[i] && P.one.cm_op[i] != (const float *)rd_cm ? 1u : 0u;
    P.joins = chan_batch_on() && P.table && P.n_ops <= ph::kMaxChanOutOps && own_cms <= 8u && (P.interlace ? out_h / 2 : out_h) && !enlarged;
    if (P.joins) ++plan_jobs, plan_ops += (uint32_t)P.n_ops, plan_outs += (uint32_t)J.n_out;
  }
  int rc = set_device(ctx);
  if (rc) return rc;
  // how many jobs a launch should take so that the launches come out even (five jobs are 3 + 2, not 4 + 1: a job alone shares nothing)
  auto over = [](uint32_t n, int per) { return (n + (uint32_t)per - 1u) / (uint32_t)per; };
  uint32_t launches = over(plan_jobs, ph::kMaxChanOutJobs);
  launches = std::max(launches, std::max(over(plan_ops, ph::kMaxChanOutOps), over(plan_outs, ph::kMaxChanBatchOuts)));
  const uint32_t jobs_per_launch = launches ? (plan_jobs + launches - 1u) / launches : 1u;
  auto hand_on = [&](int j) {
    const ph_chan_job_out &J = jobs[j];
    return ph_chan_compose_multi(ctx, queue, J.n, J.layers, J.n_out, J.outs, out_w, out_h, rd_cm, rd_lut, rd_gm);
  };
  // the launch being collected: its jobs [first_job, first_job + b.jobs), its writer table (a copy that holds across the jobs handed on) and its lines
  ph::ChanBatchOutArgs b{};
  int first_job = 0;
  const void *table = nullptr;
  LutRef wref;
  uint32_t planar = 0;
  bool fields = false, any_v210 = false;  // fields: the launch's jobs compose one field each (of either parity: a job's first line is its own)
  auto flush = [&]() -> int {
    if (!b.jobs) return PH_OK;
    const uint32_t n_launch = b.jobs;
    b.jobs = 0;
    if (n_launch == 1) {
      b = ph::ChanBatchOutArgs{};
      return hand_on(first_job);
    }
    b.jobs = n_launch;
    b.out_w = out_w, b.out_h = out_h, b.line_step = fields ? 2 : 1, b.lines = fields ? out_h / 2 : out_h;
    b.rd_cm = (const float *)rd_cm, b.rd_gm = (const float *)rd_gm, b.rd = rref.view, b.wr = wref.view;
    if (any_v210 && out_w % 48 && planar < 1) planar = 1;  // as ph_chan_compose: the tail instantiation writes lines that end in a tail / cleared slots
    b.tails = planar >= 1 ? 1u : 0u, b.planar = planar == 2 ? 1u : 0u;
    b.out_tail_from = any_v210 && out_w % 6 ? out_w - out_w % 6u : 0xFFFFFFFFu;
    for (uint32_t k = 0; k < b.n_out; ++k) {
      ph::ChanBatchOut &d = b.out[k];
      d.tail_from = d.fmt == PH_FMT_V210 ? b.out_tail_from : 0xFFFFFFFFu;
      d.round = d.fmt != PH_FMT_V210 && b.out_tail_from != 0xFFFFFFFFu ? 1u : 0u;
    }
    const size_t each = (ph::chan_index_bytes(out_w, b.lines) + 255u) & ~(size_t)255u;
    const int r = with_scratch(fn, ctx, queue, each * b.jobs, [&](hipStream_t s, void *area) {
      for (uint32_t j = 0; j < b.jobs; ++j) b.job[j].index = (char *)area + each * j;
      return ph::launch_chan_compose_batch_out(s, b, (uint32_t)ctx->props.multiProcessorCount);
    });
    b = ph::ChanBatchOutArgs{};
    return r;
  };
  for (int j = 0; j < n_jobs; ++j) {
    const ph_chan_job_out &J = jobs[j];
    const ChanJobPlan &P = plan[(size_t)j];
    if (!P.joins) {  // in its turn, on its own
      if ((rc = flush())) return rc;
      if ((rc = hand_on(j))) return rc;
      continue;
    }
    // no job of a launch reads or writes what another job of it writes (two fields of one frame excepted): such a job starts the next launch
    bool clash = false;
    for (int i = first_job; i < first_job + (int)b.jobs && !clash; ++i) clash = clashes(P.print, plan[(size_t)i].print, kAllHazards, /*fields_interleave*/ true);
    // the job's Loader matrices as indices into the launch's small table
    uint8_t cm_of[ph::kMaxChanOps] = {};
    const float *tab[8];
    if (b.jobs && (clash || P.table != table || (P.interlace != 0) != fields || b.jobs >= jobs_per_launch || b.n_ops + (uint32_t)P.n_ops > (uint32_t)ph::kMaxChanOutOps ||
                   b.n_out + (uint32_t)J.n_out > (uint32_t)ph::kMaxChanBatchOuts || !place_cms(P.n_ops, P.one.cm_op, rd_cm, b.cm_tab, tab, cm_of)))
      if ((rc = flush())) return rc;
    if (!b.jobs) {
      first_job = j, table = P.table, wref = lds_view(ctx, table), fields = P.interlace != 0, planar = 0, any_v210 = false;
      if (!wref.found) return fail(PH_E_INVALID, "%s: job %d: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn, j);
    }
    place_cms(P.n_ops, P.one.cm_op, rd_cm, b.cm_tab, tab, cm_of);  // (fits an empty table: the job has at most eight matrices of its own)
    for (int t = 0; t < 8; ++t) b.cm_tab[t] = tab[t];
    planar = std::max(planar, P.one.planar), any_v210 = any_v210 || P.any_v210;
    ph::ChanJob &jb = b.job[b.jobs];
    jb.first_op = b.n_ops, jb.n_ops = (uint32_t)P.n_ops, jb.first_line = P.interlace == 3 ? 1u : 0u;
    for (int i = 0; i < P.n_ops; ++i) {
      const uint32_t at = b.n_ops + (uint32_t)i;
      b.op[at] = P.one.op[i], b.op_job[at] = (uint8_t)b.jobs;
      b.plane_u[at] = P.one.plane_u[i], b.plane_v[at] = P.one.plane_v[i], b.cm_idx[at] = cm_of[i];
      b.any_cm |= cm_of[i] ? 1u : 0u;
    }
    for (int k = 0; k < J.n_out; ++k) {
      const ph_chan_output &o = J.outs[k];
      ph::ChanBatchOut &d = b.out[b.n_out++];
      d.fmt = (uint32_t)o.format;
      d.pitch = o.format == PH_FMT_V210 ? ph_v210_pitch_bytes(out_w) / 16u : out_w;
      d.plane[0] = o.planes[0], d.plane[1] = o.planes[1], d.plane[2] = o.planes[2];
      out_lines(o, P.same_lines, out_h, d);
      d.job = b.jobs;
      d.wr_cm = (const float *)(o.wr_col_matrix12 ? o.wr_col_matrix12 : rd_cm);
    }
    b.n_ops += (uint32_t)P.n_ops, ++b.jobs;
  }
  return flush();
}

int ph_yadif(ph_ctx *ctx, int queue, const void *prev, const void *cur, const void *next, int w, int h, int parity,
             int tff, int skip, void *out) {
  if (!prev || !cur || !next || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_yadif: NULL/zero argument");
  PH_LAUNCH(ph::launch_yadif(stream_of(ctx, queue), prev, cur, next, w, h, parity, tff ? 1 : 0, skip ? 1 : 0, out));
}

int ph_yadif_pair(ph_ctx *ctx, int queue, const void *prev, const void *cur, const void *next, int w, int h, int tff,
                  int skip, void *out_parity0, void *out_parity1) {
  if (!prev || !cur || !next || !out_parity0 || !out_parity1 || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_yadif_pair: NULL/zero argument");
  if (out_parity0 == out_parity1) return fail(PH_E_INVALID, "ph_yadif_pair: the two outputs are the same buffer");
  PH_LAUNCH(ph::launch_yadif_pair(stream_of(ctx, queue), prev, cur, next, w, h, tff ? 1 : 0, skip ? 1 : 0, out_parity0, out_parity1));
}

int ph_v210_yadif_pair(ph_ctx *ctx, int queue, int n, const ph_deint_source *src, uint32_t width, uint32_t height, int tff,
                       int skip, const void *cm, const void *lut, const void *gm) {
  return ph_v210_yadif_pair_fmt(ctx, queue, n, src, width, height, tff, skip, PH_IMG_RGBA_F32, cm, lut, gm);
}

// the layers of `jobs` sets (the same count, formats, sizes and placements; 1 <= n <= kMaxLayers checked) into a launch's arguments
static int compose_up_layers(const char *fn, int jobs, int n, const ph_image_layer *const *sets, ph::UpArgs &a, int *image_fmt) {
  const ph_image_layer *layers = sets[0];
  a.n = n;
  const int fmt = layers[0].format;
  if (fmt != PH_IMG_RGBA_F32 && fmt != PH_IMG_RGB_F32) return fail(PH_E_INVALID, "%s: image format %d", fn, fmt);
  for (int i = 0; i < n; ++i) {
    const ph_image_layer &L = layers[i];
    if (!L.data || L.width <= 0 || L.height <= 0 || !L.matrix9_host) return fail(PH_E_INVALID, "%s: layer %d is incomplete", fn, i);
    if (L.format != fmt) return fail(PH_E_INVALID, "%s: layer %d has another image format than layer 0", fn, i);
    a.layer[i].ptr = L.data, a.layer[i].w = (uint32_t)L.width, a.layer[i].h = (uint32_t)L.height;
    a.layer[i].pitch = (uint32_t)L.width * (fmt == PH_IMG_RGB_F32 ? 12u : 16u);
    for (int k = 0; k < 6; ++k) a.layer[i].m[k] = L.matrix9_host[k];
    for (int j = 1; j < jobs; ++j) {
      const ph_image_layer &B = sets[j][i];
      if (!B.data || !B.matrix9_host || B.format != L.format || B.width != L.width || B.height != L.height)
        return fail(PH_E_INVALID, jobs == 2 ? "%s: layer %d of the second set differs from the first in more than its data" : "%s: layer %d of a further set differs from the first in more than its data", fn, i);
      for (int k = 0; k < 9; ++k)
        if (B.matrix9_host[k] != L.matrix9_host[k])
          return fail(PH_E_INVALID, jobs == 2 ? "%s: layer %d of the second set is placed differently" : "%s: layer %d of a further set is placed differently", fn, i);
      a.more_ptr[j - 1][i] = B.data;
    }
  }
  a.jobs = (uint32_t)jobs;
  *image_fmt = fmt;
  return PH_OK;
}
static void compose_up_lines(ph::UpArgs &a, uint32_t out_w, uint32_t out_h, uint32_t interlace) {
  a.out_w = out_w, a.out_h = out_h;
  a.line_step = interlace ? 2 : 1, a.first_line = (interlace == 3) ? 1 : 0;
  a.lines = interlace ? out_h / 2 : out_h;
}
static int compose_up_not_eligible(const char *fn) {
  return fail(PH_E_INVALID, "%s: every layer must be enlarged (by 1 %% or more in both directions, per written row) without "
                            "rotation or mirroring and be below 1 GiB; use ph_compose_write_v210", fn);
}

// `jobs` sets of layers that differ in their data only (same count, formats, sizes and placements), each into its own output: one launch
static int compose_up_common(const char *fn, ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *sets, void *const *outs,
                             uint32_t out_w, uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  if (!ctx || !sets || !outs || !wr_cm || !wr_lut) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (jobs < 1 || jobs > ph::kMaxUpJobs) return fail(PH_E_INVALID, "%s: 1..%d jobs", fn, ph::kMaxUpJobs);
  for (int j = 0; j < jobs; ++j)
    if (!sets[j] || !outs[j]) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  // (a width that is not a multiple of 48 - 1280 - ends its lines in a tail quad and cleared slots: the kernel's TAILS instantiation)
  if (!out_w || out_w % 2) return fail(PH_E_INVALID, "%s: width %u is odd (a v210 frame needs an even width); run the separate kernels", fn, out_w);
  if (interlace != 0 && interlace != 1 && interlace != 3) return fail(PH_E_INVALID, "%s: interlace must be 0, 1 or 3", fn);
  for (int j = 1; j < jobs; ++j)
    for (int k = 0; k < j; ++k)
      if (outs[j] == outs[k]) return fail(PH_E_INVALID, jobs == 2 ? "%s: the two outputs are the same buffer" : "%s: two jobs have the same output buffer", fn);
  const LutRef wref = lds_view(ctx, wr_lut);
  const ph::LutView *wv = wref.get();
  if (!wv) return fail(PH_E_INVALID, "%s: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn);
  ph::UpArgs a{};
  int fmt = 0;
  const int lrc = compose_up_layers(fn, jobs, n, sets, a, &fmt);
  if (lrc) return lrc;
  a.out = outs[0];
  for (int j = 1; j < jobs; ++j) a.more_out[j - 1] = outs[j];
  compose_up_lines(a, out_w, out_h, interlace);
  a.wr_cm = (const float *)wr_cm, a.wr = *wv;
  if (!ph::compose_up_eligible(a)) return compose_up_not_eligible(fn);
  if (!a.lines) return PH_OK;
  PH_LAUNCH(ph::launch_compose_up_write_v210(stream_of(ctx, queue), a, fmt == PH_IMG_RGB_F32, (uint32_t)ctx->props.multiProcessorCount));
}

int ph_compose_up_write_v210(ph_ctx *ctx, int queue, int n, const ph_image_layer *layers, void *out, uint32_t out_w, uint32_t out_h,
                             uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  if (!layers || !out) return fail(PH_E_INVALID, "ph_compose_up_write_v210: NULL argument");
  return compose_up_common("ph_compose_up_write_v210", ctx, queue, 1, n, &layers, &out, out_w, out_h, interlace, wr_cm, wr_lut);
}

int ph_compose_up_write_v210_pair(ph_ctx *ctx, int queue, int n, const ph_image_layer *layers_a, const ph_image_layer *layers_b, void *out_a, void *out_b,
                                  uint32_t out_w, uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  if (!layers_a || !layers_b || !out_a || !out_b) return fail(PH_E_INVALID, "ph_compose_up_write_v210_pair: NULL argument");
  const ph_image_layer *sets[2] = {layers_a, layers_b};
  void *outs[2] = {out_a, out_b};
  return compose_up_common("ph_compose_up_write_v210_pair", ctx, queue, 2, n, sets, outs, out_w, out_h, interlace, wr_cm, wr_lut);
}

int ph_compose_up_write_v210_batch(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *layer_sets, void *const *outs, uint32_t out_w,
                                   uint32_t out_h, uint32_t interlace, const void *wr_cm, const void *wr_lut) {
  return compose_up_common("ph_compose_up_write_v210_batch", ctx, queue, jobs, n, layer_sets, outs, out_w, out_h, interlace, wr_cm, wr_lut);
}

// the outputs of a several-consumers call of the 2 x 2-block compositor (jobs x n_out entries, job-major; both counts are checked by the
// caller): every check of the frame's width and of an output that needs no context ...
static int compose_up_outputs(const char *fn, int jobs, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h) {
  if (!out_w || out_w % 2) return fail(PH_E_INVALID, "%s: width %u is odd (a block is two pixels wide); run the separate kernels", fn, out_w);
  for (int k = 0; k < n_out; ++k) {
    const ph_chan_output &o = outs[k];
    if (!o.planes[0] || !o.wr_gamma_lut) return fail(PH_E_INVALID, "%s: output %d: NULL argument", fn, k);
    if (!fmt_known(o.format)) return fail(PH_E_INVALID, "%s: output %d: format %d is not a PH_FMT_*", fn, k, o.format);
    if (!fmt_chan_out(o.format))
      return fail(PH_E_INVALID, "%s: output %d: the compositor does not write %s frames - run the separate kernels: the frame as an image, then the format's writer (ph_pack_write)", fn, k,
                  fmt_name(o.format));
    if (!fmt_rgb8(o.format) && !o.wr_col_matrix12) return fail(PH_E_INVALID, "%s: output %d: the writer's RGB -> YCbCr matrix is missing", fn, k);
    if (fmt_v420(o.format) && (out_h & 1)) return fail(PH_E_INVALID, "%s: output %d: a 4:2:0 frame needs an even height (%u)", fn, k, out_h);
    if (fmt_planar(o.format) && out_w % 8)
      return fail(PH_E_INVALID, "%s: output %d: width %u (a planar frame needs a multiple of 8); run the separate kernels", fn, k, out_w);
    if (o.interlace != 0 && o.interlace != 1 && o.interlace != 3) return fail(PH_E_INVALID, "%s: output %d: interlace must be 0, 1 or 3", fn, k);
    for (int j = 0; j < jobs; ++j) {
      const ph_chan_output &b = outs[j * n_out + k];
      if (b.format != o.format || b.interlace != o.interlace || b.wr_col_matrix12 != o.wr_col_matrix12 || b.wr_gamma_lut != o.wr_gamma_lut)
        return fail(PH_E_INVALID, "%s: output %d of job %d differs from job 0's in more than its planes", fn, k, j);
      if (!b.planes[0] || (fmt_planar(o.format) && (!b.planes[1] || (fmt_planes(o.format) == 3 && !b.planes[2]))))
        return fail(PH_E_INVALID, "%s: output %d: a planar output needs its three planes (nv12: Y and the interleaved CbCr plane)", fn, k);
      for (int i = 0; i < j * n_out + k; ++i)
        if (outs[i].planes[0] == b.planes[0]) return fail(PH_E_INVALID, "%s: outputs %d and %d name the same plane", fn, i, j * n_out + k);
    }
  }
  return PH_OK;
}
// ... then each output's writer table in its LDS form into wref[k]
static int compose_up_tables(const char *fn, ph_ctx *ctx, int n_out, const ph_chan_output *outs, LutRef *wref) {
  for (int k = 0; k < n_out; ++k) {
    wref[k] = lds_view(ctx, outs[k].wr_gamma_lut);
    if (!wref[k].get())
      return fail(PH_E_INVALID, "%s: output %d: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn, k);
  }
  return PH_OK;
}

// an output of the several-outputs kernels' launches, job 0's planes (a further job's: the caller's to add)
static ph::UpOut up_out_of(const ph_chan_output &o, bool same_lines, uint32_t out_w, uint32_t out_h) {
  ph::UpOut d{};
  d.fmt = (uint32_t)o.format;
  d.pitch = o.format == PH_FMT_V210 ? out_w / 6u : out_w;  // (planar: a multiple of 8, no padding; v210 here: a multiple of 48 - or the launcher's to set)
  d.wr_cm = (const float *)o.wr_col_matrix12;
  for (int i = 0; i < 3; ++i) d.plane[0][i] = o.planes[i];
  out_lines(o, same_lines, out_h, d);
  return d;
}

struct UpLaunch {
  bool solo;  // compose_up_write_v210_kernel: m.up alone
  int table;  // the first output that names the launch's writer table (m.up.wr: the caller's to fill)
  ph::UpMultiArgs m;
};
// the launches of such a call: per writer table, in the order the tables first appear, a v210 output that cannot share (its lines end in a tail quad,
// or nobody else names its table) through the one-output kernel, then the rest as one several-outputs launch.  split_v210 == false (layers in a
// transition, which the one-output kernel does not have): every output of a table stays in the table's launch.  keep_tails (context option
// "up_v210_tails"): a v210 output whose lines end in a tail quad stays with the others of its table - alone with its table it is split off as ever
static void compose_up_launches(const ph::UpArgs &base, int jobs, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                                bool split_v210, std::vector<UpLaunch> &launches, bool keep_tails = false) {
  int order[ph::kMaxUpOuts], start[ph::kMaxUpOuts + 1];
  const int groups = writer_table_groups(n_out, outs, order, start);
  for (int t = 0; t < groups; ++t) {
    const int *const group = order + start[t], members = start[t + 1] - start[t], k = group[0];
    UpLaunch shared{};
    const ph_chan_output *stays[ph::kMaxUpOuts];  // the outputs of shared.m.out
    shared.solo = false, shared.table = k, shared.m.up = base;
    for (int g = 0; g < members; ++g) {
      const ph_chan_output &o = outs[group[g]];
      if (split_v210 && o.format == PH_FMT_V210 && ((out_w % 48 && !keep_tails) || members == 1)) {
        UpLaunch own{};
        own.solo = true, own.table = k, own.m.up = base, own.m.up.wr_cm = (const float *)o.wr_col_matrix12;
        own.m.up.out = o.planes[0];
        for (int j = 1; j < jobs; ++j) own.m.up.more_out[j - 1] = outs[j * n_out + group[g]].planes[0];
        compose_up_lines(own.m.up, out_w, out_h, o.interlace);
        launches.push_back(own);
        continue;
      }
      ph::UpOut &d = shared.m.out[shared.m.n_out];
      d = up_out_of(o, true, out_w, out_h);  // (takes / line_end / field: settled below, once the launch's lines are known)
      for (int j = 1; j < jobs; ++j)
        for (int i = 0; i < 3; ++i) d.plane[j][i] = outs[j * n_out + group[g]].planes[i];
      stays[shared.m.n_out++] = &o;
    }
    if (!shared.m.n_out) continue;
    // a split-off v210 output does not count: the first output that stays decides what "the same" is
    bool same_lines = true;
    for (uint32_t i = 0; i < shared.m.n_out; ++i) same_lines = same_lines && stays[i]->interlace == stays[0]->interlace;
    compose_up_lines(shared.m.up, out_w, out_h, same_lines ? stays[0]->interlace : 0u);
    for (uint32_t i = 0; i < shared.m.n_out; ++i) out_lines(*stays[i], same_lines, out_h, shared.m.out[i]);
    launches.push_back(shared);
  }
}

/* Several consumers' frames of one enlarged composition: see include/phaneron_hip.h.  Every check is made, and every launch of the call
 * is planned, before anything is launched. */
// keep_tails: the context option "up_v210_tails" as this call sees it - the transition entry's all-cuts call passes false, whatever the option says
static int compose_up_write_multi(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *layer_sets, int n_out, const ph_chan_output *outs,
                                  uint32_t out_w, uint32_t out_h, bool keep_tails) {
  const char *const fn = "ph_compose_up_write_multi";
  if (!ctx || !layer_sets || !outs) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n_out < 1 || n_out > ph::kMaxUpOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxUpOuts, n_out);
  if (jobs < 1 || jobs > ph::kMaxUpJobs) return fail(PH_E_INVALID, "%s: 1..%d jobs (%d)", fn, ph::kMaxUpJobs, jobs);
  if (jobs == 1 && n_out == 1 && outs[0].format == PH_FMT_V210)
    return ph_compose_up_write_v210(ctx, queue, n, layer_sets[0], outs[0].planes[0], out_w, out_h, outs[0].interlace, outs[0].wr_col_matrix12, outs[0].wr_gamma_lut);
  PH_QUEUE(fn, queue);
  for (int j = 0; j < jobs; ++j)
    if (!layer_sets[j]) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  LutRef wref[ph::kMaxUpOuts];
  int rc = compose_up_outputs(fn, jobs, n_out, outs, out_w, out_h);
  if (!rc) rc = compose_up_tables(fn, ctx, n_out, outs, wref);
  if (rc) return rc;
  ph::UpArgs base{};
  int fmt = 0;
  rc = compose_up_layers(fn, jobs, n, layer_sets, base, &fmt);
  if (rc) return rc;
  std::vector<UpLaunch> launches;
  compose_up_launches(base, jobs, n_out, outs, out_w, out_h, true, launches, keep_tails);
  for (UpLaunch &l : launches) {
    l.m.up.wr = *wref[l.table].get();
    if (!ph::compose_up_eligible(l.m.up)) return compose_up_not_eligible(fn);
  }
  rc = set_device(ctx);
  if (rc) return rc;
  for (const UpLaunch &l : launches) {
    if (!l.m.up.lines) continue;
    hipError_t e = hipSuccess;
    if (!l.solo) e = ph::launch_compose_up_multi(stream_of(ctx, queue), l.m, fmt == PH_IMG_RGB_F32, (uint32_t)ctx->props.multiProcessorCount, keep_tails);
    else if (!ph::trace_launch("compose_up_write_v210"))
      e = ph::launch_compose_up_write_v210(stream_of(ctx, queue), l.m.up, fmt == PH_IMG_RGB_F32, (uint32_t)ctx->props.multiProcessorCount);
    if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  }
  return PH_OK;
}
int ph_compose_up_write_multi(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *layer_sets, int n_out, const ph_chan_output *outs,
                              uint32_t out_w, uint32_t out_h) {
  return compose_up_write_multi(ctx, queue, jobs, n, layer_sets, n_out, outs, out_w, out_h, ctx && ctx->up_v210_tails);
}

// What the clip entries and ph_clip_compose_batch_out's planner make of a clip (of an output: up_out_of, above): its size and placement as a
// compositor layer (ptr: the launch's own), ...
static ph::UpLayer up_layer_of(const ph_chan_source &S) {
  ph::UpLayer d{};
  d.w = (uint32_t)S.width, d.h = (uint32_t)S.height, d.pitch = (uint32_t)S.width * 16u;
  for (int k = 0; k < 6; ++k) d.m[k] = S.matrix9_host[k];
  return d;
}
// ... and the clip itself in its wire format fmt, as the clip kernel reads it
static ph::ClipSrc clip_src_of(const ph_chan_source &S, int fmt, const void *rd_cm) {
  return ph::ClipSrc{S.data, S.data_u, S.data_v, (const float *)(S.col_matrix12 ? S.col_matrix12 : rd_cm), (uint32_t)fmt,
                     fmt == PH_FMT_V210 ? ph_v210_pitch_bytes((uint32_t)S.width) / 16u : ph::pack_pitch(fmt, (uint32_t)S.width)};
}

// ---- what the file playback entries share ------------------------------------------------------------------------------------------------
// The argument checks of a clip call, in the entries' order and with their texts: NULLs, the counts, the outputs, then the layers as the
// channel kernel's entries check them.  The context is not looked at.  route: ph_clip_compose_route_multi's form - clip_route_counts has
// seen its counts, and a call without outputs need not name any
static int clip_args_check(const char *fn, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                           const void *rd_cm, const void *rd_lut, const void *rd_gm, bool route = false) {
  if (!layers || (!outs && !(route && !n_out)) || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (!route && (n_out < 1 || n_out > ph::kMaxUpOuts)) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxUpOuts, n_out);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  if (const int bad = fused_multi_outputs_check(fn, queue, n_out, outs, out_w, out_h)) return bad;
  ph::ChanArgs probe{};
  int n_ops = 0;
  return chan_ops(n, layers, out_w, out_h, probe.op, probe.plane_u, probe.plane_v, probe.cm_op, &probe.planar, &n_ops);
}
// The lines a launch for several outputs composes: the field every output wants (*same_lines; the answer is its interlace value), or the
// whole frame (0) - a field output then takes the rows of its parity
static uint32_t lines_composed(int n_out, const ph_chan_output *outs, bool *same_lines) {
  *same_lines = true;
  for (int k = 1; k < n_out; ++k) *same_lines = *same_lines && outs[k].interlace == outs[0].interlace;
  return *same_lines ? (uint32_t)outs[0].interlace : 0u;
}
// Is the image a clip in a wire format the clip kernel reads (v210 included; a 4:2:0 one needs an even height)?  *alpha: it carries alpha
static bool clip_wire(const ph_chan_source &S, bool *alpha) {
  const int fmt = fmt_of_src(S.format);
  *alpha = fmt_rgb8(fmt);
  return fmt >= 0 && !(fmt_v420(fmt) && (S.height & 1));
}
// Do the read-once routes take the outputs?  Each writer table in its LDS form into wref[k]; a planar frame's width must be a multiple of 8
static bool clip_tables_take(ph_ctx *ctx, int n_out, const ph_chan_output *outs, uint32_t out_w, LutRef *wref) {
  for (int k = 0; k < n_out; ++k) {
    wref[k] = lds_view(ctx, outs[k].wr_gamma_lut);
    if (!wref[k].get() || (fmt_planar(outs[k].format) && out_w % 8)) return false;
  }
  return true;
}
// A clip kernel launch's arguments (c: zeroed) from a writer table's group m, the reader's table and the frame's one clip S - as every
// clip entry and the batch planner make them (clip.scratch and the tiling: clip_up_plan's and the launch's)
static void clip_multi_fill(ph::ClipUpMultiArgs &c, const ph::UpMultiArgs &m, const ph::LutView &rd, const void *rd_gm, const ph_chan_source &S, const void *rd_cm) {
  c.clip.up = m.up, c.n_out = m.n_out;
  for (uint32_t i = 0; i < m.n_out; ++i) c.out[i] = m.out[i];
  c.clip.rd = rd, c.clip.rd_gm = (const float *)rd_gm;
  c.clip.src[0] = clip_src_of(S, fmt_of_src(S.format), rd_cm);
}

// The queue's scratch area through the launches of one clip call.  `images` is ctx->chan_scratch_mu[queue], held from the read of the
// clips into the queue's scratch images until the last compositor launch that takes them is enqueued - and never across ph_chan_compose
// or with_scratch, which take the area (and the lock) themselves: the images are given up in front of those.  RELEASED MEANS GONE: the
// next group that needs the images reads them again.
extern "C++" {
struct ClipScratch {
  const char *fn;
  ph_ctx *ctx;
  int queue;
  std::unique_lock<std::mutex> images;
  void *image[ph::kMaxLayers * 3];  // where the compositor finds the images read last
  void release() {
    if (images.owns_lock()) images.unlock();
  }
  // one launch of a clip kernel, planned with `grid` workgroups (clip_up_plan): launch(stream) enqueues it, clip.scratch set
  template <class Launch>
  int one_launch(ph::ClipUpArgs &clip, uint32_t grid, Launch launch) {
    release();
    return with_scratch(fn, ctx, queue, (size_t)clip.wg_bytes * grid + 4096u, [&](hipStream_t s, void *area) {
      clip.scratch = (char *)area;
      return launch(s);
    });
  }
  // the first of the two stages: every image through its format's reader into the queue's scratch images (image[f]: srcs[f]'s) - unless
  // they are still held from an earlier group of the call
  int images_for_two_stages(int n_img, const ph_chan_source *const *srcs, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
    if (images.owns_lock()) return PH_OK;
    images = std::unique_lock<std::mutex>(ctx->chan_scratch_mu[queue]);
    return chan_images_read(ctx, queue, 1, n_img, srcs, rd_cm, rd_lut, rd_gm, image);
  }
};
}
// The outputs of a clip call by writer table, in the order the tables first appear: group(m, tails) makes a table's launch(es) - m.up is
// base with the table, m.out the outputs that stay.  A v210 output whose lines end in a tail quad truncates its table indices there where
// the other writers round: through ph_chan_compose, alone, in its turn - unless keep_tails and another output names its table: then it
// stays in the group, whose launch is the kernels' TAILS form (tails; clip_up_multi_t / compose_up_multi_t).  wref[k]: output k's table
extern "C++" template <class Group>
static int clip_groups(ClipScratch &scratch, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                       const void *rd_cm, const void *rd_lut, const void *rd_gm, const ph::UpArgs &base, const LutRef *wref, bool same_lines, bool keep_tails,
                       Group group) {
  ph_ctx *const ctx = scratch.ctx;
  const int queue = scratch.queue;
  int order[ph::kMaxUpOuts], start[ph::kMaxUpOuts + 1];
  const int groups = writer_table_groups(n_out, outs, order, start);
  for (int g = 0; g < groups; ++g) {
    ph::UpMultiArgs m{};
    m.up = base, m.up.wr = *wref[order[start[g]]].get();
    bool tails = false;  // the group's launch has a v210 output whose lines end in a tail quad
    for (int i = start[g]; i < start[g + 1]; ++i) {
      const ph_chan_output &o = outs[order[i]];
      if (o.format == PH_FMT_V210 && out_w % 48) {
        if (!(keep_tails && start[g + 1] - start[g] >= 2)) {
          scratch.release();
          const int rc = ph_chan_compose(ctx, queue, n, layers, PH_FMT_V210, o.planes, out_w, out_h, o.interlace, rd_cm, rd_lut, rd_gm, o.wr_col_matrix12, o.wr_gamma_lut);
          if (rc) return rc;
          continue;
        }
        tails = true;
      }
      m.out[m.n_out++] = up_out_of(o, same_lines, out_w, out_h);
    }
    if (!m.n_out) continue;
    if (const int rc = group(m, tails)) return rc;
  }
  return PH_OK;
}
// A group's launch by ph_clip_compose_multi's routes.  one_launch: the frame is a single clip in a wire format (alpha: one that carries
// alpha) - one launch of the clip kernel, where it has a tiling; else the two stages: the clips into the queue's scratch images, then the
// 2 x 2-block compositor's launch.  image_out (ph_clip_compose_route_multi's first launch): the launch stores the combined image too
static int clip_group_launch(ClipScratch &scratch, bool one_launch, bool alpha, int n, const ph_chan_layer *layers, const void *rd_cm, const void *rd_lut,
                             const void *rd_gm, const ph::LutView &rd, ph::UpMultiArgs &m, bool tails, void *image_out) {
  ph_ctx *const ctx = scratch.ctx;
  const uint32_t cus = (uint32_t)ctx->props.multiProcessorCount;
  if (one_launch) {
    ph::ClipUpRouteArgs r{};
    ph::ClipUpMultiArgs &c = r.multi;
    clip_multi_fill(c, m, rd, rd_gm, layers[0].src, rd_cm);
    r.image = image_out;
    const uint32_t grid = ph::clip_up_plan(c.clip, !alpha, cus, /*v210_tails*/ tails);
    if (grid)
      return scratch.one_launch(c.clip, grid, [&](hipStream_t s) {
        return image_out ? ph::launch_clip_up_route(s, r, !alpha, grid) : ph::launch_clip_up_multi(s, c, !alpha, grid, tails);
      });
  }
  const ph_chan_source *srcs[ph::kMaxLayers];
  for (int i = 0; i < n; ++i) srcs[i] = &layers[i].src;
  if (const int bad = scratch.images_for_two_stages(n, srcs, rd_cm, rd_lut, rd_gm)) return bad;
  for (int i = 0; i < n; ++i) m.up.layer[i].ptr = scratch.image[i];
  hipError_t e;
  if (image_out) {
    ph::UpRouteArgs r{};
    r.multi = m, r.image = image_out;
    e = ph::launch_compose_up_route(stream_of(ctx, scratch.queue), r, cus);
  } else {
    e = ph::launch_compose_up_multi(stream_of(ctx, scratch.queue), m, false, cus, tails);
  }
  return e == hipSuccess ? PH_OK : fail(PH_E_HIP, "%s: launch failed: %s", scratch.fn, hipGetErrorString(e));
}

/* File playback for any consumer, up to four per call: see include/phaneron_hip.h.  Exactly the n_out calls of ph_chan_compose in order,
 * bit for bit; every check is made before the context is looked at, and a refused call writes nothing.  An enlarged clip (or a decoder's
 * frame under the default fill) is read ONCE per source pixel instead of four times per output pixel: one launch of clip_up_multi_kernel
 * per writer table where the frame is a single wire-format clip, else the format readers into the queue's scratch images and one
 * compose_up_multi launch per table (n > 1: measured for v210 frames only - chan_compose_enlarged - tools/clip_multi_bench.py records
 * n = 2 both ways).  Whatever these routes do not take runs ph_chan_compose_multi on the same arguments inside the call. */
static int clip_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                              const void *rd_cm, const void *rd_lut, const void *rd_gm, bool keep_tails);
int ph_clip_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                          const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  return clip_compose_multi(ctx, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, ctx && ctx->up_v210_tails);
}
// keep_tails: the context option "up_v210_tails" as this call sees it - the transition and route entries' calls pass false, whatever the option says
static int clip_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w, uint32_t out_h,
                              const void *rd_cm, const void *rd_lut, const void *rd_gm, bool keep_tails) {
  const char *const fn = "ph_clip_compose_multi";
  if (const int bad = clip_args_check(fn, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm)) return bad;
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  // 1. a single v210 frame IS ph_chan_compose: today's routes under today's names
  if (n_out == 1 && outs[0].format == PH_FMT_V210)
    return ph_chan_compose(ctx, queue, n, layers, PH_FMT_V210, outs[0].planes, out_w, out_h, outs[0].interlace, rd_cm, rd_lut, rd_gm, outs[0].wr_col_matrix12,
                           outs[0].wr_gamma_lut);
  // 2. the lines composed
  bool same_lines;
  const uint32_t interlace = lines_composed(n_out, outs, &same_lines);
  // 3. not for these routes: the channel kernel, under its own trace name
  const LutRef rref = lds_view(ctx, rd_lut);
  LutRef wref[ph::kMaxUpOuts];
  bool takes = ctx->chan_enlarged != 0 && rref.get() && chan_layers_enlarged(n, layers, out_w, out_h, interlace, /*v210_fill*/ true) &&
               clip_tables_take(ctx, n_out, outs, out_w, wref);
  ph::UpArgs base{};
  if (takes) {
    base.n = n, base.jobs = 1;
    for (int i = 0; i < n; ++i) base.layer[i] = up_layer_of(layers[i].src);
    compose_up_lines(base, out_w, out_h, interlace);
    takes = ph::compose_up_eligible(base);
  }
  if (!takes) return ph_chan_compose_multi(ctx, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm);
  if (!base.lines) return PH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  // one launch of the clip kernel per table?  A single clip in a wire format
  bool alpha = false;
  const bool one_launch = ctx->chan_enlarged == 1 && n == 1 && clip_wire(layers[0].src, &alpha);
  // 4. the outputs by writer table, each group's launch in its turn (the clips are read once for all the call's two-stage groups)
  ClipScratch scratch{fn, ctx, queue};
  return clip_groups(scratch, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, base, wref, same_lines, keep_tails, [&](ph::UpMultiArgs &m, bool tails) {
    return clip_group_launch(scratch, one_launch, alpha, n, layers, rd_cm, rd_lut, rd_gm, rref.view, m, tails, /*image_out*/ nullptr);
  });
}

static bool chan_sources_same_shape(const ph_chan_source &a, const ph_chan_source &b) {
  if (a.width != b.width || a.height != b.height) return false;
  for (int k = 0; k < 9; ++k)
    if (a.matrix9_host[k] != b.matrix9_host[k]) return false;
  return true;
}

/* File playback through a MIX or WIPE, for up to four consumers: see include/phaneron_hip.h.  ph_clip_compose_multi's signature and contract -
 * exactly the n_out calls of ph_chan_compose in order, bit for bit; every check is made before the context is looked at, a refused call
 * writes nothing - with layers in a transition taken by the read-once routes too: every present image (a layer's src, a transition's
 * incoming image, a wipe's mask) must qualify as a src does for ph_clip_compose_multi.  One layer whose images are all wire-format clips:
 * one launch of clip_up_trans_kernel per writer table; else the format readers into the queue's scratch images (f32 RGBA, whatever the
 * clips' formats: the launch is the <rgba> one) and one compose_up_trans launch per table.  What these routes do not take runs
 * ph_chan_compose_multi on the same arguments inside the call. */
int ph_clip_compose_transition_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs, uint32_t out_w,
                                     uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = "ph_clip_compose_transition_multi";
  if (const int bad = clip_args_check(fn, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm)) return bad;
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  // 1. no transition: ph_clip_compose_multi, its routes under its names
  bool any = false;
  for (int i = 0; i < n; ++i) any = any || layers[i].transition != PH_TRANSITION_CUT;
  if (!any) return clip_compose_multi(ctx, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, /*keep_tails*/ false);
  // 2. the lines composed
  bool same_lines;
  const uint32_t interlace = lines_composed(n_out, outs, &same_lines);
  // 3. every present image, in the order layer by layer: src, incoming, mask
  const ph_chan_source *img[ph::kMaxLayers * 3];
  int first_img[ph::kMaxLayers], n_img = 0;
  for (int i = 0; i < n; ++i) {
    first_img[i] = n_img;
    img[n_img++] = &layers[i].src;
    if (layers[i].transition != PH_TRANSITION_CUT) img[n_img++] = &layers[i].incoming;
    if (layers[i].transition == PH_TRANSITION_WIPE) img[n_img++] = &layers[i].mask;
  }
  const LutRef rref = lds_view(ctx, rd_lut);
  LutRef wref[ph::kMaxUpOuts];
  bool takes = ctx->chan_enlarged != 0 && rref.get() && out_w % 2u == 0 && clip_tables_take(ctx, n_out, outs, out_w, wref);
  ph::UpArgs base{};
  base.n = n, base.jobs = 1;
  compose_up_lines(base, out_w, out_h, interlace);
  bool wire = true, alpha = false;  // every image in a wire format the clip kernel reads; one of them carries alpha
  for (int f = 0; f < n_img && takes; ++f) {
    const ph_chan_source &S = *img[f];
    takes = chan_image_enlarged(S, out_w, out_h, interlace, /*v210_fill*/ true);  // (it has a placement then)
    if (!takes) break;
    ph::UpArgs one = base;
    one.n = 1, one.layer[0] = up_layer_of(S);
    takes = ph::compose_up_eligible(one);
    bool its_alpha;
    wire = clip_wire(S, &its_alpha) && wire;
    alpha = alpha || its_alpha;
  }
  if (!takes) return ph_chan_compose_multi(ctx, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm);
  if (!base.lines) return PH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  const bool one_launch = ctx->chan_enlarged == 1 && n == 1 && wire;
  for (int i = 0; i < n; ++i) base.layer[i] = up_layer_of(layers[i].src);
  const uint32_t cus = (uint32_t)ctx->props.multiProcessorCount;
  // 4. the outputs by writer table, a v210 output whose lines end in a tail quad through ph_chan_compose, alone (ph_clip_compose_multi's route 4)
  ClipScratch scratch{fn, ctx, queue};
  return clip_groups(scratch, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, base, wref, same_lines, /*keep_tails*/ false, [&](ph::UpMultiArgs &m, bool) -> int {
    // 5. the group's one launch: a single layer, every image a clip in its wire format
    if (one_launch) {
      const ph_chan_layer &L = layers[0];
      ph::ClipUpTransArgs t{};
      ph::ClipUpMultiArgs &c = t.multi;
      clip_multi_fill(c, m, rref.view, rd_gm, L.src, rd_cm);
      t.kind = (uint32_t)L.transition, t.mix = L.mix;
      const ph_chan_source *const theirs[2] = {&L.incoming, &L.mask};
      for (int w = 0; w < (L.transition == PH_TRANSITION_WIPE ? 2 : 1); ++w) {
        t.partner[w] = up_layer_of(*theirs[w]);
        t.partner_src[w] = clip_src_of(*theirs[w], fmt_of_src(theirs[w]->format), rd_cm);
        t.same |= chan_sources_same_shape(*theirs[w], L.src) ? 1u << w : 0u;
      }
      const uint32_t grid = ph::clip_up_trans_plan(t, !alpha, cus);
      if (grid) return scratch.one_launch(c.clip, grid, [&](hipStream_t s) { return ph::launch_clip_up_trans(s, t, !alpha, grid); });
    }
    // 6. the two stages: every wire-format image through its format's reader into the queue's scratch images (finished f32 images as they
    // are), then the transition compositor's launch
    if (const int bad = scratch.images_for_two_stages(n_img, img, rd_cm, rd_lut, rd_gm)) return bad;
    void *const *const image = scratch.image;
    ph::UpTransArgs t{};
    t.multi = m;
    for (int i = 0; i < n; ++i) {
      const ph_chan_layer &L = layers[i];
      t.multi.up.layer[i].ptr = image[first_img[i]];
      t.kind[i] = (uint32_t)L.transition, t.mix[0][i] = L.mix;
      const ph_chan_source *const theirs[2] = {&L.incoming, &L.mask};
      for (int w = 0; w < (L.transition == PH_TRANSITION_WIPE ? 2 : L.transition == PH_TRANSITION_CUT ? 0 : 1); ++w) {
        t.partner[i][w] = up_layer_of(*theirs[w]);
        t.partner[i][w].ptr = image[first_img[i] + 1 + w];
        t.same[i] |= chan_sources_same_shape(*theirs[w], L.src) ? 1u << w : 0u;
      }
    }
    const hipError_t e = ph::launch_compose_up_trans(stream_of(ctx, queue), t, false, cus);
    return e == hipSuccess ? PH_OK : fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  });
}

/* A ROUTED channel's file playback: ph_clip_compose_multi's frames and the combined image itself, made inside the read-once launches: see
 * include/phaneron_hip.h.  With image_out == NULL the call IS ph_clip_compose_multi.  With it the whole frame is composed, the first
 * writer table's launch (or a launch without outputs) stores the image, and what the read-once routes do not take is refused - the
 * entry runs no fallback chain.  Everything the arguments decide is decided before the context is looked at; a refused call writes nothing. */
// Everything the call refuses with image_out set, in the entry's order - the arguments first, the context last - and what the launches
// need of it: the composition's geometry and the tables' LDS forms.  Launches nothing.
static int clip_route_checked(const char *fn, ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, void *image_out, int n_out, const ph_chan_output *outs,
                              uint32_t out_w, uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm, ph::UpArgs &base, LutRef &rref,
                              LutRef (&wref)[ph::kMaxUpOuts], bool args_only = false) {
  if (const int bad = clip_args_check(fn, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, /*route*/ true)) return bad;
  const char *const chain = "nothing else makes image_out in one call: run ph_pack_read, ph_transform, ph_combine and ph_pack_write_multi";
  // what the read-once routes take, as far as the arguments say: every layer a cut, enlarged or of the channel's size under the default fill
  base = ph::UpArgs{};
  base.n = n, base.jobs = 1;
  compose_up_lines(base, out_w, out_h, 0);  // the whole frame: a field output takes the rows of its parity
  if (out_w % 2u) return fail(PH_E_INVALID, "%s: width %u is odd; %s", fn, out_w, chain);
  for (int i = 0; i < n; ++i) {
    if (layers[i].transition != PH_TRANSITION_CUT) return fail(PH_E_INVALID, "%s: layer %d is in a transition; %s", fn, i, chain);
    if (!out_h) continue;  // (an empty frame has no placement to judge: PH_OK below)
    bool takes = chan_image_enlarged(layers[i].src, out_w, out_h, 0, /*v210_fill*/ true);
    if (takes) {
      ph::UpArgs one = base;
      one.n = 1, one.layer[0] = up_layer_of(layers[i].src);
      takes = ph::compose_up_eligible(one);
    }
    if (!takes)
      return fail(PH_E_INVALID,
                  "%s: layer %d is neither enlarged by 1 %% or more without rotation or mirroring nor of the channel's size under the default fill; %s", fn, i,
                  chain);
    base.layer[i] = up_layer_of(layers[i].src);
  }
  {  // image_out against everything the call reads or writes, by byte range
    ph::Footprint fp;
    for (int i = 0; i < n; ++i) ph::span_read_source(fp, layers[i].src, 0);
    for (int k = 0; k < n_out; ++k) ph::span_write_output(fp, outs[k], out_w, out_h);
    const ph::Span image{(const char *)image_out, (size_t)out_w * out_h * 16u, -1, 0u};
    for (int r = 0; r < fp.n_reads; ++r)
      if (ph::spans_meet(image, fp.reads[r])) return fail(PH_E_INVALID, "%s: image_out overlaps a layer's source (range %d of the call's reads)", fn, r);
    for (int w = 0; w < fp.n_writes; ++w)
      if (ph::spans_meet(image, fp.writes[w])) return fail(PH_E_INVALID, "%s: image_out overlaps an output's plane (range %d of the call's writes)", fn, w);
  }
  if (args_only) return PH_OK;
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  if (ctx->chan_enlarged == 0) return fail(PH_E_INVALID, "%s: the read-once routes are switched off (\"chan_enlarged\" = 0); %s", fn, chain);
  rref = lds_view(ctx, rd_lut);
  if (!rref.get()) return fail(PH_E_INVALID, "%s: the reader's table has no LDS form; %s", fn, chain);
  for (int k = 0; k < n_out; ++k) {  // (no output: no writer table is looked at)
    wref[k] = lds_view(ctx, outs[k].wr_gamma_lut);
    if (!wref[k].get()) return fail(PH_E_INVALID, "%s: output %d: the writer's table has no LDS form; %s", fn, k, chain);
  }
  return PH_OK;
}
static const char *const kClipRouteFn = "ph_clip_compose_route_multi";
// what both forms of the call refuse before anything else
static int clip_route_counts(int n_out, const void *image_out) {
  if (n_out < 0 || n_out > ph::kMaxUpOuts) return fail(PH_E_INVALID, "%s: 0..%d outputs (%d)", kClipRouteFn, ph::kMaxUpOuts, n_out);
  if (!n_out && !image_out) return fail(PH_E_INVALID, "%s: nothing to make: no output and image_out is NULL", kClipRouteFn);
  return PH_OK;
}
// (ph_internal.h: a by-name job's check answers as its launch does)
extern "C++" int clip_compose_route_check(int queue, int n, const ph_chan_layer *layers, void *image_out, int n_out, const ph_chan_output *outs, uint32_t out_w,
                             uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  if (const int bad = clip_route_counts(n_out, image_out)) return bad;
  if (!image_out) return PH_OK;  // (ph_clip_compose_multi's job: checked as clip_compose_multi_<n> is)
  ph::UpArgs base;
  LutRef rref, wref[ph::kMaxUpOuts];
  // (the arguments' part: a job's tables get their LDS forms when the job is launched, so what the context decides is answered there)
  return clip_route_checked(kClipRouteFn, nullptr, queue, n, layers, image_out, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, base, rref, wref, /*args_only*/ true);
}

int ph_clip_compose_route_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, void *image_out, int n_out, const ph_chan_output *outs,
                                uint32_t out_w, uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm) {
  const char *const fn = kClipRouteFn;
  if (const int bad = clip_route_counts(n_out, image_out)) return bad;
  if (!image_out) return clip_compose_multi(ctx, queue, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, /*keep_tails*/ false);
  ph::UpArgs base;
  LutRef rref, wref[ph::kMaxUpOuts];
  if (const int bad = clip_route_checked(fn, ctx, queue, n, layers, image_out, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, base, rref, wref)) return bad;
  if (!base.lines) return PH_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  bool alpha = false;
  const bool one_launch = ctx->chan_enlarged == 1 && n == 1 && clip_wire(layers[0].src, &alpha);
  ClipScratch scratch{fn, ctx, queue};
  bool image_made = false;
  // a group's launch (m.n_out == 0: the image alone); the first one made stores the image, the others are ph_clip_compose_multi's
  auto launch = [&](ph::UpMultiArgs &m, bool) {
    void *const image = image_made ? nullptr : image_out;
    image_made = true;
    return clip_group_launch(scratch, one_launch, alpha, n, layers, rd_cm, rd_lut, rd_gm, rref.view, m, /*tails*/ false, image);
  };
  // the outputs by writer table (the whole frame is composed: a field output takes the rows of its parity), a v210 output whose lines end in a
  // tail quad through ph_chan_compose, alone
  rc = clip_groups(scratch, n, layers, n_out, outs, out_w, out_h, rd_cm, rd_lut, rd_gm, base, wref, /*same_lines*/ false, /*keep_tails*/ false, launch);
  if (rc || image_made) return rc;
  ph::UpMultiArgs m{};  // no output, or every output split off: the image alone, without a table
  m.up = base;
  return launch(m, false);
}

namespace {
struct ClipBatchStep {  // what the call does in its turn: a shared launch of jobs [first, first + m.clip.up.jobs), or job `first` handed on
  int first = 0;
  bool shared = false, alpha = false;
  bool tails = false;  // option "up_v210_tails": the launch has a v210 output whose lines end in a tail quad (the same for every job: one output list)
  uint32_t grid = 0;
  ph::ClipUpMultiArgs m{};
};
}  // namespace
// one job's launch arguments as ph_clip_compose_multi makes them for its one-launch route (false: the job is not for that route as a whole)
static bool clip_job_args(ph_ctx *ctx, const ph_chan_job_out &J, const ChanJobPlan &P, uint32_t out_w, uint32_t out_h, const void *rd_cm, const void *rd_gm,
                          const ph::LutView &rd, ph::ClipUpMultiArgs &c, bool &alpha, bool &tails) {
  if (ctx->chan_enlarged != 1 || J.n != 1) return false;
  if (J.n_out == 1 && J.outs[0].format == PH_FMT_V210) return false;  // (ph_chan_compose, under its names)
  const ph_chan_source &S = J.layers[0].src;
  if (!clip_wire(S, &alpha)) return false;
  tails = false;
  for (int k = 0; k < J.n_out; ++k) {
    const bool tail = J.outs[k].format == PH_FMT_V210 && out_w % 48;
    if (J.outs[k].wr_gamma_lut != J.outs[0].wr_gamma_lut || (tail && !ctx->up_v210_tails)) return false;  // (several launches there)
    tails = tails || tail;
  }
  if (!chan_layers_enlarged(1, J.layers, out_w, out_h, P.interlace, /*v210_fill*/ true)) return false;
  ph::UpMultiArgs m{};  // the job's one group, as clip_groups makes it
  ph::UpArgs &a = m.up;
  a.n = 1, a.jobs = 1, a.layer[0] = up_layer_of(S);
  compose_up_lines(a, out_w, out_h, P.interlace);
  if (!ph::compose_up_eligible(a) || !a.lines) return false;
  a.wr = lds_view(ctx, J.outs[0].wr_gamma_lut).view;
  m.n_out = (uint32_t)J.n_out;
  for (int k = 0; k < J.n_out; ++k) m.out[k] = up_out_of(J.outs[k], P.same_lines, out_w, out_h);
  c = ph::ClipUpMultiArgs{};
  clip_multi_fill(c, m, rd, rd_gm, S, rd_cm);
  ph::ClipUpArgs probe = c.clip;
  return ph::clip_up_plan(probe, !alpha, (uint32_t)ctx->props.multiProcessorCount, /*v210_tails*/ tails) != 0;
}

/* Several CHANNELS' file playback for any consumers in one launch: see include/phaneron_hip.h.  Exactly, in order and bit for bit, the
 * n_jobs calls of ph_clip_compose_multi.  Every check of the arguments is made before the context is looked at; every job is checked and
 * every launch planned before anything is launched.  Consecutive jobs that ph_clip_compose_multi would make with ONE launch of the clip
 * kernel each, of one clip size, placement and alpha-ness and of one output list (format, interlace, writer matrix and table, output by
 * output; one table for all), share a launch of clip_up_multi_kernel<.., MULTI>: a tile belongs to one job.  The clips' wire formats may
 * differ (ClipSrc::fmt is per job - as in the v210 form, chan_compose_enlarged).  Everything else runs ph_clip_compose_multi in its turn. */
int ph_clip_compose_batch_out(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job_out *jobs, uint32_t out_w, uint32_t out_h, const void *rd_cm,
                              const void *rd_lut, const void *rd_gm) {
  static const char *const fn = "ph_clip_compose_batch_out";
  if (!jobs || !rd_cm || !rd_lut || !rd_gm) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  PH_QUEUE(fn, queue);
  if (n_jobs < 1) return fail(PH_E_INVALID, "%s: no jobs", fn);
  if (!out_w) return fail(PH_E_INVALID, "%s: width 0", fn);
  std::vector<ChanJobPlan> plan((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j)
    if (const int bad = chan_job_check(fn, j, jobs[j], ph::kMaxUpOuts, /*tables: below, once there is a context*/ nullptr, out_w, out_h, plan[(size_t)j])) return bad;
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  if (n_jobs == 1)  // a group of one job is that call
    return ph_clip_compose_multi(ctx, queue, jobs[0].n, jobs[0].layers, jobs[0].n_out, jobs[0].outs, out_w, out_h, rd_cm, rd_lut, rd_gm);
  const LutRef rref = lds_view(ctx, rd_lut);
  if (!rref.get()) return fail(PH_E_INVALID, "%s: the reader gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn);
  for (int j = 0; j < n_jobs; ++j)
    for (int k = 0; k < jobs[j].n_out; ++k)
      if (!lds_view(ctx, jobs[j].outs[k].wr_gamma_lut).found)
        return fail(PH_E_INVALID, "%s: job %d: output %d: the writer gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)", fn, j, k);
  const uint32_t num_cus = (uint32_t)ctx->props.multiProcessorCount;
  // the plan: the steps of the call, in the jobs' order
  std::vector<ClipBatchStep> steps;
  ClipBatchStep cur;  // the launch being collected
  auto flush = [&]() {
    if (!cur.shared) return;
    ph::ClipUpArgs &c = cur.m.clip;
    if (c.up.jobs > 1u) cur.grid = ph::clip_up_plan(c, !cur.alpha, num_cus, /*v210_tails*/ cur.tails);
    if (c.up.jobs > 1u && cur.grid) {
      steps.push_back(cur);
    } else {  // a group of one job (or a tiling the kernel does not take): ph_clip_compose_multi, job by job
      for (uint32_t i = 0; i < c.up.jobs; ++i) {
        ClipBatchStep own;
        own.first = cur.first + (int)i;
        steps.push_back(own);
      }
    }
    cur = ClipBatchStep{};
  };
  for (int j = 0; j < n_jobs; ++j) {
    const ph_chan_job_out &J = jobs[j];
    const ChanJobPlan &P = plan[(size_t)j];
    ph::ClipUpMultiArgs c;
    bool alpha = false, tails = false;
    if (!clip_job_args(ctx, J, P, out_w, out_h, rd_cm, rd_gm, rref.view, c, alpha, tails)) {  // in its turn, on its own
      flush();
      ClipBatchStep own;
      own.first = j;
      steps.push_back(own);
      continue;
    }
    if (cur.shared) {
      const ph::UpArgs &a = cur.m.clip.up;
      const ph_chan_job_out &J0 = jobs[cur.first];
      // no job of a launch reads or writes what another job of it writes: such a job starts the next launch
      bool apart = a.jobs >= (uint32_t)ph::kMaxUpJobs || alpha != cur.alpha || J.n_out != J0.n_out || plan[(size_t)cur.first].interlace != P.interlace ||
                   !chan_enlarged_same_shape(1, J0.layers, J.layers);
      for (int k = 0; k < J.n_out && !apart; ++k) {
        const ph_chan_output &o = J.outs[k], &o0 = J0.outs[k];
        apart = o.format != o0.format || o.interlace != o0.interlace || o.wr_col_matrix12 != o0.wr_col_matrix12 || o.wr_gamma_lut != o0.wr_gamma_lut;
      }
      // (no exception for the two fields of one frame: they are two launches here)
      for (int i = cur.first; i < cur.first + (int)a.jobs && !apart; ++i) apart = clashes(P.print, plan[(size_t)i].print, kAllHazards, /*fields_interleave*/ false);
      if (apart) flush();
    }
    if (!cur.shared) {
      cur.shared = true, cur.first = j, cur.alpha = alpha, cur.tails = tails, cur.m = c;
      continue;
    }
    const uint32_t at = cur.m.clip.up.jobs++;
    cur.m.clip.src[at] = c.clip.src[0];
    for (int k = 0; k < J.n_out; ++k)
      for (int i = 0; i < 3; ++i) cur.m.out[k].plane[at][i] = c.out[k].plane[0][i];
  }
  flush();
  // the launches
  int rc = set_device(ctx);
  if (rc) return rc;
  ClipScratch scratch{fn, ctx, queue};  // (holds no images: a job handed on takes the area itself)
  for (ClipBatchStep &s : steps) {
    if (!s.shared) {
      const ph_chan_job_out &J = jobs[s.first];
      if ((rc = ph_clip_compose_multi(ctx, queue, J.n, J.layers, J.n_out, J.outs, out_w, out_h, rd_cm, rd_lut, rd_gm))) return rc;
      continue;
    }
    rc = scratch.one_launch(s.m.clip, s.grid, [&](hipStream_t st) { return ph::launch_clip_up_multi(st, s.m, !s.alpha, s.grid, s.tails); });
    if (rc) return rc;
  }
  return PH_OK;
}

// one image of a transition call (a layer's src, incoming or mask) into a launch's arguments
static int compose_up_image(const char *fn, int job, int layer, const char *what, const ph_image_layer &I, int fmt, ph::UpLayer &d) {
  if (!I.data || I.width <= 0 || I.height <= 0 || !I.matrix9_host)
    return fail(PH_E_INVALID, "%s: job %d layer %d: the %s image is missing or incomplete", fn, job, layer, what);
  if (I.format != fmt) return fail(PH_E_INVALID, "%s: job %d layer %d: the %s image has another image format than layer 0's src", fn, job, layer, what);
  d.ptr = I.data, d.w = (uint32_t)I.width, d.h = (uint32_t)I.height, d.pitch = (uint32_t)I.width * (fmt == PH_IMG_RGB_F32 ? 12u : 16u);
  for (int k = 0; k < 6; ++k) d.m[k] = I.matrix9_host[k];
  return PH_OK;
}
static bool compose_up_same_shape(const ph_image_layer &a, const ph_image_layer &b) {
  if (a.width != b.width || a.height != b.height) return false;
  for (int k = 0; k < 9; ++k)
    if (a.matrix9_host[k] != b.matrix9_host[k]) return false;
  return true;
}

/* Dissolves and wipes inside the 2 x 2-block compositor's launch: see include/phaneron_hip.h.  Every check is made, and every launch of
 * the call is planned, before anything is launched. */
int ph_compose_up_transition_multi(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_trans_layer *const *layer_sets, int n_out,
                                   const ph_chan_output *outs, uint32_t out_w, uint32_t out_h) {
  const char *const fn = "ph_compose_up_transition_multi";
  // (what the arguments alone decide is decided first - the context is looked at last, so a caller without a device learns of its mistakes too)
  if (!layer_sets || !outs) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n_out < 1 || n_out > ph::kMaxUpOuts) return fail(PH_E_INVALID, "%s: 1..%d outputs (%d)", fn, ph::kMaxUpOuts, n_out);
  if (jobs < 1 || jobs > ph::kMaxUpJobs) return fail(PH_E_INVALID, "%s: 1..%d jobs (%d)", fn, ph::kMaxUpJobs, jobs);
  for (int j = 0; j < jobs; ++j)
    if (!layer_sets[j]) return fail(PH_E_INVALID, "%s: NULL argument", fn);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "%s: 1..%d layers", fn, ph::kMaxLayers);
  bool any = false;
  for (int j = 0; j < jobs; ++j)
    for (int i = 0; i < n; ++i) {
      const int t = layer_sets[j][i].transition;
      if (t != PH_TRANSITION_CUT && t != PH_TRANSITION_DISSOLVE && t != PH_TRANSITION_WIPE)
        return fail(PH_E_INVALID, "%s: job %d layer %d: transition %d is not a PH_TRANSITION_*", fn, j, i, t);
      if (t != layer_sets[0][i].transition) return fail(PH_E_INVALID, "%s: job %d layer %d: another transition than job 0's layer has", fn, j, i);
      any = any || t != PH_TRANSITION_CUT;
    }
  if (!any) {  // every layer a cut: ph_compose_up_write_multi on the src layers
    std::vector<ph_image_layer> flat((size_t)jobs * n);
    const ph_image_layer *sets[ph::kMaxUpJobs];
    for (int j = 0; j < jobs; ++j) {
      for (int i = 0; i < n; ++i) flat[(size_t)j * n + i] = layer_sets[j][i].src;
      sets[j] = &flat[(size_t)j * n];
    }
    return compose_up_write_multi(ctx, queue, jobs, n, sets, n_out, outs, out_w, out_h, /*keep_tails*/ false);
  }
  int rc = compose_up_outputs(fn, jobs, n_out, outs, out_w, out_h);
  if (rc) return rc;
  for (int k = 0; k < n_out; ++k)
    if (outs[k].format == PH_FMT_V210 && out_w % 48)
      return fail(PH_E_INVALID, "%s: output %d: a v210 frame of width %u ends its lines in a tail quad, which this kernel does not write for layers in a "
                                "transition (width %% 48 != 0); use ph_chan_compose_multi", fn, k, out_w);
  // the layers: job 0 gives count, kinds, sizes, layouts and placements; a further job its images' data and its mix values
  ph::UpTransArgs t{};
  ph::UpArgs &base = t.multi.up;
  base.n = n, base.jobs = (uint32_t)jobs;
  const int fmt = layer_sets[0][0].src.format;
  if (fmt != PH_IMG_RGBA_F32 && fmt != PH_IMG_RGB_F32) return fail(PH_E_INVALID, "%s: image format %d", fn, fmt);
  std::vector<ph::UpLayer> partners;  // the present partner images, for the placement rule
  for (int i = 0; i < n; ++i) {
    const ph_image_trans_layer &L = layer_sets[0][i];
    const bool has[2] = {L.transition != PH_TRANSITION_CUT, L.transition == PH_TRANSITION_WIPE};
    const char *const what[2] = {"incoming", "mask"};
    t.kind[i] = (uint32_t)L.transition;
    for (int j = 0; j < jobs; ++j) {
      const ph_image_trans_layer &B = layer_sets[j][i];
      const ph_image_layer *const theirs[2] = {&B.incoming, &B.mask}, *const firsts[2] = {&L.incoming, &L.mask};
      ph::UpLayer d{};
      if ((rc = compose_up_image(fn, j, i, "src", B.src, fmt, d))) return rc;
      if (j == 0) base.layer[i] = d;
      else if (!compose_up_same_shape(B.src, L.src)) return fail(PH_E_INVALID, "%s: job %d layer %d: the src image differs from job 0's in more than its data", fn, j, i);
      else base.more_ptr[j - 1][i] = d.ptr;
      for (int w = 0; w < 2; ++w) {
        if (!has[w]) continue;
        if ((rc = compose_up_image(fn, j, i, what[w], *theirs[w], fmt, d))) return rc;
        if (j == 0) {
          t.partner[i][w] = d;
          t.same[i] |= compose_up_same_shape(*theirs[w], L.src) ? 1u << w : 0u;
          partners.push_back(d);
        } else if (!compose_up_same_shape(*theirs[w], *firsts[w])) {
          return fail(PH_E_INVALID, "%s: job %d layer %d: the %s image differs from job 0's in more than its data", fn, j, i, what[w]);
        } else {
          t.more_partner[j - 1][i][w] = d.ptr;
        }
      }
      t.mix[j][i] = B.mix;
    }
  }
  std::vector<UpLaunch> launches;
  if (out_h) compose_up_launches(base, jobs, n_out, outs, out_w, out_h, false, launches);  // (no lines: nothing to compose, PH_OK)
  for (const UpLaunch &l : launches) {  // the placement rule on the geometry each launch composes: layers and partners alike
    if (!ph::compose_up_eligible(l.m.up)) return compose_up_not_eligible(fn);
    ph::UpArgs p = l.m.up;
    p.n = 1;
    for (const ph::UpLayer &partner : partners) {
      p.layer[0] = partner;
      if (!ph::compose_up_eligible(p)) return compose_up_not_eligible(fn);
    }
  }
  if (!ctx) return fail(PH_E_INVALID, "%s: ctx is NULL", fn);
  PH_QUEUE(fn, queue);
  LutRef wref[ph::kMaxUpOuts];
  if ((rc = compose_up_tables(fn, ctx, n_out, outs, wref))) return rc;
  rc = set_device(ctx);
  if (rc) return rc;
  for (const UpLaunch &l : launches) {
    if (!l.m.up.lines) continue;
    t.multi = l.m, t.multi.up.wr = *wref[l.table].get();
    const hipError_t e = ph::launch_compose_up_trans(stream_of(ctx, queue), t, fmt == PH_IMG_RGB_F32, (uint32_t)ctx->props.multiProcessorCount);
    if (e != hipSuccess) return fail(PH_E_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
  }
  return PH_OK;
}

int ph_v210_yadif_pair_fmt(ph_ctx *ctx, int queue, int n, const ph_deint_source *src, uint32_t width, uint32_t height, int tff,
                           int skip, int out_format, const void *cm, const void *lut, const void *gm) {
  return ph_yadif_pair_packed(ctx, queue, n, src, PH_FMT_V210, width, height, tff, skip, out_format, cm, lut, gm);
}

int ph_yadif_pair_packed(ph_ctx *ctx, int queue, int n, const ph_deint_source *src, int packing, uint32_t width, uint32_t height, int tff,
                         int skip, int out_format, const void *cm, const void *lut, const void *gm) {
  if (!ctx || !src || !cm || !lut || !gm) return fail(PH_E_INVALID, "ph_v210_yadif_pair: NULL argument");
  if (!fmt_deint(packing))
    return fail(PH_E_INVALID, "ph_v210_yadif_pair: packing %d (v210, yuv422p10, yuv422p8, yuv420p or nv12; for the others - the 10-bit 4:2:0 "
                              "yuv420p10 / p010 among them - run the separate kernels: the format's reader, then yadif)", packing);
  if (fmt_v420(packing) && (height & 1))
    return fail(PH_E_INVALID, "ph_v210_yadif_pair: a 4:2:0 frame needs an even height (%u)", height);
  const bool planar = packing != PH_FMT_V210;
  if (out_format != PH_IMG_RGBA_F32 && out_format != PH_IMG_RGB_F32) return fail(PH_E_INVALID, "ph_v210_yadif_pair: output format %d", out_format);
  if (n < 1 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "ph_v210_yadif_pair: 1..%d sources", ph::kMaxLayers);
  if (!width || (planar ? width % 2 : width % 6))
    return fail(PH_E_INVALID, "ph_v210_yadif_pair: width %u is not a multiple of %d; run the separate kernels", width, planar ? 2 : 6);
  const LutRef lref = lds_view(ctx, lut);
  const ph::LutView *v = lref.get();
  if (!v) return fail(PH_E_INVALID, "ph_v210_yadif_pair: the reader gamma LUT has no LDS form (ph_lut_register it, or run the separate kernels)");
  ph::DeintArgs a{};
  for (int i = 0; i < n; ++i) {
    const ph_deint_source &s = src[i];
    if (!s.prev || !s.cur || !s.next || !s.out_parity0 || !s.out_parity1)
      return fail(PH_E_INVALID, "ph_v210_yadif_pair: source %d is incomplete", i);
    if (s.out_parity0 == s.out_parity1) return fail(PH_E_INVALID, "ph_v210_yadif_pair: source %d: the two outputs are the same buffer", i);
    a.prev[i] = (const uint4 *)s.prev, a.cur[i] = (const uint4 *)s.cur, a.next[i] = (const uint4 *)s.next;
    a.out0[i] = (float4 *)s.out_parity0, a.out1[i] = (float4 *)s.out_parity1;
    if (planar) {
      if (!s.prev_u || !s.cur_u || !s.next_u || (fmt_planes(packing) == 3 && (!s.prev_v || !s.cur_v || !s.next_v)))
        return fail(PH_E_INVALID, "ph_v210_yadif_pair: source %d: a planar window needs its chroma planes", i);
      a.prev_u[i] = s.prev_u, a.prev_v[i] = s.prev_v, a.cur_u[i] = s.cur_u, a.cur_v[i] = s.cur_v, a.next_u[i] = s.next_u, a.next_v[i] = s.next_v;
    }
  }
  if (!height) return PH_OK;
  a.pack = (uint32_t)packing;
  // quads_pitch: a v210 line in 16-byte quads, or (planar) the luma samples per line: the width rounded up to 8 (yuv422p10.ts:221)
  a.n = n, a.skip = skip ? 1 : 0, a.width = width, a.height = height, a.quads_pitch = planar ? ((width + 7u) & ~7u) : ph_v210_pitch_bytes(width) / 16;
  a.rgb12 = out_format == PH_IMG_RGB_F32 ? 1u : 0u;
  a.cm = (const float *)cm, a.gm = (const float *)gm, a.lut = *v;
  PH_LAUNCH(ph::launch_v210_yadif_pair(stream_of(ctx, queue), a, tff ? 1 : 0, (uint32_t)ctx->props.multiProcessorCount));
}

/* A packed f32 RGB image (12 bytes per pixel, alpha == 1 implied: what ph_v210_yadif_pair_fmt writes with PH_IMG_RGB_F32) made the f32 RGBA
 * image of the same pixels, IN PLACE: the packed pixels are copied to the queue's scratch area, then expanded back into the buffer.
 * For a binding that lets the de-interlacing reader write packed fields into the application's RGBA image buffers while only the 2 x 2-block
 * compositor reads them, and has to hand over a real image when anybody else asks (node/defer.js). */
int ph_image_unpack_rgb(ph_ctx *ctx, int queue, void *image, int w, int h) {
  if (!ctx || !image || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_image_unpack_rgb: NULL/zero argument");
  PH_QUEUE("ph_image_unpack_rgb", queue);
  int rc = set_device(ctx);
  if (rc) return rc;
  const size_t npx = (size_t)w * h;
  if (ph::trace_launch("rgb_unpack")) return PH_OK;
  std::lock_guard<std::mutex> scratch(ctx->chan_scratch_mu[queue]);  // until both operations are enqueued (launches on one queue are in order)
  void *tmp;
  {
    std::lock_guard<std::mutex> lock(ctx->mu);
    rc = chan_index_reserve(ctx, queue, npx * 12);
    if (rc) return rc;
    tmp = ctx->chan_index[queue];
  }
  PH_HIP(hipMemcpyAsync(tmp, image, npx * 12, hipMemcpyDeviceToDevice, stream_of(ctx, queue)));
  hipError_t e = ph::launch_rgb_unpack(stream_of(ctx, queue), tmp, image, npx);
  if (e != hipSuccess) return fail(PH_E_HIP, "ph_image_unpack_rgb: launch failed: %s", hipGetErrorString(e));
  return PH_OK;
}

int ph_transform(ph_ctx *ctx, int queue, const void *in, int iw, int ih, const void *m9, void *out, int ow, int oh) {
  if (!in || !m9 || !out || iw <= 0 || ih <= 0 || ow <= 0 || oh <= 0) return fail(PH_E_INVALID, "ph_transform: NULL/zero argument");
  PH_LAUNCH(ph::launch_transform(stream_of(ctx, queue), in, iw, ih, m9, out, ow, oh));
}

int ph_resize(ph_ctx *ctx, int queue, const void *in, int iw, int ih, float scale, float ox, float oy,
              const void *flip4, void *out, int ow, int oh) {
  if (!in || !flip4 || !out || iw <= 0 || ih <= 0 || ow <= 0 || oh <= 0) return fail(PH_E_INVALID, "ph_resize: NULL/zero argument");
  PH_LAUNCH(ph::launch_resize(stream_of(ctx, queue), in, iw, ih, scale, ox, oy, flip4, out, ow, oh));
}

int ph_combine(ph_ctx *ctx, int queue, int n, const void *const *layers, int w, int h, void *out) {
  // the reference's Combine throws below 2 inputs (combine.ts:92-93)
  if (n < 2 || n > ph::kMaxLayers) return fail(PH_E_INVALID, "Combine requires between 2 and %d input buffers, got %d", ph::kMaxLayers, n);
  if (!layers || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_combine: NULL/zero argument");
  ph::CombineArgs a{};
  for (int i = 0; i < n; ++i) {
    if (!layers[i]) return fail(PH_E_INVALID, "ph_combine: layer %d is NULL", i);
    a.layers[i] = layers[i];
  }
  a.out = out;
  a.npx = (size_t)w * h;
  PH_LAUNCH(ph::launch_combine(stream_of(ctx, queue), n, a));
}

int ph_transition_dissolve(ph_ctx *ctx, int queue, const void *in0, const void *in1, float mix, int w, int h, void *out) {
  if (!in0 || !in1 || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_transition_dissolve: NULL/zero argument");
  PH_LAUNCH(ph::launch_dissolve(stream_of(ctx, queue), in0, in1, mix, w, h, out));
}

int ph_mixer(ph_ctx *ctx, int queue, const void *in0, const void *in1, float mix, int w, int h, void *out) {
  if (!in0 || !in1 || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_mixer: NULL/zero argument");
  PH_LAUNCH(ph::launch_dissolve(stream_of(ctx, queue), in0, in1, mix, w, h, out));  // same arithmetic (mix.ts:41-42)
}

int ph_transition_wipe(ph_ctx *ctx, int queue, const void *in0, const void *in1, const void *mask, int w, int h,
                       void *out) {
  if (!in0 || !in1 || !mask || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_transition_wipe: NULL/zero argument");
  PH_LAUNCH(ph::launch_twipe(stream_of(ctx, queue), in0, in1, mask, w, h, out));
}

int ph_wipe(ph_ctx *ctx, int queue, const void *in0, const void *in1, float wipe, int w, int h, void *out) {
  if (!in0 || !in1 || !out || w <= 0 || h <= 0) return fail(PH_E_INVALID, "ph_wipe: NULL/zero argument");
  PH_LAUNCH(ph::launch_wipe(stream_of(ctx, queue), in0, in1, wipe, w, h, out));
}

}  // extern "C"
