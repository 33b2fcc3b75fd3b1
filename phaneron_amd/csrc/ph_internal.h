// ph_internal.h - what the library's two host translation units share: ph_api.cpp (context, buffers, queues, the typed entry
// points) and ph_run.cpp (programs and their by-name jobs).  Nothing here is exported: the C ABI is include/phaneron_hip.h.
// Both plan shared launches - which jobs may sit in one - with ph_spans.h: a job's byte ranges and the one hazard test on them.
#pragma once
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/phaneron_hip.h"
#include "ph_kernels.h"
#include "ph_program.h"
#include "ph_spans.h"

static_assert(ph::kSpanLayers == ph::kMaxLayers && ph::kSpanOuts >= ph::kMaxChanOuts && ph::kSpanOuts >= ph::kMaxFusedOuts && ph::kSpanOuts >= ph::kMaxUpOuts,
              "a Footprint holds any job's ranges: ph_spans.h sizes it by these limits without seeing ph_kernels.h");
static_assert(ph::kMaxChanOps <= ph::kSpanLayers * 3, "a channel job's op list is at most three sources per layer");

// sets the calling thread's ph_last_error text; returns code
#pragma GCC visibility push(hidden)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
#pragma GCC visibility pop

#define PH_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) return fail(PH_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

struct LutEntry {
  ph::LutView view{};  // bytes == 0: a plain table
  void *blob_dev = nullptr;
  float max_finite = __builtin_inff();  // ph::lut_max_finite of the host copy (Inf: not known, the fused kernel's witness guard fails)
};

// Lifetime: buffers, programs, events and graphs each hold a reference on their context, so the storage a
// handle points into outlives the handle whatever order a garbage collector finalises them in.
// ph_ctx_destroy drains the queues, marks the context closed (new work is refused) and drops the creator's
// reference; the last handle released tears the device state down.
// Threading: `mu` guards the pool, the LUT registry and the counters (the node addon calls hostAccess and
// timed runProgram from libuv pool threads while the JS thread creates and releases buffers).
struct ph_ctx {
  int device = 0;
  std::map<const void *, LutEntry> luts;  // device f32 table -> compressed LDS form
  bool use_lds_lut = true;
  int stream_images = 0;        // f32 image outputs: 0 through the caches, 1 streamed past them, 2 by size (ph_device.h store_image)
  int stream_threshold_mb = 64;  // policy 2: images larger than this stream
  hipStream_t streams[3] = {nullptr, nullptr, nullptr};
  hipDeviceProp_t props;
  std::multimap<size_t, void *> pool;  // free device blocks by exact size
  size_t pooled_bytes = 0, live_buffers = 0, live_bytes = 0;
  // Pinned host mirrors by exact size.  The reference makes a fresh destination per job and frame (io.ts:64-72, mixer.ts:196,
  // combiner.ts:230) and the node binding gives every buffer its mirror at once (an OpenCLBuffer IS a node Buffer): a
  // hipHostMalloc / hipHostFree pair of a 2160p image is ~40 ms, a pool hit nothing
  // (a block carries the event recorded behind the last asynchronous copy that touched it: the next owner waits for it -
  // normally long complete - before it writes the mirror; blocks are evicted oldest first when the budget is exceeded)
  struct HostBlock {
    void *p;
    hipEvent_t busy;  // may be null
    uint64_t seq;
  };
  std::multimap<size_t, HostBlock> host_pool;
  size_t host_pooled_bytes = 0;
  uint64_t host_pool_seq = 0;
  // what the pool may keep pinned: this many MiB, or - if that is more - as much as was ever in use at once (host_peak_bytes): a
  // pool smaller than the working set frees and pins a block per buffer again, 40 ms each (four 1080p channels create 36 images of
  // 33 MB per tick: round 5 measured 40 ms per tick under the fixed 1 GiB of round 4)
  // option "chan_enlarged" (default 1; PH_CHAN_ENLARGED=0 in the environment makes it 0): frames of enlarged clips by read + 2 x 2-block compositor
  int chan_enlarged = !(getenv("PH_CHAN_ENLARGED") && getenv("PH_CHAN_ENLARGED")[0] == '0');
  // option "chan_batch_outs" (default 0): ph_run_programs puts channel frames for other consumers than SDI into shared launches (ph_chan_compose_batch_out)
  int chan_batch_outs = 0;
  // option "clip_batch" (default 0): ph_run_programs puts consecutive clip_compose_multi_<n> jobs into shared launches (ph_clip_compose_batch_out)
  int clip_batch = 0;
  // option "up_v210_tails" (default 0): a v210 output whose lines end in a tail quad (width % 48 != 0: 1280) stays in its writer table's launch of
  // the several-outputs kernels (ph_compose_up_write_multi, ph_clip_compose_multi, ph_clip_compose_batch_out) instead of being made on its own
  int up_v210_tails = 0;
  // option "fused_multi_wgs" (default 0 = no cap): the most workgroups a ph_fused_v210_combine_multi launch may have (tests, A/B runs)
  int fused_multi_wgs = 0;
  // option "fused_multi_batch" (default 0): ph_run_programs puts consecutive fused_v210_combine_multi_<n> jobs into shared launches (ph_fused_v210_combine_multi_batch)
  int fused_multi_batch = 0;
  // option "fused_fields" (default 0): ph_fused_v210_combine_multi and ph_fused_v210_combine_multi_batch compose only the field when every output
  // takes the same one (launch_fused_v210_field_multi / _batch); 0: the whole frame, a field output taking the lines of its parity
  int fused_fields = 0;
  std::atomic<int> fail_launches{0};  // option "fail_launches" (a TEST hook): > 0 every launch through ph_run_program(s) fails; -k: the next k go through, then every one fails
  int host_pool_mb = 4096;
  size_t host_live_bytes = 0, host_peak_bytes = 0;  // mirrors attached to buffers now / at most
  uint64_t host_pins = 0;                           // hipHostMalloc calls so far (ph_ctx_host_pool_stats)
  void *chan_index[3] = {nullptr, nullptr, nullptr};  // index frame of the channel compositor, one per queue (ph_chan_compose_v210)
  size_t chan_index_bytes[3] = {0, 0, 0};
  // who is between taking a piece of a queue's area and enqueueing the last launch that uses it (callers on several threads: the launches of
  // two calls on one queue must not interleave around the shared scratch); taken before ctx->mu, never the other way round
  std::mutex chan_scratch_mu[3];
  unsigned chan_scratch_turn[3] = {0, 0, 0};  // which third of the area the next frame of enlarged clips puts its images in (chan_compose_enlarged)
  std::vector<struct ph_route *> routes;  // open ROUTEs: a recycled block must not be handed out under a transfer in flight
  std::mutex mu;
  std::atomic<int> refs{1};
  std::atomic<bool> closed{false};
  std::atomic<bool> lds_base_checked{false};  // ph_lut_register: the kernels' dynamic shared array starts at LDS address 0
};

struct ph_buf {
  ph_ctx *ctx;
  void *dptr;
  void *hptr;  // pinned host mirror, lazily allocated
  size_t bytes;
  int width, height;
  std::atomic<int> refs;
  bool owned;
  // written by libuv pool threads (hostAccess) and read by the launching thread (flush_dirty_args)
  std::atomic<bool> host_dirty;
  std::atomic<bool> lut_dirty;  // host data went into a table-sized buffer since its LDS form was last built
  std::string owner;
  hipEvent_t mirror_busy = nullptr;  // recorded behind the last asynchronous copy into or out of the mirror (travels with it into the pool)
  hipStream_t mirror_stream = nullptr;  // the stream that copy was enqueued on
};

struct ph_program {
  ph_ctx *ctx;
  ph::KernelId id;
  int n_layers;  // combine_N
  int format;    // PH_FMT_* of a read/write program
  std::string kernel;
  uint32_t global[2];
  uint32_t local;
};

#pragma GCC visibility push(hidden)
int set_device(ph_ctx *ctx);  // refuses a destroyed context; the launch that follows on this thread takes the context's store policy
void ctx_ref(ph_ctx *ctx);
void ctx_unref(ph_ctx *ctx);  // drops one reference; the last one frees the device state (streams, pool, LUT blobs)
int closed_error(const char *fn);
void refresh_buf_lut(ph_ctx *ctx, ph_buf *b);  // a ph_buf used as `gammaLut`: (re)compress from its host mirror if new data went in
void mirror_mark(ph_buf *b, hipStream_t s);    // an asynchronous copy into or out of b's mirror has just been enqueued on `s`
int chan_out_refused(const char *fn, int fmt);  // a format the channel kernel does not write: one answer from ph_chan_compose and from a program's outPacking
// everything ph_clip_compose_route_multi decides from its arguments alone - all it refuses before it looks at the context - with its texts,
// and nothing launched (a clip_compose_route_<n> job's check)
int clip_compose_route_check(int queue, int n, const ph_chan_layer *layers, void *image_out, int n_out, const ph_chan_output *outs, uint32_t out_w,
                             uint32_t out_h, const void *rd_cm, const void *rd_lut, const void *rd_gm);
bool inject_failure(ph_ctx *ctx);              // the "fail_launches" fault injection: does this launch fail?

inline bool queue_ok(int queue) { return queue >= 0 && queue < 3; }
inline int bad_queue(const char *fn, int queue) {
  return fail(PH_E_INVALID, "%s: queue %d is not PH_QUEUE_LOAD (0), PH_QUEUE_PROCESS (1) or PH_QUEUE_UNLOAD (2)", fn, queue);
}
#pragma GCC visibility pop
// The stream behind a queue index.  There is no unchecked accessor: an out-of-range index makes the ENCLOSING entry point
// return PH_E_INVALID here, whether or not it remembered PH_QUEUE() at its top - never a silent alias of the process queue.
#define stream_of(ctx, queue)                                  \
  ({                                                           \
    const int ph_q_ = (queue);                                 \
    if (!queue_ok(ph_q_)) return bad_queue(__func__, ph_q_);   \
    (ctx)->streams[ph_q_];                                     \
  })
#define PH_QUEUE(fn, queue)                        \
  do {                                             \
    if (!queue_ok(queue)) return bad_queue(fn, queue); \
  } while (0)
