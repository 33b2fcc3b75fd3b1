/* phaneron_hip.h - C ABI of libphaneron_hip.so: the MI355X (gfx950) replacement for the
 * `nodencl` binding underneath phaneron's src/process operators and src/clJobQueue.ts.
 *
 * The reference reaches its OpenCL kernels only through the nodencl JS API (npm nodencl@1.4.2,
 * not vendored).  Each entry point below replaces one piece of that surface and cites the
 * reference call sites (paths relative to the reference checkout) that define its meaning.
 * INTEGRATION.md shows the N-API stub that binds these for node (node/ph_napi.c is that stub).
 *
 * Conventions
 *   - extern "C", opaque handles, plain pointers and sizes; no C++/torch types.
 *   - every call returns 0 on success, a negative PH_E_* code otherwise; ph_last_error() gives
 *     the message (the reference surfaces failures as rejected promises / thrown Error).
 *   - one caller thread per context (the reference calls from the single node main thread);
 *     work completes asynchronously on the context's three in-order HIP streams.
 *   - device buffers are reference counted like nodencl's OpenCLBuffer (addRef/release).
 *   - there is NO CPU fallback: without a HIP device ph_ctx_create fails.
 */
#ifndef PHANERON_HIP_H
#define PHANERON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (ph_abi_version() returns PH_ABI_VERSION; a binding compiled against another value must not load the library)
 * 2: additive over 1 - ph_program_resolve, ph_route_*, ph_yadif_pair, ph_v210_yadif_pair, ph_v210_read_batch,
 *    ph_compose_wipe_write_v210, context option "stream_images"; no signature of 1 changed
 * 3: ph_chan_compose_v210 (ph_chan_source / ph_chan_layer), ph_compose_up_write_v210, ph_v210_yadif_pair_fmt, ph_check_program,
 *    ph_route_comm_count, context option "host_pool_mb"
 * 4: BREAKING for callers of ph_v210_yadif_pair: ph_deint_source grew from 40 to 88 bytes (six chroma-plane pointers for
 *    ph_yadif_pair_packed), so an array of sources built against 2 / 3 has the wrong stride.  ph_chan_compose added
 * 5: ph_compose_up_write_v210_pair, ph_lut_layout_of
 * 6: ph_fused_field_v210 / ph_field_layer REMOVED (the slowest route of its workload by 2.7x, no caller).  The fused entry
 *    points take widths that are not a multiple of 48 (1280 x 720: the reference's third format, src/config.ts:43-54)
 * 7: additive over 6 - ph_chan_compose_batch (ph_chan_job): several channels' frames in one launch; ph_run_programs; ph_compose_up_write_v210_batch; ph_pack_read_batch;
 *    ph_event_record_timed / ph_event_elapsed_us; ph_ctx_host_pool_stats; "host_pool_mb" defaults to 4096 again and never
 *    keeps less than the working set
 * 8: additive over 7 - ph_trace_begin / ph_trace_end (which kernels made a frame; dry runs); ph_run_programs_progress; ph_buf_reuse; ph_image_unpack_rgb (program "rgb_unpack").
 *    Later additive within 8: the 10-bit 4:2:0 formats PH_FMT_YUV420P10 / PH_FMT_P010 and PH_SRC_YUV420P10 / PH_SRC_P010 - new enum
 *    values an older binding never passes; no signature or struct changed.  ph_chan_compose_multi (ph_chan_output): several consumers'
 *    frames of one channel in one launch; program "chan_compose_multi_<n>".  ph_compose_up_write_multi: the same for the 2 x 2-block
 *    compositor (enlarged images), with every writer the channel kernel has.  ph_chan_compose_batch_out (ph_chan_job_out): several
 *    channels' frames for any consumers in one launch; context option "chan_batch_outs".  ph_pack_write_multi: one f32 RGBA image packed
 *    for up to four consumers, any pack format each, in one launch; program "pack_write_multi_<n>".  ph_fused_v210_combine_multi: the
 *    plain-layer composite (ph_fused_v210_combine's chain) for up to four consumers in one launch; program
 *    "fused_v210_combine_multi_<n>"; context option "fused_multi_wgs".  ph_fused_v210_combine_multi_batch: several channels' such frames in one
 *    launch; context option "fused_multi_batch".  ph_compose_up_transition_multi (ph_image_trans_layer): dissolves and wipes inside the
 *    2 x 2-block compositor's launch.  ph_fused_v210_transition_multi (ph_fused_layer): dissolves and wipes between the plain v210 layers
 *    of ph_fused_v210_combine_multi's launch; program "fused_v210_trans_<n>".  ph_fused_v210_route_multi (ph_route_layer): a routed f32 RGBA
 *    image among that launch's layers and the combined image among its outputs; program "fused_v210_route_<n>".  ph_debug_image_nt
 *    (tests): which store policy the next launch would be given.  ph_clip_compose_multi: file playback - enlarged clips, decoders' frames
 *    under the default fill - for up to four consumers of any format the channel kernel writes, read once per source pixel; program
 *    "clip_compose_multi_<n>".  ph_clip_compose_batch_out (ph_chan_job_out): several channels' such frames in one launch; context
 *    option "clip_batch".  ph_clip_compose_transition_multi: file playback through a MIX or WIPE - a layer's src, incoming and mask clips
 *    each read once per source pixel; program "clip_compose_trans_<n>".  ph_clip_compose_route_multi: a routed channel's file playback -
 *    ph_clip_compose_multi's frames and the combined f32 RGBA image itself from the read-once launches; program "clip_compose_route_<n>".
 *    Context option "fused_fields": ph_fused_v210_combine_multi and its batch compose only the field where every output takes the same
 *    one; ph_debug_fused_field_quad (tests): a field quad's place in the frame, as those launches' kernels make it */
#define PH_ABI_VERSION 8

enum {
  PH_OK = 0,
  PH_E_INVALID = -1,     /* bad argument / unknown kernel argument name */
  PH_E_NO_DEVICE = -2,   /* no HIP device (there is no CPU path) */
  PH_E_HIP = -3,         /* a HIP runtime call failed; see ph_last_error */
  PH_E_UNKNOWN_KERNEL = -4,
  PH_E_RANGE = -5        /* buffer too small for the geometry requested */
};

typedef struct ph_ctx ph_ctx;
typedef struct ph_buf ph_buf;
typedef struct ph_program ph_program;

/* nodencl `clContext.queue.{load,process,unload}` (src/index.ts:94-108, io.ts:79-98,
 * clJobQueue.ts:126,131): three in-order queues. */
enum { PH_QUEUE_LOAD = 0, PH_QUEUE_PROCESS = 1, PH_QUEUE_UNLOAD = 2 };

/* ---- context: `new clContext({platformIndex, deviceIndex, overlapping})` + `initialise()`
 *      (src/index.ts:94-107) ------------------------------------------------------------------ */
int ph_ctx_create(int device_index, ph_ctx **out);
int ph_ctx_destroy(ph_ctx *ctx);
/* `getPlatformInfo()` (src/index.ts:103-106): vendor / device name strings. */
int ph_ctx_info(ph_ctx *ctx, char *vendor, size_t vendor_len, char *device, size_t device_len);
/* message of the last failure on this thread (ctx may be NULL for ph_ctx_create failures). */
const char *ph_last_error(ph_ctx *ctx);

/* ---- which kernels made it (no nodencl counterpart: the reference runs one kernel per job, clJobQueue.ts:126; this library folds
 * jobs into fused launches and chooses among several routes by the shape of a frame - DESIGN.md section 5 lists them).
 * Between ph_trace_begin and ph_trace_end every kernel launch the CALLING THREAD's calls make is noted, in order; ph_trace_end
 * returns the names joined by '+' - e.g. "fused_v210_combine_lds", "chan_compose_v210<0,0>" (<phase-1 instantiation, output format>),
 * "chan_compose_batch<0>x4" (four jobs in the launch), "pack_read+compose_up_write_v210", "v210_yadif_pair+compose_up_write_v210".
 * dry_run != 0: the calls check their arguments and choose their kernels exactly as always but enqueue NOTHING (outputs untouched) -
 * "which route would this frame take".  PH_E_RANGE when `route` is too short (the trace is dropped), PH_E_INVALID without a begin. */
int ph_trace_begin(int dry_run);
int ph_trace_end(char *route, size_t len);
/* the hipStream_t behind a queue, for interop (tests wrap it as a torch external stream). */
void *ph_ctx_stream(ph_ctx *ctx, int queue);
/* `waitFinish(queue)` (clJobQueue.ts:131, io.ts callers): returns when the stream is idle. */
int ph_wait_finish(ph_ctx *ctx, int queue);
/* non-blocking: 1 = the queue is idle, 0 = work still in flight, negative = error.  Lets a caller
 * that expects the work to end within microseconds poll briefly instead of paying a thread hand-off. */
int ph_queue_query(ph_ctx *ctx, int queue);

/* ---- buffers: `createBuffer(bytes, access, svmType, imageDims?, owner?)` (19 call sites, e.g.
 *      io.ts:61-77,144-150, mixer.ts:196-205, combiner.ts:230-239, yadif.ts:76-86) -------------- */
enum { PH_ACCESS_READONLY = 0, PH_ACCESS_WRITEONLY = 1, PH_ACCESS_READWRITE = 2 };
enum { PH_SVM_NONE = 0, PH_SVM_COARSE = 1, PH_SVM_FINE = 2 };
/* width/height > 0 mark the buffer as an RGBA f32 image (nodencl `ImageDims`): row-major,
 * unpadded, 16 bytes per pixel.  Storage comes from a per-context pool (no hipMalloc per frame). */
int ph_buf_create(ph_ctx *ctx, size_t bytes, int access, int svm_type, int width, int height,
                  const char *owner, ph_buf **out);
/* adopt device memory owned by the caller (e.g. a torch tensor); never freed by the library. */
int ph_buf_wrap(ph_ctx *ctx, void *device_ptr, size_t bytes, int width, int height, ph_buf **out);
int ph_buf_addref(ph_buf *buf);  /* OpenCLBuffer.addRef()  (loadSave.ts:102-106 ...) */
int ph_buf_release(ph_buf *buf); /* OpenCLBuffer.release(): last release recycles the storage */
int ph_buf_refcount(const ph_buf *buf);
size_t ph_buf_bytes(const ph_buf *buf);
void *ph_buf_device_ptr(ph_buf *buf);
int ph_buf_dims(const ph_buf *buf, int *width, int *height);
/* `buf.hostAccess(dir, queue, src?)` (io.ts:89-94,172; loadSave.ts:76-99; transform.ts:84-89):
 *   WRITEONLY + src : copy `bytes` of host memory to the device on `queue` (async, pinned staging)
 *   WRITEONLY, no src: expose the host mirror for the caller to fill (ph_buf_host_ptr)
 *   NONE            : hand the (filled) host mirror back to the device
 *   READONLY        : make the device contents visible in the host mirror (sync on return) */
enum { PH_HOST_READONLY = 0, PH_HOST_WRITEONLY = 1, PH_HOST_NONE = 2 };
int ph_buf_host_access(ph_buf *buf, int dir, int queue, const void *src, size_t bytes);
/* For a binding that keeps released buffers itself and hands them to their next owner whole (node/index.js parks frames and images:
 * handle, device block, pinned mirror): what ph_buf_release + ph_buf_create would have seen to - waits for an asynchronous mirror copy
 * still in flight, orders the queues behind ROUTE transfers still using the device block, forgets the previous owner's pending host
 * data.  The contents are unspecified afterwards, as a fresh buffer's are. */
int ph_buf_reuse(ph_buf *b);
void *ph_buf_host_ptr(ph_buf *buf); /* pinned host mirror (allocated on first use) */
/* Staged producers / consumers (the queue.load / queue.unload roles of io.ts:79-98,
 * 166-174).  nodencl orders its three queues through host-side `waitFinish`; these two calls let a
 * caller that keeps a ring of frames in flight order them on the device instead, so uploads of frame
 * n+1 and downloads of frame n-1 overlap the kernels of frame n without a host round trip:
 *   ph_queue_wait_queue : work enqueued on `waiter` after this call starts only once everything
 *                         enqueued on `signal` before this call has finished (event record + wait).
 *   ph_buf_download_async: device -> pinned host mirror on `queue`, no host synchronisation; the
 *                         bytes at ph_buf_host_ptr() are valid after ph_wait_finish(queue) or after a
 *                         ph_event recorded behind it has been waited for.
 * (Upload without a host wait already exists: PH_HOST_WRITEONLY with no src, fill the mirror,
 * PH_HOST_NONE.) */
int ph_queue_wait_queue(ph_ctx *ctx, int waiter_queue, int signal_queue);
int ph_buf_download_async(ph_buf *buf, int queue);
/* a point in a queue the host can wait for without draining what was enqueued after it (one per
 * ring slot in a staged chain).  ph_event_wait returns when the work enqueued before the record has
 * finished; the event stays valid until ph_event_destroy. */
typedef struct ph_event ph_event;
int ph_event_record(ph_ctx *ctx, int queue, ph_event **out);
int ph_event_wait(ph_event *ev);
int ph_event_query(ph_event *ev); /* 1 = finished, 0 = still running, negative = error */
int ph_event_destroy(ph_event *ev);
/* Timed points: ph_event_record_timed records an event that ph_event_elapsed_us can measure from / to (microseconds of device
 * time between two such points of one queue, both finished).  nodencl's RunTimings (clJobQueue.ts:159-215 prints them) for a binding
 * whose launches do not coincide with its runProgram calls (node/defer.js with `profile`). */
int ph_event_record_timed(ph_ctx *ctx, int queue, ph_event **out);
int ph_event_elapsed_us(ph_event *from, ph_event *to, uint32_t *microseconds);
/* Recorded batches.  The reference submits a channel's per-frame batch (read x N, transform x N, wipe,
 * combine, write: 13 kernels at config 2) one `runProgram` at a time; at 1080p those kernels run for
 * 5-15 us each and the gaps between launches are a fifth of the frame.  A caller whose batch touches
 * the same buffers every frame (ring slots) can record it once and replay it as ONE submission:
 *   ph_graph_begin(ctx, queue)  - every launch issued on `queue` from this thread is recorded, not run
 *                                 (hipStreamBeginCapture); no waitFinish / hostAccess('readonly') inside
 *   ph_graph_end(ctx, queue, &g) - stop recording, build the executable graph
 *   ph_graph_launch(g, queue)   - replay on `queue` (asynchronous, ordered like any other launch)
 * Scalars and pointers are frozen at recording time. */
typedef struct ph_graph ph_graph;
int ph_graph_begin(ph_ctx *ctx, int queue);
int ph_graph_end(ph_ctx *ctx, int queue, ph_graph **out);
int ph_graph_launch(ph_graph *graph, int queue);
int ph_graph_destroy(ph_graph *graph);
/* ---- ROUTE across GPUs (src/producer/routeProducer.ts:63-126, src/channel.ts:290-300).  In the reference a
 *      route producer taps another channel's combiner output by taking a reference on the same OpenCL buffer:
 *      one process, one device.  Here channels are partitioned one process per GPU, so a route whose
 *      two ends live on different GPUs becomes ONE point-to-point message per frame: RCCL send / recv over xGMI
 *      on a communication stream of its own, ordered against the compute queues on the device:
 *        source rank:  combine ... ; ph_route_after_queue(r, PROCESS); ph_route_send(r, frame, peer)
 *        sink rank:    ph_route_recv(r, frame, peer); ph_queue_after_route(r, PROCESS); combine(... frame ...)
 *      so the transfer overlaps whatever else the sink's process queue runs before that combine (its own layers'
 *      v210 reads), and no host thread waits.  Sends / receives of one frame period go between
 *      ph_route_group_begin / _end (ncclGroupStart / End): every rank may then post them in any order.
 *      librccl is loaded on first use (dlopen); a process that never routes never needs it.
 *      ph_route_unique_id: 128 bytes made by ONE rank and handed to the others out of band (the caller's own
 *      control channel - torch.distributed in this repo's tools, a socket in a node deployment). ------------- */
typedef struct ph_route ph_route;
#define PH_ROUTE_ID_BYTES 128
int ph_route_unique_id(void *id128);
int ph_route_init(ph_ctx *ctx, const void *id128, int rank, int world, ph_route **out);
int ph_route_destroy(ph_route *route);
int ph_route_group_begin(ph_route *route);
int ph_route_group_end(ph_route *route);
/* device pointers (ph_buf_device_ptr / a wrapped tensor); bytes % 4 == 0; peer == own rank is allowed inside a group */
int ph_route_send(ph_route *route, const void *device_src, size_t bytes, int peer);
int ph_route_recv(ph_route *route, void *device_dst, size_t bytes, int peer);
/* the communication stream waits for everything enqueued so far on `queue` (the frame being sent is complete) */
int ph_route_after_queue(ph_route *route, int queue);
/* `queue` waits for everything enqueued so far on the communication stream (the received frame has landed) */
int ph_queue_after_route(ph_route *route, int queue);
int ph_route_wait(ph_route *route); /* host wait for the communication stream (tests, shutdown) */
void *ph_route_stream(ph_route *route);
/* ranks in the route's RCCL communicator (ncclCommCount): what RCCL itself saw, not what the caller passed in */
int ph_route_comm_count(ph_route *route, int *count);
/* Buffer lifetime: a frame handed to ph_route_send may be RELEASED right after the call - the pool orders the three
 * queues behind the transfers in flight before it hands a recycled block out again.  REWRITING the same buffer (a
 * source that composes the next frame into it) needs ph_queue_after_route(route, queue) first, like any other
 * cross-stream reuse. */

/* the `logBuffers()` debug hook (src/index.ts:184): live buffers / pooled bytes */
int ph_ctx_buffer_stats(ph_ctx *ctx, size_t *live_buffers, size_t *live_bytes, size_t *pooled_bytes);
/* the pinned host mirrors (an OpenCLBuffer of the node binding IS its mirror): bytes attached to live buffers, bytes kept for reuse,
 * the most that was ever attached at once, and how many blocks have been pinned (hipHostMalloc) since the context was made - a
 * count that keeps growing in steady state means the pool is smaller than the working set (context option "host_pool_mb") */
int ph_ctx_host_pool_stats(ph_ctx *ctx, size_t *in_use_bytes, size_t *pooled_bytes, size_t *peak_in_use_bytes, uint64_t *pins);

/* ---- programs: `createProgram(kernelSrc, {name, globalWorkItems, workItemsPerGroup})`
 *      (imageProcess.ts:69-72, packer.ts:97-103).  The OpenCL C text is NOT compiled: it (or a
 *      "phaneron:<op>" tag) only selects a precompiled gfx950 kernel by kernel name + argument
 *      list.  Names: read/write (v210, yuv422p10le, yuv422p8, yuv420p, nv12, rgba8, bgra8 - told
 *      apart by their argument lists), yadif, transform, resize, combine_N, transition_dissolve,
 *      transition_wipe, mixer, wipe. ------------------------------------------------------------ */
int ph_program_create(ph_ctx *ctx, const char *kernel_src, const char *name,
                      const uint32_t *global_work_items, int n_dims,
                      uint32_t work_items_per_group, ph_program **out);
/* The selection alone, without a context or a device (same rules, same errors): writes the resolved
 * kernel id ("v210_read", "yuv420p_write", "combine_4", ...), the PH_FMT_* of a read / write program
 * (-1 otherwise) and HOW it was selected - by "phaneron:" tag, by unique kernel name, by the exact text of
 * one of the reference's seven pack-format sources, or (any other text) by the kernel's argument list. */
enum { PH_RESOLVED_BY_TAG = 0, PH_RESOLVED_BY_NAME = 1, PH_RESOLVED_BY_TEXT = 2, PH_RESOLVED_BY_SIGNATURE = 3 };
int ph_program_resolve(const char *kernel_src, const char *name, char *kernel_id, size_t kernel_id_len,
                       int *format, int *how);
int ph_program_destroy(ph_program *prog);
const char *ph_program_kernel(const ph_program *prog); /* resolved kernel id, e.g. "v210_read" */

/* ---- `runProgram(program, params, queue)` (clJobQueue.ts:126): params keyed by the OpenCL
 *      kernel ARGUMENT NAME (input, output, width, colMatrix, gammaLut, gamutMatrix, interlace,
 *      prev, cur, next, parity, tff, skipSpatial, transformMatrix, scale, offsetX, offsetY, flip,
 *      l<i>In, input0, input1, mix, wipe, maskIn) ------------------------------------------------- */
enum { PH_ARG_BUF = 0, PH_ARG_U32 = 1, PH_ARG_I32 = 2, PH_ARG_F32 = 3 };
typedef struct ph_arg {
  const char *name;
  int kind;
  union {
    ph_buf *buf;
    uint32_t u32;
    int32_t i32;
    float f32;
  } v;
} ph_arg;
/* nodencl `RunTimings` in microseconds (clJobQueue.ts:159-215 prints them) */
typedef struct ph_run_timings {
  uint32_t data_to_kernel;
  uint32_t kernel_exec;
  uint32_t total_time;
} ph_run_timings;
/* timings may be NULL (no events recorded, fully asynchronous).  With timings the call
 * returns after the kernel has finished (hipEvent pair on the queue's stream). */
int ph_run_program(ph_ctx *ctx, ph_program *prog, const ph_arg *args, int n_args, int queue,
                   ph_run_timings *timings);
/* Everything ph_run_program checks before it launches - argument names and kinds, buffer sizes against the frame geometry,
 * image-ness - with nothing enqueued and no buffer touched: the same return codes and ph_last_error() texts.  For a binding
 * that records jobs and launches them later (node/defer.js): a bad job is reported where the reference posts it
 * (clJobQueue.ts:126 awaits runProgram), not where it is finally run. */
int ph_check_program(ph_ctx *ctx, ph_program *prog, const ph_arg *args, int n_args, int queue);
/* Several jobs in one call, for a binding that records jobs and launches them later (node/defer.js): exactly ph_run_program(progs[j],
 * args[j], n_args[j]) for j = 0 .. n_jobs - 1 in that order (a job that reads or writes what an earlier job of the call writes, or writes what one
 * reads, is kept out of that job's launch).  Every job is
 * checked before anything is launched (a bad job refuses the whole call).  Channel frames among the jobs - chan_compose_v210_<n>
 * programs of one geometry that name the SAME Loader / Saver buffers and make v210 frames - go to the device together
 * (ph_chan_compose_batch: the reference's channels share one context and one queue, src/index.ts:45-71,156-160); likewise consecutive
 * fused_v210_combine_<n> programs of one geometry, layer count and recipe (ph_fused_v210_combine_batch, up to eight per launch; a frame
 * that touches an earlier one's output starts the next launch), and consecutive compose_up_write_v210_<n> jobs of one shape - layer count,
 * image format and sizes, placements, frame size, field mode, Saver - each one frame or a frame's two fields (ph_compose_up_write_v210_batch, up to four frames
 * per launch).  A chan_compose_multi_<n> job - chan_compose_v210_<n>'s arguments for output 0 and, for outputs k = 1..3, out<k>Packing,
 * output<k> (output<k>U / V / C), out<k>ColMatrix, out<k>GammaLut, interlace<k>: ph_chan_compose_multi - runs in its turn as a launch of its own.
 * So does a clip_compose_multi_<n> job: the same arguments, name for name, through ph_clip_compose_multi (grouped across jobs only with the
 * context option "clip_batch" = 1: consecutive such jobs of one geometry and Loader recipe in one ph_clip_compose_batch_out call).
 * So does a clip_compose_trans_<n> job (ph_clip_compose_transition_multi: the same arguments, the transition's l<i>Transition, l<i>Mix,
 * l<i>Incoming... and l<i>Mask... included), which no option groups.
 * So does a clip_compose_route_<n> job (ph_clip_compose_route_multi: clip_compose_multi_<n>'s arguments and the optional buffer imageOut, the
 * combined f32 RGBA image; `output` may be absent only where imageOut is there), which no option groups either: no shared launch reaches
 * across it, so the image it writes is there for the next job and everything before it has been read or written.
 * So does a compose_up_multi_<n> job (ph_compose_up_write_multi): compose_up_write_v210_<n>'s layers (l<i>In, l<i>Matrix, packedRgb,
 * l<i>Width / l<i>Height) and chan_compose_multi_<n>'s outputs.  Its twin - the other field of a de-interlaced frame - is announced by
 * l0In2 (l<i>In2: its images), and its planes carry the first job's names behind the word twin: twinOutput (twinOutputU / V / C),
 * twinOutput<k> (twinOutput<k>U / V / C) - `output2` being output 2's frame here.
 * A compose_up_trans_<n> job (ph_compose_up_transition_multi) takes the same arguments and, per layer, the keys chan_compose_v210_<n> has
 * for a transition: l<i>Transition (0 cut / 1 dissolve / 2 wipe), l<i>Mix, l<i>IncomingIn, l<i>IncomingMatrix and - with packedRgb -
 * l<i>IncomingWidth / l<i>IncomingHeight, the same with Mask for a wipe; for the twin l<i>IncomingIn2, l<i>MaskIn2 and l<i>Mix2 (default:
 * l<i>Mix).
 * A fused_v210_trans_<n> job (ph_fused_v210_transition_multi) takes fused_v210_combine_multi_<n>'s arguments and, per layer, l<i>Transition (0
 * cut / 1 dissolve / 2 wipe, default 0), l<i>Mix, l<i>IncomingIn - a v210 frame of the output's size - and for a wipe l<i>MaskIn with
 * l<i>MaskPacking: 0 (PH_FMT_V210) the buffer is a v210 frame, absent it is an f32 RGBA image of the output's size.  A launch of its own,
 * in its turn.
 * A fused_v210_route_<n> job (ph_fused_v210_route_multi) takes fused_v210_combine_multi_<n>'s arguments and l<i>Image: 1 marks l<i>In as
 * an f32 RGBA image of width x height x 16 bytes (absent or 0: a v210 frame); the optional buffer imageOut receives the combined image,
 * and `output` may be absent only when imageOut is there (no packed frame at all).  A launch of its own, in its turn.
 * And so does a pack_write_multi_<n> job (ph_pack_write_multi; globalWorkItems [width, height]): input - the f32 RGBA image - width, and
 * its n = 1..4 outputs as chan_compose_multi_<n> names them, outPacking / out<k>Packing being any PH_FMT_* here (7 and 8 included). */
int ph_run_programs(ph_ctx *ctx, int n_jobs, ph_program *const *progs, const ph_arg *const *args, const int *n_args, int queue);
/* How far the calling thread's LAST ph_run_programs call got: the launches of jobs 0 .. *jobs_done - 1 were made (n_jobs after a call
 * that returned PH_OK, 0 after one refused by its checks).  A call that fails at a launch has enqueued the jobs before the failing
 * group; a binding that falls back to ph_run_program for the rest starts at *jobs_done instead of rendering those frames twice. */
int ph_run_programs_progress(int *jobs_done);

/* ---- typed entry points: the same kernels on raw device pointers, launched on `queue`.
 *      Images are row-major float RGBA (16 B/pixel); v210 is LE 32-bit words with line pitch
 *      ph_v210_pitch_bytes(width).  Matrices / LUTs are DEVICE pointers (the reference passes
 *      them as OpenCLBuffers, loadSave.ts:114-127). --------------------------------------------- */
uint32_t ph_v210_pitch_bytes(uint32_t width); /* v210.ts:198-204 */
/* v210.ts:25-111 */
int ph_v210_read(ph_ctx *ctx, int queue, const void *in, void *out, uint32_t width, uint32_t height,
                 const void *col_matrix12, const void *gamma_lut, const void *gamut_matrix9);
/* n frames of one size and one colour recipe (the layers of a channel) unpacked in one launch; outs[i] receives exactly
 * what ph_v210_read(ins[i]) writes.  The launch and the per-CU table load are paid once per batch. */
int ph_v210_read_batch(ph_ctx *ctx, int queue, int n, const void *const *ins, void *const *outs, uint32_t width,
                       uint32_t height, const void *col_matrix12, const void *gamma_lut, const void *gamut_matrix9);
/* v210.ts:113-195; interlace 0 / 1 (top, even lines) / 3 (bottom, odd lines) (packer.ts:24-28) */
int ph_v210_write(ph_ctx *ctx, int queue, const void *in, void *out, uint32_t width,
                  uint32_t height, uint32_t interlace, const void *col_matrix12,
                  const void *gamma_lut);
/* yadifCl.ts:105-167 */
int ph_yadif(ph_ctx *ctx, int queue, const void *prev, const void *cur, const void *next, int width,
             int height, int parity, int tff, int skip_spatial, void *out);
/* Both output fields of one frame in one pass: out_parity0 / out_parity1 receive exactly what ph_yadif writes with
 * parity 0 / parity 1 (the Yadif wrapper's send_field mode runs the filter twice per frame over the same window,
 * parity 1 ^ tff then parity tff: yadif.ts:100-145).  Each source row is read once instead of up to twice. */
int ph_yadif_pair(ph_ctx *ctx, int queue, const void *prev, const void *cur, const void *next, int width,
                  int height, int tff, int skip_spatial, void *out_parity0, void *out_parity1);
/* ---- fused de-interlacing reader (no single reference equivalent): per layer, ToRGBA on the frames of the Yadif
 *      window (v210.ts:25-111) and both send_field outputs of Yadif (yadif.ts:100-145) as ONE kernel.  The window
 *      stays in v210; its rows are unpacked, matrixed and gamma-corrected on the fly, and only the two de-interlaced
 *      RGBA frames are written.  out_parity0 / out_parity1 are bit-identical to ph_v210_read on prev, cur and next
 *      followed by ph_yadif with parity 0 / 1.  n sources of one size and one colour recipe per call (the layers of a
 *      channel).  Needs width % 6 == 0 and the reader LUT registered (PH_E_INVALID otherwise - run the separate kernels). */
/* (ABI 4 and later: 88 bytes - the six chroma-plane pointers were added behind the original five; an array of the 40-byte
 * struct of ABI 2 / 3 has the wrong stride, see the ABI history at the top) */
typedef struct ph_deint_source {
  const void *prev, *cur, *next;      /* device, v210, width x height (ph_yadif_pair_packed: or the Y planes of planar frames) */
  void *out_parity0, *out_parity1;    /* device, float RGBA, width x height */
  const void *prev_u, *prev_v, *cur_u, *cur_v, *next_u, *next_v; /* ph_yadif_pair_packed with a planar packing: the chroma planes */
} ph_deint_source;
int ph_v210_yadif_pair(ph_ctx *ctx, int queue, int n, const ph_deint_source *sources, uint32_t width, uint32_t height,
                       int tff, int skip_spatial, const void *rd_col_matrix12, const void *rd_gamma_lut,
                       const void *rd_gamut_matrix9);
/* the same with a choice of output layout.  PH_IMG_RGB_F32: three floats per pixel (12 bytes, rows unpadded) - what a
 * v210 reader computes, without the alpha it sets to 1 (v210.ts:73-77, yadifCl.ts:164).  Only ph_compose_up_write_v210
 * reads that layout: a quarter less to write here and to fetch there. */
#define PH_IMG_RGBA_F32 0
#define PH_IMG_RGB_F32 1
int ph_v210_yadif_pair_fmt(ph_ctx *ctx, int queue, int n, const ph_deint_source *sources, uint32_t width, uint32_t height,
                           int tff, int skip_spatial, int out_format, const void *rd_col_matrix12, const void *rd_gamma_lut,
                           const void *rd_gamut_matrix9);
/* the same over windows of interlaced FILE frames: packing = PH_FMT_YUV422P10 or PH_FMT_YUV422P8 (planar 4:2:2, what decoders of
 * XDCAM / ProRes / DNxHD material hand over), PH_FMT_YUV420P or PH_FMT_NV12 (4:2:0: interlaced H.264 / MPEG-2; nv12: *_u are the
 * interleaved CbCr planes, *_v unused; even heights) - every source of the call in that packing, unpacked with the call's Loader recipe
 * (for the 8-bit packings the 8-bit Loader's matrix) - or PH_FMT_V210 (= the call above) */
int ph_yadif_pair_packed(ph_ctx *ctx, int queue, int n, const ph_deint_source *sources, int packing, uint32_t width, uint32_t height,
                         int tff, int skip_spatial, int out_format, const void *rd_col_matrix12, const void *rd_gamma_lut,
                         const void *rd_gamut_matrix9);

/* Extension (no reference kernel): a packed f32 RGB image (12 bytes per pixel; PH_IMG_RGB_F32, what ph_v210_yadif_pair_fmt can write) expanded IN
 * PLACE into the f32 RGBA image (alpha 1) its buffer is declared as - through the queue's scratch area.  Program name "rgb_unpack"
 * (argument `image`).  For a binding that keeps de-interlaced fields packed while only ph_compose_up_write_v210 reads them. */
int ph_image_unpack_rgb(ph_ctx *ctx, int queue, void *image, int w, int h);
/* transform.ts:36-59 (matrix9: device pointer to the 3x3 row-major matrix) */
int ph_transform(ph_ctx *ctx, int queue, const void *in, int in_w, int in_h, const void *matrix9,
                 void *out, int out_w, int out_h);
/* resize.ts:35-59 (flip4: device pointer) */
int ph_resize(ph_ctx *ctx, int queue, const void *in, int in_w, int in_h, float scale,
              float offset_x, float offset_y, const void *flip4, void *out, int out_w, int out_h);
/* combine.ts:24-68, 2 <= n <= 8 */
int ph_combine(ph_ctx *ctx, int queue, int n, const void *const *layers, int width, int height,
               void *out);
/* transition.ts:60-65 / :66-74, mix.ts:30-45, wipe.ts:30-47 */
int ph_transition_dissolve(ph_ctx *ctx, int queue, const void *in0, const void *in1, float mix,
                           int width, int height, void *out);
int ph_transition_wipe(ph_ctx *ctx, int queue, const void *in0, const void *in1, const void *mask,
                       int width, int height, void *out);
int ph_mixer(ph_ctx *ctx, int queue, const void *in0, const void *in1, float mix, int width,
             int height, void *out);
int ph_wipe(ph_ctx *ctx, int queue, const void *in0, const void *in1, float wipe, int width,
            int height, void *out);

/* ---- the other pack formats (src/process/{yuv422p10,yuv422p8,yuv420p,nv12,rgba8,bgra8}.ts):
 *      planes as the reference's Readers/Writers lay them out (numBytes[] of each format).  v210
 *      is accepted too (format 0, one plane).  col_matrix12 is NULL for the RGB formats (their
 *      Loader/Saver skip it: loadSave.ts:52-61,141-149).  Returns the number of planes. ---------- */
enum {
  PH_FMT_V210 = 0,
  PH_FMT_YUV422P10 = 1,
  PH_FMT_YUV422P8 = 2,
  PH_FMT_YUV420P = 3,
  PH_FMT_NV12 = 4,
  PH_FMT_RGBA8 = 5,
  PH_FMT_BGRA8 = 6,
  /* 10-bit 4:2:0 decoder frames (no reference kernel; defined through the yuv422p10 Reader / Writer: DESIGN.md 2).  Even widths and
   * heights; P = the width rounded up to 8 samples; 16-bit little-endian samples; Loader / Saver recipe the 10-bit one (v210, yuv422p10).
   * read: chroma line r >> 1 serves line r; write: chroma from the upper line of a line pair (the lower one in field mode 3) */
  PH_FMT_YUV420P10 = 7, /* yuv420p10le: Y [h][P], Cb / Cr [h/2][P/2], LSB-aligned (the whole word is the sample, as yuv422p10) */
  PH_FMT_P010 = 8       /* p010le: Y [h][P], CbCr [h/2][P] interleaved, Cb first, MSB-aligned (read: word >> 6; write: code << 6) */
};
int ph_pack_plane_bytes(int format, uint32_t width, uint32_t height, size_t bytes[3]);
int ph_pack_read(ph_ctx *ctx, int queue, int format, const void *const planes[3], void *out,
                 uint32_t width, uint32_t height, const void *col_matrix12, const void *gamma_lut,
                 const void *gamut_matrix9);
/* n frames (1 .. 8) of ONE format, size and Loader recipe in one launch - several channels' clips of a tick (the reference's channels share a
 * context and a queue: src/index.ts:45-71,156-160): planes[i] are frame i's planes as ph_pack_read takes them, outs[i] its f32 RGBA image.
 * Exactly n ph_pack_read calls; PH_FMT_V210 goes to ph_v210_read_batch. */
int ph_pack_read_batch(ph_ctx *ctx, int queue, int format, int n, const void *const (*planes)[3], void *const *outs, uint32_t width,
                       uint32_t height, const void *col_matrix12, const void *gamma_lut, const void *gamut_matrix9);
int ph_pack_write(ph_ctx *ctx, int queue, int format, const void *in, void *const planes[3],
                  uint32_t width, uint32_t height, uint32_t interlace, const void *col_matrix12,
                  const void *gamma_lut);

/* ---- fused channel pipeline (no reference equivalent: it is the reference's job batch
 *      [v210 read] x n -> combine_n -> v210 write executed as ONE kernel with the
 *      f32 RGBA intermediates kept in registers).  Bit-identical to running the separate
 *      kernels above.  1 <= n <= 8 (n == 1: combiner passthrough, combiner.ts:222-228).
 *      All layers share one reader colourspec (matrices/LUT are device pointers). ------------- */
int ph_fused_v210_combine(ph_ctx *ctx, int queue, int n, const void *const *layers, void *out,
                          uint32_t width, uint32_t height, const void *rd_col_matrix12,
                          const void *rd_gamma_lut, const void *rd_gamut_matrix9,
                          const void *wr_col_matrix12, const void *wr_gamma_lut);
/* The same for `jobs` frames in ONE launch (channels of identical geometry and colour parameters, e.g.
 * the 1080p channels of BASELINE config 4 / 5 sharing a GPU): layers[j * n + l] is layer l of job j,
 * outs[j] its output.  The CUs are divided between the jobs, so launch, table loads and the
 * partially filled last slice are paid once per batch instead of once per frame: four 1080p frames
 * cost what one 2160p frame costs.  Up to 8 jobs; results identical to `jobs` separate calls. */
int ph_fused_v210_combine_batch(ph_ctx *ctx, int queue, int jobs, int n, const void *const *layers,
                                void *const *outs, uint32_t width, uint32_t height, const void *rd_col_matrix12,
                                const void *rd_gamma_lut, const void *rd_gamut_matrix9, const void *wr_col_matrix12,
                                const void *wr_gamma_lut);

/* ---- fused layer compositor (no single reference equivalent): the reference's job batches
 *      [transform] per layer (producer/mixer.ts:189-228) -> combine_N (combiner.ts:219-254) ->
 *      v210 write (io.ts:152-164) as ONE kernel, so the N + 1 consumer-size f32 RGBA frames between
 *      them never reach HBM.  Bit-identical to ph_transform x N + ph_combine + ph_v210_write.
 *      A layer with matrix9 == NULL is used 1:1 and must have the output size.  n == 1: passthrough
 *      of the single (transformed) layer as the combiner does.  Any even out_width (one that is not a
 *      multiple of 48 - 1280 - is served by the quad-per-lane kernel with the reference's tail
 *      arithmetic); the writer LUT must be registered (LDS form).  interlace as ph_v210_write. -- */
typedef struct ph_layer {
  const void *rgba;     /* device, float RGBA, width x height */
  int width, height;
  const void *matrix9;  /* device 3x3 transform matrix (ph_transform_matrix), or NULL */
} ph_layer;
int ph_compose_write_v210(ph_ctx *ctx, int queue, int n, const ph_layer *layers, void *out,
                          uint32_t out_width, uint32_t out_height, uint32_t interlace,
                          const void *wr_col_matrix12, const void *wr_gamma_lut);

/* The same compositor with wipe transitions inside: layer i's placed image is mixed with wipes[i].incoming_rgba by
 * the red channel of wipes[i].mask_rgba (transition.ts wipe, as the Transitioner runs it: transitioner.ts:165-176)
 * before the combine - [transform] -> transition_wipe -> combine_N -> write of a channel in mid-wipe as one kernel,
 * bit-identical to ph_transform + ph_transition_wipe + ph_combine + ph_v210_write.  Both images have the output
 * size; an entry with two NULLs leaves its layer alone.  Needs out_width % 192 == 0 (PH_E_INVALID otherwise). */
typedef struct ph_layer_wipe {
  const void *incoming_rgba; /* device, float RGBA, output size: the source the wipe reveals */
  const void *mask_rgba;     /* device, float RGBA, output size: mix factor in .x */
} ph_layer_wipe;
int ph_compose_wipe_write_v210(ph_ctx *ctx, int queue, int n, const ph_layer *layers, const ph_layer_wipe *wipes,
                               void *out, uint32_t out_width, uint32_t out_height, uint32_t interlace,
                               const void *wr_col_matrix12, const void *wr_gamma_lut);

/* ---- the compositor for magnified layers (no single reference equivalent): [transform] x N -> combine_N -> v210 write
 *      as ph_compose_write_v210, for placements that enlarge every layer (by 1 % or more) without rotation or mirroring -
 *      Mixer's default fill of HD sources on a UHD channel (producer/mixer.ts:209-223).  A lane produces a 2 x 2 block
 *      of output pixels from ONE 3 x 3 patch of each source (neighbouring output pixels share their taps): 2.25 texel
 *      loads per layer and pixel instead of 4.  Sources are f32 RGBA images or packed f32 RGB (PH_IMG_RGB_F32, alpha
 *      == 1 implied: ph_v210_yadif_pair_fmt), all layers of a call in the same layout.  Bit-identical to ph_transform +
 *      ph_combine + ph_v210_write.  A field write (interlace 1 / 3) needs more than 2x vertically: its rows are two lines apart.
 *      One placement at scale one qualifies too: an image of the frame's size under the Mixer's default fill (the identity matrix, a
 *      frame write) - de-interlaced 1080i fields on a 1080 channel.
 *      PH_E_INVALID when a placement does not qualify (use ph_compose_write_v210),
 *      out_width % 48 != 0 or the writer LUT is not registered.  interlace as ph_v210_write. ------------------- */
typedef struct ph_image_layer {
  const void *data;          /* device: width x height texels, rows unpadded */
  int format;                /* PH_IMG_RGBA_F32 | PH_IMG_RGB_F32 */
  int width, height;
  const float *matrix9_host; /* HOST: the nine values of ph_transform_matrix */
} ph_image_layer;
int ph_compose_up_write_v210(ph_ctx *ctx, int queue, int n, const ph_image_layer *layers, void *out, uint32_t out_width,
                             uint32_t out_height, uint32_t interlace, const void *wr_col_matrix12, const void *wr_gamma_lut);
/* Both fields of a de-interlaced frame in ONE launch: exactly ph_compose_up_write_v210(layers_a -> out_a) followed by
 * ph_compose_up_write_v210(layers_b -> out_b), for two sets of layers that differ in their data only (same count, formats, sizes and
 * placements: the parity-0 and parity-1 outputs of ph_v210_yadif_pair_fmt under one Mixer setting).  One launch, one table load and one
 * partly filled last round of wave steps instead of two. */
int ph_compose_up_write_v210_pair(ph_ctx *ctx, int queue, int n, const ph_image_layer *layers_a, const ph_image_layer *layers_b, void *out_a,
                                  void *out_b, uint32_t out_width, uint32_t out_height, uint32_t interlace, const void *wr_col_matrix12,
                                  const void *wr_gamma_lut);
/* The same for 1 .. 4 sets of layers that differ in their data only - several channels showing clips of one size under one placement
 * (the reference's channels share a context and a queue: src/index.ts:45-71,156-160): layer_sets[j][l] is layer l of job j, outs[j] its
 * output (all different).  The jobs of one call run side by side: no job may read - as a layer image - what another job of the call
 * writes (ph_run_programs sees to that for its by-name jobs).  ph_chan_compose_batch uses it for the frames of enlarged clips among its jobs. */
int ph_compose_up_write_v210_batch(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *layer_sets, void *const *outs,
                                   uint32_t out_width, uint32_t out_height, uint32_t interlace, const void *wr_col_matrix12,
                                   const void *wr_gamma_lut);

/* ---- the channel compositor straight from the wire format (no single reference equivalent): a channel's whole
 *      per-frame job batch - per layer ToRGBA (io.ts:79-98, v210.ts:25-111) -> Mixer transform (producer/mixer.ts:
 *      209-223, transform.ts:36-59) -> optionally the Transitioner's dissolve / wipe against a second source
 *      (transitioner.ts:165-176, transition.ts:54-79) -> combine_N (combiner.ts:219-254) -> FromRGBA (io.ts:152-164,
 *      v210.ts:113-195) - as ONE kernel that samples the v210 words themselves: each bilinear tap is unpacked,
 *      matrixed, gamma-looked-up and gamut-converted on the fly, so no f32 frame reaches HBM at all.  Bit-identical
 *      to ph_v210_read + ph_transform (+ ph_transition_dissolve / ph_transition_wipe) + ph_combine + ph_v210_write.
 *      A source is a v210 frame or (e.g. a routed frame, a generated mask) an f32 RGBA image; with matrix9_host ==
 *      NULL it is taken 1:1 and must have the output size.  All v210 sources share the reader's colour recipe.
 *      Limits (PH_E_INVALID otherwise - run the separate kernels): even widths for v210 frames, input or output (a width that
 *      is not a multiple of 6 / of 48 - 1280 x 720 - takes the reference's tail arithmetic, v210.ts:84-110,166-193, lines by
 *      pitch), planar output widths % 8 == 0, frames below 1 GiB, both gamma LUTs registered (LDS form).  interlace as
 *      ph_v210_write. ---------------------------------------------------------------------------------------------- */
#define PH_SRC_NONE 0
#define PH_SRC_V210 1
#define PH_SRC_RGBA_F32 2
/* planar YCbCr frames, as file decoders hand them over (ffmpegProducer.ts:398-412): data = the Y plane, data_u / data_v the chroma
 * planes (nv12: data_u = the interleaved CbCr plane, data_v unused), plane sizes as ph_pack_plane_bytes(PH_FMT_*, ...).  A 10-bit 4:2:2
 * Loader's matrix does not depend on the packing, so PH_SRC_YUV422P10 sources are unpacked with the call's Loader recipe like the
 * v210 ones; the 8-bit formats have code ranges of their own: col_matrix12 = that source's Loader matrix (its LUT and gamut
 * matrix are the call's: one colour space per call) */
#define PH_SRC_YUV422P10 3 /* yuv422p10.ts: 4:2:2, 16-bit little-endian samples */
#define PH_SRC_YUV422P8 4  /* yuv422p8.ts:  4:2:2, 8-bit */
#define PH_SRC_YUV420P 5   /* yuv420p.ts:   4:2:0, 8-bit */
#define PH_SRC_NV12 6      /* nv12.ts:      4:2:0, 8-bit, Cb and Cr interleaved */
/* packed 8-bit RGB (stills, graphics with alpha): four bytes per pixel, every byte - alpha too - through the call's gamma table,
 * r g b through its gamut matrix (rgba8.ts:49-62); no YCbCr matrix, no planes */
#define PH_SRC_RGBA8 7
#define PH_SRC_BGRA8 8
/* 10-bit 4:2:0 (PH_FMT_YUV420P10 / PH_FMT_P010): unpacked with the call's Loader recipe, like PH_SRC_YUV422P10 (p010: data_u = the
 * interleaved CbCr plane, data_v unused) */
#define PH_SRC_YUV420P10 9
#define PH_SRC_P010 10
typedef struct ph_chan_source {
  const void *data;          /* device: v210 words (pitch ph_v210_pitch_bytes(width)), float RGBA, or the Y plane; width x height */
  int format;                /* PH_SRC_V210 | PH_SRC_RGBA_F32 | a planar PH_SRC_* | PH_SRC_RGBA8 | PH_SRC_BGRA8 (PH_SRC_NONE: absent) */
  int width, height;
  const float *matrix9_host; /* HOST: the nine values of ph_transform_matrix, or NULL = 1:1 */
  const void *data_u, *data_v; /* planar formats: the chroma plane(s) (ignored otherwise) */
  const void *col_matrix12;  /* planar formats: DEVICE, this source's YCbCr -> RGB matrix, or NULL = the call's */
} ph_chan_source;
#define PH_TRANSITION_CUT 0
#define PH_TRANSITION_DISSOLVE 1 /* fma(src, mix, incoming * (1 - mix))            transition.ts:58-64 */
#define PH_TRANSITION_WIPE 2     /* fma(incoming, mask.r, src * (1 - mask.r))      transition.ts:66-77 */
typedef struct ph_chan_layer {
  ph_chan_source src;
  int transition;
  float mix;                     /* dissolve */
  ph_chan_source incoming, mask; /* the transition's second source and (wipe) its mask */
} ph_chan_layer;
int ph_chan_compose_v210(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, void *out, uint32_t out_width,
                         uint32_t out_height, uint32_t interlace, const void *rd_col_matrix12, const void *rd_gamma_lut,
                         const void *rd_gamut9, const void *wr_col_matrix12, const void *wr_gamma_lut);
/* The same with the packed frame in another wire format - FromRGBA with the Writers of the reference's other consumers: rgba8 / bgra8
 * (the screen, screenConsumer.ts:131; alpha 255, no writer matrix: wr_col_matrix12 may be NULL), yuv422p8 (an encoder,
 * ffmpegConsumer.ts:144), yuv422p10, and the 4:2:0 formats yuv420p / nv12 (yuv420p.ts:150-216, nv12.ts:139-196: chroma from the upper
 * line of a line pair; even heights; nv12: out_planes[1] is the interleaved CbCr plane); out_planes as ph_pack_plane_bytes(out_format,
 * ...) sizes them.  PH_FMT_V210 = the call above. */
int ph_chan_compose(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int out_format, void *const out_planes[3],
                    uint32_t out_width, uint32_t out_height, uint32_t interlace, const void *rd_col_matrix12, const void *rd_gamma_lut,
                    const void *rd_gamut9, const void *wr_col_matrix12, const void *wr_gamma_lut);
/* Several channels' frames in ONE launch.  The reference runs its channels - four of them, 1080p50 or smaller - in one context through
 * one queue (src/index.ts:45-71,156-160; src/clJobQueue.ts:114-141); a frame of that size does not fill the chip on its own.  Here the
 * jobs (frames of one geometry, one Loader / Saver colour recipe; each with its own layers, placements, transitions and interlace:
 * two jobs may be the two fields of one frame) share the workgroups of one launch: the gamma tables are loaded once, and the wave
 * steps of all jobs together are handed to the waves as they come free, dearest first.  Exactly `n_jobs` calls of ph_chan_compose_v210
 * in the order given, PROVIDED no job reads what another job of the call writes (jobs of one launch run side by side).  Jobs the
 * batch kernel does not take (planar / packed-RGB sources; more jobs, ops or wave steps than one launch holds) are split off into
 * launches of their own inside the call.  Limits and errors as ph_chan_compose_v210. */
typedef struct ph_chan_job {
  int n;                       /* layers */
  const ph_chan_layer *layers;
  void *out;                   /* device: the v210 frame, out_width x out_height */
  uint32_t interlace;          /* as ph_v210_write: 0 frame, 1 / 3 one field */
} ph_chan_job;
int ph_chan_compose_batch(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job *jobs, uint32_t out_width, uint32_t out_height,
                          const void *rd_col_matrix12, const void *rd_gamma_lut, const void *rd_gamut9, const void *wr_col_matrix12,
                          const void *wr_gamma_lut);
/* Several CONSUMERS' frames of one channel in one launch.  A channel owns a list of consumers (channel.ts:40,64-88), each of which runs
 * its own FromRGBA on the one combined image: v210 for SDI (fields on an interlaced channel), yuv422p8 for an encoder, rgba8 for the
 * screen.  Here the composition - every source's reader, transforms, transitions, combine - runs once, for the union of the lines the
 * outputs need, and only the writer's phase runs per output (outputs that name the same registered writer table share its load).
 * Exactly the `n_out` calls of ph_chan_compose with each output's format, planes, interlace and writer recipe, bit for bit.
 * n_out == 1 IS ph_chan_compose (same routes); 2..4 outputs are one launch of the channel kernel ("chan_compose_multi<mode>x<n_out>"
 * in a trace; the enlarged-clip route is not taken).  Limits and errors as ph_chan_compose, per output; two outputs naming the same
 * first plane, or n_out outside 1..4, are PH_E_INVALID.  A refused call writes nothing. */
typedef struct ph_chan_output {
  int format;                   /* a PH_FMT_* the channel kernel writes or, for ph_pack_write_multi, any PH_FMT_* */
  void *planes[3];              /* as ph_pack_plane_bytes(format, ...) sizes them */
  uint32_t interlace;           /* as ph_v210_write, per output */
  const void *wr_col_matrix12;  /* NULL for rgba8 / bgra8 */
  const void *wr_gamma_lut;     /* registered (LDS form) */
} ph_chan_output;
int ph_chan_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs,
                          uint32_t out_width, uint32_t out_height, const void *rd_col_matrix12, const void *rd_gamma_lut,
                          const void *rd_gamut9);
/* FILE PLAYBACK for any consumer, up to four per call.  A decoder's frame is uploaded at the clip's own size and the Mixer's transform
 * fills the channel with it (ffmpegProducer.ts:395-442, mixer.ts:189-228); for one v210 frame ph_chan_compose then reads every source
 * pixel once (its enlarged-clip routes) instead of converting four taps per output pixel.  This entry does the same for an encoder's
 * yuv422p10 / yuv422p8 / yuv420p / nv12 frame and the screen's rgba8 / bgra8, beside SDI's v210 or instead of it.  ph_chan_compose_multi's
 * signature and contract: exactly, bit for bit and in order, the `n_out` calls of ph_chan_compose with each output's format, planes,
 * interlace, matrix and table; it takes everything ph_chan_compose_multi takes and answers its errors (yuv420p10 / p010 outputs
 * included); every check of the arguments is made before the context is looked at, and a refused call writes nothing.
 * Routes, decided in this order.  (1) n_out == 1 with PH_FMT_V210 IS ph_chan_compose: same routes, same trace names.  (2) The lines
 * composed are the field every output wants, else the whole frame, of which a field output takes the rows of its parity.  (3) A call
 * whose layers are not all enlarged without rotation or mirroring (or decoders' frames of the channel's size under the default fill; no
 * transition), with the context option "chan_enlarged" = 0, or with a table that has no LDS form, runs ph_chan_compose_multi on the same
 * arguments inside the call, under that call's trace name.  (4) The outputs are grouped by registered writer table, in the order the
 * tables first appear; a v210 output at out_width % 48 != 0 (its tail quad truncates table indices where the other writers round) is
 * made by a ph_chan_compose call of its own.  (5) A group is ONE launch ("clip_up_multi<rgb|rgba>x<outputs>" in a trace: the format's
 * reader into an L2-resident rectangle per workgroup tile, the writer's table swapped in, the 2 x 2-block compositor, every output's
 * writer) where the frame is a single clip in a wire format - any PH_SRC_* but PH_SRC_RGBA_F32; a 4:2:0 one of an even height - and
 * "chan_enlarged" = 1; else two stages: each clip through its format's reader into the queue's scratch images (finished f32 images are
 * taken as they are), then "compose_up_multi<rgba>x<outputs>j1".  out_height == 0 is PH_OK.
 * With the context option "up_v210_tails" = 1 route (4)'s split is not made for a group of two or more outputs: the v210 output stays in
 * the group, whose launch is "clip_up_multi_t<rgb|rgba>x<outputs>" (two stages: "compose_up_multi_t<rgba>x<outputs>j1"); a group whose
 * only member is that v210 output, and n_out == 1, keep the routes above. */
int ph_clip_compose_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs,
                          uint32_t out_width, uint32_t out_height, const void *rd_col_matrix12, const void *rd_gamma_lut,
                          const void *rd_gamut9);
/* FILE PLAYBACK THROUGH A MIX OR WIPE: a playlist's transition from one clip to the next (LOADBG ... MIX 25, transitioner.ts:165-176) on the
 * read-once routes.  ph_clip_compose_multi's signature and contract: exactly, bit for bit and in order, the `n_out` calls of
 * ph_chan_compose with each output's format, planes, interlace, matrix and table - the chain ph_pack_read / ph_v210_read of every present
 * image -> ph_transform of each with its own matrix -> ph_transition_dissolve / ph_transition_wipe -> ph_combine -> ph_pack_write.  It takes
 * everything ph_chan_compose_multi takes and answers its errors (yuv420p10 / p010 outputs included); every check of the arguments is made
 * before the context is looked at, and a refused call writes nothing.  out_height == 0 is PH_OK.
 * Routes, decided in this order.  (1) Every layer PH_TRANSITION_CUT: IS ph_clip_compose_multi, same routes, same trace names.  (2) The
 * lines composed are the field every output wants, else the whole frame.  (3) Every PRESENT image - each layer's src, a dissolve's or
 * wipe's incoming, a wipe's mask - must qualify as a src does for ph_clip_compose_multi on the composed lines (enlarged by 1 % or more
 * without rotation or mirroring, or of the channel's size under the default fill on a frame write; a wire format or PH_SRC_RGBA_F32), the
 * reader's and every output's table must have an LDS form, planar outputs need out_width % 8 == 0, and "chan_enlarged" must not be 0:
 * else the call runs ph_chan_compose_multi on the same arguments, under that call's trace name.  (4) The outputs are grouped by registered
 * writer table, in the order the tables first appear; a v210 output at out_width % 48 != 0 is made by a ph_chan_compose call of its own.
 * (5) A group is ONE launch ("clip_up_trans<rgb|rgba>x<outputs>" in a trace: up to three rectangles per workgroup tile - src, incoming, mask,
 * each converted once per source pixel by its own format's reader - then the transition and every output's writer) where n == 1, every
 * present image is in a wire format (a 4:2:0 one of an even height) and "chan_enlarged" = 1; <rgb> where none of the images is rgba8 /
 * bgra8.  (6) Otherwise two stages: every wire-format image through its format's reader into the queue's scratch images (finished f32
 * images are taken as they are), then "compose_up_trans<rgba>x<outputs>j1" per table (the scratch images are f32 RGBA whatever the clips). */
int ph_clip_compose_transition_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, int n_out, const ph_chan_output *outs,
                                     uint32_t out_width, uint32_t out_height, const void *rd_col_matrix12, const void *rd_gamma_lut,
                                     const void *rd_gamut9);
/* A ROUTED CHANNEL'S FILE PLAYBACK: a ROUTE (routeProducer.ts:63-126, combiner.ts:219-254) hands another channel this channel's combined
 * image - an f32 RGBA frame of the channel's size, which arrives there as a PH_SRC_RGBA_F32 layer.  ph_clip_compose_multi's arguments and
 * `image_out` (f32 RGBA, out_width x out_height, rows unpadded, or NULL), `n_out` 0..4.
 * With image_out == NULL and n_out >= 1 the call IS ph_clip_compose_multi: same routes, trace names and errors.
 * With image_out the image is built in this order, bit for bit: the format's reader of every wire-format layer (ph_pack_read /
 * ph_v210_read; a PH_SRC_RGBA_F32 layer is taken as it is), ph_transform of each with its own matrix to the output size, ph_combine in
 * layer order into image_out (n == 1: the Combiner's passthrough, the one transformed image).  Every output is
 * ph_pack_write(image_out, ...) with its format, planes, interlace, matrix and table: ph_clip_compose_multi's frames on the same
 * arguments.  The whole frame is always composed; a field output takes the rows of its parity.  The arithmetic is ph_combine's, as
 * ph_fused_v210_route_multi states it: the bottom layer as it is (its -0 and its alpha included), above it k = 1 - l.a,
 * rgb = fma(acc, k, l), a = fma(acc.a, 0, l.a); a layer's filtered alpha is computed as a value,
 * ((w00 a00 + w10 a10) + w01 a01) + w11 a11, with 1 inside a clip that has no alpha and the border's 0 outside; only a NaN's payload is
 * unpinned.  image_out is stored under the context's store policy (option "stream_images"), as ph_combine stores its image.
 * Routes, decided in this order.  (1) The outputs are grouped by registered writer table as ph_clip_compose_multi groups them; the first
 * group's launch - or a launch with no output - also writes the image, further groups run ph_clip_compose_multi's launches; a v210
 * output at out_width % 48 != 0 is a ph_chan_compose call of its own; a lone v210 output belongs to the image's launch.  (2) ONE launch,
 * "clip_up_route<rgb|rgba>x<outputs>" in a trace, where n == 1, the clip is in a wire format (a 4:2:0 one of an even height) and
 * "chan_enlarged" = 1; <rgba> where the clip is rgba8 / bgra8.  (3) Otherwise two stages: every wire-format clip through its reader into
 * the queue's scratch images, then one "compose_up_route<rgba>x<outputs>j1" launch.  (4) With n_out == 0 no writer table is loaded or
 * looked at.  (5) PH_E_INVALID, naming the chain to run instead (ph_pack_read, ph_transform, ph_combine, ph_pack_write_multi), where the
 * call does not qualify for (2) / (3): a layer neither enlarged by 1 % or more without rotation or mirroring nor of the channel's size
 * under the default fill, a layer in a transition, "chan_enlarged" = 0, a table without an LDS form, a planar output at
 * out_width % 8 != 0: nothing else makes the image in one call, and the entry runs no chain of its own.  (6) Also refused: everything
 * ph_clip_compose_multi refuses (yuv420p10 / p010 outputs with the channel kernel's message), n_out outside 0..4, n_out == 0 with
 * image_out == NULL, image_out overlapping by byte range any source plane, f32 layer image or output plane.  Everything decidable from
 * the arguments is decided before the context is looked at; a refused call writes nothing; out_height == 0 is PH_OK. */
int ph_clip_compose_route_multi(ph_ctx *ctx, int queue, int n, const ph_chan_layer *layers, void *image_out, int n_out,
                                const ph_chan_output *outs, uint32_t out_width, uint32_t out_height, const void *rd_col_matrix12,
                                const void *rd_gamma_lut, const void *rd_gamut9);
/* Several CHANNELS' frames for any consumers in one launch: ph_chan_compose_batch's sharing (the tables loaded once, the wave steps of
 * all jobs in front of one barrier) with ph_chan_compose_multi's outputs - an encoder's yuv422p8 / yuv420p / nv12 frame, the screen's
 * rgba8 beside SDI's v210.  Exactly, in order, `n_jobs` calls of ph_chan_compose_multi (a job with n_out == 1: ph_chan_compose), bit for
 * bit.  The entry point itself sees to it that no job of a launch reads or writes what another job of it writes: a job that does starts
 * the next launch (two jobs may still be the two fields of one frame that is not 4:2:0).  A launch holds up to 4 jobs, 24 ops and 8
 * outputs of ONE writer table and one set of composed lines ("chan_compose_batch_out<0|1|2>x<jobs>o<outputs>" in a trace); longer calls
 * are split, and jobs a shared launch does not take - outputs that name another or several writer tables, one v210 frame that the
 * enlarged-clip routes serve better, more than 24 ops - run in their turn through ph_chan_compose_multi.  Limits and errors as
 * ph_chan_compose_multi, per job and output; every check is made before anything is launched: a refused call writes nothing. */
typedef struct ph_chan_job_out {
  int n;                       /* layers */
  const ph_chan_layer *layers;
  int n_out;                   /* 1..4 */
  const ph_chan_output *outs;  /* as ph_chan_compose_multi takes them */
} ph_chan_job_out;
int ph_chan_compose_batch_out(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job_out *jobs, uint32_t out_width, uint32_t out_height,
                              const void *rd_col_matrix12, const void *rd_gamma_lut, const void *rd_gamut9);
/* Several CHANNELS' FILE PLAYBACK for any consumers in one launch: ph_chan_compose_batch_out's signature, struct and contract with
 * ph_clip_compose_multi's frames.  Exactly, in order and bit for bit, the `n_jobs` calls of ph_clip_compose_multi (n_jobs == 1 IS that
 * call).  Every check of the arguments is made before the context is looked at; every job is checked and every launch planned before
 * anything is launched: a refused call writes nothing.  out_height == 0 is PH_OK.  Errors as ph_chan_compose_batch_out, per job and
 * output, under this entry's name (every table needs its LDS form).
 * Consecutive jobs share ONE launch of the clip kernel ("clip_up_multi<rgb|rgba>x<outputs>j<jobs>" in a trace; a workgroup's tile belongs
 * to one job) where each of them is a single clip in a wire format that ph_clip_compose_multi would make with one launch of that kernel
 * (route 5 there, "chan_enlarged" = 1, all its outputs naming one writer table, no v210 output at out_width % 48 != 0, not a lone v210
 * output), and all of them have one clip size and placement matrix, one alpha-ness (rgba8 / bgra8 clips against the others) and, output
 * by output, one format, interlace, writer matrix and writer table.  The clips' wire formats and Loader matrices may differ from job to
 * job.  A launch holds up to 4 jobs of up to 4 outputs; longer runs are split.  The entry point itself sees to it that no job of a
 * launch reads or writes what another job of it writes, or writes what one reads (by byte range): such a job starts the next launch.
 * Every other job - several layers, f32 images, the two-stage shapes, several writer tables, a lone v210 output, a v210 tail width - and
 * a group of one job run in their turn through ph_clip_compose_multi, under that call's trace names.
 * With the context option "up_v210_tails" = 1 the condition "no v210 output at out_width % 48 != 0" is dropped - such jobs share
 * "clip_up_multi_t<rgb|rgba>x<outputs>j<jobs>" - while "not a lone v210 output" stays. */
int ph_clip_compose_batch_out(ph_ctx *ctx, int queue, int n_jobs, const ph_chan_job_out *jobs, uint32_t out_width, uint32_t out_height,
                              const void *rd_col_matrix12, const void *rd_gamma_lut, const void *rd_gamut9);
/* Several consumers' frames of one ENLARGED composition in one launch: the 2 x 2-block compositor (ph_compose_up_write_v210) with any
 * writer the channel kernel has - v210, yuv422p10, yuv422p8, yuv420p, nv12, rgba8, bgra8 - and up to four outputs.  The composition
 * runs once; the block's twelve writer-table reads are made once, and every output packs the same twelve values with its own writer
 * matrix.  A screen (rgba8) or an encoder (yuv422p8) beside the SDI output of a channel whose sources are de-interlaced fields
 * (ph_v210_yadif_pair_fmt, packed RGB) costs no further launch, and no ph_image_unpack_rgb of the fields.
 * outs: jobs x n_out entries, job-major; entry [j][k] differs from [0][k] in its planes only.  jobs: 1..4 sets of layers that differ
 * in their data only, as ph_compose_up_write_v210_batch (the bound is the kernel's argument block: 4 jobs x 4 outputs x 3 planes).
 * Exactly the jobs x n_out separate frames, bit for bit: ph_compose_up_write_v210 for a v210 output, ph_transform x n + ph_combine +
 * ph_pack_write for the others.
 * Lines: if every output of a launch wants the same `interlace`, that field's rows are composed; otherwise the whole frame, a field
 * output taking the rows of its parity.  The placement must qualify (as ph_compose_up_write_v210) on the geometry that is composed.
 * Launches: outputs that name the same registered writer table share a launch ("compose_up_multi<rgb|rgba>x<outputs>j<jobs>" in a
 * trace); a call whose outputs name different tables is one launch per table, outputs keeping their order.  A v210 output whose
 * lines end in a tail quad (width % 48 != 0) truncates its table indices there where every other writer rounds: it is split off into
 * a launch of today's kernel ("compose_up_write_v210"), as is a v210 output that is alone with its table - so jobs = 1, n_out = 1,
 * PH_FMT_V210 IS ph_compose_up_write_v210.
 * PH_E_INVALID: a placement that does not qualify; a format the channel kernel does not write (yuv420p10, p010); an odd width, a
 * planar output whose width is not a multiple of 8, a 4:2:0 output with an odd height; n_out outside 1..4, jobs outside 1..4; two
 * outputs, of any job, naming the same first plane; a writer table that is not registered; layers of different image formats.
 * A refused call writes nothing.
 * With the context option "up_v210_tails" = 1 a v210 output at width % 48 != 0 that shares its table with at least one other output
 * stays in that table's launch ("compose_up_multi_t<rgb|rgba>x<outputs>j<jobs>" in a trace); alone with its table it is today's kernel's. */
int ph_compose_up_write_multi(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_layer *const *layer_sets, int n_out,
                              const ph_chan_output *outs, uint32_t out_width, uint32_t out_height);
/* The same with layers in a TRANSITION (transitioner.ts:165-176): a layer may bring the transition's second source and, for a wipe, its
 * mask - enlarged images like the layer itself, each with a size and a matrix of its own.  For every job and output the result is, bit
 * for bit, ph_transform of each present image (src, incoming, mask) with its own matrix to the output size, then
 * ph_transition_dissolve(src', incoming', mix) or ph_transition_wipe(src', incoming', mask') for the layers that have one, then
 * ph_combine over the n results (n == 1: the Combiner's passthrough), then ph_pack_write with the output's format, planes, interlace,
 * matrix and table - which is what ph_chan_compose_multi makes of the same layers given as PH_SRC_RGBA_F32 sources.
 * jobs: 1..4 (the argument block holds four jobs of eight layers with both partners).  Job j differs from job 0 in its images' data,
 * its outputs' planes and its `mix` values (the two fields of a tick pass the Transitioner one after the other:
 * transitioner.ts:170-175); layer count, transition kinds, image sizes, layouts and placements are job 0's.
 * All images of a call have one layout, PH_IMG_RGBA_F32 or PH_IMG_RGB_F32; a packed image has alpha 1 inside and the border's 0
 * outside, a packed mask gives its red.
 * Launches: with every layer PH_TRANSITION_CUT the call IS ph_compose_up_write_multi on the `src` layers (same routes, same trace
 * names).  Otherwise one launch per distinct registered writer table, outputs keeping their order
 * ("compose_up_trans<rgb|rgba>x<outputs>j<jobs>" in a trace) - a v210 output that is alone with its table included.
 * PH_E_INVALID, decided before anything is launched (a refused call writes nothing): everything ph_compose_up_write_multi refuses, per
 * job and output; a placement of ANY present image that does not qualify on the composed geometry; a transition outside 0..2; a
 * missing incoming image, or a missing mask for a wipe; with any layer in a transition, a v210 output at out_width % 48 != 0 (its tail
 * quad truncates table indices where the other writers round: send that frame to ph_chan_compose_multi).  out_height == 0 is PH_OK. */
typedef struct ph_image_trans_layer {
  ph_image_layer src;
  int transition;                /* PH_TRANSITION_CUT | _DISSOLVE | _WIPE */
  float mix;                     /* dissolve */
  ph_image_layer incoming, mask; /* the transition's second source and (wipe) its mask; ignored for CUT (the mask: for a dissolve too) */
} ph_image_trans_layer;
int ph_compose_up_transition_multi(ph_ctx *ctx, int queue, int jobs, int n, const ph_image_trans_layer *const *layer_sets, int n_out,
                                   const ph_chan_output *outs /* [jobs * n_out], job-major */, uint32_t out_width, uint32_t out_height);
/* One f32 RGBA image packed for up to four CONSUMERS in one call: a frame that exists as an image (a routed channel, a Combiner
 * passthrough, a frame whose fused launch was refused) and that every consumer runs its own FromRGBA on (channel.ts:40,64-88) - v210 for
 * SDI, p010 / yuv420p10 for a Main10 encoder, rgba8 for the screen.  outs: n_out = 1..4 outputs (ph_chan_output) in ANY
 * PH_FMT_*, the 10-bit 4:2:0 formats included.  Exactly, bit for bit and in order, the n_out calls of ph_pack_write with each output's
 * format, planes, interlace, matrix and table; the call takes everything those take.
 * Launches: outputs that name the same REGISTERED writer table share one launch ("pack_write_multi x<outputs>" in a trace), in which
 * every pixel is loaded once and looked up in the table once; each output then applies its own writer matrix and packing.  If every
 * output of the launch wants the same `interlace`, only that field's rows are read; otherwise the whole frame, a field output taking
 * the rows of its parity.  Outputs that name different tables are one launch per table, outputs keeping their order.  An output the
 * shared kernel does not take is split off into ph_pack_write's launch inside the call, under its present name: a table that is not
 * registered (or the context option "lds_lut" = 0), a planar output at width % 8 != 0 (the tail octet rounds twice), a v210 output at
 * width % 48 != 0 (its tail quad truncates the table index, and its cleared slots belong to the pitch), and an output that is alone
 * with its table - so n_out == 1 IS ph_pack_write, same route.
 * PH_E_INVALID, decided before anything is launched (a refused call writes nothing): a NULL ctx / in / outs, width 0, n_out outside
 * 1..4, an unknown format, interlace not 0 / 1 / 3, a missing plane, a missing matrix for a YCbCr format, a missing table, an odd width
 * or height for a format defined for even sizes only, two outputs naming the same first plane.  height == 0 is PH_OK. */
int ph_pack_write_multi(ph_ctx *ctx, int queue, const void *in, int n_out, const ph_chan_output *outs, uint32_t width,
                        uint32_t height);
/* The plain-layer composite - ph_fused_v210_combine's chain: n v210 layers of the output's size, read, combined, written - for up to
 * four CONSUMERS in one call: an encoder's yuv422p8 / yuv420p / nv12 / yuv422p10 frame or the screen's rgba8 / bgra8 beside, or instead
 * of, SDI's v210.  Exactly, bit for bit and in order, the n_out calls of ph_chan_compose on the same layers taken 1:1 (PH_SRC_V210,
 * matrix9_host == NULL, PH_TRANSITION_CUT) with each output's format, planes, interlace, matrix and table; a v210 frame output is
 * therefore ph_fused_v210_combine's frame.
 * Routes: n_out == 1, PH_FMT_V210, interlace == 0 IS ph_fused_v210_combine, same route.  Otherwise one launch of the headline kernel's
 * several-outputs form ("fused_v210_combine_multi x<outputs>" in a trace): its phase 1 is the headline kernel's; between the phases a quad
 * is its 18 writer-table indices in registers, and the writer's phase runs once per distinct writer table among the outputs - the 18
 * table reads made once, every output of that table packing the same 18 values with its own writer matrix.  No second composition
 * and no index frame in memory.  By default the whole frame is composed; a field output (interlace 1 / 3) stores the quads of its lines.
 * Context option "fused_fields" (default 0) = 1: where EVERY output is a field output of the same field (all interlace 1, or all 3 - a
 * 1080i channel's consumers; a lone v210 field, SDI's call, included) and the call qualifies for the shared launch, only that field is
 * composed: height / 2 lines from line 0 (interlace 1) or line 1 (interlace 3) are read, combined and looked up, in one launch
 * ("fused_v210_field_multi x<outputs>f<interlace>" in a trace) whose workgroups divide the FIELD's quads; height < 2 is PH_OK with nothing
 * launched.  The same bytes as with 0: the other parity's lines and, at an odd height, the last line are not touched; a 4:2:0 field
 * output's chroma row comes from the written line of the pair.  Outputs of mixed field modes, or any frame output among them, keep the
 * whole-frame launch and its name, with either value.
 * The shared launch needs width % 48 == 0, the reader's table and every writer's table registered, and the context option "lds_lut"
 * = 1; a call that does not qualify runs ph_chan_compose_multi on the equivalent layers inside the call, under that call's trace name,
 * so the entry takes everything ph_chan_compose_multi takes and answers its errors.
 * PH_E_INVALID, decided before anything is launched (a refused call writes nothing): NULL arguments, n outside 1..8, n_out outside
 * 1..4, an unknown format, a format the channel kernel does not write (yuv420p10, p010), interlace not 0 / 1 / 3, a missing plane,
 * matrix or table, an odd height for a 4:2:0 output, two outputs naming the same first plane.  height == 0 is PH_OK.
 * Context option "fused_multi_wgs" (default 0: no cap): the most workgroups the shared launch may have - a test and A/B hook that lets
 * a small frame reach several slices per lane and a second tile; the same bytes whatever its value. */
int ph_fused_v210_combine_multi(ph_ctx *ctx, int queue, int n, const void *const *layers, int n_out, const ph_chan_output *outs,
                                uint32_t width, uint32_t height, const void *rd_col_matrix12, const void *rd_gamma_lut,
                                const void *rd_gamut9);
/* Several CHANNELS' plain-layer composites, each for the same list of consumers, in one call: `jobs` = 1..8 frames of one geometry, layer
 * count and reader recipe.  layers: [jobs * n], job-major; outs: [jobs * n_out], job-major - outs[j * n_out + k] is outs[k] in everything
 * (format, interlace, writer matrix, writer table) but its planes.  Exactly, bit for bit and in order, the `jobs` calls of
 * ph_fused_v210_combine_multi.
 * Routes: jobs == 1 IS ph_fused_v210_combine_multi, same route.  Every job one v210 frame (n_out == 1, PH_FMT_V210, interlace == 0) IS
 * ph_fused_v210_combine_batch, same route.  Otherwise one launch ("fused_v210_combine_multi x<outputs>j<jobs>" in a trace): max(1, CUs /
 * jobs) workgroups per job - never more than a job's slices, "fused_multi_wgs" caps them per job - each owning an equal contiguous quad
 * range of its job; arithmetic and order within a job are ph_fused_v210_combine_multi's.  With the context option "fused_fields" = 1 and
 * every output a field output of the same field, the launch composes that field only, as ph_fused_v210_combine_multi says
 * ("fused_v210_field_multi x<outputs>j<jobs>f<interlace>"; the workgroups per job never more than the FIELD's slices); the same bytes.
 * A call the shared launch does not take
 * (width % 48 != 0, a table without its LDS form, "lds_lut" = 0, a frame too large for the kernel's division by reciprocal) runs
 * ph_fused_v210_combine_multi per job, in order, inside the call, under those calls' trace names.
 * PH_E_INVALID, decided before anything is launched (a refused call writes nothing): jobs outside 1..8; everything
 * ph_fused_v210_combine_multi refuses, per job and output; an output that differs from job 0's in anything but its planes; two outputs
 * of any jobs naming the same first plane.  height == 0 is PH_OK. */
int ph_fused_v210_combine_multi_batch(ph_ctx *ctx, int queue, int jobs, int n, const void *const *layers /* [jobs * n], job-major */,
                                      int n_out, const ph_chan_output *outs /* [jobs * n_out], job-major */, uint32_t width, uint32_t height,
                                      const void *rd_col_matrix12, const void *rd_gamma_lut, const void *rd_gamut9);
/* ph_fused_v210_combine_multi with layers in a TRANSITION (transitioner.ts:165-176: a MIX or WIPE between two clips): a layer may bring
 * the transition's second source - a v210 frame of the output's size - and, for a wipe, its mask of that size, a v210 frame or an f32
 * RGBA image.  Exactly, bit for bit and in order, the n_out calls of ph_chan_compose on these ph_chan_layers: src = the v210 frame taken
 * 1:1 (matrix9_host == NULL); transition, mix; incoming = the v210 frame taken 1:1; mask = a 1:1 source in its format - and therefore
 * ph_v210_read (of every frame) -> ph_transition_dissolve / ph_transition_wipe -> ph_combine -> ph_pack_write.  A v210 mask goes through the
 * reader (the call's Loader recipe) like any layer, and its .r is the factor.
 * Arithmetic: dissolve fma(src.c, mix, incoming.c * (1 - mix)), wipe fma(incoming.c, m, src.c * (1 - m)) on all four channels, each
 * difference and product rounded once; alpha is a value - a dissolve's is fma(1, mix, 1 * (1 - mix)), not always 1, a wipe's is per
 * pixel.  The bottom layer is taken as it is (a mask value of Inf or NaN does not reach it through a factor); above it k = 1 - v.a,
 * acc = fma(acc, k, v); n == 1 is the passthrough of the mixed image.
 * Routes: every layer PH_TRANSITION_CUT IS ph_fused_v210_combine_multi, same route and trace name.  Otherwise one launch
 * ("fused_v210_trans_multi x<outputs>" in a trace) of that call's kernel with the transitions inside its phase 1 - a v210 frame output
 * that is alone included.  The launch needs what ph_fused_v210_combine_multi's needs (width % 48 == 0, every table registered, "lds_lut"
 * = 1, a frame within the kernel's division by reciprocal); a call that does not qualify runs ph_chan_compose_multi on the equivalent
 * layers inside the call, under that call's trace name.  "fused_multi_wgs" caps the workgroups as it does there.
 * PH_E_INVALID, decided before anything is launched and before the context is looked at (a refused call writes nothing): everything
 * ph_fused_v210_combine_multi refuses (yuv420p10 / p010 outputs included); a transition outside 0..2; a dissolve or a wipe without
 * incoming_v210; a wipe without mask; a wipe whose mask_format is neither PH_SRC_V210 nor PH_SRC_RGBA_F32.  height == 0 is PH_OK. */
typedef struct ph_fused_layer {
  const void *v210;           /* device: the layer's frame, width x height */
  int transition;             /* PH_TRANSITION_CUT | _DISSOLVE | _WIPE */
  float mix;                  /* dissolve */
  const void *incoming_v210;  /* dissolve, wipe: the second source, a v210 frame of the same size */
  const void *mask;           /* wipe: the mask, of the same size, taken 1:1 */
  int mask_format;            /* PH_SRC_V210 (read with the call's Loader recipe, .r used) | PH_SRC_RGBA_F32 */
} ph_fused_layer;
int ph_fused_v210_transition_multi(ph_ctx *ctx, int queue, int n, const ph_fused_layer *layers, int n_out, const ph_chan_output *outs,
                                   uint32_t width, uint32_t height, const void *rd_col_matrix12, const void *rd_gamma_lut,
                                   const void *rd_gamut9);
/* ph_fused_v210_combine_multi for a ROUTED channel (routeProducer.ts:63-126, combiner.ts:219-254): a layer may be a finished f32 RGBA
 * image of the output's size - another channel's combined frame - and the combined image is an output, image_out, beside the n_out =
 * 0..4 packed frames.  Exactly, bit for bit and in order: ph_v210_read of every v210 layer; ph_combine of the n images in layer order
 * into image_out (n == 1: the Combiner's passthrough - image_out is that one image); ph_pack_write(image_out, ...) for each output with
 * its format, planes, interlace, matrix and table.  The packed outputs are therefore also ph_chan_compose_multi's on the same layers,
 * v210 and PH_SRC_RGBA_F32 sources both taken 1:1 (matrix9_host == NULL, PH_TRANSITION_CUT).
 * Arithmetic (ph_combine's): the bottom layer is taken as it is - its -0 and its alpha reach image_out unchanged; above it k = 1 - l.a,
 * rgb = fma(acc, k, l), a = fma(acc.a, 0, l.a).  Alpha is a value of its own: NaN above an image pixel whose alpha is Inf or NaN.  An
 * image layer's alpha is arbitrary, a v210 layer's is 1.  Only a NaN's payload is not pinned.
 * Routes: no image layer and image_out == NULL (n_out >= 1) IS ph_fused_v210_combine_multi, same route and trace name.  Otherwise one
 * launch ("fused_v210_route_multi x<n_out>i<0|1>" in a trace, i1: the image is written) of that call's kernel, the image layers loaded
 * and image_out stored inside its phase 1; with n_out == 0 no writer table is touched.  image_out is stored as ph_combine stores its
 * image (context option "stream_images").  The launch needs what ph_fused_v210_combine_multi's needs (width % 48 == 0, the reader's
 * table and every writer's table registered, "lds_lut" = 1, a frame within the kernel's division by reciprocal).  A call that does not
 * qualify and has image_out == NULL runs ph_chan_compose_multi on the equivalent layers inside the call, under that call's trace name
 * and with its errors; one that wants image_out is PH_E_INVALID - nothing else makes the image in one call: run ph_v210_read,
 * ph_combine and ph_pack_write_multi.  "fused_multi_wgs" caps the workgroups as it does for ph_fused_v210_combine_multi.
 * PH_E_INVALID, decided from the arguments before the context is looked at (a refused call writes nothing): everything
 * ph_fused_v210_combine_multi refuses about outputs and geometry (yuv420p10 / p010 outputs included); n outside 1..8; a layer with NULL
 * data; a layer format that is neither PH_SRC_V210 nor PH_SRC_RGBA_F32; n_out outside 0..4; n_out == 0 with image_out == NULL;
 * image_out equal to a layer's data (tail lanes read the range's last quad again, which another lane may just have written) or to an
 * output's first plane.  height == 0 is PH_OK and launches nothing. */
typedef struct ph_route_layer {
  const void *data;  /* device: a v210 frame, or an f32 RGBA image (16 B per pixel, rows unpadded), width x height */
  int format;        /* PH_SRC_V210 | PH_SRC_RGBA_F32 */
} ph_route_layer;
int ph_fused_v210_route_multi(ph_ctx *ctx, int queue, int n, const ph_route_layer *layers, void *image_out /* f32 RGBA, width x height, or NULL */,
                              int n_out /* 0..4 */, const ph_chan_output *outs, uint32_t width, uint32_t height, const void *rd_col_matrix12,
                              const void *rd_gamma_lut, const void *rd_gamut9);

/* ---- gamma LUT placement. The reference hands its kernels a 65536-entry f32 `gammaLut` buffer
 *      (loadSave.ts:65-73,152-160) and gathers from it 3x per pixel.  Registering the table's
 *      host contents lets the library keep an exact compressed copy for the CU's LDS
 *      (DESIGN.md "LUT placement"); kernels given a registered device pointer then use the LDS
 *      kernels, any other pointer uses the global-gather kernels.  Results are bit-identical.
 *      Buffers filled through ph_buf_host_access with 262144 bytes are registered automatically
 *      when first used as `gammaLut`.  Returns 1 if the table is LDS-capable, 0 if it is kept
 *      plain (not exactly compressible into 160 KiB), negative on error. ----------------------- */
int ph_lut_register(ph_ctx *ctx, const void *device_lut_f32, const float *host_lut65536);
int ph_lut_unregister(ph_ctx *ctx, const void *device_lut_f32);
/* lds_bytes = 0 when the pointer is unknown or plain; index_bias and blocks_per_octave_log2
 * describe the logarithmic block layout chosen for the table (ph_lut.h) */
int ph_lut_query(ph_ctx *ctx, const void *device_lut_f32, uint32_t *lds_bytes, uint32_t *index_bias,
                 uint32_t *blocks_per_octave_log2);
/* Device-free: compress a table exactly as ph_lut_register would and hand back the IMAGE of the LDS the table kernels
 * see - [0, hole) unused, then the anchors (u32 per logarithmic block), then the deltas (u16 per entry) - with the constants
 * of the lookup (phaneron_amd/csrc/ph_ldslut.h): for y = (float)idx + 1.5 * 2^23
 *     anchor byte address = (bits(fma(y, a_scale, -(1.5 * 2^23 - index_bias) * a_scale)) >> (shift - 2)) & ~3
 *     delta  byte address = delta_off + 2 * idx            (on the device: the bit pattern of a denormal fma)
 *     table[idx]          = the float whose bits are  u32 at the anchor address + u16 at the delta address.
 * `lds_image` may be NULL (layout only) or hold `capacity` >= lds_bytes bytes.  Returns the LDS footprint in bytes,
 * 0 when the table is not exactly compressible into 160 KiB (it stays plain: global-gather kernels), negative on error.
 * Replaces nothing in the reference: its kernels read the 256 KiB f32 table from global memory (v210.ts:68-70). */
typedef struct ph_lut_layout {
  uint32_t lds_bytes, hole, delta_off, shift, index_bias;
  float a_scale;
} ph_lut_layout;
int ph_lut_layout_of(const float *host_lut65536, ph_lut_layout *layout, void *lds_image, size_t capacity);
/* options: "lds_lut" (default 1): 0 forces the global-gather kernels (A/B tests, profiles);
 *          "stream_images" (default 0): 1 stores f32 image outputs (ToRGBA, Yadif, Transform, Combine ...) past the
 *          caches, for a caller that knows nothing on the device reads the image soon; 2 does so only for images
 *          larger than "stream_threshold_mb" MiB (default 64; measured neutral on the reference-shaped chains).  By
 *          default an image is treated as what it is in a channel, an intermediate the next operator reads back;
 *          wire-format outputs always stream.  The policy applies to f32 RGBA images: the packed-RGB (12 bytes per pixel)
 *          outputs of the de-interlacing reader (ph_yadif_pair_packed with PH_IMG_RGB_F32) are always stored plainly - the
 *          2 x 2-block compositor reads them back at once;
 *          "host_pool_mb" (default 4096): how much pinned host memory released buffers' mirrors may keep for the next
 *          buffer of the same size (the reference creates its destinations per job and frame: io.ts:64-72) - this much,
 *          or as much as was ever attached to live buffers at once if that is more (a pool smaller than the working set
 *          pins a block per buffer again, ~40 ms each); over the budget the oldest blocks are freed first; 0: no pool;
 *          setting the option trims the pool to the new size and restarts the working-set measurement (after a 2160p
 *          period a caller sheds the memory by setting the option again; node/index.js parks its frames under a budget
 *          of its own - parkMb - and trim() hands them back);
 *          "fail_launches" (default 0) - TEST ONLY, a fault injection for the error paths of a binding (node/test/soak_run.js): > 0:
 *          every launch made through ph_run_program / ph_run_programs fails with PH_E_HIP; -k: the next k launches (groups of
 *          ph_run_programs) go through, then every one fails; checks still pass.  Nothing in a deployment sets it;
 *          "chan_enlarged" (default 1; 0 when PH_CHAN_ENLARGED=0 is in the environment): ph_chan_compose* make a frame all of whose
 *          layers are ENLARGED v210 clips (a 720p or SD clip filling a 1080 channel: the reference uploads clips at their own size,
 *          ffmpegProducer.ts:395-442) by ph_v210_read into scratch images + ph_compose_up_write_v210 - one conversion per source pixel
 *          instead of four per output pixel, the same bits; 0: the channel kernel for those frames too;
 *          "chan_batch_outs" (default 0): 1 lets ph_run_programs put consecutive channel frames for other consumers than SDI
 *          (chan_compose_v210_<n> with outPacking, chan_compose_multi_<n>) of one geometry and Loader recipe into shared launches
 *          (ph_chan_compose_batch_out); 0: each such job a launch of its own, in its turn.  The same bits either way;
 *          "fused_multi_wgs" (default 0: no cap) - tests and A/B runs: the most workgroups a ph_fused_v210_combine_multi launch may have
 *          (a ph_fused_v210_combine_multi_batch launch: per job);
 *          "fused_multi_batch" (default 0): 1 lets ph_run_programs put consecutive fused_v210_combine_multi_<n> jobs of one geometry,
 *          layer count, Loader recipe and output list (formats, field modes, writer matrices and tables, in order) into shared launches,
 *          up to 8 jobs each (ph_fused_v210_combine_multi_batch); 0: each such job a launch of its own, in its turn.  The same bits
 *          either way.  Any other value is PH_E_INVALID;
 *          "fused_fields" (default 0): 1 lets ph_fused_v210_combine_multi and ph_fused_v210_combine_multi_batch - and what reaches them:
 *          ph_fused_v210_transition_multi with every layer a cut, ph_fused_v210_route_multi without an image layer or image_out, the
 *          programs fused_v210_combine_multi_<n> and their shared launches - compose only the field where every output takes the same one
 *          (all interlace 1 or all 3) and the call qualifies for the shared launch: half the lines read, combined and looked up
 *          ("fused_v210_field_multi ..." in a trace); 0: the whole frame, a field output storing the quads of its lines.  The same bytes
 *          either way.  Still whole-frame with 1: outputs of mixed field modes or with a frame among them, a layer in a transition, an
 *          image layer or image_out.  Any other value is PH_E_INVALID;
 *          "clip_batch" (default 0): 1 lets ph_run_programs put consecutive clip_compose_multi_<n> jobs of one geometry and Loader recipe
 *          into one ph_clip_compose_batch_out call, which shares launches among those of one clip shape and output list; 0: each such
 *          job a launch of its own, in its turn.  The same bits either way.  Any other value is PH_E_INVALID;
 *          "up_v210_tails" (default 0): 1 keeps a v210 output whose lines end in a tail quad (out_width % 48 != 0 - 1280 x 720, SDI's
 *          720p frame) inside its writer table's launch of the 2 x 2-block compositor's several-outputs kernels - ph_compose_up_write_multi,
 *          ph_clip_compose_multi, ph_clip_compose_batch_out, each of which says how, and by name compose_up_multi_<n>, clip_compose_multi_<n>
 *          and ph_run_programs with "clip_batch" - where the tail quad's lanes look the writer's table up a second time with truncated
 *          indices; 0: that output is made on its own, the composition a second time.  The same bits either way.  It leaves alone: the
 *          transition and route entries (ph_compose_up_transition_multi still refuses such an output beside a transition and, with every
 *          layer a cut, splits it off as with 0; ph_clip_compose_transition_multi and ph_clip_compose_route_multi split it off as
 *          ever), the ph_fused_v210_* family and the channel kernel.  Any other value is PH_E_INVALID. */
int ph_ctx_set_option(ph_ctx *ctx, const char *name, int value);
/* TESTS: the store policy a launch issued next on the calling thread for `ctx` would be given for an f32 RGBA image of `bytes` bytes -
 * 0 through the caches, 1 streamed - from "stream_images" and "stream_threshold_mb" (2: 1 for bytes > threshold << 20, strictly).
 * Selects the context's device as a launch does; negative on error (a NULL or destroyed context). */
int ph_debug_image_nt(ph_ctx *ctx, size_t bytes);
/* TESTS: where the field launches ("fused_fields") put field quad g of a width x height frame - the mapping their kernels use, run on the
 * host.  The field (interlace 1: the even lines, 3: the odd ones) is height / 2 lines of width / 6 quads, g counts them in raster order;
 * *f: the frame's flat quad (line * (width / 6) + col), *line: the frame line, *col: the quad's place in it (each may be NULL).
 * PH_E_INVALID: width % 48 != 0, interlace not 1 or 3, g outside the field, a frame beyond the kernels' division by reciprocal. */
int ph_debug_fused_field_quad(uint32_t width, uint32_t height, int interlace, uint32_t g, uint32_t *f, uint32_t *line, uint32_t *col);

/* ---- host colour maths (src/process/colourMaths.ts, run by Loader/Saver constructors
 *      loadSave.ts:50-63,139-149): outputs are HOST arrays the caller uploads. ------------------ */
int ph_colour_gamma2linear_lut(const char *colspec, float *lut65536);     /* :130-149 */
int ph_colour_linear2gamma_lut(const char *colspec, float *lut65536);     /* :151-169 */
int ph_colour_ycbcr2rgb_matrix(const char *colspec, int num_bits, int luma_black, int luma_white,
                               int chroma_range, float *m12);             /* :276-332 */
int ph_colour_rgb2ycbcr_matrix(const char *colspec, int num_bits, int luma_black, int luma_white,
                               int chroma_range, float *m12);             /* :334-390 */
int ph_colour_rgb2rgb_matrix(const char *src_colspec, const char *dst_colspec, float *m9); /* :392 */
/* transform.ts:119-171 */
int ph_transform_matrix(int width, int height, int flip_h, int flip_v, double anchor_x,
                        double anchor_y, double scale_x, double scale_y, double offset_x,
                        double offset_y, double rotate, float *m9);

int ph_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
