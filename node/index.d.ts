// Types of the nodencl-shaped surface implemented by index.js (what phaneron imports from 'nodencl').
/// <reference types="node" />

export interface ImageDims {
	width: number
	height: number
}

export interface RunTimings {
	dataToKernel: number
	kernelExec: number
	totalTime: number
}

export type BufDir = 'readonly' | 'writeonly' | 'readwrite'
export type BufSVMType = 'none' | 'coarse' | 'fine'
export type HostAccessDir = 'readonly' | 'writeonly' | 'none'

export interface OpenCLBuffer extends Buffer {
	readonly numBytes: number
	readonly owner: string
	readonly imageDims?: ImageDims
	readonly creationTime: [number, number]
	timestamp: number
	loadstamp: number
	hostAccess(dir: HostAccessDir, queue?: number, src?: Buffer): Promise<void>
	addRef(): void
	release(): void
	refCount(): number
	/** staging extension: device -> mirror on `queue` (default unload) without a host wait */
	downloadAsync(queue?: number): void
}

/** staging extension: a recorded point in a queue */
export interface QueueEvent {
	wait(): Promise<void>
	done(): boolean
}

export interface RouteLink {
	readonly rank: number
	readonly world: number
	/** sends and receives of one frame period go inside one group */
	group(fn: () => void): void
	send(buf: OpenCLBuffer, peer: number): void
	recv(buf: OpenCLBuffer, peer: number): void
	/** the communication stream waits for everything enqueued so far on `queue` */
	afterQueue(queue?: number): void
	/** `queue` waits for everything enqueued so far on the communication stream */
	queueAfter(queue?: number): void
	wait(): void
}

export interface OpenCLProgram {
	readonly name: string
	readonly globalWorkItems: number[]
	readonly workItemsPerGroup: number
}

export interface KernelParams {
	[key: string]: unknown
}

export interface PlatformInfo {
	vendor: string
	name: string
	devices: Array<{ type: string; name: string; vendor: string }>
}

export interface DeferredStats {
	pending: number; recorded: number; launched: number; fused: number; fusedNodes: number; plain: number; dropped: number; fallbacks: number; lastFallback: string | null
	/** frames that went to the device together with other channels' frames, several to a launch */
	batched?: number
	/** consumers' writes that came out of another write's launch as further outputs (multiWriter, upWriters, imageWriters, fusedWriters) */
	multiOutputs?: number
}

export interface BufferStats {
	/** buffers somebody owns (parked ones are nobody's) */
	liveBuffers: number; liveBytes: number
	/** device bytes in the library's own pool */
	pooledBytes: number
	/** released frames / images kept whole for the next createBuffer of their shape */
	parkedBuffers: number; parkedBytes: number
	/** pinned host mirrors: attached to buffers, pooled, the most ever attached at once, hipHostMalloc calls so far */
	pinnedInUse: number; pinnedPooled: number; pinnedPeak: number; pins: number
}

export class clContext {
	/** `deferred` (default TRUE since round 4; `false`, or PHANERON_DEFERRED=0 in the environment, gives the launch-as-posted context):
	 * runProgram records instead of launching; a packed frame's recorded operator chain reaches the device as one fused kernel when its
	 * result is asked for (hostAccess 'readonly', downloadAsync, a route send, realise).  RunTimings of recorded jobs are zeros and
	 * waitFinish(queue.process) returns at once - INTEGRATION.md 3a.
	 * `profile` on a deferred context: a frame's terminal `write` is launched where it is posted and returns the fused launch's device time.
	 * `earlyLaunch` (default false; PHANERON_EARLY_LAUNCH=1): launch a frame at the end of the tick that posted its terminal `write`.
	 * `multiWriter` (default true; PHANERON_MULTI_WRITER=0): the pending `write` jobs of several consumers on ONE combined image (SDI plus an
	 * encoder or the screen) are made by one launch of the channel kernel - one composition, a writer's phase per consumer; `false`: a launch per write.
	 * `upWriters` (default true for both classes of frame, as measured: DESIGN.md 5.1; PHANERON_UP_WRITERS=0): frames made from de-interlaced fields or
	 * enlarged images for a consumer that is not SDI, and the writes of several consumers on one such image, are one launch of the 2 x 2-block
	 * compositor from the packed fields (`compose_up_multi_<n>`); `false`: the fields unpacked and the channel kernel, a launch per consumer.
	 * `upTransitions` (default false; PHANERON_UP_TRANSITIONS=1): a frame of such images with a layer in a dissolve or a wipe - the layer, the incoming
	 * image and a wipe's mask all enlarged (or fields at their own size), none of them a wire-format frame, an even width (a v210 frame: a multiple of
	 * 48) - is one launch of the same compositor (`compose_up_trans_<n>`, ph_compose_up_transition_multi) ahead of the channel kernel, from the packed
	 * fields when every image of the frame is one; `false`: the recorded stream reaches the device exactly as without the option.  The same bytes either
	 * way.  Measured through the library (DESIGN.md 5.1), not through node.
	 * `fusedTransitions` (default false; PHANERON_FUSED_TRANSITIONS=1): a frame of plain v210 layers of the output's size with a layer in a dissolve
	 * or a wipe - the layer, its incoming frame and a wipe's mask plain v210 reads under one Loader recipe (the mask may be an f32 image of the
	 * frame's size), no transform or yadif in the chain - is one launch of the headline kernel's several-outputs form (`fused_v210_trans_<n>`,
	 * ph_fused_v210_transition_multi) ahead of the channel kernel, the other consumers' writes of the image folded in; `false`: the recorded
	 * stream reaches the device exactly as without the option.  The same bytes either way.  Measured through the library (DESIGN.md 5.1), not
	 * through node.
	 * `batchOuts` (default false; PHANERON_BATCH_OUTS=1): the frames several channels post in one tick for consumers other than SDI (an encoder's
	 * yuv422p8, the screen's rgba8) and for several consumers at once share ONE launch of the channel kernel (the library's context option
	 * `chan_batch_outs`, ph_chan_compose_batch_out); `false`: a launch per channel, in its turn.  The same bytes either way.
	 * `clipBatch` (default false; PHANERON_CLIP_BATCH=1): the `clip_compose_multi_<n>` jobs (file playback, posted by name) that several channels
	 * post in one tick go down in ONE runPrograms call with the library's context option `clip_batch` set, where jobs of one clip shape and list
	 * of consumers share ONE launch (ph_clip_compose_batch_out, `clip_up_multi<rgb|rgba>x<outputs>j<jobs>` in a trace; counted under
	 * `deferredStats().batched`); `false`: a launch per job, in its turn.  The same bytes either way.  No route is planned for it: the programs
	 * are those the caller names.
	 * `upTails` (default false; PHANERON_UP_TAILS=1): on a channel whose v210 lines end in a tail quad (width % 48 != 0 - 1280 x 720) SDI's v210
	 * frame stays inside the launch that makes the other consumers' frames (`compose_up_multi_<n>`, `clip_compose_multi_<n>`:
	 * `compose_up_multi_t<..>` / `clip_up_multi_t<..>` in a trace) instead of a launch of its own - the library's context option
	 * `up_v210_tails`, set once in front of the context's first launch.  The same bytes either way; nothing is planned differently.
	 * `imageWriters` (default false; PHANERON_IMAGE_WRITERS=1): wire-format `write` jobs that are launched as posted (no fused plan, or every fused
	 * candidate refused) take the pending writes of the other consumers of the same image - any of the nine formats, yuv420p10 / p010 included -
	 * with them as ONE `pack_write_multi_<n>` launch (ph_pack_write_multi: the image read and looked up once); `false`: a launch per write.
	 * The same bytes either way.  Measured: three consumers 27 % faster, v210 + rgba8 alone 4 % slower from HBM (DESIGN.md 5.1).
	 * `fusedWriters` (default false; PHANERON_FUSED_WRITERS=1): a frame whose chain is the headline's - plain `read`s of the output's size, `combine_<n>`,
	 * `write` - whose terminal write is not a v210 frame (an encoder's, the screen's, a field), or which has sibling writes on the combined image,
	 * is ONE `fused_v210_combine_multi_<n>` launch (ph_fused_v210_combine_multi: up to four outputs) instead of the channel kernel's; `false`: the
	 * recorded stream reaches the device exactly as without the option.  The same bytes either way.
	 * `fusedBatch` (default false; PHANERON_FUSED_BATCH=1; only with `fusedWriters`): the `fused_v210_combine_multi_<n>` frames several channels post in one
	 * tick - one size, layer count, Loader recipe and list of consumers - go down in ONE runPrograms call and share ONE launch (the library's context option
	 * `fused_multi_batch`, ph_fused_v210_combine_multi_batch; counted under `deferredStats().batched`); a refused batch falls back frame by frame; `false`: a
	 * launch per channel, in its turn.  The same bytes either way.  Measured through the library, not through node (DESIGN.md 5.1), per call: four 1080p
	 * channels' yuv422p8 frames 75.5 -> 53.7 us, SDI + the screen 89.7 -> 69.4, eight nv12 channels 149.7 -> 102.5, two channels with three consumers
	 * 47.5 -> 40.7; two 2160p channels 106.4 -> 103.6 - a win, and the smallest.  No shape lost.
	 * `fusedFields` (default false; PHANERON_FUSED_FIELDS=1): where every consumer of a `fused_v210_combine_multi_<n>` frame takes the same field
	 * (a 1080i channel: `interlace` 1 or 3 on every output) only that field's lines are composed - half the reads, combines and table look-ups
	 * (`fused_v210_field_multi ...` in a trace) - the library's context option `fused_fields`, set once in front of the context's first launch.
	 * The same bytes either way; nothing is planned differently.  Frames with a layer in a transition, routed frames and consumers of mixed field
	 * modes are composed whole as before.
	 * `recycleBuffers` (default true; PHANERON_RECYCLE=0): released frames / images are parked for the next createBuffer of their shape,
	 * up to `parkMb` MiB (default 4096) or the most that was ever in use at once.  A parked buffer is taken over as the same JS object;
	 * `strictHandles` (default false; PHANERON_STRICT_HANDLES=1): a fresh object per takeover, so that a reference kept past release()
	 * is refused ('... released buffer') instead of aliasing the next owner's buffer - for running an application under test. */
	constructor(params?: { platformIndex?: number; deviceIndex?: number; overlapping?: boolean; profile?: boolean; spinWaitMicros?: number; deferred?: boolean;
		earlyLaunch?: boolean; multiWriter?: boolean; upWriters?: boolean; upTransitions?: boolean; fusedTransitions?: boolean; batchOuts?: boolean; clipBatch?: boolean; upTails?: boolean; imageWriters?: boolean; fusedWriters?: boolean; fusedBatch?: boolean; fusedFields?: boolean; recycleBuffers?: boolean; parkMb?: number; strictHandles?: boolean })
	readonly queue: { load: number; process: number; unload: number }
	initialise(): Promise<void>
	getPlatformInfo(): PlatformInfo
	createBuffer(numBytes: number, bufDir: BufDir, bufType: BufSVMType, imageDims?: ImageDims, owner?: string): Promise<OpenCLBuffer>
	/** extension: `name` may be `clip_compose_multi_<n>` (n = layers): `chan_compose_multi_<n>`'s arguments, name for name, through
	 * ph_clip_compose_multi - file playback (an enlarged clip, a decoder's frame under the default fill) for up to four consumers with the clip
	 * read once per source pixel; same bytes as `chan_compose_multi_<n>`.  Reached by name only: the recording context (defer.js) does not plan it
	 * (`clipBatch` lets the jobs of a tick share launches).
	 * `name` may also be `clip_compose_trans_<n>`: the same arguments with the transition's (`l<i>Transition` 1 dissolve / 2 wipe, `l<i>Mix`,
	 * `l<i>Incoming...`, `l<i>Mask...`) through ph_clip_compose_transition_multi - file playback through a MIX or WIPE, every clip of the
	 * transition read once per source pixel; same bytes as `chan_compose_multi_<n>`.  Reached by name only: defer.js does not plan it and
	 * `clipBatch` does not group it - every job is a launch of its own in its turn.
	 * `name` may also be `clip_compose_route_<n>`: `clip_compose_multi_<n>`'s arguments and the optional image buffer `imageOut` through
	 * ph_clip_compose_route_multi - a routed channel's file playback: the consumers' frames (same bytes as `clip_compose_multi_<n>`) and the combined f32
	 * RGBA image another channel takes as a layer, from the same read-once launch; `output` may be absent only where `imageOut` is there (the image
	 * alone).  A frame the read-once routes do not take is REFUSED (post `read`, `transform`, `combine_<n>` and the writers instead).  Reached by name only:
	 * defer.js does not plan it and `clipBatch` does not group it - every job is a launch of its own in its turn. */
	createProgram(kernel: string, options: { name: string; globalWorkItems?: number | Uint32Array | number[]; workItemsPerGroup?: number }): Promise<OpenCLProgram>
	runProgram(program: OpenCLProgram, params: KernelParams, queue?: number): Promise<RunTimings>
	/** Recording contexts only: runProgram without the promise (node/jobs.js uses it per job of a batch).  null = not a recording
	 *  context, or a `profile` one - call runProgram; throws what runProgram would reject with. */
	recordProgram(program: OpenCLProgram, params: KernelParams, queue?: number): RunTimings | null
	waitFinish(queue?: number): Promise<void>
	/** deferred contexts: make these buffers' contents real now, as a consumer on the device would need them */
	realise(...bufs: OpenCLBuffer[]): void
	/** deferred contexts: run everything still recorded; returns the recording's counters (null on a plain context) */
	flushDeferred(): DeferredStats | null
	deferredStats(): DeferredStats | null
	/** extension: note the kernels the calls made from here on (this thread) launch; dryRun: choose and check, enqueue nothing */
	traceBegin(dryRun?: boolean): void
	/** extension: the kernels launched since traceBegin, '+'-joined, e.g. "v210_yadif_pair+compose_up_write_v210" */
	traceEnd(): string
	/** wait until everything launched so far on `queue` has finished (on a deferred context waitFinish(queue.process) returns at once) */
	drain(queue?: number): Promise<void>
	/** staging extension: later work on `waiter` starts after everything enqueued so far on `signal` */
	queueWaitQueue(waiter: number, signal: number): void
	/** staging extension: a point in `queue`; wait() polls on the JS thread for up to `spinWaitMicros` before handing the wait to the libuv pool */
	recordEvent(queue?: number): QueueEvent
	/** ROUTE across GPUs: RCCL send / recv on a communication stream of its own, ordered on the device */
	openRoute(id: Buffer, rank: number, world: number): RouteLink
	static routeUniqueId(): Buffer
	/** library options: 'lds_lut' (0 | 1), 'stream_images' (0 cached | 1 streamed | 2 by size), 'stream_threshold_mb', 'host_pool_mb' (pinned mirrors kept for reuse) */
	setOption(name: string, value: number): void
	/** library options also: 'fail_launches' (tests: every launch fails while set) */
	logBuffers(): BufferStats
	bufferStats(): BufferStats
	/** hand the parked buffers back to the library */
	trim(): void
}

/** which precompiled kernel createProgram(kernelSrc, {name}) selects - needs no context and no GPU */
export function resolveProgram(kernelSrc: string, name: string): { kernel: string; format: string | null; how: 'tag' | 'name' | 'text' | 'signature' }

/** the library's host colour maths (the numbers src/process/colourMaths.ts and transform.ts:119-171 produce) */
export const colour: {
	gamma2linearLUT(colSpec: string): Float32Array
	linear2gammaLUT(colSpec: string): Float32Array
	ycbcr2rgbMatrix(colSpec: string, numBits?: number, lumaBlack?: number, lumaWhite?: number, chromaRange?: number): Float32Array
	rgb2ycbcrMatrix(colSpec: string, numBits?: number, lumaBlack?: number, lumaWhite?: number, chromaRange?: number): Float32Array
	rgb2rgbMatrix(srcColSpec: string, dstColSpec: string): Float32Array
	transformMatrix(width: number, height: number, params?: { flipH?: boolean; flipV?: boolean; anchorX?: number; anchorY?: number; scaleX?: number; scaleY?: number; offsetX?: number; offsetY?: number; rotate?: number }): Float32Array
}
/** the pack formats, indexed as PH_FMT_*: 'v210', 'yuv422p10', 'yuv422p8', 'yuv420p', 'nv12', 'rgba8', 'bgra8', 'yuv420p10', 'p010'
 * (the last two: 10-bit 4:2:0 decoder frames, yuv420p10le and p010le; their programs resolve by the tags 'phaneron:yuv420p10' / 'phaneron:p010') */
export const FORMATS: string[]
/** bytes per plane of a frame in `format` (yuv420p10: [2Ph, Ph/2, Ph/2]; p010: [2Ph, Ph] with P the width rounded up to 8) */
export function planeBytes(format: string, width: number, height: number): number[]
