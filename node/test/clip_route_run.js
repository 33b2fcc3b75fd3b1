'use strict'
// GPU check: a ROUTED channel's file playback through the addon BY NAME.  A channel posts program clip_compose_route_1 - a yuv420p clip
// smaller than the channel, filling it - for an encoder's nv12 frame, the screen's rgba8 and imageOut, the combined f32 RGBA image another
// channel takes as a layer, for three ticks on a recording context (with and without clipBatch, which must not touch these jobs) and on
// a launch-as-posted context.  Every tick must be ONE launch ("clip_up_route<rgb>x2" in a trace: ph_clip_compose_route_multi), and the
// image and every consumer's frame must be the bytes of the posted chain on a launch-as-posted context: the format's `read`, `transform`,
// then a `write` per consumer (ph_pack_read -> ph_transform -> ph_pack_write).  The image alone (no `output` at all) is posted too.
// node/defer.js plans no route here: the programs are those named.
// usage: node clip_route_run.js [width=384] [height=54]; prints one JSON object { scenarios, problems }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '54')
const SW = Math.floor(W / 3 / 2) * 2, SH = Math.floor(H * 2 / 3 / 2) * 2
const TICKS = 3
const problems = []
const scenarios = []

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }

async function clipOf(rig, w, h, seed) {
	const clip = await rig.planes('yuv420p', w, h)
	const r = lcg(seed)
	for (const p of clip) {
		const b = Buffer.alloc(p.length)
		for (let i = 0; i < b.length; ++i) b[i] = (r() >>> 8) & 255
		await rig.upload(p, b)
	}
	return clip
}

async function poisoned(rig, buffers) {
	for (const o of buffers) await rig.upload(o, Buffer.alloc(o.length, 0x5a))
}

async function seenOf(rig, buffers, seen) {
	for (const p of buffers) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
}

// the posted chain, tick by tick: what the consumers and the next channel see - [nv12 Y, nv12 CbCr, rgba8, the image] per tick
async function chain() {
	const rig = await Rig.open({ deviceIndex: 0, spinWaitMicros: 100, deferred: false })
	const read = await rig.unpack('yuv420p', SW, SH, '709', '709')
	const transform = await rig.transform(W, H)
	const fill = await transform.matrix({})
	const nv12 = await rig.pack('nv12', W, H, '709')
	const rgba8 = await rig.pack('rgba8', W, H, '709')
	const seen = []
	for (let t = 0; t < TICKS; ++t) {
		const src = await clipOf(rig, SW, SH, 20261021 + t)
		const small = await rig.image(SW, SH)
		const image = await rig.image(W, H)
		const o0 = await rig.planes('nv12', W, H, 'readwrite')
		const o1 = await rig.planes('rgba8', W, H, 'readwrite')
		await poisoned(rig, [...o0, ...o1, image])
		await rig.sync(rig.ctx.queue.load)
		await rig.run(read(src, small))
		await rig.run(transform(small, image, fill))
		await rig.run(nv12(image, o0))
		await rig.run(rgba8(image, o1))
		await seenOf(rig, [...o0, ...o1, image], seen)
		;[...src, small, image, ...o0, ...o1].forEach((p) => p.release())
	}
	rig.close()
	return seen
}

// the ticks with program clip_compose_route_1; returns what was seen and the kernels of every tick
async function play(options, alone) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, spinWaitMicros: 100 }, options))
	const ctx = rig.ctx
	const transform = await rig.transform(W, H)
	const fill = await transform.matrix({})
	const loader = await rig.colourIn('v210', '709', '709') // the call's Loader recipe; the 8-bit clip brings its own matrix
	const own = await rig.colourIn('yuv420p', '709', '709')
	const nv12 = await rig.colourOut('nv12', '709')
	const rgba8 = await rig.colourOut('rgba8', '709')
	const name = 'clip_compose_route_1'
	const program = await rig.program(name, 'chan', { globalWorkItems: [W, H] })
	const seen = []
	const routes = []
	for (let t = 0; t < TICKS; ++t) {
		const src = await clipOf(rig, SW, SH, 20261021 + t)
		const image = await rig.image(W, H)
		const o0 = alone ? [] : await rig.planes('nv12', W, H, 'readwrite')
		const o1 = alone ? [] : await rig.planes('rgba8', W, H, 'readwrite')
		const outs = [...o0, ...o1, image]
		await poisoned(rig, outs)
		await rig.sync(ctx.queue.load)
		const params = {
			l0In: src[0], l0InU: src[1], l0InV: src[2], l0Packing: 3 /* PH_FMT_YUV420P */, l0Width: SW, l0Height: SH, l0Matrix: fill, l0ColMatrix: own.colMatrix,
			colMatrix: loader.colMatrix, gammaLut: loader.gammaLut, gamutMatrix: loader.gamutMatrix, imageOut: image
		}
		if (!alone)
			Object.assign(params, {
				outPacking: 4 /* PH_FMT_NV12 */, output: o0[0], outputC: o0[1], outColMatrix: nv12.colMatrix, outGammaLut: nv12.gammaLut, interlace: 0,
				out1Packing: 5 /* PH_FMT_RGBA8 */, output1: o1[0], out1GammaLut: rgba8.gammaLut, interlace1: 0
			})
		const id = { source: 'chan0', timestamp: t }
		rig.post(id, { name, program, params }, () => src.forEach((p) => p.release()))
		ctx.traceBegin(false)
		try {
			await rig.board.flush(id)
			await seenOf(rig, outs, seen)
		} finally { routes.push(ctx.traceEnd()) }
		outs.forEach((p) => p.release())
	}
	rig.close()
	return { seen, routes }
}

async function scenario(what, options, want, alone) {
	const route = alone ? 'clip_up_route<rgb>x0' : 'clip_up_route<rgb>x2'
	try {
		const r = await play(options, alone)
		scenarios.push({ name: what, routes: r.routes })
		for (const got of r.routes)
			if (got !== route) problems.push({ scenario: what, what: `a tick's launches: ${got}` })
		if (r.seen.length !== want.length) problems.push({ scenario: what, what: `buffers seen: ${r.seen.length}, ${want.length} expected` })
		for (let i = 0; i < Math.min(r.seen.length, want.length); ++i)
			if (Buffer.compare(r.seen[i], want[i]) !== 0) problems.push({ scenario: what, what: `buffer ${i} differs from the posted chain's` })
	} catch (e) {
		problems.push({ scenario: what, what: String(e && e.stack || e) })
	}
}

async function main() {
	const want = await chain()
	if (want.length !== TICKS * 4 || want.some((b) => b.every((x) => x === 0x5a))) problems.push({ what: 'the chain did not write every buffer' })
	await scenario('a recording context', { deferred: true }, want)
	await scenario('a recording context, clipBatch: true', { deferred: true, clipBatch: true }, want)
	await scenario('a plain context', { deferred: false }, want)
	await scenario('a plain context, the image alone', { deferred: false }, want.filter((b, i) => i % 4 === 3), true)
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
