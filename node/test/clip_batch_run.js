'use strict'
// GPU check: four channels' file playback of a tick through the addon BY NAME.  Every channel posts program clip_compose_multi_1 - its own
// yuv420p clip, smaller than the channel, to an encoder's nv12 frame and the screen's rgba8 - for three ticks on a recording context.
// With `clipBatch: true` the four jobs of a tick go down in one runPrograms call and come out of ONE launch ("clip_up_multi<rgb>x2j4" in
// a trace: ph_clip_compose_batch_out); with the option off every job is a launch of its own, in its turn.  Both ways every consumer must
// see the bytes chan_compose_multi_1 makes on a launch-as-posted context.  node/defer.js plans no route here: the programs are those named.
// usage: node clip_batch_run.js [width=384] [height=54]; prints one JSON object { scenarios, problems }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '54')
const SW = Math.floor(W / 3 / 2) * 2, SH = Math.floor(H * 2 / 3 / 2) * 2
const TICKS = 3
const CHANNELS = 4
const problems = []
const scenarios = []

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }

// TICKS ticks of the four channels with program `name`; returns what the consumers saw, the kernels of every tick and the counters
async function play(name, options) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, spinWaitMicros: 100 }, options))
	const ctx = rig.ctx
	const transform = await rig.transform(W, H)
	const fill = await transform.matrix({})
	const loader = await rig.colourIn('v210', '709', '709') // the call's Loader recipe; the 8-bit clips bring their own matrix
	const own = await rig.colourIn('yuv420p', '709', '709')
	const nv12 = await rig.colourOut('nv12', '709')
	const rgba8 = await rig.colourOut('rgba8', '709')
	const program = await rig.program(name, 'chan', { globalWorkItems: [W, H] })
	const seen = []
	const routes = []
	for (let t = 0; t < TICKS; ++t) {
		const outs = []
		const ids = []
		for (let c = 0; c < CHANNELS; ++c) {
			const clip = await rig.planes('yuv420p', SW, SH)
			const r = lcg(20261021 + 16 * t + c)
			for (const p of clip) {
				const b = Buffer.alloc(p.length)
				for (let i = 0; i < b.length; ++i) b[i] = (r() >>> 8) & 255
				await rig.upload(p, b)
			}
			const o0 = await rig.planes('nv12', W, H, 'readwrite')
			const o1 = await rig.planes('rgba8', W, H, 'readwrite')
			for (const o of [...o0, ...o1]) await rig.upload(o, Buffer.alloc(o.length, 0x5a))
			await rig.sync(ctx.queue.load)
			const params = {
				l0In: clip[0], l0InU: clip[1], l0InV: clip[2], l0Packing: 3 /* PH_FMT_YUV420P */, l0Width: SW, l0Height: SH, l0Matrix: fill, l0ColMatrix: own.colMatrix,
				colMatrix: loader.colMatrix, gammaLut: loader.gammaLut, gamutMatrix: loader.gamutMatrix,
				outPacking: 4 /* PH_FMT_NV12 */, output: o0[0], outputC: o0[1], outColMatrix: nv12.colMatrix, outGammaLut: nv12.gammaLut, interlace: 0,
				out1Packing: 5 /* PH_FMT_RGBA8 */, output1: o1[0], out1GammaLut: rgba8.gammaLut, interlace1: 0
			}
			const id = { source: `chan${c}`, timestamp: t }
			rig.post(id, { name, program, params }, () => clip.forEach((p) => p.release()))
			ids.push(id)
			outs.push([...o0, ...o1])
		}
		ctx.traceBegin(false)
		try {
			await Promise.all(ids.map((id) => rig.board.flush(id)))
			for (const planes of outs) for (const p of planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		} finally { routes.push(ctx.traceEnd()) }
		for (const planes of outs) planes.forEach((p) => p.release())
	}
	const st = ctx.deferredStats ? ctx.deferredStats() : null
	rig.close()
	return { seen, routes, st }
}

async function scenario(what, options, check) {
	try {
		const r = await play('clip_compose_multi_1', Object.assign({ deferred: true }, options))
		scenarios.push({ name: what, routes: r.routes, deferred: r.st })
		for (const route of r.routes) {
			const kernels = route.split('+').filter((k) => k)
			if (!check(kernels)) problems.push({ scenario: what, what: `a tick's launches: ${route}` })
		}
		return r.seen
	} catch (e) {
		problems.push({ scenario: what, what: String(e && e.stack || e) })
		return []
	}
}

async function main() {
	const want = (await play('chan_compose_multi_1', { deferred: false })).seen
	if (want.length !== TICKS * CHANNELS * 3 || want.some((b) => b.every((x) => x === 0x5a))) problems.push({ what: 'the baseline did not write every plane' })
	const on = await scenario('clipBatch: true', { clipBatch: true }, (k) => k.length === 1 && k[0] === 'clip_up_multi<rgb>x2j4')
	const off = await scenario('clipBatch off (the default)', {}, (k) => k.length === CHANNELS && k.every((x) => x === 'clip_up_multi<rgb>x2'))
	for (const [what, got] of [['clipBatch: true', on], ['clipBatch off', off]]) {
		if (got.length !== want.length) problems.push({ scenario: what, what: `planes seen: ${got.length}, ${want.length} expected` })
		for (let i = 0; i < Math.min(got.length, want.length); ++i)
			if (Buffer.compare(got[i], want[i]) !== 0) problems.push({ scenario: what, what: `plane ${i} differs from chan_compose_multi_1's` })
	}
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
