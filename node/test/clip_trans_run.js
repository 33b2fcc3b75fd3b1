'use strict'
// GPU check: file playback through a MIX through the addon BY NAME.  A channel posts program clip_compose_trans_1 - a yuv420p clip
// dissolving into another yuv420p clip of another size, both smaller than the channel, to an encoder's nv12 frame and the screen's rgba8 -
// for three ticks of a transition (mix 0.75, 0.5, 0.25) on a recording context (with and without clipBatch, which must not touch these jobs)
// and on a launch-as-posted context.  Every tick must be ONE launch of the transition clip kernel ("clip_up_trans<rgb>x2" in a trace:
// ph_clip_compose_transition_multi), and every consumer must see the bytes the library's channel kernel makes of the same arguments
// (chan_compose_multi_1 on a launch-as-posted context).  node/defer.js plans no route here: the programs are those named.
// usage: node clip_trans_run.js [width=384] [height=54]; prints one JSON object { scenarios, problems }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '54')
const SW = Math.floor(W / 3 / 2) * 2, SH = Math.floor(H * 2 / 3 / 2) * 2
const IW = Math.floor(W / 4 / 2) * 2, IH = Math.floor(H / 3 / 2) * 2
const MIXES = [0.75, 0.5, 0.25]
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

// the ticks of the transition with program `name`; returns what the consumers saw and the kernels of every tick
async function play(name, options) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, spinWaitMicros: 100 }, options))
	const ctx = rig.ctx
	const transform = await rig.transform(W, H)
	const fill = await transform.matrix({})
	const inset = await transform.matrix({ scaleX: 0.9, scaleY: 0.9 })
	const loader = await rig.colourIn('v210', '709', '709') // the call's Loader recipe; the 8-bit clips bring their own matrix
	const own = await rig.colourIn('yuv420p', '709', '709')
	const nv12 = await rig.colourOut('nv12', '709')
	const rgba8 = await rig.colourOut('rgba8', '709')
	const program = await rig.program(name, 'chan', { globalWorkItems: [W, H] })
	const seen = []
	const routes = []
	for (let t = 0; t < MIXES.length; ++t) {
		const src = await clipOf(rig, SW, SH, 20261021 + 2 * t)
		const incoming = await clipOf(rig, IW, IH, 20261022 + 2 * t)
		const o0 = await rig.planes('nv12', W, H, 'readwrite')
		const o1 = await rig.planes('rgba8', W, H, 'readwrite')
		const outs = [...o0, ...o1]
		for (const o of outs) await rig.upload(o, Buffer.alloc(o.length, 0x5a))
		await rig.sync(ctx.queue.load)
		const params = {
			l0In: src[0], l0InU: src[1], l0InV: src[2], l0Packing: 3 /* PH_FMT_YUV420P */, l0Width: SW, l0Height: SH, l0Matrix: fill, l0ColMatrix: own.colMatrix,
			l0Transition: 1 /* PH_TRANSITION_DISSOLVE */, l0Mix: MIXES[t],
			l0IncomingIn: incoming[0], l0IncomingInU: incoming[1], l0IncomingInV: incoming[2], l0IncomingPacking: 3, l0IncomingWidth: IW, l0IncomingHeight: IH,
			l0IncomingMatrix: inset, l0IncomingColMatrix: own.colMatrix,
			colMatrix: loader.colMatrix, gammaLut: loader.gammaLut, gamutMatrix: loader.gamutMatrix,
			outPacking: 4 /* PH_FMT_NV12 */, output: o0[0], outputC: o0[1], outColMatrix: nv12.colMatrix, outGammaLut: nv12.gammaLut, interlace: 0,
			out1Packing: 5 /* PH_FMT_RGBA8 */, output1: o1[0], out1GammaLut: rgba8.gammaLut, interlace1: 0
		}
		const id = { source: 'chan0', timestamp: t }
		rig.post(id, { name, program, params }, () => [...src, ...incoming].forEach((p) => p.release()))
		ctx.traceBegin(false)
		try {
			await rig.board.flush(id)
			for (const p of outs) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		} finally { routes.push(ctx.traceEnd()) }
		outs.forEach((p) => p.release())
	}
	rig.close()
	return { seen, routes }
}

async function scenario(what, options) {
	try {
		const r = await play('clip_compose_trans_1', options)
		scenarios.push({ name: what, routes: r.routes })
		for (const route of r.routes)
			if (route !== 'clip_up_trans<rgb>x2') problems.push({ scenario: what, what: `a tick's launches: ${route}` })
		return r.seen
	} catch (e) {
		problems.push({ scenario: what, what: String(e && e.stack || e) })
		return []
	}
}

async function main() {
	const base = await play('chan_compose_multi_1', { deferred: false })
	const want = base.seen
	if (want.length !== MIXES.length * 3 || want.some((b) => b.every((x) => x === 0x5a))) problems.push({ what: 'the baseline did not write every plane' })
	if (!base.routes.every((r) => r.startsWith('chan_compose_multi<'))) problems.push({ what: `the baseline's launches: ${base.routes.join(' ')}` })
	const runs = [['a recording context', await scenario('a recording context', { deferred: true })],
		['a recording context, clipBatch: true', await scenario('a recording context, clipBatch: true', { deferred: true, clipBatch: true })],
		['a plain context', await scenario('a plain context', { deferred: false })]]
	for (const [what, got] of runs) {
		if (got.length !== want.length) problems.push({ scenario: what, what: `planes seen: ${got.length}, ${want.length} expected` })
		for (let i = 0; i < Math.min(got.length, want.length); ++i)
			if (Buffer.compare(got[i], want[i]) !== 0) problems.push({ scenario: what, what: `plane ${i} differs from the channel kernel's` })
	}
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
