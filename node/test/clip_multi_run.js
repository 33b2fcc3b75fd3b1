'use strict'
// GPU check: file playback for several consumers through the addon BY NAME.  A yuv420p clip smaller than its channel goes to an
// encoder's nv12 frame and the screen's rgba8 with program clip_compose_multi_1 (ph_clip_compose_multi: the clip read once per source
// pixel, one launch); the bytes must be chan_compose_multi_1's on the same buffers (the channel kernel: four conversions per output
// pixel), and the traced route must start with clip_up_multi.  node/defer.js does not plan this route: the programs are run as posted.
// usage: node clip_multi_run.js [width=384] [height=54]; prints one JSON object { route, baseline, bytes, problems }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '54')
const SW = Math.floor(W / 3 / 2) * 2, SH = Math.floor(H * 2 / 3 / 2) * 2

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }

async function main() {
	const problems = []
	const rig = await Rig.open({ deviceIndex: 0, deferred: false })
	const ctx = rig.ctx
	const clip = await rig.planes('yuv420p', SW, SH)
	const r = lcg(20261020)
	for (const p of clip) {
		const b = Buffer.alloc(p.length)
		for (let i = 0; i < b.length; ++i) b[i] = (r() >>> 8) & 255
		await rig.upload(p, b)
	}
	const transform = await rig.transform(W, H)
	const fill = await transform.matrix({})
	const loader = await rig.colourIn('v210', '709', '709') // the call's Loader recipe; the 8-bit clip brings its own matrix
	const own = await rig.colourIn('yuv420p', '709', '709')
	const nv12 = await rig.colourOut('nv12', '709')
	const rgba8 = await rig.colourOut('rgba8', '709')
	const o0 = await rig.planes('nv12', W, H, 'readwrite')
	const o1 = await rig.planes('rgba8', W, H, 'readwrite')
	await rig.sync(ctx.queue.load)
	const params = {
		l0In: clip[0], l0InU: clip[1], l0InV: clip[2], l0Packing: 3 /* PH_FMT_YUV420P */, l0Width: SW, l0Height: SH, l0Matrix: fill, l0ColMatrix: own.colMatrix,
		colMatrix: loader.colMatrix, gammaLut: loader.gammaLut, gamutMatrix: loader.gamutMatrix,
		outPacking: 4 /* PH_FMT_NV12 */, output: o0[0], outputC: o0[1], outColMatrix: nv12.colMatrix, outGammaLut: nv12.gammaLut, interlace: 0,
		out1Packing: 5 /* PH_FMT_RGBA8 */, output1: o1[0], out1GammaLut: rgba8.gammaLut, interlace1: 0
	}
	const outs = [...o0, ...o1]
	const poison = async () => { for (const o of outs) await rig.upload(o, Buffer.alloc(o.length, 0x5a)) }
	const make = async (name) => {
		await poison()
		const program = await rig.program(name, 'chan', { globalWorkItems: [W, H] })
		ctx.traceBegin(false)
		let route
		try { await rig.run({ program, params }) } finally { route = ctx.traceEnd() }
		await rig.sync()
		const got = []
		for (const o of outs) { await rig.download(o); got.push(Buffer.from(o)) }
		return { route, got }
	}
	const mine = await make('clip_compose_multi_1')
	const theirs = await make('chan_compose_multi_1')
	if (!mine.route.startsWith('clip_up_multi')) problems.push({ what: 'the route of clip_compose_multi_1', got: mine.route })
	if (!theirs.route.startsWith('chan_compose_multi')) problems.push({ what: 'the route of chan_compose_multi_1', got: theirs.route })
	let bytes = 0
	mine.got.forEach((b, i) => {
		bytes += b.length
		if (!b.equals(theirs.got[i])) problems.push({ what: `plane ${i} differs from chan_compose_multi_1's` })
		if (b.every((x) => x === 0x5a)) problems.push({ what: `plane ${i} was not written` })
	})
	console.log(JSON.stringify({ route: mine.route, baseline: theirs.route, bytes, problems }))
	for (const b of [...clip, ...outs]) b.release()
	rig.close()
}
main().catch((e) => { process.stderr.write(String(e && e.stack || e) + '\n'); process.exit(1) })
