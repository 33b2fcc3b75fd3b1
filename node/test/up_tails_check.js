'use strict'
// node/defer.js without a device: the context option `upTails` (the stand-in for the addon only counts, as in up_out_defer_check.js).  A
// 1280-wide channel - every v210 line ends in a tail quad - posts SDI's v210 write and the screen's bgra8 write of both de-interlaced fields
// of a tick.  With `upTails: true` the library's "up_v210_tails" is set ONCE, in front of the first launch; the recorded stream folds into
// one compose_up_multi_<n> job whose outputs include the v210 write, with the option or without (no planning changes); without `upTails`
// the option is never set.  Prints one JSON object { checks, problems }.
const { Deferral } = require('../defer.js')
const { bufferPrototype, newPark } = require('../index.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function rig(opt = {}) {
	const events = [] // ['option', name, value] | ['launch', program name, parameter names]
	let nextId = 1
	const refs = new Map()
	const native = {
		bufAddRef: (h) => refs.set(h, refs.get(h) + 1),
		bufRelease: (h) => refs.set(h, refs.get(h) - 1),
		bufRefCount: (h) => refs.get(h) || 0,
		createProgram: (_ctx, _src, name) => ({ name }),
		setOption: (_ctx, name, value) => events.push(['option', name, value]),
		runProgram: (_ctx, prog, names, values, queue, _timed, checkOnly) => {
			if (checkOnly) return null
			events.push(['launch', prog.name, names.slice().sort()])
			return { dataToKernel: 0, kernelExec: 0, totalTime: 0 }
		},
		queueWaitQueue: () => {}
	}
	const ctx = { _native: native, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, upWriters: true, upTails: opt.upTails }
	const d = new Deferral(ctx)
	const proto = bufferPrototype(native, d, newPark(false, 0))
	const buffer = (bytes, dims, owner) => {
		const b = Buffer.alloc(bytes)
		const h = { id: nextId++ }
		refs.set(h, 1)
		Object.setPrototypeOf(b, proto)
		Object.defineProperty(b, '_handle', { value: h })
		b._refs = 1
		b._dead = false
		b.imageDims = dims
		b.owner = owner || ''
		Deferral.adopt(b, true)
		return b
	}
	const W = 1280 // 1280 % 48 = 32: a tail quad of two pixels, two cleared slots up to the 1296-pixel pitch
	const H = 4
	const SW = 636, SH = 2 // the interlaced source: a v210 frame of whole quads, enlarged about 2 x onto the channel
	const program = (name, extra, dims = [W, H]) => Object.assign({ name, globalWorkItems: dims, workItemsPerGroup: 0, _handle: { name } }, extra || {})
	const writer = (format, lines) => program('write', { format, globalWorkItems: [2 * lines], workItemsPerGroup: 2 })
	const P = { read: program('read', { format: 'v210', globalWorkItems: [2 * SH], workItemsPerGroup: 2 }), transform: program('transform'), yadif: program('yadif', {}, [SW, SH]),
		v210: writer('v210', H), bgra8: writer('bgra8', H) }
	const param = (tag, bytes, fill) => { const b = buffer(bytes, undefined, tag); b.fill(fill); return b }
	const L = { colMatrix: param('cm', 48, 1), gammaLut: param('lut', 64, 2), gamutMatrix: param('gm', 36, 3) }
	const saver = { colMatrix: param('wcm', 48, 7), gammaLut: param('wlut', 64, 8) }
	const image = (owner, w = W, h = H) => buffer(w * h * 16, { width: w, height: h }, owner)
	const plane = (owner, pitch = 3456, h = H) => buffer(pitch * h, undefined, owner) // (a v210 line of 1280 pixels: 3456 bytes)
	const matrix = buffer(48, undefined, 'matrix')
	matrix.fill(0)
	new Float32Array(matrix.buffer, matrix.byteOffset, 9).set([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1]) // enlarged 2 x: the 2 x 2-block compositor's
	const fields = () => {
		const win = [0, 1, 2].map((i) => { const im = image(`w${i}`, SW, SH); d.record(P.read, Object.assign({ input: plane(`s${i}`, 1792, SH), output: im, width: SW }, L), 1); return im })
		return [0, 1].map((parity) => {
			const y = image(`y${parity}`, SW, SH), t = image(`t${parity}`)
			d.record(P.yadif, { prev: win[0], cur: win[1], next: win[2], parity, tff: 1, skipSpatial: 0, output: y }, 1)
			d.record(P.transform, { input: y, transformMatrix: matrix, output: t }, 1)
			return { field: y, placed: t }
		})
	}
	const write = (prog, img, outs) => d.record(prog, Object.assign({ input: img, width: W, interlace: 0 }, outs, saver), 1)
	// a tick: SDI + the screen on both fields; every frame is asked for
	const tick = () => {
		const f = fields()
		const sdi = [plane('sdi0'), plane('sdi1')], screen = [plane('scr0', W * 4), plane('scr1', W * 4)]
		f.forEach((x, i) => { write(P.v210, x.placed, { output: sdi[i] }); write(P.bgra8, x.placed, { output: screen[i] }) })
		for (const b of [...sdi, ...screen]) d.touch(b, 'readonly', 2)
	}
	return { d, events, tick, launches: () => events.filter((e) => e[0] === 'launch'), options: () => events.filter((e) => e[0] === 'option') }
}

for (const upTails of [true, false, undefined]) {
	const tag = `upTails ${upTails}`
	const r = rig({ upTails })
	expect(`${tag}: nothing is set before something is launched`, r.events.length, 0)
	r.tick()
	expect(`${tag}: SDI + screen of both fields fold into one compositor job`, r.launches().map((l) => l[1]), ['v210_yadif_pair_1', 'compose_up_multi_1'])
	const names = r.launches()[1][2]
	// (output: the v210 write - its packing is the default, it brings the writer's matrix; output1: the screen's bgra8)
	for (const n of ['packedRgb', 'l0In', 'l0In2', 'output', 'outColMatrix', 'outGammaLut', 'interlace', 'output1', 'out1Packing', 'twinOutput', 'twinOutput1'])
		expect(`${tag}: the launch names '${n}'`, names.includes(n), true)
	expect(`${tag}: the v210 write is output 0 (no packing named: v210), and no write is left`, [names.includes('outPacking'), [...r.d.pending].some((n) => n.program.name === 'write'), r.d.stats.fallbacks],
		[false, false, 0])
	r.tick()
	r.tick()
	expect(`${tag}: three ticks, two launches each`, r.launches().length, 6)
	if (upTails === true) {
		expect(`${tag}: the option is set once`, r.options(), [['option', 'up_v210_tails', 1]])
		expect(`${tag}: ... in front of the first launch`, [r.events[0][0], r.events[1][0]], ['option', 'launch'])
	} else {
		expect(`${tag}: the option is never set`, r.options(), [])
	}
}

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
