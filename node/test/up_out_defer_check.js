'use strict'
// node/defer.js without a device: frames of the 2 x 2-block compositor (de-interlaced fields, enlarged) for consumers other than SDI and
// for several consumers at once (the stand-in for the addon only counts, as in multi_defer_check.js).  What goes to the device, what the
// launch's parameters are called, and what happens when the option is off, a sibling comes late, the launch is refused, or a field was
// unpacked between plan and commit.  Prints one JSON object { checks, problems }.
const { Deferral } = require('../defer.js')
const { bufferPrototype, newPark } = require('../index.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function rig(opt = {}) {
	const launches = [] // [program name, parameter names]
	let nextId = 1
	const refs = new Map()
	const native = {
		bufAddRef: (h) => refs.set(h, refs.get(h) + 1),
		bufRelease: (h) => refs.set(h, refs.get(h) - 1),
		bufRefCount: (h) => refs.get(h) || 0,
		createProgram: (_ctx, _src, name) => ({ name }),
		runProgram: (_ctx, prog, names, values, queue, _timed, checkOnly) => {
			if (checkOnly) return null
			if (opt.refuse && opt.refuse(prog.name)) throw new Error(`${prog.name}: refused`)
			launches.push([prog.name, names.slice().sort()])
			return { dataToKernel: 0, kernelExec: 0, totalTime: 0 }
		},
		queueWaitQueue: () => {}
	}
	const ctx = { _native: native, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, upWriters: opt.upWriters === undefined ? true : opt.upWriters } // (the option on unless a scenario says otherwise: its default follows the measurement)
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
	const W = 96
	const H = 4
	const program = (name, extra) => Object.assign({ name, globalWorkItems: [W, H], workItemsPerGroup: 0, _handle: { name } }, extra || {})
	const writer = (format, lines) => program('write', { format, globalWorkItems: [2 * lines], workItemsPerGroup: 2 })
	const P = { read: program('read', { format: 'v210', globalWorkItems: [2 * H], workItemsPerGroup: 2 }), transform: program('transform'), yadif: program('yadif'),
		v210: writer('v210', H), bgra8: writer('bgra8', H), yuv422p8: writer('yuv422p8', H) }
	const param = (tag, bytes, fill) => { const b = buffer(bytes, undefined, tag); b.fill(fill); return b }
	const L = { colMatrix: param('cm', 48, 1), gammaLut: param('lut', 64, 2), gamutMatrix: param('gm', 36, 3) }
	const saver = { colMatrix: param('wcm', 48, 7), gammaLut: param('wlut', 64, 8) }
	const image = (owner) => buffer(W * H * 16, { width: W, height: H }, owner)
	const plane = (owner) => buffer(256 * H, undefined, owner)
	const matrix = buffer(48, undefined, 'matrix')
	matrix.fill(0)
	new Float32Array(matrix.buffer, matrix.byteOffset, 9).set([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1]) // enlarged 2 x: the 2 x 2-block compositor's
	// a tick of a 1080i-source channel: a window, both de-interlaced fields, each placed: the two images the consumers write
	const fields = () => {
		const win = [0, 1, 2].map((i) => { const im = image(`w${i}`); d.record(P.read, Object.assign({ input: plane(`s${i}`), output: im, width: W }, L), 1); return im })
		return [0, 1].map((parity) => {
			const y = image(`y${parity}`), t = image(`t${parity}`)
			d.record(P.yadif, { prev: win[0], cur: win[1], next: win[2], parity, tff: 1, skipSpatial: 0, output: y }, 1)
			d.record(P.transform, { input: y, transformMatrix: matrix, output: t }, 1)
			return { field: y, placed: t }
		})
	}
	const write = (prog, img, outs) => d.record(prog, Object.assign({ input: img, width: W, interlace: 0 }, outs, saver), 1)
	return { d, launches, P, plane, fields, write, names: () => launches.map((l) => l[0]) }
}
const planar = (r, tag) => ({ outputY: r.plane(`${tag}y`), outputU: r.plane(`${tag}u`), outputV: r.plane(`${tag}v`) })

// 1. an encoder alone on de-interlaced fields: the fields stay packed, one launch of the compositor's several-outputs form
{
	const r = rig()
	const f = r.fields()
	const o = planar(r, 'enc')
	r.write(r.P.yuv422p8, f[0].placed, o)
	r.d.touch(o.outputY, 'readonly', 2)
	expect('a yuv422p8 write of a de-interlaced field', r.names(), ['v210_yadif_pair_1', 'compose_up_multi_1'])
	const names = r.launches[1][1]
	for (const n of ['packedRgb', 'l0In', 'l0Matrix', 'l0Width', 'l0Height', 'output', 'outputU', 'outputV', 'outPacking', 'outColMatrix', 'outGammaLut', 'interlace'])
		expect(`the launch names '${n}'`, names.includes(n), true)
	expect('the reader was told to pack, nothing was unpacked, no fallback', [r.launches[0][1].includes('packedRgb'), r.d.stats.unpacked || 0, r.d.stats.fallbacks], [true, 0, 0])
}

// 1a. ... and with both fields' writes posted, both frames in that one launch: the twin's planes under their own names
{
	const r = rig()
	const f = r.fields()
	const o = [planar(r, 'a'), planar(r, 'b')]
	f.forEach((x, i) => r.write(r.P.yuv422p8, x.placed, o[i]))
	r.d.touch(o[0].outputY, 'readonly', 2)
	r.d.touch(o[1].outputV, 'readonly', 2)
	expect('both fields of an encoder\'s tick', r.names(), ['v210_yadif_pair_1', 'compose_up_multi_1'])
	for (const n of ['l0In2', 'twinOutput', 'twinOutputU', 'twinOutputV']) expect(`the launch names '${n}'`, r.launches[1][1].includes(n), true)
}

// 2. SDI + the screen, both fields of the tick: ONE launch - two jobs, two outputs each
{
	const r = rig()
	const f = r.fields()
	const sdi = [r.plane('sdi0'), r.plane('sdi1')], screen = [r.plane('scr0'), r.plane('scr1')]
	f.forEach((x, i) => { r.write(r.P.v210, x.placed, { output: sdi[i] }); r.write(r.P.bgra8, x.placed, { output: screen[i] }) })
	r.d.touch(sdi[0], 'readonly', 2)
	expect('v210 + bgra8 siblings, twin included', r.names(), ['v210_yadif_pair_1', 'compose_up_multi_1'])
	const names = r.launches[1][1]
	for (const n of ['packedRgb', 'l0In', 'l0In2', 'output', 'output1', 'out1Packing', 'out1GammaLut', 'interlace1', 'twinOutput', 'twinOutput1'])
		expect(`the launch names '${n}'`, names.includes(n), true)
	expect('no matrix for the packed-RGB consumer, no output2', names.includes('out1ColMatrix') || names.includes('output2'), false)
	for (const b of [...sdi, ...screen]) r.d.touch(b, 'readonly', 2)
	expect('all four frames came out of it', [r.names().length, [...r.d.pending].some((n) => n.program.name === 'write'), r.d.stats.unpacked || 0], [2, false, 0])
}

// 2a. two screens beside SDI, both fields: each of the twin's writes is matched once - six frames from one launch, no buffer named twice
{
	const r = rig()
	const f = r.fields()
	const outs = []
	f.forEach((x) => { for (const p of [r.P.v210, r.P.bgra8, r.P.bgra8]) { const o = r.plane('o'); outs.push(o); r.write(p, x.placed, { output: o }) } })
	r.d.touch(outs[0], 'readonly', 2)
	expect('two consumers of one format, twin included', [r.names(), r.d.stats.fallbacks], [['v210_yadif_pair_1', 'compose_up_multi_1'], 0])
	const names = r.launches[1][1]
	expect('... named apart', ['output1', 'output2', 'twinOutput', 'twinOutput1', 'twinOutput2'].every((n) => names.includes(n)), true)
	for (const o of outs) r.d.touch(o, 'readonly', 2)
	expect('... and nothing more is launched for the other five', r.names().length, 2)
}

// 3. the option off: today's launches
{
	const r = rig({ upWriters: false })
	const f = r.fields()
	const sdi = r.plane('sdi'), screen = r.plane('scr')
	r.write(r.P.v210, f[0].placed, { output: sdi })
	r.write(r.P.bgra8, f[0].placed, { output: screen })
	r.d.touch(sdi, 'readonly', 2)
	r.d.touch(screen, 'readonly', 2)
	// (what these two writes have always been: the SDI write finds the screen's beside it, and the channel kernel makes both from the unpacked field)
	expect('upWriters false: today\'s launches', r.names(), ['v210_yadif_pair_1', 'rgb_unpack', 'chan_compose_multi_1'])
	const r2 = rig({ upWriters: false })
	const f2 = r2.fields()
	const o = planar(r2, 'enc')
	r2.write(r2.P.yuv422p8, f2[0].placed, o)
	r2.d.touch(o.outputY, 'readonly', 2)
	expect('upWriters false, an encoder alone: the fields are not packed, the channel kernel', [r2.names().filter((n) => n.startsWith('compose_up_')).length, r2.launches[0][1].includes('packedRgb'),
		r2.names().some((n) => n.startsWith('chan_compose_v210_'))], [0, false, true])
}

// 4. a sibling posted after the first frame was asked for: a launch of its own (from the fields that are still packed)
{
	const r = rig()
	const f = r.fields()
	const sdi = r.plane('sdi'), screen = r.plane('scr')
	r.write(r.P.v210, f[0].placed, { output: sdi })
	r.d.touch(sdi, 'readonly', 2)
	r.write(r.P.bgra8, f[0].placed, { output: screen })
	r.d.touch(screen, 'readonly', 2)
	expect('a late sibling', r.names(), ['v210_yadif_pair_1', 'compose_up_write_v210_1', 'compose_up_multi_1'])
}

// 5. the launch refused: today's candidates make the frame that was asked for, the sibling still gets its own
{
	const r = rig({ refuse: (name) => name.startsWith('compose_up_multi_') })
	const f = r.fields()
	const sdi = r.plane('sdi'), screen = r.plane('scr')
	r.write(r.P.v210, f[0].placed, { output: sdi })
	r.write(r.P.bgra8, f[0].placed, { output: screen })
	r.d.touch(sdi, 'readonly', 2)
	expect('a refused launch falls through to today\'s', [r.names(), r.d.stats.fallbacks >= 1], [['v210_yadif_pair_1', 'compose_up_write_v210_1'], true])
	r.d.touch(screen, 'readonly', 2)
	expect('... and the screen gets its frame from the unpacked field', [r.names().includes('rgb_unpack'), r.names().some((n) => n.startsWith('chan_compose_')),
		[...r.d.pending].some((n) => n.program.name === 'write')], [true, true, false])
}

// 6. a field unpacked between plan and commit: the plan (made with packedRgb) is stale, the frame is planned again
{
	const r = rig()
	const f = r.fields()
	const o = planar(r, 'enc')
	const w = r.write(r.P.yuv422p8, f[0].placed, o)
	const node = [...r.d.pending].find((n) => n.program.name === 'write')
	const plan = r.d._plan(node)
	expect('the plan is for packed fields', [plan.candidates[0][0], plan.candidates[0][1].packedRgb, r.d._fresh(plan)], ['compose_up_multi_1', 1, true])
	r.d._unpack(f[0].field) // (another consumer's launch took the field as an image)
	expect('... and stale once one is unpacked', r.d._fresh(plan), false)
	r.d._commit(plan)
	const last = r.launches[r.launches.length - 1]
	expect('planned again: no launch is told packedRgb about an RGBA image', [last[0], last[1].includes('packedRgb'), node.state !== 'pending'], ['compose_up_multi_1', false, true])
	void w
}

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
