'use strict'
// node/defer.js without a device: several consumers' writes of one combined image (the stand-in for the addon only counts, as in
// defer_check.js).  What goes to the device for them, what the launch's parameters are called, and what happens when the option is
// off, a sibling comes late, or the launch is refused.  Prints one JSON object { checks, problems }.
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
	const ctx = { _native: native, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, multiWriter: opt.multiWriter }
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
	const P = { read: program('read', { format: 'v210', globalWorkItems: [2 * H], workItemsPerGroup: 2 }), transform: program('transform'), combine2: program('combine_2'),
		v210: writer('v210', H), v210Field: writer('v210', H / 2), bgra8: writer('bgra8', H), yuv422p8: writer('yuv422p8', H), nv12: writer('nv12', H / 2) }
	const param = (tag, bytes, fill) => { const b = buffer(bytes, undefined, tag); b.fill(fill); return b }
	const L = { colMatrix: param('cm', 48, 1), gammaLut: param('lut', 64, 2), gamutMatrix: param('gm', 36, 3) }
	const saver = { colMatrix: param('wcm', 48, 7), gammaLut: param('wlut', 64, 8) }
	const image = (owner) => buffer(W * H * 16, { width: W, height: H }, owner)
	const plane = (owner) => buffer(256 * H, undefined, owner)
	// a tick's chain up to the combined image: a plain v210 layer under a placed one (the channel kernel's frame, not the headline's)
	const combined = () => {
		const u = [image('u0'), image('u1')], placed = image('p1'), comb = image('comb')
		u.forEach((im, i) => d.record(P.read, Object.assign({ input: plane(`s${i}`), output: im, width: W }, L), 1))
		d.record(P.transform, { input: u[1], output: placed, transformMatrix: param('m', 48, 0) }, 1)
		d.record(P.combine2, { l0In: u[0], l1In: placed, output: comb }, 1)
		return comb
	}
	const write = (prog, comb, outs, interlace = 0) => d.record(prog, Object.assign({ input: comb, width: W, interlace }, outs, saver), 1)
	return { d, launches, P, L, W, image, plane, combined, write, names: () => launches.map((l) => l[0]) }
}

// 1. SDI + the screen + an encoder + a 4:2:0 consumer on one image: one launch with four outputs, named as the program wants them
{
	const r = rig()
	const comb = r.combined()
	const out = { v210: r.plane('sdi'), bgra8: r.plane('screen'), y: r.plane('y'), u: r.plane('u'), v: r.plane('v'), ny: r.plane('ny'), nc: r.plane('nc') }
	r.write(r.P.v210Field, comb, { output: out.v210 }, 1)
	r.write(r.P.bgra8, comb, { output: out.bgra8 })
	r.write(r.P.yuv422p8, comb, { outputY: out.y, outputU: out.u, outputV: out.v })
	r.write(r.P.nv12, comb, { outputY: out.ny, outputC: out.nc })
	r.d.touch(out.bgra8, 'readonly', 2) // whichever consumer asks first
	expect('one launch for four consumers', r.names(), ['chan_compose_multi_2'])
	const names = r.launches[0][1]
	// (the consumer that asked is output 0; the others follow in the order they were posted: the SDI field, the encoder, the 4:2:0 consumer)
	for (const n of ['output', 'interlace', 'outPacking', 'outGammaLut', 'output1', 'out1ColMatrix', 'out1GammaLut', 'interlace1', 'output2', 'output2U', 'output2V', 'out2Packing',
		'out2ColMatrix', 'out2GammaLut', 'interlace2', 'output3', 'output3C', 'out3Packing', 'out3ColMatrix', 'out3GammaLut', 'interlace3'])
		expect(`the launch names '${n}'`, names.includes(n), true)
	expect('no matrix for a packed-RGB consumer, no packing for v210', names.includes('outColMatrix') || names.includes('out1Packing') || names.includes('output1U'), false)
	expect('every write is done', [r.d.pending.size > 0 && [...r.d.pending].some((n) => n.program.name === 'write'), r.d.stats.multiOutputs, r.d.stats.launched], [false, 3, 1])
	for (const b of Object.values(out)) r.d.touch(b, 'readonly', 2)
	expect('asking the other consumers launches nothing more', r.names(), ['chan_compose_multi_2'])
}

// 2. the option off: a launch per consumer, as ever
{
	const r = rig({ multiWriter: false })
	const comb = r.combined()
	const a = r.plane('sdi'), b = r.plane('screen')
	r.write(r.P.v210, comb, { output: a })
	r.write(r.P.bgra8, comb, { output: b })
	r.d.touch(a, 'readonly', 2)
	r.d.touch(b, 'readonly', 2)
	expect('multiWriter false', [r.names(), r.d.stats.multiOutputs || 0], [['chan_compose_v210_2', 'chan_compose_v210_2'], 0])
}

// 3. a sibling posted after the first frame was asked for: a launch of its own
{
	const r = rig()
	const comb = r.combined()
	const a = r.plane('sdi'), b = r.plane('screen')
	r.write(r.P.v210, comb, { output: a })
	r.d.touch(a, 'readonly', 2)
	r.write(r.P.bgra8, comb, { output: b })
	r.d.touch(b, 'readonly', 2)
	expect('a late sibling', r.names(), ['chan_compose_v210_2', 'chan_compose_v210_2'])
}

// 4. the multi launch refused: today's candidates make the frame that was asked for, the sibling stays recorded until it is asked for
{
	const r = rig({ refuse: (name) => name.startsWith('chan_compose_multi_') })
	const comb = r.combined()
	const a = r.plane('sdi'), b = r.plane('screen')
	r.write(r.P.v210, comb, { output: a })
	r.write(r.P.bgra8, comb, { output: b })
	r.d.touch(a, 'readonly', 2)
	expect('a refused multi launch falls through', [r.names(), r.d.stats.fallbacks >= 1], [['chan_compose_v210_2'], true])
	r.d.touch(b, 'readonly', 2)
	expect('... and the sibling still gets its frame', [r.names().length, r.d.pending.size > 0 && [...r.d.pending].some((n) => n.program.name === 'write')], [2, false])
}

// 5. two consumers writing into ONE buffer are not siblings; five consumers are one launch of four and one of one
{
	const r = rig()
	const comb = r.combined()
	const a = r.plane('sdi')
	r.write(r.P.v210Field, comb, { output: a }, 1)
	r.write(r.P.v210Field, comb, { output: a }, 3) // (recording the second field runs the first: it fills part of the same frame)
	r.d.touch(a, 'readonly', 2)
	expect('two fields into one frame', r.names(), ['chan_compose_v210_2', 'chan_compose_v210_2'])
	const r2 = rig()
	const comb2 = r2.combined()
	const outs = [0, 1, 2, 3, 4].map((i) => r2.plane(`o${i}`))
	outs.forEach((o) => r2.write(r2.P.v210, comb2, { output: o }))
	outs.forEach((o) => r2.d.touch(o, 'readonly', 2))
	expect('five consumers', r2.names(), ['chan_compose_multi_2', 'chan_compose_v210_2'])
}

// 6. a field write that is still being recorded is nobody's sibling: recording it runs the pending frame write of its destination,
// and that launch takes the other recorded frames with it - among them a write of the very image the new job reads
{
	const r = rig()
	const I = r.combined(), K = r.combined()
	const o = r.plane('frame'), other = r.plane('other')
	r.write(r.P.v210, K, { output: o }) // a whole frame into o, pending
	r.write(r.P.bgra8, I, { output: other }) // another consumer of I, pending
	r.write(r.P.v210Field, I, { output: o }, 1) // a field of I into o: the frame write runs first
	expect('recording a field runs the frame under it, and only that and its group', r.names().every((n) => n === 'chan_compose_v210_2'), true)
	r.d.touch(o, 'readonly', 2)
	r.d.touch(other, 'readonly', 2)
	expect('the field is written after the frame, every write has run exactly once', [r.names().filter((n) => n.startsWith('chan_compose_multi_')).length <= 1,
		[...r.d.pending].filter((n) => n.program.name === 'write' || n.state !== 'pending').length], [true, 0])
}

// 7. the headline's shape (plain reads of the output's size) with two consumers: one launch too; with one consumer the headline kernel as ever
{
	const r = rig()
	const plain = () => {
		const u = [r.image('u0'), r.image('u1')], comb = r.image('comb')
		u.forEach((im, i) => r.d.record(r.P.read, Object.assign({ input: r.plane(`s${i}`), output: im, width: r.W }, r.L), 1))
		r.d.record(r.P.combine2, { l0In: u[0], l1In: u[1], output: comb }, 1)
		return comb
	}
	const one = plain(), a = r.plane('sdi')
	r.write(r.P.v210, one, { output: a })
	r.d.touch(a, 'readonly', 2)
	const two = plain(), b = r.plane('sdi'), c = r.plane('screen')
	r.write(r.P.v210, two, { output: b })
	r.write(r.P.bgra8, two, { output: c })
	r.d.touch(b, 'readonly', 2)
	r.d.touch(c, 'readonly', 2)
	expect('plain reads: one consumer, then two', r.names(), ['fused_v210_combine_2', 'chan_compose_multi_2'])
}

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
