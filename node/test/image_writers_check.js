'use strict'
// node/defer.js without a device (the stand-in for the addon only counts, as in defer_check.js): the `imageWriters` option.  Wire-format
// writes of an image that already exists are launched as posted; with the option the pending writes of the other consumers of that image
// go with the first one asked for as ONE pack_write_multi_<n> launch.  Prints one JSON object { checks, problems }.
const { Deferral } = require('../defer.js')
const { bufferPrototype, newPark } = require('../index.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function rig(opt = {}) {
	const launches = [] // [program name, parameter names, values by name]
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
			const byName = {}
			names.forEach((n, i) => { byName[n] = values[i] })
			launches.push([prog.name, names.slice().sort(), byName])
			return { dataToKernel: 0, kernelExec: 0, totalTime: 0 }
		},
		queueWaitQueue: () => {}
	}
	const ctx = { _native: native, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, imageWriters: opt.imageWriters }
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
	const writer = (format, lines) => ({ name: 'write', format, globalWorkItems: [2 * lines], workItemsPerGroup: 2, _handle: { name: 'write' } })
	const P = { v210: writer('v210', H), v210Field: writer('v210', H / 2), rgba8: writer('rgba8', H), p010: writer('p010', H / 2), yuv420p10: writer('yuv420p10', H / 2), yuv422p8: writer('yuv422p8', H) }
	const param = (tag, bytes, fill) => { const b = buffer(bytes, undefined, tag); b.fill(fill); return b }
	// every consumer's Saver makes its own buffers (loadSave.ts:152-160): equal contents, other buffers
	const saver = () => ({ colMatrix: param('wcm', 48, 7), gammaLut: param('wlut', 64, 8) })
	const image = (owner) => buffer(W * H * 16, { width: W, height: H }, owner)
	const plane = (owner) => buffer(256 * H, undefined, owner)
	const write = (prog, img, outs, interlace = 0) => d.record(prog, Object.assign({ input: img, width: W, interlace }, outs, saver()), 1)
	return { d, launches, P, W, H, image, plane, write, names: () => launches.map((l) => l[0]) }
}
const writesPending = (r) => [...r.d.pending].some((n) => n.program.name === 'write')

// 1. SDI + a Main10 encoder + the screen on an image that is already made: one launch with three outputs, named as the program wants them
{
	const r = rig({ imageWriters: true })
	const img = r.image('routed')
	const out = { sdi: r.plane('sdi'), y: r.plane('y'), c: r.plane('c'), screen: r.plane('screen') }
	r.write(r.P.v210, img, { output: out.sdi })
	r.write(r.P.p010, img, { outputY: out.y, outputC: out.c })
	r.write(r.P.rgba8, img, { output: out.screen })
	r.d.touch(out.sdi, 'readonly', 2)
	expect('one launch for three consumers', r.names(), ['pack_write_multi_3'])
	const [, names, v] = r.launches[0]
	for (const n of ['input', 'width', 'output', 'outPacking', 'outColMatrix', 'outGammaLut', 'interlace', 'output1', 'output1C', 'out1Packing', 'out1ColMatrix', 'out1GammaLut', 'interlace1',
		'output2', 'out2Packing', 'out2GammaLut', 'interlace2'])
		expect(`the launch names '${n}'`, names.includes(n), true)
	expect('no matrix for the packed-RGB consumer, no third output', names.includes('out2ColMatrix') || names.includes('output3') || names.includes('output1U'), false)
	expect('the formats and the width', [v.outPacking, v.out1Packing, v.out2Packing, v.width], [0, 8, 5, r.W])
	expect('tables of the same contents are one table', v.outGammaLut === v.out1GammaLut && v.outGammaLut === v.out2GammaLut, true)
	expect('every write is done', [writesPending(r), r.d.stats.multiOutputs, r.d.stats.imageWrites, r.d.stats.launched], [false, 2, 1, 1])
	for (const b of Object.values(out)) r.d.touch(b, 'readonly', 2)
	expect('asking the other consumers launches nothing more', r.names(), ['pack_write_multi_3'])
}

// 2. the option off (the default): three `write` launches, as ever
for (const imageWriters of [false, undefined]) {
	const r = rig({ imageWriters })
	const img = r.image('routed')
	const out = { sdi: r.plane('sdi'), y: r.plane('y'), c: r.plane('c'), screen: r.plane('screen') }
	r.write(r.P.v210, img, { output: out.sdi })
	r.write(r.P.p010, img, { outputY: out.y, outputC: out.c })
	r.write(r.P.rgba8, img, { output: out.screen })
	for (const b of Object.values(out)) r.d.touch(b, 'readonly', 2)
	expect(`imageWriters ${imageWriters}`, [r.names(), r.d.stats.multiOutputs || 0], [['write', 'write', 'write'], 0])
}

// 3. a sibling posted after the first frame was asked for: a launch of its own
{
	const r = rig({ imageWriters: true })
	const img = r.image('routed')
	const a = r.plane('sdi'), b = r.plane('screen')
	r.write(r.P.v210, img, { output: a })
	r.d.touch(a, 'readonly', 2)
	r.write(r.P.rgba8, img, { output: b })
	r.d.touch(b, 'readonly', 2)
	expect('a late sibling', [r.names(), r.d.stats.multiOutputs || 0], [['write', 'write'], 0])
}

// 4. the shared launch refused: the write that was asked for is launched as posted, the sibling stays recorded until it is asked for
{
	const r = rig({ imageWriters: true, refuse: (name) => name.startsWith('pack_write_multi_') })
	const img = r.image('routed')
	const a = r.plane('sdi'), b = r.plane('screen')
	r.write(r.P.v210, img, { output: a })
	r.write(r.P.rgba8, img, { output: b })
	r.d.touch(a, 'readonly', 2)
	expect('a refused launch falls through', [r.names(), r.d.stats.fallbacks >= 1, writesPending(r)], [['write'], true, true])
	r.d.touch(b, 'readonly', 2)
	expect('... and the sibling still gets its frame', [r.names(), writesPending(r)], [['write', 'write'], false])
}

// 5. two writes into ONE buffer never share a launch: posting the second field of SDI's frame launches the first (the recorder runs a
// buffer's pending producer before a job that fills part of it is registered), and the second field shares with the other consumers
{
	const r = rig({ imageWriters: true })
	const img = r.image('routed')
	const sdi = r.plane('sdi'), screen = r.plane('screen'), y = r.plane('y'), u = r.plane('u'), vv = r.plane('v')
	r.write(r.P.v210Field, img, { output: sdi }, 1)
	r.write(r.P.v210Field, img, { output: sdi }, 3)
	expect('the first field goes when the second is posted', [r.names(), r.launches[0][2].interlace], [['write'], 1])
	r.write(r.P.rgba8, img, { output: screen })
	r.write(r.P.yuv420p10, img, { outputY: y, outputU: u, outputV: vv })
	r.d.touch(screen, 'readonly', 2)
	const shared = r.launches[1]
	expect('the screen, the other field and the encoder share a launch', [shared[0], shared[2].outPacking, shared[2].out1Packing, shared[2].interlace1, shared[2].out2Packing], ['pack_write_multi_3', 5, 0, 3, 7])
	const outs = ['output', 'output1', 'output2', 'output2U', 'output2V'].map((n) => shared[2][n])
	expect('... into five different buffers', new Set(outs).size, 5)
	r.d.touch(sdi, 'readonly', 2)
	expect('nothing more is launched', [r.names(), writesPending(r)], [['write', 'pack_write_multi_3'], false])
}

// 6. one consumer alone: its own launch, whatever the option says
{
	const r = rig({ imageWriters: true })
	const img = r.image('routed')
	const y = r.plane('y'), c = r.plane('c')
	r.write(r.P.p010, img, { outputY: y, outputC: c })
	r.d.touch(y, 'readonly', 2)
	expect('one consumer', [r.names(), r.d.stats.fallbacks], [['write'], 0])
}

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
