'use strict'
// The counting stand-in for the addon that the device-free checks of node/defer.js share (defer_check.js, packed_state_check.js): a
// Deferral on a context whose native calls only note what was launched, in which order, on which buffers.
const { Deferral } = require('../defer.js')
const { bufferPrototype, newPark } = require('../index.js')

// native.observe (optional, set by the caller): called with (program name, argument names, values) for every job that reaches the device,
// alone or in a runPrograms call - buffers are their handles
function rig(opt) { // opt.early: frames are launched at the end of the posting tick (clContext's earlyLaunch); opt.batch: the addon has runPrograms
	opt = opt || {}
	const launches = [] // [program name, queue]
	const orders = [] // [waiter, signal]
	let nextId = 1
	const refs = new Map() // handle -> count (0 = freed)
	const native = {
		bufAddRef: (h) => { if (!refs.get(h)) throw new Error(`addRef on freed buffer ${h}`); refs.set(h, refs.get(h) + 1) },
		bufRelease: (h) => { if (!refs.get(h)) throw new Error(`release on freed buffer ${h}`); refs.set(h, refs.get(h) - 1) },
		bufRefCount: (h) => refs.get(h) || 0,
		createProgram: (_ctx, _src, name) => ({ name }),
		runProgram: (_ctx, prog, names, values, queue, _timed, checkOnly) => {
			if (checkOnly) return null
			if (native.refuse && native.refuse(prog.name)) throw new Error(`${prog.name}: refused`)
			for (const v of values) if (v && typeof v === 'object' && !refs.get(v)) throw new Error(`${prog.name} launched on a freed buffer`)
			if (native.observe) native.observe(prog.name, names, values)
			launches.push([prog.name, queue, names.join(',')])
			return { dataToKernel: 0, kernelExec: 0, totalTime: 0 }
		},
		queueWaitQueue: (_ctx, waiter, signal) => orders.push([waiter, signal])
	}
	if (opt.batch) native.runPrograms = (_ctx, progs, names, values, queue) => {
		if (opt.progress) native.progress = 0 // (the addon: a call that throws before it reaches the library has made nothing)
		if (native.refuse && native.refuse('batch')) throw new Error('batch: refused')
		for (const vs of values) for (const v of vs) if (v && typeof v === 'object' && !refs.get(v)) throw new Error('batch launched on a freed buffer')
		if (native.observe) progs.forEach((p, j) => native.observe(p.name, names[j], values[j]))
		launches.push([`batch:${progs.map((p) => p.name).join('+')}`, queue, names.map((n) => n.join(',')).join(';'), values])
		if (opt.progress) native.progress = progs.length
	}
	// opt.progress: the addon has runProgramsProgress - how many jobs of the last runPrograms call had their launches made
	if (opt.batch && opt.progress) { native.progress = 0; native.runProgramsProgress = () => native.progress }
	const ctx = { _native: native, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, earlyLaunch: !!opt.early }
	const d = new Deferral(ctx)
	const proto = bufferPrototype(native, d, newPark(false, 0)) // the real reference counting of node/index.js; nothing is parked here
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
		b.alive = () => refs.get(h) > 0
		b.appRefs = () => b._refs
		Deferral.adopt(b, true)
		return b
	}
	const W = 96
	const H = 4
	const program = (name, extra) => Object.assign({ name, globalWorkItems: [W, H], workItemsPerGroup: 0, _handle: { name } }, extra || {})
	const P = {
		read: program('read', { format: 'v210', globalWorkItems: [2 * H], workItemsPerGroup: 2 }),
		write: program('write', { format: 'v210', globalWorkItems: [2 * H], workItemsPerGroup: 2 }),
		writeField: program('write', { format: 'v210', globalWorkItems: [H], workItemsPerGroup: 2 }),
		transform: program('transform'), combine2: program('combine_2'), dissolve: program('transition_dissolve'), yadif: program('yadif'),
		other: program('resize')
	}
	const param = (tag, bytes, fill) => { const b = buffer(bytes, undefined, tag); b.fill(fill); return b }
	const loader = (fill = 1) => ({ colMatrix: param('cm', 48, fill), gammaLut: param('lut', 64, fill + 1), gamutMatrix: param('gm', 36, fill + 2) })
	const saver = { colMatrix: param('wcm', 48, 7), gammaLut: param('wlut', 64, 8) }
	const image = (owner) => buffer(W * H * 16, { width: W, height: H }, owner)
	const v210 = (owner) => buffer(256 * H, undefined, owner)
	// a placement the 2 x 2-block compositor takes (node/defer.js `enlarged`): half a source texel per output pixel, no rotation
	const enlarging = () => { const b = buffer(48, undefined, 'matrix'); b.fill(0); new Float32Array(b.buffer, b.byteOffset, 9).set([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1]); return b }
	return { d, native, launches, orders, buffer, image, v210, P, loader, saver, enlarging, W, H, names: () => launches.map((l) => l[0]) }
}

module.exports = { rig, Deferral }
