'use strict'
// The `imageWriters` option through the node layer on the GPU: a recording context with imageWriters: true and the plain context post the
// same job stream - an image that already exists (a routed channel's frame) consumed by v210 writers in both field modes, a p010 writer
// (a Main10 encoder) and an rgba8 writer (the screen) - and every consumer must see the same bytes.  The recording side makes a tick's
// four frames with ONE pack_write_multi_4 launch; with the option off, a sibling posted late or a refused launch it makes today's launches.
// usage: node image_writers_run.js [width=96] [height=8] [ticks=2]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const TICKS = parseInt(process.argv[4] || '2')
const problems = []
const scenarios = []

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }
function imageBytes(w, h, seed) { // f32 RGBA in [-0.05, 1.05)
	const r = lcg(seed)
	const f = new Float32Array(w * h * 4)
	for (let i = 0; i < f.length; ++i) f[i] = (r() >>> 8) / 16777216 * 1.1 - 0.05
	return Buffer.from(f.buffer)
}

const CONSUMERS = [['v210', 1], ['v210', 3], ['p010', 0], ['rgba8', 0]]

async function side(deferred, options, W, H) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, deferred, spinWaitMicros: 100 }, options))
	const s = { rig, deferred, frame: 0, W, H, writeAs: {}, fieldAs: {} }
	for (const fmt of ['v210', 'p010', 'rgba8']) s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	s.fieldAs.v210 = await rig.pack('v210', W, H, '709', true)
	// the frame's planes, filled with a pattern first (a field write leaves the other field's lines as they are)
	s.planes = async (fmt) => {
		const planes = await rig.planes(fmt, W, H, 'readwrite')
		for (const p of planes) await rig.upload(p, Buffer.alloc(p.length, 0x5a))
		await rig.sync(rig.ctx.queue.load)
		return planes
	}
	// an image that exists: what a ROUTE from another channel hands over
	s.routed = async (seed) => {
		const im = await rig.image(W, H)
		await rig.upload(im, imageBytes(W, H, seed))
		await rig.sync(rig.ctx.queue.load)
		return im
	}
	s.id = (name) => ({ source: name, timestamp: s.frame })
	s.flush = (id) => rig.board.flush(id)
	s.consume = async (planes) => {
		const seen = []
		for (const p of planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		return seen
	}
	s.post = (image, [fmt, field], planes, done) => rig.post(s.id('out'), (field ? s.fieldAs[fmt] : s.writeAs[fmt])(image, planes, field), done || (() => {}))
	return s
}

// fn(side) -> the Buffers the consumers saw, on both sides; returns the recording side's counters
async function scenario(name, fn, options = {}, W = parseInt(process.argv[2] || '96'), H = parseInt(process.argv[3] || '8')) {
	const got = []
	let st = null
	for (const deferred of [false, true]) {
		const s = await side(deferred, options, W, H)
		try {
			got.push(await fn(s))
			if (deferred) st = s.rig.ctx.deferredStats()
			s.rig.close()
			const left = s.rig.ctx.flushDeferred ? s.rig.ctx.flushDeferred() : null
			if (deferred && left && left.pending) problems.push({ scenario: name, what: `${left.pending} recorded jobs still pending` })
			const live = s.rig.ctx.bufferStats()
			if (live.liveBuffers !== 0) problems.push({ scenario: name, what: `${live.liveBuffers} buffers still alive on the ${deferred ? 'deferred' : 'plain'} side` })
		} catch (e) {
			problems.push({ scenario: name, what: `${deferred ? 'deferred' : 'plain'} side: ${e && e.stack || e}` })
			got.push([])
		}
	}
	const [plain, lazy] = got
	if (plain.length !== lazy.length || !plain.length) problems.push({ scenario: name, what: `frames seen: plain ${plain.length}, deferred ${lazy.length}` })
	for (let i = 0; i < Math.min(plain.length, lazy.length); ++i)
		if (Buffer.compare(plain[i], lazy[i]) !== 0) problems.push({ scenario: name, what: `frame ${i} differs between the plain and the recording context` })
	for (const b of plain) if (b.every((x) => x === 0x5a)) problems.push({ scenario: name, what: 'a frame nobody wrote' })
	scenarios.push({ name, frames: plain.length, deferred: st })
	return st || {}
}

// TICKS ticks of the consumers on a routed image
const ticks = async (s) => {
	const seen = []
	for (let t = 0; t < TICKS; ++t) {
		const im = await s.routed(100 + t)
		const outs = []
		for (const [fmt] of CONSUMERS) outs.push(await s.planes(fmt))
		CONSUMERS.forEach((c, i) => s.post(im, c, outs[i], i === CONSUMERS.length - 1 ? () => im.release() : null))
		await s.flush(s.id('out'))
		for (const planes of outs) { seen.push(...await s.consume(planes)); planes.forEach((p) => p.release()) }
		s.frame++
	}
	return seen
}

function expectLaunches(name, st, want) {
	if (st.launched !== want) problems.push({ scenario: name, what: `${st.launched} launches, ${want} expected (${JSON.stringify(st)})` })
}

async function main() {
	let st = await scenario('v210 fields + p010 + rgba8', ticks, { imageWriters: true })
	expectLaunches('v210 fields + p010 + rgba8', st, TICKS)
	if (st.multiOutputs !== 3 * TICKS) problems.push({ scenario: 'v210 fields + p010 + rgba8', what: `${st.multiOutputs} sibling writes folded, ${3 * TICKS} expected` })
	// the parent's behaviour (and the default): a launch per writer
	st = await scenario('imageWriters off', ticks, {})
	expectLaunches('imageWriters off', st, CONSUMERS.length * TICKS)
	if (st.multiOutputs) problems.push({ scenario: 'imageWriters off', what: `${st.multiOutputs} sibling writes folded with the option off` })
	// a sibling write posted after the first frame was asked for: a launch of its own, the same bytes
	st = await scenario('a sibling posted late', async (s) => {
		const im = await s.routed(300)
		const first = await s.planes('p010'), second = await s.planes('rgba8')
		s.post(im, ['p010', 0], first)
		await s.flush(s.id('out'))
		const seen = await s.consume(first)
		s.frame++
		s.post(im, ['rgba8', 0], second, () => im.release())
		await s.flush(s.id('out'))
		seen.push(...await s.consume(second))
		;[...first, ...second].forEach((p) => p.release())
		return seen
	}, { imageWriters: true })
	expectLaunches('a sibling posted late', st, 2)
	// the shared launch made to fail (context option fail_launches while it is being made): today's launches make the frames
	st = await scenario('a refused launch falls back', async (s) => {
		const native = s.rig.ctx._native
		const run = native.runProgram
		const deferral = s.rig.ctx._deferral
		if (deferral) native.runProgram = function (ctx, handle, names, values, queue, profile, checkOnly) {
			let multi = false
			for (const p of deferral.programs.values()) if (p._handle === handle && p.name.startsWith('pack_write_multi_')) multi = true
			if (!multi || checkOnly) return run.apply(this, arguments)
			s.rig.ctx.setOption('fail_launches', 1)
			try { return run.apply(this, arguments) } finally { s.rig.ctx.setOption('fail_launches', 0) }
		}
		try { return await ticks(s) } finally { native.runProgram = run }
	}, { imageWriters: true })
	expectLaunches('a refused launch falls back', st, CONSUMERS.length * TICKS)
	if (!(st.fallbacks >= TICKS) || st.multiOutputs) problems.push({ scenario: 'a refused launch falls back', what: `fallbacks ${st.fallbacks}, folded ${st.multiOutputs}: ${st.lastFallback}` })
	// a 1280 x 720 channel: the v210 frames' lines end in a tail quad - split off inside the call, still one job per tick
	st = await scenario('1280 x 720', ticks, { imageWriters: true }, 1280, 720)
	expectLaunches('1280 x 720', st, TICKS)
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
