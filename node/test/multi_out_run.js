'use strict'
// Several consumers on one channel (channel.ts:64-88: SDI plus an encoder or the screen, each with its own FromRGBA on the one combined
// image) through the recording context (node/defer.js) against the plain one, on the GPU.  Every consumer must see the same bytes on
// both sides; on the recording side the writes of a tick come out of ONE launch (chan_compose_multi_<n>) where a launch per writer was
// needed - unless the context says `multiWriter: false`, a sibling write is posted after the first frame was asked for, or the launch
// is refused (then today's launches make the frames).
// usage: node multi_out_run.js [width=384] [height=108]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '108')
const TICKS = 2
const problems = []
const scenarios = []

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }
function v210Frame(bytes, seed) {
	const r = lcg(seed)
	const b = Buffer.alloc(bytes)
	const code = () => 64 + (r() >>> 8) % 877
	for (let i = 0; i + 4 <= bytes; i += 4) b.writeUInt32LE((code() | (code() << 10) | (code() << 20)) >>> 0, i)
	return b
}

async function side(deferred, options) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, deferred, spinWaitMicros: 100 }, options))
	const s = { rig, deferred, frame: 0, writeAs: {}, fieldAs: {} }
	s.read = await rig.unpack('v210', W, H, '709', '709')
	for (const fmt of ['v210', 'yuv422p8', 'rgba8', 'bgra8']) s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	s.fieldAs.v210 = await rig.pack('v210', W, H, '709', true)
	s.combine = await rig.combine(2, W, H)
	s.transform = await rig.transform(W, H)
	s.source = async (seed) => {
		const p = (await rig.planes('v210', W, H))[0]
		await rig.upload(p, v210Frame(p.length, seed))
		await rig.sync(rig.ctx.queue.load)
		return p
	}
	// the frame's planes, filled with a pattern first (a field write leaves the other field's lines as they are)
	s.planes = async (fmt) => {
		const planes = await rig.planes(fmt, W, H, 'readwrite')
		for (const p of planes) await rig.upload(p, Buffer.alloc(p.length, 0x5a))
		await rig.sync(rig.ctx.queue.load)
		return planes
	}
	s.id = (name) => ({ source: name, timestamp: s.frame })
	s.flush = (id) => rig.board.flush(id)
	s.consume = async (planes) => {
		const seen = []
		for (const p of planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		return seen
	}
	// a tick's chain up to the combined image: a v210 background under a placed v210 inset
	s.combined = async (seed) => {
		const a = await s.source(seed), b = await s.source(seed + 50)
		const ua = await rig.image(W, H), ub = await rig.image(W, H), pb = await rig.image(W, H), comb = await rig.image(W, H)
		rig.post(s.id('A'), s.read([a], ua), () => a.release())
		rig.post(s.id('B'), s.read([b], ub), () => b.release())
		rig.post(s.id('B'), s.transform(ub, pb, await s.transform.matrix({ scaleX: 0.5, scaleY: 0.5, offsetX: 0.25, offsetY: -0.25 })), () => ub.release())
		rig.post(s.id('mix'), s.combine([ua, pb], comb), () => [ua, pb].forEach((x) => x.release()))
		return comb
	}
	return s
}

// fn(side) -> the Buffers the consumers saw, on both sides; returns the recording side's counters
async function scenario(name, fn, options = {}) {
	const got = []
	let st = null
	for (const deferred of [false, true]) {
		const s = await side(deferred, options)
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
	scenarios.push({ name, frames: plain.length, deferred: st })
	return st || {}
}

// TICKS ticks of one channel with these consumers: [format, field] each (field 0: a whole frame)
const consumers = (list) => async (s) => {
	const seen = []
	for (let t = 0; t < TICKS; ++t) {
		const comb = await s.combined(100 + t)
		const outs = []
		for (const [fmt, field] of list) outs.push(await s.planes(fmt))
		list.forEach(([fmt, field], i) => {
			const write = field ? s.fieldAs[fmt] : s.writeAs[fmt]
			s.rig.post(s.id('mix'), write(comb, outs[i], field), i === list.length - 1 ? () => comb.release() : () => {})
		})
		for (const k of ['A', 'B', 'mix']) await s.flush(s.id(k))
		for (const planes of outs) { seen.push(...await s.consume(planes)); planes.forEach((p) => p.release()) }
		s.frame++
	}
	return seen
}

function expectLaunches(name, st, want) {
	if (st.launched !== want) problems.push({ scenario: name, what: `${st.launched} launches, ${want} expected (${JSON.stringify(st)})` })
}

async function main() {
	let st = await scenario('v210 + bgra8', consumers([['v210', 0], ['bgra8', 0]]))
	expectLaunches('v210 + bgra8', st, TICKS)
	if (st.multiOutputs !== TICKS) problems.push({ scenario: 'v210 + bgra8', what: `${st.multiOutputs} sibling writes folded, ${TICKS} expected` })
	st = await scenario('v210 + yuv422p8 + rgba8', consumers([['v210', 0], ['yuv422p8', 0], ['rgba8', 0]]))
	expectLaunches('v210 + yuv422p8 + rgba8', st, TICKS)
	st = await scenario('v210 field + rgba8 frame', consumers([['v210', 1], ['rgba8', 0]]))
	expectLaunches('v210 field + rgba8 frame', st, TICKS)
	// the parent's behaviour: a launch per writer
	st = await scenario('multiWriter: false', consumers([['v210', 0], ['bgra8', 0]]), { multiWriter: false })
	expectLaunches('multiWriter: false', st, 2 * TICKS)
	if (st.multiOutputs) problems.push({ scenario: 'multiWriter: false', what: `${st.multiOutputs} sibling writes folded with the option off` })
	// a sibling write posted after the first frame was asked for: a launch of its own, the same bytes
	st = await scenario('a sibling posted late', async (s) => {
		const comb = await s.combined(300)
		const first = await s.planes('v210'), second = await s.planes('bgra8')
		s.rig.post(s.id('mix'), s.writeAs.v210(comb, first, 0), () => {})
		for (const k of ['A', 'B', 'mix']) await s.flush(s.id(k))
		const seen = await s.consume(first)
		s.frame++
		s.rig.post(s.id('mix'), s.writeAs.bgra8(comb, second, 0), () => comb.release())
		await s.flush(s.id('mix'))
		seen.push(...await s.consume(second))
		;[...first, ...second].forEach((p) => p.release())
		return seen
	})
	expectLaunches('a sibling posted late', st, 2)
	// the multi launch made to fail (context option fail_launches while it is being made): today's launches make the frames
	st = await scenario('a refused multi launch falls back', async (s) => {
		const native = s.rig.ctx._native
		const run = native.runProgram
		const deferral = s.rig.ctx._deferral
		if (deferral) native.runProgram = function (ctx, handle, names, values, queue, profile, checkOnly) {
			let multi = false
			for (const p of deferral.programs.values()) if (p._handle === handle && p.name.startsWith('chan_compose_multi_')) multi = true
			if (!multi || checkOnly) return run.apply(this, arguments)
			s.rig.ctx.setOption('fail_launches', 1)
			try { return run.apply(this, arguments) } finally { s.rig.ctx.setOption('fail_launches', 0) }
		}
		try { return await consumers([['v210', 0], ['bgra8', 0]])(s) } finally { native.runProgram = run }
	})
	expectLaunches('a refused multi launch falls back', st, 2 * TICKS)
	if (!(st.fallbacks >= TICKS) || st.multiOutputs) problems.push({ scenario: 'a refused multi launch falls back', what: `fallbacks ${st.fallbacks}, folded ${st.multiOutputs}: ${st.lastFallback}` })
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
