'use strict'
// The `fusedWriters` option through the node layer on the GPU: a headline-shaped frame - plain v210 reads of the output's size, combine_2,
// write - (a) with ONE terminal write that is not a v210 frame (an encoder's yuv422p8) and (b) with sibling writes (SDI's v210 + the
// screen's bgra8), posted to the launch-as-posted context and to the recording context with the option off and on.  Either way every
// consumer must see the launch-as-posted context's bytes.  With the option off the recorded stream's launches are the parent's - the
// channel kernel's ("chan_compose_v210<0,2>" for a yuv422p8 frame, "chan_compose_multi<0>x2" for v210 + bgra8 in a trace); with it on a
// tick is one "fused_v210_combine_multi x<outputs>" launch.
// usage: node fused_writers_run.js [width=384] [height=12]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '12')
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
	const s = { rig, deferred, frame: 0, writeAs: {} }
	s.read = await rig.unpack('v210', W, H, '709', '709')
	for (const fmt of ['v210', 'yuv422p8', 'bgra8']) s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	s.combine = await rig.combine(2, W, H)
	s.source = async (seed) => {
		const p = (await rig.planes('v210', W, H))[0]
		await rig.upload(p, v210Frame(p.length, seed))
		await rig.sync(rig.ctx.queue.load)
		return p
	}
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
	// the headline's chain up to the combined image: two plain v210 layers of the output's size
	s.combined = async (seed) => {
		const a = await s.source(seed), b = await s.source(seed + 50)
		const ua = await rig.image(W, H), ub = await rig.image(W, H), comb = await rig.image(W, H)
		rig.post(s.id('A'), s.read([a], ua), () => a.release())
		rig.post(s.id('B'), s.read([b], ub), () => b.release())
		rig.post(s.id('mix'), s.combine([ua, ub], comb), () => [ua, ub].forEach((x) => x.release()))
		return comb
	}
	return s
}

// TICKS ticks of one channel with these consumers, on one context; returns what the consumers saw, the traced routes and the counters
async function run(deferred, options, list) {
	const s = await side(deferred, options)
	const seen = []
	const routes = []
	try {
		for (let t = 0; t < TICKS; ++t) {
			const comb = await s.combined(100 + t)
			const outs = []
			for (const fmt of list) outs.push(await s.planes(fmt))
			if (deferred) s.rig.ctx.traceBegin(false)
			list.forEach((fmt, i) => s.rig.post(s.id('mix'), s.writeAs[fmt](comb, outs[i], 0), i === list.length - 1 ? () => comb.release() : () => {}))
			for (const k of ['A', 'B', 'mix']) await s.flush(s.id(k))
			for (const planes of outs) { seen.push(...await s.consume(planes)); planes.forEach((p) => p.release()) }
			if (deferred) routes.push(s.rig.ctx.traceEnd())
			s.frame++
		}
		const st = deferred ? s.rig.ctx.deferredStats() : null
		s.rig.close()
		const left = s.rig.ctx.flushDeferred ? s.rig.ctx.flushDeferred() : null
		if (deferred && left && left.pending) problems.push({ what: `${left.pending} recorded jobs still pending` })
		const live = s.rig.ctx.bufferStats()
		if (live.liveBuffers !== 0) problems.push({ what: `${live.liveBuffers} buffers still alive on the ${deferred ? 'deferred' : 'plain'} side` })
		return { seen, routes, st }
	} catch (e) {
		problems.push({ what: `${deferred ? 'deferred' : 'plain'} side: ${e && e.stack || e}` })
		return { seen: [], routes, st: null }
	}
}

async function scenario(name, list, offRoute, onRoute) {
	const plain = await run(false, {}, list)
	const off = await run(true, {}, list)
	const on = await run(true, { fusedWriters: true }, list)
	for (const [what, got] of [['fusedWriters off', off], ['fusedWriters on', on]]) {
		if (got.seen.length !== plain.seen.length || !plain.seen.length) problems.push({ scenario: name, what: `${what}: frames seen ${got.seen.length}, launch-as-posted ${plain.seen.length}` })
		for (let i = 0; i < Math.min(plain.seen.length, got.seen.length); ++i)
			if (Buffer.compare(plain.seen[i], got.seen[i]) !== 0) problems.push({ scenario: name, what: `${what}: plane ${i} differs from the launch-as-posted context's` })
	}
	for (const b of plain.seen) if (b.every((x) => x === 0x5a)) problems.push({ scenario: name, what: 'a frame nobody wrote' })
	if (!off.routes.every((r) => offRoute.test(r))) problems.push({ scenario: name, what: `fusedWriters off: a tick's launches ${JSON.stringify(off.routes)}` })
	if (!on.routes.every((r) => r === onRoute)) problems.push({ scenario: name, what: `fusedWriters on: a tick's launches ${JSON.stringify(on.routes)}, ${onRoute} expected` })
	if (on.st && on.st.launched !== TICKS) problems.push({ scenario: name, what: `fusedWriters on: ${on.st.launched} launches, ${TICKS} expected` })
	scenarios.push({ name, frames: plain.seen.length, off: off.routes, on: on.routes })
}

async function main() {
	await scenario('yuv422p8 alone', ['yuv422p8'], /^chan_compose_v210<\d,2>$/, 'fused_v210_combine_multi x1')
	await scenario('v210 + bgra8', ['v210', 'bgra8'], /^chan_compose_multi<\d>x2$/, 'fused_v210_combine_multi x2')
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
