'use strict'
// The `fusedTransitions` option through the node layer on the GPU: a headline-shaped frame with its top layer in a transition - plain v210
// reads of the output's size (x2, + a wipe's mask), transition_dissolve / transition_wipe, combine_2, write - posted to the launch-as-posted
// context and to the recording context with the option off and on.  Three ticks: a dissolve, a wipe by an f32 mask image, a wipe by a
// v210 mask frame; (a) SDI's v210 write alone and (b) with the screen's bgra8 write beside it.  Either way every consumer must see the
// launch-as-posted context's bytes.  With the option off the recorded stream's launches are today's - the channel kernel's; with it on a
// tick is one "fused_v210_trans_multi x<outputs>" launch.
// usage: node fused_trans_run.js [width=384] [height=6]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '6')
const TICKS = [{ kind: 'dissolve', mix: 0.375 }, { kind: 'wipe', mask: 'image' }, { kind: 'wipe', mask: 'v210' }]
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

function maskImage(w, h, seed) { // f32 RGBA, red in [0, 1]
	const r = lcg(seed)
	const f = new Float32Array(w * h * 4)
	for (let i = 0; i < f.length; ++i) f[i] = (r() >>> 8) / 16777215
	return Buffer.from(f.buffer)
}

async function side(deferred, options) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, deferred, spinWaitMicros: 100 }, options))
	const s = { rig, deferred, frame: 0, writeAs: {} }
	s.read = await rig.unpack('v210', W, H, '709', '709')
	for (const fmt of ['v210', 'bgra8']) s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	s.combine = await rig.combine(2, W, H)
	s.dissolve = await rig.two('transition_dissolve', W, H)
	s.wipe = await rig.two('transition_wipe', W, H)
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
	// the chain up to the combined image: a plain layer under a layer in the tick's transition
	s.combined = async (seed, tick) => {
		const a = await s.source(seed), b = await s.source(seed + 50), c = await s.source(seed + 90)
		const ua = await rig.image(W, H), ub = await rig.image(W, H), uc = await rig.image(W, H), mixed = await rig.image(W, H), comb = await rig.image(W, H)
		rig.post(s.id('A'), s.read([a], ua), () => a.release())
		rig.post(s.id('B'), s.read([b], ub), () => b.release())
		rig.post(s.id('C'), s.read([c], uc), () => c.release())
		if (tick.kind === 'dissolve') {
			rig.post(s.id('mix'), s.dissolve(ub, uc, tick.mix, mixed), () => [ub, uc].forEach((x) => x.release()))
		} else {
			const mask = await rig.image(W, H)
			if (tick.mask === 'image') {
				await rig.upload(mask, maskImage(W, H, seed + 400))
			} else {
				const m = await s.source(seed + 130)
				rig.post(s.id('M'), s.read([m], mask), () => m.release())
			}
			rig.post(s.id('mix'), s.wipe(ub, uc, mask, mixed), () => [ub, uc, mask].forEach((x) => x.release()))
		}
		rig.post(s.id('mix'), s.combine([ua, mixed], comb), () => [ua, mixed].forEach((x) => x.release()))
		return comb
	}
	return s
}

// one tick per transition of one channel with these consumers, on one context; returns what the consumers saw, the traced routes and the counters
async function run(deferred, options, list) {
	const s = await side(deferred, options)
	const seen = []
	const routes = []
	try {
		for (let t = 0; t < TICKS.length; ++t) {
			const comb = await s.combined(100 + t, TICKS[t])
			const outs = []
			for (const fmt of list) outs.push(await s.planes(fmt))
			if (deferred) s.rig.ctx.traceBegin(false)
			list.forEach((fmt, i) => s.rig.post(s.id('mix'), s.writeAs[fmt](comb, outs[i], 0), i === list.length - 1 ? () => comb.release() : () => {}))
			for (const k of ['A', 'B', 'C', 'M', 'mix']) if (s.rig.board.peek(s.id(k))) await s.flush(s.id(k))
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
	const on = await run(true, { fusedTransitions: true }, list)
	for (const [what, got] of [['fusedTransitions off', off], ['fusedTransitions on', on]]) {
		if (got.seen.length !== plain.seen.length || !plain.seen.length) problems.push({ scenario: name, what: `${what}: frames seen ${got.seen.length}, launch-as-posted ${plain.seen.length}` })
		for (let i = 0; i < Math.min(plain.seen.length, got.seen.length); ++i)
			if (Buffer.compare(plain.seen[i], got.seen[i]) !== 0) problems.push({ scenario: name, what: `${what}: plane ${i} differs from the launch-as-posted context's` })
	}
	for (const b of plain.seen) if (b.every((x) => x === 0x5a)) problems.push({ scenario: name, what: 'a frame nobody wrote' })
	if (!off.routes.every((r) => offRoute.test(r))) problems.push({ scenario: name, what: `fusedTransitions off: a tick's launches ${JSON.stringify(off.routes)}` })
	if (!on.routes.every((r) => r === onRoute)) problems.push({ scenario: name, what: `fusedTransitions on: a tick's launches ${JSON.stringify(on.routes)}, ${onRoute} expected` })
	if (on.st && on.st.launched !== TICKS.length) problems.push({ scenario: name, what: `fusedTransitions on: ${on.st.launched} launches, ${TICKS.length} expected` })
	scenarios.push({ name, frames: plain.seen.length, off: off.routes, on: on.routes })
}

async function main() {
	await scenario('v210 alone', ['v210'], /^chan_compose_v210<\d,\d>$/, 'fused_v210_trans_multi x1')
	await scenario('v210 + bgra8', ['v210', 'bgra8'], /^chan_compose_multi<\d>x2$/, 'fused_v210_trans_multi x2')
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
