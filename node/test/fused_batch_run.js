'use strict'
// Four channels in one context (src/index.ts:45-71), each a headline-shaped frame - two plain v210 layers of the output's size, combine_2 -
// for SDI (v210) and the screen (bgra8), through the recording context (node/defer.js) with `fusedWriters` against the launch-as-posted
// one, on the GPU.  Every consumer must see the same bytes on both sides.  With `fusedBatch: true` the eight frames of a tick come out
// of ONE launch (runPrograms -> ph_fused_v210_combine_multi_batch: "fused_v210_combine_multi x2j4" in a trace); without it every
// channel's "fused_v210_combine_multi x2" launch is made in its turn, as before.
// usage: node fused_batch_run.js [width=384] [height=12]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '12')
const TICKS = 2
const CHANNELS = [['v210', 'bgra8'], ['v210', 'bgra8'], ['v210', 'bgra8'], ['v210', 'bgra8']]
const PLANES = TICKS * CHANNELS.reduce((n, list) => n + list.reduce((m, fmt) => m + (fmt === 'yuv422p8' ? 3 : 1), 0), 0)
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
	s.consume = async (planes) => {
		const seen = []
		for (const p of planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		return seen
	}
	// a channel's chain up to its combined image, the headline's: two plain v210 layers of the output's size
	s.combined = async (id, seed) => {
		const a = await s.source(seed), b = await s.source(seed + 50)
		const ua = await rig.image(W, H), ub = await rig.image(W, H), comb = await rig.image(W, H)
		rig.post(id, s.read([a], ua), () => a.release())
		rig.post(id, s.read([b], ub), () => b.release())
		rig.post(id, s.combine([ua, ub], comb), () => [ua, ub].forEach((x) => x.release()))
		return comb
	}
	return s
}

// TICKS ticks of the four channels, every channel's frames posted before any is asked for; returns what the consumers saw and,
// on the recording side, the kernels of every tick
async function ticks(s) {
	const seen = []
	const routes = []
	for (let t = 0; t < TICKS; ++t) {
		const outs = []
		const ids = []
		for (let c = 0; c < CHANNELS.length; ++c) {
			const id = { source: `chan${c}`, timestamp: s.frame }
			const comb = await s.combined(id, 100 + 10 * c + t)
			const mine = []
			for (const fmt of CHANNELS[c]) mine.push(await s.planes(fmt))
			CHANNELS[c].forEach((fmt, i) => s.rig.post(id, s.writeAs[fmt](comb, mine[i], 0), i === CHANNELS[c].length - 1 ? () => comb.release() : () => {}))
			outs.push(...mine)
			ids.push(id)
		}
		if (s.deferred) s.rig.ctx.traceBegin(false)
		await Promise.all(ids.map((id) => s.rig.board.flush(id)))
		for (const planes of outs) { seen.push(...await s.consume(planes)); planes.forEach((p) => p.release()) }
		if (s.deferred) routes.push(s.rig.ctx.traceEnd())
		s.frame++
	}
	return { seen, routes }
}

async function scenario(name, options) {
	const got = []
	let st = null
	let routes = []
	for (const deferred of [false, true]) {
		try {
			const s = await side(deferred, options)
			const r = await ticks(s)
			got.push(r.seen)
			if (deferred) { st = s.rig.ctx.deferredStats(); routes = r.routes }
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
	if (plain.length !== lazy.length || plain.length !== PLANES) problems.push({ scenario: name, what: `planes seen: plain ${plain.length}, deferred ${lazy.length}, ${PLANES} expected` })
	for (let i = 0; i < Math.min(plain.length, lazy.length); ++i)
		if (Buffer.compare(plain[i], lazy[i]) !== 0) problems.push({ scenario: name, what: `plane ${i} differs between the plain and the recording context` })
	scenarios.push({ name, planes: plain.length, deferred: st, routes })
	return { st: st || {}, routes }
}

async function main() {
	// both options on: one runPrograms call and one launch per tick, every sibling write folded
	let r = await scenario('fusedBatch: true', { fusedWriters: true, fusedBatch: true })
	if (r.st.launched !== TICKS || r.st.batched !== 4 * TICKS || r.st.multiOutputs !== 4 * TICKS) problems.push({ scenario: 'fusedBatch: true', what: `counters ${JSON.stringify(r.st)}` })
	for (const route of r.routes) if (route !== 'fused_v210_combine_multi x2j4') problems.push({ scenario: 'fusedBatch: true', what: `a tick's launches: ${route}` })
	// fusedWriters alone: every channel's several-outputs launch in its turn, as before
	r = await scenario('fusedBatch off (the default)', { fusedWriters: true })
	if (r.st.launched !== 4 * TICKS || r.st.multiOutputs !== 4 * TICKS || r.st.batched) problems.push({ scenario: 'fusedBatch off', what: `counters ${JSON.stringify(r.st)}` })
	for (const route of r.routes) if (route !== Array(4).fill('fused_v210_combine_multi x2').join('+')) problems.push({ scenario: 'fusedBatch off', what: `a tick's launches: ${route}` })
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
