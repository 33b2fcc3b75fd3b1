'use strict'
// Consumers of a 1080i-source channel (de-interlaced fields, enlarged by the default fill: the 2 x 2-block compositor's frames) through
// the recording context (node/defer.js) against the plain one, on the GPU.  Every consumer must see the same bytes on both sides; on
// the recording side a consumer that is not SDI, and several consumers at once, get their frames from ONE launch of
// compose_up_multi_<n> per tick (both fields of the tick in it) - unless the context says `upWriters: false`, a sibling write is
// posted after the first frame was asked for, or the launch is refused (then today's launches make the frames).
// usage: node up_out_run.js [width=384] [height=108]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '108')
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
	const s = { rig, deferred, writeAs: {} }
	s.readHalf = await rig.unpack('v210', W / 2, H / 2, '709', '709')
	for (const fmt of ['v210', 'yuv422p8', 'yuv420p', 'rgba8', 'bgra8']) s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	s.transform = await rig.transform(W, H)
	s.yadifHalf = await rig.yadif(W / 2, H / 2)
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
	// a tick: a window of three half-size frames, both de-interlaced fields, each enlarged 2 x by the default fill
	s.fields = async (seed) => {
		const held = []
		const u = []
		for (let i = 0; i < 3; ++i) {
			const src = (await rig.planes('v210', W / 2, H / 2))[0]
			await rig.upload(src, v210Frame(src.length, seed + i))
			await rig.sync(rig.ctx.queue.load)
			const im = await rig.image(W / 2, H / 2)
			await rig.run(s.readHalf([src], im))
			held.push(src, im)
			u.push(im)
		}
		const fill = await s.transform.matrix({})
		const placed = []
		for (const second of [0, 1]) {
			const y = await rig.image(W / 2, H / 2)
			await rig.run(s.yadifHalf(u[0], u[1], u[2], y, { parity: second ? 1 : 0, tff: 1, skipSpatial: 0 }))
			const im = await rig.image(W, H)
			await rig.run(s.transform(y, im, fill))
			y.release()
			placed.push(im)
		}
		held.forEach((x) => x.release())
		return placed
	}
	return s
}

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

// one tick of the channel with these consumers, each writing both fields' frames
const consumers = (list) => async (s) => {
	const placed = await s.fields(700)
	const outs = []
	for (const second of [0, 1]) for (const fmt of list) outs.push({ second, fmt, planes: await s.planes(fmt) })
	for (const o of outs) await s.rig.run(s.writeAs[o.fmt](placed[o.second], o.planes, 0))
	placed.forEach((x) => x.release())
	const seen = []
	for (const o of outs) { seen.push(...await s.consume(o.planes)); o.planes.forEach((p) => p.release()) }
	return seen
}

// launches: the reader pair launch + what follows
function expectLaunches(name, st, want) {
	if (st.launched !== want) problems.push({ scenario: name, what: `${st.launched} launches, ${want} expected (${JSON.stringify(st)})` })
}

async function main() {
	let st = await scenario('yuv422p8 alone', consumers(['yuv422p8']), { upWriters: true })
	expectLaunches('yuv422p8 alone', st, 2)
	if (st.unpacked || st.fallbacks) problems.push({ scenario: 'yuv422p8 alone', what: `unpacked ${st.unpacked}, fallbacks ${st.fallbacks}: ${st.lastFallback}` })
	st = await scenario('v210 + bgra8', consumers(['v210', 'bgra8']), { upWriters: true })
	expectLaunches('v210 + bgra8', st, 2)
	if (st.unpacked || st.fallbacks) problems.push({ scenario: 'v210 + bgra8', what: `unpacked ${st.unpacked}, fallbacks ${st.fallbacks}: ${st.lastFallback}` })
	st = await scenario('v210 + yuv420p + rgba8', consumers(['v210', 'yuv420p', 'rgba8']), { upWriters: true })
	expectLaunches('v210 + yuv420p + rgba8', st, 2)
	await scenario('upWriters: false', consumers(['v210', 'bgra8']), { upWriters: false })
	await scenario('the default', consumers(['v210', 'yuv422p8']))
	st = await scenario('a sibling posted late', async (s) => {
		const placed = await s.fields(800)
		const first = await s.planes('v210'), second = await s.planes('bgra8')
		await s.rig.run(s.writeAs.v210(placed[0], first, 0))
		const seen = await s.consume(first)
		await s.rig.run(s.writeAs.bgra8(placed[0], second, 0))
		placed.forEach((x) => x.release())
		seen.push(...await s.consume(second))
		;[...first, ...second].forEach((p) => p.release())
		return seen
	}, { upWriters: true })
	st = await scenario('a refused launch falls back', async (s) => {
		const native = s.rig.ctx._native
		const run = native.runProgram
		const deferral = s.rig.ctx._deferral
		if (deferral) native.runProgram = function (ctx, handle, names, values, queue, profile, checkOnly) {
			let multi = false
			for (const p of deferral.programs.values()) if (p._handle === handle && p.name.startsWith('compose_up_multi_')) multi = true
			if (!multi || checkOnly) return run.apply(this, arguments)
			s.rig.ctx.setOption('fail_launches', 1)
			try { return run.apply(this, arguments) } finally { s.rig.ctx.setOption('fail_launches', 0) }
		}
		try { return await consumers(['v210', 'bgra8'])(s) } finally { native.runProgram = run }
	}, { upWriters: true })
	if (!(st.fallbacks >= 1)) problems.push({ scenario: 'a refused launch falls back', what: `fallbacks ${st.fallbacks}: ${st.lastFallback}` })
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
