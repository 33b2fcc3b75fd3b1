'use strict'
// A 720p-wide channel (1280 x 10: every v210 line ends in a tail quad) of a 636 x 4 interlaced source - de-interlaced fields, packed, enlarged
// by the default fill: the 2 x 2-block compositor's frames - with SDI (v210) and the screen (bgra8) as consumers, one tick, on the GPU:
// the plain context, the recording context (node/defer.js) and the recording context with `upTails: true`.  Every consumer must see the
// same bytes on all three; with `upTails` the v210 frames come out of the launch that makes the screen's ("compose_up_multi_t<rgb>x2j2" in
// a trace) and the tick is one kernel fewer than without ("compose_up_write_v210" + "compose_up_multi<rgb>x1j2").
// usage: node up_tails_run.js; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = 1280, H = 10, SW = 636, SH = 4
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

async function tick(name, options, traced) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, spinWaitMicros: 100 }, options))
	const ctx = rig.ctx
	const seen = []
	let route = null
	try {
		const read = await rig.unpack('v210', SW, SH, '709', '709')
		const writeAs = { v210: await rig.pack('v210', W, H, '709', false), bgra8: await rig.pack('bgra8', W, H, '709', false) }
		const transform = await rig.transform(W, H)
		const yadif = await rig.yadif(SW, SH)
		const held = []
		const u = []
		for (let i = 0; i < 3; ++i) {
			const src = (await rig.planes('v210', SW, SH))[0]
			await rig.upload(src, v210Frame(src.length, 900 + i))
			await rig.sync(ctx.queue.load)
			held.push(src)
		}
		const outs = []
		for (const second of [0, 1]) for (const fmt of ['v210', 'bgra8']) {
			const planes = await rig.planes(fmt, W, H, 'readwrite')
			for (const p of planes) await rig.upload(p, Buffer.alloc(p.length, 0x5a))
			outs.push({ second, fmt, planes })
		}
		await rig.sync(ctx.queue.load)
		if (traced) ctx.traceBegin(false)
		try {
			for (const src of held) {
				const im = await rig.image(SW, SH)
				await rig.run(read([src], im))
				u.push(im)
			}
			const fill = await transform.matrix({})
			const placed = []
			for (const second of [0, 1]) {
				const y = await rig.image(SW, SH)
				await rig.run(yadif(u[0], u[1], u[2], y, { parity: second ? 1 : 0, tff: 1, skipSpatial: 0 }))
				const im = await rig.image(W, H)
				await rig.run(transform(y, im, fill))
				y.release()
				placed.push(im)
			}
			for (const o of outs) await rig.run(writeAs[o.fmt](placed[o.second], o.planes, 0))
			placed.forEach((x) => x.release())
			for (const o of outs) for (const p of o.planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		} finally { if (traced) route = ctx.traceEnd() }
		for (const o of outs) o.planes.forEach((p) => p.release())
		;[...held, ...u].forEach((x) => x.release())
		const st = ctx.deferredStats ? ctx.deferredStats() : null
		if (st && (st.unpacked || st.fallbacks)) problems.push({ scenario: name, what: `unpacked ${st.unpacked}, fallbacks ${st.fallbacks}: ${st.lastFallback}` })
	} catch (e) {
		problems.push({ scenario: name, what: String(e && e.stack || e) })
	}
	rig.close()
	const kernels = route === null ? null : String(route).split('+').filter((k) => k.length)
	scenarios.push({ name, frames: seen.length, kernels })
	return { seen, kernels }
}

async function main() {
	const plain = await tick('a plain context', { deferred: false }, false)
	const off = await tick('a recording context', { deferred: true, upWriters: true }, true)
	const on = await tick('a recording context, upTails: true', { deferred: true, upWriters: true, upTails: true }, true)
	if (plain.seen.length !== 4 || plain.seen.some((b) => b.every((x) => x === 0x5a))) problems.push({ what: 'the plain context did not write every frame' })
	for (const [what, got] of [['without upTails', off], ['upTails: true', on]]) {
		if (got.seen.length !== plain.seen.length) problems.push({ scenario: what, what: `frames seen: ${got.seen.length}, ${plain.seen.length} expected` })
		for (let i = 0; i < Math.min(got.seen.length, plain.seen.length); ++i)
			if (Buffer.compare(got.seen[i], plain.seen[i]) !== 0) problems.push({ scenario: what, what: `frame ${i} differs from the plain context's` })
	}
	const k0 = off.kernels || [], k1 = on.kernels || []
	if (!(k1.length === k0.length - 1)) problems.push({ what: `kernels per tick: ${k1.length} with upTails, ${k0.length} without`, with: k1, without: k0 })
	if (!k1.includes('compose_up_multi_t<rgb>x2j2') || k1.includes('compose_up_write_v210')) problems.push({ what: 'upTails: the v210 frames are not in the several-outputs launch', kernels: k1 })
	if (!k0.includes('compose_up_write_v210') || !k0.includes('compose_up_multi<rgb>x1j2') || k0.some((k) => k.includes('_t<'))) problems.push({ what: 'without upTails: not today\'s launches', kernels: k0 })
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
