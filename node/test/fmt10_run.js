'use strict'
// The 10-bit 4:2:0 decoder frames (yuv420p10le, p010le) through the recording context (node/defer.js) against the plain one, on the GPU.
// Readers made by tag ('phaneron:yuv420p10', 'phaneron:p010'): a clip read, placed and combined over a v210 background must give the
// same v210 bytes on both sides, and the recording side must make it with as many launches as for the 8-bit 4:2:0 formats (yuv420p,
// nv12: the channel kernel's planar sources).  A 10-bit 4:2:0 WRITE job and a Yadif window of 10-bit 4:2:0 frames have no fused form:
// they run as recorded (more launches than the 8-bit twins), with the same bytes.
// usage: node fmt10_run.js [width=384] [height=108]; prints one JSON object { scenarios: [...], problems: [...] }
const { Rig } = require('../device.js')

const W = parseInt(process.argv[2] || '384')
const H = parseInt(process.argv[3] || '108')
const problems = []
const scenarios = []
const TWIN = { yuv420p10: 'yuv420p', p010: 'nv12' }

function lcg(seed) { let s = seed >>> 0; return () => (s = (Math.imul(s, 1664525) + 1013904223) >>> 0) }
function v210Frame(bytes, seed) {
	const r = lcg(seed)
	const b = Buffer.alloc(bytes)
	const code = () => 64 + (r() >>> 8) % 877
	for (let i = 0; i + 4 <= bytes; i += 4) b.writeUInt32LE((code() | (code() << 10) | (code() << 20)) >>> 0, i)
	return b
}

async function side(deferred) {
	const rig = await Rig.open({ deviceIndex: 0, deferred, spinWaitMicros: 100 })
	const s = { rig, deferred, frame: 0, readAs: {}, writeAs: {} }
	s.read = await rig.unpack('v210', W, H, '709', '709')
	for (const fmt of ['yuv420p', 'nv12', 'yuv420p10', 'p010']) {
		s.readAs[fmt] = await rig.unpack(fmt, W, H, '709', '709')
		s.writeAs[fmt] = await rig.pack(fmt, W, H, '709', false)
	}
	s.write = await rig.pack('v210', W, H, '709', false)
	s.combine = await rig.combine(2, W, H)
	s.transform = await rig.transform(W, H)
	s.yadif = await rig.yadif(W, H)
	s.source = async (seed) => {
		const p = (await rig.planes('v210', W, H))[0]
		await rig.upload(p, v210Frame(p.length, seed))
		await rig.sync(rig.ctx.queue.load)
		return p
	}
	// a decoder's frame: 16-bit words with every bit set at random (10-bit formats: codes above 1023, p010: low bits), or random bytes
	s.sourcePlanar = async (fmt, seed) => {
		const planes = await rig.planes(fmt, W, H)
		const r = lcg(seed)
		for (const p of planes) {
			const b = Buffer.alloc(p.length)
			for (let i = 0; i < b.length; ++i) b[i] = (r() >>> 8) & 255
			await rig.upload(p, b)
		}
		await rig.sync(rig.ctx.queue.load)
		return planes
	}
	s.id = (name) => ({ source: name, timestamp: s.frame })
	s.flush = (id) => rig.board.flush(id)
	s.consume = async (out) => { await rig.sync(); await rig.download(out); return Buffer.from(out) }
	return s
}

// fn(side) -> the Buffers a consumer saw, on both sides; returns the recording side's counters
async function scenario(name, fn) {
	const got = []
	let st = null
	for (const deferred of [false, true]) {
		const s = await side(deferred)
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

const PIP = { scaleX: 0.5, scaleY: 0.5, offsetX: 0.25, offsetY: -0.25 }

async function main() {
	// a clip (a decoder's frame) placed over a v210 background, written as v210: the channel kernel's planar sources
	const clip = async (fmt) => scenario(`clip ${fmt} over v210`, async (s) => {
		const seen = []
		for (let f = 0; f < 2; ++f) {
			const a = await s.source(100 + f)
			const b = await s.sourcePlanar(fmt, 200 + f)
			const ua = await s.rig.image(W, H), ub = await s.rig.image(W, H), pb = await s.rig.image(W, H), comb = await s.rig.image(W, H)
			s.rig.post(s.id('A'), s.read([a], ua), () => a.release())
			s.rig.post(s.id('B'), s.readAs[fmt](b, ub), () => b.forEach((p) => p.release()))
			s.rig.post(s.id('B'), s.transform(ub, pb, await s.transform.matrix(PIP)), () => ub.release())
			s.rig.post(s.id('mix'), s.combine([ua, pb], comb), () => [ua, pb].forEach((x) => x.release()))
			const out = (await s.rig.planes('v210', W, H, 'writeonly'))[0]
			s.rig.post(s.id('mix'), s.write(comb, [out], 0), () => comb.release())
			for (const k of ['A', 'B', 'mix']) await s.flush(s.id(k))
			seen.push(await s.consume(out))
			out.release()
			s.frame++
		}
		return seen
	})
	// a channel whose consumer takes a 4:2:0 frame: the 10-bit Writers have no fused form
	const write = async (fmt) => scenario(`write ${fmt}`, async (s) => {
		const a = await s.source(300)
		const ua = await s.rig.image(W, H), pa = await s.rig.image(W, H)
		s.rig.post(s.id('A'), s.read([a], ua), () => a.release())
		s.rig.post(s.id('A'), s.transform(ua, pa, await s.transform.matrix(PIP)), () => ua.release())
		const out = await s.rig.planes(fmt, W, H, 'writeonly')
		s.rig.post(s.id('A'), s.writeAs[fmt](pa, out, 0), () => pa.release())
		await s.flush(s.id('A'))
		const seen = []
		for (const p of out) { seen.push(await s.consume(p)); p.release() }
		return seen
	})
	// an interlaced file: a window of three frames, both fields de-interlaced, placed over a v210 background
	const window = async (fmt) => scenario(`yadif window ${fmt}`, async (s) => {
		const win = [], u = []
		for (let i = 0; i < 3; ++i) {
			const planes = await s.sourcePlanar(fmt, 400 + i)
			const im = await s.rig.image(W, H)
			await s.rig.run(s.readAs[fmt](planes, im))
			win.push(planes)
			u.push(im)
		}
		const bg = await s.source(410)
		const ubg = await s.rig.image(W, H)
		await s.rig.run(s.read([bg], ubg))
		const seen = []
		const fields = []
		for (const parity of [0, 1]) { // (both fields of the window, as the Yadif valve posts them: yadif.ts:100-145)
			const y = await s.rig.image(W, H)
			await s.rig.run(s.yadif(u[0], u[1], u[2], y, { parity, tff: 1, skipSpatial: 0 }))
			fields.push(y)
		}
		for (const y of fields) {
			const py = await s.rig.image(W, H), comb = await s.rig.image(W, H)
			await s.rig.run(s.transform(y, py, await s.transform.matrix({ scaleX: 0.6, scaleY: 0.6, offsetX: 0.1 })))
			await s.rig.run(s.combine([ubg, py], comb))
			const out = (await s.rig.planes('v210', W, H, 'writeonly'))[0]
			await s.rig.run(s.write(comb, [out], 0))
			;[y, py, comb].forEach((x) => x.release())
			seen.push(await s.consume(out))
			out.release()
		}
		;[...win.flat(), ...u, bg, ubg].forEach((x) => x.release())
		return seen
	})
	for (const fmt of ['yuv420p10', 'p010']) {
		const twin = TWIN[fmt]
		const [c10, c8] = [await clip(fmt), await clip(twin)]
		if (!(c10.fused > 0) || c10.launched !== c8.launched || c10.fused !== c8.fused)
			problems.push({ what: `clip ${fmt}: ${c10.launched} launches (${c10.fused} fused), ${twin}: ${c8.launched} (${c8.fused} fused)` })
		const [w10, w8] = [await write(fmt), await write(twin)]
		if (w10.fused !== 0 || !(w10.launched > w8.launched))
			problems.push({ what: `write ${fmt}: ${w10.launched} launches (${w10.fused} fused), ${twin}: ${w8.launched} (${w8.fused} fused) - expected separate launches` })
		const [y10, y8] = [await window(fmt), await window(twin)]
		if (!(y10.launched >= y8.launched) || !(y10.launched >= 7)) // (3 reads, 2 yadif, 2 compositor launches at the least)
			problems.push({ what: `yadif window ${fmt}: ${y10.launched} launches, ${twin}: ${y8.launched} - expected the separate kernels` })
	}
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
