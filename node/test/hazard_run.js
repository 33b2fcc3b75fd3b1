'use strict'
// The packed-field hazards of the recording context (node/defer.js), on the GPU through the real addon: the directed scenarios of
// packed_state_check.js - a compositor frame planned on packed de-interlaced fields and, inside the same _runMany, a plain consumer of
// the same field (or of the twin's field) whose launch unpacks it - at 192 x 54 fields on a 384 x 108 channel, through
// `new clContext({deferred: true})` and through the launch-as-posted context: every frame a consumer sees must be the same bytes.
// Then runProgramsProgress() after a runPrograms call that throws at marshalling (a bad program handle): 0, not the call before's count.
// Prints one JSON object { scenarios, frames, unpacked, progress, problems }.
const { Rig } = require('../device.js')

const W = 384, H = 108, FW = 192, FH = 54
const problems = []
let scenarios = 0
let frames = 0
let unpacked = 0

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
	const s = { rig, deferred }
	s.read = await rig.unpack('v210', W, H, '709', '709')
	s.readField = await rig.unpack('v210', FW, FH, '709', '709')
	s.write = await rig.pack('v210', W, H, '709', false)
	s.writeField = await rig.pack('v210', FW, FH, '709', false)
	s.transform = await rig.transform(W, H)
	s.resize = await rig.resize(FW, FH)
	s.yadif = await rig.yadif(FW, FH)
	s.source = async (bytes, w, h) => {
		const p = await rig.planes('v210', w, h)
		await rig.upload(p[0], bytes)
		await rig.sync(rig.ctx.queue.load)
		return p[0]
	}
	s.consume = async (out) => { await rig.sync(); await rig.download(out); return Buffer.from(out) }
	return s
}

// which: 'own' - one field's frame and a consumer of that field; 'twin' - both fields' frames (one launch: the second is the first's twin)
// and a consumer of the second field.  order: whose jobs are posted first.
async function packedField(s, which, order) {
	const fieldBytes = (await s.rig.planes('v210', FW, FH))
	const bytes = fieldBytes[0].length
	fieldBytes[0].release()
	const held = []
	const u = []
	for (let i = 0; i < 3; ++i) {
		const src = await s.source(v210Frame(bytes, 4100 + i), FW, FH)
		const im = await s.rig.image(FW, FH)
		await s.rig.run(s.readField([src], im))
		held.push(src, im)
		u.push(im)
	}
	const fill = await s.transform.matrix({})
	const y = []
	for (const parity of [0, 1]) {
		const f = await s.rig.image(FW, FH)
		await s.rig.run(s.yadif(u[0], u[1], u[2], f, { parity, tff: 1, skipSpatial: 0 }))
		y.push(f)
	}
	const outs = []
	const compositor = async () => {
		for (const parity of which === 'twin' ? [0, 1] : [0]) {
			const im = await s.rig.image(W, H)
			await s.rig.run(s.transform(y[parity], im, fill))
			const out = (await s.rig.planes('v210', W, H, 'writeonly'))[0]
			await s.rig.run(s.write(im, [out], 0))
			im.release()
			outs.push(out)
		}
	}
	let shown = null
	const consumer = async () => { // somebody who is not the compositor shows the field: a program the recording does not fold, then its own frame
		const z = await s.rig.image(FW, FH)
		await s.rig.run(await s.resize(y[which === 'twin' ? 1 : 0], z, { scale: 0.75, offsetX: 0.1 }))
		shown = (await s.rig.planes('v210', FW, FH, 'writeonly'))[0]
		await s.rig.run(s.writeField(z, [shown], 0))
		z.release()
	}
	if (order === 'compositor first') { await compositor(); await consumer() } else { await consumer(); await compositor() }
	const seen = []
	for (const out of outs) { seen.push(await s.consume(out)); out.release() } // (the first one asked for takes the tick's other frames with it)
	seen.push(await s.consume(shown))
	shown.release()
	for (const f of y) { seen.push(await s.consume(f)); f.release() } // the application looks at the fields themselves, too
	held.forEach((x) => x.release())
	return seen
}

async function scenario(name, fn, env) {
	const got = []
	for (const deferred of [false, true]) {
		const old = {}
		for (const k of Object.keys(env || {})) { old[k] = process.env[k]; process.env[k] = env[k] }
		let s = null
		try {
			s = await side(deferred)
			got.push(await fn(s))
			if (deferred) unpacked += s.rig.ctx.deferredStats().unpacked || 0
			s.rig.close()
			const left = s.rig.ctx.flushDeferred()
			const live = s.rig.ctx.bufferStats()
			if (deferred && left && left.pending) problems.push({ scenario: name, what: `${left.pending} recorded jobs are still pending after everything was released` })
			if (live.liveBuffers !== 0) problems.push({ scenario: name, what: `${live.liveBuffers} buffers still alive on the ${deferred ? 'deferred' : 'plain'} side` })
		} catch (e) {
			problems.push({ scenario: name, what: `${deferred ? 'deferred' : 'plain'} side: ${e && e.stack || e}` })
			got.push([])
		}
		for (const k of Object.keys(old)) { if (old[k] === undefined) delete process.env[k]; else process.env[k] = old[k] }
	}
	const [plain, lazy] = got
	if (plain.length !== lazy.length || !plain.length) problems.push({ scenario: name, what: `frames seen: plain ${plain.length}, deferred ${lazy.length}` })
	for (let i = 0; i < Math.min(plain.length, lazy.length); ++i)
		if (Buffer.compare(plain[i], lazy[i]) !== 0) {
			let at = 0, n = 0
			while (at < plain[i].length && plain[i][at] === lazy[i][at]) ++at
			for (let k = at; k < plain[i].length; ++k) if (plain[i][k] !== lazy[i][k]) ++n
			problems.push({ scenario: name, what: `frame ${i} differs from byte ${at} of ${plain[i].length}`, differing: n })
		}
	++scenarios
	frames += plain.length
}

// runProgramsProgress() behind a call that went through and behind one that never reached the library
async function progress() {
	const s = await side(true)
	const native = s.rig.ctx._native
	const result = { afterBatch: null, afterThrow: null }
	const bytes = (await s.rig.planes('v210', W, H))
	const n = bytes[0].length
	bytes[0].release()
	const held = []
	const outs = []
	for (let c = 0; c < 2; ++c) { // two channels of plain reads posted in one tick: one runPrograms call of two jobs
		const src = await s.source(v210Frame(n, 4200 + c), W, H)
		const im = await s.rig.image(W, H)
		await s.rig.run(s.read([src], im))
		const out = (await s.rig.planes('v210', W, H, 'writeonly'))[0]
		await s.rig.run(s.write(im, [out], 0))
		held.push(src, im)
		outs.push(out)
	}
	for (const out of outs) await s.consume(out)
	result.afterBatch = native.runProgramsProgress()
	if ((s.rig.ctx.deferredStats().batched || 0) !== 2) problems.push({ scenario: 'progress', what: 'the two frames did not go down in one runPrograms call', stats: s.rig.ctx.deferredStats() })
	let threw = null
	try { native.runPrograms(s.rig.ctx._ctx, [{}], [[]], [[]], s.rig.ctx.queue.process) } catch (e) { threw = String(e && e.message || e) }
	if (!threw || !/bad program/.test(threw)) problems.push({ scenario: 'progress', what: `runPrograms with a bad program handle: ${threw}` })
	result.afterThrow = native.runProgramsProgress()
	;[...held, ...outs].forEach((x) => x.release())
	s.rig.close()
	s.rig.ctx.flushDeferred()
	return result
}

;(async () => {
	for (const which of ['own', 'twin']) for (const order of ['compositor first', 'consumer first'])
		await scenario(`${which} field, ${order}`, (s) => packedField(s, which, order), which === 'twin' ? { PHANERON_FIELD_BATCH: '1' } : null)
	let p = null
	try { p = await progress() } catch (e) { problems.push({ scenario: 'progress', what: String(e && e.stack || e) }) }
	process.stdout.write(JSON.stringify({ scenarios, frames, unpacked, progress: p, problems }) + '\n')
})()
