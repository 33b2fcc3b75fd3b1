'use strict'
// A 1080i-source channel in a transition (de-interlaced fields, enlarged by the default fill; an inset layer dissolving to another
// source, then wiping to it under a mask image) through the recording context (node/defer.js) against the plain one, on the GPU.
// Every frame must be the same bytes on both sides and whatever the options say.  With `upTransitions: true` the frames come out of
// compose_up_trans_<n> (ph_compose_up_transition_multi) - a dissolve between two field sources from the PACKED fields, no rgb_unpack;
// with the option off the recorded stream launches what it launches without this route (the channel kernel).
// usage: node up_trans_run.js [width=384] [height=108]; prints one JSON object { scenarios: [...], problems: [...] }
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
function maskImage(w, h, seed) { // f32 RGBA, red in [0, 1]
	const r = lcg(seed)
	const f = new Float32Array(w * h * 4)
	for (let i = 0; i < f.length; ++i) f[i] = (r() >>> 8) / 16777215
	return Buffer.from(f.buffer)
}

async function side(deferred, options) {
	const rig = await Rig.open(Object.assign({ deviceIndex: 0, deferred, spinWaitMicros: 100 }, options))
	const s = { rig, deferred }
	s.read = { 2: await rig.unpack('v210', W / 2, H / 2, '709', '709'), 4: await rig.unpack('v210', W / 4, H / 4, '709', '709') }
	s.write = await rig.pack('v210', W, H, '709', false)
	s.transform = await rig.transform(W, H)
	s.yadif = { 2: await rig.yadif(W / 2, H / 2), 4: await rig.yadif(W / 4, H / 4) }
	s.combine = await rig.combine(2, W, H)
	s.dissolve = await rig.two('transition_dissolve', W, H)
	s.wipe = await rig.two('transition_wipe', W, H)
	s.frame = async () => {
		const planes = await rig.planes('v210', W, H, 'readwrite')
		for (const p of planes) await rig.upload(p, Buffer.alloc(p.length, 0x5a))
		await rig.sync(rig.ctx.queue.load)
		return planes
	}
	s.consume = async (planes) => {
		const seen = []
		for (const p of planes) { await rig.sync(); await rig.download(p); seen.push(Buffer.from(p)) }
		return seen
	}
	// a source's tick: a window of three frames of 1 / div the channel's size, both de-interlaced fields, each placed (div 2: enlarged 2 x by
	// the default fill; div 4: 2 x as an inset of half the frame)
	s.fields = async (seed, placement, div) => {
		const w = W / div, h = H / div
		const held = []
		const u = []
		for (let i = 0; i < 3; ++i) {
			const src = (await rig.planes('v210', w, h))[0]
			await rig.upload(src, v210Frame(src.length, seed + i))
			await rig.sync(rig.ctx.queue.load)
			const im = await rig.image(w, h)
			await rig.run(s.read[div]([src], im))
			held.push(src, im)
			u.push(im)
		}
		const matrix = await s.transform.matrix(placement)
		const placed = []
		for (const second of [0, 1]) {
			const y = await rig.image(w, h)
			await rig.run(s.yadif[div](u[0], u[1], u[2], y, { parity: second ? 1 : 0, tff: 1, skipSpatial: 0 }))
			const im = await rig.image(W, H)
			await rig.run(s.transform(y, im, matrix))
			y.release()
			placed.push(im)
		}
		held.forEach((x) => x.release())
		return placed
	}
	return s
}

// ticks of the channel: a full-frame source under an inset layer that dissolves (two ticks, a mix per field), then wipes (one tick), to another source
async function stream(s) {
	const inset = { scaleX: 0.5, scaleY: 0.5, offsetX: 0.2, offsetY: -0.15 }
	const seen = []
	const ticks = [{ kind: 'dissolve', mix: [0.25, 0.3] }, { kind: 'dissolve', mix: [0.75, 0.8] }, { kind: 'wipe' }]
	for (let t = 0; t < ticks.length; ++t) {
		const below = await s.fields(100 + 10 * t, {}, 2)
		const going = await s.fields(200 + 10 * t, inset, 4)
		const coming = await s.fields(300 + 10 * t, inset, 4)
		let mask = null
		if (ticks[t].kind === 'wipe') {
			const raw = await s.rig.image(W, H)
			await s.rig.upload(raw, maskImage(W, H, 400 + t))
			mask = await s.rig.image(W, H)
			await s.rig.run(s.transform(raw, mask, await s.transform.matrix({})))
			raw.release()
		}
		const outs = []
		for (const second of [0, 1]) {
			const mixed = await s.rig.image(W, H)
			if (mask) await s.rig.run(s.wipe(going[second], coming[second], mask, mixed))
			else await s.rig.run(s.dissolve(going[second], coming[second], ticks[t].mix[second], mixed))
			const all = await s.rig.image(W, H)
			await s.rig.run(s.combine([below[second], mixed], all))
			const planes = await s.frame()
			await s.rig.run(s.write(all, planes, 0))
			mixed.release(); all.release()
			outs.push(planes)
		}
		;[...below, ...going, ...coming].forEach((x) => x.release())
		if (mask) mask.release()
		for (const planes of outs) { seen.push(...await s.consume(planes)); planes.forEach((p) => p.release()) }
	}
	return seen
}

async function scenario(name, options) {
	const got = []
	let st = null
	let programs = []
	for (const deferred of [false, true]) {
		const s = await side(deferred, options)
		try {
			got.push(await stream(s))
			if (deferred) {
				st = s.rig.ctx.deferredStats()
				programs = [...new Set([...s.rig.ctx._deferral.programs.values()].map((p) => p.name))].sort()
			}
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
	scenarios.push({ name, frames: plain.length, deferred: st, programs, plain })
	return { st: st || {}, programs }
}

async function main() {
	const on = await scenario('upTransitions: true', { upTransitions: true })
	if (!on.programs.includes('compose_up_trans_2')) problems.push({ scenario: 'upTransitions: true', what: `no compose_up_trans_2 among ${on.programs}` })
	if (on.programs.some((n) => n.startsWith('chan_compose_'))) problems.push({ scenario: 'upTransitions: true', what: `the channel kernel ran: ${on.programs}` })
	if (on.programs.includes('rgb_unpack') && !(on.st.unpacked <= 4)) problems.push({ scenario: 'upTransitions: true', what: `unpacked ${on.st.unpacked}: only the wipe tick's fields (its mask is no field) may be` })
	if (on.st.fallbacks) problems.push({ scenario: 'upTransitions: true', what: `fallbacks ${on.st.fallbacks}: ${on.st.lastFallback}` })
	const off = await scenario('upTransitions: false', { upTransitions: false })
	const dflt = await scenario('the default', {})
	for (const [name, r] of [['upTransitions: false', off], ['the default', dflt]]) {
		if (r.programs.some((n) => n.startsWith('compose_up_trans_'))) problems.push({ scenario: name, what: `compose_up_trans ran: ${r.programs}` })
		if (!r.programs.some((n) => n.startsWith('chan_compose_v210_'))) problems.push({ scenario: name, what: `the channel kernel did not run: ${r.programs}` })
	}
	if (JSON.stringify(off.programs) !== JSON.stringify(dflt.programs) || off.st.launched !== dflt.st.launched)
		problems.push({ scenario: 'the default', what: `differs from upTransitions: false: ${dflt.programs} (${dflt.st.launched} launches) against ${off.programs} (${off.st.launched})` })
	// the same frames whatever the option says
	const frames = scenarios.map((s) => s.plain)
	for (let k = 1; k < frames.length; ++k)
		for (let i = 0; i < frames[0].length; ++i)
			if (!frames[k][i] || Buffer.compare(frames[0][i], frames[k][i]) !== 0) problems.push({ scenario: scenarios[k].name, what: `frame ${i} differs from the first scenario's` })
	for (const s of scenarios) delete s.plain
}

main().then(() => {
	console.log(JSON.stringify({ scenarios, problems }))
	process.exit(0)
}, (e) => {
	for (const s of scenarios) delete s.plain
	console.log(JSON.stringify({ scenarios, problems: problems.concat([{ what: String(e && e.stack || e) }]) }))
	process.exit(1)
})
