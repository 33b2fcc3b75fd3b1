'use strict'
// node/defer.js without a device: is a de-interlaced field that travels as packed f32 RGB (12 bytes per pixel in its RGBA image buffer)
// ever read by somebody who takes it for the image it is declared as - or the other way round?  The counting stand-in of defer_check.js
// (defer_rig.js) with a LAYOUT per buffer handle, `rgba` or `packed`, and these rules at every launch, alone or in a runPrograms call:
//   * the de-interlacing pair program told packedRgb leaves its outputs `packed` (not told: `rgba`)
//   * rgb_unpack needs `packed` and leaves `rgba`
//   * a compose_up_* job with packedRgb = 1 needs every l<i>In / l<i>In2 `packed`, one without needs them `rgba`
//   * any other program that reads a `packed` handle is a problem; whatever a program writes is `rgba` afterwards
// Directed scenarios, then seeded random streams of the same jobs (seed: argv[2], default 1; streams: argv[3], default 300) with and
// without runPrograms, earlyLaunch on and off.  A broken rule gives a garbled frame and no error on a device: here it is a problem.
// Prints one JSON object { checks, problems, streams }.
const { rig } = require('./defer_rig.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

const OUTPUT_ARG = /^(output|twinOutput|l\d+Out)/
// the rig with the layout rules; `where`: what a broken rule is reported under
function layoutRig(opt, where) {
	const r = rig(opt)
	const layout = new Map() // handle -> 'packed' (absent: 'rgba')
	const broken = []
	r.layoutOf = (buf) => layout.get(buf._handle) || 'rgba'
	r.hostWrote = (buf) => layout.delete(buf._handle) // (what the host writes is the image the buffer is declared as)
	r.broken = broken
	r.native.observe = (name, names, values) => {
		const arg = (k) => { const at = names.indexOf(k); return at < 0 ? undefined : values[at] }
		const isBuf = (v) => v && typeof v === 'object'
		const told = !!arg('packedRgb')
		const bad = (k, want) => { const p = { where: where(), what: `${name}: '${k}' is ${want === 'packed' ? 'an RGBA image' : 'packed RGB'}, read as ${want === 'packed' ? 'packed RGB' : 'an RGBA image'}` }; broken.push(p); problems.push(p) }
		if (/^v210_yadif_pair_\d+$/.test(name)) {
			names.forEach((k, i) => { if (/^l\d+Out[01]$/.test(k)) { if (told) layout.set(values[i], 'packed'); else layout.delete(values[i]) } })
			return
		}
		if (name === 'rgb_unpack') {
			if (layout.get(arg('image')) !== 'packed') bad('image', 'packed')
			layout.delete(arg('image'))
			return
		}
		names.forEach((k, i) => {
			if (!isBuf(values[i]) || OUTPUT_ARG.test(k)) return
			const is = layout.get(values[i]) || 'rgba'
			if (/^compose_up_/.test(name) && /^l\d+In2?$/.test(k)) { if (is !== (told ? 'packed' : 'rgba')) bad(k, told ? 'packed' : 'rgba') }
			else if (is === 'packed') bad(k, 'rgba')
		})
		names.forEach((k, i) => { if (isBuf(values[i]) && OUTPUT_ARG.test(k)) layout.delete(values[i]) })
	}
	// a channel showing a de-interlaced source: the window's reads, both fields' yadif, and per field in `fields` transform -> write
	r.channel = (tag, fields, L, m) => {
		const win = [0, 1, 2].map((i) => { const im = r.image(`${tag}w${i}`); r.d.record(r.P.read, Object.assign({ input: r.v210(`${tag}s${i}`), output: im, width: r.W }, L), 1); return im })
		const ch = { y: [], out: [] }
		for (const parity of [0, 1]) {
			const y = r.image(`${tag}y${parity}`)
			r.d.record(r.P.yadif, { prev: win[0], cur: win[1], next: win[2], parity, tff: 1, skipSpatial: 0, output: y }, 1)
			ch.y.push(y)
		}
		for (const parity of fields) {
			const t = r.image(`${tag}t${parity}`)
			r.d.record(r.P.transform, { input: ch.y[parity], transformMatrix: m, output: t }, 1)
			const out = r.v210(`${tag}out${parity}`)
			r.d.record(r.P.write, Object.assign({ input: t, output: out, width: r.W, interlace: 0 }, r.saver), 1)
			ch.out[parity] = out
		}
		return ch
	}
	// somebody who is not the compositor shows a field: resize (a program the recording does not fold) -> write
	r.plainConsumer = (tag, field) => {
		const z = r.image(`${tag}z`)
		r.d.record(r.P.other, { input: field, output: z, scale: 1, offsetX: 0, offsetY: 0, flip: r.flip }, 1)
		const out = r.v210(`${tag}out`)
		r.d.record(r.P.write, Object.assign({ input: z, output: out, width: r.W, interlace: 0 }, r.saver), 1)
		return { z, out }
	}
	// ... without a frame of its own: the reader stays recorded until somebody needs its image, or its operand changes
	r.plainReader = (tag, field) => {
		const z = r.image(`${tag}z`)
		r.d.record(r.P.other, { input: field, output: z, scale: 1, offsetX: 0, offsetY: 0, flip: r.flip }, 1)
		return z
	}
	r.flip = r.buffer(16, undefined, 'flip')
	return r
}
const count = (names, what) => names.filter((n) => n === what || n.split(/[:+]/).includes(what)).length

// 1. a compositor plan on packed fields and a plain consumer of the same field, forced inside the same _runMany: the plan made for packed
// fields is stale once the consumer's launch has unpacked one - in both recording orders, for the frame's own field and for the twin's
// (the frames of a tick are planned first and launched afterwards where they share launches: runPrograms; fieldBatch for the twin's)
for (const batch of [false, true]) for (const which of ['own', 'twin']) for (const order of ['compositor first', 'consumer first']) for (const ask of ['compositor', 'consumer']) {
	const what = `1. ${which} field, ${order}, ${ask}'s frame asked for${batch ? ', runPrograms' : ''}`
	const r = layoutRig({ batch, progress: batch }, () => what)
	r.d.fieldBatch = which === 'twin' // (the default launches a frame's two fields as soon as they are planned: nothing can come in between)
	const L = r.loader()
	const m = r.enlarging()
	let ch, plain
	const fields = which === 'twin' ? [0, 1] : [0]
	if (order === 'compositor first') { ch = r.channel('a', fields, L, m); plain = r.plainConsumer('p', ch.y[which === 'twin' ? 1 : 0]) } else {
		// (the consumer's jobs name the field image before the channel's own jobs do: the images first)
		ch = r.channel('a', [], L, m)
		plain = r.plainConsumer('p', ch.y[which === 'twin' ? 1 : 0])
		for (const parity of fields) {
			const t = r.image(`at${parity}`)
			r.d.record(r.P.transform, { input: ch.y[parity], transformMatrix: m, output: t }, 1)
			const out = r.v210(`aout${parity}`)
			r.d.record(r.P.write, Object.assign({ input: t, output: out, width: r.W, interlace: 0 }, r.saver), 1)
			ch.out[parity] = out
		}
	}
	r.d.touch(ask === 'compositor' ? ch.out[0] : plain.out, 'readonly', 2)
	for (const o of [...fields.map((f) => ch.out[f]), plain.out]) r.d.touch(o, 'readonly', 2)
	expect(`${what}: no field read in the wrong layout`, r.broken, [])
	expect(`${what}: every frame made`, Array.from(r.d.pending).filter((n) => n.program.name === 'write').length, 0)
	expect(`${what}: the consumer's jobs ran as recorded`, [count(r.names(), 'resize'), count(r.names(), 'write')], [1, 1])
}

// 2. a packed field with a pending reader that is not the compositor, overwritten by the host: the reader runs first - on the real image
for (const dir of ['writeonly', 'none']) {
	const what = `2. hostAccess('${dir}') of a packed field somebody still reads`
	const r = layoutRig({}, () => what)
	const ch = r.channel('a', [0, 1], r.loader(), r.enlarging())
	r.d.touch(ch.out[0], 'readonly', 2)
	expect(`${what}: the fields were made packed and stay so behind the compositor`, [r.names(), r.layoutOf(ch.y[0]), r.layoutOf(ch.y[1])], [['v210_yadif_pair_1', 'compose_up_write_v210_1'], 'packed', 'packed'])
	r.plainReader('p', ch.y[0])
	r.d.touch(ch.y[0], dir, 0)
	r.hostWrote(ch.y[0])
	// (the frame's own transform is still recorded - its owner holds the image - and reads the field too)
	expect(`${what}: unpacked, then read`, [r.names().slice(2), r.broken], [['rgb_unpack', 'transform', 'resize'], []])
	expect(`${what}: the buffer is an image again`, [ch.y[0]._packed == null, r.layoutOf(ch.y[0])], [true, 'rgba'])
	r.d.touch(ch.y[1], dir, 0)
	r.hostWrote(ch.y[1])
	expect(`${what}: the other field likewise`, [r.names().slice(5), r.broken, ch.y[1]._packed == null], [['rgb_unpack', 'transform'], [], true])
}

// 3. a runPrograms call that throws while runProgramsProgress could still hold the count of the call before (the stand-in models the addon:
// a call that throws before it reaches the library leaves 0): no frame is retired as made - each is launched on its own
{
	const what = '3. a batch that throws behind one that went through'
	const r = layoutRig({ batch: true, progress: true }, () => what)
	const L = r.loader()
	const tick = () => [0, 1].map((c) => {
		const u = r.image(`u${c}`)
		r.d.record(r.P.read, Object.assign({ input: r.v210(`s${c}`), output: u, width: r.W }, L), 1)
		const out = r.v210(`out${c}`)
		r.d.record(r.P.write, Object.assign({ input: u, output: out, width: r.W, interlace: 0 }, r.saver), 1)
		return out
	})
	let outs = tick()
	r.d.touch(outs[0], 'readonly', 2)
	expect(`${what}: the first tick's frames in one call`, [r.names(), r.native.runProgramsProgress()], [['batch:fused_v210_combine_1+fused_v210_combine_1'], 2])
	outs = tick()
	r.native.refuse = (name) => name === 'batch'
	r.d.touch(outs[0], 'readonly', 2)
	r.native.refuse = null
	expect(`${what}: nothing counted as made by the call that threw`, [r.native.runProgramsProgress(), r.d.stats.batched], [0, 2])
	expect(`${what}: both frames launched on their own`, r.names().slice(1), ['fused_v210_combine_1', 'fused_v210_combine_1'])
	expect(`${what}: no write left`, Array.from(r.d.pending).filter((n) => n.program.name === 'write').length, 0)
}

// 4. seeded random streams of these jobs
const mulberry = (a) => () => { a |= 0; a = a + 0x6D2B79F5 | 0; let t = Math.imul(a ^ a >>> 15, 1 | a); t = t + Math.imul(t ^ t >>> 7, 61 | t) ^ t; return ((t ^ t >>> 14) >>> 0) / 4294967296 }
const tickEnd = () => new Promise((resolve) => setImmediate(resolve))
async function stream(seed, batch, early) {
	const rnd = mulberry(seed)
	const pick = (list) => list[Math.floor(rnd() * list.length)]
	const log = []
	const r = layoutRig({ batch, progress: batch, early }, () => `4. stream seed ${seed}${batch ? ', runPrograms' : ''}${early ? ', earlyLaunch' : ''}: ${log.join(' ')}`)
	r.d.fieldBatch = rnd() < 0.5
	const L = r.loader()
	const m = r.enlarging()
	const fields = [] // every field image there is
	const outs = [] // every frame somebody may ask for
	const step = async (k) => {
		const op = pick(['channel', 'channel', 'oneField', 'consumer', 'reader', 'fused', 'ask', 'ask', 'hostWrite', 'tick'])
		log.push(op)
		if (op === 'channel' || op === 'oneField') {
			const ch = r.channel(`c${k}`, op === 'channel' ? [0, 1] : [pick([0, 1])], L, m)
			fields.push(...ch.y)
			outs.push(...ch.out.filter(Boolean))
		} else if (op === 'consumer' && fields.length) outs.push(r.plainConsumer(`p${k}`, pick(fields)).out)
		else if (op === 'reader' && fields.length) r.plainReader(`r${k}`, pick(fields))
		else if (op === 'fused') {
			const u = r.image(`u${k}`)
			r.d.record(r.P.read, Object.assign({ input: r.v210(`s${k}`), output: u, width: r.W }, L), 1)
			const out = r.v210(`o${k}`)
			r.d.record(r.P.write, Object.assign({ input: u, output: out, width: r.W, interlace: 0 }, r.saver), 1)
			outs.push(out)
		} else if (op === 'ask' && outs.length) r.d.touch(pick(outs), 'readonly', 2)
		else if (op === 'hostWrite' && fields.length) { const f = pick(fields); r.d.touch(f, pick(['writeonly', 'none']), 0); r.hostWrote(f) }
		else if (op === 'tick') await tickEnd()
	}
	const steps = 6 + Math.floor(rnd() * 10)
	try {
		for (let k = 0; k < steps; ++k) await step(k)
		await tickEnd()
		for (const o of outs) r.d.touch(o, 'readonly', 2)
		r.d.forceAll()
	} catch (e) {
		problems.push({ where: `4. stream seed ${seed}${batch ? ', runPrograms' : ''}${early ? ', earlyLaunch' : ''}: ${log.join(' ')}`, what: `threw: ${e && e.message || e}` })
	}
	expect(`4. stream seed ${seed}${batch ? ', runPrograms' : ''}${early ? ', earlyLaunch' : ''}: nothing left recorded`, r.d.pending.size, 0)
}

;(async () => {
	const seed0 = Number(process.argv[2] || 1)
	const streams = Number(process.argv[3] || 300)
	for (let s = 0; s < streams; ++s) for (const batch of [false, true]) for (const early of [false, true]) await stream(seed0 + s, batch, early)
	process.stdout.write(JSON.stringify({ checks, problems: problems.slice(0, 20), nProblems: problems.length, streams, seed: seed0 }) + '\n')
})()
