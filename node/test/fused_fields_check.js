'use strict'
// node/defer.js without a device: the context option `fusedFields` (the stand-in for the addon only counts, as in up_tails_check.js).  A
// 1080i-shaped channel - plain v210 reads of the output's size, combine_2, and SDI's v210 write of ONE field - posts three ticks with
// `fusedWriters`.  With `fusedFields: true` the library's "fused_fields" is set ONCE, in front of the first launch; the recorded stream
// folds into the same fused_v210_combine_multi_<n> job with the same arguments, with the option or without (no planning changes);
// without `fusedFields` the option is never set.  Prints one JSON object { checks, problems }.
const { rig, Deferral } = require('./defer_rig.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function setup(fusedFields) {
	const r = rig()
	const events = [] // ['option', name, value] | ['launch', program name, parameter names]
	r.native.setOption = (_ctx, name, value) => events.push(['option', name, value])
	r.native.observe = (name, names) => events.push(['launch', name, names.slice().sort()])
	r.d.fusedWriters = true
	// (what the Deferral's constructor makes of the context's `fusedFields`: see the constructor's own check below)
	r.d.fusedFields = fusedFields === true
	const writer = (format, lines) => ({ name: 'write', format, globalWorkItems: [2 * lines], workItemsPerGroup: 2, _handle: { name: 'write' } })
	const field = { v210: writer('v210', r.H / 2), bgra8: writer('bgra8', r.H / 2) }
	const L = r.loader()
	const tick = (interlace, screen) => {
		const u = [r.image('u0'), r.image('u1')], comb = r.image('comb')
		u.forEach((im, i) => r.d.record(r.P.read, Object.assign({ input: r.v210(`s${i}`), output: im, width: r.W }, L), 1))
		r.d.record(r.P.combine2, { l0In: u[0], l1In: u[1], output: comb }, 1)
		const sdi = r.v210('sdi')
		r.d.record(field.v210, Object.assign({ input: comb, width: r.W, interlace, output: sdi }, r.saver), 1)
		const scr = screen ? r.v210('screen') : null
		if (scr) r.d.record(field.bgra8, Object.assign({ input: comb, width: r.W, interlace, output: scr }, r.saver), 1)
		r.d.touch(sdi, 'readonly', 2)
		if (scr) r.d.touch(scr, 'readonly', 2)
	}
	return { r, events, tick, launches: () => events.filter((e) => e[0] === 'launch'), options: () => events.filter((e) => e[0] === 'option') }
}

// the constructor reads the context's option: true only when asked for
for (const [given, want] of [[true, true], [false, false], [undefined, false], [1, false]]) {
	const d = new Deferral({ _native: {}, _ctx: {}, queue: { load: 0, process: 1, unload: 2 }, fusedFields: given })
	expect(`new Deferral: fusedFields ${given}`, [d.fusedFields, d.fusedFieldsSet], [want, false])
}

const seen = {}
for (const fusedFields of [true, false, undefined]) {
	const tag = `fusedFields ${fusedFields}`
	const s = setup(fusedFields)
	expect(`${tag}: nothing is set before something is launched`, s.events.length, 0)
	s.tick(1, false)
	expect(`${tag}: SDI's field is one launch of the several-outputs form`, s.launches().map((l) => l[1]), ['fused_v210_combine_multi_2'])
	for (const n of ['l0In', 'l1In', 'output', 'interlace', 'outColMatrix', 'outGammaLut', 'colMatrix', 'gammaLut', 'gamutMatrix'])
		expect(`${tag}: the launch names '${n}'`, s.launches()[0][2].includes(n), true)
	s.tick(3, true)
	s.tick(1, true)
	expect(`${tag}: three ticks, a launch each`, s.launches().map((l) => l[1]), ['fused_v210_combine_multi_2', 'fused_v210_combine_multi_2', 'fused_v210_combine_multi_2'])
	for (const n of ['output1', 'interlace1', 'out1GammaLut'])
		expect(`${tag}: SDI + the screen, one field: the launch names '${n}'`, s.launches()[1][2].includes(n), true)
	expect(`${tag}: no write is left, nothing fell back`, [[...s.r.d.pending].some((n) => n.program.name === 'write'), s.r.d.stats.fallbacks], [false, 0])
	if (fusedFields === true) {
		expect(`${tag}: the option is set once`, s.options(), [['option', 'fused_fields', 1]])
		expect(`${tag}: ... in front of the first launch`, [s.events[0][0], s.events[1][0]], ['option', 'launch'])
	} else {
		expect(`${tag}: the option is never set`, s.options(), [])
	}
	seen[tag] = s.launches()
}
// nothing is planned differently: the same programs with the same arguments, in the same order
expect('the launches do not depend on the option', seen['fusedFields true'], seen['fusedFields false'])
expect('... nor on its absence', seen['fusedFields undefined'], seen['fusedFields false'])

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
