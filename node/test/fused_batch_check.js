'use strict'
// node/defer.js without a device: the `fusedBatch` option (the stand-in for the addon only counts, as in fused_writers_check.js).  Four
// channels post a headline-shaped frame each in one tick - plain v210 reads of the output's size, combine_2, SDI's v210 write and the
// screen's bgra8 write on the combined image.  With `fusedWriters` and `fusedBatch` the four frames go down in ONE runPrograms call of
// four fused_v210_combine_multi_2 jobs that name one Loader and, output by output, one writer matrix and table; with `fusedBatch` off
// each is a call of its own; a refused batch falls back plan by plan.  Prints one JSON object { checks, problems }.
const { rig } = require('./defer_rig.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function tick(fusedBatch, opt) {
	opt = opt || {}
	const r = rig({ early: true, batch: true, progress: true })
	r.d.fusedWriters = opt.fusedWriters !== false
	r.d.fusedBatch = fusedBatch
	r.options = []
	r.native.setOption = (_ctx, name, value) => r.options.push([name, value])
	if (opt.refuse) r.native.refuse = opt.refuse
	const writer = (format) => ({ name: 'write', format, globalWorkItems: [2 * r.H], workItemsPerGroup: 2, _handle: { name: 'write' } })
	const W8 = { v210: writer('v210'), bgra8: writer('bgra8'), yuv422p8: writer('yuv422p8') }
	const outs = []
	for (let c = 0; c < 4; ++c) {
		const L = r.loader(opt.loaderOf ? opt.loaderOf(c) : 1) // a Loader of its own per channel, of equal contents
		const u = [r.image(`c${c}u0`), r.image(`c${c}u1`)], comb = r.image(`c${c}comb`)
		u.forEach((im, i) => r.d.record(r.P.read, Object.assign({ input: r.v210(`c${c}s${i}`), output: im, width: r.W }, L), 1))
		r.d.record(r.P.combine2, { l0In: u[0], l1In: u[1], output: comb }, 1)
		const sdi = r.v210(`c${c}sdi`), screen = r.v210(`c${c}screen`)
		r.d.record(W8.v210, Object.assign({ input: comb, width: r.W, interlace: 0, output: sdi }, r.saver), 1)
		if (opt.otherList && opt.otherList(c)) {
			const y = r.v210(`c${c}y`)
			r.d.record(W8.yuv422p8, Object.assign({ input: comb, width: r.W, interlace: 0, outputY: y, outputU: r.v210(`c${c}u`), outputV: r.v210(`c${c}v`) }, r.saver), 1)
			outs.push(sdi, y)
		} else {
			r.d.record(W8.bgra8, Object.assign({ input: comb, width: r.W, interlace: 0, output: screen }, r.saver), 1)
			outs.push(sdi, screen)
		}
		;[...u, comb].forEach((b) => b.release()) // (the channel keeps its frames only)
	}
	r.outs = outs
	return r
}

const JOB = 'fused_v210_combine_multi_2'
const scenarios = [
	['fusedBatch on', tick(true), (r) => {
		expect('fusedBatch on: four channels\' frames are one runPrograms call of four jobs', r.names(), [`batch:${[JOB, JOB, JOB, JOB].join('+')}`])
		const batch = r.launches[0]
		const at = (job, name) => batch[3][job][batch[2].split(';')[job].split(',').indexOf(name)]
		const shared = ['colMatrix', 'gammaLut', 'gamutMatrix', 'outColMatrix', 'outGammaLut', 'out1GammaLut']
		expect('the jobs name ONE Loader and one writer matrix and table per output: the first job\'s buffers', [1, 2, 3].map((j) => shared.every((k) => at(0, k) !== undefined && at(0, k) === at(j, k))), [true, true, true])
		expect('every job keeps its own layers and frames', new Set([0, 1, 2, 3].flatMap((j) => ['l0In', 'l1In', 'output', 'output1'].map((k) => at(j, k)))).size, 16)
		expect('the library\'s option is set once', r.options, [['fused_multi_batch', 1]])
		expect('counted under batched', [r.d.stats.batched, r.d.stats.launched, r.d.stats.fallbacks, r.d.pending.size], [4, 1, 0, 0])
		r.outs.forEach((o) => r.d.touch(o, 'readonly', 2))
		expect('asking for the frames afterwards launches nothing', r.launches.length, 1)
	}],
	['fusedBatch off', tick(false), (r) => {
		expect('fusedBatch off: four calls', r.names(), [JOB, JOB, JOB, JOB])
		expect('the option is not touched', [r.options, r.d.stats.batched || 0], [[], 0])
	}],
	['fusedBatch without fusedWriters', tick(true, { fusedWriters: false }), (r) => {
		expect('fusedBatch has no effect without fusedWriters', [r.names().some((n) => n.includes('fused_v210_combine_multi')), r.options], [false, []])
	}],
	['a refused batch', tick(true, { refuse: (name) => name === 'batch' }), (r) => {
		expect('a refused batch falls back plan by plan', [r.names(), r.d.stats.fallbacks, r.d.pending.size], [[JOB, JOB, JOB, JOB], 1, 0])
	}],
	['another Loader', tick(true, { loaderOf: (c) => (c === 3 ? 5 : 1) }), (r) => {
		expect('a channel of another Loader recipe stays a call of its own', r.names().sort(), [`batch:${[JOB, JOB, JOB].join('+')}`, JOB].sort())
	}],
	['another output list', tick(true, { otherList: (c) => c === 0 }), (r) => {
		expect('a channel with another list of consumers stays a call of its own', r.names().sort(), [`batch:${[JOB, JOB, JOB].join('+')}`, JOB].sort())
	}]
]

setImmediate(() => { // (earlyLaunch: the frames are launched at the end of the tick that posted them)
	for (const [, r, look] of scenarios) look(r)
	console.log(JSON.stringify({ checks, problems }))
	process.exit(problems.length ? 1 : 0)
})
