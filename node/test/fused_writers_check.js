'use strict'
// node/defer.js without a device: the `fusedWriters` option (the stand-in for the addon only counts, as in defer_check.js).  A headline-
// shaped frame - plain v210 reads of the output's size, combine_2, write - with one write that is not a v210 frame, with sibling writes,
// with the option off, and with the shared launch refused.  Prints one JSON object { checks, problems }.
const { rig } = require('./defer_rig.js')

const problems = []
let checks = 0
const expect = (what, got, want) => {
	++checks
	if (JSON.stringify(got) !== JSON.stringify(want)) problems.push({ what, got, want })
}

function setup(on, refuse) {
	const r = rig()
	r.d.fusedWriters = on
	if (refuse) r.native.refuse = refuse
	const writer = (format, lines) => ({ name: 'write', format, globalWorkItems: [2 * lines], workItemsPerGroup: 2, _handle: { name: 'write' } })
	r.W8 = { v210: writer('v210', r.H), v210Field: writer('v210', r.H / 2), bgra8: writer('bgra8', r.H), yuv422p8: writer('yuv422p8', r.H) }
	r.L = r.loader()
	r.plain = () => {
		const u = [r.image('u0'), r.image('u1')], comb = r.image('comb')
		u.forEach((im, i) => r.d.record(r.P.read, Object.assign({ input: r.v210(`s${i}`), output: im, width: r.W }, r.L), 1))
		r.d.record(r.P.combine2, { l0In: u[0], l1In: u[1], output: comb }, 1)
		return comb
	}
	r.write = (prog, comb, outs, interlace = 0) => r.d.record(prog, Object.assign({ input: comb, width: r.W, interlace }, outs, r.saver), 1)
	r.args = (i) => r.launches[i][2].split(',').sort()
	return r
}

// 1. one consumer that is not a v210 frame: an encoder's yuv422p8
{
	const r = setup(true)
	const comb = r.plain(), y = r.v210('y'), u = r.v210('u'), v = r.v210('v')
	r.write(r.W8.yuv422p8, comb, { outputY: y, outputU: u, outputV: v })
	r.d.touch(y, 'readonly', 2)
	expect('yuv422p8 alone: one launch of the headline kernel\'s several-outputs form', r.names(), ['fused_v210_combine_multi_2'])
	expect('its arguments', r.args(0), ['colMatrix', 'gammaLut', 'gamutMatrix', 'interlace', 'l0In', 'l1In', 'outColMatrix', 'outGammaLut', 'outPacking', 'output', 'outputU', 'outputV'])
}
// 2. a v210 field alone
{
	const r = setup(true)
	const comb = r.plain(), a = r.v210('sdi')
	r.write(r.W8.v210Field, comb, { output: a }, 3)
	r.d.touch(a, 'readonly', 2)
	expect('a v210 field: the several-outputs form', r.names(), ['fused_v210_combine_multi_2'])
}
// 3. SDI + the screen on one combined image: one launch, the sibling named as output 1
{
	const r = setup(true)
	const comb = r.plain(), a = r.v210('sdi'), b = r.v210('screen')
	r.write(r.W8.v210, comb, { output: a })
	r.write(r.W8.bgra8, comb, { output: b })
	r.d.touch(b, 'readonly', 2) // whichever consumer asks first
	expect('v210 + bgra8: one launch', r.names(), ['fused_v210_combine_multi_2'])
	// (the screen asked: its bgra8 frame is output 0 - outPacking, no matrix - and SDI's v210 frame output 1)
	expect('the sibling is output 1', r.args(0).filter((n) => /1/.test(n) && !/^l1/.test(n)), ['interlace1', 'out1ColMatrix', 'out1GammaLut', 'output1'])
	expect('output 0 is the write that was asked for', [r.args(0).includes('outPacking'), r.args(0).includes('outColMatrix')], [true, false])
	r.d.touch(a, 'readonly', 2)
	expect('asking the other consumer launches nothing more', r.names(), ['fused_v210_combine_multi_2'])
}
// 4. one v210 frame: the headline kernel as ever, option on or off
for (const on of [true, false]) {
	const r = setup(on)
	const comb = r.plain(), a = r.v210('sdi')
	r.write(r.W8.v210, comb, { output: a })
	r.d.touch(a, 'readonly', 2)
	expect(`one v210 frame, fusedWriters ${on}`, r.names(), ['fused_v210_combine_2'])
}
// 5. the option off: the parent's launches
{
	const r = setup(false)
	let comb = r.plain()
	const y = r.v210('y'), u = r.v210('u'), v = r.v210('v')
	r.write(r.W8.yuv422p8, comb, { outputY: y, outputU: u, outputV: v })
	r.d.touch(y, 'readonly', 2)
	comb = r.plain()
	const a = r.v210('sdi'), b = r.v210('screen')
	r.write(r.W8.v210, comb, { output: a })
	r.write(r.W8.bgra8, comb, { output: b })
	r.d.touch(a, 'readonly', 2)
	r.d.touch(b, 'readonly', 2)
	expect('fusedWriters off: the channel kernel\'s launches', r.names(), ['chan_compose_v210_2', 'chan_compose_multi_2'])
}
// 6. the shared launch refused: the channel kernel's candidates follow
{
	const r = setup(true, (name) => name.startsWith('fused_v210_combine_multi_'))
	const comb = r.plain(), a = r.v210('sdi'), b = r.v210('screen')
	r.write(r.W8.v210, comb, { output: a })
	r.write(r.W8.bgra8, comb, { output: b })
	r.d.touch(a, 'readonly', 2)
	r.d.touch(b, 'readonly', 2)
	expect('refused: the channel kernel makes both frames in one launch', r.names(), ['chan_compose_multi_2'])
}

console.log(JSON.stringify({ checks, problems }))
process.exit(problems.length ? 1 : 0)
