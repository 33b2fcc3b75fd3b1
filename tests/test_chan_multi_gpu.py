"""GPU tests (-m gpu) of ph_chan_compose_multi: a channel's frame packed for several consumers (channel.ts:64-88: each runs its own
FromRGBA on the one combined image) from ONE composition.  Every output of every case is compared, byte for byte, with the oracle's
chain ending in that format's writer (destinations poisoned with 0x5A first) and with a separate ph_chan_compose call."""
import re

import numpy as np
import pytest

import frames
import packfmt
from oracle import orc
from test_chan_gpu import PIP, Src, colour, device_layers, m, pack_random, pip_layers, random_layers

pytestmark = pytest.mark.gpu

POISON = 0x5A
ALL_OUT = ["v210"] + list(packfmt.CHAN_OUT)


def composite(layers, ow, oh, rd_o):
    """the oracle's combined image of a layer list, transitions included (test_chan_gpu.oracle_chain without its writer)"""
    placed = []
    for L in layers:
        t = L["src"].oracle(rd_o, ow, oh)
        kind = L.get("transition", "cut")
        if kind == "dissolve":
            t = orc.transition_dissolve(t, L["incoming"].oracle(rd_o, ow, oh), L["mix"])
        elif kind == "wipe":
            t = orc.transition_wipe(t, L["incoming"].oracle(rd_o, ow, oh), L["mask"].oracle(rd_o, ow, oh))
        placed.append(t)
    return placed[0] if len(placed) == 1 else orc.combine(placed)


_writers = {}


def writer(fmt, spec, own_table=False):
    """a format's writer recipe on both sides: (oracle matrix, oracle table, device matrix, device table); own_table: a table of the same
    contents registered under a pointer of its own; spec: a colour space's name, or a table of the caller's own"""
    import hip_harness as hh
    from phaneron_amd import capi
    if not isinstance(spec, str):  # (host table, registered device table) of the caller's own (tests/luts.py) under the 709 matrix; not cached
        rng = orc.FORMAT_RANGE[fmt]
        return (None if rng is None else orc.rgb2ycbcr_matrix("709", *rng), spec[0], None if rng is None else hh.dev(capi.rgb2ycbcr_matrix("709", *rng)), spec[1])
    key = (fmt, spec, own_table)
    if key not in _writers:
        rng = orc.FORMAT_RANGE[fmt]
        lut_d = hh.ColourParams.writer(spec)[1]
        if own_table:
            lut = capi.linear2gamma_lut(spec)
            lut_d = hh.dev(lut)
            hh.ctx().register_lut(lut_d, lut)
        _writers[key] = (None if rng is None else orc.rgb2ycbcr_matrix(spec, *rng), orc.linear2gamma_lut(spec),
                         None if rng is None else hh.dev(capi.rgb2ycbcr_matrix(spec, *rng)), lut_d)
    return _writers[key]


def out(fmt, interlace=0, spec="709", own_table=False):
    return dict(fmt=fmt, interlace=interlace, spec=spec, own_table=own_table)


def poisoned(fmt, w, h):
    return [np.full(n, POISON, np.uint8) for n in frames.pack_plane_bytes(fmt, w, h)]


def oracle_frame(fmt, comp, w, h, interlace, wcm, wlut):
    """the oracle's writer of `fmt` on poisoned planes, as byte arrays"""
    before = poisoned(fmt, w, h)
    if fmt == "v210":
        words = orc.v210_write(comp, w, h, interlace, wcm, wlut, out=before[0].view(np.uint32).copy())
        return [np.asarray(words).reshape(-1).view(np.uint8)]
    return orc.pack_write(fmt, comp, w, h, interlace, wcm, wlut, planes=before)


def check_multi(layers, w, h, outs, what, rspec="709", separate=True):
    """one ph_chan_compose_multi call against the oracle and against separate calls; returns the call's traced route"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, _, rd_d, _ = colour(rspec, rspec)
    comp = composite(layers, w, h, rd_o)
    k = hh.ctx()
    dl = device_layers(layers)
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
    dst = [[hh.dev(p) for p in poisoned(o["fmt"], w, h)] for o in outs]
    outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]
    with capi.trace() as t:
        k.chan_compose_multi(dl, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8) for p in d] for d in dst]
    for i, o in enumerate(outs):
        for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
            bad = np.flatnonzero(g != wnt)
            assert bad.size == 0, "%s: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d" % (
                what, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0])
    if separate:
        for i, (o, rc) in enumerate(zip(outs, recipes)):
            alone = [hh.dev(p) for p in poisoned(o["fmt"], w, h)]
            k.chan_compose_v210(dl, alone[0] if o["fmt"] == "v210" else alone, w, h, o["interlace"], *rd_d, rc[2], rc[3], out_fmt=o["fmt"])
            k.wait()
            torch.cuda.synchronize()
            for pl, a in enumerate(alone):
                assert np.array_equal(got[i][pl], hh.host(a, np.uint8)), "%s: output %d (%s) plane %d differs from a separate ph_chan_compose call" % (what, i, o["fmt"], pl)
    return t.route


def mixed_program(w, h, seed):
    """the 5-layer program of test_other_output_formats: v210 PiP layers, a placed bgra8 graphic, a placed yuv420p clip"""
    layers = pip_layers(w, h, seed, 3)
    layers.append(dict(src=Src(frames.pack_random("bgra8", 100, 30, seed + 1), 100, 30, m(w, h, scale_x=0.3, scale_y=0.5, offset_x=0.3, offset_y=-0.2), fmt="bgra8")))
    layers.append(dict(src=Src(frames.pack_random("yuv420p", w, h + (h & 1), seed + 2), w, h + (h & 1), m(w, h, **PIP[3]), fmt="yuv420p")))
    return layers


_mixed = {}


def mixed(w, h):
    if (w, h) not in _mixed:
        _mixed[(w, h)] = mixed_program(w, h, 1700 + w + h)
    return _mixed[(w, h)]


PAIRS = [("v210", f) for f in packfmt.CHAN_OUT] + [("yuv422p8", "bgra8"), ("nv12", "rgba8")]


@pytest.mark.parametrize("a,b", PAIRS)
def test_format_pairs(a, b):
    route = check_multi(mixed(384, 54), 384, 54, [out(a), out(b)], "%s + %s" % (a, b))
    assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route


def test_four_outputs_in_one_call():
    route = check_multi(mixed(384, 54), 384, 54, [out("v210"), out("yuv422p8"), out("yuv420p"), out("bgra8")], "four outputs")
    assert re.fullmatch(r"chan_compose_multi<\d>x4", route), route


LINE_MIXES = [[("v210", 1), ("rgba8", 0)], [("v210", 3), ("yuv422p8", 0)], [("v210", 1), ("v210", 3)]]


@pytest.mark.parametrize("w,h", [(384, 54), (96, 9)])
@pytest.mark.parametrize("mix", range(len(LINE_MIXES)))
def test_line_mixes(w, h, mix):
    """outputs that want different lines: the whole frame is composed, a field output takes the index rows of its parity.  96 x 9: an odd
    height (fields of 5 and 4 lines, of which a field write makes 4: v210.ts:323), v210 and packed-RGB outputs only"""
    outs = [out(f if (h % 2 == 0 or f in ("v210", "rgba8")) else "bgra8", il) for f, il in LINE_MIXES[mix]]
    layers = mixed(w, h) if h % 2 == 0 else pip_layers(w, h, 1720, 3)
    check_multi(layers, w, h, outs, "%dx%d %r" % (w, h, LINE_MIXES[mix]))


def test_one_field_for_every_output_composes_that_field_only():
    """v210 field 1 + yuv420p field 1: the field's lines are all that is composed and written (one launch; the other field's lines keep
    their poison, 4:2:0 chroma from the written line of each pair)"""
    route = check_multi(mixed(384, 54), 384, 54, [out("v210", 1), out("yuv420p", 1)], "v210 field 1 + yuv420p field 1")
    assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route


def test_a_420_field_beside_a_420_frame():
    check_multi(mixed(384, 54), 384, 54, [out("yuv420p", 3), out("nv12", 0)], "yuv420p field 3 + nv12 frame")


@pytest.mark.parametrize("w,h,fmts", [(100, 9, ("v210", "rgba8", "bgra8")), (1280, 6, ("v210", "yuv422p8", "nv12")), (200, 10, ("yuv422p10", "yuv420p"))])
def test_ragged_lines(w, h, fmts):
    """a v210 output whose lines end in a tail quad (its tail pixels' table indices are truncated, v210.ts:176-178) beside outputs that
    round theirs; planar outputs on a width that is no multiple of 48"""
    layers = pip_layers(w, h, 1730 + w, 3)
    check_multi(layers, w, h, [out(f) for f in fmts], "%dx%d %r" % (w, h, fmts))


def test_more_chunks_than_workgroups():
    w, h = 384, 540
    layers = pip_layers(w, h, 1740, 3)
    check_multi(layers, w, h, [out("v210"), out("bgra8"), out("yuv422p10")], "384x540: several slots per workgroup")


def mode_programs():
    w, h = 384, 54
    progs = []
    for src in ["v210", "yuv420p", "yuv422p10"] + packfmt.PLANAR_10_420:
        def clip(seed, ww, hh_, src=src, **kw):
            data = frames.v210_random(ww, hh_, frames.layer_seed(seed, 0)) if src == "v210" else pack_random(src, ww, hh_, seed)
            return dict(src=Src(data, ww, hh_, m(w, h, **kw), fmt=src))
        progs.append(("%s clip under the default fill" % src, lambda clip=clip: [clip(900, w, h)]))
        progs.append(("%s clips placed" % src, lambda clip=clip: [clip(901, w, h), clip(902, 192, 30, **PIP[1]), clip(903, 192, 30, scale_x=0.4, scale_y=0.4, rotate=0.1, offset_x=0.2)]))
    progs.append(("rgba8 graphic over a v210 clip", lambda: [dict(src=Src(frames.v210_random(w, h, frames.layer_seed(92, 0)), w, h, m(w, h))),
                                                            dict(src=Src(frames.pack_random("rgba8", w, h, 975), w, h, m(w, h), fmt="rgba8"))]))
    progs.append(("ragged v210 sources", lambda: pip_layers(100, 8, 1750, 2)))
    progs.append(("v210 clips, a graphic and a planar clip", lambda: mixed(w, h)))
    return progs


@pytest.mark.parametrize("case", range(13))
def test_every_phase_one_mode(case):
    """every kind of program the one-output launcher has a phase-1 instantiation for: v210 + rgba8, and the traced MODE is the one the
    one-output v210 call of the same program gets"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    what, make = mode_programs()[case]
    layers = make()
    w, h = (100, 8) if what.startswith("ragged") else (384, 54)
    k = hh.ctx()
    k.set_option("chan_enlarged", 0)  # (the one-output call is to name the channel kernel's instantiation, whatever other route the frame could take)
    try:
        route = check_multi(layers, w, h, [out("v210"), out("rgba8")], what)
        _, _, rd_d, wr_d = colour("709", "709")
        with capi.trace(dry_run=True) as t:
            k.chan_compose_v210(device_layers(layers), torch.zeros(frames.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda"), w, h, 0, *rd_d, *wr_d)
    finally:
        k.set_option("chan_enlarged", 1)
    one = re.fullmatch(r"chan_compose_v210<(\d),0>", t.route)
    multi = re.fullmatch(r"chan_compose_multi<(\d)>x2", route)
    assert one and multi and one.group(1) == multi.group(1), "%s: one output %r, two outputs %r" % (what, t.route, route)


def test_all_six_modes_are_met():
    """(the cases of test_every_phase_one_mode name every instantiation between them: a dry run per program)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    seen = set()
    for what, make in mode_programs():
        layers = make()
        w, h = (100, 8) if what.startswith("ragged") else (384, 54)
        outputs = [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in ("v210", "rgba8")]
        with capi.trace(dry_run=True) as t:
            k.chan_compose_multi(device_layers(layers), outputs, w, h, *rd_d)
        seen.add(t.route)
        assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"]), "%s: a dry run wrote" % what
    assert seen == {"chan_compose_multi<%d>x2" % mode for mode in range(6)}, sorted(seen)


def test_transitions():
    w, h = 384, 64
    second = frames.v210_random(w, h, frames.layer_seed(1760, 1), legal=False)
    layers = pip_layers(w, h, 1761)
    layers[3].update(transition="wipe", incoming=Src(second, w, h, m(w, h)), mask=Src(frames.v210_ramp(w, h), w, h, m(w, h, scale_x=1.5, scale_y=1.5)))
    layers[1].update(transition="dissolve", mix=1.0 / 3.0, incoming=Src(second, w, h, m(w, h, scale_x=0.5, scale_y=0.5)))
    check_multi(layers, w, h, [out("v210"), out("yuv422p8")], "a wipe and a dissolve, two outputs")


def test_writer_recipes_of_their_own():
    """'709' v210 + '2020' yuv422p10 + 'sRGB' rgba8: three writer tables, swapped in one after the other"""
    check_multi(mixed(384, 54), 384, 54, [out("v210", spec="709"), out("yuv422p10", spec="2020"), out("rgba8", spec="sRGB")], "three writer recipes")


def test_equal_tables_under_different_pointers():
    check_multi(mixed(384, 54), 384, 54, [out("v210"), out("yuv422p8", own_table=True)], "equal tables, two registrations")
    check_multi(mixed(384, 54), 384, 54, [out("rgba8", own_table=True), out("v210"), out("bgra8", own_table=True), out("nv12")], "two tables, outputs interleaved")


def test_refusals():
    """every refusal is PH_E_INVALID (-1) and leaves every output as it was"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    rd_d = hh.ColourParams.reader("709", "709")

    def attempt(w, h, specs, match, tweak=None):
        layers = [dict(src=Src.random("v210", w, h, 1).device())]
        outputs = []
        for fmt in specs:
            f = packfmt.get(fmt)
            cm, lut = (writer(fmt, "709")[2:]) if fmt in orc.FORMAT_RANGE else hh.ColourParams.writer("709")
            outputs.append(dict(fmt=fmt, planes=[hh.dev(np.full(n, POISON, np.uint8)) for n in f.plane_bytes(w + (w & 1), h + (h & 1))], interlace=0, wr_cm=cm, wr_lut=lut))
        if tweak:
            tweak(outputs)
        with pytest.raises(capi.PhaneronError, match=match):
            k.chan_compose_multi(layers, outputs, w, h, *rd_d)
        assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"]), "a refused call wrote (%s)" % match

    attempt(384, 8, [], r"error -1: .*1\.\.4 outputs")
    attempt(384, 8, ["v210", "rgba8", "bgra8", "yuv422p8", "nv12"], r"error -1: .*1\.\.4 outputs")
    for fmt in packfmt.NOT_CHAN_OUT:
        attempt(384, 8, ["v210", fmt], r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt)
    attempt(384, 8, ["v210", "rgba8"], r"error -1: .*same plane", lambda o: o[1].update(planes=o[0]["planes"]))
    plain = hh.dev(capi.linear2gamma_lut("709"))  # never registered
    attempt(384, 8, ["v210", "rgba8"], r"error -1: .*output 1.*writer gamma LUT has no LDS form", lambda o: o[1].update(wr_lut=plain))
    attempt(100, 8, ["v210", "yuv422p8"], r"error -1: .*output 1.*width 100")
    attempt(384, 9, ["rgba8", "yuv420p"], r"error -1: .*output 1.*4:2:0 frame needs an even height")


# ---- by name: chan_compose_multi_<n> ---------------------------------------------------------------------------------------------------
class ByName:
    """a context of its own with buffers as a binding makes them (runProgram's arguments are buffers and numbers)"""

    def __init__(self, w, h):
        from phaneron_amd import capi
        self.capi, self.w, self.h = capi, w, h
        self.ctx = capi.Context(0)
        self.bufs = []
        up = self.upload
        self.recipe = {"colMatrix": up(capi.ycbcr2rgb_matrix("709")), "gammaLut": up(capi.gamma2linear_lut("709"), svm="coarse"),
                       "gamutMatrix": up(capi.rgb2rgb_matrix("709", "709")), "outColMatrix": up(capi.rgb2ycbcr_matrix("709")),
                       "outGammaLut": up(capi.linear2gamma_lut("709"), svm="coarse")}
        self.cm8 = up(capi.rgb2ycbcr_matrix("709", *capi.FORMAT_RANGE["yuv422p8"]))
        self.rd_o = (orc.ycbcr2rgb_matrix("709"), orc.gamma2linear_lut("709"), orc.rgb2rgb_matrix("709", "709"))
        self.ctx.wait(capi.QUEUE_LOAD)

    def upload(self, arr, access="readwrite", svm="none"):
        a = np.ascontiguousarray(arr)
        b = self.ctx.create_buffer(a.nbytes, access, svm)
        b.host_access("writeonly", self.capi.QUEUE_LOAD, a)
        self.bufs.append(b)
        return b

    def planes(self, fmt):
        return [self.upload(p, svm="coarse") for p in poisoned(fmt, self.w, self.h)]

    def read(self, b):
        b.host_access("readonly", self.capi.QUEUE_UNLOAD)
        return b.host(np.uint8).copy()

    def close(self):
        for b in self.bufs:
            b.release()
        self.ctx.close()


@pytest.fixture
def by_name():
    b = ByName(384, 54)
    yield b
    b.close()


def three_output_params(b, src_buf):
    """a one-layer frame for v210 (output 0), yuv422p8 (1) and rgba8, field 3 (2)"""
    capi = b.capi
    o0, o1, o2 = b.planes("v210"), b.planes("yuv422p8"), b.planes("rgba8")
    params = dict(b.recipe, l0In=src_buf, output=o0[0], interlace=0,
                  out1Packing=capi.FORMATS["yuv422p8"], output1=o1[0], output1U=o1[1], output1V=o1[2], out1ColMatrix=b.cm8, out1GammaLut=b.recipe["outGammaLut"], interlace1=0,
                  out2Packing=capi.FORMATS["rgba8"], output2=o2[0], out2GammaLut=b.recipe["outGammaLut"], interlace2=3)
    return params, (o0, o1, o2)


def expect_three(b, comp):
    w, h = b.w, b.h
    wlut = orc.linear2gamma_lut("709")
    return [oracle_frame("v210", comp, w, h, 0, orc.rgb2ycbcr_matrix("709"), wlut),
            oracle_frame("yuv422p8", comp, w, h, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["yuv422p8"]), wlut),
            oracle_frame("rgba8", comp, w, h, 3, None, wlut)]


def test_by_name_run_program(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    src = frames.v210_random(w, h, frames.layer_seed(1770, 0))
    params, outs = three_output_params(b, b.upload(src, svm="coarse"))
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "chan_compose_multi_1", [w, h])
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert re.fullmatch(r"chan_compose_multi<\d>x3", t.route), t.route
    want = expect_three(b, orc.v210_read(src, w, h, *b.rd_o))
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    prog.destroy()


def test_by_name_run_programs_keeps_order(by_name):
    """a job that WRITES the multi job's source in front of it and a job that READS its output 2 behind it, in one ph_run_programs call"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    first = frames.v210_random(w, h, frames.layer_seed(1771, 0))
    stale = b.upload(np.full(frames.v210_pitch_bytes(w) * h, POISON, np.uint8), svm="coarse")  # what the first job overwrites
    last_out = b.planes("v210")[0]
    params, outs = three_output_params(b, stale)
    b.ctx.wait(capi.QUEUE_LOAD)
    one = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    multi = b.ctx.create_program("phaneron:chan", "chan_compose_multi_1", [w, h])
    jobs = [(one, dict(b.recipe, l0In=b.upload(first, svm="coarse"), output=stale)),
            (multi, params),
            (one, dict(b.recipe, l0In=outs[2][0], l0Packing=capi.FORMATS["rgba8"], l0Width=w, l0Height=h, output=last_out))]
    b.ctx.wait(capi.QUEUE_LOAD)
    b.ctx.run_programs(jobs)
    b.ctx.wait()
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    frame0 = np.asarray(orc.v210_write(orc.v210_read(first, w, h, *b.rd_o), w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(stale).view(np.uint32), frame0.view(np.uint32))
    want = expect_three(b, orc.v210_read(frame0.view(np.uint32), w, h, *b.rd_o))
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    # the last job read output 2 as it stood after the multi job: its field-3 lines written, the others still poison
    rgba8 = packfmt.get("rgba8")
    img = rgba8.oracle_read([want[2][0]], w, h, None, b.rd_o[1], b.rd_o[2])
    last = np.asarray(orc.v210_write(img, w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(last_out).view(np.uint32), last.view(np.uint32))
    one.destroy(), multi.destroy()


def test_by_name_checks_answer_as_output_zero_does(by_name):
    """one defect per new argument: ph_check_program and ph_run_program give the same code and text, and the text is output 0's with the
    argument's own name in it"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    params, outs = three_output_params(b, b.upload(frames.v210_random(w, h, 5), svm="coarse"))
    small = b.upload(np.zeros(64, np.uint8))
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "chan_compose_multi_1", [w, h])

    def without(d, *names):
        return {k: v for k, v in d.items() if k not in names}
    p0 = dict(params, outPacking=capi.FORMATS["yuv422p8"], outputU=params["output1U"], outputV=params["output1V"])  # output 0 planar too, for the twin defects
    defects = [  # (the multi job's defect, output 0's twin, the new argument's name, output 0's name)
        (dict(params, out1Packing=99), dict(params, outPacking=99), "out1Packing", "outPacking"),
        (dict(params, out2Packing=capi.FORMATS["p010"]), dict(params, outPacking=capi.FORMATS["p010"]), "out2Packing", "outPacking"),
        (dict(params, output1=small), dict(p0, output=small), "output1", "output"),
        (without(params, "output1U"), without(p0, "outputU"), "output1U", "outputU"),
        (dict(params, output1V=small), dict(p0, outputV=small), "output1V", "outputV"),
        (dict(params, out1Packing=capi.FORMATS["nv12"]), dict(p0, outPacking=capi.FORMATS["nv12"]), "output1C", "outputC"),
        (without(params, "out1ColMatrix"), without(params, "outColMatrix"), "out1ColMatrix", "outColMatrix"),
        (without(params, "out2GammaLut"), without(params, "outGammaLut"), "out2GammaLut", "outGammaLut"),
        (dict(params, interlace2=small), dict(params, interlace=small), "interlace2", "interlace"),
    ]
    for bad, twin, name, name0 in defects:
        texts = []
        for job in (bad, twin):
            seen = []
            for check_only in (True, False):
                with pytest.raises(capi.PhaneronError) as e:
                    b.ctx.run_program(prog, job, check_only=check_only)
                seen.append(str(e.value))
            assert seen[0] == seen[1], "%s: check %r, run %r" % (name, seen[0], seen[1])
            texts.append(seen[0])
        assert "'%s'" % name in texts[0], texts[0]
        assert texts[0].replace("'%s'" % name, "'%s'" % name0) == texts[1], "%s: %r against output 0's %r" % (name, texts[0], texts[1])
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    prog.destroy()


# ---- seeded campaign -----------------------------------------------------------------------------------------------------------------
def test_random_programs_with_random_outputs():
    """40 seeded random channel programs (test_chan_gpu.random_layers, decoders' frames and graphics among the sources), each packed for
    2-4 outputs of random formats and per-output interlace; sizes that every format takes (widths % 8, even heights)"""
    r = np.random.default_rng(20261017)
    sizes = [(192, 2), (192, 10), (384, 34), (576, 18), (768, 6), (960, 20), (200, 10), (1280, 6)]
    for case in range(40):
        w, h = sizes[case % len(sizes)]
        layers = random_layers(r, w, h, int(r.integers(1, 5)), with_planar=True)
        outs = [out(str(r.choice(ALL_OUT)), int(r.choice([0, 0, 1, 3])), spec=str(r.choice(["709", "709", "2020"]))) for _ in range(int(r.integers(2, 5)))]
        check_multi(layers, w, h, outs, "random program %d: %dx%d, %d layers, outputs %r" % (case, w, h, len(layers), [(o["fmt"], o["interlace"], o["spec"]) for o in outs]))
