"""GPU tests (-m gpu) of ph_chan_compose_batch_out: several channels' frames, each packed for up to four consumers, in one launch.  The
contract is equality: every plane of every output of every job is compared, byte for byte, with ph_chan_compose called once per
output in the call's order (destinations poisoned with 0x5A first, so lines nobody writes count too); one case also runs against the
oracle's chain of the reference's operators."""
import re

import numpy as np
import pytest

import frames
import packfmt
from oracle import orc
from test_chan_gpu import PIP, Src, channel_variants, colour, device_layers, m, pack_random, pip_layers, random_layers
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned, writer

pytestmark = pytest.mark.gpu

ALL_OUT = ["v210"] + list(packfmt.CHAN_OUT)


def run_both(jobs, w, h, what, rspec="709"):
    """jobs: list of (layers, outs).  layers: a layer list (test_chan_gpu), or a function of the side's planes {slot: [tensors]} that
    returns DEVICE layers (a job that reads what an earlier job wrote); outs: test_chan_multi_gpu.out(...) dicts, optionally with a
    `slot` - outputs of one slot (and format) name the same planes.  Returns (route of the one call, planes of the call's side by slot,
    jobs as posted) after comparing both sides."""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    _, _, rd_d, _ = colour(rspec, rspec)
    k = hh.ctx()
    sides = []
    for _ in range(2):
        planes = {}
        for j, (_, outs) in enumerate(jobs):
            for i, o in enumerate(outs):
                planes.setdefault(o.get("slot", (j, i)), [hh.dev(p) for p in poisoned(o["fmt"], w, h)])
        sides.append(planes)
    uploaded = {}  # a job's sources are uploaded once and read by both sides

    def posted(side):
        res = []
        for j, (layers, outs) in enumerate(jobs):
            if callable(layers):
                dl = layers(sides[side])
            else:
                if j not in uploaded:
                    uploaded[j] = device_layers(layers)
                dl = uploaded[j]
            recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
            res.append((dl, [dict(fmt=o["fmt"], planes=sides[side][o.get("slot", (j, i))], interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3])
                             for i, (o, rc) in enumerate(zip(outs, recipes))]))
        return res
    together = posted(0)
    with capi.trace() as t:
        k.chan_compose_batch_out(together, w, h, *rd_d)
    k.wait()
    for dl, outputs in posted(1):
        for o in outputs:
            k.chan_compose_v210(dl, o["planes"][0] if o["fmt"] == "v210" else o["planes"], w, h, o["interlace"], *rd_d, o["wr_cm"], o["wr_lut"], out_fmt=o["fmt"])
    k.wait()
    torch.cuda.synchronize()
    for slot in sides[0]:
        for pl, (a, b) in enumerate(zip(sides[0][slot], sides[1][slot])):
            got, want = hh.host(a, np.uint8), hh.host(b, np.uint8)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s: output %r plane %d: %d of %d bytes differ from the separate ph_chan_compose calls, first at %d (route %s)" % (
                what, slot, pl, bad.size, got.size, bad[0], t.route)
    return t.route, sides[0], together


SIZES = [(384, 54), (200, 10), (1280, 24)]
OUT_SETS = [[(f, 0)] for f in ALL_OUT] + [[("v210", 0), ("bgra8", 0)], [("v210", 0), ("yuv422p8", 0), ("rgba8", 0)], [("yuv420p", 0), ("nv12", 0)],
                                          [("v210", 1), ("rgba8", 0)]]

_variants = {}


def variants(w, h):
    """four channels' programs (insets, a wipe with an f32 mask, a dissolve under an f32 layer, one plain layer), made once per size"""
    if (w, h) not in _variants:
        _variants[(w, h)] = channel_variants(w, h, 2100 + w + h)
    return _variants[(w, h)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("outset", range(len(OUT_SETS)))
def test_four_channels_equal_separate_calls(w, h, outset):
    """384 x 54: whole 48-pixel blocks; 200 x 10: a v210 tail quad, a multiple of 8, h % 4 == 2; 1280 x 24: the reference's third format"""
    outs = [out(f, il) for f, il in OUT_SETS[outset]]
    route, _, _ = run_both([(layers, outs) for layers in variants(w, h)], w, h, "%dx%d %r" % (w, h, OUT_SETS[outset]))
    if OUT_SETS[outset] == [("v210", 0)]:
        return  # (v210 alone: frames the enlarged-clip routes may take are handed on, as ph_chan_compose_batch hands them on)
    per = len(outs)
    assert "chan_compose_batch_out<" in route and re.search(r"x(\d)o(\d)", route), route
    assert sum(int(x.split("o")[1]) for x in re.findall(r"x\do\d", route)) == 4 * per, route  # every output came from a shared launch


@pytest.mark.parametrize("first", [("v210", 0), ("rgba8", 3)])
def test_an_odd_height_field_beside_a_frame(first):
    """96 x 9: an rgba8 field of an odd-height frame (5 and 4 lines, of which a field write makes 4: line_end) beside a whole frame"""
    w, h = 96, 9
    outs = [out("rgba8", 1), out("v210", 0)] if first[0] == "v210" else [out("rgba8", 3), out("bgra8", 0)]
    jobs = [(pip_layers(w, h, 2200 + i, 3), outs) for i in range(3)]
    route, _, _ = run_both(jobs, w, h, "96x9 %r" % (outs,))
    assert re.fullmatch(r"chan_compose_batch_out<\d>x3o6", route), route


def test_against_the_oracle_chain():
    """four channels, each v210 + a yuv422p8 field 3: every plane is the oracle's writer on the oracle's combined image"""
    import hip_harness as hh
    w, h = 384, 54
    outs = [out("v210"), out("yuv422p8", 3)]
    route, planes, _ = run_both([(layers, outs) for layers in variants(w, h)], w, h, "oracle case")
    assert route == "chan_compose_batch_out<0>x4o8", route
    rd_o = colour("709", "709")[0]
    for j, layers in enumerate(variants(w, h)):
        comp = composite(layers, w, h, rd_o)
        for i, o in enumerate(outs):
            rc = writer(o["fmt"], o["spec"])
            for pl, wnt in enumerate(oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1])):
                assert np.array_equal(hh.host(planes[(j, i)][pl], np.uint8), wnt), "job %d output %d (%s) plane %d differs from the oracle" % (j, i, o["fmt"], pl)


def test_a_tail_v210_output_and_a_rounding_output_share_an_index_frame():
    """width 200: the v210 writer truncates its tail pixels' table indices, every other writer rounds - phase 1 parks the truncated index
    with the rounding beside it, and ONE launch serves both"""
    w, h = 200, 10
    outs = [out("v210"), out("yuv422p8")]
    route, _, _ = run_both([(layers, outs) for layers in variants(w, h)], w, h, "200x10 v210 + yuv422p8")
    assert route == "chan_compose_batch_out<1>x4o8", route
    # and where the tail output and the rounding output are different jobs' of one launch
    route, _, _ = run_both([(variants(w, h)[0], [out("v210")]), (variants(w, h)[1], [out("rgba8")]), (variants(w, h)[2], [out("nv12")])], w, h, "200x10 one output each")
    assert route == "chan_compose_batch_out<1>x3o3", route


# ---- sources -------------------------------------------------------------------------------------------------------------------------
def test_planar_sources_take_the_planar_instantiation():
    w, h = 384, 54
    v = variants(w, h)
    clip = [dict(src=Src(frames.pack_random("yuv422p8", w, h, 2301), w, h, fmt="yuv422p8")),
            dict(src=Src(frames.pack_random("bgra8", 100, 30, 2302), 100, 30, m(w, h, scale_x=0.3, scale_y=0.5, offset_x=0.3, offset_y=-0.2), fmt="bgra8")),
            dict(src=Src(frames.pack_random("nv12", 192, 30, 2303), 192, 30, m(w, h, **PIP[2]), fmt="nv12"))]
    outs = [out("yuv422p8"), out("bgra8")]
    route, _, _ = run_both([(v[0], outs), (clip, outs), (v[2], outs)], w, h, "a job of planar and packed-RGB sources")
    assert route == "chan_compose_batch_out<2>x3o6", route


def test_an_images_only_call_loads_no_reader_table():
    w, h = 384, 54
    jobs = []
    for j in range(3):
        img = lambda s, **kw: dict(src=Src(frames.rgba_random(w, h, 2310 + 10 * j + s, -0.05, 1.05), w, h, m(w, h, **kw) if kw else None, fmt="rgba"))
        jobs.append(([img(0), img(1, **PIP[1]), img(2, scale_x=0.4, scale_y=0.4, rotate=0.1, offset_x=0.2)], [out("yuv420p"), out("v210", 1)]))
    route, _, _ = run_both(jobs, w, h, "f32 images only")
    assert route == "chan_compose_batch_out<0>x3o6", route


def test_a_ten_bit_420_job_among_v210_jobs():
    w, h = 384, 54
    v = variants(w, h)
    clip = [dict(src=Src(pack_random("yuv420p10", w, h, 2320), w, h, m(w, h), fmt="yuv420p10")), v[0][1]]
    outs = [out("nv12"), out("v210")]
    route, _, _ = run_both([(v[0], outs), (clip, outs), (v[3], outs)], w, h, "a yuv420p10 clip among v210 jobs")
    assert route == "chan_compose_batch_out<2>x3o6", route


# ---- splits and hand-overs -------------------------------------------------------------------------------------------------------------
def launches(route):
    return [(int(j), int(o)) for j, o in re.findall(r"chan_compose_batch_out<\d>x(\d)o(\d)", route)]


def test_five_jobs_are_two_even_launches():
    w, h = 384, 54
    v = variants(w, h)
    route, _, _ = run_both([(x, [out("yuv422p8")]) for x in v + [v[1]]], w, h, "five jobs")
    assert launches(route) == [(3, 3), (2, 2)], route


def test_nine_outputs_do_not_fit_one_launch():
    w, h = 384, 54
    v = variants(w, h)
    three = [out("v210"), out("rgba8"), out("yuv420p", 1)]
    route, _, _ = run_both([(v[0], three), (v[1], three), (v[2], three)], w, h, "nine outputs")
    assert route == "chan_compose_batch_out<0>x2o6+chan_compose_multi<0>x3", route  # (even launches: two jobs share, the third is on its own)


def test_more_ops_than_a_launch_holds():
    """a wipe on every one of four layers is 12 ops: three such jobs are 36, a launch holds 24"""
    w, h = 192, 12
    second = frames.v210_random(w, h, frames.layer_seed(2330, 9))
    mask = Src(frames.mask_ramp(w, h), w, h, fmt="rgba")

    def wipes(seed):
        layers = pip_layers(w, h, seed)
        for L in layers:
            L.update(transition="wipe", incoming=Src(second, w, h), mask=mask)
        return layers
    outs = [out("bgra8"), out("yuv422p10")]
    route, _, _ = run_both([(wipes(2331), outs), (wipes(2332), outs), (wipes(2333), outs), (wipes(2334), outs)], w, h, "48 ops")
    assert launches(route) == [(2, 4), (2, 4)], route


def test_two_jobs_writing_one_plane_the_later_wins():
    w, h = 384, 54
    v = variants(w, h)
    jobs = [(v[0], [dict(out("rgba8"), slot="shared"), out("v210")]), (v[1], [out("yuv422p8")]), (v[2], [dict(out("rgba8"), slot="shared"), out("v210", 3)])]
    route, _, _ = run_both(jobs, w, h, "two jobs, one rgba8 frame")
    assert launches(route) == [(2, 3)], route  # (the third job starts a launch of its own: alone, it is ph_chan_compose_multi's)
    assert route.endswith("+chan_compose_multi<0>x2"), route


def test_a_job_reading_an_earlier_jobs_output():
    w, h = 384, 54
    v = variants(w, h)
    uploaded = device_layers(v[3])

    def reader(planes):  # the first job's rgba8 frame as a placed graphic over a v210 clip
        return uploaded + [dict(src=(planes["screen"][0], w, h, m(w, h, **PIP[1]), "rgba8"))]
    jobs = [(v[0], [dict(out("rgba8"), slot="screen"), out("v210")]), (v[1], [out("v210"), out("bgra8")]), (reader, [out("yuv422p8"), out("rgba8")]),
            (v[2], [out("yuv422p8"), out("rgba8")])]
    route, _, _ = run_both(jobs, w, h, "a job that reads what the first job writes")
    assert launches(route) == [(2, 4), (2, 4)], route


def test_a_job_writing_what_an_earlier_job_reads():
    """the second job's rgba8 frame is the graphic the first job places over its clip: the first job has read it before the second writes
    it - the second job starts the next launch, with the third"""
    w, h = 384, 54
    v = variants(w, h)
    uploaded = device_layers(v[3])

    def reader(planes):
        return uploaded + [dict(src=(planes["screen"][0], w, h, m(w, h, **PIP[1]), "rgba8"))]
    jobs = [(reader, [out("yuv422p8"), out("rgba8")]), (v[0], [dict(out("rgba8"), slot="screen"), out("v210")]), (v[1], [out("v210"), out("bgra8")])]
    route, _, _ = run_both(jobs, w, h, "a job that writes what the first job reads")
    # (three jobs without a hazard are one launch - test_an_odd_height_field_beside_a_frame; here the first is alone: ph_chan_compose_multi's)
    assert launches(route) == [(2, 4)] and re.match(r"chan_compose_multi<\d>x2\+chan_compose_batch_out<", route), route


def test_a_second_writer_table_in_the_middle_runs_in_its_turn():
    w, h = 384, 54
    v = variants(w, h)
    ours = [out("v210"), out("yuv422p8")]
    other = [out("v210", spec="2020"), out("rgba8", spec="2020")]
    route, _, _ = run_both([(v[0], ours), (v[1], ours), (v[2], other), (v[3], ours), (v[0], ours)], w, h, "a job with another writer table")
    assert route == "chan_compose_batch_out<0>x2o4+chan_compose_multi<0>x2+chan_compose_batch_out<0>x2o4", route
    # a job whose outputs name two tables between them joins no launch either
    mixed = [out("v210"), out("rgba8", spec="sRGB")]
    route, _, _ = run_both([(v[0], ours), (v[1], ours), (v[2], mixed), (v[3], ours), (v[0], ours)], w, h, "a job with two writer tables")
    assert launches(route) == [(2, 4), (2, 4)] and "chan_compose_multi<0>x2" in route, route
    # equal tables under another registration are another table
    route, _, _ = run_both([(v[0], ours), (v[1], [out("v210", own_table=True)]), (v[2], ours)], w, h, "an equal table registered twice")
    assert "chan_compose_batch_out" not in route, route


def test_the_two_fields_of_one_frame_as_two_jobs():
    w, h = 384, 54
    v = variants(w, h)
    f422 = lambda il: dict(out("yuv422p8", il), slot="frame")
    route, _, _ = run_both([(v[0], [f422(1)]), (v[1], [f422(3)])], w, h, "two fields of one yuv422p8 frame")
    assert route == "chan_compose_batch_out<0>x2o2", route
    # 4:2:0: both fields write the line pairs' chroma lines - the later call has to win, so the jobs do not share a launch
    f420 = lambda il: dict(out("yuv420p", il), slot="frame")
    route, _, _ = run_both([(v[0], [f420(1)]), (v[1], [f420(3)])], w, h, "two fields of one yuv420p frame")
    assert "chan_compose_batch_out" not in route, route
    # a field beside a frame composes the frame's lines: frames and fields do not share a launch, fields of one parity do
    route, _, _ = run_both([(v[0], [out("rgba8", 1)]), (v[1], [out("nv12", 1)]), (v[2], [out("rgba8")]), (v[3], [out("v210")])], w, h, "fields, then frames")
    assert launches(route) == [(2, 2), (2, 2)], route


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every refusal is PH_E_INVALID (-1), names its job, and leaves every output of every job as it was: three good jobs and a bad one"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    rd_d = hh.ColourParams.reader("709", "709")

    def attempt(w, h, bad_specs, match, tweak=None, at=2):
        layers = [dict(src=Src.random("v210", w, h, 1).device())]

        def outputs(specs):
            res = []
            for fmt in specs:
                f = packfmt.get(fmt)
                cm, lut = (writer(fmt, "709")[2:]) if fmt in orc.FORMAT_RANGE else hh.ColourParams.writer("709")
                res.append(dict(fmt=fmt, planes=[hh.dev(np.full(n, POISON, np.uint8)) for n in f.plane_bytes(w + (w & 1), h + (h & 1))], interlace=0, wr_cm=cm, wr_lut=lut))
            return res
        jobs = [(layers, outputs(["v210", "rgba8"])) for _ in range(3)]
        jobs.insert(at, (layers, outputs(bad_specs)))
        if tweak:
            tweak(jobs[at][1], jobs)
        with pytest.raises(capi.PhaneronError, match=match):
            k.chan_compose_batch_out(jobs, w, h, *rd_d)
        assert all((hh.host(p, np.uint8) == POISON).all() for _, outs in jobs for o in outs for p in o["planes"]), "a refused call wrote (%s)" % match

    attempt(384, 8, [], r"error -1: .*job 2: 1\.\.4 outputs")
    attempt(384, 8, ["v210", "rgba8", "bgra8", "yuv422p8", "nv12"], r"error -1: .*job 3: 1\.\.4 outputs", at=3)
    for fmt in packfmt.NOT_CHAN_OUT:
        attempt(384, 8, ["v210", fmt], r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt)
        attempt(384, 8, [fmt], r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt, at=0)
    attempt(384, 8, ["v210", "rgba8"], r"error -1: .*job 2: outputs 0 and 1 name the same plane", lambda o, jobs: o[1].update(planes=o[0]["planes"]))
    plain = hh.dev(capi.linear2gamma_lut("709"))  # never registered
    attempt(384, 8, ["v210", "rgba8"], r"error -1: .*job 2: output 1.*writer gamma LUT has no LDS form", lambda o, jobs: o[1].update(wr_lut=plain))
    attempt(384, 8, ["yuv422p8"], r"error -1: .*job 3: output 0.*writer's RGB -> YCbCr matrix is missing", lambda o, jobs: o[0].update(wr_cm=None), at=3)
    attempt(100, 8, ["v210", "yuv422p8"], r"error -1: .*job 2: output 1.*width 100")
    attempt(384, 9, ["rgba8", "yuv420p"], r"error -1: .*job 1: output 1.*4:2:0 frame needs an even height", at=1)
    attempt(384, 8, ["rgba8"], r"error -1: .*job 2: output 0.*interlace must be 0, 1 or 3", lambda o, jobs: o[0].update(interlace=2))

    def empty_source(o, jobs):
        jobs[2] = ([dict(src=(jobs[0][0][0]["src"][0], 192, 8, None))], o)  # no transform, not the output's size
    attempt(384, 8, ["rgba8"], r"error -1: .*no transform but is 192x8", empty_source)
    with pytest.raises(capi.PhaneronError, match=r"error -1: .*no jobs"):
        k.chan_compose_batch_out([], 384, 8, *rd_d)


# ---- routes and the option -----------------------------------------------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(384, 54)
    b.progs = []
    yield b
    for p in b.progs:
        p.destroy()
    b.close()


def named_jobs(b, kinds, seed):
    """by-name jobs on one-layer v210 sources: "v210" (chan_compose_v210_1), "yuv422p8" (the same with outPacking), "multi"
    (chan_compose_multi_1: v210 + yuv422p8 + rgba8 field 3).  Returns (jobs for run_programs, every output plane buffer in order)"""
    capi, w, h = b.capi, b.w, b.h
    one = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    multi = b.ctx.create_program("phaneron:chan", "chan_compose_multi_1", [w, h])
    b.progs += [one, multi]
    jobs, planes = [], []
    for i, kind in enumerate(kinds):
        src = b.upload(frames.v210_random(w, h, frames.layer_seed(seed, i)), svm="coarse")
        if kind == "v210":
            o = b.planes("v210")
            jobs.append((one, dict(b.recipe, l0In=src, output=o[0])))
        elif kind == "yuv422p8":
            o = b.planes("yuv422p8")
            jobs.append((one, dict(b.recipe, l0In=src, outPacking=capi.FORMATS["yuv422p8"], output=o[0], outputU=o[1], outputV=o[2], outColMatrix=b.cm8)))
        else:
            o0, o1, o2 = b.planes("v210"), b.planes("yuv422p8"), b.planes("rgba8")
            jobs.append((multi, dict(b.recipe, l0In=src, output=o0[0], interlace=0,
                                     out1Packing=capi.FORMATS["yuv422p8"], output1=o1[0], output1U=o1[1], output1V=o1[2], out1ColMatrix=b.cm8,
                                     out1GammaLut=b.recipe["outGammaLut"], interlace1=0,
                                     out2Packing=capi.FORMATS["rgba8"], output2=o2[0], out2GammaLut=b.recipe["outGammaLut"], interlace2=3)))
            o = o0 + o1 + o2
        planes += o
    b.ctx.wait(capi.QUEUE_LOAD)
    return jobs, planes


def test_the_option_decides_the_route_of_four_encoder_frames(by_name):
    """dry runs: with chan_batch_outs 0 a ph_run_programs call of four yuv422p8 jobs takes the route of the same jobs posted one
    ph_run_program each; with 1 it is one shared launch"""
    b = by_name
    jobs, _ = named_jobs(b, ["yuv422p8"] * 4, 2400)
    with b.capi.trace(dry_run=True) as single:
        for prog, params in jobs:
            b.ctx.run_program(prog, params)
    assert re.fullmatch(r"chan_compose_v210<\d,2>(\+chan_compose_v210<\d,2>){3}", single.route), single.route
    with b.capi.trace(dry_run=True) as off:
        b.ctx.run_programs(jobs)
    assert off.route == single.route, (off.route, single.route)
    b.ctx.set_option("chan_batch_outs", 1)
    with b.capi.trace(dry_run=True) as on:
        b.ctx.run_programs(jobs)
    assert on.route == "chan_compose_batch_out<0>x4o4", on.route
    b.ctx.set_option("chan_batch_outs", 0)
    with b.capi.trace(dry_run=True) as again:
        b.ctx.run_programs(jobs)
    assert again.route == single.route
    with pytest.raises(b.capi.PhaneronError, match="chan_batch_outs"):
        b.ctx.set_option("chan_batch_outs", 2)


@pytest.mark.parametrize("option", [0, 1])
def test_by_name_a_mixed_call_equals_the_jobs_posted_one_by_one(by_name, option):
    b = by_name
    kinds = ["v210", "yuv422p8", "multi", "multi", "yuv422p8", "v210", "v210", "multi"]
    want_jobs, want_planes = named_jobs(b, kinds, 2410)
    for prog, params in want_jobs:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    jobs, planes = named_jobs(b, kinds, 2410)
    b.ctx.set_option("chan_batch_outs", option)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert ("chan_compose_batch_out" in t.route) == bool(option), t.route
    if option:
        # (the four jobs between the v210 frames - yuv422p8, multi, multi, yuv422p8 - are one launch; the last multi job is on its own)
        assert t.route.count("chan_compose_batch_out<0>x4o8") == 1 and t.route.count("chan_compose_batch_out") == 1, t.route
    for i, (g, wnt) in enumerate(zip(planes, want_planes)):
        got, want = b.read(g), b.read(wnt)
        assert not (want == POISON).all() and np.array_equal(got, want), "plane %d of the call differs from the jobs posted one by one (route %s)" % (i, t.route)


# ---- seeded campaign -----------------------------------------------------------------------------------------------------------------
def test_random_calls():
    """40 seeded calls: 2 - 6 jobs of 1 - 4 random layers (decoders' frames and graphics among the sources in every other call), each with
    1 - 3 outputs of random formats, frames and fields mixed, now and then another writer recipe; widths with whole blocks, with a v210
    tail (200) and with several chunks per row"""
    r = np.random.default_rng(20261018)
    sizes = [(192, 10), (200, 10), (384, 18)]
    for case in range(40):
        w, h = sizes[case % len(sizes)]
        jobs = []
        for _ in range(int(r.integers(2, 7))):
            layers = random_layers(r, w, h, int(r.integers(1, 5)), with_planar=case % 2 == 1)
            fmts = r.choice(ALL_OUT, size=int(r.integers(1, 4)), replace=False)
            same_field = int(r.choice([0, 0, 1, 3]))
            outs = [out(str(f), same_field if r.random() < 0.7 else int(r.choice([0, 1, 3])), spec="2020" if r.random() < 0.1 else "709") for f in fmts]
            jobs.append((layers, outs))
        run_both(jobs, w, h, "random call %d: %dx%d, %r" % (case, w, h, [[(o["fmt"], o["interlace"], o["spec"]) for o in outs] for _, outs in jobs]))


# ---- full size -----------------------------------------------------------------------------------------------------------------------
def test_four_1080p_channels_for_sdi_and_the_screen():
    w, h = 1920, 1080
    route, _, _ = run_both([(layers, [out("v210"), out("bgra8")]) for layers in channel_variants(w, h, 2500)], w, h, "4 channels 1920x1080, v210 + bgra8")
    assert route == "chan_compose_batch_out<0>x4o8", route


# ---- through the node layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(__import__("shutil").which("node") is None, reason="node is not installed")
def test_four_channels_through_the_recording_context():
    """node/test/batch_out_run.js: four channels per tick, each with the screen beside SDI or an encoder; with `batchOuts` the tick is one
    launch, without it a launch per channel - the same bytes as the launch-as-posted context either way"""
    import json
    import os
    import shutil
    import subprocess
    import sys
    from phaneron_amd import build as hipbuild
    root = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    hipbuild.build()
    subprocess.run([sys.executable, os.path.join(root, "node", "build.py")], check=True)
    r = subprocess.run([shutil.which("node"), os.path.join(root, "node", "test", "batch_out_run.js")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["problems"], json.dumps(res["problems"], indent=1)
    assert [s["name"] for s in res["scenarios"]] == ["batchOuts: true", "batchOuts off (the default)"]
    assert all(s["planes"] == 24 for s in res["scenarios"])  # (two ticks of 2 x (1 + 1) + 2 x (3 + 1) planes)
