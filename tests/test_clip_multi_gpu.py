"""GPU tests (-m gpu) of ph_clip_compose_multi: file playback - an enlarged clip, or a decoder's frame under the default fill - packed for
up to four consumers of any format the channel kernel writes, every source pixel read once.  Every output of every case is compared,
byte for byte, with the oracle's chain (format reader -> transform -> combine -> format writer, destinations poisoned with 0x5A first)
and with a separate ph_chan_compose call; the routes are pinned with dry-run traces."""
import re

import numpy as np
import pytest

import frames
import packfmt
from oracle import orc
from test_chan_gpu import Src, both_routes, colour, device_layers, m, pack_random
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned, writer

pytestmark = pytest.mark.gpu

ALL_OUT = ["v210"] + list(packfmt.CHAN_OUT)
SOURCES = ["yuv420p", "nv12", "yuv422p8", "yuv422p10", "yuv420p10", "p010", "rgba8", "bgra8", "v210"]
ONE = r"clip_up_multi<(rgb|rgba)>x%d"


def outputs_of(outs, w, h):
    import hip_harness as hh
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    dst = [[hh.dev(p) for p in poisoned(o["fmt"], w, h)] for o in outs]
    return recipes, dst, [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]


def dry_route(layers, w, h, outs, specs=("709", "709")):
    """the route the call would take; a dry run writes nothing"""
    import hip_harness as hh
    from phaneron_amd import capi
    _, _, rd_d, _ = colour(*specs)
    _, dst, outputs = outputs_of(outs, w, h)
    with capi.trace(dry_run=True) as t:
        hh.ctx().clip_compose_multi(device_layers(layers), outputs, w, h, *rd_d)
    assert all((hh.host(p, np.uint8) == POISON).all() for d in dst for p in d), "a dry run wrote"
    return t.route


def check_clip(layers, w, h, outs, what, specs=("709", "709"), separate=True, comp=None):
    """one ph_clip_compose_multi call against the oracle and against separate ph_chan_compose calls; returns (traced route, the frames)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, _, rd_d, _ = colour(*specs)
    if comp is None:
        comp = composite(layers, w, h, rd_o)
    k = hh.ctx()
    dl = device_layers(layers)
    recipes, dst, outputs = outputs_of(outs, w, h)
    want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
    with capi.trace() as t:
        k.clip_compose_multi(dl, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8) for p in d] for d in dst]
    for i, o in enumerate(outs):
        for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
            bad = np.flatnonzero(g != wnt)
            assert bad.size == 0, "%s [%s]: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d" % (
                what, t.route, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0])
    if separate:
        for i, (o, rc) in enumerate(zip(outs, recipes)):
            alone = [hh.dev(p) for p in poisoned(o["fmt"], w, h)]
            k.chan_compose_v210(dl, alone[0] if o["fmt"] == "v210" else alone, w, h, o["interlace"], *rd_d, rc[2], rc[3], out_fmt=o["fmt"])
            k.wait()
            torch.cuda.synchronize()
            for pl, a in enumerate(alone):
                assert np.array_equal(got[i][pl], hh.host(a, np.uint8)), "%s: output %d (%s) plane %d differs from a separate ph_chan_compose call" % (what, i, o["fmt"], pl)
    return t.route, got


def clip(fmt, sw, sh, w, h, seed, **kw):
    return dict(src=Src.random(fmt, sw, sh, seed, m(w, h, **kw)))


# ---- every source format to every writer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh", [(128, 36), (384, 54)])
@pytest.mark.parametrize("src", SOURCES)
def test_every_source_format_to_every_writer(src, sw, sh):
    """a clip 128 x 36 enlarged to 384 x 54, and a 384 x 54 frame under the default fill, to each writer alone (v210 beside rgba8: alone it is
    ph_chan_compose): one launch of the clip kernel, <rgba> where the source has alpha"""
    w, h = 384, 54
    layers = [clip(src, sw, sh, w, h, 2100 + sw)]
    comp = composite(layers, w, h, colour("709", "709")[0])
    inst = "rgba" if src in ("rgba8", "bgra8") else "rgb"
    for fmt in ALL_OUT:
        outs = [out("v210"), out("rgba8")] if fmt == "v210" else [out(fmt)]
        route, _ = check_clip(layers, w, h, outs, "%s %dx%d -> %s" % (src, sw, sh, fmt), comp=comp)
        assert route == "clip_up_multi<%s>x%d" % (inst, len(outs)), route
        assert dry_route(layers, w, h, outs) == route


def test_four_outputs_in_one_call():
    w, h = 384, 54
    for layers in ([clip("yuv420p", 128, 36, w, h, 2110)], [clip("bgra8", 384, 54, w, h, 2111)]):
        route, _ = check_clip(layers, w, h, [out("v210"), out("yuv422p8"), out("nv12"), out("rgba8")], "four outputs")
        assert re.fullmatch(ONE % 4, route), route


# ---- which lines are composed ------------------------------------------------------------------------------------------------------------
def small_clip(seed=2120, fmt="yuv422p10"):
    return [clip(fmt, 96, 20, 384, 54, seed)]  # (a field write enlarges it by more than 2 vertically)


def test_one_field_for_every_output_composes_that_field_only():
    """v210 field 1 + yuv420p field 1: only that field's rows are composed and written - the other field's lines keep their poison (the
    oracle's frames are written into poisoned planes), 4:2:0 chroma from the written line of each pair"""
    route, _ = check_clip(small_clip(), 384, 54, [out("v210", 1), out("yuv420p", 1)], "v210 field 1 + yuv420p field 1")
    assert route == "clip_up_multi<rgb>x2", route
    route, _ = check_clip(small_clip(2121, "nv12"), 384, 54, [out("nv12", 3), out("bgra8", 3), out("yuv422p8", 3)], "three outputs, field 3")
    assert route == "clip_up_multi<rgb>x3", route


def test_fields_beside_a_frame():
    route, _ = check_clip(small_clip(2122), 384, 54, [out("rgba8", 1), out("yuv422p8", 3), out("v210", 0)], "fields 1 and 3 beside a frame")
    assert route == "clip_up_multi<rgb>x3", route


def test_a_420_field_beside_a_420_frame():
    """the field takes its chroma from the written line of each pair, the frame from the pair's upper line"""
    route, _ = check_clip(small_clip(2123, "yuv420p"), 384, 54, [out("yuv420p", 3), out("nv12", 0)], "yuv420p field 3 + nv12 frame")
    assert route == "clip_up_multi<rgb>x2", route
    check_clip(small_clip(2124, "p010"), 384, 54, [out("nv12", 1), out("yuv420p", 0)], "nv12 field 1 + yuv420p frame")


# ---- the kernel's units -------------------------------------------------------------------------------------------------------------------
PLANAR_SIZES = [(128, 10), (384, 54), (640, 36), (1280, 24), (1920, 40), (2520, 12)]
RGB_SIZES = [(126, 8), (50, 4), (252, 6), (1290, 14)]
UNIT_FORMATS = ["yuv420p", "yuv422p10", "yuv422p8", "nv12", "rgba8", "bgra8", "p010", "yuv420p10", "v210"]


@pytest.mark.parametrize("part", range(4))
def test_random_shapes_around_the_kernels_units(part):
    """seeded clips and placements on channels barely wider than one 126-column wave step, with tiles that end mid-frame, widths that 126
    does not divide, a channel narrower than one step; placements that push the clip partly off screen or leave a border; progressive and
    both fields.  yuv422p8 + rgba8 where a planar writer takes the width, else rgba8 + bgra8.  At least half the cases must take the
    one-launch route (a condition on the test's shapes, asserted from dry runs)"""
    r = np.random.default_rng(20261020 + part)
    sizes = PLANAR_SIZES + RGB_SIZES
    cases, one_launch = 10, 0
    for case in range(cases):
        ow, oh = sizes[(case + 3 * part) % len(sizes)]
        fmt = UNIT_FORMATS[int(r.integers(0, len(UNIT_FORMATS)))]
        interlace = int(r.choice([0, 0, 1, 3])) if oh % 2 == 0 else 0
        if r.random() < 0.25 and not interlace:
            sw, sh, kw = ow, oh, dict()
        else:
            sw = max(2, int(ow * r.uniform(0.2, 0.9)) // 2 * 2)
            sh = max(2, int(oh * r.uniform(0.2, 0.9) / (2 if interlace else 1)) // 2 * 2)
            kw = dict(scale_x=float(r.choice([1.0, 0.8, 0.6])), scale_y=float(r.choice([1.0, 0.8, 0.6])), offset_x=float(r.uniform(-0.3, 0.3)), offset_y=float(r.uniform(-0.3, 0.3)))
        layers = [clip(fmt, sw, sh, ow, oh, 5200 + 16 * part + case, **kw)]
        outs = [out("yuv422p8", interlace), out("rgba8", interlace)] if (ow, oh) in PLANAR_SIZES else [out("rgba8", interlace), out("bgra8", interlace)]
        specs = [("709", "709"), ("709", "2020")][case % 2]
        outs = [dict(o, spec=specs[1]) for o in outs]
        what = "units case %d.%d: %s %dx%d on %dx%d il %d %r" % (part, case, fmt, sw, sh, ow, oh, interlace, kw)
        route = dry_route(layers, ow, oh, outs, specs)
        one_launch += bool(re.fullmatch(ONE % 2, route))
        assert re.fullmatch(ONE % 2, route) or re.fullmatch(r"chan_compose_multi<\d>x2", route), (what, route)
        check_clip(layers, ow, oh, outs, what, specs=specs, separate=case % 3 == 0)
    assert one_launch * 2 >= cases, "only %d of %d random shapes took the one-launch route" % (one_launch, cases)


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def v210_route(layers, w, h, interlace=0):
    """what ph_chan_compose makes of a v210 frame of these layers today"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    _, _, rd_d, wr_d = colour("709", "709")
    with capi.trace(dry_run=True) as t:
        hh.ctx().chan_compose_v210(device_layers(layers), torch.zeros(frames.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda"), w, h, interlace, *rd_d, *wr_d)
    return t.route


def test_one_v210_output_is_ph_chan_compose():
    w, h = 384, 54
    for layers in ([clip("yuv420p", 128, 36, w, h, 2130)], [clip("v210", 126, 36, w, h, 2131)], [clip("yuv422p10", 96, 20, w, h, 2132), clip("nv12", 96, 20, w, h, 2133, scale_x=0.7, scale_y=0.7)],
                   [clip("yuv420p", 384, 54, w, h, 2134, rotate=0.1)]):
        for interlace in (0, 3):
            route, _ = check_clip(layers, w, h, [out("v210", interlace)], "one v210 output il %d" % interlace, separate=interlace == 0)
            assert route == v210_route(layers, w, h, interlace), route
    assert v210_route([clip("yuv420p", 128, 36, w, h, 2130)], w, h) == "clip_up_write_v210<rgb>"  # (today's one-launch kernel, untouched)


def test_a_v210_output_whose_lines_end_in_a_tail_quad_is_split_off():
    """width 1280: the v210 frame by today's route (its tail quad truncates table indices), the rgba8 frame by the new kernel"""
    w, h = 1280, 10
    layers = [clip("yuv420p", 320, 6, w, h, 2140)]
    route, _ = check_clip(layers, w, h, [out("v210"), out("rgba8")], "v210 + rgba8 at 1280")
    assert route == v210_route(layers, w, h) + "+clip_up_multi<rgb>x1", route
    route, _ = check_clip(layers, w, h, [out("yuv422p8"), out("v210", 1), out("bgra8")], "yuv422p8 + v210 field 1 + bgra8 at 1280")
    assert route == v210_route(layers, w, h, 1) + "+clip_up_multi<rgb>x2", route


def test_a_launch_per_writer_table():
    w, h = 384, 54
    layers = [clip("nv12", 128, 36, w, h, 2150)]
    route, _ = check_clip(layers, w, h, [out("yuv422p8"), out("rgba8", own_table=True)], "two tables")
    assert route == "clip_up_multi<rgb>x1+clip_up_multi<rgb>x1", route
    route, _ = check_clip(layers, w, h, [out("rgba8", own_table=True), out("v210"), out("rgba8", own_table=True), out("nv12")], "two tables, outputs interleaved")
    assert route == "clip_up_multi<rgb>x2+clip_up_multi<rgb>x2", route
    # (test_chan_multi_gpu.writer registers a table per format: three tables, in the order they first appear)
    route, _ = check_clip(layers, w, h, [out("rgba8", own_table=True), out("v210"), out("bgra8", own_table=True), out("nv12")], "three tables, outputs interleaved")
    assert route == "clip_up_multi<rgb>x1+clip_up_multi<rgb>x2+clip_up_multi<rgb>x1", route
    route, _ = check_clip(layers, w, h, [out("v210", spec="709"), out("yuv422p10", spec="2020"), out("rgba8", spec="sRGB")], "three writer recipes")
    assert route == "+".join(["clip_up_multi<rgb>x1"] * 3), route


def two_stage(route, n_out):
    parts = route.split("+")
    return len(parts) >= 2 and parts[-1] == "compose_up_multi<rgba>x%dj1" % n_out and all("read" in p for p in parts[:-1])


def test_several_layers_and_images_take_two_stages():
    import hip_harness as hh
    w, h = 384, 54
    two = [clip("yuv420p", 128, 36, w, h, 2160), clip("yuv420p", 128, 36, w, h, 2161, scale_x=0.8, scale_y=0.8, offset_x=0.1)]
    route, _ = check_clip(two, w, h, [out("yuv422p8"), out("rgba8")], "two clips")
    assert two_stage(route, 2), route
    mixed = [clip("v210", 126, 36, w, h, 2162), clip("bgra8", 100, 30, w, h, 2163, scale_x=0.6, scale_y=0.7, offset_y=-0.1), clip("p010", 96, 20, w, h, 2164, scale_x=0.5, scale_y=0.5, offset_x=0.2)]
    route, _ = check_clip(mixed, w, h, [out("nv12"), out("v210", 3), out("bgra8", own_table=True)], "three clips of three formats, two tables")
    parts = route.split("+")
    assert parts.count("compose_up_multi<rgba>x2j1") == 1 and parts.count("compose_up_multi<rgba>x1j1") == 1 and len(parts) == 5, route  # (the clips are read once)
    image = [dict(src=Src(frames.rgba_random(128, 36, 2165, -0.05, 1.05), 128, 36, m(w, h), fmt="rgba"))]
    route, _ = check_clip(image, w, h, [out("yuv420p"), out("rgba8")], "a finished image")
    assert route == "compose_up_multi<rgba>x2j1", route
    one = [clip("yuv422p8", 128, 36, w, h, 2166)]
    k = hh.ctx()
    k.set_option("chan_enlarged", 2)
    try:
        route, _ = check_clip(one, w, h, [out("yuv422p8"), out("rgba8")], "one clip, chan_enlarged = 2")
    finally:
        k.set_option("chan_enlarged", 1)
    assert two_stage(route, 2) and len(route.split("+")) == 2, route


def test_what_the_routes_do_not_take_runs_the_channel_kernel():
    import hip_harness as hh
    w, h = 384, 54
    outs = [out("yuv422p8"), out("rgba8")]
    second = Src.random("yuv420p", 128, 36, 2171, m(w, h))
    cases = [("a shrinking placement", [clip("yuv420p", 384, 54, w, h, 2172, scale_x=0.5, scale_y=0.5)]),
             ("a rotated placement", [clip("yuv420p", 128, 36, w, h, 2173, rotate=0.05)]),
             ("a layer in a dissolve", [dict(clip("yuv420p", 128, 36, w, h, 2174), transition="dissolve", mix=0.25, incoming=second)]),
             ("a clip enlarged by less than a field write needs", [clip("yuv420p", 128, 36, w, h, 2175)])]
    for what, layers in cases:
        o = [out("yuv422p8", 1), out("rgba8", 1)] if what.endswith("needs") else outs
        route, _ = check_clip(layers, w, h, o, what)
        assert re.fullmatch(r"chan_compose_multi<\d>x2", route), (what, route)
    k = hh.ctx()
    k.set_option("chan_enlarged", 0)
    try:
        route, _ = check_clip([clip("yuv420p", 128, 36, w, h, 2176)], w, h, outs, "chan_enlarged = 0")
        alone, _ = check_clip([clip("yuv420p", 128, 36, w, h, 2176)], w, h, [out("nv12")], "chan_enlarged = 0, one output")
    finally:
        k.set_option("chan_enlarged", 1)
    assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route
    assert re.fullmatch(r"chan_compose_v210<\d,\d>", alone), alone  # (ph_chan_compose_multi with one output IS ph_chan_compose)


def test_all_three_routes_give_the_same_bytes():
    w, h = 384, 54
    layers = [clip("yuv420p10", 128, 36, w, h, 2180, scale_x=0.9, scale_y=0.9, offset_x=0.05)]
    outs = [out("v210"), out("yuv420p", 3), out("bgra8")]
    seen = []
    both_routes(lambda name: seen.append(check_clip(layers, w, h, outs, "every route: " + name, separate=False)))
    routes = [s[0] for s in seen]
    assert routes[0] == "clip_up_multi<rgb>x3" and two_stage(routes[1], 3) and re.fullmatch(r"chan_compose_multi<\d>x3", routes[2]), routes
    for other in seen[1:]:
        for a, b in zip(seen[0][1], other[1]):
            for pa, pb in zip(a, b):
                assert np.array_equal(pa, pb)


# ---- recipes -----------------------------------------------------------------------------------------------------------------------------
def test_recipes():
    """reader 709 with writer 2020 (the gamut matrix between them); a writer table of the output's own; a source with its own 8-bit matrix"""
    w, h = 384, 54
    layers = [clip("yuv422p10", 128, 36, w, h, 2190)]
    route, _ = check_clip(layers, w, h, [out("v210", spec="2020"), out("yuv422p8", spec="2020"), out("rgba8", spec="2020")], "709 -> 2020", specs=("709", "2020"))
    assert route == "clip_up_multi<rgb>x3", route
    route, _ = check_clip(layers, w, h, [out("nv12", own_table=True)], "a table of the output's own")
    assert route == "clip_up_multi<rgb>x1", route
    eight = clip("yuv420p", 128, 36, w, h, 2191)
    assert eight["src"].own_matrix()  # (col_matrix12: the 8-bit code ranges)
    route, _ = check_clip([eight], w, h, [out("yuv422p10"), out("bgra8")], "a source with its own 8-bit matrix")
    assert route == "clip_up_multi<rgb>x2", route


# ---- by name: clip_compose_multi_<n> -----------------------------------------------------------------------------------------------------
SW, SH = 128, 36


@pytest.fixture
def by_name():
    b = ByName(384, 54)
    yield b
    b.close()


def clip_params(b, planes, fmt="yuv420p"):
    """a one-layer job: a yuv420p clip SW x SH filling the channel, for nv12 (output 0) and rgba8 (1)"""
    capi = b.capi
    bufs = [p if isinstance(p, capi.Buffer) else b.upload(p, svm="coarse") for p in planes]
    o0, o1 = b.planes("nv12"), b.planes("rgba8")
    params = dict(b.recipe, l0In=bufs[0], l0Packing=capi.FORMATS[fmt], l0Width=SW, l0Height=SH, l0Matrix=b.upload(np.asarray(m(b.w, b.h), np.float32)),
                  outPacking=capi.FORMATS["nv12"], output=o0[0], outputC=o0[1], outColMatrix=b.cm8, interlace=0,
                  out1Packing=capi.FORMATS["rgba8"], output1=o1[0], out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    if fmt == "yuv420p":
        params.update(l0InU=bufs[1], l0InV=bufs[2], l0ColMatrix=b.upload(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE["yuv420p"])))
    return params, (o0, o1)


def expect_two(b, comp):
    wlut = orc.linear2gamma_lut("709")
    return [oracle_frame("nv12", comp, b.w, b.h, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["nv12"]), wlut), oracle_frame("rgba8", comp, b.w, b.h, 0, None, wlut)]


def test_by_name_run_program_equals_the_typed_call(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    src = Src.random("yuv420p", SW, SH, 2200, m(w, h))
    params, outs = clip_params(b, src.data)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [w, h])
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == "clip_up_multi<rgb>x2", t.route
    _, typed = check_clip([dict(src=src)], w, h, [out("nv12"), out("rgba8")], "the typed call")
    for i, planes in enumerate(outs):
        for pl, p in enumerate(planes):
            assert np.array_equal(b.read(p), typed[i][pl]), "output %d plane %d" % (i, pl)
    prog.destroy()


def test_by_name_run_programs_keeps_order(by_name):
    """a job that WRITES the clip job's source in front of it and a job that READS its output 1 behind it, in one ph_run_programs call"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    first = frames.v210_random(SW, SH, frames.layer_seed(2210, 0))
    stale = b.upload(np.full(frames.v210_pitch_bytes(SW) * SH, POISON, np.uint8), svm="coarse")  # what the first job overwrites
    last_out = b.planes("v210")[0]
    params, outs = clip_params(b, [stale], fmt="v210")
    del params["l0Packing"]
    b.ctx.wait(capi.QUEUE_LOAD)
    small = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [SW, SH])
    one = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    clip_prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [w, h])
    jobs = [(small, dict(b.recipe, l0In=b.upload(first, svm="coarse"), output=stale)),
            (clip_prog, params),
            (one, dict(b.recipe, l0In=outs[1][0], l0Packing=capi.FORMATS["rgba8"], l0Width=w, l0Height=h, output=last_out))]
    b.ctx.wait(capi.QUEUE_LOAD)
    with capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    launches = t.route.split("+")
    assert launches.count("clip_up_multi<rgb>x2") == 1 and launches[0] != "clip_up_multi<rgb>x2" != launches[-1], t.route  # a launch of its own, in its turn
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    frame0 = np.asarray(orc.v210_write(orc.v210_read(first, SW, SH, *b.rd_o), SW, SH, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(stale).view(np.uint32), frame0.view(np.uint32))
    want = expect_two(b, orc.transform(orc.v210_read(frame0.view(np.uint32), SW, SH, *b.rd_o), m(w, h), w, h))
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    img = packfmt.get("rgba8").oracle_read([want[1][0]], w, h, None, b.rd_o[1], b.rd_o[2])
    last = np.asarray(orc.v210_write(img, w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(last_out).view(np.uint32), last.view(np.uint32))
    small.destroy(), one.destroy(), clip_prog.destroy()


def test_by_name_checks_answer_as_the_typed_call_does(by_name):
    """ph_check_program and ph_run_program give the same code and text, the text names the argument, and it is chan_compose_multi_1's for
    the same defect; a refused job writes nothing"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    params, outs = clip_params(b, Src.random("yuv420p", SW, SH, 2220).data)
    small = b.upload(np.zeros(64, np.uint8))
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [w, h])
    sibling = b.ctx.create_program("phaneron:chan", "chan_compose_multi_1", [w, h])

    def without(d, *names):
        return {k: v for k, v in d.items() if k not in names}
    defects = [(dict(params, out1Packing=99), "out1Packing"), (dict(params, out1Packing=capi.FORMATS["p010"]), "out1Packing"), (dict(params, outPacking=capi.FORMATS["yuv420p10"]), "outPacking"),
               (dict(params, output1=small), "output1"), (without(params, "outputC"), "outputC"), (without(params, "outColMatrix"), "outColMatrix"),
               (without(params, "out1GammaLut"), "out1GammaLut"), (dict(params, interlace1=small), "interlace1"), (without(params, "l0InV"), "l0InV"), (dict(params, l0InU=small), "l0InU")]
    for bad, name in defects:
        texts = []
        for p in (prog, sibling):
            seen = []
            for check_only in (True, False):
                with pytest.raises(capi.PhaneronError) as e:
                    b.ctx.run_program(p, bad, check_only=check_only)
                seen.append(str(e.value))
            assert seen[0] == seen[1], "%s: check %r, run %r" % (name, seen[0], seen[1])
            texts.append(seen[0])
        assert name in texts[0], texts[0]
        assert texts[0].replace("ph_clip_compose_multi", "ph_chan_compose_multi") == texts[1], "%s: %r against the sibling's %r" % (name, texts[0], texts[1])
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    prog.destroy(), sibling.destroy()
