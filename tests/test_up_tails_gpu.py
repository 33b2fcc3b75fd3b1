"""GPU tests (-m gpu) of the context option "up_v210_tails": with 1, a v210 output whose lines end in a tail quad (width % 48 != 0 - 1280,
SDI's 720p frame) stays inside its writer table's launch of the several-outputs kernels of the 2 x 2-block compositor
(ph_compose_up_write_multi, ph_clip_compose_multi, ph_clip_compose_batch_out) instead of being made on its own.  Every plane of every
output is compared, byte for byte over poisoned buffers, with the oracle's frame, with the separate one-output calls and with the same
call under the option's default 0 - the v210 frame's tail-quad words and cleared slots and the lines a field output must not touch
included; the routes are pinned with traces.  Every test sets the option on the shared harness context and puts it back to 0.

Widths (v210 pitch in pixels): 128 (144) - 21 whole quads fill the first 126-column wave step, the two-pixel tail quad opens the second;
104 (144) - a two-pixel tail quad, the second step holds cleared slots only; 136 (144) - a four-pixel tail quad over two lanes;
264 (288) - no tail pixels, four cleared slots, three steps; 50 (96) - no multiple of 8: v210 + rgba8 only; 1280 (1296) - the format."""
import contextlib
import re

import numpy as np
import pytest

import frames
import packfmt
from oracle import orc
from test_chan_gpu import Src, colour, device_layers, m
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned
from test_clip_batch_gpu import check_batch, clips
from test_clip_multi_gpu import check_clip, clip, dry_route, outputs_of, two_stage, v210_route
from test_clip_route_gpu import dry_route as route_dry_route
from test_clip_trans_gpu import dissolve, rnd
import test_up_out_gpu as up_out
import test_up_trans_gpu as up_trans

pytestmark = pytest.mark.gpu

OPTION = "up_v210_tails"


@contextlib.contextmanager
def option(value):
    import hip_harness as hh
    k = hh.ctx()
    k.set_option(OPTION, value)
    try:
        yield k
    finally:
        k.set_option(OPTION, 0)


@pytest.fixture
def tails():
    with option(1) as k:
        yield k


def run_clip(layers, w, h, outs, dry_run=False):
    """one ph_clip_compose_multi call over poisoned planes: (route, planes[output][plane] as bytes)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_d = colour("709", "709")[2]
    _, dst, outputs = outputs_of(outs, w, h)
    with capi.trace(dry_run=dry_run) as t:
        hh.ctx().clip_compose_multi(device_layers(layers), outputs, w, h, *rd_d)
    hh.ctx().wait()
    torch.cuda.synchronize()
    return t.route, [[hh.host(p, np.uint8) for p in d] for d in dst]


def same_planes(got, want, what):
    for i, (g, w_) in enumerate(zip(got, want)):
        for pl, (a, b) in enumerate(zip(g, w_)):
            bad = np.flatnonzero(a != b)
            assert bad.size == 0, "%s: output %d plane %d: %d of %d bytes differ, first at %d" % (what, i, pl, bad.size, a.size, bad[0])


def clip_both(layers, w, h, outs, what, name, comp=None):
    """the call with the option at 1 (the caller's fixture) against the oracle and the separate ph_chan_compose calls, then against the
    same call with the option at 0, whose route is today's; returns the route with 1"""
    import hip_harness as hh
    route, got = check_clip(layers, w, h, outs, what, comp=comp)
    assert re.fullmatch(name, route), (what, route)
    assert dry_route(layers, w, h, outs) == route, what
    k = hh.ctx()
    k.set_option(OPTION, 0)
    try:
        before, want = run_clip(layers, w, h, outs)
    finally:
        k.set_option(OPTION, 1)
    assert "_t<" not in before and len(before.split("+")) > len(route.split("+")), (what, before, route)
    same_planes(got, want, what + " against the option at 0")
    return route


ONE_T = r"clip_up_multi_t<%s>x%d"


# ---- ph_clip_compose_multi --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,sw,sh", [(128, 10, 48, 4), (136, 6, 60, 2)])
def test_every_sibling_format_beside_v210(tails, w, h, sw, sh):
    layers = [clip("yuv420p", sw, sh, w, h, 7100 + w)]
    comp = composite(layers, w, h, colour("709", "709")[0])
    for fmt in packfmt.CHAN_OUT:
        clip_both(layers, w, h, [out("v210"), out(fmt)], "%dx%d v210 + %s" % (w, h, fmt), ONE_T % ("rgb", 2), comp=comp)
        clip_both(layers, w, h, [out(fmt), out("v210")], "%dx%d %s + v210" % (w, h, fmt), ONE_T % ("rgb", 2), comp=comp)


@pytest.mark.parametrize("w,h,sw,sh,fmts", [(104, 6, 40, 2, ["v210", "yuv420p", "bgra8"]), (264, 10, 100, 4, ["nv12", "v210", "yuv422p10"]),
                                            (128, 5, 48, 2, ["v210", "yuv422p8", "rgba8"]), (136, 2, 48, 1, ["rgba8", "v210"]),
                                            (50, 6, 20, 2, ["v210", "rgba8"]), (128, 2, 126, 1, ["v210", "yuv422p8"])])
def test_widths_and_heights(tails, w, h, sw, sh, fmts):
    """the widths of the module's docstring at heights 2, 6, 10 and 5 (odd: no 4:2:0 output)"""
    layers = [clip("yuv422p10", sw, sh, w, h, 7200 + w + h)]
    clip_both(layers, w, h, [out(f) for f in fmts], "%dx%d %r" % (w, h, fmts), ONE_T % ("rgb", len(fmts)))


def test_four_outputs_at_1280(tails):
    w, h = 1280, 10
    layers = [clip("yuv420p", 320, 6, w, h, 7300)]
    clip_both(layers, w, h, [out("v210"), out("yuv422p8"), out("rgba8"), out("nv12")], "four outputs at 1280", ONE_T % ("rgb", 4))


@pytest.mark.parametrize("field", [1, 3])
def test_a_v210_field(tails, field):
    """beside a frame (the whole frame is composed, the field takes the rows of its parity: the other rows keep their poison, as the oracle's
    frame over the same poison does) and with every output a field (that field's rows alone are composed)"""
    w, h = 128, 10
    layers = [clip("yuv422p10", 48, 2, w, h, 7400 + field)]
    comp = composite(layers, w, h, colour("709", "709")[0])
    clip_both(layers, w, h, [out("v210", field), out("rgba8", 0)], "v210 field %d + rgba8 frame" % field, ONE_T % ("rgb", 2), comp=comp)
    clip_both(layers, w, h, [out("v210", field), out("rgba8", field)], "v210 + rgba8, field %d" % field, ONE_T % ("rgb", 2), comp=comp)
    _, got = run_clip(layers, w, h, [out("v210", field), out("rgba8", 0)])
    rows = got[0][0].reshape(h, -1)
    assert np.all(rows[(0 if field == 3 else 1)::2] == POISON) and not np.any(np.all(rows[(1 if field == 3 else 0)::2] == POISON, axis=1))


def test_two_v210_outputs_beside_yuv420p(tails):
    w, h = 136, 6
    layers = [clip("nv12", 48, 2, w, h, 7500)]
    clip_both(layers, w, h, [out("v210", 0), out("yuv420p", 0), out("v210", 3)], "a v210 frame, yuv420p, a v210 field", ONE_T % ("rgb", 3))
    clip_both(layers, w, h, [out("v210", 1), out("v210", 3)], "the two v210 fields of a frame", ONE_T % ("rgb", 2))


@pytest.mark.parametrize("fmt", ["yuv420p", "p010", "bgra8", "v210"])
def test_clip_formats_enlarged_and_under_the_default_fill(tails, fmt):
    w, h = 1280, 10
    inst = "rgba" if fmt == "bgra8" else "rgb"
    outs = [out("v210"), out("rgba8")]
    clip_both([clip(fmt, 320, 6, w, h, 7600)], w, h, outs, "%s 320x6 enlarged" % fmt, ONE_T % (inst, 2))
    clip_both([clip(fmt, w, h, w, h, 7601)], w, h, outs, "%s of the channel's size" % fmt, ONE_T % (inst, 2))


def two_stage_t(route, n_out):
    parts = route.split("+")
    return len(parts) >= 2 and parts[-1] == "compose_up_multi_t<rgba>x%dj1" % n_out and all("read" in p for p in parts[:-1])


def test_two_layers_and_an_image_layer_take_the_two_stage_form(tails):
    w, h = 136, 6
    two = [clip("yuv420p", 48, 2, w, h, 7700), clip("yuv422p8", 48, 2, w, h, 7701, scale_x=0.8, scale_y=0.8, offset_x=0.1)]
    route, got = check_clip(two, w, h, [out("v210"), out("yuv422p8")], "two clips")
    assert two_stage_t(route, 2), route
    with option(0):
        before, want = run_clip(two, w, h, [out("v210"), out("yuv422p8")])
    tails.set_option(OPTION, 1)
    assert before.split("+")[-1] == "compose_up_multi<rgba>x1j1" and "_t<" not in before, before
    same_planes(got, want, "two clips against the option at 0")
    image = [dict(src=Src(frames.rgba_random(48, 2, 7702, -0.05, 1.05), 48, 2, m(w, h), fmt="rgba"))]
    route, _ = check_clip(image, w, h, [out("rgba8"), out("v210", 3)], "a finished image")
    assert route == "compose_up_multi_t<rgba>x2j1", route


# ---- ph_compose_up_write_multi ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
@pytest.mark.parametrize("jobs,interlace,ow,oh", [(1, 0, 1280, 10), (2, 1, 136, 10), (4, 0, 104, 6)], ids=["1-job-1280", "2-fields", "4-jobs"])
def test_compose_up_write_multi(tails, rgb, jobs, interlace, ow, oh):
    """packed-RGB and RGBA images (two layers, the upper one an inset: the border colour takes part), jobs 1, 2 - the two fields of a tick,
    every output a field - and 4: against the oracle, the one-output calls (a v210 output: ph_compose_up_write_v210) and the option at 0"""
    inst = "rgb" if rgb else "rgba"
    specs = [(ow // 2 - 4, max(oh // 4, 1), dict()), (ow // 4, 1, dict(scale_x=0.5, scale_y=0.5, offset_x=0.26, offset_y=-0.1))]
    sets = [up_out.images(ow, oh, specs, rgb, 7800 + 10 * j) for j in range(jobs)]
    dev = [up_out.device_set(s, rgb) for s in sets]
    outs = [out("v210", interlace), out("rgba8", interlace), out("yuv422p8", interlace)]
    route, got = up_out.check(sets, ow, oh, outs, "%d jobs" % jobs, rgb, dev_sets=dev)
    assert route == "compose_up_multi_t<%s>x3j%d" % (inst, jobs), route
    assert up_out.call(dev, ow, oh, outs, rgb, dry_run=True)[0] == route
    with option(0):
        before, want = up_out.call(dev, ow, oh, outs, rgb)
        up_out.separate(sets[0], ow, oh, outs, rgb, got[0])
    tails.set_option(OPTION, 1)
    assert before == "compose_up_write_v210+compose_up_multi<%s>x2j%d" % (inst, jobs), before
    for j in range(jobs):
        same_planes(got[j], want[j], "job %d against the option at 0" % j)


# ---- ph_clip_compose_batch_out ------------------------------------------------------------------------------------------------------------------
def test_three_jobs_share_a_launch_at_1280(tails):
    w, h = 1280, 10
    outs = [out("v210"), out("rgba8")]
    jobs = [(layers, outs) for layers in clips(3, seed=7900, sw=320, sh=6, w=w, h=h)]
    route = check_batch(jobs, w, h, "v210 + rgba8 at 1280")  # (against a ph_chan_compose call per output and the oracle too)
    assert route == "clip_up_multi_t<rgb>x2j3", route
    # a lone v210 output stays what it is
    route = check_batch([(layers, [out("v210")]) for layers in clips(2, seed=7910, sw=320, sh=6, w=w, h=h)], w, h, "a v210 frame alone at 1280")
    assert "clip_up_multi" not in route, route


def tail_params(b, planes):
    """a one-layer job by name: a yuv420p clip filling the channel, for v210 (output 0) and rgba8 (1)"""
    capi = b.capi
    bufs = [b.upload(p, svm="coarse") for p in planes]
    o0, o1 = b.planes("v210"), b.planes("rgba8")
    params = dict(b.recipe, l0In=bufs[0], l0InU=bufs[1], l0InV=bufs[2], l0Packing=capi.FORMATS["yuv420p"], l0Width=320, l0Height=6,
                  l0Matrix=b.upload(np.asarray(m(b.w, b.h), np.float32)), l0ColMatrix=b.upload(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE["yuv420p"])),
                  output=o0[0], interlace=0, out1Packing=capi.FORMATS["rgba8"], output1=o1[0], out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    return params, (o0, o1)


def test_by_name_with_clip_batch():
    """clip_compose_multi_<n> and ph_run_programs with clip_batch call the same functions: they follow the option"""
    b = ByName(1280, 10)
    try:
        prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [b.w, b.h])
        srcs = [Src.random("yuv420p", 320, 6, 7950 + j, m(b.w, b.h)) for j in range(3)]
        jobs, outs = [], []
        for s in srcs:
            params, o = tail_params(b, s.data)
            jobs.append((prog, params)), outs.append(o)
        b.ctx.wait(b.capi.QUEUE_LOAD)
        wlut = orc.linear2gamma_lut("709")
        b.ctx.set_option(OPTION, 1)
        with b.capi.trace() as t:
            b.ctx.run_program(prog, jobs[0][1])
        b.ctx.wait()
        assert t.route == "clip_up_multi_t<rgb>x2", t.route
        b.ctx.set_option("clip_batch", 1)
        with b.capi.trace() as t:
            b.ctx.run_programs(jobs)
        b.ctx.wait()
        assert t.route == "clip_up_multi_t<rgb>x2j3", t.route
        for j, s in enumerate(srcs):
            comp = composite([dict(src=s)], b.w, b.h, b.rd_o)
            want = [oracle_frame("v210", comp, b.w, b.h, 0, orc.rgb2ycbcr_matrix("709"), wlut), oracle_frame("rgba8", comp, b.w, b.h, 0, None, wlut)]
            for i, (planes, wnt) in enumerate(zip(outs[j], want)):
                assert np.array_equal(b.read(planes[0]), wnt[0]), "job %d output %d" % (j, i)
        prog.destroy()
    finally:
        b.close()


# ---- routes ---------------------------------------------------------------------------------------------------------------------------------
def test_what_keeps_todays_route(tails):
    """a v210 output alone with its table, n_out == 1, and every transition and route entry trace with 1 as they do with 0"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 136, 6
    layers = [clip("yuv420p", 48, 2, w, h, 8000)]
    rd_d = colour("709", "709")[2]

    def clip_trans(ls, outs):
        _, _, outputs = outputs_of(outs, w, h)
        with capi.trace(dry_run=True) as t:
            hh.ctx().clip_compose_transition_multi(device_layers(ls), outputs, w, h, *rd_d)
        return t.route

    up_layers = up_out.images(w, h, [(48, 2, dict())], True, 8001)
    up_dev = up_out.device_set(up_layers, True)
    cut = [up_trans.device_layers([up_trans.layer(up_layers[0])], True)]
    mixing = [up_trans.device_layers([up_trans.layer(up_layers[0], "dissolve", 0.25, up_out.images(w, h, [(48, 2, dict())], True, 8002)[0])], True)]
    pair = [out("v210"), out("rgba8")]
    probes = {
        "clip: a v210 output alone with its table": lambda: dry_route(layers, w, h, [out("v210"), out("rgba8", own_table=True)]),
        "clip: n_out == 1": lambda: dry_route(layers, w, h, [out("v210", 1)]),
        "compose_up: a v210 output alone with its table": lambda: up_out.call([up_dev], w, h, [out("v210"), out("rgba8", own_table=True)], True, dry_run=True)[0],
        "compose_up: several jobs, one v210 output": lambda: up_out.call([up_dev, up_dev], w, h, [out("v210")], True, dry_run=True)[0],
        "clip transition: every layer a cut": lambda: clip_trans(layers, pair),
        "clip transition: a dissolve": lambda: clip_trans([dissolve(rnd("yuv420p", 48, 2, 8003, w, h), rnd("yuv420p", 48, 2, 8004, w, h))], pair),
        "clip route": lambda: route_dry_route(layers, w, h, pair),
        "compose_up transition: every layer a cut": lambda: up_trans.call(cut, w, h, pair, True, dry_run=True)[0],
    }
    with_1 = {what: probe() for what, probe in probes.items()}
    tails.set_option(OPTION, 0)
    try:
        with_0 = {what: probe() for what, probe in probes.items()}
    finally:
        tails.set_option(OPTION, 1)
    assert with_1 == with_0
    assert not any("_t<" in r for r in with_1.values()), with_1
    assert with_1["clip: a v210 output alone with its table"] == v210_route(layers, w, h) + "+clip_up_multi<rgb>x1"
    assert with_1["clip: n_out == 1"] == v210_route(layers, w, h, 1)
    assert with_1["compose_up: a v210 output alone with its table"] == "compose_up_write_v210+compose_up_multi<rgb>x1j1"
    assert with_1["compose_up: several jobs, one v210 output"] == "compose_up_write_v210"
    assert with_1["clip transition: every layer a cut"] == v210_route(layers, w, h) + "+clip_up_multi<rgb>x1"
    # the transition kernel has no TAILS form: a tail-width v210 output beside a transition is refused as ever
    with pytest.raises(capi.PhaneronError, match="tail quad"):
        up_trans.call(mixing, w, h, pair, True, dry_run=True)


def test_a_launch_per_table(tails):
    w, h = 128, 10
    layers = [clip("yuv420p", 48, 4, w, h, 8100)]
    route, _ = check_clip(layers, w, h, [out("v210"), out("rgba8", own_table=True), out("yuv422p8"), out("bgra8", own_table=True)], "two tables, outputs interleaved")
    assert route == "clip_up_multi_t<rgb>x2+clip_up_multi<rgb>x1+clip_up_multi<rgb>x1", route  # (a table per format: test_chan_multi_gpu.writer)
    dev = up_out.device_set(up_out.images(w, h, [(48, 4, dict())], True, 8101), True)
    route, _ = up_out.call([dev], w, h, [out("yuv422p8", 0, "709"), out("v210", 0, "2020"), out("v210", 0, "709"), out("bgra8", 0, "2020")], True, dry_run=True)
    assert route == "compose_up_multi_t<rgb>x2j1+compose_up_multi_t<rgb>x2j1", route
    # a width that is a multiple of 48 keeps its names
    assert dry_route([clip("yuv420p", 64, 4, 192, 10, 8102)], 192, 10, [out("v210"), out("rgba8")]) == "clip_up_multi<rgb>x2"


def test_the_default_is_0_and_other_values_are_refused():
    """with 0 the traces are today's; the option takes 0 and 1 only; a dry run writes nothing (dry_route asserts it)"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 136, 6
    layers = [clip("yuv420p", 48, 2, w, h, 8200)]
    outs = [out("v210"), out("rgba8")]
    k = hh.ctx()
    try:
        for bad in (2, -1):
            with pytest.raises(capi.PhaneronError, match=r"error -1: .*up_v210_tails"):
                k.set_option(OPTION, bad)
        assert dry_route(layers, w, h, outs) == v210_route(layers, w, h) + "+clip_up_multi<rgb>x1"  # (a refused value changed nothing)
        k.set_option(OPTION, 1)
        assert dry_route(layers, w, h, outs) == "clip_up_multi_t<rgb>x2"
        k.set_option(OPTION, 0)
        assert dry_route(layers, w, h, outs) == v210_route(layers, w, h) + "+clip_up_multi<rgb>x1"
    finally:
        k.set_option(OPTION, 0)
