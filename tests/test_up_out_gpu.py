"""GPU tests (-m gpu) of ph_compose_up_write_multi: the 2 x 2-block compositor with every writer the channel kernel has and up to four
outputs per launch.  Every plane of every output is compared, byte for byte, with the oracle's chain transform.ts -> combine.ts -> the
format's writer over planes poisoned with 0x5A; v210 outputs also with ph_compose_up_write_v210."""
import re

import numpy as np
import pytest

import frames
from oracle import orc
from test_chan_multi_gpu import ALL_OUT, POISON, oracle_frame, out, poisoned, writer
from test_up_gpu import m, opaque

pytestmark = pytest.mark.gpu

V420 = ("yuv420p", "nv12")
INSETS = [(192, 60, dict()), (48, 15, dict(scale_x=0.5, scale_y=0.5, offset_x=-0.25, offset_y=0.2)),
          (64, 20, dict(scale_x=0.5, scale_y=0.5, offset_x=0.3, offset_y=-0.3)), (96, 24, dict(scale_x=0.625, scale_y=0.5, offset_x=0.05, offset_y=0.1))]


def images(ow, oh, specs, rgb, seed):
    """specs: [(source width, source height, placement)] -> [(h x w x 4 image, matrix)]; packed RGB implies alpha 1"""
    mk = opaque if rgb else (lambda w, h, s: frames.rgba_random(w, h, s, -0.05, 1.05).reshape(h, w, 4))
    return [(mk(sw, sh, seed + i), m(ow, oh, **kw)) for i, (sw, sh, kw) in enumerate(specs)]


def composite(layers, ow, oh):
    placed = [orc.transform(img, mat, ow, oh) for img, mat in layers]
    return placed[0] if len(placed) == 1 else orc.combine(placed)


def device_set(layers, rgb):
    import hip_harness as hh
    return [(hh.dev((np.ascontiguousarray(img[..., :3]) if rgb else img).reshape(-1)), img.shape[1], img.shape[0], mat) for img, mat in layers]


def outputs_of(outs, dst):
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    return [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, dst, recipes)]


def call(dev_sets, ow, oh, outs, rgb, dry_run=False):
    """one ph_compose_up_write_multi call over poisoned planes: (route, planes[job][output][plane] as bytes)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    dst = [[[hh.dev(p) for p in poisoned(o["fmt"], ow, oh)] for o in outs] for _ in dev_sets]
    with capi.trace(dry_run=dry_run) as t:
        k.compose_up_write_multi(dev_sets, [outputs_of(outs, d) for d in dst], ow, oh, rgb=rgb)
    k.wait()
    torch.cuda.synchronize()
    return t.route, [[[hh.host(p, np.uint8) for p in d] for d in job] for job in dst]


def same(got, want, what):
    for pl, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != np.asarray(w).reshape(-1).view(np.uint8))
        assert bad.size == 0, "%s plane %d: %d of %d bytes differ, first at %d" % (what, pl, bad.size, g.size, bad[0])


def check(sets, ow, oh, outs, what, rgb, comps=None, dev_sets=None):
    """the call against the oracle, every job and output; returns (route, planes)"""
    comps = comps or [composite(s, ow, oh) for s in sets]
    dev_sets = dev_sets or [device_set(s, rgb) for s in sets]
    route, got = call(dev_sets, ow, oh, outs, rgb)
    for j, comp in enumerate(comps):
        for i, o in enumerate(outs):
            rc = writer(o["fmt"], o["spec"], o["own_table"])
            same(got[j][i], oracle_frame(o["fmt"], comp, ow, oh, o["interlace"], rc[0], rc[1]), "%s: job %d output %d (%s il %d)" % (what, j, i, o["fmt"], o["interlace"]))
    return route, got


def check_each_format(layers, ow, oh, what, rgb, interlace=0, formats=ALL_OUT):
    comp, dev = composite(layers, ow, oh), device_set(layers, rgb)
    for fmt in formats:
        route, _ = check([layers], ow, oh, [out(fmt, interlace)], "%s %s" % (what, fmt), rgb, [comp], [dev])
        assert route == ("compose_up_write_v210" if fmt == "v210" else "compose_up_multi<%s>x1j1" % ("rgb" if rgb else "rgba")), route


@pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_every_format_one_output(n, rgb):
    """384 = 3 wave steps of 126 + 6 columns: planar 8-sample groups straddle every step boundary and the last step is short"""
    sw, sh, ow, oh = 192, 54, 384, 108
    check_each_format(images(ow, oh, [(sw, sh, dict())] * n, rgb, 10), ow, oh, "%d layers 2x" % n, rgb)


@pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
def test_insets_and_borders(rgb):
    """2x, 4x inset, 3x partly off screen, 2.5x: the border colour and its alpha 0 take part"""
    ow, oh = 384, 120
    check_each_format(images(ow, oh, INSETS, rgb, 1), ow, oh, "insets", rgb)


@pytest.mark.parametrize("interlace", [1, 3])
def test_fields(interlace):
    """27 field rows (the last row is its own partner); a 4:2:0 field writes all 27 chroma rows from its own lines; the other field's
    luma rows keep the poison (the oracle wrote over the same poison)"""
    ow, oh = 192, 54
    layers = images(ow, oh, [(96, 13, dict()), (48, 6, dict(scale_x=0.5, scale_y=0.5, offset_x=0.2))], True, 20)
    check_each_format(layers, ow, oh, "interlace %d" % interlace, True, interlace)
    _, got = call([device_set(layers, True)], ow, oh, [out("yuv420p", interlace)], True)
    y = got[0][0][0].reshape(oh, ow)
    assert np.all(y[(0 if interlace == 3 else 1)::2] == POISON) and not np.all(y[(1 if interlace == 3 else 0)::2] == POISON)
    assert not np.any(np.all(got[0][0][1].reshape(oh // 2, ow // 2) == POISON, axis=1)), "a chroma row was not written"


@pytest.mark.parametrize("ow,oh,sw,sh", [(48, 6, 24, 3), (192, 7, 96, 3), (336, 10, 100, 4), (3840, 26, 1920, 13)])
def test_shapes(ow, oh, sw, sh):
    """a row shorter than a step, an odd height (not for 4:2:0), rows that end in a short step, a frame smaller than the chip"""
    layers = images(ow, oh, [(sw, sh, dict()), (sw // 2, max(sh // 2, 1), dict(scale_x=0.5, scale_y=0.5, offset_x=-0.2, offset_y=0.1))], True, 30)
    check_each_format(layers, ow, oh, "%dx%d" % (ow, oh), True, formats=[f for f in ALL_OUT if not (oh & 1 and f in V420)])


def test_rgb8_at_a_width_that_is_no_multiple_of_8():
    layers = images(100, 8, [(40, 4, dict())], True, 33)
    check_each_format(layers, 100, 8, "100x8", True, formats=["rgba8", "bgra8"])


def separate(layers, ow, oh, outs, rgb, got):
    """every output of a several-outputs call equals the call made for it alone; a v210 one equals ph_compose_up_write_v210"""
    import hip_harness as hh
    dev = device_set(layers, rgb)
    for i, o in enumerate(outs):
        _, alone = call([dev], ow, oh, [o], rgb)
        for pl in range(len(alone[0][0])):
            assert np.array_equal(got[i][pl], alone[0][0][pl]), "output %d (%s) plane %d differs from its own call" % (i, o["fmt"], pl)
        if o["fmt"] == "v210":
            rc = writer("v210", o["spec"], o["own_table"])
            frame = hh.dev(poisoned("v210", ow, oh)[0])
            hh.ctx().compose_up_write_v210(dev, frame, ow, oh, o["interlace"], rc[2], rc[3], rgb=rgb)
            assert np.array_equal(got[i][0], hh.host(frame, np.uint8)), "output %d differs from ph_compose_up_write_v210" % i


SEVERAL = [[out("v210"), out("bgra8")], [out("v210"), out("yuv422p8"), out("rgba8")], [out("yuv420p"), out("nv12"), out("yuv422p10"), out("bgra8")]]


@pytest.mark.parametrize("outs", SEVERAL, ids=["+".join(o["fmt"] for o in outs) for outs in SEVERAL])
@pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
def test_several_outputs(outs, rgb):
    ow, oh = 384, 120
    layers = images(ow, oh, INSETS, rgb, 40)
    route, got = check([layers], ow, oh, outs, "several", rgb)
    assert route == "compose_up_multi<%s>x%dj1" % ("rgb" if rgb else "rgba", len(outs)), route
    separate(layers, ow, oh, outs, rgb, got[0])


@pytest.mark.parametrize("outs", [[out("v210", 1), out("rgba8", 0)], [out("yuv420p", 3), out("v210", 0)]], ids=["v210-field+rgba8", "yuv420p-field+v210"])
def test_a_field_beside_a_frame(outs):
    """outputs that want different lines: the whole frame is composed and the field output takes the rows of its parity (4x: a field's
    rows alone and the frame's rows both qualify)"""
    ow, oh = 192, 54
    layers = images(ow, oh, [(96, 13, dict()), (48, 6, dict(scale_x=0.5, scale_y=0.5, offset_x=0.2))], True, 50)
    route, got = check([layers], ow, oh, outs, "field beside frame", True)
    assert route == "compose_up_multi<rgb>x2j1", route
    separate(layers, ow, oh, outs, True, got[0])


@pytest.mark.parametrize("interlace", [0, 1, 3])
def test_v210_inside_the_several_outputs_kernel_from_rgba_images(interlace):
    """the new kernel's own v210 writer (126-column steps) on RGBA images with borders, frames and fields"""
    ow, oh = 192, 54
    layers = images(ow, oh, [(96, 13, dict()), (48, 6, dict(scale_x=0.5, scale_y=0.5, offset_x=0.2))], False, 55)
    outs = [out("v210", interlace), out("yuv422p8", interlace)]
    route, got = check([layers], ow, oh, outs, "v210 il %d" % interlace, False)
    assert route == "compose_up_multi<rgba>x2j1", route
    separate(layers, ow, oh, outs, False, got[0])


def test_outputs_with_different_tables_are_a_launch_per_table():
    ow, oh = 384, 108
    layers = images(ow, oh, [(192, 54, dict())] * 2, True, 60)
    outs = [out("yuv422p8", 0, "709"), out("bgra8", 0, "2020"), out("rgba8", 0, "709"), out("v210", 0, "2020")]
    route, got = check([layers], ow, oh, outs, "two tables", True)
    assert route == "compose_up_multi<rgb>x2j1+compose_up_multi<rgb>x2j1", route
    separate(layers, ow, oh, outs, True, got[0])
    # a table of the same contents under another pointer is another table; a v210 output alone with its table takes today's kernel
    route, _ = check([layers], ow, oh, [out("v210", 0, "709"), out("yuv422p8", 0, "709", own_table=True)], "own table", True)
    assert route == "compose_up_write_v210+compose_up_multi<rgb>x1j1", route


def test_a_v210_tail_quad_beside_a_rounding_writer():
    """1280 % 48 != 0: the v210 writer truncates its table indices in the tail quad where yuv422p8 rounds them - the v210 output is split
    off into a launch of today's kernel, and the trace says so"""
    ow, oh = 1280, 12
    layers = images(ow, oh, [(640, 6, dict()), (320, 3, dict(scale_x=0.5, scale_y=0.5, offset_x=0.26))], True, 70)
    outs = [out("v210"), out("yuv422p8")]
    route, got = check([layers], ow, oh, outs, "tail quad", True)
    assert route == "compose_up_write_v210+compose_up_multi<rgb>x1j1", route
    separate(layers, ow, oh, outs, True, got[0])


@pytest.mark.parametrize("jobs,outs", [(2, [out("v210"), out("bgra8")]), (4, [out("yuv422p8"), out("nv12")]), (2, [out("v210", 1), out("yuv420p", 1), out("rgba8", 1), out("yuv422p10", 1)])],
                         ids=["2x2", "4x2", "2x4-fields"])
def test_jobs(jobs, outs):
    """sets of layers that differ in their data only, each with its own planes: against the oracle and the single-job calls"""
    ow, oh = 384, 108
    sets = [images(ow, oh, [(96, 24, dict()), (48, 12, dict(scale_x=0.5, scale_y=0.5, offset_x=-0.2))], True, 80 + 10 * j) for j in range(jobs)]
    dev = [device_set(s, True) for s in sets]
    route, got = check(sets, ow, oh, outs, "%d jobs" % jobs, True, dev_sets=dev)
    assert route == "compose_up_multi<rgb>x%dj%d" % (len(outs), jobs), route
    for j in range(jobs):
        _, alone = call([dev[j]], ow, oh, outs, True)
        for i in range(len(outs)):
            for pl in range(len(alone[0][i])):
                assert np.array_equal(got[j][i][pl], alone[0][i][pl]), "job %d output %d plane %d differs from the single-job call" % (j, i, pl)


def refused(match, dev_sets, ow, oh, outs, rgb=True, outputs=None):
    """the call raises with `match`, and no plane was touched"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    dst = [[[hh.dev(p) for p in poisoned(o["fmt"], ow, oh)] for o in outs] for _ in dev_sets]
    args = outputs(dst) if outputs else [outputs_of(outs, d) for d in dst]
    with pytest.raises(capi.PhaneronError, match=match):
        k.compose_up_write_multi(dev_sets, args, ow, oh, rgb=rgb)
    k.wait()
    torch.cuda.synchronize()
    for job in dst:
        for d in job:
            for p in d:
                assert np.all(hh.host(p, np.uint8) == POISON), "a refused call wrote to a plane"


def test_refusals():
    import hip_harness as hh
    from phaneron_amd import capi
    ow, oh = 192, 54
    good = device_set(images(ow, oh, [(96, 13, dict())], True, 90), True)
    both = [out("v210"), out("rgba8")]
    for kw in (dict(rotate=0.1), dict(flip_h=True)):
        refused("must be enlarged", [[(good[0][0], 96, 13, m(ow, oh, **kw))]], ow, oh, both)
    refused("must be enlarged", [device_set(images(ow, oh, [(96, 27, dict())], True, 91), True)], ow, oh, [out("yuv422p8", 1), out("rgba8", 1)])  # 2x: a field's rows are a texel apart
    for fmt in ("yuv420p10", "p010"):
        refused("does not write %s frames" % fmt, [good], ow, oh, [dict(fmt=fmt, interlace=0, spec="709", own_table=False), out("rgba8")],
                outputs=lambda dst: [[dict(fmt=fmt, planes=d[0], interlace=0, wr_cm=writer("yuv422p10", "709")[2], wr_lut=writer("v210", "709")[3])] + outputs_of([out("rgba8")], d[1:]) for d in dst])
    small = device_set(images(100, 8, [(40, 4, dict())], True, 92), True)
    refused("multiple of 8", [small], 100, 8, [out("rgba8"), out("yuv422p8")])
    refused("even height", [device_set(images(192, 7, [(96, 3, dict())], True, 93), True)], 192, 7, [out("rgba8"), out("nv12")])
    refused("odd", [good], 191, oh, [out("rgba8")])
    refused("1..4 outputs", [good], ow, oh, [out("rgba8")] * 5, outputs=lambda dst: [outputs_of([out("rgba8")] * 5, d) for d in dst])
    refused("same plane", [good], ow, oh, both, outputs=lambda dst: [outputs_of(both, [d[0], d[0]]) for d in dst])
    refused("same plane", [good, good], ow, oh, both, outputs=lambda dst: [outputs_of(both, dst[0]), outputs_of(both, [dst[1][0], dst[0][1]])])
    plain = hh.dev(capi.linear2gamma_lut("709"))
    refused("no LDS form", [good], ow, oh, both, outputs=lambda dst: [[dict(o, wr_lut=plain) if i else o for i, o in enumerate(outputs_of(both, d))] for d in dst])
    rgba = device_set(images(ow, oh, [(96, 13, dict())], False, 94), False)
    with pytest.raises(capi.PhaneronError, match="another image format"):
        mixed_formats(good, rgba, ow, oh)  # (the binding gives one layout per call: the mixed set is built by hand)
    refused("1..4 jobs", [good] * 5, ow, oh, both)


def mixed_formats(rgb_set, rgba_set, ow, oh):
    """two layers of different image layouts in one set, through the C call"""
    import ctypes as C
    import hip_harness as hh
    from phaneron_amd import capi
    arr = (capi.PhImageLayer * 2)()
    keep = []
    for i, ((t, w, h, mat), f) in enumerate(((rgb_set[0], capi.IMG_RGB_F32), (rgba_set[0], capi.IMG_RGBA_F32))):
        mh = np.ascontiguousarray(mat, np.float32)
        keep.append(mh)
        arr[i].data, arr[i].width, arr[i].height, arr[i].format = t.data_ptr(), w, h, f
        arr[i].matrix9_host = mh.ctypes.data_as(C.POINTER(C.c_float))
    sets = (C.POINTER(capi.PhImageLayer) * 1)(C.cast(arr, C.POINTER(capi.PhImageLayer)))
    dst = hh.dev(poisoned("rgba8", ow, oh)[0])
    o = (capi.PhChanOutput * 1)()
    o[0].format, o[0].interlace, o[0].wr_gamma_lut = capi.FORMATS["rgba8"], 0, writer("rgba8", "709")[3].data_ptr()
    o[0].planes[0] = dst.data_ptr()
    k = hh.ctx()
    try:
        capi.check(capi.lib().ph_compose_up_write_multi(k.h, capi.QUEUE_PROCESS, 1, 2, sets, 1, o, ow, oh), k.h)
    finally:
        assert np.all(hh.host(dst, np.uint8) == POISON)


def test_routes():
    """one v210 output of one job IS ph_compose_up_write_v210; a dry run names the same kernels and writes nothing"""
    import hip_harness as hh
    from phaneron_amd import capi
    ow, oh = 384, 108
    layers = images(ow, oh, [(192, 54, dict())], True, 95)
    dev = device_set(layers, True)
    rc = writer("v210", "709")
    k = hh.ctx()
    frame = hh.dev(poisoned("v210", ow, oh)[0])
    with capi.trace() as t:
        k.compose_up_write_v210(dev, frame, ow, oh, 0, rc[2], rc[3], rgb=True)
    route, got = call([dev], ow, oh, [out("v210")], True)
    assert route == t.route == "compose_up_write_v210"
    assert np.array_equal(got[0][0][0], hh.host(frame, np.uint8))
    outs = [out("v210"), out("yuv420p"), out("bgra8", 0, "2020")]
    wet, _ = call([dev], ow, oh, outs, True)
    dry, planes = call([dev], ow, oh, outs, True, dry_run=True)
    assert dry == wet == "compose_up_multi<rgb>x2j1+compose_up_multi<rgb>x1j1", (dry, wet)
    assert "compose_up_write_v210" not in wet and re.fullmatch(r"compose_up_multi<rgba?>x[1-4]j[1-4](\+compose_up_multi<rgba?>x[1-4]j[1-4])*", wet)
    assert all(np.all(p == POISON) for d in planes[0] for p in d), "a dry run wrote to a plane"


def chan_frame(tensors, sw, sh, ow, oh, o):
    """today's route to a frame that is not v210: the images unpacked, then ph_chan_compose"""
    import hip_harness as hh
    k = hh.ctx()
    rd = hh.ColourParams.reader("709", "709")
    rc = writer(o["fmt"], o["spec"])
    dst = [hh.dev(p) for p in poisoned(o["fmt"], ow, oh)]
    k.chan_compose_v210([dict(src=(t, sw, sh, m(ow, oh), "rgba")) for t in tensors], dst[0] if o["fmt"] == "v210" else dst, ow, oh, o["interlace"], *rd, rc[2], rc[3], out_fmt=o["fmt"])
    return [hh.host(p, np.uint8) for p in dst]


@pytest.mark.parametrize("sw,sh,ow,oh,outs", [(1920, 1080, 1920, 1080, [out("v210"), out("bgra8")]), (1920, 1080, 1920, 1080, [out("yuv422p8")]),
                                                (1920, 1080, 3840, 2160, [out("v210"), out("yuv420p")])], ids=["f3-v210+bgra8", "f3-yuv422p8", "config3-v210+yuv420p"])
def test_full_size_as_benched(sw, sh, ow, oh, outs):
    """four packed-RGB 1080p images under the identity fill (a frame write), at their own size and enlarged 2x: against ph_chan_compose on
    the same images unpacked (pinned to the oracle at this size in test_fullsize_gpu.py) and ph_compose_up_write_v210"""
    import torch
    import hip_harness as hh
    gen = torch.Generator(device="cuda").manual_seed(ow)
    rgba = [torch.rand(sw * sh * 4, device="cuda", generator=gen) * 1.1 - 0.05 for _ in range(4)]
    for im in rgba:
        im.view(-1, 4)[:, 3] = 1.0
    rgb = [im.view(-1, 4)[:, :3].contiguous().view(-1) for im in rgba]
    torch.cuda.synchronize()
    dev = [(t, sw, sh, m(ow, oh)) for t in rgb]
    _, got = call([dev], ow, oh, outs, True)
    for i, o in enumerate(outs):
        if o["fmt"] == "v210":
            rc = writer("v210", o["spec"])
            frame = hh.dev(poisoned("v210", ow, oh)[0])
            hh.ctx().compose_up_write_v210(dev, frame, ow, oh, 0, rc[2], rc[3], rgb=True)
            want = [hh.host(frame, np.uint8)]
            if (sw, sh) == (ow, oh):
                assert np.array_equal(want[0], chan_frame(rgba, sw, sh, ow, oh, o)[0]), "ph_compose_up_write_v210 differs from ph_chan_compose"
        else:
            want = chan_frame(rgba, sw, sh, ow, oh, o)
        for pl, (g, w) in enumerate(zip(got[0][i], want)):
            assert np.array_equal(g, w), "output %d (%s) plane %d" % (i, o["fmt"], pl)
