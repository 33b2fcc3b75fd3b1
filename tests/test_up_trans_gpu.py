"""GPU tests (-m gpu) of ph_compose_up_transition_multi: dissolves and wipes inside the 2 x 2-block compositor's launch.  Every plane of
every output is compared, byte for byte, with the oracle's chain transform.ts -> transition.ts (dissolve / wipe) -> combine.ts -> the
format's writer over planes poisoned with 0x5A."""
import re

import numpy as np
import pytest

import frames
import guard
from oracle import orc
from test_chan_multi_gpu import ALL_OUT, POISON, oracle_frame, out, poisoned, writer
from test_up_gpu import m, opaque
from test_up_out_gpu import device_set, images, outputs_of, same

pytestmark = pytest.mark.gpu

V420 = ("yuv420p", "nv12")
LAYOUTS = pytest.mark.parametrize("rgb", [False, True], ids=["rgba", "packed-rgb"])
# the layers of a 384 x 108 frame, bottom to top: a 2x full-frame image, then insets that leave the layers below them in sight
STACK = [(192, 54, dict()), (96, 27, dict(scale_x=0.5, scale_y=0.5, offset_x=-0.2, offset_y=0.15)),
         (64, 20, dict(scale_x=0.5, scale_y=0.5, offset_x=0.25, offset_y=-0.2)), (48, 15, dict(scale_x=0.5, scale_y=0.5, offset_x=0.1, offset_y=0.2))]


def layer(src, kind="cut", mix=0.0, incoming=None, mask=None):
    """a layer as the tests carry it: its images are (h x w x 4 array, matrix) pairs"""
    return dict(src=src, transition=kind, mix=mix, incoming=incoming, mask=mask)


def stack(ow, oh, specs, rgb, seed, transitions):
    """specs: per layer (width, height, placement); transitions: {layer index: (kind, mix)} - the partners have the layer's size and
    placement (other seeds)"""
    srcs, ins, masks = images(ow, oh, specs, rgb, seed), images(ow, oh, specs, rgb, seed + 100), images(ow, oh, specs, rgb, seed + 200)
    layers = []
    for i, s in enumerate(srcs):
        kind, mix = transitions.get(i, ("cut", 0.0))
        layers.append(layer(s, kind, mix, ins[i] if kind != "cut" else None, masks[i] if kind == "wipe" else None))
    return layers


def composite(layers, ow, oh):
    placed = []
    for L in layers:
        t = orc.transform(*L["src"], ow, oh)
        if L["transition"] == "dissolve":
            t = orc.transition_dissolve(t, orc.transform(*L["incoming"], ow, oh), L["mix"])
        elif L["transition"] == "wipe":
            t = orc.transition_wipe(t, orc.transform(*L["incoming"], ow, oh), orc.transform(*L["mask"], ow, oh))
        placed.append(t)
    return placed[0] if len(placed) == 1 else orc.combine(placed)


def device_layers(layers, rgb, put=None):
    """the layers with their images on the device, as capi.Context.compose_up_transition_multi takes them"""
    put = put or (lambda pair: device_set([pair], rgb)[0])
    return [dict(L, **{k: put(L[k]) for k in ("src", "incoming", "mask") if L[k] is not None}) for L in layers]


def call(dev_sets, ow, oh, outs, rgb, dry_run=False, dst=None):
    """one ph_compose_up_transition_multi call over poisoned planes: (route, planes[job][output][plane] as bytes)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    dst = dst or [[[hh.dev(p) for p in poisoned(o["fmt"], ow, oh)] for o in outs] for _ in dev_sets]
    with capi.trace(dry_run=dry_run) as t:
        k.compose_up_transition_multi(dev_sets, [outputs_of(outs, d) for d in dst], ow, oh, rgb=rgb)
    k.wait()
    torch.cuda.synchronize()
    return t.route, [[[hh.host(p, np.uint8) for p in d] for d in job] for job in dst]


def check(sets, ow, oh, outs, what, rgb, comps=None, dev_sets=None):
    """the call against the oracle, every job and output; returns (route, planes)"""
    comps = comps or [composite(s, ow, oh) for s in sets]
    dev_sets = dev_sets or [device_layers(s, rgb) for s in sets]
    route, got = call(dev_sets, ow, oh, outs, rgb)
    for j, comp in enumerate(comps):
        for i, o in enumerate(outs):
            rc = writer(o["fmt"], o["spec"], o["own_table"])
            same(got[j][i], oracle_frame(o["fmt"], comp, ow, oh, o["interlace"], rc[0], rc[1]), "%s: job %d output %d (%s il %d)" % (what, j, i, o["fmt"], o["interlace"]))
    return route, got


def name_of(rgb, n_out, jobs=1):
    return "compose_up_trans<%s>x%dj%d" % ("rgb" if rgb else "rgba", n_out, jobs)


def check_each_format(layers, ow, oh, what, rgb, interlace=0, formats=ALL_OUT):
    comp, dev = composite(layers, ow, oh), device_layers(layers, rgb)
    for fmt in formats:
        route, _ = check([layers], ow, oh, [out(fmt, interlace)], "%s %s" % (what, fmt), rgb, [comp], [dev])
        assert route == name_of(rgb, 1), route  # (a v210 output alone with its table too: the one-output kernel has no transitions)


WHERE = {"dissolve-bottom-of-2": (2, {0: ("dissolve", 0.3)}), "dissolve-top-of-2": (2, {1: ("dissolve", 0.7)}), "dissolve-middle-of-4": (4, {1: ("dissolve", 0.45)}),
         "wipe-middle-of-4": (4, {2: ("wipe", 0.0)}), "every-layer-of-4": (4, {0: ("dissolve", 0.25), 1: ("wipe", 0.0), 2: ("dissolve", 0.6), 3: ("wipe", 0.0)})}


@LAYOUTS
@pytest.mark.parametrize("where", list(WHERE))
def test_every_format(where, rgb):
    """384 = 3 wave steps of 126 + 6 columns: planar 8-sample groups straddle every step boundary and the last step is short"""
    n, transitions = WHERE[where]
    check_each_format(stack(384, 108, STACK[:n], rgb, 10, transitions), 384, 108, where, rgb)


@LAYOUTS
def test_one_layer_is_the_combiners_passthrough(rgb):
    for kind in ("dissolve", "wipe"):
        check_each_format(stack(384, 108, STACK[:1], rgb, 15, {0: (kind, 0.4)}), 384, 108, "one layer " + kind, rgb, formats=["v210", "yuv420p", "bgra8"])


@LAYOUTS
def test_mix_values(rgb):
    """0 and 1 (one side alone), values that round ((1 - mix) is rounded once), and mixes outside [0, 1], where a dissolve of two
    opaque pixels has no alpha of exactly 1 to rely on; the incoming image is an inset, so the border's alpha 0 is mixed as well"""
    ow, oh = 384, 108
    base = stack(ow, oh, STACK[:2], rgb, 20, {})
    incoming = images(ow, oh, [STACK[3]], rgb, 21)[0]
    full = images(ow, oh, [STACK[0]], rgb, 22)[0]
    outs = [out("v210"), out("rgba8")]
    for mix in (0.0, 1.0, 0.5, 1.0 / 3.0, 24.0 / 25.0, -0.25, 1.25):
        mix = float(np.float32(mix))
        layers = [layer(base[0]["src"], "dissolve", mix, full), layer(base[1]["src"], "dissolve", mix, incoming)]
        route, _ = check([layers], ow, oh, outs, "mix %r" % mix, rgb)
        assert route == name_of(rgb, 2), route


def unlike(ow, oh, rgb, seed):
    """partners that have another size and placement than their layer, and ones that have the same"""
    src = images(ow, oh, STACK[:3], rgb, seed)
    inset = images(ow, oh, [(48, 15, dict(scale_x=0.5, scale_y=0.5, offset_x=-0.25, offset_y=0.2))], rgb, seed + 1)[0]  # 4x, inset
    off = images(ow, oh, [(64, 20, dict(scale_x=0.5, scale_y=0.5, offset_x=0.4, offset_y=-0.4))], rgb, seed + 2)[0]  # partly off screen
    mask_fill = images(ow, oh, [(ow, oh, dict())], rgb, seed + 3)[0]  # the output's size under the identity
    mask_2x = images(ow, oh, [(ow // 2, oh // 2, dict())], rgb, seed + 4)[0]
    twin = images(ow, oh, [STACK[1]], rgb, seed + 5)[0]  # layer 1's size and placement
    twin_mask = images(ow, oh, [STACK[1]], rgb, seed + 6)[0]
    return {
        "incoming-4x-inset": [layer(src[0], "dissolve", 0.35, inset), layer(src[1])],
        "incoming-partly-off-screen": [layer(src[0]), layer(src[1], "dissolve", 0.6, off), layer(src[2])],
        "mask-of-the-output-size": [layer(src[0]), layer(src[1], "wipe", 0.0, inset, mask_fill)],
        "mask-2x-incoming-like-the-layer": [layer(src[0]), layer(src[1], "wipe", 0.0, twin, mask_2x), layer(src[2])],
        "partners-like-the-layer": [layer(src[0]), layer(src[1], "wipe", 0.0, twin, twin_mask), layer(src[2], "dissolve", 0.5, images(ow, oh, [STACK[2]], rgb, seed + 7)[0])],
        "mask-like-the-layer-incoming-not": [layer(src[0]), layer(src[1], "wipe", 0.0, off, twin_mask)],
    }


@LAYOUTS
@pytest.mark.parametrize("which", ["incoming-4x-inset", "incoming-partly-off-screen", "mask-of-the-output-size", "mask-2x-incoming-like-the-layer", "partners-like-the-layer",
                                   "mask-like-the-layer-incoming-not"])
def test_partners_unlike_their_layer(which, rgb):
    ow, oh = 384, 108
    outs = [out("v210"), out("yuv420p"), out("rgba8")]
    route, _ = check([unlike(ow, oh, rgb, 30)[which]], ow, oh, outs, which, rgb)
    assert route == name_of(rgb, 3), route


FIELD = [(96, 13, dict()), (48, 6, dict(scale_x=0.5, scale_y=0.5, offset_x=0.2))]


@pytest.mark.parametrize("interlace", [1, 3])
def test_fields(interlace):
    """27 field rows (the last row is its own partner); a 4:2:0 field writes all 27 chroma rows from its own lines; the other field's
    luma rows keep the poison"""
    ow, oh = 192, 54
    layers = stack(ow, oh, FIELD, True, 40, {0: ("dissolve", 0.4), 1: ("wipe", 0.0)})
    check_each_format(layers, ow, oh, "interlace %d" % interlace, True, interlace)
    _, got = call([device_layers(layers, True)], ow, oh, [out("yuv420p", interlace)], True)
    y = got[0][0][0].reshape(oh, ow)
    assert np.all(y[(0 if interlace == 3 else 1)::2] == POISON) and not np.all(y[(1 if interlace == 3 else 0)::2] == POISON)
    assert not np.any(np.all(got[0][0][1].reshape(oh // 2, ow // 2) == POISON, axis=1)), "a chroma row was not written"


@pytest.mark.parametrize("ow,oh,sw,sh", [(48, 6, 24, 3), (192, 7, 96, 3), (336, 10, 100, 4), (3840, 26, 1920, 13)])
def test_shapes(ow, oh, sw, sh):
    """a row shorter than a step, an odd height (not for 4:2:0), rows that end in a short step, a frame smaller than the chip"""
    specs = [(sw, sh, dict()), (sw // 2, max(sh // 2, 1), dict(scale_x=0.5, scale_y=0.5, offset_x=-0.2, offset_y=0.1))]
    layers = stack(ow, oh, specs, True, 50, {0: ("wipe", 0.0), 1: ("dissolve", 0.55)})
    check_each_format(layers, ow, oh, "%dx%d" % (ow, oh), True, formats=[f for f in ALL_OUT if not (oh & 1 and f in V420)])


def test_rgb8_at_a_width_that_is_no_multiple_of_8():
    layers = stack(100, 8, [(40, 4, dict())], True, 55, {0: ("dissolve", 0.5)})
    check_each_format(layers, 100, 8, "100x8", True, formats=["rgba8", "bgra8"])


def separate(layers, ow, oh, outs, rgb, got):
    """every output of a several-outputs call equals the call made for it alone"""
    dev = device_layers(layers, rgb)
    for i, o in enumerate(outs):
        _, alone = call([dev], ow, oh, [o], rgb)
        for pl in range(len(alone[0][0])):
            assert np.array_equal(got[i][pl], alone[0][0][pl]), "output %d (%s) plane %d differs from its own call" % (i, o["fmt"], pl)


SEVERAL = [[out("v210"), out("bgra8")], [out("v210"), out("yuv422p8"), out("rgba8")], [out("yuv420p"), out("nv12"), out("yuv422p10"), out("bgra8")],
           [out("v210", 1), out("rgba8", 0)], [out("yuv420p", 3), out("v210", 0), out("yuv422p8", 1)]]


@pytest.mark.parametrize("outs", SEVERAL, ids=["+".join("%s.%d" % (o["fmt"], o["interlace"]) for o in outs) for outs in SEVERAL])
@LAYOUTS
def test_several_outputs(outs, rgb):
    """the last two: outputs that want different lines - the whole frame is composed, a field output takes the rows of its parity (4x:
    a field's rows alone and the frame's rows both qualify)"""
    ow, oh = 192, 54
    layers = stack(ow, oh, FIELD, rgb, 60, {0: ("dissolve", 0.3), 1: ("wipe", 0.0)})
    route, got = check([layers], ow, oh, outs, "several", rgb)
    assert route == name_of(rgb, len(outs)), route
    separate(layers, ow, oh, outs, rgb, got[0])


def test_outputs_with_different_tables_are_a_launch_per_table():
    ow, oh = 384, 108
    layers = stack(ow, oh, STACK[:2], True, 65, {1: ("dissolve", 0.5)})
    outs = [out("yuv422p8", 0, "709"), out("bgra8", 0, "2020"), out("rgba8", 0, "709"), out("v210", 0, "2020")]
    route, got = check([layers], ow, oh, outs, "two tables", True)
    assert route == name_of(True, 2) + "+" + name_of(True, 2), route
    separate(layers, ow, oh, outs, True, got[0])
    # a v210 output alone with its table is a launch of this kernel too
    route, _ = check([layers], ow, oh, [out("v210", 0, "709"), out("yuv422p8", 0, "709", own_table=True)], "own table", True)
    assert route == name_of(True, 1) + "+" + name_of(True, 1), route


@pytest.mark.parametrize("jobs,outs", [(2, [out("v210"), out("bgra8")]), (4, [out("yuv422p8"), out("nv12")]), (2, [out("v210", 1), out("yuv420p", 1)])], ids=["2x2", "4x2", "2x2-fields"])
def test_jobs(jobs, outs):
    """sets of layers that differ in their data and their mix values, each with its own planes: against the oracle and the one-job calls"""
    ow, oh = 192, 54
    sets = [stack(ow, oh, FIELD, True, 70 + 10 * j, {0: ("dissolve", 0.2 + 0.15 * j), 1: ("wipe", 0.0)}) for j in range(jobs)]
    dev = [device_layers(s, True) for s in sets]
    route, got = check(sets, ow, oh, outs, "%d jobs" % jobs, True, dev_sets=dev)
    assert route == name_of(True, len(outs), jobs), route
    for j in range(jobs):
        _, alone = call([dev[j]], ow, oh, outs, True)
        for i in range(len(outs)):
            for pl in range(len(alone[0][i])):
                assert np.array_equal(got[j][i][pl], alone[0][i][pl]), "job %d output %d plane %d differs from the one-job call" % (j, i, pl)


def test_routes():
    """every layer a cut: ph_compose_up_write_multi's routes and bytes; a transition: this kernel's name; a dry run writes nothing"""
    import test_up_out_gpu as tu
    ow, oh = 384, 108
    plain = images(ow, oh, STACK[:2], True, 80)
    dev = device_set(plain, True)
    for outs in ([out("v210")], [out("v210"), out("yuv420p"), out("bgra8", 0, "2020")], [out("yuv422p8")]):
        want_route, want = tu.call([dev], ow, oh, outs, True)
        for as_dicts in (False, True):
            route, got = call([[dict(src=d) for d in dev] if as_dicts else dev], ow, oh, outs, True)
            assert route == want_route, (route, want_route)
            for i in range(len(outs)):
                for pl in range(len(want[0][i])):
                    assert np.array_equal(got[0][i][pl], want[0][i][pl])
    assert tu.call([dev], ow, oh, [out("v210")], True)[0] == "compose_up_write_v210"
    layers = device_layers(stack(ow, oh, STACK[:2], True, 81, {0: ("dissolve", 0.5)}), True)
    outs = [out("v210"), out("yuv420p"), out("bgra8", 0, "2020")]
    wet, _ = call([layers], ow, oh, outs, True)
    dry, planes = call([layers], ow, oh, outs, True, dry_run=True)
    assert dry == wet == name_of(True, 2) + "+" + name_of(True, 1), (dry, wet)
    assert re.fullmatch(r"compose_up_trans<rgba?>x[1-4]j[1-4](\+compose_up_trans<rgba?>x[1-4]j[1-4])*", wet)
    assert all(np.all(p == POISON) for d in planes[0] for p in d), "a dry run wrote to a plane"


@LAYOUTS
def test_the_channel_kernel_makes_the_same_frames(rgb):
    """ph_chan_compose_multi on the same layers given as PH_SRC_RGBA_F32 sources (packed images: unpacked, alpha 1)"""
    import torch
    import hip_harness as hh
    ow, oh = 384, 108
    layers = unlike(ow, oh, rgb, 90)["partners-like-the-layer"]
    layers[0] = layer(layers[0]["src"], "dissolve", 1.0 / 3.0, images(ow, oh, [(48, 15, dict(scale_x=0.5, scale_y=0.5, offset_x=-0.25, offset_y=0.2))], rgb, 91)[0])
    outs = [out("v210"), out("yuv420p", 1), out("bgra8")]
    _, got = check([layers], ow, oh, outs, "cross-check", rgb)
    src = lambda pair: (hh.dev(pair[0].reshape(-1)), pair[0].shape[1], pair[0].shape[0], pair[1], "rgba")
    chan = [dict(src=src(L["src"]), transition=L["transition"], mix=L["mix"], incoming=L["incoming"] and src(L["incoming"]), mask=L["mask"] and src(L["mask"])) for L in layers]
    dst = [[hh.dev(p) for p in poisoned(o["fmt"], ow, oh)] for o in outs]
    k = hh.ctx()
    k.chan_compose_multi(chan, outputs_of(outs, dst), ow, oh, *hh.ColourParams.reader("709", "709"))
    k.wait()
    torch.cuda.synchronize()
    for i, d in enumerate(dst):
        for pl, p in enumerate(d):
            assert np.array_equal(got[0][i][pl], hh.host(p, np.uint8)), "output %d plane %d differs from ph_chan_compose_multi" % (i, pl)


@LAYOUTS
def test_between_guard_bands(rgb):
    """every image, partner, mask and output plane between guards: no byte is written outside a plane, and no tap is read where the
    border colour belongs (a source guard holds NaNs: one tap of it and the frame differs from the oracle's)"""
    import hip_harness as hh
    guard.reset()
    try:
        for ow, oh, jobs in ((48, 6, 1), (336, 10, 2), (384, 108, 1)):
            texel = 12 if rgb else 16
            put = lambda pair: (guard.dev((np.ascontiguousarray(pair[0][..., :3]) if rgb else pair[0]).reshape(-1), "src", pitch=pair[0].shape[1] * texel), pair[0].shape[1], pair[0].shape[0], pair[1])
            specs = [(ow // 2, oh // 2, dict()), (max(ow // 8, 2), max(oh // 4, 1), dict(scale_x=0.5, scale_y=0.5, offset_x=0.3, offset_y=-0.3))]
            sets = []
            for j in range(jobs):
                s = stack(ow, oh, specs, rgb, 100 + 10 * j, {0: ("wipe", 0.0), 1: ("dissolve", 0.4 + 0.1 * j)})
                s[0]["incoming"] = images(ow, oh, [specs[1]], rgb, 105 + 10 * j)[0]  # partly off screen, unlike its layer
                sets.append(s)
            outs = [out("v210"), out("yuv420p"), out("rgba8")]
            dst = [[[guard.dev(p, "dst", pitch=max(p.size // oh, 1)) for p in poisoned(o["fmt"], ow, oh)] for o in outs] for _ in sets]
            route, got = call([device_layers(s, rgb, put) for s in sets], ow, oh, outs, rgb, dst=dst)
            assert route == name_of(rgb, 3, jobs), route
            for j, s in enumerate(sets):
                comp = composite(s, ow, oh)
                for i, o in enumerate(outs):
                    rc = writer(o["fmt"], o["spec"])
                    same(got[j][i], oracle_frame(o["fmt"], comp, ow, oh, 0, rc[0], rc[1]), "guards %dx%d job %d %s" % (ow, oh, j, o["fmt"]))
            n_src, n_dst = guard.check()
            assert n_src >= 5 * jobs and n_dst >= 5 * jobs
            guard.reset()
        hh.ctx().wait()
    finally:
        guard.reset()


def refused(match, dev_sets, ow, oh, outs, rgb=True):
    """the call raises with `match`, and no plane was touched"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    dst = [[[hh.dev(p) for p in poisoned(o["fmt"], ow, oh)] for o in outs] for _ in dev_sets]
    for dry_run in (True, False):
        with pytest.raises(capi.PhaneronError, match=match):
            with capi.trace(dry_run=True) if dry_run else capi.trace():
                k.compose_up_transition_multi(dev_sets, [outputs_of(outs, d) for d in dst], ow, oh, rgb=rgb)
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
    good = device_layers(stack(ow, oh, FIELD, True, 120, {0: ("dissolve", 0.5), 1: ("wipe", 0.0)}), True)
    both = [out("v210"), out("rgba8")]
    src = good[0]["src"]
    for kw in (dict(rotate=0.1), dict(flip_h=True), dict(scale_x=0.25, scale_y=0.25)):  # a partner that is rotated, mirrored, reduced (4 texels per pixel)
        bad = (src[0], src[1], src[2], m(ow, oh, **kw))
        refused("must be enlarged", [[dict(good[0], incoming=bad), good[1]]], ow, oh, both)
        refused("must be enlarged", [[good[0], dict(good[1], mask=bad)]], ow, oh, both)
        refused("must be enlarged", [[dict(good[0], src=bad), good[1]]], ow, oh, both)
    twice = device_set(images(ow, oh, [(96, 27, dict())], True, 123), True)[0]  # 2x: a field's rows are a texel apart
    refused("must be enlarged", [[dict(good[0], incoming=twice), good[1]]], ow, oh, [out("yuv422p8", 1), out("rgba8", 1)])
    refused("transition 3", [[dict(good[0], transition=3), good[1]]], ow, oh, both)
    refused("transition -1", [[dict(good[0], transition=-1), good[1]]], ow, oh, both)
    refused("incoming image is missing", [[dict(good[0], incoming=None), good[1]]], ow, oh, both)
    refused("mask image is missing", [[good[0], dict(good[1], mask=None)]], ow, oh, both)
    refused("another transition than job 0", [good, [good[0], dict(good[1], transition="dissolve")]], ow, oh, both)
    other = device_set(images(ow, oh, [(48, 13, dict())], True, 121), True)[0]
    refused("differs from job 0's in more than its data", [good, [dict(good[0], incoming=other), good[1]]], ow, oh, both)
    refused("1..4 jobs", [good] * 5, ow, oh, both)
    for fmt in ("yuv420p10", "p010"):
        with pytest.raises(capi.PhaneronError, match="does not write %s frames" % fmt):
            d = hh.dev(poisoned("v210", ow, oh)[0])
            hh.ctx().compose_up_transition_multi([good], [[dict(fmt=fmt, planes=[d, d, d], interlace=0, wr_cm=writer("yuv422p10", "709")[2], wr_lut=writer("v210", "709")[3])]], ow, oh, rgb=True)
    refused("odd", [good], 191, oh, [out("rgba8")])
    small = device_layers(stack(100, 8, [(40, 4, dict())], True, 122, {0: ("dissolve", 0.5)}), True)
    refused("tail quad", [small], 100, 8, [out("rgba8"), out("v210")])
    refused("multiple of 8", [small], 100, 8, [out("rgba8"), out("yuv422p8")])
    plain = hh.dev(capi.linear2gamma_lut("709"))
    with pytest.raises(capi.PhaneronError, match="no LDS form"):
        d = hh.dev(poisoned("rgba8", ow, oh)[0])
        hh.ctx().compose_up_transition_multi([good], [[dict(fmt="rgba8", planes=d, interlace=0, wr_lut=plain)]], ow, oh, rgb=True)
    # a frame without lines is nothing to do
    hh.ctx().compose_up_transition_multi([good], [outputs_of([out("rgba8")], [[hh.dev(np.zeros(4, np.uint8))]])], ow, 0, rgb=True)


# ---- by name: compose_up_trans_<n> through ph_run_program / ph_run_programs ------------------------------------------------------
def named_params(b, layers, twin=None):
    """compose_up_multi_<n>'s arguments for packed images, with the transition keys chan_compose_v210_<n> uses"""
    up = lambda pair: b.upload(np.ascontiguousarray(pair[0][..., :3]), svm="coarse")
    p = dict(packedRgb=1)
    for i, L in enumerate(layers):
        for role, key in (("", "src"), ("Incoming", "incoming"), ("Mask", "mask")):
            if L[key] is None:
                continue
            img, mat = L[key]
            p["l%d%sIn" % (i, role)] = up(L[key])
            p["l%d%sWidth" % (i, role)], p["l%d%sHeight" % (i, role)] = img.shape[1], img.shape[0]
            p["l%d%sMatrix" % (i, role)] = b.upload(np.ascontiguousarray(mat, np.float32))
            if twin:
                p["l%d%sIn2" % (i, role)] = up(twin[i][key])
        p["l%dTransition" % i] = {"cut": 0, "dissolve": 1, "wipe": 2}[L["transition"]]
        p["l%dMix" % i] = L["mix"]
        if twin:
            p["l%dMix2" % i] = twin[i]["mix"]
    return p


def named_outputs(b, prefix="output"):
    """v210 (output 0) and yuv422p8, field 1 (output 1): the planes by their argument names"""
    o0, o1 = b.planes("v210"), b.planes("yuv422p8")
    one = prefix + "1"
    return {prefix: o0[0], one: o1[0], one + "U": o1[1], one + "V": o1[2]}, (o0, o1)


def named_recipe(b):
    return dict(outColMatrix=b.recipe["outColMatrix"], outGammaLut=b.recipe["outGammaLut"], interlace=0,
                out1Packing=b.capi.FORMATS["yuv422p8"], out1ColMatrix=b.cm8, out1GammaLut=b.recipe["outGammaLut"], interlace1=1)


def named_compare(b, outs, comp, ow, oh, what):
    wlut = orc.linear2gamma_lut("709")
    want = [oracle_frame("v210", comp, ow, oh, 0, orc.rgb2ycbcr_matrix("709"), wlut),
            oracle_frame("yuv422p8", comp, ow, oh, 1, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["yuv422p8"]), wlut)]
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), np.asarray(x).reshape(-1).view(np.uint8)), "%s: output %d plane %d" % (what, i, pl)


def test_by_name_with_its_twin():
    from test_chan_multi_gpu import ByName
    ow, oh = 192, 54
    b = ByName(ow, oh)
    try:
        first = stack(ow, oh, FIELD, True, 300, {0: ("dissolve", 0.25), 1: ("wipe", 0.0)})
        second = stack(ow, oh, FIELD, True, 310, {0: ("dissolve", 0.75), 1: ("wipe", 0.0)})
        names, outs = named_outputs(b)
        params = dict(named_params(b, first), **named_recipe(b), **names)
        b.ctx.wait(b.capi.QUEUE_LOAD)
        prog = b.ctx.create_program("phaneron:up", "compose_up_trans_2", [ow, oh])
        b.ctx.run_program(prog, params, check_only=True)
        for p in outs[0] + outs[1]:
            assert (b.read(p) == POISON).all(), "a dry run wrote"
        with b.capi.trace() as t:
            b.ctx.run_program(prog, params)
        b.ctx.wait()
        assert t.route == name_of(True, 2), t.route
        named_compare(b, outs, composite(first, ow, oh), ow, oh, "one job")
        # both fields of a tick in one launch, each with its own mix, through ph_run_programs
        names, outs = named_outputs(b)
        twin_names, twin_outs = named_outputs(b, "twinOutput")
        params = dict(named_params(b, first, second), **named_recipe(b), **names, **twin_names)
        b.ctx.wait(b.capi.QUEUE_LOAD)
        with b.capi.trace() as t:
            b.ctx.run_programs([(prog, params)])
        b.ctx.wait()
        assert t.route == name_of(True, 2, 2), t.route
        named_compare(b, outs, composite(first, ow, oh), ow, oh, "first job")
        named_compare(b, twin_outs, composite(second, ow, oh), ow, oh, "twin")
        # ph_check_program fails where the run does, with the run's words
        names, outs = named_outputs(b)
        params = dict(named_params(b, first), **named_recipe(b), **names)
        b.ctx.wait(b.capi.QUEUE_LOAD)
        defects = [({k: v for k, v in params.items() if k != "l0IncomingIn"}, "l0IncomingIn"), ({k: v for k, v in params.items() if k != "l1MaskMatrix"}, "l1MaskMatrix"),
                   (dict(params, l1Transition=3), "l1Transition"), (dict(params, l1MaskWidth=4000), "l1MaskIn"), ({k: v for k, v in params.items() if k != "out1GammaLut"}, "out1GammaLut")]
        for job, name in defects:
            seen = []
            for check_only in (True, False):
                with pytest.raises(b.capi.PhaneronError) as e:
                    b.ctx.run_program(prog, job, check_only=check_only)
                seen.append(str(e.value))
            assert seen[0] == seen[1] and "'%s'" % name in seen[0], seen
        for p in outs[0] + outs[1]:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
        prog.destroy()
    finally:
        b.close()
