"""GPU tests (-m gpu) of ph_clip_compose_transition_multi: file playback through a MIX or WIPE - a layer's src clip dissolving or wiping
into an incoming clip, a wipe through a mask clip - packed for up to four consumers, every source pixel of every clip read once.  Every
plane of every output of every case is compared, byte for byte, in destinations poisoned with 0x5A, with the oracle's chain (format
reader of every present image -> transform of each -> dissolve / wipe -> combine -> format writer) and with a separate ph_chan_compose
call; a dry-run trace must name the route the real call took and write nothing."""
import re

import numpy as np
import pytest

import frames
from oracle import orc
from test_chan_gpu import Src, both_routes, colour, device_layers, m
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned
from test_clip_multi_gpu import ALL_OUT, PLANAR_SIZES, RGB_SIZES, SOURCES, UNIT_FORMATS, clip, outputs_of
from test_clip_multi_gpu import dry_route as cut_route

pytestmark = pytest.mark.gpu

ONE = r"clip_up_trans<(rgb|rgba)>x%d"
W, H = 384, 54


def two_stage(route, n_out, reads=None):
    """the format readers' launches, then ONE launch of the transition compositor (its scratch images are f32 RGBA: <rgba>)"""
    parts = route.split("+")
    return parts[-1] == "compose_up_trans<rgba>x%dj1" % n_out and all("read" in p for p in parts[:-1]) and (reads is None or len(parts) == reads + 1)


def dissolve(src, incoming, mix=0.25):
    return dict(src=src, transition="dissolve", mix=mix, incoming=incoming)


def wipe(src, incoming, mask):
    return dict(src=src, transition="wipe", mix=0.0, incoming=incoming, mask=mask)


def rnd(fmt, sw, sh, seed, w=W, h=H, **kw):
    return Src.random(fmt, sw, sh, seed, m(w, h, **kw))


def check_trans(layers, w, h, outs, what, specs=("709", "709"), separate=True, comp=None):
    """one ph_clip_compose_transition_multi call against the oracle, against separate ph_chan_compose calls and against its own dry run;
    returns (traced route, the frames)"""
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
    with capi.trace(dry_run=True) as dry:
        k.clip_compose_transition_multi(dl, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    assert all((hh.host(p, np.uint8) == POISON).all() for d in dst for p in d), "%s: a dry run wrote" % what
    with capi.trace() as t:
        k.clip_compose_transition_multi(dl, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    assert dry.route == t.route, "%s: the dry run names %s, the call took %s" % (what, dry.route, t.route)
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


# ---- a dissolve to every writer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("partner", ["same", "own"])
def test_a_dissolve_to_every_writer(partner):
    """src 128 x 36 yuv420p; incoming of the same size and placement (the kernel's `same` path: the layer's geometry serves both), or a
    96 x 20 yuv422p10 clip under its own fill; to each writer alone (v210 beside rgba8), at mix 0.25, 0 and 1"""
    src = rnd("yuv420p", 128, 36, 3100)
    incoming = rnd("yuv420p", 128, 36, 3101) if partner == "same" else rnd("yuv422p10", 96, 20, 3102)
    rd_o = colour("709", "709")[0]
    for mix in (0.25, 0.0, 1.0):
        layers = [dissolve(src, incoming, mix)]
        comp = composite(layers, W, H, rd_o)
        for fmt in ALL_OUT:
            outs = [out("v210"), out("rgba8")] if fmt == "v210" else [out(fmt)]
            route, _ = check_trans(layers, W, H, outs, "dissolve %s mix %g -> %s" % (partner, mix, fmt), comp=comp, separate=mix == 0.25)
            assert route == "clip_up_trans<rgb>x%d" % len(outs), route


def test_a_dissolves_alpha_is_a_value():
    """a dissolve mixes alpha like any channel: above a bottom layer, an incoming clip placed partly off screen leaves the layer's alpha at
    `mix` where only src covers the pixel, and the layer below shows through by that much (two layers: the two-stage route)"""
    below = dict(src=rnd("yuv422p8", 128, 36, 3110))
    top = dissolve(rnd("yuv420p", 128, 36, 3111, scale_x=0.8, scale_y=0.8), rnd("nv12", 96, 20, 3112, scale_x=0.7, scale_y=0.7, offset_x=0.4, offset_y=-0.3), 0.25)
    rd_o = colour("709", "709")[0]
    shown = composite([below, top], W, H, rd_o)
    alpha = np.asarray(composite([top], W, H, rd_o)).reshape(H, W, 4)[..., 3]
    assert ((alpha > 0.2) & (alpha < 0.3)).any() and (alpha == 1.0).any() and (alpha == 0.0).any()  # (the test's own shapes show all three)
    route, _ = check_trans([below, top], W, H, [out("yuv422p10"), out("rgba8")], "a dissolve over a layer", comp=shown)
    assert two_stage(route, 2, reads=3), route


# ---- a wipe ------------------------------------------------------------------------------------------------------------------------------
def test_a_wipe_through_a_mask_clip_and_through_an_image():
    src, incoming = rnd("yuv420p", 128, 36, 3120), rnd("yuv422p10", 96, 20, 3121)
    outs = [out("yuv422p8"), out("rgba8")]
    route, _ = check_trans([wipe(src, incoming, rnd("v210", 64, 18, 3122))], W, H, outs, "a wipe, the mask a v210 clip enlarged")
    assert route == "clip_up_trans<rgb>x2", route
    route, _ = check_trans([wipe(src, incoming, rnd("v210", 64, 18, 3122))], W, H, [out("v210"), out("nv12"), out("bgra8"), out("yuv420p", 1)], "a wipe to four outputs")
    assert route == "clip_up_trans<rgb>x4", route
    image = Src(frames.rgba_random(64, 18, 3123, -0.05, 1.05), 64, 18, m(W, H), fmt="rgba")
    route, _ = check_trans([wipe(src, incoming, image)], W, H, outs, "a wipe, the mask an f32 image")
    assert two_stage(route, 2, reads=2), route
    assert route.endswith("+compose_up_trans<rgba>x2j1"), route


def test_a_wipes_partners_of_the_layers_shape_share_its_geometry():
    """the `same` bits one by one: the mask like the layer and the incoming clip not (the incoming clip's geometry replaces the layer's),
    the incoming clip like the layer and the mask not (the layer's geometry is made again behind the mask's), both, neither"""
    src = rnd("yuv420p", 128, 36, 3124, scale_x=0.9, scale_y=0.9, offset_x=0.2)  # (partly off screen)
    like = lambda fmt, seed: Src.random(fmt, src.w, src.h, seed, src.matrix)
    other = lambda fmt, seed: rnd(fmt, 96, 20, seed, offset_y=-0.15)
    for what, incoming, mask in (("mask", other("nv12", 3125), like("yuv422p8", 3126)), ("incoming", like("yuv422p10", 3127), other("v210", 3128)),
                                 ("both", like("p010", 3129), like("yuv420p", 3130)), ("neither", other("yuv420p10", 3131), other("yuv422p8", 3132))):
        route, _ = check_trans([wipe(src, incoming, mask)], W, H, [out("v210"), out("yuv420p")], "a wipe, like the layer: " + what, separate=what == "both")
        assert route == "clip_up_trans<rgb>x2", route


# ---- every source format in every role ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", SOURCES)
def test_every_source_format_as_src_incoming_and_mask(fmt):
    """a wipe of three clips with `fmt` as src, as incoming and as the mask in turn (the others yuv420p, yuv422p10, nv12 of other sizes and
    placements); rgba8 / bgra8 anywhere switches the launch to <rgba>"""
    inst = "rgba" if fmt in ("rgba8", "bgra8") else "rgb"
    others = [("yuv420p", 128, 36, dict()), ("yuv422p10", 96, 20, dict(scale_x=0.9, scale_y=0.9, offset_x=0.05)), ("nv12", 64, 18, dict(offset_y=0.1))]
    for role in range(3):
        images = [rnd(fmt if i == role else f, sw, sh, 3130 + 3 * role + i, **kw) for i, (f, sw, sh, kw) in enumerate(others)]
        route, _ = check_trans([wipe(*images)], W, H, [out("yuv422p8"), out("rgba8")], "%s in role %d of a wipe" % (fmt, role), separate=role == 0)
        assert route == "clip_up_trans<%s>x2" % inst, route
    route, _ = check_trans([dissolve(rnd("yuv420p", 128, 36, 3140), rnd(fmt, 128, 36, 3141), 0.6)], W, H, [out("nv12")], "%s dissolving in" % fmt, separate=False)
    assert route == "clip_up_trans<%s>x1" % inst, route


# ---- which lines are composed ------------------------------------------------------------------------------------------------------------
def small_pair(seed, a="yuv422p10", b="yuv420p"):
    """two clips that a field write still enlarges (by more than 2 vertically), placed differently"""
    return [dissolve(rnd(a, 96, 20, seed), rnd(b, 100, 22, seed + 1, scale_x=0.9, scale_y=0.9, offset_x=-0.05), 0.4)]


def test_one_field_for_every_output_composes_that_field_only():
    route, _ = check_trans(small_pair(3150), W, H, [out("v210", 1), out("yuv420p", 1)], "v210 field 1 + yuv420p field 1")
    assert route == "clip_up_trans<rgb>x2", route
    route, _ = check_trans(small_pair(3152, "nv12", "p010"), W, H, [out("nv12", 3), out("bgra8", 3), out("yuv422p8", 3)], "three outputs, field 3")
    assert route == "clip_up_trans<rgb>x3", route


def test_fields_beside_a_frame():
    route, _ = check_trans(small_pair(3154), W, H, [out("rgba8", 1), out("yuv422p8", 3), out("v210", 0)], "fields 1 and 3 beside a frame")
    assert route == "clip_up_trans<rgb>x3", route


def test_a_420_field_beside_a_420_frame():
    route, _ = check_trans(small_pair(3156, "yuv420p", "yuv420p10"), W, H, [out("yuv420p", 3), out("nv12", 0)], "yuv420p field 3 + nv12 frame")
    assert route == "clip_up_trans<rgb>x2", route


def test_a_clip_enlarged_by_less_than_a_field_write_needs_falls_to_the_channel_kernel():
    """128 x 36 on 384 x 54: enlarged for a frame write, not for a field's 27 lines - as src and as the incoming clip"""
    small, tall = rnd("yuv420p", 96, 20, 3158), rnd("yuv420p", 128, 36, 3159)
    for layers in ([dissolve(tall, small)], [dissolve(small, tall)]):
        route, _ = check_trans(layers, W, H, [out("yuv422p8", 1), out("rgba8", 1)], "a clip too tall for a field write")
        assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route
        route, _ = check_trans(layers, W, H, [out("yuv422p8"), out("rgba8")], "the same clips, a frame write", separate=False)
        assert route == "clip_up_trans<rgb>x2", route


# ---- the kernel's units ------------------------------------------------------------------------------------------------------------------
def eligible_image(r, fmt, ow, oh, step, seed, fill_ok):
    """a clip and a placement the read-once routes take: enlarged by 5 % or more of its fit in both directions per written row (the
    routes ask for 1 %), unrotated; pushed partly off screen or leaving a border; sometimes a frame of the channel's size under the fill"""
    if fill_ok and step == 1 and r.random() < 0.2:
        return Src.random(fmt, ow, oh, seed, m(ow, oh))
    sx, sy = float(r.choice([1.0, 0.8, 0.6])), float(r.choice([1.0, 0.8, 0.6]))
    if int(0.95 * sy * oh / step) < 2:
        sy = 1.0
    sw = max(2, int(min(0.95, r.uniform(0.2, 0.95)) * sx * ow) // 2 * 2)
    sh = max(2, int(min(0.95, r.uniform(0.2, 0.95)) * sy * oh / step) // 2 * 2)
    assert sw <= 0.95 * sx * ow and sh * step <= 0.95 * sy * oh, (sw, sh, ow, oh, sx, sy, step)
    return Src.random(fmt, sw, sh, seed, m(ow, oh, scale_x=sx, scale_y=sy, offset_x=float(r.uniform(-0.3, 0.3)), offset_y=float(r.uniform(-0.3, 0.3))))


@pytest.mark.parametrize("part", range(4))
def test_random_shapes_around_the_kernels_units(part):
    """seeded dissolves and wipes on channels barely wider than one 126-column wave step, with tiles that end mid-frame (1920 x 40 and
    2520 x 12 give several tiles), widths that 126 does not divide, a channel narrower than one step; every image with a size and a
    placement of its own, or the partner with the layer's (`same`); progressive and both fields; now and then an f32 image among the
    partners (two stages).  Every placement generated is eligible, so every case must take one of the two new routes."""
    r = np.random.default_rng(20261021 + part)
    sizes = PLANAR_SIZES + RGB_SIZES
    cases, taken = 10, {"one": 0, "two": 0}
    for case in range(cases):
        ow, oh = sizes[(case + 3 * part) % len(sizes)]
        interlace = int(r.choice([0, 0, 1, 3])) if oh >= 8 else 0
        step = 2 if interlace else 1
        seed = 5600 + 40 * part + 4 * case
        kind = "wipe" if r.random() < 0.4 else "dissolve"
        fmts = [UNIT_FORMATS[int(r.integers(0, len(UNIT_FORMATS)))] for _ in range(3)]
        if r.random() < 0.15:
            fmts[1 + int(r.integers(0, 2 if kind == "wipe" else 1))] = "rgba"
        src = eligible_image(r, fmts[0], ow, oh, step, seed, True)
        if r.random() < 0.3 and fmts[1] != "rgba":  # the playlist's common case: two files of one size under one fill
            incoming = Src.random(fmts[1], src.w, src.h, seed + 1, src.matrix)
        else:
            incoming = eligible_image(r, fmts[1], ow, oh, step, seed + 1, True)
        if kind == "wipe":
            layers = [wipe(src, incoming, eligible_image(r, fmts[2], ow, oh, step, seed + 2, False))]
        else:
            layers = [dissolve(src, incoming, float(r.choice([0.0, 0.25, 0.5, 0.9, 1.0])))]
        outs = [out("yuv422p8", interlace), out("rgba8", interlace)] if (ow, oh) in PLANAR_SIZES else [out("rgba8", interlace), out("bgra8", interlace)]
        specs = [("709", "709"), ("709", "2020")][case % 2]
        outs = [dict(o, spec=specs[1]) for o in outs]
        present = [src, incoming] + ([layers[0]["mask"]] if kind == "wipe" else [])
        what = "units case %d.%d: %s of %s on %dx%d il %d" % (part, case, kind, ["%s %dx%d" % (s.fmt, s.w, s.h) for s in present], ow, oh, interlace)
        route, _ = check_trans(layers, ow, oh, outs, what, specs=specs, separate=case % 3 == 0)
        one = bool(re.fullmatch(ONE % 2, route))
        assert one or two_stage(route, 2), (what, route)
        assert one == all(s.fmt != "rgba" and not (s.fmt in ("yuv420p", "nv12", "yuv420p10", "p010") and s.h % 2) for s in present), (what, route)
        taken["one" if one else "two"] += 1
    assert taken["one"] >= cases // 2, taken


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def test_what_takes_two_stages():
    import hip_harness as hh
    outs = [out("yuv422p8"), out("rgba8")]
    src = rnd("yuv420p", 128, 36, 3160)
    # (a 4:2:0 clip of odd height, which the clip kernel's reader would not take, never gets this far: the test below)
    image = Src(frames.rgba_random(100, 21, 3161, -0.05, 1.05), 100, 21, m(W, H), fmt="rgba")
    route, _ = check_trans([dissolve(src, image, 0.5)], W, H, outs, "an f32 image dissolving in")
    assert two_stage(route, 2, reads=1), route
    route, _ = check_trans([dissolve(image, image, 0.5)], W, H, outs, "two f32 images: nothing to read")
    assert route == "compose_up_trans<rgba>x2j1", route
    k = hh.ctx()
    k.set_option("chan_enlarged", 2)
    try:
        route, _ = check_trans([dissolve(src, rnd("yuv420p", 128, 36, 3162), 0.5)], W, H, outs, "chan_enlarged = 2")
    finally:
        k.set_option("chan_enlarged", 1)
    assert two_stage(route, 2) and len(route.split("+")) in (2, 3), route  # (one batched read where the two frames name one Loader matrix)
    below = dict(src=rnd("yuv422p10", 96, 20, 3163))
    top = dissolve(rnd("yuv420p", 128, 36, 3164, scale_x=0.8, scale_y=0.8), rnd("v210", 126, 36, 3165, scale_x=0.8, scale_y=0.8), 0.5)
    route, _ = check_trans([below, top], W, H, outs, "n == 2 with the top layer dissolving")
    assert two_stage(route, 2, reads=3), route
    route, _ = check_trans([top, below], W, H, outs, "n == 2 with the bottom layer dissolving", separate=False)
    assert two_stage(route, 2, reads=3), route


def test_a_420_partner_of_odd_height_is_refused_as_the_channel_kernel_refuses_it():
    """ph_chan_compose takes no 4:2:0 frame of an odd height, so neither does this entry: its answer is ph_chan_compose_multi's text"""
    import hip_harness as hh
    from phaneron_amd import capi
    odd = Src(Src.random("yuv420p", 100, 22, 3166).data, 100, 21, m(W, H), fmt="yuv420p")
    layers = device_layers([dissolve(rnd("yuv420p", 128, 36, 3167), odd, 0.5)])
    _, dst, outputs = outputs_of([out("yuv422p8"), out("rgba8")], W, H)
    rd_d = colour("709", "709")[2]
    texts = []
    for call in (hh.ctx().clip_compose_transition_multi, hh.ctx().chan_compose_multi):
        with pytest.raises(capi.PhaneronError) as e:
            call(layers, outputs, W, H, *rd_d)
        texts.append(str(e.value))
    assert "incoming source is a yuv420p frame" in texts[0] and texts[0] == texts[1], texts
    assert all((hh.host(p, np.uint8) == POISON).all() for d in dst for p in d), "a refused call wrote"


def test_what_the_routes_do_not_take_runs_the_channel_kernel():
    import hip_harness as hh
    outs = [out("yuv422p8"), out("rgba8")]
    src = rnd("yuv420p", 128, 36, 3170)
    cases = [("a rotated partner", [dissolve(src, rnd("yuv420p", 128, 36, 3171, rotate=0.05))]),
             ("a shrinking partner", [dissolve(src, rnd("yuv420p", 384, 54, 3172, scale_x=0.5, scale_y=0.5))]),
             ("a shrinking mask", [wipe(src, rnd("yuv420p", 128, 36, 3173), rnd("v210", 384, 54, 3174, scale_x=0.7, scale_y=0.7))]),
             ("a rotated src", [dissolve(rnd("yuv420p", 128, 36, 3175, rotate=-0.05), src)]),
             ("a mirrored partner", [dissolve(src, rnd("yuv420p", 128, 36, 3176, scale_x=-1.0))])]
    for what, layers in cases:
        route, _ = check_trans(layers, W, H, outs, what)
        assert re.fullmatch(r"chan_compose_multi<\d>x2", route), (what, route)
    k = hh.ctx()
    k.set_option("chan_enlarged", 0)
    try:
        route, _ = check_trans([dissolve(src, rnd("yuv420p", 128, 36, 3177))], W, H, outs, "chan_enlarged = 0")
    finally:
        k.set_option("chan_enlarged", 1)
    assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route


def test_all_cuts_is_ph_clip_compose_multi():
    for layers, outs in (([clip("yuv420p", 128, 36, W, H, 3180)], [out("nv12"), out("rgba8")]),
                         ([clip("yuv420p", 128, 36, W, H, 3181), clip("bgra8", 100, 30, W, H, 3182, scale_x=0.6, scale_y=0.7)], [out("yuv422p8")]),
                         ([clip("yuv420p", 128, 36, W, H, 3183)], [out("v210")]),
                         ([clip("yuv420p", 128, 36, W, H, 3184, rotate=0.1)], [out("v210"), out("rgba8")])):
        route, _ = check_trans(layers, W, H, outs, "every layer a cut")
        assert route == cut_route(layers, W, H, outs), route
    assert cut_route([clip("yuv420p", 128, 36, W, H, 3180)], W, H, [out("nv12"), out("rgba8")]) == "clip_up_multi<rgb>x2"


def test_a_launch_per_writer_table():
    layers = [dissolve(rnd("nv12", 128, 36, 3190), rnd("yuv422p8", 96, 20, 3191), 0.3)]
    route, _ = check_trans(layers, W, H, [out("yuv422p8"), out("rgba8", own_table=True)], "two tables")
    assert route == "clip_up_trans<rgb>x1+clip_up_trans<rgb>x1", route
    route, _ = check_trans(layers, W, H, [out("rgba8", own_table=True), out("v210"), out("rgba8", own_table=True), out("nv12")], "two tables, outputs interleaved")
    assert route == "clip_up_trans<rgb>x2+clip_up_trans<rgb>x2", route
    image = Src(frames.rgba_random(64, 18, 3192, -0.05, 1.05), 64, 18, m(W, H), fmt="rgba")
    route, _ = check_trans([wipe(layers[0]["src"], layers[0]["incoming"], image)], W, H, [out("yuv422p10", spec="2020"), out("v210", spec="709"), out("bgra8", spec="2020")],
                           "two writer recipes, two stages: the clips are read once")
    parts = route.split("+")
    assert len(parts) == 4 and parts[2:] == ["compose_up_trans<rgba>x2j1", "compose_up_trans<rgba>x1j1"] and all("read" in p for p in parts[:2]), route


def v210_route(layers, w, h, interlace=0):
    """what ph_chan_compose makes of a v210 frame of these layers"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    _, _, rd_d, wr_d = colour("709", "709")
    with capi.trace(dry_run=True) as t:
        hh.ctx().chan_compose_v210(device_layers(layers), torch.zeros(frames.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda"), w, h, interlace, *rd_d, *wr_d)
    return t.route


def test_a_v210_output_whose_lines_end_in_a_tail_quad_is_split_off():
    """width 400 (400 % 48 != 0): the v210 frame by the channel kernel (its tail quad truncates table indices), the rest by the new launch"""
    w, h = 400, 10
    layers = [dissolve(rnd("yuv420p", 100, 6, 3200, w, h), rnd("yuv422p10", 120, 8, 3201, w, h), 0.5)]
    alone = v210_route(layers, w, h)
    assert re.fullmatch(r"chan_compose_v210<\d,\d>", alone), alone
    route, _ = check_trans(layers, w, h, [out("v210"), out("rgba8")], "v210 + rgba8 at 400")
    assert route == alone + "+clip_up_trans<rgb>x1", route
    route, _ = check_trans(layers, w, h, [out("rgba8"), out("v210", 1), out("bgra8")], "rgba8 + v210 field 1 + bgra8 at 400")
    assert route == v210_route(layers, w, h, 1) + "+clip_up_trans<rgb>x2", route
    w = 1280
    layers = [wipe(rnd("yuv420p", 320, 6, 3202, w, h), rnd("nv12", 320, 6, 3203, w, h), rnd("v210", 126, 4, 3204, w, h))]
    route, _ = check_trans(layers, w, h, [out("yuv422p8"), out("v210")], "yuv422p8 + v210 at 1280")
    assert route == v210_route(layers, w, h) + "+clip_up_trans<rgb>x1", route


def test_all_three_routes_give_the_same_bytes():
    layers = [wipe(rnd("yuv420p10", 128, 36, 3210, scale_x=0.9, scale_y=0.9, offset_x=0.05), rnd("bgra8", 100, 30, 3211), rnd("v210", 64, 18, 3212, offset_x=-0.1))]
    outs = [out("v210"), out("yuv420p", 3), out("bgra8")]
    seen = []
    both_routes(lambda name: seen.append(check_trans(layers, W, H, outs, "every route: " + name, separate=False)))
    routes = [s[0] for s in seen]
    assert routes[0] == "clip_up_trans<rgba>x3" and two_stage(routes[1], 3, reads=3) and re.fullmatch(r"chan_compose_multi<\d>x3", routes[2]), routes
    for other in seen[1:]:
        for a, b in zip(seen[0][1], other[1]):
            for pa, pb in zip(a, b):
                assert np.array_equal(pa, pb)


def test_recipes():
    """reader 709 with writer 2020 (the gamut matrix between them); partners with 8-bit matrices of their own beside a 10-bit src"""
    layers = [dissolve(rnd("yuv422p10", 128, 36, 3220), rnd("yuv420p", 96, 20, 3221), 0.7)]
    assert layers[0]["incoming"].own_matrix() and not layers[0]["src"].own_matrix()
    route, _ = check_trans(layers, W, H, [out("v210", spec="2020"), out("yuv422p8", spec="2020"), out("rgba8", spec="2020")], "709 -> 2020", specs=("709", "2020"))
    assert route == "clip_up_trans<rgb>x3", route


# ---- by name: clip_compose_trans_<n> -----------------------------------------------------------------------------------------------------
SW, SH = 128, 36


@pytest.fixture
def by_name():
    b = ByName(W, H)
    yield b
    b.close()


def trans_params(b, src, incoming, mix):
    """a one-layer job: a yuv420p clip dissolving into another, for nv12 (output 0) and rgba8 (1)"""
    capi = b.capi
    o0, o1 = b.planes("nv12"), b.planes("rgba8")
    own = b.upload(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE["yuv420p"]))
    params = dict(b.recipe, l0Transition=1, l0Mix=mix, outPacking=capi.FORMATS["nv12"], output=o0[0], outputC=o0[1], outColMatrix=b.cm8, interlace=0,
                  out1Packing=capi.FORMATS["rgba8"], output1=o1[0], out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    for role, s in (("", src), ("Incoming", incoming)):
        bufs = [b.upload(p, svm="coarse") for p in s.data]
        params.update({"l0%sIn" % role: bufs[0], "l0%sInU" % role: bufs[1], "l0%sInV" % role: bufs[2], "l0%sPacking" % role: capi.FORMATS["yuv420p"],
                       "l0%sWidth" % role: s.w, "l0%sHeight" % role: s.h, "l0%sMatrix" % role: b.upload(np.asarray(s.matrix, np.float32)), "l0%sColMatrix" % role: own})
    return params, (o0, o1)


def test_by_name_run_programs_equals_the_typed_call(by_name):
    b = by_name
    src, incoming = rnd("yuv420p", SW, SH, 3230), rnd("yuv420p", 96, 20, 3231, scale_x=0.9, scale_y=0.9)
    params, outs = trans_params(b, src, incoming, 0.25)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_trans_1", [W, H])
    with b.capi.trace() as t:
        b.ctx.run_programs([(prog, params)])
    b.ctx.wait()
    assert t.route == "clip_up_trans<rgb>x2", t.route
    _, typed = check_trans([dissolve(src, incoming, 0.25)], W, H, [out("nv12"), out("rgba8")], "the typed call")
    for i, planes in enumerate(outs):
        for pl, p in enumerate(planes):
            assert np.array_equal(b.read(p), typed[i][pl]), "output %d plane %d" % (i, pl)
    prog.destroy()


def test_by_name_a_refused_job_writes_nothing(by_name):
    b = by_name
    capi = b.capi
    params, outs = trans_params(b, rnd("yuv420p", SW, SH, 3240), rnd("yuv420p", 96, 20, 3241), 0.5)
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_trans_1", [W, H])

    def without(d, *names):
        return {k: v for k, v in d.items() if k not in names}
    for bad, name in ((dict(params, out1Packing=capi.FORMATS["p010"]), "out1Packing"), (without(params, "l0IncomingIn"), "l0IncomingIn"), (dict(params, l0Transition=7), "transition 7"),
                      (without(params, "l0IncomingInV"), "l0IncomingInV")):
        for run in (lambda: b.ctx.run_program(prog, bad), lambda: b.ctx.run_programs([(prog, bad)])):
            with pytest.raises(capi.PhaneronError) as e:
                run()
            assert name in str(e.value), str(e.value)
    b.ctx.wait()
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    prog.destroy()
