"""GPU tests (-m gpu) of ph_clip_compose_route_multi: a routed channel's file playback - ph_clip_compose_multi's frames and the combined
f32 RGBA image itself from the read-once launches.  Throughout, the destinations and the image start poisoned (0x5A).  image_out is
compared as uint32 with the oracle's image (format reader -> transform -> combine; one layer: the transformed image): the same NaN
positions, every other value bit-equal, -0 included - only a NaN's payload is unpinned.  Every plane of every output is compared, byte
for byte, with the oracle's writer on that image and with ph_clip_compose_multi's frame on the same arguments; the routes are pinned
with traces."""
import re

import numpy as np
import pytest

import frames
import packfmt
from oracle import orc
from test_chan_gpu import Src, colour, device_layers, m
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned, writer
from test_clip_multi_gpu import PLANAR_SIZES, RGB_SIZES, SOURCES, UNIT_FORMATS, clip, outputs_of, v210_route
from test_fused_route_gpu import poison_image, same_image, specials_image

pytestmark = pytest.mark.gpu

ALL_OUT = ["v210"] + list(packfmt.CHAN_OUT)
ONE = r"clip_up_route<(rgb|rgba)>x%d"
TWO = "compose_up_route<rgba>x%dj1"
W, H = 384, 54


def two_stage(route, n_out, reads=None):
    parts = route.split("+")
    return parts[-1] == TWO % n_out and all("read" in p for p in parts[:-1]) and (reads is None or len(parts) == reads + 1)


def gpu_chain_image(layers, w, h, rd_d):
    """ph_pack_read / ph_v210_read -> ph_transform -> ph_combine on the GPU (one layer: its transformed image)"""
    import hip_harness as hh
    k = hh.ctx()
    placed = []
    for L in layers:
        s = L["src"]
        d = s.device()
        if s.fmt == "rgba":
            img = d[0]
        else:
            img = hh.dev(poison_image(s.w, s.h))
            if s.fmt == "v210":
                k.v210_read(d[0], img, s.w, s.h, *rd_d)
            else:
                f = packfmt.get(s.fmt)
                planes = [d[0]] if f.code_range is None else list(d[0])
                cm = None if f.code_range is None else d[5] if d[5] is not None else rd_d[0]
                k.pack_read(s.fmt, planes, img, s.w, s.h, cm, rd_d[1], rd_d[2])
        t = hh.dev(poison_image(w, h))
        k.transform(img, s.w, s.h, hh.dev(np.asarray(s.matrix, np.float32)), t, w, h)
        placed.append(t)
    if len(placed) == 1:
        return hh.host(placed[0], np.float32)
    t = hh.dev(poison_image(w, h))
    k.combine(placed, t, w, h)
    return hh.host(t, np.float32)


def check_route(layers, w, h, outs, what, specs=("709", "709"), comp=None, sibling=True, chain=False, oracle=True):
    """one ph_clip_compose_route_multi call against the oracle, ph_clip_compose_multi on the same arguments and (chain) the GPU's own
    chain; returns (traced route, the frames, the image)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, _, rd_d, _ = colour(*specs)
    k = hh.ctx()
    dl = device_layers(layers)
    recipes, dst, outputs = outputs_of(outs, w, h)
    image_out = hh.dev(poison_image(w, h))
    with capi.trace() as t:
        k.clip_compose_route_multi(dl, image_out, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8) for p in d] for d in dst]
    image = hh.host(image_out, np.float32).reshape(h, w, 4)
    print("%s: route %s" % (what, t.route))
    if oracle:
        if comp is None:
            comp = composite(layers, w, h, rd_o)
        same_image(image, comp, "%s [%s]: image_out against the oracle's image" % (what, t.route))
        want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
        for i, o in enumerate(outs):
            for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
                bad = np.flatnonzero(g != wnt)
                assert bad.size == 0, "%s [%s]: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d" % (
                    what, t.route, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0])
    if chain:
        same_image(image, gpu_chain_image(layers, w, h, rd_d), "%s: image_out against the reader, ph_transform and ph_combine on the GPU" % what)
    if sibling and outs:
        _, theirs, outputs_theirs = outputs_of(outs, w, h)
        k.clip_compose_multi(dl, outputs_theirs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            for pl, p in enumerate(theirs[i]):
                assert np.array_equal(got[i][pl], hh.host(p, np.uint8)), "%s: output %d (%s) plane %d differs from ph_clip_compose_multi's" % (what, i, o["fmt"], pl)
    return t.route, got, image


def dry_route(layers, w, h, outs, specs=("709", "709")):
    """the route the call would take; a dry run writes nothing"""
    import hip_harness as hh
    from phaneron_amd import capi
    _, _, rd_d, _ = colour(*specs)
    _, dst, outputs = outputs_of(outs, w, h)
    image_out = hh.dev(poison_image(w, h))
    with capi.trace(dry_run=True) as t:
        hh.ctx().clip_compose_route_multi(device_layers(layers), image_out, outputs, w, h, *rd_d)
    assert all((hh.host(p, np.uint8) == POISON).all() for d in dst for p in d) and (hh.host(image_out, np.uint8) == POISON).all(), "a dry run wrote"
    return t.route


# ---- every source format ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sw,sh", [(128, 36), (384, 54)])
@pytest.mark.parametrize("src", SOURCES)
def test_every_source_format(src, sw, sh):
    """a clip 128 x 36 enlarged to 384 x 54, and a 384 x 54 frame under the default fill, to v210 + rgba8 and the image: one launch, <rgba>
    where the source has alpha"""
    layers = [clip(src, sw, sh, W, H, 6100 + sw)]
    outs = [out("v210"), out("rgba8")]
    route, _, _ = check_route(layers, W, H, outs, "%s %dx%d" % (src, sw, sh), chain=True)
    assert route == "clip_up_route<%s>x2" % ("rgba" if src in ("rgba8", "bgra8") else "rgb"), route
    assert dry_route(layers, W, H, outs) == route


# ---- outputs and fields -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_OUT)
def test_each_writer_alone_beside_the_image(fmt):
    """(a lone v210 output belongs to the image's launch too)"""
    route, _, _ = check_route([clip("yuv422p10", 128, 36, W, H, 6110)], W, H, [out(fmt)], "%s alone" % fmt)
    assert route == "clip_up_route<rgb>x1", route


def test_four_outputs():
    for layers in ([clip("yuv420p", 128, 36, W, H, 6120)], [clip("bgra8", 384, 54, W, H, 6121)]):
        route, _, _ = check_route(layers, W, H, [out("v210"), out("yuv422p8"), out("nv12"), out("rgba8")], "four outputs")
        assert re.fullmatch(ONE % 4, route), route


def test_the_image_alone_touches_no_writer_table():
    """n_out == 0: one launch; the two-stage form is the readers' launches and one compositor launch without outputs"""
    route, _, _ = check_route([clip("nv12", 128, 36, W, H, 6130)], W, H, [], "no outputs: one clip", chain=True)
    assert route == "clip_up_route<rgb>x0", route
    route, _, _ = check_route([clip("rgba8", 100, 30, W, H, 6131, scale_x=0.8, scale_y=0.8)], W, H, [], "no outputs: a clip with alpha")
    assert route == "clip_up_route<rgba>x0", route
    two = [clip("yuv420p", 128, 36, W, H, 6132), clip("bgra8", 100, 30, W, H, 6133, scale_x=0.6, scale_y=0.7, offset_y=-0.1)]
    route, _, _ = check_route(two, W, H, [], "no outputs: two clips", chain=True)
    assert two_stage(route, 0, reads=2), route


def test_field_outputs_beside_the_image():
    """the image is whole; the fields take their rows (the other field's rows keep their poison: the oracle writes into poisoned planes)"""
    small = [clip("yuv422p10", 96, 20, W, H, 6140)]
    route, got, _ = check_route(small, W, H, [out("v210", 1), out("rgba8", 3)], "fields 1 and 3")
    assert route == "clip_up_route<rgb>x2", route
    rows = got[1][0].reshape(H, -1)
    assert (rows[0::2] == POISON).all() and not (rows[1::2] == POISON).all()
    route, _, _ = check_route(small, W, H, [out("yuv422p8", 1), out("yuv422p8", 1, own_table=True)], "one field for every output: still the whole image")
    assert route == "clip_up_route<rgb>x1+clip_up_multi<rgb>x1", route
    route, _, _ = check_route([clip("yuv420p", 96, 20, W, H, 6141)], W, H, [out("yuv420p", 3), out("nv12", 0)], "a 4:2:0 field beside a 4:2:0 frame")
    assert route == "clip_up_route<rgb>x2", route
    check_route([clip("p010", 96, 20, W, H, 6142)], W, H, [out("nv12", 1)], "a 4:2:0 field alone")


# ---- clips with alpha ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgba8", "bgra8"])
def test_an_inset_with_alpha_whose_border_shows(fmt):
    layers = [clip(fmt, 100, 30, W, H, 6150, scale_x=0.7, scale_y=0.6, offset_x=0.1, offset_y=-0.05)]
    assert (np.asarray(layers[0]["src"].data[0]).reshape(-1).view(np.uint8)[3::4] < 255).any()  # alpha below 1
    route, _, image = check_route(layers, W, H, [out("v210"), out("bgra8")], "%s inset" % fmt, chain=True)
    assert route == "clip_up_route<rgba>x2", route
    alpha = image[..., 3]
    assert (alpha[0] == 0).all() and (alpha[:, 0] == 0).all() and (alpha > 0).any() and ((alpha > 0) & (alpha < 1)).any()  # the border, the inside, the filtered rim


# ---- two stages ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at", [0, 1, 2])
@pytest.mark.parametrize("fill", [False, True])
def test_two_clips_and_a_special_value_image(at, fill):
    """an f32 image with NaN, Inf and -0 in alpha and red at the bottom, in the middle and on top - enlarged, and of the channel's size
    under the default fill - with two clips: the readers, then one compose_up_route launch"""
    clips = [clip("yuv420p", 128, 36, W, H, 6160), clip("bgra8", 100, 30, W, H, 6161, scale_x=0.6, scale_y=0.7, offset_y=-0.1)]
    sw, sh = (W, H) if fill else (128, 36)
    layers = list(clips)
    layers.insert(at, dict(src=Src(specials_image(sw, sh), sw, sh, m(W, H), fmt="rgba")))
    outs = [out("nv12"), out("v210", 3), out("rgba8")]
    route, _, _ = check_route(layers, W, H, outs, "specials at %d, fill %d" % (at, fill), chain=True)
    assert two_stage(route, 3, reads=2), route
    assert dry_route(layers, W, H, outs) == route


def test_one_clip_in_two_stages():
    import hip_harness as hh
    layers = [clip("yuv422p8", 128, 36, W, H, 6170)]
    outs = [out("yuv422p8"), out("rgba8")]
    _, one, image_one = check_route(layers, W, H, outs, "one launch")
    k = hh.ctx()
    k.set_option("chan_enlarged", 2)
    try:
        route, two, image_two = check_route(layers, W, H, outs, "chan_enlarged = 2")
    finally:
        k.set_option("chan_enlarged", 1)
    assert two_stage(route, 2, reads=1), route
    assert np.array_equal(image_one.view(np.uint32), image_two.view(np.uint32)) and all(np.array_equal(a, b) for x, y in zip(one, two) for a, b in zip(x, y))
    # an image alone, a 4:2:0 clip of an odd height: nothing for the one-launch kernel
    route, _, _ = check_route([dict(src=Src(frames.rgba_random(128, 36, 6171, -0.05, 1.05), 128, 36, m(W, H), fmt="rgba"))], W, H, [out("yuv420p")], "a finished image")
    assert route == TWO % 1, route


# ---- units --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_random_shapes_around_the_kernels_units(part):
    """seeded clips and placements that qualify on channels barely wider than one 126-column wave step, with tiles that end mid-frame,
    widths that 126 does not divide, a channel narrower than one step; placements that push the clip partly off screen or leave a
    border; frame and field outputs.  Every case takes a route launch."""
    r = np.random.default_rng(20261021 + part)
    sizes = PLANAR_SIZES + RGB_SIZES
    for case in range(10):
        ow, oh = sizes[(case + 3 * part) % len(sizes)]
        fmt = UNIT_FORMATS[int(r.integers(0, len(UNIT_FORMATS)))]
        interlace = int(r.choice([0, 0, 1, 3])) if oh % 2 == 0 else 0
        if r.random() < 0.25:
            sw, sh, kw = ow, oh, dict()
        else:
            sw = max(2, int(ow * r.uniform(0.2, 0.5)) // 2 * 2)
            sh = max(2, int(oh * r.uniform(0.2, 0.5)) // 2 * 2)
            kw = dict(scale_x=float(r.choice([1.0, 0.8])), scale_y=float(r.choice([1.0, 0.8])), offset_x=float(r.uniform(-0.3, 0.3)), offset_y=float(r.uniform(-0.3, 0.3)))
        layers = [clip(fmt, sw, sh, ow, oh, 6200 + 16 * part + case, **kw)]
        outs = [out("yuv422p8", interlace), out("rgba8")] if (ow, oh) in PLANAR_SIZES else [out("rgba8"), out("bgra8", interlace)]
        specs = [("709", "709"), ("709", "2020")][case % 2]
        outs = [dict(o, spec=specs[1]) for o in outs]
        what = "units case %d.%d: %s %dx%d on %dx%d il %d %r" % (part, case, fmt, sw, sh, ow, oh, interlace, kw)
        route, _, _ = check_route(layers, ow, oh, outs, what, specs=specs, sibling=case % 3 == 0)
        assert re.fullmatch(ONE % 2, route) or two_stage(route, 2, reads=1), (what, route)


# ---- splits and equivalences --------------------------------------------------------------------------------------------------------------
def test_three_writer_tables_the_image_by_the_first_launch_only():
    layers = [clip("nv12", 128, 36, W, H, 6300)]
    route, _, _ = check_route(layers, W, H, [out("rgba8", own_table=True), out("v210"), out("bgra8", own_table=True), out("nv12")], "three tables, outputs interleaved")
    assert route == "clip_up_route<rgb>x1+clip_up_multi<rgb>x2+clip_up_multi<rgb>x1", route
    two = layers + [clip("yuv420p", 100, 30, W, H, 6301, scale_x=0.6, scale_y=0.7)]
    route, _, _ = check_route(two, W, H, [out("v210", spec="709"), out("yuv422p10", spec="2020"), out("rgba8", spec="sRGB")], "three writer recipes, two stages")
    parts = route.split("+")
    assert parts.count(TWO % 1) == 1 and parts.count("compose_up_multi<rgba>x1j1") == 2 and parts.index(TWO % 1) < parts.index("compose_up_multi<rgba>x1j1"), route


def test_a_1280_wide_v210_output_is_split_off():
    w, h = 1280, 10
    layers = [clip("yuv420p", 320, 6, w, h, 6310)]
    route, _, _ = check_route(layers, w, h, [out("v210"), out("rgba8")], "v210 + rgba8 at 1280")
    assert route == v210_route(layers, w, h) + "+clip_up_route<rgb>x1", route
    route, _, _ = check_route(layers, w, h, [out("v210", 1)], "a v210 field alone at 1280: the image by a launch without outputs")
    assert route == v210_route(layers, w, h, 1) + "+clip_up_route<rgb>x0", route


def test_without_the_image_the_call_is_ph_clip_compose_multi():
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    for layers, outs in (([clip("yuv420p", 128, 36, W, H, 6320)], [out("v210"), out("nv12")]), ([clip("p010", 128, 36, W, H, 6321)], [out("v210", 3)]),
                         ([clip("yuv420p", 384, 54, W, H, 6322, rotate=0.1)], [out("yuv422p8"), out("rgba8")])):
        dl = device_layers(layers)
        seen = []
        for call in (lambda o: k.clip_compose_route_multi(dl, None, o, W, H, *rd_d), lambda o: k.clip_compose_multi(dl, o, W, H, *rd_d)):
            _, dst, outputs = outputs_of(outs, W, H)
            with capi.trace() as t:
                call(outputs)
            k.wait()
            torch.cuda.synchronize()
            seen.append((t.route, [hh.host(p, np.uint8) for d in dst for p in d]))
        assert seen[0][0] == seen[1][0] and "route" not in seen[0][0], seen[0][0]
        assert all(np.array_equal(a, b) for a, b in zip(seen[0][1], seen[1][1]))


def test_both_store_policy_arms_give_equal_bytes():
    import hip_harness as hh
    k = hh.ctx()
    one = [clip("yuv420p10", 128, 36, W, H, 6330, scale_x=0.9, scale_y=0.9, offset_x=0.05)]
    two = one + [clip("rgba8", 100, 30, W, H, 6331, scale_x=0.6, scale_y=0.7)]
    for layers in (one, two):
        seen = []
        for images in (0, 1):
            k.set_option("stream_images", images)
            try:
                assert k.debug_image_nt(W * H * 16) == images
                seen.append(check_route(layers, W, H, [out("v210"), out("yuv420p", 3)], "stream_images = %d" % images, sibling=False))
            finally:
                k.set_option("stream_images", 0)
        assert seen[0][0] == seen[1][0]
        assert np.array_equal(seen[0][2].view(np.uint32), seen[1][2].view(np.uint32)) and all(np.array_equal(a, b) for x, y in zip(seen[0][1], seen[1][1]) for a, b in zip(x, y))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
CHAIN = r"run ph_pack_read, ph_transform, ph_combine and ph_pack_write_multi"


def refused(layers, outs, match, image=None, option=None, w=W, h=H):
    """the call is refused with `match`, launches nothing and writes nothing; image: (device layers, outputs) -> the image_out to pass"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")
    dl = device_layers(layers)
    _, dst, outputs = outputs_of(outs, w, h)
    own = hh.dev(poison_image(w, h))
    image_out = own if image is None else image(dl, outputs)
    tensors = [t for d in dl for t in (d["src"][0] if isinstance(d["src"][0], tuple) else (d["src"][0],))]
    before = [hh.host(t, np.uint8).copy() for t in tensors]
    if option:
        k.set_option(*option)
    try:
        with capi.trace() as t:
            with pytest.raises(capi.PhaneronError, match=match):
                k.clip_compose_route_multi(dl, image_out, outputs, w, h, *rd_d)
    finally:
        if option:
            k.set_option(option[0], 1)
    assert t.route == "", "a refused call launched (%s)" % match
    assert all((hh.host(p, np.uint8) == POISON).all() for d in dst for p in d) and (hh.host(own, np.uint8) == POISON).all(), "a refused call wrote (%s)" % match
    assert all(np.array_equal(a, hh.host(t, np.uint8)) for a, t in zip(before, tensors)), "a refused call wrote a source (%s)" % match


def test_refusals_write_nothing():
    outs = [out("yuv422p8"), out("rgba8")]
    second = Src.random("yuv420p", 128, 36, 6401, m(W, H))
    refused([clip("yuv420p", 384, 54, W, H, 6402, scale_x=0.5, scale_y=0.5)], outs, r"error -1: .*layer 0 is neither enlarged.*" + CHAIN)  # a shrunk clip
    refused([clip("yuv420p", 128, 36, W, H, 6403, rotate=0.05)], outs, r"error -1: .*layer 0 is neither enlarged.*" + CHAIN)
    refused([clip("nv12", 128, 36, W, H, 6404), dict(clip("yuv420p", 128, 36, W, H, 6405), transition="dissolve", mix=0.25, incoming=second)], outs,
            r"error -1: .*layer 1 is in a transition.*" + CHAIN)
    refused([clip("yuv420p", 128, 36, W, H, 6406)], outs, r'error -1: .*"chan_enlarged" = 0.*' + CHAIN, option=("chan_enlarged", 0))
    refused([clip("yuv420p", 128, 36, W, H, 6406)], [], r'error -1: .*"chan_enlarged" = 0.*' + CHAIN, option=("chan_enlarged", 0))


def test_image_out_overlapping_anything_is_refused():
    import torch
    image_bytes = W * H * 16

    def inside(t, off=0):
        """a view that starts `off` bytes into a tensor's storage: image_out = its address"""
        return t.view(torch.uint8).reshape(-1)[off:]
    one = [clip("yuv420p", 128, 36, W, H, 6410)]
    outs = [out("yuv422p8"), out("rgba8")]
    for plane in range(3):
        refused(one, outs, r"error -1: .*image_out overlaps a layer's source", image=lambda dl, o, p=plane: inside(dl[0]["src"][0][p], 16))
    big = [clip("yuv422p10", 128, 36, W, H, 6411), dict(src=Src(frames.rgba_random(W, H, 6412, 0.0, 1.0), W, H, m(W, H), fmt="rgba"))]
    refused(big, outs, r"error -1: .*image_out overlaps a layer's source", image=lambda dl, o: dl[1]["src"][0])
    refused(big, outs, r"error -1: .*image_out overlaps a layer's source", image=lambda dl, o: inside(dl[1]["src"][0], image_bytes - 16))
    import hip_harness as hh

    def into_plane(o, k, p):
        """the plane moved into the middle of one large allocation, the image 64 bytes into it: nothing else lies under the image"""
        big = hh.dev(np.full(3 * image_bytes, POISON, np.uint8))
        planes = list(o[k]["planes"])
        planes[p] = big[image_bytes:image_bytes + planes[p].numel() * planes[p].element_size()]
        o[k]["planes"] = planes
        return big[image_bytes + 64:]
    for k_out, planes in ((0, 3), (1, 1)):
        for p in range(planes):
            refused(one, outs, r"error -1: .*image_out overlaps an output's plane", image=lambda dl, o, k=k_out, p=p: into_plane(o, k, p))


# ---- by name: clip_compose_route_<n> ------------------------------------------------------------------------------------------------------
SW, SH = 128, 36


@pytest.fixture
def by_name():
    b = ByName(W, H)
    yield b
    b.close()


def image_buffer(b):
    """a poisoned image buffer (createBuffer with imageDims): a later job may take it as an f32 RGBA layer"""
    a = np.ascontiguousarray(poison_image(b.w, b.h))
    buf = b.ctx.create_buffer(a.nbytes, "readwrite", "coarse", dims=(b.w, b.h))
    buf.host_access("writeonly", b.capi.QUEUE_LOAD, a)
    b.bufs.append(buf)
    return buf


def route_params(b, planes, fmt="yuv420p"):
    """a one-layer job: a clip SW x SH filling the channel, for nv12 (output 0) and rgba8 (1), and the image"""
    capi = b.capi
    bufs = [p if isinstance(p, capi.Buffer) else b.upload(p, svm="coarse") for p in planes]
    o0, o1 = b.planes("nv12"), b.planes("rgba8")
    image_out = image_buffer(b)
    params = dict(b.recipe, l0In=bufs[0], l0Packing=capi.FORMATS[fmt], l0Width=SW, l0Height=SH, l0Matrix=b.upload(np.asarray(m(b.w, b.h), np.float32)), imageOut=image_out,
                  outPacking=capi.FORMATS["nv12"], output=o0[0], outputC=o0[1], outColMatrix=b.cm8, interlace=0,
                  out1Packing=capi.FORMATS["rgba8"], output1=o1[0], out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    if fmt == "yuv420p":
        params.update(l0InU=bufs[1], l0InV=bufs[2], l0ColMatrix=b.upload(capi.ycbcr2rgb_matrix("709", *capi.FORMAT_RANGE["yuv420p"])))
    return params, (o0, o1), image_out


def test_by_name_run_program_equals_the_typed_call(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    src = Src.random("yuv420p", SW, SH, 6500, m(w, h))
    params, outs, image_out = route_params(b, src.data)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_route_1", [w, h])
    b.ctx.run_program(prog, params, check_only=True)
    assert all((b.read(p) == POISON).all() for planes in outs for p in planes) and (b.read(image_out) == POISON).all(), "a check wrote"
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == "clip_up_route<rgb>x2", t.route
    _, typed, image = check_route([dict(src=src)], w, h, [out("nv12"), out("rgba8")], "the typed call")
    for i, planes in enumerate(outs):
        for pl, p in enumerate(planes):
            assert np.array_equal(b.read(p), typed[i][pl]), "output %d plane %d" % (i, pl)
    same_image(b.read(image_out).view(np.float32), image, "imageOut against the typed call's image")
    # the image alone: no `output` at all
    alone = {k: v for k, v in params.items() if not k.startswith("out") and k not in ("interlace", "interlace1")}
    alone["imageOut"] = only = b.upload(poison_image(w, h), svm="coarse")
    b.ctx.wait(b.capi.QUEUE_LOAD)
    with b.capi.trace() as t:
        b.ctx.run_program(prog, alone)
    b.ctx.wait()
    assert t.route == "clip_up_route<rgb>x0", t.route
    same_image(b.read(only).view(np.float32), image, "imageOut alone against the typed call's image")
    # without imageOut the job is clip_compose_multi_1's
    plain = {k: v for k, v in params.items() if k != "imageOut"}
    with b.capi.trace() as t:
        b.ctx.run_program(prog, plain)
    b.ctx.wait()
    assert t.route == "clip_up_multi<rgb>x2", t.route
    prog.destroy()


def test_by_name_run_programs_keeps_order(by_name):
    """a job that WRITES the route job's source in front of it and a job that READS its imageOut as a layer behind it, in one
    ph_run_programs call: each a launch of its own, in its turn"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    first = frames.v210_random(SW, SH, frames.layer_seed(6510, 0))
    stale = b.upload(np.full(frames.v210_pitch_bytes(SW) * SH, POISON, np.uint8), svm="coarse")  # what the first job overwrites
    last_out = b.planes("v210")[0]
    params, outs, image_out = route_params(b, [stale], fmt="v210")
    del params["l0Packing"]
    b.ctx.wait(capi.QUEUE_LOAD)
    small = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [SW, SH])
    one = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    route_prog = b.ctx.create_program("phaneron:chan", "clip_compose_route_1", [w, h])
    jobs = [(small, dict(b.recipe, l0In=b.upload(first, svm="coarse"), output=stale)),
            (route_prog, params),
            (one, dict(b.recipe, l0In=image_out, output=last_out))]
    with capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    launches = t.route.split("+")
    assert launches.count("clip_up_route<rgb>x2") == 1 and launches[0] != "clip_up_route<rgb>x2" != launches[-1], t.route
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    frame0 = np.asarray(orc.v210_write(orc.v210_read(first, SW, SH, *b.rd_o), SW, SH, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(stale).view(np.uint32), frame0.view(np.uint32))
    comp = orc.transform(orc.v210_read(frame0.view(np.uint32), SW, SH, *b.rd_o), m(w, h), w, h)
    same_image(b.read(image_out).view(np.float32), comp, "imageOut against the oracle")
    wlut = orc.linear2gamma_lut("709")
    want = [oracle_frame("nv12", comp, w, h, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["nv12"]), wlut), oracle_frame("rgba8", comp, w, h, 0, None, wlut)]
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    last = np.asarray(orc.v210_write(comp, w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(last_out).view(np.uint32), last.view(np.uint32)), "the job behind did not read this job's image"
    small.destroy(), one.destroy(), route_prog.destroy()


def test_by_name_checks_answer_as_the_typed_call_does(by_name):
    """ph_check_program and ph_run_program give the same code and text, and the text names the argument or the typed call's cause; a
    refused job writes nothing"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    params, outs, image_out = route_params(b, Src.random("yuv420p", SW, SH, 6520).data)
    small = b.upload(np.zeros(64, np.uint8))
    big = [b.upload(np.full(w * h * 16, POISON, np.uint8)) for _ in range(2)]  # large enough for a clip's plane, an output's plane or the image
    shrunk = b.upload(np.asarray(m(w, h, scale_x=0.2, scale_y=0.2), np.float32))
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_route_1", [w, h])

    def without(d, *names):
        return {k: v for k, v in d.items() if k not in names}
    defects = [(dict(params, imageOut=small), "'imageOut'"), (without(params, "output", "imageOut"), "'output' (buffer) missing"), (dict(params, out1Packing=capi.FORMATS["p010"]), "out1Packing"),
               (without(params, "outputC"), "outputC"), (dict(params, l0InU=small), "l0InU"), (dict(params, l0In=big[0], imageOut=big[0]), "image_out overlaps a layer's source"),
               (dict(params, output1=big[1], imageOut=big[1]), "image_out overlaps an output's plane"), (dict(params, l0Matrix=shrunk), "layer 0 is neither enlarged"),
               (dict(params, l0Transition=1, l0Mix=0.5, l0IncomingIn=params["l0In"], l0IncomingInU=params["l0InU"], l0IncomingInV=params["l0InV"], l0IncomingPacking=params["l0Packing"],
                     l0IncomingWidth=SW, l0IncomingHeight=SH, l0IncomingMatrix=params["l0Matrix"]), "layer 0 is in a transition")]
    for bad, needle in defects:
        seen = []
        for check_only in (True, False):
            with pytest.raises(capi.PhaneronError) as e:
                b.ctx.run_program(prog, bad, check_only=check_only)
            seen.append(str(e.value))
        assert seen[0] == seen[1] and needle in seen[0], (needle, seen)
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    assert (b.read(image_out) == POISON).all() and all((b.read(x) == POISON).all() for x in big), "a refused job wrote the image"
    prog.destroy()


# ---- several ticks, full size -------------------------------------------------------------------------------------------------------------
def test_two_channels_for_three_ticks():
    """A plays a clip and routes its image; B plays its own clip over A's image of the tick before - a PH_SRC_RGBA_F32 layer under the
    default fill - and routes on.  Tick -1's image is opaque black.  Every image and frame is the oracle's."""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    rd_o, _, rd_d, _ = colour("709", "709")
    black = np.zeros((H, W, 4), np.float32)
    black[..., 3] = 1.0
    image_a = [hh.dev(black), hh.dev(black)]
    image_b = hh.dev(poison_image(W, H))
    want_prev = black
    wr_a, wr_b = writer("v210", "709"), writer("nv12", "709")
    for tick in range(3):
        cur, prev = tick & 1, (tick & 1) ^ 1
        a = [clip("yuv420p", 128, 36, W, H, 6600 + tick)]
        own = clip("bgra8", 100, 30, W, H, 6610 + tick, scale_x=0.6, scale_y=0.7, offset_x=0.1)
        frame_a = [hh.dev(p) for p in poisoned("v210", W, H)]
        frame_b = [hh.dev(p) for p in poisoned("nv12", W, H)]
        with capi.trace() as t:
            k.clip_compose_route_multi(device_layers(a), image_a[cur], [dict(fmt="v210", planes=frame_a, interlace=0, wr_cm=wr_a[2], wr_lut=wr_a[3])], W, H, *rd_d)
        assert t.route == "clip_up_route<rgb>x1", t.route
        with capi.trace() as t:
            k.clip_compose_route_multi([dict(src=(image_a[prev], W, H, m(W, H), "rgba"), transition="cut", mix=0.0)] + device_layers([own]), image_b,
                                       [dict(fmt="nv12", planes=frame_b, interlace=0, wr_cm=wr_b[2], wr_lut=wr_b[3])], W, H, *rd_d)
        assert two_stage(t.route, 1, reads=1), t.route
        comp_a = composite(a, W, H, rd_o)
        comp_b = np.asarray(orc.combine([orc.transform(want_prev, m(W, H), W, H), own["src"].oracle(rd_o, W, H)]))
        same_image(hh.host(image_a[cur], np.float32), comp_a, "tick %d: A's image" % tick)
        same_image(hh.host(image_b, np.float32), comp_b, "tick %d: B's image" % tick)
        for got, want in ((frame_a, oracle_frame("v210", comp_a, W, H, 0, wr_a[0], wr_a[1])), (frame_b, oracle_frame("nv12", comp_b, W, H, 0, wr_b[0], wr_b[1]))):
            for pl, (g, x) in enumerate(zip(got, want)):
                assert np.array_equal(hh.host(g, np.uint8), x), "tick %d: plane %d" % (tick, pl)
        want_prev = comp_a


def test_as_benched_1080p_against_the_gpu_chain():
    """a 1080p yuv420p file on a 1080p channel, image + v210: the image against ph_pack_read -> ph_transform on the GPU, the frame against
    ph_clip_compose_multi's (not the oracle: seconds)"""
    w, h = 1920, 1080
    route, _, _ = check_route([clip("yuv420p", w, h, w, h, 6700)], w, h, [out("v210"), out("rgba8")], "1080p", oracle=False, chain=True)
    assert route == "clip_up_route<rgb>x2", route
