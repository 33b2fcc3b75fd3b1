"""GPU tests (-m gpu) of ph_fused_v210_route_multi: the plain-layer composite for up to four consumers with f32 RGBA images among the
layers and the combined image as an output.  Every packed output of every case is compared byte for byte, on planes poisoned with 0x5A,
with
  (a) the oracle's chain: orc.v210_read of every v210 layer -> orc.combine -> that format's oracle writer;
  (b) one ph_chan_compose_multi call on the equivalent layers.
image_out starts as a poison pattern and is compared as uint32 with orc.combine's image (one layer: with that layer's image) and with
ph_combine's image made on the GPU from ph_v210_read's images: the same NaN positions, and every other value bit-equal, -0 included.
Only a NaN's payload is left unpinned: x86 fmaf and v_fma_f32 keep different operands' payloads.
The harness is test_fused_multi_gpu's and test_chan_multi_gpu's; its reader's table has +Inf as entry 0, so every layer shows."""
import re

import numpy as np
import pytest

import frames
import guard
import luts
import packfmt
from oracle import orc
from test_chan_multi_gpu import ALL_OUT, POISON, ByName, oracle_frame, out, poisoned, writer
from test_fused_multi_gpu import layer_words, reader

pytestmark = pytest.mark.gpu

ROUTE = r"fused_v210_route_multi x%di%d"
PLAIN = r"fused_v210_combine_multi x%d"
CHAN = r"chan_compose_multi<\d>x%d"
V = "v210"  # a layer spec: the v210 frame of the layer's index; anything else is an f32 RGBA image (h, w, 4)


# ---- layers -------------------------------------------------------------------------------------------------------------------------
_made = {}


def seeded_image(w, h, seed=0):
    """colours in [-0.25, 1.25], alpha in [0, 1]; made once per shape and seed"""
    key = ("img", w, h, seed)
    if key not in _made:
        rng = np.random.default_rng(0xA11CE + seed)
        m = rng.uniform(-0.25, 1.25, (h, w, 4)).astype(np.float32)
        m[..., 3] = rng.uniform(0.0, 1.0, (h, w)).astype(np.float32)
        _made[key] = m
    return _made[key]


def specials_image(w, h):
    """pixel x takes value x % 8 of {0, 1, 1/3, -0.25, 1.25, -0, +Inf, NaN} in alpha and, shifted by 3, in red (lines shifted as
    specials_mask shifts them); green and blue seeded"""
    key = ("specials", w, h)
    if key not in _made:
        vals = np.array([0.0, 1.0, 1.0 / 3.0, -0.25, 1.25, -0.0, np.inf, np.nan], np.float32)
        at = np.arange(w)[None, :] + 3 * np.arange(h)[:, None]
        m = seeded_image(w, h, 99).copy()
        m[..., 3] = vals[at % 8]
        m[..., 0] = vals[(at + 3) % 8]
        _made[key] = m
    return _made[key]


def finite_image(w, h):
    """opaque-to-transparent, every colour in the unit range: nothing that could make a NaN"""
    key = ("finite", w, h)
    if key not in _made:
        _made[key] = np.clip(seeded_image(w, h, 5), 0.0, 1.0)
    return _made[key]


def read_image(w, h, i, rd_o, seed=7):
    """the oracle's read of v210 frame i; computed once and left unchanged"""
    key = ("read", w, h, seed, i, id(rd_o[1]))
    if key not in _made:
        _made[key] = orc.v210_read(layer_words(w, h, i + 1, seed)[i], w, h, *rd_o)
    return _made[key]


def oracle_images(w, h, specs, rd_o, seed=7):
    return [read_image(w, h, i, rd_o, seed) if isinstance(s, str) else s for i, s in enumerate(specs)]


def oracle_combine(imgs):
    return np.asarray(imgs[0]) if len(imgs) == 1 else np.asarray(orc.combine(imgs))


def poison_image(w, h):
    return np.full(w * h * 16, POISON, np.uint8).view(np.float32).reshape(h, w, 4)


def same_image(got, want, what):
    """the image rule: NaN exactly where the reference has NaN, everything else equal to the bit"""
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    assert got.size == want.size, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.flatnonzero(gn != wn)
    assert bad.size == 0, "%s: %d values are NaN on one side only, first at %d (got %r, want %r)" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])
    g, x = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.flatnonzero(g != x)
    assert bad.size == 0, "%s: %d of %d values differ in their bits, first (of the non-NaN ones) at %d (got %#x, want %#x)" % (what, bad.size, got.size, bad[0], g[bad[0]], x[bad[0]])


def plain_reader():
    """(oracle reader, device reader) of the plain 709 table"""
    import hip_harness as hh
    return (orc.ycbcr2rgb_matrix("709"), orc.gamma2linear_lut("709"), orc.rgb2rgb_matrix("709", "709")), hh.ColourParams.reader("709", "709")


def device_layers(w, h, specs, seed, src):
    """(the call's layers, the equivalent ph_chan_layers, the device buffers)"""
    mine, chan, bufs = [], [], []
    for i, s in enumerate(specs):
        if isinstance(s, str):
            d = src(layer_words(w, h, i + 1, seed)[i], "v210")
            mine.append(d)
            chan.append(dict(src=(d, w, h, None), transition="cut", mix=0.0))
        else:
            d = src(s, "rgba")
            mine.append(dict(data=d, format="rgba"))
            chan.append(dict(src=(d, w, h, None, "rgba"), transition="cut", mix=0.0))
        bufs.append(d)
    return mine, chan, bufs


def gpu_chain_image(w, h, specs, bufs, rd_d):
    """ph_v210_read of every v210 layer and ph_combine of the images, on the GPU; one layer: its image"""
    import hip_harness as hh
    k = hh.ctx()
    imgs = []
    for s, d in zip(specs, bufs):
        if isinstance(s, str):
            t = hh.dev(poison_image(w, h))
            k.v210_read(d, t, w, h, *rd_d)
            imgs.append(t)
        else:
            imgs.append(d)
    if len(imgs) == 1:
        return hh.host(imgs[0], np.float32)
    t = hh.dev(poison_image(w, h))
    k.combine(imgs, t, w, h)
    return hh.host(t, np.float32)


def check(w, h, specs, outs, what, image=True, route=None, rd=None, seed=7, dst=None, src=None, chan=True, gpu_chain=True):
    """one ph_fused_v210_route_multi call against the oracle, one ph_chan_compose_multi call and the GPU's own chain; returns (route,
    the outputs' bytes, image_out or None)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, rd_d = rd or reader()
    k = hh.ctx()
    comp = oracle_combine(oracle_images(w, h, specs, rd_o, seed))
    mine, chan_layers, bufs = device_layers(w, h, specs, seed, src or (lambda a, fmt: hh.dev(a)))
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
    make = dst or (lambda p, fmt: hh.dev(p))

    def outputs():
        planes = [[make(p, o["fmt"]) for p in poisoned(o["fmt"], w, h)] for o in outs]
        return planes, [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, planes, recipes)]
    planes, outputs_mine = outputs()
    image_out = make(poison_image(w, h), "image") if image else None
    with capi.trace() as t:
        k.fused_v210_route_multi(mine, image_out, outputs_mine, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8).reshape(-1) for p in d] for d in planes]
    print("%s: route %s" % (what, t.route))
    if route is not None:
        assert re.fullmatch(route, t.route), "%s: route %r" % (what, t.route)
    for i, o in enumerate(outs):
        for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
            bad = np.flatnonzero(g != wnt)
            assert bad.size == 0, "%s: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d (got %#x, want %#x)" % (
                what, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0], g[bad[0]], wnt[bad[0]])
    got_image = None
    if image:
        got_image = hh.host(image_out, np.float32).reshape(h, w, 4)
        same_image(got_image, comp, "%s: image_out against the oracle's combine" % what)
        if gpu_chain:
            same_image(got_image, gpu_chain_image(w, h, specs, bufs, rd_d), "%s: image_out against ph_v210_read + ph_combine" % what)
    if chan and outs:
        theirs, outputs_theirs = outputs()
        k.chan_compose_multi(chan_layers, outputs_theirs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            for pl, p in enumerate(theirs[i]):
                assert np.array_equal(got[i][pl], hh.host(p, np.uint8).reshape(-1)), "%s: output %d (%s) plane %d differs from ph_chan_compose_multi's" % (what, i, o["fmt"], pl)
    return t.route, got, got_image


def with_image(n, at, img):
    specs = [V] * n
    specs[at] = img
    return specs


# ---- 1. positions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_the_image_layer_at_the_bottom_in_the_middle_and_on_top(n):
    w, h = 384, 6
    outs = [out("v210"), out("rgba8")]
    for at in sorted({0, n // 2, n - 1}):
        specs = with_image(n, at, seeded_image(w, h, at))
        check(w, h, specs, outs, "%d layers, the image is layer %d, image out" % (n, at), route=ROUTE % (2, 1))
        check(w, h, specs, outs, "%d layers, the image is layer %d, no image out" % (n, at), image=False, route=ROUTE % (2, 0))


# ---- 2. one layer -------------------------------------------------------------------------------------------------------------------
def test_an_image_alone_is_a_copy():
    w, h = 384, 6
    img = specials_image(w, h)
    _, _, got = check(w, h, [img], [out("v210"), out("rgba8")], "the specials image alone", route=ROUTE % (2, 1))
    nan = np.isnan(img)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], img.view(np.uint32)[~nan]), "-0, Inf and alpha must come through untouched"
    assert np.signbit(got[~nan]).sum() == np.signbit(img[~nan]).sum() > 0


def test_a_v210_layer_alone_gives_the_readers_image():
    import hip_harness as hh
    w, h = 384, 6
    _, _, got = check(w, h, [V], [out("v210"), out("yuv422p8")], "one v210 layer, image out", route=ROUTE % (2, 1))
    _, rd_d = reader()
    t = hh.dev(poison_image(w, h))
    hh.ctx().v210_read(hh.dev(layer_words(w, h, 1)[0]), t, w, h, *rd_d)
    same_image(got, hh.host(t, np.float32), "image_out against ph_v210_read's image")
    assert (got[..., 3] == 1.0).all()


# ---- 3. the bottom layer as it is ---------------------------------------------------------------------------------------------------
def test_a_specials_image_at_the_bottom_under_a_v210_layer():
    w, h = 384, 6
    img = specials_image(w, h)
    _, _, got = check(w, h, [img, V], [out("v210"), out("rgba8")], "specials at the bottom", route=ROUTE % (2, 1))
    bad = ~np.isfinite(img[..., 3])
    assert np.array_equal(np.isnan(got[..., 3]), bad), "alpha is NaN exactly where the image's alpha is Inf or NaN"
    assert (got[..., 3][~bad] == 1.0).all()


# ---- 4. specials further up, two images ---------------------------------------------------------------------------------------------
def test_specials_in_the_middle_and_on_top():
    w, h = 384, 6
    outs = [out("v210"), out("rgba8")]
    check(w, h, [V, specials_image(w, h), V], outs, "specials in the middle", route=ROUTE % (2, 1))
    check(w, h, [V, V, specials_image(w, h)], outs, "specials on top", route=ROUTE % (2, 1))


def test_two_image_layers_in_one_call():
    w, h = 384, 6
    check(w, h, [specials_image(w, h), V, seeded_image(w, h, 3), V], [out("v210"), out("bgra8")], "specials under a seeded image", route=ROUTE % (2, 1))
    check(w, h, [seeded_image(w, h, 3), specials_image(w, h)], [out("yuv422p10")], "two images and nothing else", route=ROUTE % (1, 1))
    check(w, h, [V, seeded_image(w, h, 1), specials_image(w, h)], [out("nv12")], "two images on top, no image out", image=False, route=ROUTE % (1, 0))


# ---- 5. outputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_OUT)
def test_every_format_alone_and_beside_v210(fmt):
    w, h = 384, 6
    specs = [V, V, seeded_image(w, h)]
    check(w, h, specs, [out(fmt)], "%s alone with the image" % fmt, route=ROUTE % (1, 1))
    check(w, h, specs, [out("v210"), out(fmt, 0 if fmt != "v210" else 3)], "v210 + %s with the image" % fmt, route=ROUTE % (2, 1))


def test_four_outputs_with_three_writer_tables():
    w, h = 384, 6
    tab = luts.layout_table(32, 8, 0xF00D)
    specs = [V, seeded_image(w, h), V]
    with luts.register(tab) as dtab:
        outs = [out("v210"), out("yuv422p8", spec=(tab, dtab)), out("rgba8", own_table=True), out("nv12")]
        _, got, _ = check(w, h, specs, outs, "three tables, outputs interleaved", route=ROUTE % (4, 1))
        _, same, _ = check(w, h, specs, [out("yuv422p8")], "the same output from the shared table", image=False, chan=False)
        assert not np.array_equal(got[1][0], same[0][0]), "the table of other contents does not show in its output"


def test_field_outputs_beside_a_frame_output():
    w, h = 384, 6
    _, got, _ = check(w, h, [V, seeded_image(w, h)], [out("v210", 1), out("rgba8", 0), out("bgra8", 3), out("v210", 3)], "fields beside a frame", route=ROUTE % (4, 1))
    rows = got[0][0].reshape(h, -1)
    assert (rows[1::2] == POISON).all() and not (rows[0::2] == POISON).all(), "a v210 field 1 output takes the even lines only"
    rows = got[2][0].reshape(h, -1)
    assert (rows[0::2] == POISON).all() and not (rows[1::2] == POISON).all(), "a bgra8 field 3 output takes the odd lines only"


def test_a_420_output_as_a_field():
    w, h = 384, 8
    _, got, _ = check(w, h, [seeded_image(w, h), V], [out("yuv420p", 3), out("nv12", 0), out("v210", 1)], "4:2:0 field 3 + 4:2:0 frame", route=ROUTE % (3, 1))
    luma = got[0][0].reshape(h, w)
    assert (luma[0::2] == POISON).all() and not (luma[1::2] == POISON).all()


def test_the_image_alone_touches_no_writer_table():
    w, h = 384, 6
    check(w, h, [V, V, V, seeded_image(w, h)], [], "no outputs: the image only", route=ROUTE % (0, 1))
    check(w, h, [V, V], [], "no outputs, no image layer", route=ROUTE % (0, 1))
    check(w, h, [specials_image(w, h)], [], "no outputs, an image alone", route=ROUTE % (0, 1))


# ---- 6. slices and tiles ------------------------------------------------------------------------------------------------------------
FOUR = [out("v210"), out("nv12", 3), out("yuv420p"), out("bgra8")]


def test_less_than_one_wave():
    """48 x 2: 16 quads, so 48 lanes of the one wave are tail lanes that recompute the last quad, for every pointer they follow"""
    w, h = 48, 2
    check(w, h, [V, specials_image(w, h), V], FOUR, "48x2", route=ROUTE % (4, 1))
    check(w, h, [V, V, V], FOUR, "48x2 without an image layer", route=ROUTE % (4, 1))


@pytest.mark.parametrize("w,h,wgs,why", [(1920, 8, 1, "2560 quads: several slices a lane, the last partly filled per wave"),
                                         (1920, 20, 1, "6400 quads: a second, partial tile - the reader table is loaded again"),
                                         (384, 6, 3, "ranges of 128 quads that begin in mid-line")])
def test_capped_workgroups(w, h, wgs, why):
    import hip_harness as hh
    k = hh.ctx()
    k.set_option("fused_multi_wgs", wgs)
    try:
        check(w, h, [V, seeded_image(w, h), V, specials_image(w, h)], FOUR, "%dx%d, %d workgroups (%s)" % (w, h, wgs, why), route=ROUTE % (4, 1))
        check(w, h, [V, V], FOUR, "%dx%d, %d workgroups, no image layer" % (w, h, wgs), route=ROUTE % (4, 1), chan=False)
    finally:
        k.set_option("fused_multi_wgs", 0)


# ---- 7. the plain reader ------------------------------------------------------------------------------------------------------------
def test_the_plain_reader_and_finite_images_make_no_nan_at_all():
    w, h = 384, 6
    rd = plain_reader()
    specs = [V, finite_image(w, h), V, finite_image(w, h)[::-1].copy()]
    comp = oracle_combine(oracle_images(w, h, specs, rd[0]))
    assert not np.isnan(comp).any(), "the oracle's image of this case holds no NaN: the comparison is plain bit equality"
    _, _, got = check(w, h, specs, [out("v210"), out("rgba8")], "plain reader, finite images", rd=rd, route=ROUTE % (2, 1))
    assert np.array_equal(got.view(np.uint32), comp.view(np.uint32))


# ---- 8. routes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmts,route", [(("v210",), "fused_v210_combine_lds"), (("yuv422p8",), PLAIN % 1), (("v210", "rgba8", "nv12"), PLAIN % 3)])
def test_plain_layers_without_the_image_are_the_plain_call(fmts, route):
    import hip_harness as hh
    w, h, n = 384, 6, 3
    _, got, _ = check(w, h, [V] * n, [out(f) for f in fmts], "plain layers -> %s" % (fmts,), image=False, route=route)
    k = hh.ctx()
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, n)]
    planes = [[hh.dev(p) for p in poisoned(f, w, h)] for f in fmts]
    k.fused_v210_combine_multi(dl, [dict(fmt=f, planes=d, interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f, d in zip(fmts, planes)], w, h, *rd_d)
    for i, d in enumerate(planes):
        for pl, p in enumerate(d):
            assert np.array_equal(got[i][pl], hh.host(p, np.uint8).reshape(-1)), "output %d plane %d differs from ph_fused_v210_combine_multi's" % (i, pl)


NOT_TAKEN = (r"error -1: ph_fused_v210_route_multi: the one-launch route does not take this frame \(it needs width % 48 == 0, the reader's and every writer's table "
             r"registered, \"lds_lut\" = 1 and a frame within the kernel's division by reciprocal\) and nothing else makes image_out: run ph_v210_read, ph_combine and "
             r"ph_pack_write_multi$")


def refused_with_the_image(w, h, specs, outputs_of, match):
    """the call with image_out is refused with `match`, and every buffer keeps its poison"""
    import hip_harness as hh
    from phaneron_amd import capi
    _, rd_d = reader()
    k = hh.ctx()
    mine, _, _ = device_layers(w, h, specs, 7, lambda a, fmt: hh.dev(a))
    outputs = outputs_of()
    image_out = hh.dev(poison_image(w, h))
    with capi.trace() as t:
        with pytest.raises(capi.PhaneronError, match=match):
            k.fused_v210_route_multi(mine, image_out, outputs, w, h, *rd_d)
    assert t.route == ""
    assert (hh.host(image_out, np.uint8) == POISON).all()
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"])


def plain_outputs(w, h, fmts):
    import hip_harness as hh
    return [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in fmts]


def test_another_width_takes_the_channel_kernels_route_or_is_refused():
    w, h = 1280, 6
    specs = [V, seeded_image(w, h), V]
    check(w, h, specs, [out("v210"), out("yuv422p8"), out("nv12")], "1280x6 without image_out", image=False, route=CHAN % 3)
    refused_with_the_image(w, h, specs, lambda: plain_outputs(w, h, ("v210", "yuv422p8")), NOT_TAKEN)
    refused_with_the_image(w, h, specs, lambda: [], NOT_TAKEN)


def test_an_unregistered_writer_table_both_ways():
    """without image_out the call runs ph_chan_compose_multi, whose answer - it has no kernel for a table without its LDS form either, and
    says so - is this call's; with image_out it is refused as a frame the launch does not take.  Nothing is written either way"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 6
    _, rd_d = reader()
    k = hh.ctx()
    specs = [V, seeded_image(w, h)]
    mine, chan, _ = device_layers(w, h, specs, 7, lambda a, fmt: hh.dev(a))
    plain = hh.dev(capi.linear2gamma_lut("709"))

    def outputs():
        o = plain_outputs(w, h, ("v210", "rgba8"))
        o[1]["wr_lut"] = plain
        return o
    outs = outputs()
    texts = []
    for call in (lambda: k.fused_v210_route_multi(mine, None, outs, w, h, *rd_d), lambda: k.chan_compose_multi(chan, outs, w, h, *rd_d)):
        with pytest.raises(capi.PhaneronError, match=r"error -1: .*ph_chan_compose_multi: output 1.*writer gamma LUT has no LDS form") as e:
            call()
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outs for p in o["planes"])
    refused_with_the_image(w, h, specs, outputs, NOT_TAKEN)


# ---- 9. refusals on the device ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, rd_d = reader()
    w0, h0 = 384, 8

    def attempt(match, layers=None, specs=("v210", "rgba8"), tweak=None, w=w0, h=h0, rd=None, image="own"):
        mine, _, _ = device_layers(w0, h0 + 1, [V, seeded_image(w0, h0 + 1), V, V], 7, lambda a, fmt: hh.dev(a))  # (384 x 9: large enough for every case)
        image_out = hh.dev(poison_image(w0, h0 + 1)) if image == "own" else image
        if layers:
            alias = layers(mine, image_out)
            image_out = image_out if alias is None else alias
        outputs = []
        for fmt in specs:
            f = packfmt.get(fmt)
            cm, lut = (writer(fmt, "709")[2:]) if fmt in orc.FORMAT_RANGE else hh.ColourParams.writer("709")
            outputs.append(dict(fmt=fmt, planes=[hh.dev(np.full(nb, POISON, np.uint8)) for nb in f.plane_bytes(w, h + (h & 1))], interlace=0, wr_cm=cm, wr_lut=lut))
        if tweak:
            alias = tweak(outputs, image_out)
            image_out = image_out if alias is None else alias
        before = [hh.host(m["data"] if isinstance(m, dict) else m, np.uint8).copy() for m in mine if (m["data"] if isinstance(m, dict) else m) is not None]
        with capi.trace() as t:
            with pytest.raises(capi.PhaneronError, match=match):
                k.fused_v210_route_multi(mine, image_out, outputs, w, h, *(rd or rd_d))
        assert t.route == "", "a refused call launched (%s)" % match
        assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"] if p is not None), "a refused call wrote (%s)" % match
        after = [hh.host(m["data"] if isinstance(m, dict) else m, np.uint8) for m in mine if (m["data"] if isinstance(m, dict) else m) is not None]
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), "a refused call wrote a layer (%s)" % match
        if image_out is not None and all(image_out is not (m["data"] if isinstance(m, dict) else m) for m in mine):
            assert (hh.host(image_out, np.uint8) == POISON).all(), "a refused call wrote the image (%s)" % match

    attempt(r"error -1: .*1\.\.8 layers", lambda l, i: l.extend([l[0]] * 5))
    attempt(r"error -1: .*1\.\.8 layers", lambda l, i: l.clear())
    attempt(r"error -1: .*layer 2 is NULL", lambda l, i: l.__setitem__(2, None))
    attempt(r"error -1: .*layer 1 is NULL", lambda l, i: l[1].update(data=None))
    attempt(r"error -1: .*layer 1: format 7 \(a v210 frame, PH_SRC_V210, or an f32 RGBA image, PH_SRC_RGBA_F32\)", lambda l, i: l[1].update(format=capi.SRC_RGBA8))
    attempt(r"error -1: .*layer 1: format 0 ", lambda l, i: l[1].update(format=0))
    attempt(r"error -1: .*0\.\.4 outputs \(5\)", specs=("v210", "rgba8", "bgra8", "yuv422p8", "nv12"))
    attempt(r"error -1: .*nothing to make: no output and image_out is NULL", specs=(), image=None)
    attempt(r"error -1: .*image_out is layer 1's data", lambda l, i: l[1]["data"])
    attempt(r"error -1: .*image_out is layer 0's data", lambda l, i: l[0])
    attempt(r"error -1: .*image_out is output 1's first plane", tweak=lambda o, i: o[1]["planes"][0])
    attempt(r"error -1: .*NULL argument", rd=(None, rd_d[1], rd_d[2]))
    attempt(r"error -1: .*NULL argument", rd=(rd_d[0], None, rd_d[2]))
    attempt(r"error -1: .*NULL argument", rd=(rd_d[0], rd_d[1], None), specs=())
    attempt(r"error -1: .*output 1.*format 99 is not a PH_FMT", tweak=lambda o, i: o[1].update(fmt=99))
    for fmt in packfmt.NOT_CHAN_OUT:
        attempt(r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt, specs=("v210", fmt))
        attempt(r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt, specs=(fmt,))
    attempt(r"error -1: .*output 1.*interlace must be 0, 1 or 3", tweak=lambda o, i: o[1].update(interlace=2))
    attempt(r"error -1: .*output 0.*NULL argument", tweak=lambda o, i: o[0].update(planes=[None]))
    attempt(r"error -1: .*output 1.*planar output needs its three planes", specs=("v210", "yuv422p8"), tweak=lambda o, i: o[1].update(planes=o[1]["planes"][:2] + [None]))
    attempt(r"error -1: .*output 1.*matrix is missing", specs=("rgba8", "v210"), tweak=lambda o, i: o[1].update(wr_cm=None))
    attempt(r"error -1: .*output 1.*NULL argument", tweak=lambda o, i: o[1].update(wr_lut=None))
    attempt(r"error -1: .*output 1.*4:2:0 frame needs an even height", specs=("rgba8", "yuv420p"), h=9)
    attempt(r"error -1: .*same plane", tweak=lambda o, i: o[1].update(planes=o[0]["planes"]))
    attempt(r"error -1: .*width 0", w=0, specs=())
    # an empty frame is PH_OK and launches nothing
    mine, _, _ = device_layers(w0, h0, [V, seeded_image(w0, h0)], 7, lambda a, fmt: hh.dev(a))
    planes = [hh.dev(p) for p in poisoned("rgba8", w0, h0)]
    image_out = hh.dev(poison_image(w0, h0))
    with capi.trace() as t:
        k.fused_v210_route_multi(mine, image_out, [dict(fmt="rgba8", planes=planes, interlace=0, wr_cm=None, wr_lut=writer("rgba8", "709")[3])], w0, 0, *rd_d)
    assert t.route == "" and (hh.host(planes[0], np.uint8) == POISON).all() and (hh.host(image_out, np.uint8) == POISON).all()


# ---- 10. guard bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 2), (384, 6)])
def test_between_guard_bands(w, h):
    """every v210 layer, the image layer, image_out and every plane of every output between guard bands: nothing outside a buffer is
    written, and nothing read outside one reaches an output (48 x 2: most lanes are tail lanes)"""
    guard.reset()
    try:
        def dst(p, fmt):
            return guard.dev(p, "dst", pitch=w * 16 if fmt == "image" else max(1, p.size // h))

        def src(a, fmt):
            return guard.dev(a, "src", pitch=frames.v210_pitch_bytes(w) if fmt == "v210" else w * 16, fill="codes" if fmt == "v210" else "float")
        specs = [V, seeded_image(w, h), V, V]
        kw = dict(route=ROUTE % (4, 1), dst=dst, src=src, chan=False, gpu_chain=False)
        check(w, h, specs, [out("v210"), out("yuv422p10"), out("yuv422p8", 3), out("rgba8")], "%dx%d between guards" % (w, h), **kw)
        check(w, h, specs, [out("yuv420p"), out("nv12", 1), out("bgra8", 3), out("v210", 1)], "%dx%d between guards" % (w, h), **kw)
        # sources: 3 v210 layers + the image, twice; destinations: image_out + 8 planes, image_out + 7 planes
        assert guard.check() == (2 * 4, (1 + 8) + (1 + 7))
    finally:
        guard.reset()


# ---- 11. by name: fused_v210_route_<n> ----------------------------------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(384, 6)
    yield b
    b.close()


def typed_route(w, h, layers, fmts, image=True):
    """the typed call with the plain 709 recipe the by-name context uses: (the outputs' bytes, image_out)"""
    import hip_harness as hh
    k = hh.ctx()
    rd_d = hh.ColourParams.reader("709", "709")
    mine = [hh.dev(x) if x.dtype != np.float32 else dict(data=hh.dev(x), format="rgba") for x in layers]
    planes = [[hh.dev(p) for p in poisoned(f, w, h)] for f in fmts]
    outputs = [dict(fmt=f, planes=p, interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f, p in zip(fmts, planes)]
    image_out = hh.dev(poison_image(w, h)) if image else None
    k.fused_v210_route_multi(mine, image_out, outputs, w, h, *rd_d)
    return [[hh.host(p, np.uint8).reshape(-1) for p in d] for d in planes], hh.host(image_out, np.float32).reshape(h, w, 4) if image else None


def route_params(b, words, img):
    capi = b.capi
    o0, o1 = b.planes("v210"), b.planes("yuv422p8")
    image_out = b.upload(poison_image(b.w, b.h), svm="coarse")
    params = dict(b.recipe, l0In=b.upload(words, svm="coarse"), l1In=b.upload(img, svm="coarse"), l1Image=1, imageOut=image_out,
                  output=o0[0], interlace=0, out1Packing=capi.FORMATS["yuv422p8"], output1=o1[0], output1U=o1[1], output1V=o1[2], out1ColMatrix=b.cm8,
                  out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    return params, (o0, o1), image_out


def test_by_name_run_program(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    words, img = layer_words(w, h, 1)[0], seeded_image(w, h)
    want, want_image = typed_route(w, h, [words, img], ("v210", "yuv422p8"))
    params, outs, image_out = route_params(b, words, img)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_route_2", [w, h])
    b.ctx.run_program(prog, params, check_only=True)
    assert all((b.read(p) == POISON).all() for planes in outs for p in planes) and (b.read(image_out) == POISON).all(), "a check wrote"
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == ROUTE % (2, 1), t.route
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d differs from the typed call's" % (i, pl)
    same_image(b.read(image_out).view(np.float32), want_image, "imageOut against the typed call's image")
    # the image alone: no `output` at all
    alone = {k: v for k, v in params.items() if not k.startswith("out") or k == "outGammaLut" or k == "outColMatrix"}
    alone = {k: v for k, v in alone.items() if k not in ("interlace", "interlace1")}
    alone["imageOut"] = only = b.upload(poison_image(w, h), svm="coarse")
    b.ctx.wait(b.capi.QUEUE_LOAD)
    with b.capi.trace() as t:
        b.ctx.run_program(prog, alone)
    b.ctx.wait()
    assert t.route == ROUTE % (0, 1), t.route
    same_image(b.read(only).view(np.float32), want_image, "imageOut alone against the typed call's image")
    # a check answers as a launch does
    small = b.upload(np.zeros(frames.v210_pitch_bytes(w) * h, np.uint8))  # a v210 frame's bytes: too small for an image
    b.ctx.wait(b.capi.QUEUE_LOAD)
    neither = {k: v for k, v in params.items() if k not in ("output", "imageOut")}
    for bad, needle in [(dict(params, l1Image=2), "'l1Image': 2"), (dict(params, l1In=small), "'l1In'"), (dict(params, imageOut=small), "'imageOut'"),
                        (neither, "'output' (buffer) missing"), (dict(params, imageOut=params["l1In"]), "'imageOut': the buffer is layer 1's too")]:
        seen = []
        for check_only in (True, False):
            with pytest.raises(b.capi.PhaneronError) as e:
                b.ctx.run_program(prog, bad, check_only=check_only)
            seen.append(str(e.value))
        assert seen[0] == seen[1] and needle in seen[0], seen
    prog.destroy()


def test_by_name_inside_run_programs_between_two_other_jobs(by_name):
    """a reader job that WRITES the job's image layer in front of it and a job that READS its imageOut as a layer behind it: each a
    launch of its own, in its turn, and the frames are those of the separate typed calls"""
    import hip_harness as hh
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    words = layer_words(w, h, 2)
    # the typed calls, one after the other
    k = hh.ctx()
    rd_d = hh.ColourParams.reader("709", "709")
    routed = hh.dev(poison_image(w, h))
    k.v210_read(hh.dev(words[1]), routed, w, h, *rd_d)
    routed = hh.host(routed, np.float32).reshape(h, w, 4)
    want, want_image = typed_route(w, h, [words[0], routed], ("v210", "yuv422p8"))
    want_last, _ = typed_route(w, h, [want_image], ("v210",), image=False)
    # the same as three jobs of one call
    stale = poison_image(w, h)  # what the first job overwrites
    params, outs, image_out = route_params(b, words[0], stale)
    last_out = b.planes("v210")[0]
    wipg = frames.v210_pitch_pixels(w) // 48
    rd = b.ctx.create_program("phaneron:v210", "read", wipg * h, wipg)
    route = b.ctx.create_program("phaneron:fused", "fused_v210_route_2", [w, h])
    behind = b.ctx.create_program("phaneron:fused", "fused_v210_route_1", [w, h])
    loader = {k_: b.recipe[k_] for k_ in ("colMatrix", "gammaLut", "gamutMatrix")}
    jobs = [(rd, dict(loader, input=b.upload(words[1], svm="coarse"), output=params["l1In"], width=w)), (route, params),
            (behind, dict(b.recipe, l0In=image_out, l0Image=1, output=last_out, interlace=0))]
    b.ctx.wait(capi.QUEUE_LOAD)
    with capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert len(t.kernels) == 3 and "v210_read" in t.kernels[0] and t.kernels[1:] == [ROUTE % (2, 1), ROUTE % (1, 0)], t.route
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d differs from the typed call's" % (i, pl)
    same_image(b.read(image_out).view(np.float32), want_image, "imageOut against the typed call's image")
    assert np.array_equal(b.read(last_out), want_last[0][0]), "the job behind did not read this job's image"
    rd.destroy(), route.destroy(), behind.destroy()


# ---- 12. config 5's loop, small -----------------------------------------------------------------------------------------------------
def test_two_channels_routing_each_others_image_for_four_steps():
    """each channel's fourth layer is the other channel's image_out of the step before, double-buffered; frame -1 is opaque black.  Every
    step's v210 frame and image are those of the oracle's chain: read x 3 -> combine_4 -> write"""
    import hip_harness as hh
    w, h, steps = 384, 6, 4
    rd_o, rd_d = reader()
    k = hh.ctx()
    wcm_o, wlut_o, wcm_d, wlut_d = writer("v210", "709")
    black = np.zeros((h, w, 4), np.float32)
    black[..., 3] = 1.0
    words = [layer_words(w, h, 3, seed=70 + c) for c in range(2)]
    own = [[orc.v210_read(x, w, h, *rd_o) for x in words[c]] for c in range(2)]
    dwords = [[hh.dev(x) for x in words[c]] for c in range(2)]
    image = [[hh.dev(black), hh.dev(black)] for _ in range(2)]  # [channel][buffer]
    frame = [hh.dev(poisoned("v210", w, h)[0]) for _ in range(2)]
    want_prev = [black, black]
    from phaneron_amd import capi
    for step in range(steps):
        cur, prev = step & 1, (step & 1) ^ 1
        want_now = []
        for c in range(2):
            with capi.trace() as t:
                k.fused_v210_route_multi(dwords[c] + [dict(data=image[c ^ 1][prev], format="rgba")], image[c][cur],
                                         [dict(fmt="v210", planes=[frame[c]], interlace=0, wr_cm=wcm_d, wr_lut=wlut_d)], w, h, *rd_d)
            assert t.route == ROUTE % (1, 1), t.route
            comp = np.asarray(orc.combine(own[c] + [want_prev[c ^ 1]]))
            same_image(hh.host(image[c][cur], np.float32), comp, "step %d channel %d: image" % (step, c))
            v210 = oracle_frame("v210", comp, w, h, 0, wcm_o, wlut_o)[0]
            assert np.array_equal(hh.host(frame[c], np.uint8).reshape(-1), v210), "step %d channel %d: v210 frame" % (step, c)
            want_now.append(comp)
        want_prev = want_now
