"""GPU tests (-m gpu) of ph_fused_v210_transition_multi: the plain-layer composite for up to four consumers with layers in a dissolve or
a wipe.  Every output of every case is compared byte for byte, on planes poisoned with 0x5A, with
  (a) the oracle's chain: orc.v210_read of every frame -> orc.transition_dissolve / orc.transition_wipe -> orc.combine -> that format's
      oracle writer;
  (b) one ph_chan_compose_multi call on the equivalent ph_chan_layers.
The harness is test_fused_multi_gpu's: its reader (the table whose entry 0 is +Inf, so every layer and both sides of a transition
show), its layer frames and the out / writer / poisoned / oracle_frame helpers."""
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

TRANS = r"fused_v210_trans_multi x%d"
PLAIN = r"fused_v210_combine_multi x%d"
CHAN = r"chan_compose_multi<\d>x%d"
INCOMING, MASK = 1000, 2000  # seed offsets of a layer's incoming frame and of its v210 mask


# ---- layers -------------------------------------------------------------------------------------------------------------------------
def cut():
    return dict(kind="cut")


def dissolve(mix):
    return dict(kind="dissolve", mix=mix)


def wipe(mask="ramp"):
    """mask: "ramp" / "specials" (f32 images), "v210" (a frame of every 10-bit code), or an f32 array of the caller's"""
    return dict(kind="wipe", mask=mask)


def specials_mask(w, h):
    """an f32 mask whose red holds 0, 1, 1/3, -0.25, 1.25, -0, +Inf and NaN in known pixels (pixel x: value x % 8), the other channels
    values that must not matter"""
    vals = np.array([0.0, 1.0, 1.0 / 3.0, -0.25, 1.25, -0.0, np.inf, np.nan], np.float32)
    m = np.full((h, w, 4), 0.625, np.float32)
    m[..., 0] = vals[(np.arange(w)[None, :] + 3 * np.arange(h)[:, None]) % 8]
    return m


_images = {}


def image_of(w, h, seed, i, rd_o):
    """the oracle's read of frame i of a seed; computed once and left unchanged"""
    key = (w, h, seed, i, id(rd_o[1]))
    if key not in _images:
        _images[key] = orc.v210_read(layer_words(w, h, i + 1, seed)[i], w, h, *rd_o)
    return _images[key]


def mask_of(spec, w, h, i, seed):
    """(format, host array) of layer i's mask"""
    m = spec["mask"]
    if isinstance(m, np.ndarray):
        return "rgba", m
    if m == "v210":
        return "v210", layer_words(w, h, i + 1, seed + MASK)[i]
    return "rgba", frames.mask_ramp(w, h) if m == "ramp" else specials_mask(w, h)


def oracle_composite(w, h, specs, rd_o, seed):
    imgs = []
    for i, s in enumerate(specs):
        t = image_of(w, h, seed, i, rd_o)
        if s["kind"] == "dissolve":
            t = orc.transition_dissolve(t, image_of(w, h, seed + INCOMING, i, rd_o), s["mix"])
        elif s["kind"] == "wipe":
            fmt, m = mask_of(s, w, h, i, seed)
            t = orc.transition_wipe(t, image_of(w, h, seed + INCOMING, i, rd_o), image_of(w, h, seed + MASK, i, rd_o) if fmt == "v210" else m)
        imgs.append(t)
    return imgs[0] if len(imgs) == 1 else orc.combine(imgs)


def device_layers(w, h, specs, seed, src):
    """(the call's layers, the equivalent ph_chan_layers)"""
    mine, chan = [], []
    for i, s in enumerate(specs):
        own = src(layer_words(w, h, i + 1, seed)[i], "v210")
        if s["kind"] == "cut":
            mine.append(own)
            chan.append(dict(src=(own, w, h, None), transition="cut", mix=0.0))
            continue
        inc = src(layer_words(w, h, i + 1, seed + INCOMING)[i], "v210")
        L = dict(v210=own, transition=s["kind"], mix=s.get("mix", 0.0), incoming=inc)
        C = dict(src=(own, w, h, None), transition=s["kind"], mix=s.get("mix", 0.0), incoming=(inc, w, h, None))
        if s["kind"] == "wipe":
            fmt, m = mask_of(s, w, h, i, seed)
            dm = src(m, fmt)
            L.update(mask=dm, mask_format=fmt)
            C.update(mask=(dm, w, h, None) if fmt == "v210" else (dm, w, h, None, "rgba"))
        mine.append(L)
        chan.append(C)
    return mine, chan


def check(w, h, specs, outs, what, route=None, seed=7, dst=None, src=None, chan=True):
    """one ph_fused_v210_transition_multi call against the oracle and against one ph_chan_compose_multi call; returns (route, bytes)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, rd_d = reader()
    k = hh.ctx()
    comp = oracle_composite(w, h, specs, rd_o, seed)
    mine, chan_layers = device_layers(w, h, specs, seed, src or (lambda a, fmt: hh.dev(a)))
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
    make = dst or (lambda p, fmt: hh.dev(p))

    def outputs():
        planes = [[make(p, o["fmt"]) for p in poisoned(o["fmt"], w, h)] for o in outs]
        return planes, [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, planes, recipes)]
    planes, outputs_mine = outputs()
    with capi.trace() as t:
        k.fused_v210_transition_multi(mine, outputs_mine, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8).reshape(-1) for p in d] for d in planes]
    print("%s: route %s" % (what, t.route))
    for i, o in enumerate(outs):
        for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
            bad = np.flatnonzero(g != wnt)
            assert bad.size == 0, "%s: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d (got %#x, want %#x)" % (
                what, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0], g[bad[0]], wnt[bad[0]])
    if route is not None:
        assert re.fullmatch(route, t.route), "%s: route %r" % (what, t.route)
    if chan:
        theirs, outputs_theirs = outputs()
        k.chan_compose_multi(chan_layers, outputs_theirs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            for pl, p in enumerate(theirs[i]):
                assert np.array_equal(got[i][pl], hh.host(p, np.uint8).reshape(-1)), "%s: output %d (%s) plane %d differs from ph_chan_compose_multi's" % (what, i, o["fmt"], pl)
    return t.route, got


# ---- 1. formats ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_OUT)
def test_every_format_alone_and_beside_v210(fmt):
    w, h = 384, 6
    check(w, h, [cut(), dissolve(0.375)], [out(fmt)], "%s alone, layer 1 dissolving" % fmt, route=TRANS % 1)
    check(w, h, [cut(), wipe()], [out("v210"), out(fmt, 0 if fmt != "v210" else 3)], "v210 + %s, layer 1 wiping" % fmt, route=TRANS % 2)


def test_four_outputs_in_one_launch():
    check(384, 6, [cut(), dissolve(0.25), wipe("v210"), cut()], [out("nv12"), out("v210"), out("bgra8"), out("yuv422p10")], "four outputs", route=TRANS % 4)


# ---- 2. layer positions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 8])
def test_the_transition_on_the_bottom_a_middle_and_the_top_layer(n):
    outs = [out("v210"), out("rgba8")]
    for at in sorted({0, n // 2, n - 1}):
        for layer, name in ((dissolve(0.625), "dissolve"), (wipe("ramp"), "wipe")):
            specs = [cut()] * n
            specs[at] = layer
            check(384, 6, specs, outs, "%d layers, layer %d in a %s" % (n, at, name), route=TRANS % 2)


def test_one_layer_is_the_passthrough_of_the_mixed_image():
    check(384, 6, [dissolve(1.0 / 3.0)], [out("v210")], "one layer dissolving", route=TRANS % 1)
    check(384, 6, [wipe("ramp")], [out("v210"), out("yuv422p8")], "one layer wiping", route=TRANS % 2)


def test_two_layers_in_transitions_at_once():
    check(384, 6, [cut(), dissolve(0.75), cut(), wipe("ramp")], [out("v210"), out("bgra8")], "a dissolve and a wipe", route=TRANS % 2)
    check(384, 6, [wipe("v210"), dissolve(0.1)], [out("yuv422p10")], "a wipe under a dissolve", route=TRANS % 1)


def test_all_eight_layers_dissolving():
    check(384, 6, [dissolve((i + 1) / 9.0) for i in range(8)], [out("v210"), out("nv12")], "eight dissolves", route=TRANS % 2)


# ---- 3. mix values ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [0.0, 1.0, 0.5, 1.0 / 3.0, 24.0 / 25.0, -0.25, 1.25])
def test_mix_values(mix):
    """alpha is fma(1, mix, 1 - mix): not 1 at 1/3, and outside [0, 1] it leaves the unit range with the colours"""
    check(384, 6, [cut(), dissolve(mix), cut()], [out("v210"), out("rgba8")], "mix %r in the middle" % mix, route=TRANS % 2)
    check(384, 6, [dissolve(mix), cut()], [out("v210")], "mix %r at the bottom" % mix, route=TRANS % 1)


# ---- 4. masks -----------------------------------------------------------------------------------------------------------------------
def test_an_f32_ramp_mask():
    check(384, 6, [cut(), wipe("ramp"), cut()], [out("v210"), out("yuv422p8")], "ramp mask", route=TRANS % 2)


def test_an_f32_mask_of_special_values():
    """0, 1, 1/3, -0.25, 1.25, -0, +Inf and NaN in known pixels.  On the bottom layer this pins acc = v: the oracle's bottom layer does
    not see k = 1 - v.a, which is NaN where the mask is Inf or NaN"""
    _, got = check(384, 6, [wipe("specials"), cut()], [out("v210"), out("rgba8")], "special values, bottom layer", route=TRANS % 2)
    check(384, 6, [wipe("specials")], [out("rgba8")], "special values, the only layer", route=TRANS % 1)
    check(384, 6, [cut(), wipe("specials"), cut()], [out("v210"), out("rgba8")], "special values, a middle layer", route=TRANS % 2)
    check(384, 6, [cut(), cut(), wipe("specials")], [out("v210"), out("rgba8")], "special values, the top layer", route=TRANS % 2)


def test_a_v210_mask_of_every_code():
    check(384, 6, [cut(), wipe("v210")], [out("v210"), out("bgra8")], "v210 mask on top", route=TRANS % 2)
    check(384, 6, [wipe("v210"), cut(), cut()], [out("yuv422p10")], "v210 mask at the bottom", route=TRANS % 1)


# ---- 5. slice, tile and partial-wave shapes -----------------------------------------------------------------------------------------
SHAPE_LAYERS = [dissolve(0.3), wipe("ramp"), cut(), wipe("v210")]


def test_less_than_one_wave():
    """48 x 2: 16 quads, so 48 lanes of the one wave are tail lanes that recompute the last quad, for every pointer they follow"""
    check(48, 2, SHAPE_LAYERS, [out("v210"), out("yuv420p"), out("rgba8", 3)], "48x2", route=TRANS % 3)


@pytest.mark.parametrize("w,h,wgs,why", [(1920, 8, 1, "2560 quads: several slices a lane, the last partly filled per wave"),
                                         (1920, 20, 1, "6400 quads: a second, partial tile - the reader table is loaded again"),
                                         (384, 6, 3, "ranges of 128 quads that begin in mid-line")])
def test_capped_workgroups(w, h, wgs, why):
    import hip_harness as hh
    k = hh.ctx()
    k.set_option("fused_multi_wgs", wgs)
    try:
        check(w, h, SHAPE_LAYERS, [out("v210"), out("nv12", 3), out("yuv420p"), out("bgra8")], "%dx%d, %d workgroups (%s)" % (w, h, wgs, why), route=TRANS % 4)
    finally:
        k.set_option("fused_multi_wgs", 0)


# ---- 6. fields and writer tables ----------------------------------------------------------------------------------------------------
def test_field_outputs_beside_a_frame_output():
    w, h = 384, 6
    _, got = check(w, h, [cut(), dissolve(0.4)], [out("v210", 1), out("rgba8", 0), out("bgra8", 3), out("v210", 3)], "fields beside a frame", route=TRANS % 4)
    rows = got[0][0].reshape(h, -1)
    assert (rows[1::2] == POISON).all() and not (rows[0::2] == POISON).all(), "a v210 field 1 output takes the even lines only"
    rows = got[2][0].reshape(h, -1)
    assert (rows[0::2] == POISON).all() and not (rows[1::2] == POISON).all(), "a bgra8 field 3 output takes the odd lines only"


def test_a_420_output_as_a_field():
    w, h = 384, 8
    _, got = check(w, h, [wipe("ramp"), cut()], [out("yuv420p", 3), out("nv12", 0), out("v210", 1)], "4:2:0 field 3 + 4:2:0 frame", route=TRANS % 3)
    luma = got[0][0].reshape(h, w)
    assert (luma[0::2] == POISON).all() and not (luma[1::2] == POISON).all()


def test_two_writer_tables_in_one_launch():
    tab = luts.layout_table(32, 8, 0xF00D)
    with luts.register(tab) as dtab:
        outs = [out("v210"), out("yuv422p8", spec=(tab, dtab)), out("rgba8", own_table=True), out("nv12")]
        _, got = check(384, 6, [cut(), dissolve(0.5), wipe("ramp")], outs, "three tables, outputs interleaved", route=TRANS % 4)
        _, same = check(384, 6, [cut(), dissolve(0.5), wipe("ramp")], [out("yuv422p8")], "the same output from the shared table", chan=False)
        assert not np.array_equal(got[1][0], same[0][0]), "the table of other contents does not show in its output"


# ---- 7. fallbacks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmts,route", [(("v210",), "fused_v210_combine_lds"), (("yuv422p8",), PLAIN % 1), (("v210", "rgba8", "nv12"), PLAIN % 3)])
def test_every_layer_a_cut_is_the_plain_call(fmts, route):
    import hip_harness as hh
    w, h, n = 384, 6, 3
    got_route, got = check(w, h, [cut()] * n, [out(f) for f in fmts], "cuts only -> %s" % (fmts,), route=route)
    k = hh.ctx()
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, n)]
    planes = [[hh.dev(p) for p in poisoned(f, w, h)] for f in fmts]
    k.fused_v210_combine_multi(dl, [dict(fmt=f, planes=d, interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f, d in zip(fmts, planes)], w, h, *rd_d)
    for i, d in enumerate(planes):
        for pl, p in enumerate(d):
            assert np.array_equal(got[i][pl], hh.host(p, np.uint8).reshape(-1)), "output %d plane %d differs from ph_fused_v210_combine_multi's" % (i, pl)


def test_another_width_takes_the_channel_kernels_route():
    check(1280, 6, [cut(), dissolve(0.5), wipe("ramp")], [out("v210"), out("yuv422p8"), out("nv12")], "1280x6", route=CHAN % 3)
    check(1280, 6, [wipe("v210"), cut()], [out("yuv422p8")], "1280x6, one output", route=r"chan_compose_v210<\d,\d>")


def test_an_unregistered_writer_table_gets_ph_chan_compose_multis_answer():
    """the call does not qualify for the shared launch and runs ph_chan_compose_multi, whose answer - it has no kernel for a table
    without its LDS form either, and says so - is this call's; nothing is written"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 6
    _, rd_d = reader()
    k = hh.ctx()
    mine, chan = device_layers(w, h, [cut(), dissolve(0.5)], 7, lambda a, fmt: hh.dev(a))
    plain = hh.dev(capi.linear2gamma_lut("709"))
    outputs = [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in ("v210", "rgba8")]
    outputs[1]["wr_lut"] = plain
    texts = []
    for call in (lambda: k.fused_v210_transition_multi(mine, outputs, w, h, *rd_d), lambda: k.chan_compose_multi(chan, outputs, w, h, *rd_d)):
        with pytest.raises(capi.PhaneronError, match=r"error -1: .*ph_chan_compose_multi: output 1.*writer gamma LUT has no LDS form") as e:
            call()
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"])


# ---- 8. refusals on the device ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, rd_d = reader()
    w0, h0 = 384, 8

    def attempt(match, layers=None, specs=("v210", "rgba8"), tweak=None, w=w0, h=h0, rd=None):
        mine, _ = device_layers(w0, h0 + 1, [cut(), dissolve(0.5), wipe("ramp"), wipe("v210")], 7, lambda a, fmt: hh.dev(a))  # (384 x 9: large enough for every case)
        if layers:
            layers(mine)
        outputs = []
        for fmt in specs:
            f = packfmt.get(fmt)
            cm, lut = (writer(fmt, "709")[2:]) if fmt in orc.FORMAT_RANGE else hh.ColourParams.writer("709")
            outputs.append(dict(fmt=fmt, planes=[hh.dev(np.full(nb, POISON, np.uint8)) for nb in f.plane_bytes(w, h + (h & 1))], interlace=0, wr_cm=cm, wr_lut=lut))
        if tweak:
            tweak(outputs)
        with pytest.raises(capi.PhaneronError, match=match):
            k.fused_v210_transition_multi(mine, outputs, w, h, *(rd or rd_d))
        assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"] if p is not None), "a refused call wrote (%s)" % match

    attempt(r"error -1: .*layer 1: transition 3 is not", lambda l: l[1].update(transition=3))
    attempt(r"error -1: .*layer 1: a layer in a transition needs its incoming frame", lambda l: l[1].update(incoming=None))
    attempt(r"error -1: .*layer 2: a layer in a transition needs its incoming frame", lambda l: l[2].update(incoming=None))
    attempt(r"error -1: .*layer 2: a wipe needs its mask", lambda l: l[2].update(mask=None))
    attempt(r"error -1: .*layer 3: mask format 7", lambda l: l[3].update(mask_format=capi.SRC_RGBA8))
    attempt(r"error -1: .*layer 2 is NULL", lambda l: l[2].update(v210=None))
    attempt(r"error -1: .*NULL argument", rd=(None, rd_d[1], rd_d[2]))
    attempt(r"error -1: .*NULL argument", rd=(rd_d[0], None, rd_d[2]))
    attempt(r"error -1: .*NULL argument", rd=(rd_d[0], rd_d[1], None))
    attempt(r"error -1: .*1\.\.8 layers", lambda l: l.extend([l[0]] * 5))
    attempt(r"error -1: .*1\.\.8 layers", lambda l: l.clear())
    attempt(r"error -1: .*1\.\.4 outputs", specs=())
    attempt(r"error -1: .*1\.\.4 outputs", specs=("v210", "rgba8", "bgra8", "yuv422p8", "nv12"))
    attempt(r"error -1: .*output 1.*format 99 is not a PH_FMT", tweak=lambda o: o[1].update(fmt=99))
    for fmt in packfmt.NOT_CHAN_OUT:
        attempt(r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt, specs=("v210", fmt))
        attempt(r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt, specs=(fmt,))
    attempt(r"error -1: .*output 1.*interlace must be 0, 1 or 3", tweak=lambda o: o[1].update(interlace=2))
    attempt(r"error -1: .*output 0.*NULL argument", tweak=lambda o: o[0].update(planes=[None]))
    attempt(r"error -1: .*output 1.*planar output needs its three planes", specs=("v210", "yuv422p8"), tweak=lambda o: o[1].update(planes=o[1]["planes"][:2] + [None]))
    attempt(r"error -1: .*output 1.*matrix is missing", specs=("rgba8", "v210"), tweak=lambda o: o[1].update(wr_cm=None))
    attempt(r"error -1: .*output 1.*NULL argument", tweak=lambda o: o[1].update(wr_lut=None))
    attempt(r"error -1: .*output 1.*4:2:0 frame needs an even height", specs=("rgba8", "yuv420p"), h=9)
    attempt(r"error -1: .*same plane", tweak=lambda o: o[1].update(planes=o[0]["planes"]))
    # an empty frame is PH_OK and launches nothing
    mine, _ = device_layers(w0, h0, [cut(), dissolve(0.5)], 7, lambda a, fmt: hh.dev(a))
    planes = [hh.dev(p) for p in poisoned("rgba8", w0, h0)]
    with capi.trace() as t:
        k.fused_v210_transition_multi(mine, [dict(fmt="rgba8", planes=planes, interlace=0, wr_cm=None, wr_lut=writer("rgba8", "709")[3])], w0, 0, *rd_d)
    assert t.route == "" and (hh.host(planes[0], np.uint8) == POISON).all()


# ---- 9. guard bands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 2), (384, 6)])
def test_between_guard_bands(w, h):
    """every layer, incoming frame, mask of both kinds and every plane of every output between guard bands: nothing outside a buffer is
    written, and nothing read outside one reaches an output (48 x 2: most lanes are tail lanes)"""
    guard.reset()
    try:
        def dst(p, fmt):
            return guard.dev(p, "dst", pitch=max(1, p.size // h))

        def src(a, fmt):
            return guard.dev(a, "src", pitch=frames.v210_pitch_bytes(w) if fmt == "v210" else w * 16, fill="codes" if fmt == "v210" else "float")
        specs = [dissolve(0.3), wipe("ramp"), cut(), wipe("v210")]
        check(w, h, specs, [out("v210"), out("yuv422p10"), out("yuv422p8", 3), out("rgba8")], "%dx%d between guards" % (w, h), route=TRANS % 4, dst=dst, src=src, chan=False)
        check(w, h, specs, [out("yuv420p"), out("nv12", 1), out("bgra8", 3), out("v210", 1)], "%dx%d between guards" % (w, h), route=TRANS % 4, dst=dst, src=src, chan=False)
        assert guard.check() == (2 * 9, 7 + 8)
    finally:
        guard.reset()


# ---- 10. by name: fused_v210_trans_<n> ----------------------------------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(384, 6)
    yield b
    b.close()


def typed_frames(w, h, words, mask_words, mask_f32):
    """the typed call's v210 + yuv422p8 frames of: layer 0 dissolving into words[2] at 0.375, layer 1 wiping to words[3] by the v210 mask -
    or, mask_words None, by the f32 mask - with the plain 709 recipe the by-name context uses"""
    import hip_harness as hh
    k = hh.ctx()
    rd_d = hh.ColourParams.reader("709", "709")
    d = [hh.dev(x) for x in words]
    mask = dict(mask=hh.dev(mask_words), mask_format="v210") if mask_words is not None else dict(mask=hh.dev(mask_f32), mask_format="rgba")
    layers = [dict(v210=d[0], transition="dissolve", mix=0.375, incoming=d[2]), dict(v210=d[1], transition="wipe", incoming=d[3], **mask)]
    planes = [[hh.dev(p) for p in poisoned(f, w, h)] for f in ("v210", "yuv422p8")]
    outputs = [dict(fmt=f, planes=p, interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f, p in zip(("v210", "yuv422p8"), planes)]
    k.fused_v210_transition_multi(layers, outputs, w, h, *rd_d)
    return [[hh.host(p, np.uint8).reshape(-1) for p in d] for d in planes]


def trans_params(b, words, mask_words, mask_f32):
    capi = b.capi
    o0, o1 = b.planes("v210"), b.planes("yuv422p8")
    up = [b.upload(x, svm="coarse") for x in words]
    params = dict(b.recipe, l0In=up[0], l1In=up[1], l0Transition=1, l0Mix=0.375, l0IncomingIn=up[2], l1Transition=2, l1IncomingIn=up[3],
                  output=o0[0], interlace=0, out1Packing=capi.FORMATS["yuv422p8"], output1=o1[0], output1U=o1[1], output1V=o1[2], out1ColMatrix=b.cm8,
                  out1GammaLut=b.recipe["outGammaLut"], interlace1=0)
    if mask_words is not None:
        params.update(l1MaskIn=b.upload(mask_words, svm="coarse"), l1MaskPacking=capi.FORMATS["v210"])
    else:
        params.update(l1MaskIn=b.upload(mask_f32, svm="coarse"))
    return params, (o0, o1)


@pytest.mark.parametrize("mask", ["v210", "rgba"])
def test_by_name_run_program(by_name, mask):
    b, w, h = by_name, by_name.w, by_name.h
    words = layer_words(w, h, 4)
    mask_words = layer_words(w, h, 1, 7 + MASK)[0] if mask == "v210" else None
    want = typed_frames(w, h, words, mask_words, frames.mask_ramp(w, h))
    params, outs = trans_params(b, words, mask_words, frames.mask_ramp(w, h))
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_trans_2", [w, h])
    b.ctx.run_program(prog, params, check_only=True)
    assert all((b.read(p) == POISON).all() for planes in outs for p in planes), "a check wrote"
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == TRANS % 2, t.route
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d differs from the typed call's" % (i, pl)
    # a check answers as a launch does
    small = b.upload(np.zeros(64, np.uint8))
    b.ctx.wait(b.capi.QUEUE_LOAD)
    for bad, needle in [({k: v for k, v in params.items() if k != "l0IncomingIn"}, "l0IncomingIn"), (dict(params, l1MaskIn=small), "l1MaskIn"),
                        (dict(params, l1Transition=3), "'l1Transition': 3"), (dict(params, l1MaskPacking=5), "'l1MaskPacking': 5")]:
        seen = []
        for check_only in (True, False):
            with pytest.raises(b.capi.PhaneronError) as e:
                b.ctx.run_program(prog, bad, check_only=check_only)
            seen.append(str(e.value))
        assert seen[0] == seen[1] and needle in seen[0], seen
    prog.destroy()


def test_by_name_inside_run_programs_between_two_other_jobs(by_name):
    """a headline job that WRITES the job's layer 0 in front of it and a channel job that READS its output 0 behind it: each a launch of
    its own, in its turn"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    words = layer_words(w, h, 4)
    first = layer_words(w, h, 5)[4]
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    frame0 = np.asarray(orc.v210_write(orc.v210_read(first, w, h, *b.rd_o), w, h, 0, *wr_o)).reshape(-1).view(np.uint32)
    want = typed_frames(w, h, [frame0] + list(words[1:]), None, frames.mask_ramp(w, h))
    params, outs = trans_params(b, words, None, frames.mask_ramp(w, h))
    stale = b.upload(np.full(frames.v210_pitch_bytes(w) * h, POISON, np.uint8), svm="coarse")  # what the first job overwrites
    params["l0In"] = stale
    last_out = b.planes("v210")[0]
    head = b.ctx.create_program("phaneron:fused", "fused_v210_combine_1", [w, h])
    trans = b.ctx.create_program("phaneron:fused", "fused_v210_trans_2", [w, h])
    chan = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    jobs = [(head, dict(b.recipe, l0In=b.upload(first, svm="coarse"), output=stale)), (trans, params), (chan, dict(b.recipe, l0In=outs[0][0], output=last_out))]
    b.ctx.wait(capi.QUEUE_LOAD)
    with capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels[:2] == ["fused_v210_combine_lds", TRANS % 2] and len(t.kernels) == 3, t.route
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d differs from the typed call's" % (i, pl)
    last = np.asarray(orc.v210_write(orc.v210_read(want[0][0].view(np.uint32), w, h, *b.rd_o), w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(last_out).view(np.uint32), last.view(np.uint32)), "the job behind did not read this job's frame"
    head.destroy(), trans.destroy(), chan.destroy()
