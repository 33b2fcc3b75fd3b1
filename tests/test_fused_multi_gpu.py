"""GPU tests (-m gpu) of ph_fused_v210_combine_multi: the headline chain - N plain v210 layers of the output's size, read, combined,
written - for up to four consumers in one launch.  Every output of every case is compared byte for byte, on planes poisoned with 0x5A,
with the oracle's chain (orc.v210_read x n -> orc.combine -> that format's oracle writer), with separate ph_chan_compose calls on the
layers taken 1:1 and - a v210 frame - with ph_fused_v210_combine.

The reader's table has entry 0 = +Inf (test_chains_gpu._poison_lut): a pixel of ANY layer whose R, G or B clamps to index 0 turns the
accumulator into Inf and the next layer's fma(acc, 0, t) into NaN, which the writers map to index 0 - so every layer shows."""
import ctypes
import re

import numpy as np
import pytest

import frames
import guard
import luts
import packfmt
from oracle import orc
from test_chains_gpu import _poison_lut
from test_chan_multi_gpu import ALL_OUT, POISON, ByName, oracle_frame, out, poisoned, writer

pytestmark = pytest.mark.gpu

SHARED = r"fused_v210_combine_multi x%d"
_state = {}


def reader():
    """(oracle reader, device reader) with the poisoned table, registered once"""
    if "rd" not in _state:
        import hip_harness as hh
        from phaneron_amd import capi
        lut = _poison_lut()
        dlut = hh.dev(lut)
        assert hh.ctx().register_lut(dlut, lut) == 1, "the poisoned table must keep its LDS form"
        gm = capi.rgb2rgb_matrix("709", "709")
        _state["rd"] = ((orc.ycbcr2rgb_matrix("709"), lut, orc.rgb2rgb_matrix("709", "709")),
                        (hh.dev(capi.ycbcr2rgb_matrix("709")), dlut, hh.dev(np.concatenate([gm, np.zeros(3, np.float32)]))))
    return _state["rd"]


_layers, _comps = {}, {}


def layer_words(w, h, n, seed=7):
    """n random v210 frames, every 10-bit code (codes below black clamp to table index 0: the poison); made once per shape"""
    key = (w, h, seed)
    have = _layers.setdefault(key, [])
    while len(have) < n:
        have.append(frames.v210_random(w, h, frames.layer_seed(seed, len(have)), legal=False))
    return have[:n]


def composite(w, h, n, rd_o, seed=7):
    """the oracle's combined image of the first n layers; computed once and shared"""
    key = (w, h, n, seed, id(rd_o[1]))
    if key not in _comps:
        imgs = [orc.v210_read(l, w, h, *rd_o) for l in layer_words(w, h, n, seed)]
        _comps[key] = imgs[0] if n == 1 else orc.combine(imgs)
    return _comps[key]


def chan_layers(dev_layers, w, h):
    return [dict(src=(t, w, h, None), transition="cut", mix=0.0) for t in dev_layers]


def check(w, h, n, outs, what, rd=None, seed=7, route=None, separate=True, dst=None, src=None):
    """one ph_fused_v210_combine_multi call against the oracle, the separate ph_chan_compose calls and (v210 frames) the headline
    kernel; returns (route, the outputs' bytes).  dst / src: makers of device buffers (guard bands)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, rd_d = rd or reader()
    k = hh.ctx()
    comp = composite(w, h, n, rd_o, seed)
    dl = [(src or hh.dev)(l) for l in layer_words(w, h, n, seed)]
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
    want = [oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)]
    make = dst or (lambda p, fmt: hh.dev(p))
    planes = [[make(p, o["fmt"]) for p in poisoned(o["fmt"], w, h)] for o in outs]
    outputs = [dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, planes, recipes)]
    with capi.trace() as t:
        k.fused_v210_combine_multi(dl, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = [[hh.host(p, np.uint8).reshape(-1) for p in d] for d in planes]
    for i, o in enumerate(outs):
        for pl, (g, wnt) in enumerate(zip(got[i], want[i])):
            bad = np.flatnonzero(g != wnt)
            assert bad.size == 0, "%s: output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d (got %#x, want %#x)" % (
                what, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0], g[bad[0]], wnt[bad[0]])
    if route is not None:
        assert re.fullmatch(route, t.route), "%s: route %r" % (what, t.route)
    if separate:
        cl = chan_layers(dl, w, h)
        for i, (o, rc) in enumerate(zip(outs, recipes)):
            alone = [hh.dev(p) for p in poisoned(o["fmt"], w, h)]
            k.chan_compose_v210(cl, alone[0] if o["fmt"] == "v210" else alone, w, h, o["interlace"], *rd_d, rc[2], rc[3], out_fmt=o["fmt"])
            k.wait()
            torch.cuda.synchronize()
            for pl, a in enumerate(alone):
                assert np.array_equal(got[i][pl], hh.host(a, np.uint8).reshape(-1)), "%s: output %d (%s) plane %d differs from a separate ph_chan_compose call" % (what, i, o["fmt"], pl)
            if o["fmt"] == "v210" and o["interlace"] == 0:
                head = hh.dev(poisoned("v210", w, h)[0])
                with capi.trace() as t1:
                    k.fused_v210_combine(dl, head, w, h, *rd_d, rc[2], rc[3])
                assert t1.route == "fused_v210_combine_lds", t1.route
                assert np.array_equal(got[i][0], hh.host(head, np.uint8).reshape(-1)), "%s: output %d differs from ph_fused_v210_combine's frame" % (what, i)
    return t.route, got


# ---- formats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 8])
@pytest.mark.parametrize("fmt", ALL_OUT)
def test_every_format_alone_and_beside_v210(fmt, n):
    w, h = 384, 6
    route, _ = check(w, h, n, [out(fmt)], "%s alone, %d layers" % (fmt, n))
    assert route == ("fused_v210_combine_lds" if fmt == "v210" else SHARED % 1), route  # one v210 frame IS the headline kernel's call
    check(w, h, n, [out("v210"), out(fmt, 0 if fmt != "v210" else 3)], "v210 + %s, %d layers" % (fmt, n), route=SHARED % 2)


def test_four_outputs_in_one_launch():
    check(384, 6, 4, [out("nv12"), out("v210"), out("bgra8"), out("yuv422p10")], "four outputs", route=SHARED % 4)


def test_every_layer_shows():
    """the poison reaches the oracle's frame from every layer: swapping any one lower layer for another frame changes it"""
    w, h, n = 384, 6, 4
    rd_o, _ = reader()
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    layers = layer_words(w, h, n)
    want = orc.pipeline_v210_combine(layers, w, h, *rd_o, *wr_o)
    comp = composite(w, h, n, rd_o)
    assert np.array_equal(np.asarray(orc.v210_write(comp, w, h, 0, *wr_o)).reshape(-1), np.asarray(want).reshape(-1))
    for l in range(n - 1):
        alt = list(layers)
        alt[l] = frames.v210_random(w, h, 0xABC0 + l, legal=False)
        assert not np.array_equal(orc.pipeline_v210_combine(alt, w, h, *rd_o, *wr_o), want), l


# ---- writer tables ------------------------------------------------------------------------------------------------------------------
def test_two_tables_in_one_launch():
    """a table of other contents (tests/luts.py) and a table of equal contents under a second pointer, interleaved with the shared one:
    outputs keep their order and each output's bytes come from its own table"""
    tab = luts.layout_table(32, 8, 0xF00D)
    with luts.register(tab) as dtab:
        outs = [out("v210"), out("yuv422p8", spec=(tab, dtab)), out("rgba8", own_table=True), out("nv12")]
        _, got = check(384, 6, 3, outs, "three tables, outputs interleaved", route=SHARED % 4)
        _, same = check(384, 6, 3, [out("yuv422p8")], "the same output from the shared table", separate=False)
        assert not np.array_equal(got[1][0], same[0][0]), "the table of other contents does not show in its output"
        check(384, 6, 3, [out("bgra8", spec=(tab, dtab)), out("v210", 1, spec=(tab, dtab)), out("bgra8")], "two outputs on the other table")


@pytest.mark.parametrize("rl,wl", [(luts.SMALLEST, luts.LARGEST), (luts.LARGEST, luts.SMALLEST)], ids=["wr-largest", "rd-largest"])
def test_table_layouts(rl, wl):
    """a 157 712-byte writer table beside a smaller reader table, and the reverse (the launch's LDS is the largest table's)"""
    import hip_harness as hh
    from phaneron_amd import capi
    from test_lut_layouts_gpu import forced, gamut12
    with forced(rl, "r") as (rtab, drtab), forced(wl, "w") as (wtab, dwtab):
        rd = ((orc.ycbcr2rgb_matrix("709"), rtab, luts.IDENTITY), (hh.dev(capi.ycbcr2rgb_matrix("709")), drtab, hh.dev(gamut12())))
        outs = [out("v210", spec=(wtab, dwtab)), out("yuv422p10", spec=(wtab, dwtab)), out("rgba8")]
        check(384, 6, 2, outs, "layouts %r / %r" % (rl, wl), rd=rd, route=SHARED % 3)


# ---- lines ---------------------------------------------------------------------------------------------------------------------------
def test_field_mixes_on_an_odd_height():
    """96 x 9 (fields of 5 and 4 lines, of which a field write makes 4), no 4:2:0 output"""
    w, h = 96, 9
    _, got = check(w, h, 3, [out("v210", 1), out("rgba8", 0), out("bgra8", 3), out("v210", 3)], "96x9 fields", route=SHARED % 4)
    rows = got[0][0].reshape(h, -1)
    assert (rows[1::2] == POISON).all() and (rows[8] == POISON).all() and not (rows[0:8:2] == POISON).all(), "a v210 field 1 output takes lines 0, 2, 4, 6 only"
    rows = got[2][0].reshape(h, -1)
    assert (rows[0::2] == POISON).all() and not (rows[1::2] == POISON).all(), "a bgra8 field 3 output takes the odd lines only"
    check(w, h, 2, [out("yuv422p8", 3), out("yuv422p10", 0)], "96x9 planar 4:2:2 field beside a frame")


def test_a_420_field_beside_a_420_frame():
    w, h = 384, 10
    _, got = check(w, h, 3, [out("yuv420p", 3), out("nv12", 0), out("v210", 1), out("yuv422p8", 3)], "384x10: 4:2:0 field 3 + 4:2:0 frame", route=SHARED % 4)
    luma = got[0][0].reshape(h, w)
    assert (luma[0::2] == POISON).all() and not (luma[1::2] == POISON).all(), "a yuv420p field 3 output takes the odd lines only"
    check(w, h, 2, [out("nv12", 1), out("yuv420p", 0)], "384x10: nv12 field 1 + yuv420p frame")


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_default_workgroups_begin_in_mid_line():
    """1920 x 8: 2560 quads, three workgroups of 854 quads - ranges that begin and end in mid-line - with 4:2:0 outputs"""
    check(1920, 8, 2, [out("nv12"), out("yuv420p"), out("v210")], "1920x8, default workgroups", route=SHARED % 3)


@pytest.mark.parametrize("w,h,wgs,why", [(384, 48, 1, "three full slices a lane"), (768, 50, 1, "a second tile of 256 quads that four waves hold"),
                                         (96, 33, 2, "ranges of 264 quads: a partly filled wave")])
def test_capped_workgroups(w, h, wgs, why):
    import hip_harness as hh
    k = hh.ctx()
    k.set_option("fused_multi_wgs", wgs)
    try:
        outs = [out("v210"), out("rgba8", 3), out("yuv422p8")] if h % 2 else [out("v210"), out("nv12", 3), out("yuv420p"), out("bgra8")]
        check(w, h, 2, outs, "%dx%d, %d workgroups (%s)" % (w, h, wgs, why), route=SHARED % len(outs))
    finally:
        k.set_option("fused_multi_wgs", 0)


def test_the_option_refuses_a_negative_cap():
    import hip_harness as hh
    from phaneron_amd import capi
    with pytest.raises(capi.PhaneronError, match="fused_multi_wgs"):
        hh.ctx().set_option("fused_multi_wgs", -1)


# ---- fallback -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,fmts", [(1280, 6, ("v210", "yuv422p8", "nv12")), (100, 4, ("v210", "rgba8"))])
def test_other_widths_take_the_channel_kernels_route(w, h, fmts):
    check(w, h, 3, [out(f) for f in fmts], "%dx%d" % (w, h), route=r"chan_compose_multi<\d>x%d" % len(fmts))


def test_one_output_of_another_width_is_ph_chan_compose():
    check(1280, 6, 2, [out("yuv422p8")], "1280x6 yuv422p8 alone", route=r"chan_compose_v210<\d,\d>")


def test_without_lds_tables_the_answer_is_ph_chan_compose_multis():
    """option "lds_lut" = 0: no table has an LDS form, so the call does not qualify and runs ph_chan_compose_multi - whose answer, a
    refusal that names the reader's table, is this call's too; nothing is written"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 6
    _, rd_d = reader()
    k = hh.ctx()
    dl = [hh.dev(l) for l in layer_words(w, h, 2)]
    outputs = [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in ("v210", "rgba8")]
    k.set_option("lds_lut", False)
    try:
        texts = []
        for call in (lambda: k.fused_v210_combine_multi(dl, outputs, w, h, *rd_d), lambda: k.chan_compose_multi(chan_layers(dl, w, h), outputs, w, h, *rd_d)):
            with pytest.raises(capi.PhaneronError, match=r"error -1: .*reader gamma LUT has no LDS form") as e:
                call()
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    finally:
        k.set_option("lds_lut", True)
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every refusal is PH_E_INVALID (-1), decided before anything is launched: every plane keeps its poison"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, rd_d = reader()
    w0, h0 = 384, 8

    def attempt(specs, match, tweak=None, n=2, w=w0, h=h0, rd=None, drop_layer=False):
        dl = [hh.dev(l) for l in layer_words(w0, h0 + 1, max(n, 1))][:n]  # (frames of 384 x 9: large enough for every case)
        if drop_layer:
            dl[1] = None
        outputs = []
        for fmt in specs:
            f = packfmt.get(fmt)
            cm, lut = (writer(fmt, "709")[2:]) if fmt in orc.FORMAT_RANGE else hh.ColourParams.writer("709")
            outputs.append(dict(fmt=fmt, planes=[hh.dev(np.full(nb, POISON, np.uint8)) for nb in f.plane_bytes(w, h + (h & 1))], interlace=0, wr_cm=cm, wr_lut=lut))
        if tweak:
            tweak(outputs)
        with pytest.raises(capi.PhaneronError, match=match):
            k.fused_v210_combine_multi(dl, outputs, w, h, *(rd or rd_d))
        assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"] if p is not None), "a refused call wrote (%s)" % match

    attempt(["v210", "rgba8"], r"error -1: .*NULL argument", rd=(None, rd_d[1], rd_d[2]))
    attempt(["v210", "rgba8"], r"error -1: .*NULL argument", rd=(rd_d[0], None, rd_d[2]))
    attempt(["v210", "rgba8"], r"error -1: .*NULL argument", rd=(rd_d[0], rd_d[1], None))
    attempt(["v210", "rgba8"], r"error -1: .*layer 1 is NULL", drop_layer=True)
    attempt(["v210", "rgba8"], r"error -1: .*1\.\.8 layers", n=0)
    attempt(["v210", "rgba8"], r"error -1: .*1\.\.8 layers", n=9)
    attempt([], r"error -1: .*1\.\.4 outputs")
    attempt(["v210", "rgba8", "bgra8", "yuv422p8", "nv12"], r"error -1: .*1\.\.4 outputs")
    attempt(["v210", "rgba8"], r"error -1: .*output 1.*format 99 is not a PH_FMT", lambda o: o[1].update(fmt=99))
    for fmt in packfmt.NOT_CHAN_OUT:
        attempt(["v210", fmt], r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt)
        attempt([fmt], r"error -1: .*%s.*run the separate kernels.*ph_pack_write" % fmt)
    attempt(["v210", "rgba8"], r"error -1: .*output 1.*interlace must be 0, 1 or 3", lambda o: o[1].update(interlace=2))
    attempt(["v210"], r"error -1: .*output 0.*interlace must be 0, 1 or 3", lambda o: o[0].update(interlace=2))
    attempt(["v210", "rgba8"], r"error -1: .*output 0.*NULL argument", lambda o: o[0].update(planes=[None]))
    attempt(["v210", "yuv422p8"], r"error -1: .*output 1.*planar output needs its three planes", lambda o: o[1].update(planes=o[1]["planes"][:2] + [None]))
    attempt(["rgba8", "nv12"], r"error -1: .*output 1.*planar output needs its three planes", lambda o: o[1].update(planes=[o[1]["planes"][0], None]))
    attempt(["rgba8", "v210"], r"error -1: .*output 1.*matrix is missing", lambda o: o[1].update(wr_cm=None))
    attempt(["v210", "rgba8"], r"error -1: .*output 1.*NULL argument", lambda o: o[1].update(wr_lut=None))
    attempt(["rgba8", "yuv420p"], r"error -1: .*output 1.*4:2:0 frame needs an even height", h=9)
    attempt(["nv12"], r"error -1: .*output 0.*4:2:0 frame needs an even height", h=9)
    attempt(["v210", "rgba8"], r"error -1: .*same plane", lambda o: o[1].update(planes=o[0]["planes"]))
    plain = hh.dev(capi.linear2gamma_lut("709"))  # never registered: the call does not qualify, and ph_chan_compose_multi answers
    attempt(["v210", "rgba8"], r"error -1: .*output 1.*writer gamma LUT has no LDS form", lambda o: o[1].update(wr_lut=plain))


def test_null_arrays_and_a_zero_height():
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, rd_d = reader()
    w, h = 384, 6
    dl = [hh.dev(l) for l in layer_words(w, h, 1)]
    planes = [hh.dev(p) for p in poisoned("rgba8", w, h)]
    outs = k._chan_outputs([dict(fmt="rgba8", planes=planes, interlace=0, wr_cm=None, wr_lut=writer("rgba8", "709")[3])])
    arr = (ctypes.c_void_p * 1)(dl[0].data_ptr())
    fn, rd = capi.lib().ph_fused_v210_combine_multi, [ctypes.c_void_p(t.data_ptr()) for t in rd_d]
    assert fn(k.h, capi.QUEUE_PROCESS, 1, None, 1, outs, w, h, *rd) == -1
    assert fn(k.h, capi.QUEUE_PROCESS, 1, arr, 1, None, w, h, *rd) == -1
    assert fn(k.h, capi.QUEUE_PROCESS, 1, arr, 1, outs, 0, h, *rd) == -1
    assert fn(k.h, capi.QUEUE_PROCESS, 1, arr, 1, outs, w, 0, *rd) == 0  # an empty frame: PH_OK, nothing launched
    assert (hh.host(planes[0], np.uint8) == POISON).all()


# ---- by name: fused_v210_combine_multi_<n> ------------------------------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(384, 6)
    yield b
    b.close()


def three_outputs(b, sources):
    """n plain layers for v210 (output 0), yuv422p8 (1) and rgba8, field 3 (2)"""
    capi = b.capi
    o0, o1, o2 = b.planes("v210"), b.planes("yuv422p8"), b.planes("rgba8")
    params = dict(b.recipe, output=o0[0], interlace=0,
                  out1Packing=capi.FORMATS["yuv422p8"], output1=o1[0], output1U=o1[1], output1V=o1[2], out1ColMatrix=b.cm8, out1GammaLut=b.recipe["outGammaLut"], interlace1=0,
                  out2Packing=capi.FORMATS["rgba8"], output2=o2[0], out2GammaLut=b.recipe["outGammaLut"], interlace2=3)
    for i, s in enumerate(sources):
        params["l%dIn" % i] = s
    return params, (o0, o1, o2)


def expect_three(b, comp):
    w, h = b.w, b.h
    wlut = orc.linear2gamma_lut("709")
    return [oracle_frame("v210", comp, w, h, 0, orc.rgb2ycbcr_matrix("709"), wlut),
            oracle_frame("yuv422p8", comp, w, h, 0, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["yuv422p8"]), wlut),
            oracle_frame("rgba8", comp, w, h, 3, None, wlut)]


def test_by_name_run_program(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    words = layer_words(w, h, 2)
    params, outs = three_outputs(b, [b.upload(l, svm="coarse") for l in words])
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])
    b.ctx.run_program(prog, params, check_only=True)
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a check wrote"
    with b.capi.trace() as t:
        b.ctx.run_program(prog, params)
    b.ctx.wait()
    assert t.route == SHARED % 3, t.route
    want = expect_three(b, orc.combine([orc.v210_read(l, w, h, *b.rd_o) for l in words]))
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    prog.destroy()


def test_by_name_checks_and_runs_give_the_same_answers(by_name):
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    params, outs = three_outputs(b, [b.upload(l, svm="coarse") for l in layer_words(w, h, 2)])
    small = b.upload(np.zeros(64, np.uint8))
    b.ctx.wait(capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])

    def without(d, *names):
        return {k: v for k, v in d.items() if k not in names}
    defects = [(without(params, "l1In"), "l1In"), (dict(params, l0In=small), "l0In"), (without(params, "gammaLut"), "gammaLut"),
               (dict(params, out1Packing=99), "out1Packing"), (dict(params, out2Packing=capi.FORMATS["p010"]), "p010"),
               (dict(params, output1=small), "output1"), (without(params, "output1U"), "output1U"), (without(params, "out1ColMatrix"), "out1ColMatrix"),
               (without(params, "out2GammaLut"), "out2GammaLut"), (without(params, "outGammaLut"), "outGammaLut"),
               (dict(params, interlace2=2), "'interlace2': must be 0, 1 or 3"), (dict(params, output=params["output2"]), "'output2': the buffer is another output's too")]
    for bad, needle in defects:
        seen = []
        for check_only in (True, False):
            with pytest.raises(capi.PhaneronError) as e:
                b.ctx.run_program(prog, bad, check_only=check_only)
            seen.append(str(e.value))
        assert seen[0] == seen[1], "%s: check %r, run %r" % (needle, seen[0], seen[1])
        assert needle in seen[0], seen[0]
    for planes in outs:
        for p in planes:
            assert (b.read(p) == POISON).all(), "a refused job wrote"
    prog.destroy()


def test_by_name_run_programs_keeps_order(by_name):
    """a headline job that WRITES the multi job's layer 0 in front of it and a job that READS its output 2 behind it, in one
    ph_run_programs call"""
    b, w, h = by_name, by_name.w, by_name.h
    capi = b.capi
    first, second = layer_words(w, h, 2)
    stale = b.upload(np.full(frames.v210_pitch_bytes(w) * h, POISON, np.uint8), svm="coarse")  # what the first job overwrites
    last_out = b.planes("v210")[0]
    params, outs = three_outputs(b, [stale, b.upload(second, svm="coarse")])
    head = b.ctx.create_program("phaneron:fused", "fused_v210_combine_1", [w, h])
    multi = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])
    chan = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [w, h])
    jobs = [(head, dict(b.recipe, l0In=b.upload(first, svm="coarse"), output=stale)),
            (multi, params),
            (chan, dict(b.recipe, l0In=outs[2][0], l0Packing=capi.FORMATS["rgba8"], l0Width=w, l0Height=h, output=last_out))]
    b.ctx.wait(capi.QUEUE_LOAD)
    with capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels[:2] == ["fused_v210_combine_lds", SHARED % 3], t.route
    wr_o = (orc.rgb2ycbcr_matrix("709"), orc.linear2gamma_lut("709"))
    frame0 = np.asarray(orc.v210_write(orc.v210_read(first, w, h, *b.rd_o), w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(stale).view(np.uint32), frame0.view(np.uint32))
    want = expect_three(b, orc.combine([orc.v210_read(frame0.view(np.uint32), w, h, *b.rd_o), orc.v210_read(second, w, h, *b.rd_o)]))
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "output %d plane %d" % (i, pl)
    # the last job read output 2 as it stood after the multi job: its field-3 lines written, the others still poison
    img = packfmt.get("rgba8").oracle_read([want[2][0]], w, h, None, b.rd_o[1], b.rd_o[2])
    last = np.asarray(orc.v210_write(img, w, h, 0, *wr_o)).reshape(-1)
    assert np.array_equal(b.read(last_out).view(np.uint32), last.view(np.uint32))
    head.destroy(), multi.destroy(), chan.destroy()


# ---- guard bands --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(384, 6), (1920, 8)])
def test_between_guard_bands(w, h):
    """every layer and every plane of every output between guard bands: nothing outside a buffer is written, and nothing read outside
    one reaches an output"""
    guard.reset()
    try:
        def dst(p, fmt):
            return guard.dev(p, "dst", pitch=max(1, p.size // h))

        def src(l):
            return guard.dev(l, "src", pitch=frames.v210_pitch_bytes(w))
        check(w, h, 3, [out("v210"), out("yuv422p10"), out("yuv422p8", 3), out("rgba8")], "%dx%d between guards" % (w, h), separate=False, dst=dst, src=src)
        check(w, h, 3, [out("yuv420p"), out("nv12", 1), out("bgra8", 3), out("v210", 1)], "%dx%d between guards" % (w, h), separate=False, dst=dst, src=src)
        assert guard.check() == (6, 15)
    finally:
        guard.reset()


# ---- seeded campaign ----------------------------------------------------------------------------------------------------------------
def test_random_outputs_of_random_frames():
    """40 seeded cases: 1..8 layers, a width of 48 / 96 / 384 / 768, a height of 1..12 (even wherever a 4:2:0 output is drawn, so the
    generator never discards a case), 1..4 outputs of random formats, field modes and writer tables"""
    r = np.random.default_rng(20261019)
    for case in range(40):
        n = int(r.integers(1, 9))
        w = int(r.choice([48, 96, 384, 768]))
        outs = [out(str(r.choice(ALL_OUT)), int(r.choice([0, 0, 1, 3])), spec=str(r.choice(["709", "709", "2020"]))) for _ in range(int(r.integers(1, 5)))]
        h = int(r.integers(1, 13))
        if any(o["fmt"] in ("yuv420p", "nv12") for o in outs):
            h += h & 1
        check(w, h, n, outs, "case %d: %dx%d, %d layers, outputs %r" % (case, w, h, n, [(o["fmt"], o["interlace"], o["spec"]) for o in outs]), seed=100 + case,
              separate=case % 4 == 0)


# ---- full size ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_full_size_equals_the_channel_kernels_bytes(w, h):
    """4 layers, v210 + bgra8 + yuv422p8 at full size against ph_chan_compose_multi's bytes (that call is itself oracle-pinned at full
    size: test_fullsize_gpu)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, 4, seed=31)]
    fmts = ("v210", "bgra8", "yuv422p8")

    def outputs():
        return [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=0, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in fmts]
    mine, theirs = outputs(), outputs()
    with capi.trace() as t:
        k.fused_v210_combine_multi(dl, mine, w, h, *rd_d)
    assert t.route == SHARED % 3, t.route
    k.chan_compose_multi(chan_layers(dl, w, h), theirs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    for a, b in zip(mine, theirs):
        for pl, (p, q) in enumerate(zip(a["planes"], b["planes"])):
            assert torch.equal(p, q), "%dx%d %s plane %d differs from ph_chan_compose_multi's" % (w, h, a["fmt"], pl)
            assert not bool((p == POISON).all())
    del _layers[(w, h, 31)]
