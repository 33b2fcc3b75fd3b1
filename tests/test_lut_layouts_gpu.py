"""GPU tests (-m gpu) of the LDS gamma table in every layout lut_compress can choose (ph_lut.h, ph_ldslut.h): tests/luts.py forces a
layout with a table made for it, and the inputs make the kernels visit EVERY index - asserted on the oracle's output (index_probe()),
never on the code under test.  The readers run under an identity gamut, so their f32 output is the table entry itself: one wrong bit
of an anchor or a delta shows.  Then two tables in one launch in every size order (the writer's larger than the reader's has no
other test), and tap sharing when the room behind a 157712-byte table does not take every op.  Every comparison is bit for bit
(f32 images) or word / byte for byte (packed frames) against the oracle."""
import contextlib
import functools
import re

import numpy as np
import pytest

import frames
import luts
import packfmt
from oracle import orc
from test_chan_gpu import Src, both_routes, channel_variants, check, check_batch, check_format, device_layers, dry_route, m, pip_layers
from test_chan_multi_gpu import mixed_program

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def table(bias, m_, role):
    """the forced table of a layout; role: "r" / "w" / "w2" - a reader's, a writer's and a second writer's table differ"""
    return luts.layout_table(bias, m_, 0x1A7 + 16 * bias + m_ + {"r": 0, "w": 1000, "w2": 2000}[role])


@contextlib.contextmanager
def forced(layout, role="r"):
    """(host table, registered device table) of a layout; the registry must report the layout that was meant"""
    import hip_harness as hh
    tab = table(layout[0], layout[1], role)
    with luts.register(tab) as dev:
        info = hh.ctx().lut_info(dev)
        assert info == dict(lds_bytes=luts.LDS_BYTES[layout], index_bias=layout[0], blocks_per_octave_log2=layout[1]), (layout, info)
        yield tab, dev


def gamut12():
    return np.concatenate([luts.IDENTITY, np.zeros(3, np.float32)])


def bits_eq(got, want, what):
    a, b = np.ascontiguousarray(got).reshape(-1).view(np.uint32), np.ascontiguousarray(want, np.float32).reshape(-1).view(np.uint32)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, "%s: %d of %d f32 words differ, first at %d (pixel %d): got %08x, want %08x" % (
        what, bad.size, a.size, bad[0], bad[0] // 4, a[bad[0]], b[bad[0]])


def same_planes(got, want, what):
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g).reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s plane %d: %d of %d bytes differ, first at %d" % (what, i, bad.size, g.size, bad[0])


def covered(fmt, kind):
    why = luts.reader_coverage(fmt, kind)
    assert why is None, why


# ---- 3a: every index of every layout through the single-table kernels -----------------------------------------------------------
@pytest.mark.parametrize("kind", ["std", "general"])
@pytest.mark.parametrize("layout", luts.LAYOUTS, ids=lambda l: "bias%d-m%d" % l)
def test_v210_read_every_index_of_every_layout(layout, kind):
    """a 1282-wide frame (213 whole quads and a 4-pixel tail per line) under which the oracle uses all 65536 indices in R, in G and
    in B - with the 709 matrix (read_px_lds' STD path) and with a matrix of another shape (the general dot products)"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    covered("v210", kind)
    (words,), w, h, cm = luts.reader_case("v210", kind)
    with forced(layout) as (tab, dtab):
        out = torch.full((w * h * 4,), float("nan"), dtype=torch.float32, device="cuda")
        src, dcm, dgm = hh.dev(words), hh.dev(cm), hh.dev(gamut12())
        with capi.trace() as t:
            hh.ctx().v210_read(src, out, w, h, dcm, dtab, dgm)
        assert t.route == "v210_read_lds", t.route
        bits_eq(hh.host(out), orc.v210_read(words, w, h, cm, tab, luts.IDENTITY), "v210_read %s layout %r" % (kind, layout))


@pytest.mark.parametrize("layout", luts.LAYOUTS, ids=lambda l: "bias%d-m%d" % l)
def test_v210_write_every_index_of_every_layout(layout):
    """an image whose R, G and B each hold every index, every exact tie i + 0.5 and the ties' neighbours (a different order per
    channel) and the special values; 1282 wide: each line ends in a tail, whose indices are truncated.  (A wrong delta shows only
    where it moves the 10-bit code - luts.layout_table - the reader tests are the exact ones.)"""
    import hip_harness as hh
    from phaneron_amd import capi
    why = luts.writer_coverage()
    assert why is None, why
    img = luts.writer_image()
    h, w = img.shape[:2]
    wcm = orc.rgb2ycbcr_matrix("709")
    with forced(layout, "w") as (tab, dtab):
        for il in (0, 3):
            dst = np.full(frames.v210_pitch_bytes(w) * h // 4, 0x2AAAAAAA, np.uint32)
            out, src, dcm = hh.dev(dst), hh.dev(img), hh.dev(capi.rgb2ycbcr_matrix("709"))
            with capi.trace() as t:
                hh.ctx().v210_write(src, out, w, h, il, dcm, dtab)
            assert t.route == "v210_write_lds", t.route
            want = np.asarray(orc.v210_write(img, w, h, il, wcm, tab, out=dst.copy())).reshape(-1)
            got = hh.host(out, np.uint32)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "v210_write layout %r il %d: %d of %d words differ, first at word %d" % (layout, il, bad.size, got.size, bad[0])


@pytest.mark.parametrize("layout", luts.THREE, ids=lambda l: "bias%d-m%d" % l)
def test_v210_read_batch_every_index(layout):
    """two frames in one launch: the covering frame and the same lines in reverse order, under each matrix"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    with forced(layout) as (tab, dtab):
        for kind in ("std", "general"):
            covered("v210", kind)
            (words,), w, h, cm = luts.reader_case("v210", kind)
            srcs = [words, np.ascontiguousarray(words.reshape(h, -1)[::-1]).reshape(-1)]
            outs = [torch.full((w * h * 4,), float("nan"), dtype=torch.float32, device="cuda") for _ in srcs]
            ins, dcm, dgm = [hh.dev(x) for x in srcs], hh.dev(cm), hh.dev(gamut12())
            with capi.trace() as t:
                hh.ctx().v210_read_batch(ins, outs, w, h, dcm, dtab, dgm)
            assert t.route == "v210_read_lds_batch", t.route
            for i, x in enumerate(srcs):
                bits_eq(hh.host(outs[i]), orc.v210_read(x, w, h, cm, tab, luts.IDENTITY), "v210_read_batch %s layout %r frame %d" % (kind, layout, i))


def reader_kinds(fmt):
    """the matrices a format's reader is taken through: RGB formats have none"""
    return ["std"] if packfmt.get(fmt).code_range is None else ["std", "general"]


@pytest.mark.parametrize("fmt", packfmt.STANDALONE)
@pytest.mark.parametrize("layout", luts.THREE, ids=lambda l: "bias%d-m%d" % l)
def test_pack_read_and_read_batch_every_index(layout, fmt):
    """10-bit formats: all 65536 indices in every channel under both matrices; 8-bit planar ones under the general matrix (Y * 256 + C),
    and every input code in every plane under their standard one; rgba8 / bgra8: every code in every byte lane"""
    import torch
    import hip_harness as hh
    f = packfmt.get(fmt)
    with forced(layout) as (tab, dtab):
        for kind in reader_kinds(fmt):
            covered(fmt, kind)
            planes, w, h, cm = luts.reader_case(fmt, kind)
            want = f.oracle_read(planes, w, h, cm, tab, luts.IDENTITY)
            dcm, dgm = None if cm is None else hh.dev(cm), hh.dev(gamut12())
            out = torch.full((w * h * 4,), float("nan"), dtype=torch.float32, device="cuda")
            dplanes = [hh.dev(p) for p in planes]
            hh.ctx().pack_read(fmt, dplanes, out, w, h, dcm, dtab, dgm)
            bits_eq(hh.host(out), want, "%s pack_read %s layout %r" % (fmt, kind, layout))
            outs = [torch.full((w * h * 4,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
            again = [hh.dev(p) for p in planes]
            hh.ctx().pack_read_batch(fmt, [dplanes, again], outs, w, h, dcm, dtab, dgm)
            for i in range(2):
                bits_eq(hh.host(outs[i]), want, "%s pack_read_batch %s layout %r frame %d" % (fmt, kind, layout, i))


@pytest.mark.parametrize("fmt", packfmt.STANDALONE)
@pytest.mark.parametrize("layout", luts.THREE, ids=lambda l: "bias%d-m%d" % l)
def test_pack_write_every_index(layout, fmt):
    """the writer image (every index, tie and neighbour per channel) through every format's writer, whole frames and field 3"""
    import hip_harness as hh
    f = packfmt.get(fmt)
    why = luts.writer_coverage()
    assert why is None, why
    img = luts.writer_image()
    h, w = img.shape[:2]
    wcm = f.writer_matrix("709")
    with forced(layout, "w") as (tab, dtab):
        dcm = None if wcm is None else hh.dev(wcm)
        src = hh.dev(img)
        for il in (0, 3):
            dst = f.poisoned(w, h)
            dplanes = [hh.dev(d) for d in dst]
            hh.ctx().pack_write(fmt, src, dplanes, w, h, il, dcm, dtab)
            same_planes([hh.host(p) for p in dplanes], f.oracle_write(img, w, h, il, wcm, tab, dst), "%s pack_write layout %r il %d" % (fmt, layout, il))


@pytest.mark.parametrize("layout", luts.THREE, ids=lambda l: "bias%d-m%d" % l)
def test_v210_yadif_pair_every_index(layout):
    """the fused de-interlacing reader (whole quads only: 1278 wide) under the 709 matrix and under a matrix of another shape (the
    kernel has its own branch on the matrix's shape): the covering frame as the current frame of the window, its lines rolled by
    one and by two as the previous and the next one"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    with forced(layout) as (tab, dtab):
        for kind in ("std", "general"):
            cm = luts.std_matrix() if kind == "std" else luts.general_matrix()
            y, cb, cr = luts.codes10(kind, w=1278)
            h, w = y.shape
            cur = frames.v210_pack_codes(y, cb, cr, w, h)
            idx = orc.v210_read(cur, w, h, cm, luts.index_probe(), luts.IDENTITY)
            gaps = [luts.missing(idx[..., ch]) for ch in range(3)]
            assert not any(gaps), "the 1278-wide %s frame leaves out %r of the 65536 indices in R, G, B (oracle)" % (kind, gaps)
            wins = [frames.v210_pack_codes(np.roll(y, k, 0), np.roll(cb, k, 0), np.roll(cr, k, 0), w, h) for k in (1, 0, 2)]
            outs = [torch.full((w * h * 4,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
            dw, dcm, dgm = [hh.dev(x) for x in wins], hh.dev(cm), hh.dev(gamut12())
            with capi.trace() as t:
                hh.ctx().v210_yadif_pair([(dw[0], dw[1], dw[2], outs[0], outs[1])], w, h, 1, False, dcm, dtab, dgm)
            assert "yadif_pair" in t.route, t.route
            p, c, n = (orc.v210_read(x, w, h, cm, tab, luts.IDENTITY) for x in wins)
            for parity in (0, 1):
                bits_eq(hh.host(outs[parity]), orc.yadif(p, c, n, parity, 1, False), "v210_yadif_pair %s layout %r parity %d" % (kind, layout, parity))


# ---- 3b: two tables in one launch, in every size order ----------------------------------------------------------------------------
PAIRINGS = [(luts.SMALLEST, luts.LARGEST), (luts.LARGEST, luts.SMALLEST), (luts.LARGEST, luts.LARGEST)]


@pytest.fixture(params=PAIRINGS, ids=["wr-larger", "rd-larger", "both-largest"])
def pair(request):
    """reader and writer colour tuples (as test_chan_gpu.colour takes them) with forced tables: the 709 matrices, an identity gamut.
    Also a second writer table of the OTHER size than the writer's (the several-outputs launchers take the maximum over outputs)."""
    import hip_harness as hh
    from phaneron_amd import capi
    rl, wl = request.param
    w2 = luts.SMALLEST if wl == luts.LARGEST else luts.LARGEST
    with forced(rl, "r") as (rtab, drtab), forced(wl, "w") as (wtab, dwtab), forced(w2, "w2") as (w2tab, dw2tab):
        rd = ((orc.ycbcr2rgb_matrix("709"), rtab, luts.IDENTITY), (hh.dev(capi.ycbcr2rgb_matrix("709")), drtab, hh.dev(gamut12())))
        wr = ((orc.rgb2ycbcr_matrix("709"), wtab), (hh.dev(capi.rgb2ycbcr_matrix("709")), dwtab))
        yield dict(rd=rd, wr=wr, wr_table=(wtab, dwtab), wr2_table=(w2tab, dw2tab), layouts=(rl, wl, w2))


def own_scale(w, h, seed, **kw):
    """a v210 source sampled at its own scale (tap sharing is on: its halo sits right behind the larger table)"""
    return dict(src=Src(frames.v210_random(w, h, frames.layer_seed(seed, 0)), w, h, m(w, h, **kw)))


def test_fused_v210_combine_pairings(pair):
    """the headline kernel, one frame and two jobs: whole 48-pixel blocks, and lines with tails"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, rd_d = pair["rd"]
    wr_o, wr_d = pair["wr"]
    for w, h in ((192, 54), (1280, 10), (100, 9)):
        jobs = [[frames.v210_random(w, h, frames.layer_seed(50 + j, l), legal=(l != 2)) for l in range(4)] for j in range(2)]
        want = [orc.pipeline_v210_combine(layers, w, h, *rd_o, *wr_o) for layers in jobs]
        words = frames.v210_pitch_bytes(w) * h // 4
        dl = [[hh.dev(l) for l in layers] for layers in jobs]
        one = torch.zeros(words, dtype=torch.int32, device="cuda")
        with capi.trace() as t:
            hh.ctx().fused_v210_combine(dl[0], one, w, h, *rd_d, *wr_d)
        assert t.route == "fused_v210_combine_lds", t.route
        assert np.array_equal(hh.host(one, np.uint32), want[0]), "fused_v210_combine %dx%d layouts %r" % (w, h, pair["layouts"])
        outs = [torch.zeros(words, dtype=torch.int32, device="cuda") for _ in range(2)]
        with capi.trace() as t:
            hh.ctx().fused_v210_combine_batch(dl, outs, w, h, *rd_d, *wr_d)
        assert set(t.kernels) == {"fused_v210_combine_lds"}, t.route
        for j in range(2):
            assert np.array_equal(hh.host(outs[j], np.uint32), want[j]), "fused_v210_combine_batch %dx%d job %d layouts %r" % (w, h, j, pair["layouts"])


def test_chan_compose_v210_pairings(pair):
    """the channel kernel's three instantiations - whole 48-pixel blocks, lines with tails, planar / RGB sources - each with a v210
    source at its own scale among the layers (shared taps: the halo lies behind the larger table)"""
    specs = (pair["rd"], pair["wr"])
    cases = [(192, 54, r"chan_compose_v210<0,0>", pip_layers(192, 54, 60) + [own_scale(192, 54, 61, offset_x=6.0 / 192, offset_y=-2.0 / 54)]),
             (100, 9, r"chan_compose_v210<1,0>", [own_scale(100, 9, 62)] + pip_layers(100, 9, 63, 3)),
             (1280, 10, r"chan_compose_v210<1,0>", [own_scale(1280, 10, 64)] + pip_layers(1280, 10, 65, 2) + [own_scale(1280, 10, 66, offset_x=0.3 / 1280 + 0.25)]),
             (384, 33, r"chan_compose_v210<[2-5],0>", [own_scale(384, 33, 67)] + mixed_program(384, 33, 68))]
    for w, h, route, layers in cases:
        for il in (0, 3):
            check(layers, w, h, "%dx%d il %d layouts %r" % (w, h, il, pair["layouts"]), interlace=il, specs=specs, poison_dst=True)
        got = dry_route(layers, w, h, 0, specs)
        assert re.fullmatch(route, got), "%dx%d: route %r" % (w, h, got)


@pytest.mark.parametrize("fmt", ["yuv422p8", "nv12", "bgra8", "yuv422p10"])
def test_chan_compose_other_formats_pairings(pair, fmt):
    w, h = 192, 54
    layers = [own_scale(w, h, 70)] + pip_layers(w, h, 71, 3)
    check_format(layers, w, h, fmt, "%s layouts %r" % (fmt, pair["layouts"]), reader=pair["rd"], wr_table=pair["wr_table"])
    check_format(mixed_program(384, 54, 72), 384, 54, fmt, "%s planar layouts %r" % (fmt, pair["layouts"]), interlace=3, reader=pair["rd"], wr_table=pair["wr_table"])


def test_chan_compose_multi_pairings(pair):
    """two outputs that bring writer tables of different sizes, in both orders: the launcher sizes the LDS by the largest of the call"""
    from test_chan_multi_gpu import check_multi, out
    a, b = pair["wr_table"], pair["wr2_table"]
    for w, h, layers in ((192, 54, [own_scale(192, 54, 80)] + pip_layers(192, 54, 81, 3)), (100, 9, [own_scale(100, 9, 82)] + pip_layers(100, 9, 83, 2)),
                         (384, 54, mixed_program(384, 54, 84))):
        for first, second in ((a, b), (b, a)):
            fmt2 = "rgba8" if w % 8 else "yuv422p8"
            route = check_multi(layers, w, h, [out("v210", spec=first), out(fmt2, 0 if h & 1 else 3, spec=second)],
                                "%dx%d layouts %r" % (w, h, pair["layouts"]), rspec=pair["rd"])
            assert re.fullmatch(r"chan_compose_multi<\d>x2", route), route


def test_chan_compose_batch_pairings(pair):
    """two jobs in one launch: whole blocks, lines with tails, a planar job"""
    specs = (pair["rd"], pair["wr"])
    for w, h in ((192, 54), (100, 9)):
        v = channel_variants(w, h, 90 + w)
        jobs = [([own_scale(w, h, 91 + w)] + v[0], 0, 0), (v[1] + [own_scale(w, h, 92 + w, offset_x=6.0 / w)], 0, 1)]
        check_batch(jobs, w, h, "2 jobs %dx%d layouts %r" % (w, h, pair["layouts"]), specs=specs)
    w, h = 384, 54
    check_batch([(mixed_program(w, h, 93), 0, 0), ([own_scale(w, h, 94)] + pip_layers(w, h, 95, 2), 3, 1)], w, h, "a planar job and a field, layouts %r" % (pair["layouts"],), specs=specs)


def test_chan_compose_batch_out_pairings(pair):
    """two jobs, each for two consumers, in one launch: against separate ph_chan_compose calls and against the oracle's chain"""
    import hip_harness as hh
    from test_chan_batch_out_gpu import run_both
    from test_chan_multi_gpu import composite, oracle_frame, out, writer
    for w, h in ((192, 54), (200, 10)):
        outs = [out("v210", spec=pair["wr_table"]), out("yuv422p8", 3 if h % 4 == 2 else 0, spec=pair["wr_table"])]
        programs = [[own_scale(w, h, 100 + w)] + pip_layers(w, h, 101 + w, 3), channel_variants(w, h, 102 + w)[1]]
        route, planes, _ = run_both([(layers, outs) for layers in programs], w, h, "%dx%d layouts %r" % (w, h, pair["layouts"]), rspec=pair["rd"])
        assert re.fullmatch(r"chan_compose_batch_out<\d>x2o4", route), route
        for j, layers in enumerate(programs):
            comp = composite(layers, w, h, pair["rd"][0])
            for i, o in enumerate(outs):
                rc = writer(o["fmt"], o["spec"])
                same_planes([hh.host(p, np.uint8) for p in planes[(j, i)]], oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]),
                            "%dx%d job %d output %d (%s) against the oracle" % (w, h, j, i, o["fmt"]))


@pytest.mark.parametrize("sw,sh,ow,oh,interlace", [(128, 36, 192, 54, 0), (52, 7, 100, 9, 3), (100, 24, 384, 33, 0), (128, 36, 1280, 10, 0)])
def test_enlarged_clips_pairings(pair, sw, sh, ow, oh, interlace):
    """v210 clips smaller than their channel, and a yuv420p clip beside one: read + 2 x 2-block compositor as two launches (what options
    1 and 2 both take for these programs) and the channel kernel.  The one-launch clip kernel: test_one_launch_clip_kernel_pairings"""
    specs = (pair["rd"], pair["wr"])
    clip = lambda seed, w, h, **kw: dict(src=Src(frames.v210_random(w, h, frames.layer_seed(seed, w + h), legal=bool(seed & 1)), w, h, m(ow, oh, **kw)))
    p420 = dict(src=Src(frames.pack_random("yuv420p", sw, sh + (sh & 1), 113), sw, sh + (sh & 1), m(ow, oh, scale_x=0.8, scale_y=0.8, offset_x=0.1), fmt="yuv420p"))
    cases = [[clip(110, sw, sh)], [clip(111, sw, sh), clip(112, sw, sh, scale_x=0.8, scale_y=0.8, offset_x=0.1, offset_y=-0.1)], [clip(114, sw, sh), p420]]
    for layers in cases:
        both_routes(lambda route: check(layers, ow, oh, "%d enlarged clips %dx%d on %dx%d il %d layouts %r by the %s" % (len(layers), sw, sh, ow, oh, interlace, pair["layouts"], route),
                                        interlace=interlace, specs=specs, poison_dst=bool(interlace)))


@pytest.mark.parametrize("sw,sh,ow,oh,interlace", [(128, 36, 192, 54, 0), (128, 18, 192, 54, 3), (200, 30, 384, 54, 0), (96, 24, 1280, 30, 0), (52, 8, 100, 10, 0)])
@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10", "bgra8"])
def test_one_launch_clip_kernel_pairings(pair, fmt, sw, sh, ow, oh, interlace):
    """ONE clip in its wire format filling the frame: reader and 2 x 2-block compositor in one launch (clip_up_write_v210_kernel), which
    loads the reader's table, then swaps the writer's in over it - a larger one in the first pairing - and keeps its rectangle
    descriptors behind the larger of the two (48 .. 6128 bytes of room).  Planar clips take the <rgb> instantiation, a bgra8 graphic
    (its alpha travels along) <rgba>; 192 and 384 wide: whole 48-pixel blocks, 1280 and 100: lines with tails.  The route is asserted
    for the default option; the same frame by the two-launch route and by the channel kernel as well."""
    import hip_harness as hh
    specs = (pair["rd"], pair["wr"])
    layers = [dict(src=Src(packfmt.get(fmt).random_planes(sw, sh, 140 + sw), sw, sh, m(ow, oh), fmt=fmt))]
    hh.ctx().set_option("chan_enlarged", 1)
    route = dry_route(layers, ow, oh, interlace, specs)
    assert route == "clip_up_write_v210<%s>" % ("rgba" if fmt == "bgra8" else "rgb"), "%s %dx%d on %dx%d il %d: route %r" % (fmt, sw, sh, ow, oh, interlace, route)
    both_routes(lambda how: check(layers, ow, oh, "one %s clip %dx%d on %dx%d il %d layouts %r by the %s" % (fmt, sw, sh, ow, oh, interlace, pair["layouts"], how),
                                  interlace=interlace, specs=specs, poison_dst=True))


def test_compose_up_write_multi_pairings(pair):
    """the 2 x 2-block compositor's several-outputs form (f32 images in: the writer's table is the only one), one table per launch and
    two tables of different sizes in one call"""
    from test_chan_multi_gpu import out
    from test_up_out_gpu import check as up_check, images
    a, b = pair["wr_table"], pair["wr2_table"]
    for ow, oh, sw, sh in ((192, 54, 96, 27), (100, 8, 40, 4), (1280, 10, 320, 5)):
        for rgb in (False, True):
            layers = images(ow, oh, [(sw, sh, dict()), (sw // 2, max(sh // 2, 1), dict(scale_x=0.5, scale_y=0.5, offset_x=-0.2, offset_y=0.1))], rgb, 120 + ow)
            up_check([layers], ow, oh, [out("v210", spec=a), out("rgba8", spec=a)], "%dx%d one table, layouts %r" % (ow, oh, pair["layouts"]), rgb)
            up_check([layers], ow, oh, [out("v210", spec=a), out("bgra8", spec=b)], "%dx%d two tables, layouts %r" % (ow, oh, pair["layouts"]), rgb)


# ---- 3c: tap sharing when it does not all fit ---------------------------------------------------------------------------------------
def sharing_ops_that_fit(out_w, lines, num_cus, table_bytes, behind_table):
    """chan_plan / chan_batch_plan (ph_kernels_chan.hip) restated: how many sharing ops get a halo behind a table of `table_bytes`,
    `behind_table` bytes of scheduling data in front of the halo (the batch kernels: 304)"""
    cpr = (out_w + 191) // 192
    cpg = 4 * cpr
    chunks = cpr * ((lines + 1) // 2)
    grid = min(chunks, num_cus)
    if grid % 8 == 0:
        groups = (chunks + cpg - 1) // cpg
        mine, vstep = (groups + 7) // 8, grid // 8
        slots = (mine * cpg + vstep - 1) // vstep
    else:
        slots = (chunks + grid - 1) // grid
    steps = 3 * slots
    room = 160 * 1024 - (((table_bytes + 15) & ~15) + behind_table)
    return min(8, room // (steps * 36)), steps, room


def test_tap_sharing_that_does_not_all_fit():
    """1920 x 1080, four v210 layers at their own scale, each moved a further eighth of the frame (so every layer shows), reader and
    writer table both (16, 9): 157712 bytes.  The launchers' arithmetic on a 256-CU device: 10 chunks per row, 5400 chunks, 256
    workgroups in 8 bands of 32, 135 groups of 40 chunks -> at most 17 groups = 680 chunks per band -> 22 slots, 66 wave steps per
    workgroup, 66 x 36 = 2376 bytes of halo per sharing op.  Behind the table are 163840 - 157712 = 6128 bytes (one frame) and 6128 -
    304 = 5824 (the batch kernel's scheduling data first): two ops fit (4752 bytes), the third (7128) does not - layers 2 and 3 go
    without sharing, in the one-frame call and in the 2-job batch (where ops 2 .. 7 do).  The numbers are recomputed for the device
    at hand and the test insists that at least one op shares and at least one goes without; the frames must equal the oracle's
    chain word for word either way.  The count comes from this file's restatement of the launchers' arithmetic (sharing_ops_that_fit):
    the route trace names the kernel, not the ops it marked, so nothing here observes the launcher's own n_share - if that
    arithmetic changes, restate it here, or the case may no longer hold an op that is denied sharing and still pass."""
    import torch
    w, h = 1920, 1080
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = luts.LDS_BYTES[luts.LARGEST]
    for behind in (0, 304):
        fit, steps, room = sharing_ops_that_fit(w, h, cus, big, behind)
        assert 1 <= fit < 4, "%d CUs: %d wave steps, %d bytes behind the table: %d sharing ops fit - the case needs some, not all four" % (cus, steps, room, fit)
    if cus == 256:
        assert sharing_ops_that_fit(w, h, cus, big, 0) == (2, 66, 6128) and sharing_ops_that_fit(w, h, cus, big, 304) == (2, 66, 5824)
    import hip_harness as hh
    from phaneron_amd import capi

    def program(seed):
        return [dict(src=Src(frames.v210_random(w, h, frames.layer_seed(seed, l)), w, h, m(w, h, offset_x=(240.0 * l + 0.25 * (l & 1)) / w, offset_y=135.0 * l / h)))
                for l in range(4)]
    with forced(luts.LARGEST, "r") as (rtab, drtab), forced(luts.LARGEST, "w") as (wtab, dwtab):
        rd = ((orc.ycbcr2rgb_matrix("709"), rtab, luts.IDENTITY), (hh.dev(capi.ycbcr2rgb_matrix("709")), drtab, hh.dev(gamut12())))
        wr = ((orc.rgb2ycbcr_matrix("709"), wtab), (hh.dev(capi.rgb2ycbcr_matrix("709")), dwtab))
        a, b = program(130), program(131)
        route = dry_route(a, w, h, 0, (rd, wr))
        assert route == "chan_compose_v210<0,0>", route
        frame = lambda: torch.zeros(frames.v210_pitch_bytes(w) * h // 4, dtype=torch.int32, device="cuda")
        with capi.trace(dry_run=True) as t:
            hh.ctx().chan_compose_batch([(device_layers(a), frame(), 0), (device_layers(b), frame(), 0)], w, h, *rd[1], *wr[1])
        assert t.route == "chan_compose_batch<0>x2", t.route
        # (check_batch compares each job with the oracle's chain AND with its own one-frame call: both forms are judged)
        check_batch([(a, 0, 0), (b, 0, 1)], w, h, "four own-scale layers behind a 157712-byte table", specs=(rd, wr))
