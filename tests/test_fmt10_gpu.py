"""GPU tests (-m gpu) of the 10-bit 4:2:0 decoder formats (yuv420p10le, p010le).  They have no reference kernel: a read is the
reference's yuv422p10 Reader on the 4:2:2 frame F' whose chroma line r is the source's line r >> 1 (p010: every word >> 6), a write
is its yuv422p10 Writer with the chroma taken from the upper line of a line pair (the lower one in field mode 3) - DESIGN.md 2.  So
every result is compared, bit for bit, with the oracle's yuv422p10 Reader / Writer and (where the build made it) the reference's own
yuv422p10 kernel run on this GPU, through the standalone, batch, channel-kernel and one-launch clip routes."""
import numpy as np
import pytest

import fmt10
import frames
import packfmt
import refgpu
import test_chan_gpu as chan
from oracle import orc

pytestmark = pytest.mark.gpu
SIZES = [(1920, 1080), (1280, 720), (718, 480), (3840, 2160)]
RSPEC, WSPEC = "709", "2020"
needs_ref = pytest.mark.skipif(not refgpu.available(), reason="oracle/_ref/refgpu is built where the reference checkout exists")


@pytest.fixture(params=["lds_lut", "global_lut"])
def lut_path(request):
    import hip_harness as hh
    hh.ctx().set_option("lds_lut", request.param == "lds_lut")
    yield request.param
    hh.ctx().set_option("lds_lut", True)


@pytest.fixture(scope="module")
def ref():
    return refgpu.RefGpu()


def reader_o():
    return orc.ycbcr2rgb_matrix(RSPEC), orc.gamma2linear_lut(RSPEC), orc.rgb2rgb_matrix(RSPEC, WSPEC)


def writer_o():
    return orc.rgb2ycbcr_matrix(WSPEC), orc.linear2gamma_lut(WSPEC)


def dev_planes(planes):
    import hip_harness as hh
    return [hh.dev(p) for p in fmt10.as_bytes(planes)]


def read_ours(fmt, planes, w, h):
    import torch
    import hip_harness as hh
    cm, lut, gm = hh.ColourParams.fmt_reader(fmt, RSPEC, WSPEC)
    d = dev_planes(planes)
    out = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    hh.ctx().pack_read(fmt, d, out, w, h, cm, lut, gm)
    return hh.host(out).view(np.uint32)


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_read_equals_the_yuv422p10_reader_on_the_equivalent_frame(fmt, size, lut_path):
    w, h = size
    planes = fmt10.random_frame(fmt, w, h, 1000 + w + (fmt == "p010"))
    if fmt == "yuv420p10":
        assert (np.concatenate(planes) > 1023).any()
    else:
        assert (np.concatenate(planes) & 0x3F).any()
    want = orc.pack_read("yuv422p10", fmt10.as_bytes(fmt10.to_422(fmt, planes, w, h)), w, h, *reader_o()).reshape(-1).view(np.uint32)
    got = read_ours(fmt, planes, w, h)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s read %dx%d (%s): %d of %d floats differ, first at pixel %d" % (fmt, w, h, lut_path, bad.size, got.size, bad[0] // 4)


@needs_ref
@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_read_equals_the_reference_yuv422p10_kernel_on_this_gpu(ref, fmt, size):
    ref_read(ref, fmt, size[0], size[1], 2000 + size[0])


def ref_read(ref, fmt, w, h, seed):
    import torch
    import hip_harness as hh
    planes = fmt10.random_frame(fmt, w, h, seed)
    cm, lut, gm = hh.ColourParams.fmt_reader(fmt, RSPEC, WSPEC)
    f422 = dev_planes(fmt10.to_422(fmt, planes, w, h))
    want = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
    wg = -(-fmt10.pitch(w) // 64)  # yuv422p10.ts:305-306
    torch.cuda.synchronize()
    ref.launch("yuv422p10", "read", wg * h, wg, f422 + [want, w, cm, lut, gm])
    got = read_ours(fmt, planes, w, h)
    b = want.cpu().numpy().view(np.uint32)
    assert np.count_nonzero(b) > b.size // 2, "the reference kernel did not run"
    assert np.array_equal(got, b), "%s read %dx%d: %d floats differ from the reference kernel's" % (fmt, w, h, int((got != b).sum()))


def write_both(fmt, w, h, fields, seed):
    """(ours, the oracle's) planes as uint8 after the write calls of `fields` (0: progressive; 1 then 3: both fields into one buffer)"""
    import hip_harness as hh
    rgba = frames.rgba_random(w, h, seed, -0.05, 1.05)
    cm, lut = hh.ColourParams.fmt_writer(fmt, WSPEC)
    d_rgba = hh.dev(rgba)
    got = [hh.dev(np.full(n, 0x5A, np.uint8)) for n in fmt10.plane_bytes(fmt, w, h)]
    p422 = None
    for il in fields:
        hh.ctx().pack_write(fmt, d_rgba, got, w, h, il, cm, lut)
        p422 = orc.pack_write("yuv422p10", rgba, w, h, il, *writer_o(), planes=p422)
    want = fmt10.as_bytes(fmt10.from_422_write(fmt, [p.view(np.uint16) for p in p422], w, h, fields[-1]))
    return [hh.host(g) for g in got], want, rgba


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fields", [(0,), (1, 3)], ids=["progressive", "both-fields"])
def test_write_equals_the_yuv422p10_writer_with_the_upper_line_chroma(fmt, size, fields, lut_path):
    w, h = size
    got, want, _ = write_both(fmt, w, h, fields, 300 + w + fields[0])
    for i, (a, b) in enumerate(zip(got, want)):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, "%s write %dx%d fields %s (%s) plane %d: %d of %d bytes differ, first at %d" % (fmt, w, h, fields, lut_path, i, bad.size, a.size, bad[0])


@needs_ref
@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("size", [(1920, 1080), (718, 480)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("fields", [(0,), (1, 3)], ids=["progressive", "both-fields"])
def test_write_equals_the_reference_yuv422p10_kernel_on_this_gpu(ref, fmt, size, fields):
    ref_write(ref, fmt, size[0], size[1], fields, 400 + size[0])


def ref_write(ref, fmt, w, h, fields, seed):
    import hip_harness as hh
    got, _, rgba = write_both(fmt, w, h, fields, seed)
    cm, lut = hh.ColourParams.fmt_writer(fmt, WSPEC)
    d_rgba = hh.dev(rgba)
    want = [hh.dev(np.full(n, 0x5A, np.uint8)) for n in frames.pack_plane_bytes("yuv422p10", w, h)]
    wg = -(-fmt10.pitch(w) // 64)  # yuv422p10.ts:337-338
    for il in fields:
        ref.launch("yuv422p10", "write", wg * h // (2 if il else 1), wg, [d_rgba] + want + [w, il, cm, lut])
    p422 = [hh.host(p).view(np.uint16) for p in want]
    assert all(np.count_nonzero(p != 0x5A5A) > p.size // (2 if fields in ((0,), (1, 3)) else 5) for p in p422), "the reference kernel did not run"  # (one field alone: half the lines)
    want = fmt10.as_bytes(fmt10.from_422_write(fmt, p422, w, h, fields[-1]))
    if fields in ((1,), (3,)):  # one field alone: the other field's luma lines keep the destination's bytes (from_422_write shifted the 4:2:2 poison)
        keep = np.setdiff1d(np.arange(h), fmt10.rows_written(h, fields[0]))
        want[0].reshape(h, -1)[keep] = 0x5A
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), "%s write plane %d: %d bytes differ from the reference kernel's" % (fmt, i, int((a != b).sum()))


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
def test_batch_read_equals_separate_reads(fmt):
    import torch
    import hip_harness as hh
    w, h = 1280, 720
    k = hh.ctx()
    cm, lut, gm = hh.ColourParams.fmt_reader(fmt, RSPEC, WSPEC)
    srcs = [dev_planes(fmt10.random_frame(fmt, w, h, 500 + i)) for i in range(8)]
    single = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda") for _ in range(8)]
    for i in range(8):
        k.pack_read(fmt, srcs[i], single[i], w, h, cm, lut, gm)
    want = [hh.host(s).view(np.uint32) for s in single]
    for n in range(1, 9):
        outs = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda") for _ in range(n)]
        k.pack_read_batch(fmt, srcs[:n], outs, w, h, cm, lut, gm)
        for i in range(n):
            assert np.array_equal(hh.host(outs[i]).view(np.uint32), want[i]), "%s batch of %d: frame %d differs" % (fmt, n, i)


# ---- the channel kernel and the clip route: F' -> transform -> combine -> v210_write -------------------------------------------------
def Clip(fmt, w, h, seed, matrix):
    """a source of any pack format on both sides (test_chan_gpu.Src over tests/packfmt.py)"""
    return chan.Src.random(fmt, w, h, seed, matrix)


def m(ow, oh, **kw):
    from phaneron_amd import capi
    return capi.transform_matrix(ow, oh, **kw)


def oracle_frame(clips, ow, oh):
    placed = [c.oracle(reader_o(), ow, oh) for c in clips]
    return np.asarray(orc.v210_write(placed[0] if len(placed) == 1 else orc.combine(placed), ow, oh, 0, *writer_o())).reshape(-1)


def colour_d():
    import hip_harness as hh
    return hh.ColourParams.reader(RSPEC, WSPEC) + hh.ColourParams.writer(WSPEC)


def compose(clips, ow, oh, dry=False):
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    out = torch.zeros(frames.v210_pitch_bytes(ow) * oh // 4, dtype=torch.int32, device="cuda")
    layers = [dict(src=c.device()) for c in clips]
    with capi.trace(dry_run=dry) as t:
        hh.ctx().chan_compose_v210(layers, out, ow, oh, 0, *colour_d())
    return (None if dry else hh.host(out, np.uint32)), t.route


def check_frame(clips, ow, oh, what):
    got, route = compose(clips, ow, oh)
    want = oracle_frame(clips, ow, oh)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s (%s): %d of %d words differ, first at line %d" % (what, route, bad.size, got.size, bad[0] // (frames.v210_pitch_bytes(ow) // 4))
    return route


EIGHT_BIT = {f: packfmt.get(f).sibling8 for f in fmt10.FORMATS}


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
@pytest.mark.parametrize("shape", [(1920, 1080), (1280, 720)], ids=["1080p-default-fill", "720p-filling-1080p"])
def test_one_clip_channel_equals_the_oracle_chain_and_takes_the_8bit_route(fmt, shape):
    ow, oh = 1920, 1080
    w, h = shape
    route = check_frame([Clip(fmt, w, h, 600 + w, m(ow, oh))], ow, oh, "%s %dx%d on 1080p" % (fmt, w, h))
    _, dry = compose([Clip(fmt, w, h, 600 + w, m(ow, oh))], ow, oh, dry=True)
    _, dry8 = compose([Clip(fmt, w, h, 600 + w, m(ow, oh)).like(EIGHT_BIT[fmt])], ow, oh, dry=True)
    assert dry == route and dry == dry8, (route, dry, dry8)


def test_config2_shape_with_both_formats_beside_v210_layers():
    """BASELINE config 2's placements: a full-frame layer and three quarter-size insets - v210, yuv420p10, p010, v210"""
    ow, oh = 1920, 1080
    pip = [dict(), dict(scale_x=0.5, scale_y=0.5, offset_x=-0.25, offset_y=-0.25), dict(scale_x=0.5, scale_y=0.5, offset_x=0.25, offset_y=-0.25),
           dict(scale_x=0.5, scale_y=0.5, offset_x=0.25, offset_y=0.25)]
    fmts = ["v210", "yuv420p10", "p010", "v210"]
    check_frame([Clip(f, ow, oh, 700 + i, m(ow, oh, **pip[i])) for i, f in enumerate(fmts)], ow, oh, "config 2 shape")


def test_four_channels_in_one_batch_launch():
    import torch
    import hip_harness as hh
    ow, oh = 1920, 1080
    jobs, want, outs = [], [], []
    shapes = [("yuv420p10", 1920, 1080), ("p010", 1280, 720), ("p010", 1920, 1080), ("yuv420p10", 1280, 720)]
    for j, (fmt, w, h) in enumerate(shapes):
        clips = [Clip(fmt, w, h, 800 + j, m(ow, oh)), Clip("v210", ow, oh, 810 + j, m(ow, oh, scale_x=0.5, scale_y=0.5, offset_x=0.25))]
        want.append(oracle_frame(clips, ow, oh))
        out = torch.zeros(frames.v210_pitch_bytes(ow) * oh // 4, dtype=torch.int32, device="cuda")
        outs.append(out)
        jobs.append(([dict(src=c.device()) for c in clips], out, 0))
    hh.ctx().chan_compose_batch(jobs, ow, oh, *colour_d())
    for j in range(4):
        got = hh.host(outs[j], np.uint32)
        assert np.array_equal(got, want[j]), "channel %d (%s): %d words differ" % (j, shapes[j][0], int((got != want[j]).sum()))


@pytest.mark.parametrize("fmt", fmt10.FORMATS)
def test_deinterlacing_reader_refuses_the_formats(fmt):
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 64, 16
    cm, lut, gm = hh.ColourParams.fmt_reader(fmt, RSPEC, WSPEC)
    frame = tuple(dev_planes(fmt10.random_frame(fmt, w, h, 9)))
    outs = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda") for _ in range(2)]
    with pytest.raises(capi.PhaneronError, match="error -1: .*run the separate kernels"):  # PH_E_INVALID
        hh.ctx().v210_yadif_pair([(frame, frame, frame, outs[0], outs[1])], w, h, True, False, cm, lut, gm, packing=fmt)


# ---- the edges: frames smaller than a work group, every tail shape, h % 4 == 2, single fields, other colour recipes ------------------
EDGE_WIDTHS = [2, 4, 6, 8, 10, 12, 14, 16, 64, 66, 70, 72, 74, 76, 78, 250, 256, 258, 1918, 1920]  # every w % 8, one octet, less than a wave, around 256-lane blocks
EDGE_HEIGHTS = [2, 4, 6, 10]  # (2, 6, 10: the last chroma line serves a line pair that starts on an even field line)
RECIPES = [("709", "2020"), ("2020", "709"), ("2020", "2020"), ("601-625", "709")]
FIELD_SEQUENCES = [(0,), (1,), (3,), (1, 3)]


@pytest.mark.parametrize("fmt", packfmt.PLANAR_10_420)
@pytest.mark.parametrize("w", EDGE_WIDTHS, ids=lambda w: "w%d" % w)
def test_read_at_the_edges(fmt, w, lut_path):
    """ph_pack_read of frames of 2 ... 1920 x 2 ... 10 pixels, words of all 16 bits, under four colour recipes (BT.2020 and 601 Loader
    matrices among them) = the oracle's yuv422p10 Reader on F', float for float"""
    import torch
    import hip_harness as hh
    f = packfmt.get(fmt)
    for h in EDGE_HEIGHTS:
        planes = f.random_planes(w, h, 1100 + 16 * w + h)
        d = [hh.dev(p) for p in planes]
        for rspec, wspec in RECIPES:
            out = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
            hh.ctx().pack_read(fmt, d, out, w, h, *hh.ColourParams.fmt_reader(fmt, rspec, wspec))
            got = hh.host(out).view(np.uint32)
            want = f.oracle_read(planes, w, h, *f.oracle_reader(rspec, wspec)).reshape(-1).view(np.uint32)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "%s read %dx%d %s -> %s (%s): %d of %d floats differ, first at pixel %d" % (fmt, w, h, rspec, wspec, lut_path, bad.size, got.size, bad[0] // 4)


def write_at_an_edge(fmt, w, h, fields, rgba, wspec, what):
    """the write calls of `fields` into planes full of 0xA5: the rows they write equal the definition, every other byte is still 0xA5"""
    import hip_harness as hh
    f = packfmt.get(fmt)
    want = f.poisoned(w, h)
    got = [hh.dev(p) for p in want]
    d_rgba = hh.dev(rgba)
    for il in fields:
        hh.ctx().pack_write(fmt, d_rgba, got, w, h, il, *hh.ColourParams.fmt_writer(fmt, wspec))
        want = f.oracle_write(rgba, w, h, il, *f.oracle_writer(wspec), want)
    got = [hh.host(g) for g in got]
    untouched = np.arange(h)
    for il in fields:
        untouched = np.intersect1d(untouched, f.rows_untouched(h, il))
    rows = got[0].reshape(h, -1)
    assert (rows[untouched] == packfmt.POISON).all(), "%s: luma rows %s of the other field were written" % (what, untouched[(rows[untouched] != packfmt.POISON).any(axis=1)])
    for i, (a, b) in enumerate(zip(got, want)):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, "%s plane %d: %d of %d bytes differ, first at %d (row %d)" % (what, i, bad.size, a.size, bad[0], bad[0] // (a.size // (h if i == 0 else h // 2)))


@pytest.mark.parametrize("fmt", packfmt.PLANAR_10_420)
@pytest.mark.parametrize("w", EDGE_WIDTHS, ids=lambda w: "w%d" % w)
def test_write_at_the_edges(fmt, w, lut_path):
    """ph_pack_write at the same sizes: whole frames, field 1 alone, field 3 alone (what an interlaced channel writes per tick: chroma row g
    from line 2g, or 2g + 1), field 1 then 3 - random input beyond [0, 1] and NaN / +-Inf / -0 / denormals / huge values / LUT-index ties;
    the three tail shapes of the last octet (remain 2, 4, 6, with the 4:2:2 writers' overwritten slot 1) on h % 4 == 2 frames too"""
    for h in EDGE_HEIGHTS:
        inputs = [("random", frames.rgba_random(w, h, 1200 + 16 * w + h, -0.1, 1.1)), ("specials", frames.rgba_specials(w, h, 1300 + 16 * w + h))]
        for name, rgba in inputs:
            for fields in FIELD_SEQUENCES:
                write_at_an_edge(fmt, w, h, fields, rgba, "2020" if name == "random" else "709",
                                 "%s write %dx%d fields %s, %s input (%s)" % (fmt, w, h, fields, name, lut_path))


@pytest.mark.parametrize("fmt", packfmt.PLANAR_10_420)
@pytest.mark.parametrize("size", [(1920, 1080), (718, 480)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("il", [1, 3])
def test_one_field_alone_at_full_size(fmt, size, il):
    """what an interlaced channel writes per tick, at real sizes: one field into poisoned planes, the other field's lines untouched"""
    w, h = size
    write_at_an_edge(fmt, w, h, (il,), frames.rgba_random(w, h, 1400 + w + il, -0.05, 1.05), "2020", "%s write %dx%d field %d alone" % (fmt, w, h, il))


@pytest.mark.parametrize("fmt", packfmt.PLANAR_10_420)
@pytest.mark.parametrize("size", [(74, 6), (258, 10)], ids=lambda s: "%dx%d" % s)
def test_batch_read_of_small_ragged_frames_equals_separate_reads(fmt, size):
    import torch
    import hip_harness as hh
    w, h = size
    k, f = hh.ctx(), packfmt.get(fmt)
    recipe = hh.ColourParams.fmt_reader(fmt, "2020", "709")
    planes = [f.random_planes(w, h, 1500 + w + i) for i in range(8)]
    srcs = [[hh.dev(p) for p in ps] for ps in planes]
    want = [f.oracle_read(ps, w, h, *f.oracle_reader("2020", "709")).reshape(-1).view(np.uint32) for ps in planes]
    for i in range(8):
        single = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda")
        k.pack_read(fmt, srcs[i], single, w, h, *recipe)
        assert np.array_equal(hh.host(single).view(np.uint32), want[i]), "%s %dx%d: frame %d read alone differs from the oracle" % (fmt, w, h, i)
    for n in range(1, 9):
        outs = [torch.zeros(w * h * 4, dtype=torch.float32, device="cuda") for _ in range(n)]
        k.pack_read_batch(fmt, srcs[:n], outs, w, h, *recipe)
        for i in range(n):
            assert np.array_equal(hh.host(outs[i]).view(np.uint32), want[i]), "%s %dx%d batch of %d: frame %d differs" % (fmt, w, h, n, i)


REF_SIZES = [(14, 2), (74, 6), (250, 6), (258, 10)]  # one to five work items per line, last octets of 6 and 2 pixels (76 x 4 below: of 4)


@needs_ref
@pytest.mark.parametrize("fmt", packfmt.PLANAR_10_420)
@pytest.mark.parametrize("size", REF_SIZES + [(76, 4)], ids=lambda s: "%dx%d" % s)
def test_small_ragged_frames_equal_the_reference_yuv422p10_kernels_on_this_gpu(ref, fmt, size):
    """the reference's own read / write kernels on F' at small ragged sizes (one work group of ceil(pitch / 64) items per line, as its
    Reader / Writer classes launch them): reads, whole-frame writes, each field alone and both"""
    w, h = size
    ref_read(ref, fmt, w, h, 2100 + w)
    for fields in FIELD_SEQUENCES:
        ref_write(ref, fmt, w, h, fields, 2200 + w + fields[0])


@pytest.mark.parametrize("fmt", packfmt.names(even_size=True))
def test_odd_frames_are_refused_on_the_device_entry_points(fmt):
    """ph_pack_read, ph_pack_read_batch and ph_pack_write refuse odd widths and heights (PH_E_INVALID, "even width and height") and
    leave their outputs alone"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    k, f = hh.ctx(), packfmt.get(fmt)
    w, h = 64, 16
    planes = [hh.dev(p) for p in f.random_planes(w, h, 5)]
    rgba = hh.dev(frames.rgba_random(w, h, 6))
    rd, wr = hh.ColourParams.fmt_reader(fmt, "709", "709"), hh.ColourParams.fmt_writer(fmt, "709")
    for ww, hh_ in ((w - 1, h), (w, h - 1), (w - 1, h - 1)):
        out = [torch.full((w * h * 4,), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
        dst = [hh.dev(p) for p in f.poisoned(w, h)]
        with pytest.raises(capi.PhaneronError, match="error -1: ph_pack_read: .*%s.*even width and height" % fmt):
            k.pack_read(fmt, planes, out[0], ww, hh_, *rd)
        with pytest.raises(capi.PhaneronError, match="error -1: ph_pack_read_batch: .*%s.*even width and height" % fmt):
            k.pack_read_batch(fmt, [planes, planes], out, ww, hh_, *rd)
        with pytest.raises(capi.PhaneronError, match="error -1: ph_pack_write: .*%s.*even width and height" % fmt):
            k.pack_write(fmt, rgba, dst, ww, hh_, 0, *wr)
        assert all((hh.host(o) == 7.0).all() for o in out) and all((hh.host(p) == packfmt.POISON).all() for p in dst)
