"""GPU tests (-m gpu) of the f32 images' STREAMED store path and of the decision that selects it.

Every kernel that writes an f32 RGBA image has two store arms (ph_device.h store_image): a plain store, the default, and a nontemporal
one taken when the launch's `nt` argument is 1.  `nt` is ph::image_nt(bytes) of the context options "stream_images" (0 cached, 1
streamed, 2 by size) and "stream_threshold_mb", which set_device copies into thread-locals in front of each launch.

1. The guarded, bit-exact cases of tests/test_guard_gpu.py (its `gb` fixture and its test bodies, called, not copied) and the
   ph_fused_v210_route_multi cases of tests/test_fused_route_gpu.py (its `check`) run with the streamed arm selected, under both
   policies that select it: "stream_images" = 1, and "stream_images" = 2 with "stream_threshold_mb" = 0 (every image of a byte or more
   streams).  The wire-format outputs those bodies also compare always stream and stay as they are.  The packed-RGB outputs of the
   de-interlacing reader are stored plainly under every policy (ph_kernels_deint.hip); the body's RGBA cases take the streamed arm.
2. Bits cannot tell which arm ran, so ph_debug_image_nt(ctx, bytes) answers what a launch issued next on the calling thread for that
   context would be given.  The fixtures below ask it before and after every body; the tests at the end pin the decision itself: the
   strict comparison, the shift in size_t, refusals, two contexts on one thread and on two."""
import contextlib
import re
import threading

import numpy as np
import pytest

import frames
import guard
import packfmt
import test_fused_route_gpu as tr
import test_guard_gpu as tg
from oracle import orc
from test_chan_multi_gpu import oracle_frame, out, writer
from test_fused_multi_gpu import layer_words
from test_guard_gpu import gb  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

DEFAULT = (0, 64)
POLICIES = [(1, 64), (2, 0)]  # ("stream_images", "stream_threshold_mb"): both select the streamed arm for every image
IDS = ["streamed", "by-size-0"]


@contextlib.contextmanager
def store_policy(k, images, mb):
    """the policy on context k for the body, the library's defaults after it - also when the body fails: the context is the session's"""
    try:
        k.set_option("stream_threshold_mb", mb)
        k.set_option("stream_images", images)
        assert k.debug_image_nt(16) == 1, "one pixel must stream under %r" % ((images, mb),)
        yield
        assert k.debug_image_nt(16) == 1, "the body changed the store policy"
    finally:
        k.set_option("stream_images", DEFAULT[0])
        k.set_option("stream_threshold_mb", DEFAULT[1])
    assert k.debug_image_nt(16) == 0 and k.debug_image_nt(1 << 33) == 0


@pytest.fixture(params=POLICIES, ids=IDS)
def streamed(request, gb):  # noqa: F811
    """test_guard_gpu's session with the streamed arm selected on the real context (the session hands every call on to it); its
    finish() is counted, for run()"""
    gb.tallies, finish = [], gb.finish

    def counted():
        gb.tallies.append(finish())
        return gb.tallies[-1]
    gb.finish = counted
    with store_policy(gb, *request.param):
        yield gb


def run(body, gb, *args):  # noqa: F811
    """a body of test_guard_gpu, which must reach its own gb.finish() tally"""
    body(gb, *args)
    assert len(gb.tallies) == 1 and gb.tallies[0][1] > 0, "the body did not reach its tally"


@pytest.fixture(params=POLICIES, ids=IDS)
def policy(request):
    import hip_harness as hh
    with store_policy(hh.ctx(), *request.param):
        yield request.param


# ---- 1a. the guarded bodies ----------------------------------------------------------------------------------------------------------
def test_yadif_and_yadif_pair_streamed(streamed):
    run(tg.test_yadif_and_yadif_pair, streamed)


def test_transform_and_resize_streamed(streamed):
    run(tg.test_transform_and_resize, streamed)


def test_combine_transitions_mixer_and_wipe_streamed(streamed):
    run(tg.test_combine_transitions_mixer_and_wipe, streamed)


def test_v210_read_batch_and_write_streamed(streamed):
    run(tg.test_v210_read_batch_and_write, streamed)


@pytest.mark.parametrize("fmt", packfmt.STANDALONE)
def test_pack_formats_streamed(streamed, fmt):
    run(tg.test_pack_formats_between_guards, streamed, fmt)


@pytest.mark.parametrize("fmt", packfmt.names(deint=True))
def test_deinterlacing_reader_streamed(streamed, fmt):
    """both output forms (the body alternates RGBA and packed RGB), 1 and 3 sources, tff 0 and 1, widths on both sides of one and two
    58-column strips; the RGBA form takes the streamed arm, the packed-RGB form has none"""
    run(tg.test_deinterlacing_reader_between_guards, streamed, fmt)


def test_compose_up_write_v210_pair_and_batch_streamed(streamed):
    run(tg.test_compose_up_write_v210_pair_and_batch, streamed)


# ---- 1b. ph_fused_v210_route_multi: image_out stored with karg->nt -------------------------------------------------------------------
def guarded(w, h):
    """test_fused_route_gpu.check's dst / src makers, every buffer between guards (as its guard-band case makes them)"""
    def dst(p, fmt):
        return guard.dev(p, "dst", pitch=w * 16 if fmt == "image" else max(1, p.size // h))

    def src(a, fmt):
        return guard.dev(a, "src", pitch=frames.v210_pitch_bytes(w) if fmt == "v210" else w * 16, fill="codes" if fmt == "v210" else "float")
    return dict(dst=dst, src=src, chan=False, gpu_chain=False)


def n_planes(outs, w, h):
    return sum(len(frames.pack_plane_bytes(o["fmt"], w, h)) for o in outs)


def route_cases(w, h, cases, what):
    """[(layer specs, outputs)] through tr.check with image_out, between guards; the tally is the cases' own"""
    guard.reset()
    try:
        n_src = n_dst = 0
        for specs, outs in cases:
            tr.check(w, h, specs, outs, "%s: %d layers, %d outputs" % (what, len(specs), len(outs)), route=tr.ROUTE % (len(outs), 1), **guarded(w, h))
            n_src, n_dst = n_src + len(specs), n_dst + 1 + n_planes(outs, w, h)
        assert guard.check() == (n_src, n_dst)
    finally:
        guard.reset()


@pytest.mark.parametrize("w,h", [(48, 2), (384, 6)])
def test_route_image_out_streamed(policy, w, h):
    """48 x 2 is less than one wave (48 of its 64 lanes are tail lanes); v210 layers only; an image layer in the middle with two
    outputs; no output at all, with and without an image layer"""
    V = tr.V
    route_cases(w, h, [([V, V, V], [out("v210"), out("yuv422p8")]),
                       ([V, tr.specials_image(w, h), V], [out("v210"), out("rgba8")]),
                       ([V, tr.seeded_image(w, h), V], []),
                       ([V, V], [])], "%dx%d under %r" % (w, h, policy))


@pytest.mark.parametrize("w,h", [(48, 2), (384, 6)])
def test_route_guard_band_case_streamed(policy, w, h):
    tr.test_between_guard_bands(w, h)


def test_route_tail_lanes_streamed(policy):
    """1920 x 8 in one workgroup: several slices a lane, the last partly filled per wave - the `own` predicate guards the streamed store"""
    import hip_harness as hh
    w, h = 1920, 8
    k = hh.ctx()
    k.set_option("fused_multi_wgs", 1)
    try:
        route_cases(w, h, [([tr.V, tr.seeded_image(w, h), tr.V, tr.specials_image(w, h)], tr.FOUR), ([tr.V, tr.V], tr.FOUR)], "1920x8 in one workgroup under %r" % (policy,))
    finally:
        k.set_option("fused_multi_wgs", 0)


def test_by_name_reader_then_route_streamed():
    """ph_run_programs on a context of its own under policy 1: a v210_read job writes the route job's image layer, fused_v210_route_2
    writes imageOut - each launch made from inside the program runner - against the oracle's read, combine and writers"""
    w, h = 384, 6
    b = tr.ByName(w, h)
    capi = b.capi
    try:
        b.ctx.set_option("stream_images", 1)
        assert b.ctx.debug_image_nt(w * h * 16) == 1
        words = layer_words(w, h, 2)
        params, outs, image_out = tr.route_params(b, words[0], tr.poison_image(w, h))
        wipg = frames.v210_pitch_pixels(w) // 48
        rd = b.ctx.create_program("phaneron:v210", "read", wipg * h, wipg)
        route = b.ctx.create_program("phaneron:fused", "fused_v210_route_2", [w, h])
        loader = {k_: b.recipe[k_] for k_ in ("colMatrix", "gammaLut", "gamutMatrix")}
        jobs = [(rd, dict(loader, input=b.upload(words[1], svm="coarse"), output=params["l1In"], width=w)), (route, params)]
        b.ctx.wait(capi.QUEUE_LOAD)
        with capi.trace() as t:
            b.ctx.run_programs(jobs)
        b.ctx.wait()
        assert len(t.kernels) == 2 and "v210_read" in t.kernels[0] and t.kernels[1] == tr.ROUTE % (2, 1), t.route
        assert b.ctx.debug_image_nt(w * h * 16) == 1
        imgs = [orc.v210_read(x, w, h, *b.rd_o) for x in words]
        comp = np.asarray(orc.combine(imgs))
        tr.same_image(b.read(params["l1In"]).view(np.float32), imgs[1], "the reader job's image against the oracle's read")
        tr.same_image(b.read(image_out).view(np.float32), comp, "imageOut against the oracle's combine")
        for i, fmt in enumerate(("v210", "yuv422p8")):
            rc = writer(fmt, "709")
            for pl, (p, want) in enumerate(zip(outs[i], oracle_frame(fmt, comp, w, h, 0, rc[0], rc[1]))):
                assert np.array_equal(b.read(p), np.asarray(want).reshape(-1).view(np.uint8)), "output %d (%s) plane %d differs from the oracle's" % (i, fmt, pl)
        rd.destroy(), route.destroy()
    finally:
        b.close()


# ---- 2. the decision -----------------------------------------------------------------------------------------------------------------
MIB = 1 << 20
REFUSALS = [("stream_images", -1, "stream_images: 0 (cached), 1 (streamed) or 2 (by size)"), ("stream_images", 3, "stream_images: 0 (cached), 1 (streamed) or 2 (by size)"),
            ("stream_threshold_mb", -1, "stream_threshold_mb: a size in MiB")]


@pytest.fixture
def k():
    """the session's context, at the library's defaults before and after"""
    import hip_harness as hh
    c = hh.ctx()
    assert c.debug_image_nt(1 << 33) == 0, "a test before this one leaked a store policy"
    try:
        yield c
    finally:
        c.set_option("stream_images", DEFAULT[0])
        c.set_option("stream_threshold_mb", DEFAULT[1])


def test_policies_0_and_1_answer_for_every_size(k):
    for images in (0, 1):
        k.set_option("stream_images", images)
        for mb in (64, 0):  # the threshold has no say
            k.set_option("stream_threshold_mb", mb)
            assert [k.debug_image_nt(n) for n in (0, 1, 1 << 33)] == [images] * 3, (images, mb)


@pytest.mark.parametrize("mb", [0, 1, 64])
def test_policy_2_compares_strictly(k, mb):
    k.set_option("stream_images", 2)
    k.set_option("stream_threshold_mb", mb)
    assert k.debug_image_nt(mb * MIB) == 0, "an image of exactly the threshold does not stream"
    assert k.debug_image_nt(mb * MIB + 1) == 1
    assert k.debug_image_nt(0) == 0
    if mb:
        assert k.debug_image_nt(mb * MIB - 1) == 0 and k.debug_image_nt(1) == 0
    assert k.debug_image_nt(1 << 33) == 1


def test_policy_2_shifts_in_size_t(k):
    """2047 MiB is the largest threshold whose byte count fits 31 bits; 4096 MiB is 2^32 bytes, which a 32-bit shift would turn into 0"""
    k.set_option("stream_images", 2)
    for mb in (2047, 4096):
        k.set_option("stream_threshold_mb", mb)
        assert [k.debug_image_nt(n) for n in (1, mb * MIB - 1, mb * MIB, mb * MIB + 1, 1 << 33)] == [0, 0, 0, 1, 1], mb


def test_refusals_leave_the_policy_in_force(k):
    from phaneron_amd import capi
    for images, mb, sizes, want in ((2, 1, (MIB, MIB + 1), [0, 1]), (1, 64, (0, 1), [1, 1])):
        k.set_option("stream_images", images)
        k.set_option("stream_threshold_mb", mb)
        for name, value, text in REFUSALS:
            with pytest.raises(capi.PhaneronError, match=re.escape(text) + "$"):
                k.set_option(name, value)
            assert [k.debug_image_nt(n) for n in sizes] == want, (images, mb, name, value)


def test_two_contexts_keep_their_own_policy():
    """a second context on the same device with the other policy: interleaved on one thread, after a launch on the first, and from a
    second thread - the thread-locals are per thread and refreshed per call"""
    import hip_harness as hh
    from phaneron_amd import capi
    a = hh.ctx()
    assert a.debug_image_nt(16) == 0
    b = capi.Context(0)
    try:
        n = 6 * 1 * 16
        for pa, pb in ((1, 0), (0, 1)):
            a.set_option("stream_images", pa)
            b.set_option("stream_images", pb)
            assert [c.debug_image_nt(n) for c in (a, b, b, a, b, a, a, b)] == [pa, pb, pb, pa, pb, pa, pa, pb]
            # a launch on A sets this thread's values to A's; the next query for B refreshes them
            cm, lut, gm = hh.ColourParams.reader("709", "2020")
            words = frames.v210_random(6, 1, 6200 + pa)
            img = hh.dev(tr.poison_image(6, 1))
            a.v210_read(hh.dev(words), img, 6, 1, cm, lut, gm)
            assert b.debug_image_nt(n) == pb and a.debug_image_nt(n) == pa
            want = orc.v210_read(words, 6, 1, orc.ycbcr2rgb_matrix("709"), orc.gamma2linear_lut("709"), orc.rgb2rgb_matrix("709", "2020"))
            tg.bits_eq(hh.host(img), want, "6x1 v210_read under policy %d" % pa)
            # a second thread asks for B while this thread last used A, then for A; this thread's next answers are unchanged
            assert a.debug_image_nt(n) == pa
            seen = []
            t = threading.Thread(target=lambda: seen.extend([b.debug_image_nt(n), a.debug_image_nt(n), b.debug_image_nt(n)]))
            t.start()
            t.join()
            assert seen == [pb, pa, pb]
            assert a.debug_image_nt(n) == pa and b.debug_image_nt(n) == pb
        # by size, a threshold each
        a.set_option("stream_images", 2), b.set_option("stream_images", 2)
        a.set_option("stream_threshold_mb", 1), b.set_option("stream_threshold_mb", 0)
        assert [c.debug_image_nt(s) for c, s in ((a, MIB), (b, MIB), (a, 1), (b, 1), (a, MIB + 1), (b, 0))] == [0, 1, 0, 1, 1, 0]
    finally:
        b.close()
        a.set_option("stream_images", DEFAULT[0])
        a.set_option("stream_threshold_mb", DEFAULT[1])
    assert a.debug_image_nt(1 << 33) == 0
