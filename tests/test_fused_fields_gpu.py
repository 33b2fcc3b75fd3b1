"""GPU tests (-m gpu) of the context option "fused_fields": ph_fused_v210_combine_multi and ph_fused_v210_combine_multi_batch compose only
the field where every output takes the same one ("fused_v210_field_multi ..." in a trace).  The option changes the route and nothing
else, so the checks are test_fused_multi_gpu's and test_fused_multi_batch_gpu's own: every plane of every output byte for byte, on
planes poisoned with 0x5A - the lines of the other parity and an odd height's last line must still be poison, which the oracle's field
write on poisoned planes asks for - against the oracle's chain and against separate ph_chan_compose calls."""
import contextlib
import re

import numpy as np
import pytest

import frames
import guard
import luts
from oracle import orc
from test_chan_multi_gpu import ALL_OUT, POISON, oracle_frame, out, poisoned, writer
from test_fused_multi_batch_gpu import check as batch_check
from test_fused_multi_gpu import SHARED, by_name, chan_layers, check, layer_words, reader, three_outputs  # noqa: F401 (by_name: a fixture)

pytestmark = pytest.mark.gpu

FIELD = "fused_v210_field_multi x%df%d"
FIELD_BATCH = "fused_v210_field_multi x%dj%df%d"


@contextlib.contextmanager
def fields(ctx=None, **more):
    """the option on for the block, with other options beside it, all put back"""
    import hip_harness as hh
    k = ctx or hh.ctx()
    k.set_option("fused_fields", 1)
    try:
        for name, value in more.items():
            k.set_option(name, value)
        yield k
    finally:
        for name in more:
            k.set_option(name, 1 if name == "lds_lut" else 0)
        k.set_option("fused_fields", 0)


def field_route(n_out, il):
    return re.escape(FIELD % (n_out, il))


# ---- formats ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 8])
@pytest.mark.parametrize("fmt", ALL_OUT)
def test_every_format_alone_and_beside_v210_in_both_fields(fmt, n):
    """a lone v210 field - SDI's call at 1080i - included"""
    w, h = 384, 12
    with fields():
        check(w, h, n, [out(fmt, 1)], "%s field 1 alone, %d layers" % (fmt, n), route=field_route(1, 1))
        check(w, h, n, [out("v210", 3), out(fmt, 3)], "v210 + %s, field 3, %d layers" % (fmt, n), route=field_route(2, 3))


def test_two_writer_tables_in_one_launch():
    tab = luts.layout_table(32, 8, 0xF00D)
    with luts.register(tab) as dtab, fields():
        outs = [out("v210", 1), out("yuv422p8", 1, spec=(tab, dtab)), out("rgba8", 1), out("nv12", 1, spec=(tab, dtab))]
        _, got = check(384, 12, 3, outs, "two tables, outputs interleaved, field 1", route=field_route(4, 1))
        _, same = check(384, 12, 3, [out("yuv422p8", 1)], "the same output from the shared table", separate=False)
        assert not np.array_equal(got[1][0], same[0][0]), "the table of other contents does not show in its output"


# ---- lines --------------------------------------------------------------------------------------------------------------------------
def test_field_3_of_an_odd_height():
    """96 x 9: lines 1, 3, 5 and 7 are written; 0, 2, 4, 6 and 8 are still poison"""
    w, h = 96, 9
    with fields():
        _, got = check(w, h, 3, [out("v210", 3), out("bgra8", 3), out("yuv422p8", 3)], "96x9 field 3", route=field_route(3, 3))
    for planes in got:
        for p in planes:
            rows = p.reshape(h, -1)
            assert (rows[0::2] == POISON).all(), "an even line was written"
            assert all(not (rows[y] == POISON).all() for y in (1, 3, 5, 7)), "an odd line was not written"


@pytest.mark.parametrize("il", [1, 3])
def test_420_fields_take_the_chroma_of_the_written_line(il):
    w, h = 384, 10
    with fields():
        _, got = check(w, h, 3, [out("yuv420p", il), out("nv12", il)], "384x10 4:2:0 field %d" % il, route=field_route(2, il))
    luma = got[0][0].reshape(h, w)
    other = luma[1::2] if il == 1 else luma[0::2]
    assert (other == POISON).all() and not (got[0][1] == POISON).all() and not (got[1][1] == POISON).all()


# ---- geometry -----------------------------------------------------------------------------------------------------------------------
def test_default_workgroups_begin_in_mid_line():
    """1920 x 16: the field is 2560 quads - three workgroups of 854, ranges that begin and end in mid-line - with 4:2:0 outputs"""
    with fields():
        check(1920, 16, 2, [out("nv12", 1), out("yuv420p", 1), out("v210", 1)], "1920x16 field 1, default workgroups", route=field_route(3, 1))
        check(1920, 16, 2, [out("v210", 3), out("nv12", 3)], "1920x16 field 3, default workgroups", route=field_route(2, 3))


@pytest.mark.parametrize("w,h,wgs,why", [(384, 96, 1, "the field is three full slices a lane"), (768, 100, 1, "the field is 6400 quads: a second tile of 256"),
                                         (96, 66, 2, "ranges of 264 field quads: a partly filled wave")])
@pytest.mark.parametrize("il", [1, 3])
def test_capped_workgroups(w, h, wgs, why, il):
    with fields(fused_multi_wgs=wgs):
        outs = [out("v210", il), out("nv12", il), out("yuv422p8", il), out("bgra8", il)]
        check(w, h, 2, outs, "%dx%d field %d, %d workgroups (%s)" % (w, h, il, wgs, why), route=field_route(4, il), separate=False)


# ---- what the option leaves alone ---------------------------------------------------------------------------------------------------
def test_mixed_field_modes_keep_the_whole_frame_launch():
    with fields():
        check(384, 12, 2, [out("v210", 1), out("rgba8", 0)], "a field beside a frame", route=re.escape(SHARED % 2))
        check(384, 12, 2, [out("v210", 1), out("bgra8", 3)], "field 1 beside field 3", route=re.escape(SHARED % 2))


def test_one_v210_frame_is_still_the_headline_kernel():
    with fields():
        check(384, 12, 2, [out("v210")], "one v210 frame", route="fused_v210_combine_lds")


def test_another_width_still_takes_the_channel_kernels_route():
    with fields():
        check(1280, 6, 2, [out("v210", 1), out("yuv422p8", 1), out("nv12", 1)], "1280x6 field 1", route=r"chan_compose_multi<\d>x3")


def test_without_lds_tables_the_answer_is_still_ph_chan_compose_multis():
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 12
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, 2)]
    outputs = [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=1, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in ("v210", "rgba8")]
    with fields(lds_lut=0) as k:
        texts = []
        for call in (lambda: k.fused_v210_combine_multi(dl, outputs, w, h, *rd_d), lambda: k.chan_compose_multi(chan_layers(dl, w, h), outputs, w, h, *rd_d)):
            with capi.trace() as t:
                with pytest.raises(capi.PhaneronError, match=r"error -1: .*reader gamma LUT has no LDS form") as e:
                    call()
            texts.append((t.route, str(e.value)))
        assert texts[0] == texts[1] and "field" not in texts[0][0], texts
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"])


def test_with_the_option_off_the_names_and_the_bytes_are_todays():
    w, h = 384, 12
    first = [out("v210", 1)]  # (test_every_format_alone_and_beside_v210_in_both_fields' first case)
    with fields():
        _, on = check(w, h, 1, first, "option 1", route=field_route(1, 1), separate=False)
    _, off = check(w, h, 1, first, "option 0", route=re.escape(SHARED % 1), separate=False)
    assert all(np.array_equal(a, b) for x, y in zip(on, off) for a, b in zip(x, y)), "the option changed the bytes"
    check(w, h, 4, [out("v210", 3), out("nv12", 3)], "option 0, two field 3 outputs", route=re.escape(SHARED % 2), separate=False)


def test_a_frame_of_one_line_launches_nothing():
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 1
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, 2)]
    outputs = [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=1, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in ("v210", "rgba8")]
    with fields() as k:
        with capi.trace() as t:
            k.fused_v210_combine_multi(dl, outputs, w, h, *rd_d)  # PH_OK: the binding raises on anything else
        k.wait()
    assert t.route == "", t.route
    assert all((hh.host(p, np.uint8) == POISON).all() for o in outputs for p in o["planes"])


def test_the_option_takes_0_or_1():
    import hip_harness as hh
    from phaneron_amd import capi
    with pytest.raises(capi.PhaneronError, match=r"error -1: .*fused_fields"):
        hh.ctx().set_option("fused_fields", 2)


# ---- batch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(384, 12), (1920, 16)])
@pytest.mark.parametrize("jobs", [2, 5])
def test_batch(jobs, w, h):
    """every job has layers of its own (a seed per job): a job that reads another's layers or writes another's planes shows; each job's
    bytes are the oracle's and its single call's"""
    with fields():
        _, _, alone = batch_check(w, h, 2, jobs, [out("v210", 1), out("nv12", 1)], "%dx%d, %d jobs, field 1" % (w, h, jobs), route=FIELD_BATCH % (2, jobs, 1))
    assert alone.split("+") == [FIELD % (2, 1)] * jobs, alone


def test_batch_field_3_with_capped_workgroups():
    with fields(fused_multi_wgs=2):
        batch_check(96, 66, 3, 3, [out("v210", 3), out("yuv420p", 3), out("rgba8", 3)], "96x66, 3 jobs, field 3, 2 workgroups each", route=FIELD_BATCH % (3, 3, 3),
                    separate=False)


# ---- by name: fused_v210_combine_multi_<n> ------------------------------------------------------------------------------------------
def field_1_job(b, words):
    """a fused_v210_combine_multi_2 job for v210, yuv422p8 and rgba8, all field 1: (params, the outputs' buffers, the oracle's planes)"""
    params, outs = three_outputs(b, [b.upload(l, svm="coarse") for l in words])
    params.update(interlace=1, interlace1=1, interlace2=1)
    comp = orc.combine([orc.v210_read(l, b.w, b.h, *b.rd_o) for l in words])
    wlut = orc.linear2gamma_lut("709")
    want = [oracle_frame("v210", comp, b.w, b.h, 1, orc.rgb2ycbcr_matrix("709"), wlut),
            oracle_frame("yuv422p8", comp, b.w, b.h, 1, orc.rgb2ycbcr_matrix("709", *orc.FORMAT_RANGE["yuv422p8"]), wlut),
            oracle_frame("rgba8", comp, b.w, b.h, 1, None, wlut)]
    return params, outs, want


def expect(b, outs, want, what):
    for i, (planes, wnt) in enumerate(zip(outs, want)):
        for pl, (p, x) in enumerate(zip(planes, wnt)):
            assert np.array_equal(b.read(p), x), "%s: output %d plane %d" % (what, i, pl)


def test_by_name_run_program(by_name):
    b = by_name
    params, outs, want = field_1_job(b, layer_words(b.w, b.h, 2))
    b.ctx.wait(b.capi.QUEUE_LOAD)
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [b.w, b.h])
    with fields(b.ctx):
        b.ctx.run_program(prog, params, check_only=True)
        for planes in outs:
            for p in planes:
                assert (b.read(p) == POISON).all(), "a check wrote"
        with b.capi.trace() as t:
            b.ctx.run_program(prog, params)
        b.ctx.wait()
    assert t.route == FIELD % (3, 1), t.route
    expect(b, outs, want, "by name")
    prog.destroy()


def test_by_name_two_jobs_share_a_field_launch(by_name):
    b = by_name
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [b.w, b.h])
    made = [field_1_job(b, layer_words(b.w, b.h, 2, seed=60 + j)) for j in range(2)]
    b.ctx.wait(b.capi.QUEUE_LOAD)
    with fields(b.ctx, fused_multi_batch=1):
        with b.capi.trace() as t:
            b.ctx.run_programs([(prog, params) for params, _, _ in made])
        b.ctx.wait()
    assert t.route == FIELD_BATCH % (3, 2, 1), t.route
    for j, (_, outs, want) in enumerate(made):
        expect(b, outs, want, "job %d" % j)
    prog.destroy()


# ---- guard bands --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(384, 12), (1920, 16)])
def test_between_guard_bands(w, h):
    """test_fused_multi_gpu.test_between_guard_bands' two output lists with every output taking field 1, then field 3"""
    guard.reset()
    try:
        def dst(p, fmt):
            return guard.dev(p, "dst", pitch=max(1, p.size // h))

        def src(l):
            return guard.dev(l, "src", pitch=frames.v210_pitch_bytes(w))
        with fields():
            for il in (1, 3):
                check(w, h, 3, [out("v210", il), out("yuv422p10", il), out("yuv422p8", il), out("rgba8", il)], "%dx%d field %d between guards" % (w, h, il),
                      route=field_route(4, il), separate=False, dst=dst, src=src)
                check(w, h, 3, [out("yuv420p", il), out("nv12", il), out("bgra8", il), out("v210", il)], "%dx%d field %d between guards" % (w, h, il),
                      route=field_route(4, il), separate=False, dst=dst, src=src)
        assert guard.check() == (12, 30)
    finally:
        guard.reset()


# ---- seeded campaign ----------------------------------------------------------------------------------------------------------------
def test_random_outputs_of_random_frames():
    """32 seeded cases: 1..8 layers, a width of 48 / 96 / 384 / 768, a height of 2..13 (even wherever a 4:2:0 output is drawn, so the
    generator never discards a case), 1..4 outputs of random formats and writer tables with ONE field mode per case"""
    r = np.random.default_rng(20261021)
    with fields():
        for case in range(32):
            n = int(r.integers(1, 9))
            w = int(r.choice([48, 96, 384, 768]))
            il = int(r.choice([1, 3]))
            outs = [out(str(r.choice(ALL_OUT)), il, spec=str(r.choice(["709", "709", "2020"]))) for _ in range(int(r.integers(1, 5)))]
            h = int(r.integers(2, 14))
            if any(o["fmt"] in ("yuv420p", "nv12") for o in outs):
                h += h & 1
            check(w, h, n, outs, "case %d: %dx%d, %d layers, field %d, outputs %r" % (case, w, h, n, il, [(o["fmt"], o["spec"]) for o in outs]), seed=200 + case,
                  route=field_route(len(outs), il), separate=case % 4 == 0)


# ---- full size ----------------------------------------------------------------------------------------------------------------------
def test_full_size_equals_the_channel_kernels_bytes():
    """1920 x 1080, 4 layers, v210 + yuv422p8, both field 1, against ph_chan_compose_multi's bytes"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    from test_fused_multi_gpu import _layers
    w, h = 1920, 1080
    _, rd_d = reader()
    dl = [hh.dev(l) for l in layer_words(w, h, 4, seed=31)]
    fmts = ("v210", "yuv422p8")

    def outputs():
        return [dict(fmt=f, planes=[hh.dev(p) for p in poisoned(f, w, h)], interlace=1, wr_cm=writer(f, "709")[2], wr_lut=writer(f, "709")[3]) for f in fmts]
    mine, theirs = outputs(), outputs()
    with fields() as k:
        with capi.trace() as t:
            k.fused_v210_combine_multi(dl, mine, w, h, *rd_d)
        assert t.route == FIELD % (2, 1), t.route
        k.chan_compose_multi(chan_layers(dl, w, h), theirs, w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
    for a, b in zip(mine, theirs):
        for pl, (p, q) in enumerate(zip(a["planes"], b["planes"])):
            assert torch.equal(p, q), "%s plane %d differs from ph_chan_compose_multi's" % (a["fmt"], pl)
            assert not bool((p == POISON).all())
    _layers.pop((w, h, 31), None)
