"""GPU tests (-m gpu) of ph_fused_v210_combine_multi_batch: several channels' plain-layer composites, each for the same list of up to
four consumers, in one launch.  Every plane of every output of every job is compared byte for byte, on planes poisoned with 0x5A, with
the oracle's chain (orc.v210_read x n -> orc.combine -> that format's oracle writer) and with the same jobs posted as separate
ph_fused_v210_combine_multi calls.  Every job has a layer seed of its own: a job that reads another job's layers, or writes another
job's planes, shows.  The reader's table is test_fused_multi_gpu's (entry 0 = +Inf: every layer shows)."""
import re

import numpy as np
import pytest

import frames
import guard
import luts
from oracle import orc
from test_chan_multi_gpu import POISON, ByName, oracle_frame, out, poisoned, writer
from test_fused_multi_gpu import composite, expect_three, layer_words, reader, three_outputs

pytestmark = pytest.mark.gpu

ONE = "fused_v210_combine_multi x%d"
SHARED = "fused_v210_combine_multi x%dj%d"


def seed_of(job):
    return 60 + job


def make_jobs(w, h, n, jobs, outs, rd_o, dst=None, src=None):
    """(device layers per job, output dicts per job, plane tensors per job, the oracle's planes per job)"""
    import hip_harness as hh
    recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]  # once: every job names the same matrices and tables
    make = dst or (lambda p, fmt: hh.dev(p))
    layers, outputs, planes, want = [], [], [], []
    for j in range(jobs):
        layers.append([(src or hh.dev)(l) for l in layer_words(w, h, n, seed_of(j))])
        comp = composite(w, h, n, rd_o, seed_of(j))
        planes.append([[make(p, o["fmt"]) for p in poisoned(o["fmt"], w, h)] for o in outs])
        outputs.append([dict(fmt=o["fmt"], planes=d, interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3]) for o, d, rc in zip(outs, planes[j], recipes)])
        want.append([oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1]) for o, rc in zip(outs, recipes)])
    return layers, outputs, planes, want


def fetch(planes):
    import hip_harness as hh
    return [[[hh.host(p, np.uint8).reshape(-1) for p in d] for d in job] for job in planes]


def check(w, h, n, jobs, outs, what, rd=None, route=None, separate=True, dst=None, src=None):
    """one ph_fused_v210_combine_multi_batch call against the oracle and the separate ph_fused_v210_combine_multi calls; returns
    (route, the bytes [job][output][plane])"""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, rd_d = rd or reader()
    k = hh.ctx()
    layers, outputs, planes, want = make_jobs(w, h, n, jobs, outs, rd_o, dst, src)
    with capi.trace() as t:
        k.fused_v210_combine_multi_batch(layers, outputs, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    got = fetch(planes)
    for j in range(jobs):
        for i, o in enumerate(outs):
            for pl, (g, wnt) in enumerate(zip(got[j][i], want[j][i])):
                bad = np.flatnonzero(g != wnt)
                assert bad.size == 0, "%s: job %d output %d (%s il %d) plane %d: %d of %d bytes differ from the oracle, first at %d (got %#x, want %#x)" % (
                    what, j, i, o["fmt"], o["interlace"], pl, bad.size, g.size, bad[0], g[bad[0]], wnt[bad[0]])
    if route is not None:
        assert t.route == route, "%s: route %r" % (what, t.route)
    if separate:
        _, alone_outputs, alone_planes, _ = make_jobs(w, h, n, jobs, outs, rd_o)
        with capi.trace() as t1:
            for j in range(jobs):
                k.fused_v210_combine_multi(layers[j], alone_outputs[j], w, h, *rd_d)
        k.wait()
        torch.cuda.synchronize()
        alone = fetch(alone_planes)
        for j in range(jobs):
            for i in range(len(outs)):
                for pl in range(len(got[j][i])):
                    assert np.array_equal(got[j][i][pl], alone[j][i][pl]), "%s: job %d output %d plane %d differs from the separate call's" % (what, j, i, pl)
        return t.route, got, t1.route
    return t.route, got


# ---- shapes and job counts ----------------------------------------------------------------------------------------------------------
FOUR = [out("nv12"), out("v210"), out("bgra8"), out("yuv422p10")]


@pytest.mark.parametrize("jobs", [2, 3, 5, 8])
@pytest.mark.parametrize("n", [1, 4])
def test_four_outputs_for_every_job_count(n, jobs):
    """384 x 6; 3 and 5 jobs do not divide the CU count"""
    check(384, 6, n, jobs, FOUR, "%d jobs, %d layers" % (jobs, n), route=SHARED % (4, jobs))


def test_ranges_begin_in_mid_line():
    """1920 x 8: each job has 2560 quads and three workgroups of 854 - ranges that begin and end in mid-line - with 4:2:0 chroma rows"""
    check(1920, 8, 2, 3, [out("nv12"), out("yuv420p"), out("v210")], "1920x8, 3 jobs", route=SHARED % (3, 3))


@pytest.mark.parametrize("w,h,jobs,wgs,why", [(384, 48, 2, 1, "three full slices a lane"), (768, 50, 2, 1, "a second tile of 256 quads that four waves hold"),
                                              (96, 33, 3, 2, "ranges of 264 quads: a partly filled wave, an odd height")])
def test_capped_workgroups(w, h, jobs, wgs, why):
    import hip_harness as hh
    k = hh.ctx()
    k.set_option("fused_multi_wgs", wgs)
    try:
        outs = [out("v210"), out("rgba8", 3), out("yuv422p8")] if h % 2 else [out("v210"), out("nv12", 3), out("yuv420p"), out("bgra8")]
        check(w, h, 2, jobs, outs, "%dx%d, %d jobs, %d workgroups each (%s)" % (w, h, jobs, wgs, why), route=SHARED % (len(outs), jobs))
    finally:
        k.set_option("fused_multi_wgs", 0)


# ---- fields -------------------------------------------------------------------------------------------------------------------------
def test_field_mixes_on_an_odd_height():
    w, h = 96, 9
    _, got, _ = check(w, h, 3, 2, [out("v210", 1), out("rgba8", 0), out("bgra8", 3), out("v210", 3)], "96x9 fields", route=SHARED % (4, 2))
    for job in got:
        rows = job[0][0].reshape(h, -1)
        assert (rows[1::2] == POISON).all() and (rows[8] == POISON).all() and not (rows[0:8:2] == POISON).all(), "a v210 field 1 output takes lines 0, 2, 4, 6 only"
        rows = job[2][0].reshape(h, -1)
        assert (rows[0::2] == POISON).all() and not (rows[1::2] == POISON).all(), "a bgra8 field 3 output takes the odd lines only"


def test_a_420_field_beside_a_420_frame():
    w, h = 384, 10
    _, got, _ = check(w, h, 3, 2, [out("yuv420p", 3), out("nv12", 0), out("v210", 1), out("yuv422p8", 3)], "384x10: 4:2:0 field 3 + 4:2:0 frame", route=SHARED % (4, 2))
    for job in got:
        luma = job[0][0].reshape(h, w)
        assert (luma[0::2] == POISON).all() and not (luma[1::2] == POISON).all(), "a yuv420p field 3 output takes the odd lines only"


# ---- tables -------------------------------------------------------------------------------------------------------------------------
def test_two_tables_interleaved():
    tab = luts.layout_table(32, 8, 0xF00D)
    with luts.register(tab) as dtab:
        outs = [out("v210"), out("yuv422p8", spec=(tab, dtab)), out("rgba8"), out("nv12", spec=(tab, dtab))]
        _, got, _ = check(384, 6, 3, 2, outs, "two tables, outputs interleaved", route=SHARED % (4, 2))
        _, same = check(384, 6, 3, 2, [out("yuv422p8"), out("rgba8")], "the same output from the shared table", separate=False)
        assert not np.array_equal(got[1][1][0], same[1][0][0]), "the table of other contents does not show in its output"


@pytest.mark.parametrize("rl,wl", [(luts.SMALLEST, luts.LARGEST), (luts.LARGEST, luts.SMALLEST)], ids=["wr-largest", "rd-largest"])
def test_table_layouts(rl, wl):
    import hip_harness as hh
    from phaneron_amd import capi
    from test_lut_layouts_gpu import forced, gamut12
    with forced(rl, "r") as (rtab, drtab), forced(wl, "w") as (wtab, dwtab):
        rd = ((orc.ycbcr2rgb_matrix("709"), rtab, luts.IDENTITY), (hh.dev(capi.ycbcr2rgb_matrix("709")), drtab, hh.dev(gamut12())))
        outs = [out("v210", spec=(wtab, dwtab)), out("yuv422p10", spec=(wtab, dwtab)), out("rgba8")]
        check(384, 6, 2, 2, outs, "layouts %r / %r" % (rl, wl), rd=rd, route=SHARED % (3, 2))


# ---- identities ---------------------------------------------------------------------------------------------------------------------
def test_one_job_is_the_single_call():
    _, _, alone = check(384, 6, 2, 1, [out("v210"), out("rgba8"), out("nv12")], "one job", route=ONE % 3)
    assert alone == ONE % 3


def test_v210_frames_only_is_the_headline_batch():
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    w, h, n, jobs = 384, 6, 3, 3
    route, got, _ = check(w, h, n, jobs, [out("v210")], "v210 frames only")
    k = hh.ctx()
    _, rd_d = reader()
    rc = writer("v210", "709")
    layers = [[hh.dev(l) for l in layer_words(w, h, n, seed_of(j))] for j in range(jobs)]
    dsts = [hh.dev(poisoned("v210", w, h)[0]) for _ in range(jobs)]
    with capi.trace() as t:
        k.fused_v210_combine_batch(layers, dsts, w, h, *rd_d, rc[2], rc[3])
    k.wait()
    torch.cuda.synchronize()
    assert route == t.route and "multi" not in route, (route, t.route)
    for j in range(jobs):
        assert np.array_equal(got[j][0][0], hh.host(dsts[j], np.uint8).reshape(-1)), "job %d differs from ph_fused_v210_combine_batch's frame" % j


# ---- fallback -----------------------------------------------------------------------------------------------------------------------
def test_another_width_runs_the_jobs_one_by_one():
    route, _, alone = check(100, 4, 2, 3, [out("v210"), out("rgba8")], "100x4")
    assert route == alone and "fused_v210_combine_multi" not in route and len(route.split("+")) == len(alone.split("+")) >= 3, (route, alone)


def test_an_unregistered_writer_table_answers_as_the_single_calls_do():
    """the call does not qualify for the shared launch and runs ph_fused_v210_combine_multi per job, whose answer (here a refusal that
    names the writer's table: no kernel of the several-outputs calls gathers from a plain table) is this call's; nothing is written"""
    import hip_harness as hh
    from phaneron_amd import capi
    w, h = 384, 6
    rd_o, rd_d = reader()
    k = hh.ctx()
    plain = hh.dev(capi.linear2gamma_lut("709"))  # never registered
    layers, outputs, planes, _ = make_jobs(w, h, 2, 2, [out("v210"), out("rgba8")], rd_o)
    for job in outputs:
        job[1]["wr_lut"] = plain
    answers = []
    for call in (lambda: k.fused_v210_combine_multi_batch(layers, outputs, w, h, *rd_d), lambda: k.fused_v210_combine_multi(layers[0], outputs[0], w, h, *rd_d)):
        with capi.trace() as t:
            with pytest.raises(capi.PhaneronError, match=r"error -1: .*output 1.*writer gamma LUT has no LDS form") as e:
                call()
        answers.append((t.route, str(e.value)))
    assert answers[0] == answers[1], answers
    k.wait()
    assert all((g == POISON).all() for job in fetch(planes) for o in job for g in o), "a refused call wrote"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every refusal is PH_E_INVALID (-1), decided before anything is launched: every plane of every job keeps its poison"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    rd_o, rd_d = reader()
    w, h = 384, 6
    tab = luts.layout_table(32, 8, 0xBEE)

    def attempt(match, jobs=2, tweak=None, fmts=("v210", "rgba8", "yuv422p8")):
        layers, outputs, planes, _ = make_jobs(w, h, 2, max(jobs, 1), [out(f) for f in fmts], rd_o)
        if jobs == 0:
            layers, outputs = [], []
        if tweak:
            tweak(layers, outputs)
        with pytest.raises(capi.PhaneronError, match=match):
            k.fused_v210_combine_multi_batch(layers, outputs, w, h, *rd_d)
        k.wait()
        assert all((g == POISON).all() for job in fetch(planes) for o in job for g in o), "a refused call wrote (%s)" % match

    attempt(r"error -1: .*1\.\.8 jobs", jobs=0)
    attempt(r"error -1: .*1\.\.8 jobs", jobs=9)
    attempt(r"error -1: .*job 1: output 1 differs from job 0's", tweak=lambda l, o: o[1][1].update(fmt="bgra8"))
    attempt(r"error -1: .*job 1: output 0 differs from job 0's", tweak=lambda l, o: o[1][0].update(interlace=1))
    with luts.register(tab) as dtab:
        attempt(r"error -1: .*job 1: output 2 differs from job 0's", tweak=lambda l, o: o[1][2].update(wr_lut=dtab))
    attempt(r"error -1: .*job 0 output 1 and job 1 output 1 name the same plane", tweak=lambda l, o: o[1][1].update(planes=o[0][1]["planes"]))
    attempt(r"error -1: .*p010.*run the separate kernels.*ph_pack_write", tweak=lambda l, o: [j[1].update(fmt="p010") for j in o], fmts=("v210", "yuv422p10"))
    attempt(r"error -1: .*job 1: layer 1 is NULL", tweak=lambda l, o: l[1].__setitem__(1, None))
    attempt(r"error -1: .*job 0: output 1.*interlace must be 0, 1 or 3", tweak=lambda l, o: [j[1].update(interlace=2) for j in o])


# ---- guard bands --------------------------------------------------------------------------------------------------------------------
def test_between_guard_bands():
    """a 2-job, 3-output call with every layer and every plane between guard bands"""
    w, h = 384, 6
    guard.reset()
    try:
        def dst(p, fmt):
            return guard.dev(p, "dst", pitch=max(1, p.size // h))

        def src(l):
            return guard.dev(l, "src", pitch=frames.v210_pitch_bytes(w))
        check(w, h, 3, 2, [out("yuv420p"), out("v210", 1), out("bgra8", 3)], "between guards", route=SHARED % (3, 2), separate=False, dst=dst, src=src)
        assert guard.check() == (6, 10)
    finally:
        guard.reset()


# ---- by name: ph_run_programs with the option "fused_multi_batch" -------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(384, 6)
    yield b
    b.ctx.set_option("fused_multi_batch", 0)
    b.close()


def four_jobs(b, prog):
    """four fused_v210_combine_multi_2 jobs for v210 + yuv422p8 + rgba8 field 3 (test_fused_multi_gpu.three_outputs), a layer seed each"""
    jobs, outs, want = [], [], []
    for j in range(4):
        words = layer_words(b.w, b.h, 2, seed_of(j))
        params, o = three_outputs(b, [b.upload(l, svm="coarse") for l in words])
        jobs.append((prog, params)), outs.append(o)
        want.append(expect_three(b, orc.combine([orc.v210_read(l, b.w, b.h, *b.rd_o) for l in words])))
    b.ctx.wait(b.capi.QUEUE_LOAD)
    return jobs, outs, want


def expect_bytes(b, outs, want, what):
    for j, (job, wj) in enumerate(zip(outs, want)):
        for i, (planes, wnt) in enumerate(zip(job, wj)):
            for pl, (p, x) in enumerate(zip(planes, wnt)):
                assert np.array_equal(b.read(p), x), "%s: job %d output %d plane %d" % (what, j, i, pl)


@pytest.mark.parametrize("option,route", [(0, [ONE % 3] * 4), (1, [SHARED % (3, 4)])], ids=["off", "on"])
def test_by_name_the_option_decides_the_launches(by_name, option, route):
    b = by_name
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [b.w, b.h])
    jobs, outs, want = four_jobs(b, prog)
    if option:
        b.ctx.set_option("fused_multi_batch", option)
    with b.capi.trace(dry_run=True) as t:
        b.ctx.run_programs(jobs)
    assert t.kernels == route, t.route
    for job in outs:
        for planes in job:
            for p in planes:
                assert (b.read(p) == POISON).all(), "a dry run wrote"
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels == route, t.route
    expect_bytes(b, outs, want, "option %d" % option)
    prog.destroy()


def test_by_name_a_job_that_reads_an_earlier_output_splits_the_group(by_name):
    """job 2's layer 0 is job 0's v210 output: jobs 0 and 1 share a launch, job 2 starts the next with job 3"""
    b, w, h = by_name, by_name.w, by_name.h
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])
    jobs, outs, want = four_jobs(b, prog)
    jobs[2][1]["l0In"] = outs[0][0][0]
    second = layer_words(w, h, 2, seed_of(2))[1]
    want[2] = expect_three(b, orc.combine([orc.v210_read(want[0][0][0].view(np.uint32), w, h, *b.rd_o), orc.v210_read(second, w, h, *b.rd_o)]))
    b.ctx.set_option("fused_multi_batch", 1)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels == [SHARED % (3, 2), SHARED % (3, 2)], t.route
    expect_bytes(b, outs, want, "a read after a write")
    prog.destroy()


def test_by_name_a_job_that_writes_an_earlier_layer_splits_the_group(by_name):
    """job 2's v210 frame is written over job 0's layer 0: jobs 0 and 1 share a launch - job 0 has read its layer by then - and job 2
    starts the next with job 3"""
    b, w, h = by_name, by_name.w, by_name.h
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])
    jobs, outs, want = four_jobs(b, prog)
    layer = jobs[0][1]["l0In"]
    jobs[2][1]["output"] = layer
    outs[2] = ([layer],) + tuple(outs[2][1:])
    b.ctx.set_option("fused_multi_batch", 1)
    with b.capi.trace(dry_run=True) as dry:
        b.ctx.run_programs(jobs)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels == dry.kernels == [SHARED % (3, 2), SHARED % (3, 2)], t.route
    expect_bytes(b, outs, want, "a write after a read")
    prog.destroy()


def test_by_name_a_job_that_writes_an_earlier_output_splits_the_group(by_name):
    """job 2's yuv422p8 chroma plane U is job 0's - no first plane, which the typed call would refuse: jobs 0 and 1 share a launch, job 2
    starts the next with job 3, and its chroma stands"""
    b, w, h = by_name, by_name.w, by_name.h
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [w, h])
    jobs, outs, want = four_jobs(b, prog)
    jobs[2][1]["output1U"] = outs[0][1][1]
    outs[2] = (outs[2][0], [outs[2][1][0], outs[0][1][1], outs[2][1][2]], outs[2][2])
    want[0][1] = [want[0][1][0], want[2][1][1], want[0][1][2]]
    b.ctx.set_option("fused_multi_batch", 1)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels == [SHARED % (3, 2), SHARED % (3, 2)], t.route
    expect_bytes(b, outs, want, "a write after a write")
    prog.destroy()


def test_by_name_another_output_list_splits_the_group(by_name):
    b = by_name
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [b.w, b.h])
    jobs, outs, want = four_jobs(b, prog)
    jobs[1][1]["interlace2"] = 0  # job 1's rgba8 output: a frame, where the others write field 3
    words = layer_words(b.w, b.h, 2, seed_of(1))
    comp = orc.combine([orc.v210_read(l, b.w, b.h, *b.rd_o) for l in words])
    want[1][2] = oracle_frame("rgba8", comp, b.w, b.h, 0, None, orc.linear2gamma_lut("709"))
    b.ctx.set_option("fused_multi_batch", 1)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.kernels == [ONE % 3, ONE % 3, SHARED % (3, 2)], t.route
    expect_bytes(b, outs, want, "another output list")
    prog.destroy()


def test_by_name_the_option_takes_0_or_1(by_name):
    with pytest.raises(by_name.capi.PhaneronError, match=r"error -1: .*fused_multi_batch"):
        by_name.ctx.set_option("fused_multi_batch", 2)


def test_by_name_an_injected_failure_is_asked_once_in_front_of_the_group(by_name):
    import ctypes
    b = by_name
    capi = b.capi
    prog = b.ctx.create_program("phaneron:fused", "fused_v210_combine_multi_2", [b.w, b.h])
    jobs, outs, want = four_jobs(b, prog)
    b.ctx.set_option("fused_multi_batch", 1)
    b.ctx.set_option("fail_launches", 1)
    try:
        with pytest.raises(capi.PhaneronError, match="injected"):
            b.ctx.run_programs(jobs)
        done = ctypes.c_int(-1)
        assert capi.lib().ph_run_programs_progress(ctypes.byref(done)) == 0 and done.value == 0
    finally:
        b.ctx.set_option("fail_launches", 0)
    for job in outs:
        for planes in job:
            for p in planes:
                assert (b.read(p) == POISON).all(), "a failed call wrote"
    # -1: one launch goes through, then every one fails - the group of four is ONE launch, and the call after it fails
    b.ctx.set_option("fail_launches", -1)
    try:
        b.ctx.run_programs(jobs)
        with pytest.raises(capi.PhaneronError, match="injected"):
            b.ctx.run_programs(jobs)
    finally:
        b.ctx.set_option("fail_launches", 0)
    b.ctx.wait()
    expect_bytes(b, outs, want, "the launch that went through")
    prog.destroy()
