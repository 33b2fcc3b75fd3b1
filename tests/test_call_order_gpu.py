"""GPU tests (-m gpu) of the one promise every launch-sharing of ph_run_programs rests on: the call is exactly ph_run_program for
j = 0 .. n_jobs - 1 in that order - a job that reads what an earlier job of the call writes, writes what one reads or writes what one
writes is kept out of that job's launch.  A broken promise gives a stale or garbled frame and no error, so it is pinned from both sides:
the frames (one call against the same jobs posted one by one, byte for byte over every buffer; against the oracle's chain) and the
launches (a call with a hazard takes more of them than the same call without).  The calls come from tests/call_order.py: directed cells
[A, B, C] for every kind of job and hazard - the 2 x 2-block compositor's layer images, either field's, both image formats, any layer -
and seeded random calls (PH_FUZZ_SEED / PH_FUZZ_CASES).  Also ph_run_programs_progress after calls that made nothing."""
import ctypes
import os

import numpy as np
import pytest

import call_order as co
import frames
from oracle import orc
from phaneron_amd import capi

pytestmark = pytest.mark.gpu

W, H, SW, SH = co.W, co.H, co.SW, co.SH
WORDS = co.IMAGE_BYTES // 4
CELLS = co.directed_cells()
# one cell per kind of job is also held against the oracle's chain of operators (frames feeding frames for the v210 kinds; for the
# compositor a frame written over an image an earlier job shows)
ORACLE_CELLS = ("fused-RAW", "chan-RAW", "up_rgba-WAR-l1", "up_packed-WAR", "up_pair-WAR")


def upload(ctx, arr, dims=None, svm="coarse"):
    a = np.ascontiguousarray(arr)
    b = ctx.create_buffer(a.nbytes, "readwrite", svm, dims=dims, owner="call_order")
    b.host_access("writeonly", capi.QUEUE_LOAD, a)
    return b


def pool_words(i):
    """what pool buffer i holds before a call: v210 words (384 x 90 of them fill the 92 160 bytes)"""
    return frames.v210_random(W, co.IMAGE_BYTES // (W * 8 // 3), frames.layer_seed(170, i))


def image_words(i):
    """... or, for the comparison with the oracle, an image with something to show (its first three quarters: the packed-RGB image)"""
    return frames.rgba_random(SW, SH, 1700 + i, -0.05, 1.05).reshape(-1).view(np.uint32)


class Rig:
    """what every job of these calls names besides its frames: the Loader's and Saver's buffers, the placements, the programs, the
    fixed planes of a planar source"""

    def __init__(self, ctx):
        self.ctx = ctx
        spec = "709"
        # (as loadSave.ts:50-99,139-160 creates them, and tests/test_boundary_gpu.py's Colour)
        self.recipe = {"colMatrix": upload(ctx, capi.ycbcr2rgb_matrix(spec), svm="none"), "gammaLut": upload(ctx, capi.gamma2linear_lut(spec)),
                       "gamutMatrix": upload(ctx, capi.rgb2rgb_matrix(spec, spec), svm="none"),
                       "outColMatrix": upload(ctx, capi.rgb2ycbcr_matrix(spec), svm="none"), "outGammaLut": upload(ctx, capi.linear2gamma_lut(spec))}
        self.saver = {k: self.recipe[k] for k in ("outColMatrix", "outGammaLut")}
        self.oracle_rd = (orc.ycbcr2rgb_matrix(spec), orc.gamma2linear_lut(spec), orc.rgb2rgb_matrix(spec, spec))
        self.oracle_wr = (orc.rgb2ycbcr_matrix(spec), orc.linear2gamma_lut(spec))
        self.fill, self.small = np.zeros(12, np.float32), np.zeros(12, np.float32)
        self.fill[:9] = capi.transform_matrix(W, H)
        self.small[:9] = capi.transform_matrix(W, H, scale_x=0.5, scale_y=0.5, offset_x=0.2)
        self.bf, self.bs = upload(ctx, self.fill, svm="none"), upload(ctx, self.small, svm="none")
        y, _, v = frames.pack_random("yuv422p8", W, H, 171)  # a planar layer's Y and V planes: read-only, its U plane is a pool buffer
        self.y_plane, self.v_plane = upload(ctx, y), upload(ctx, v)
        ctx.wait(capi.QUEUE_LOAD)
        self.progs = {("fused", n): ctx.create_program("phaneron:fused", "fused_v210_combine_%d" % n, [W, H]) for n in (1, 2, 3)}
        self.progs.update({("chan", n): ctx.create_program("phaneron:chan", "chan_compose_v210_%d" % n, [W, H]) for n in (1, 2)})
        self.progs.update({("up", n): ctx.create_program("phaneron:up", "compose_up_write_v210_%d" % n, [W, H]) for n in (1, 2)})
        self.own = list(self.recipe.values()) + [self.bf, self.bs, self.y_plane, self.v_plane]

    def pool(self, contents):
        bufs = [upload(self.ctx, contents[i], dims=(SW, SH) if i in co.IMAGES else None) for i in range(co.POOL)]
        self.ctx.wait(capi.QUEUE_LOAD)
        return bufs

    def job(self, j, pool):
        """(program, by-name arguments) of a job of the spec"""
        kind, n = j["kind"], j["n"]
        if kind == "fused":
            params = dict(self.recipe, output=pool[j["out"]])
            params.update({"l%dIn" % l: pool[i] for l, i in enumerate(j["ins"])})
        elif kind == "chan":
            params = dict(self.recipe, output=pool[j["out"]], interlace=0)
            for l, i in enumerate(j["ins"]):
                params["l%dMatrix" % l] = self.bs if j["small"][l] else self.bf
                if j["planar"][l]:
                    params.update({"l%dIn" % l: self.y_plane, "l%dInU" % l: pool[i], "l%dInV" % l: self.v_plane, "l%dPacking" % l: capi.FORMATS["yuv422p8"],
                                   "l%dWidth" % l: W, "l%dHeight" % l: H})
                else:  # a buffer with image dims: an RGBA image of its dims; one without: a v210 frame of the size named
                    params.update({"l%dIn" % l: pool[i], "l%dWidth" % l: W, "l%dHeight" % l: H})
        else:
            params = dict(self.saver, interlace=0, output=pool[j["out"]])
            if j["out2"] is not None:
                params["output2"] = pool[j["out2"]]
            for l, i in enumerate(j["ins"]):
                params.update({"l%dIn" % l: pool[i], "l%dMatrix" % l: self.bf})
                if j["ins2"] is not None:
                    params["l%dIn2" % l] = pool[j["ins2"][l]]
                if j["packed"]:
                    params.update({"packedRgb": 1, "l%dWidth" % l: SW, "l%dHeight" % l: SH})
        return self.progs[(kind, n)], params

    def release(self):
        for b in self.own:
            b.release()


@pytest.fixture(scope="module")
def rig():
    c = capi.Context(0)
    r = Rig(c)
    yield r
    r.release()
    c.close()


@pytest.fixture(scope="module")
def contents():
    return [pool_words(i) for i in range(co.POOL)]


def read_back(pool):
    got = []
    for b in pool:
        b.host_access("readonly", capi.QUEUE_UNLOAD)
        got.append(b.host(np.uint32).copy())
    return got


def run_both(rig, spec, contents, traced=False):
    """the call as one ph_run_programs and, on a second set of buffers that starts out the same, one ph_run_program per job:
    (every buffer of the first, every buffer of the second, the one call's launches)"""
    sides, launches = [], None
    for one_call in (True, False):
        pool = rig.pool(contents)
        jobs = [rig.job(j, pool) for j in spec]
        if not one_call:
            for prog, params in jobs:
                rig.ctx.run_program(prog, params)
        elif traced:
            with capi.trace() as t:
                rig.ctx.run_programs(jobs)
            launches = len(t.kernels)
        else:
            rig.ctx.run_programs(jobs)
        rig.ctx.wait()
        sides.append(read_back(pool))
        for b in pool:
            b.release()
    return sides[0], sides[1], launches


def dry_launches(rig, spec, contents):
    """how many launches ph_run_programs makes of the call (a dry run: the kernels are chosen, nothing is enqueued)"""
    pool = rig.pool(contents)
    jobs = [rig.job(j, pool) for j in spec]
    with capi.trace(dry_run=True) as t:
        rig.ctx.run_programs(jobs)
    for b in pool:
        b.release()
    return len(t.kernels)


def oracle_pool(rig, spec, contents):
    """every pool buffer after the call, by the oracle's operators job by job"""
    mem = [np.array(c, dtype=np.uint32) for c in contents]
    frame_words = co.FRAME_BYTES // 4

    def v210(i):
        return orc.v210_read(mem[i][:frame_words], W, H, *rig.oracle_rd)

    def image(i, packed=False):
        if not packed:
            return mem[i].view(np.float32).reshape(SH, SW, 4)
        rgba = np.ones((SH, SW, 4), np.float32)
        rgba[..., :3] = mem[i][:co.PACKED_BYTES // 4].view(np.float32).reshape(SH, SW, 3)
        return rgba

    def write(i, img):
        mem[i][:frame_words] = np.asarray(orc.v210_write(img, W, H, 0, *rig.oracle_wr)).reshape(-1).view(np.uint32)

    for j in spec:
        if j["kind"] == "fused":
            layers = [v210(i) for i in j["ins"]]
            write(j["out"], layers[0] if len(layers) == 1 else orc.combine(layers))
        elif j["kind"] == "chan":
            assert not any(j["planar"])  # (no cell held against the oracle has a planar layer)
            placed = [orc.transform(image(i) if i in co.IMAGES else v210(i), (rig.small if s else rig.fill)[:9], W, H) for i, s in zip(j["ins"], j["small"])]
            write(j["out"], placed[0] if len(placed) == 1 else orc.combine(placed))
        else:
            for ins, out in ((j["ins"], j["out"]),) + (((j["ins2"], j["out2"]),) if j["out2"] is not None else ()):
                placed = [orc.transform(image(i, j["packed"]), rig.fill[:9], W, H) for i in ins]
                write(out, placed[0] if len(placed) == 1 else orc.combine(placed))
    return mem


@pytest.mark.parametrize("name", sorted(CELLS))
def test_a_job_with_a_hazard_against_the_job_before_it_keeps_out_of_its_launch(rig, contents, name):
    """[A, B, C] of one shape, B with exactly one hazard against A (its kind and argument in the cell's name), C independent: every buffer
    after the one call equals, byte for byte, the jobs posted one by one; the call takes more launches than the same call with B's
    clashing argument replaced by a buffer of its own, which takes one"""
    cls, hazard, hot, free = CELLS[name]
    if name in ORACLE_CELLS:  # images with something to show where a job of the cell reads a buffer as an image
        as_image = {i for j in hot if j["kind"] != "fused" for i in co.reads(j) if i in co.IMAGES or j["kind"] == "up"}
        contents = [image_words(i) if i in as_image else c for i, c in enumerate(contents)]
    one, each, hot_launches = run_both(rig, hot, contents, traced=True)
    for i, (a, b) in enumerate(zip(one, each)):
        assert np.array_equal(a, b), "%s: buffer %d of the one call differs from the separate calls (%d words): %r" % (name, i, int(np.count_nonzero(a != b)), hot)
    written = {i for j in hot for i in co.writes(j)}
    for i in range(co.POOL):
        assert np.array_equal(one[i], contents[i]) == (i not in written), "%s: buffer %d" % (name, i)
    free_launches = dry_launches(rig, free, contents)
    print("%s: %d launches with the hazard, %d without" % (name, hot_launches, free_launches))
    assert free_launches == 1, "%s: the call without a hazard takes %d launches" % (name, free_launches)
    assert hot_launches > free_launches, "%s: %d launches with the hazard, %d without" % (name, hot_launches, free_launches)
    assert dry_launches(rig, hot, contents) == hot_launches
    if name in ORACLE_CELLS:
        want = oracle_pool(rig, hot, contents)
        for i in range(co.POOL):
            assert np.array_equal(one[i], want[i]), "%s: buffer %d differs from the oracle's chain (%d words)" % (name, i, int(np.count_nonzero(one[i] != want[i])))


def test_the_two_fields_of_one_frame_from_the_channel_kernel_stay_in_one_launch(rig, contents):
    """chan_compose_v210_<n> jobs that write the same frame are not parted by ph_run_programs - the upper and the lower field of buffer 4,
    from two sources, are one launch (ph_chan_compose_batch keeps the two fields of a frame together) - while the same field written
    twice is two, the later job's lines standing: every buffer equals the jobs posted one by one"""
    upper, lower = co.job("chan", 1, [0], 4, small=[True]), co.job("chan", 1, [6], 4, small=[True])

    class Fields(Rig):  # the rig's jobs, each with the field named in its spec
        def __init__(self):
            self.__dict__.update(rig.__dict__)

        def job(self, j, pool):
            prog, params = Rig.job(self, j, pool)
            return prog, dict(params, interlace=j["field"])
    fields = Fields()
    for (fa, fb), launches in (((1, 3), 1), ((3, 1), 1), ((1, 1), 2), ((3, 3), 2)):
        spec = [dict(upper, field=fa), dict(lower, field=fb)]
        one, each, traced = run_both(fields, spec, contents, traced=True)
        for i, (a, b) in enumerate(zip(one, each)):
            assert np.array_equal(a, b), "fields %d, %d: buffer %d of the one call differs from the separate calls" % (fa, fb, i)
        assert not np.array_equal(one[4], contents[4])
        assert traced == launches and dry_launches(fields, spec, contents) == launches, "fields %d, %d: %d launches" % (fa, fb, traced)


def test_random_calls_of_every_kind_of_job_equal_the_jobs_posted_one_by_one(rig, contents):
    """seeded random calls (PH_FUZZ_SEED, PH_FUZZ_CASES; 25 cases of 2 - 8 jobs by default, tests/test_call_order_cpu.py says what they
    hold) of headline, channel and compositor jobs - RGBA and packed images, one field and two - whose arguments are each other's frames:
    every buffer of the pool after the one call equals the same jobs posted one ph_run_program each"""
    specs = co.draw_cases(os.environ.get("PH_FUZZ_SEED", co.DEFAULT_SEED), os.environ.get("PH_FUZZ_CASES", co.DEFAULT_CASES))
    for case, spec in enumerate(specs):
        one, each, _ = run_both(rig, spec, contents)
        for i, (a, b) in enumerate(zip(one, each)):
            assert np.array_equal(a, b), "case %d: buffer %d of the one call differs from the separate calls (%d words): %r" % (
                case, i, int(np.count_nonzero(a != b)), spec)
        assert any(not np.array_equal(one[i], contents[i]) for i in range(co.POOL)), "case %d wrote nothing" % case
    assert specs, "no cases drawn"
    print("%d calls, %d jobs, %d pairs of launch-sharing candidates" % (len(specs), sum(len(s) for s in specs), co.census(specs)[1]))


def test_progress_is_zero_after_every_call_that_made_nothing(rig, contents):
    """ph_run_programs_progress: 4 after a call of four jobs; 0 after a call refused at its first checks (n_jobs = 0) and after one refused
    by a bad job - never the count of the call before, which a binding would take for frames made (node/defer.js retires that many plans)"""
    pool = rig.pool(contents)
    done = ctypes.c_int(-1)

    def progress():
        capi.check(capi.lib().ph_run_programs_progress(ctypes.byref(done)))
        return done.value

    four = [rig.job(co.job("fused", 1, [i], 4 + i), pool) for i in range(4)]
    rig.ctx.run_programs(four)
    assert progress() == 4
    rc = capi.lib().ph_run_programs(rig.ctx.h, 0, None, None, None, capi.QUEUE_PROCESS)
    assert rc != 0
    assert progress() == 0
    rig.ctx.run_programs(four)
    assert progress() == 4
    prog, params = rig.job(co.job("fused", 2, [0, 1], 5), pool)
    del params["l1In"]  # a two-layer job without its second layer
    with pytest.raises(capi.PhaneronError, match="l1In"):
        rig.ctx.run_programs(four[:2] + [(prog, params)])
    assert progress() == 0
    rig.ctx.run_programs(four)
    assert progress() == 4
    with pytest.raises(capi.PhaneronError):  # a queue there is not: refused before any job is looked at
        rig.ctx.run_programs(four, queue=99)
    assert progress() == 0
    rig.ctx.wait()
    for b in pool:
        b.release()
