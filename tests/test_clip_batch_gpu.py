"""GPU tests (-m gpu) of ph_clip_compose_batch_out: several channels' file playback - an enlarged clip, or a decoder's frame under the
default fill - each packed for up to four consumers, in one launch of the clip kernel.  Every output of every job is compared, byte for
byte, with the oracle's chain (destinations poisoned with 0x5A first), with a separate ph_clip_compose_multi call per job and with a
separate ph_chan_compose call per output; every case meant for the shared launch asserts its traced route (a silent per-job fallback
cannot pass), and that a dry run gives the same route and writes nothing."""
import ctypes

import numpy as np
import pytest

import frames
import packfmt
from test_chan_gpu import Src, colour, device_layers, m
from test_chan_multi_gpu import POISON, ByName, composite, oracle_frame, out, poisoned, writer
from test_clip_multi_gpu import SH, SW, clip, clip_params, expect_two, outputs_of, small_clip

pytestmark = pytest.mark.gpu

ALL_OUT = ["v210"] + list(packfmt.CHAN_OUT)
SOURCES = ["yuv420p", "nv12", "yuv422p8", "yuv422p10", "yuv420p10", "p010", "rgba8", "bgra8", "v210"]
W, H = 384, 54


class Reads:
    """a job's layers that are an earlier job's output: the rgba8 frame in `slot`, as a decoder's frame under the default fill"""

    def __init__(self, slot, w, h):
        self.slot, self.w, self.h = slot, w, h

    def device(self, planes):
        return [dict(src=(planes[self.slot][0], self.w, self.h, m(self.w, self.h), "rgba8"))]

    def oracle(self, host):  # (a frame nobody has written yet holds the poison)
        frame = host[self.slot] if self.slot in host else poisoned("rgba8", self.w, self.h)
        return [dict(src=Src([frame[0]], self.w, self.h, m(self.w, self.h), fmt="rgba8"))]


def check_batch(jobs, w, h, what, specs=("709", "709")):
    """jobs: list of (layers, outs) - layers a layer list (test_clip_multi_gpu.clip) or a Reads; outs: test_chan_multi_gpu.out(...) dicts,
    optionally with a `slot`: outputs of one slot name the same planes.  One ph_clip_compose_batch_out call against the oracle, against a
    ph_clip_compose_multi call per job and against a ph_chan_compose call per output.  Returns the traced route."""
    import torch
    import hip_harness as hh
    from phaneron_amd import capi
    rd_o, _, rd_d, _ = colour(*specs)
    k = hh.ctx()
    sides = []
    for _ in range(3):
        planes = {}
        for j, (_, outs) in enumerate(jobs):
            for i, o in enumerate(outs):
                if o.get("slot", (j, i)) not in planes:
                    planes[o.get("slot", (j, i))] = [hh.dev(p) for p in poisoned(o["fmt"], w, h)]
        sides.append(planes)
    uploaded = {}  # a job's sources are uploaded once and read by every side

    def posted(side):
        res = []
        for j, (layers, outs) in enumerate(jobs):
            if isinstance(layers, Reads):
                dl = layers.device(sides[side])
            else:
                if j not in uploaded:
                    uploaded[j] = device_layers(layers)
                dl = uploaded[j]
            recipes = [writer(o["fmt"], o["spec"], o["own_table"]) for o in outs]
            res.append((dl, [dict(fmt=o["fmt"], planes=sides[side][o.get("slot", (j, i))], interlace=o["interlace"], wr_cm=rc[2], wr_lut=rc[3])
                             for i, (o, rc) in enumerate(zip(outs, recipes))]))
        return res
    together = posted(0)
    with capi.trace(dry_run=True) as dry:
        k.clip_compose_batch_out(together, w, h, *rd_d)
    k.wait()
    torch.cuda.synchronize()
    assert all((hh.host(p, np.uint8) == POISON).all() for planes in sides[0].values() for p in planes), "%s: a dry run wrote" % what
    with capi.trace() as t:
        k.clip_compose_batch_out(together, w, h, *rd_d)
    k.wait()
    assert dry.route == t.route, "%s: the dry run's route %s, the call's %s" % (what, dry.route, t.route)
    for dl, outputs in posted(1):
        k.clip_compose_multi(dl, outputs, w, h, *rd_d)
    for dl, outputs in posted(2):
        for o in outputs:
            k.chan_compose_v210(dl, o["planes"][0] if o["fmt"] == "v210" else o["planes"], w, h, o["interlace"], *rd_d, o["wr_cm"], o["wr_lut"], out_fmt=o["fmt"])
    k.wait()
    torch.cuda.synchronize()
    got = {slot: [hh.host(p, np.uint8) for p in planes] for slot, planes in sides[0].items()}
    for other, name in ((1, "a ph_clip_compose_multi call per job"), (2, "a ph_chan_compose call per output")):
        for slot in got:
            for pl, b in enumerate(sides[other][slot]):
                want = hh.host(b, np.uint8)
                bad = np.flatnonzero(got[slot][pl] != want)
                assert bad.size == 0, "%s [%s]: output %r plane %d: %d of %d bytes differ from %s, first at %d" % (what, t.route, slot, pl, bad.size, want.size, name, bad[0])
    # the oracle, job after job: a later writer of a slot wins, a reader takes what the jobs before it left
    host = {}
    for j, (layers, outs) in enumerate(jobs):
        comp = composite(layers.oracle(host) if isinstance(layers, Reads) else layers, w, h, rd_o)
        for i, o in enumerate(outs):
            rc = writer(o["fmt"], o["spec"], o["own_table"])
            slot, frame = o.get("slot", (j, i)), oracle_frame(o["fmt"], comp, w, h, o["interlace"], rc[0], rc[1])
            if o["interlace"] and slot in host:  # a field into a frame an earlier job wrote (a format with a row per line in every plane): its lines over that frame's
                lines = slice(1 if o["interlace"] == 3 else 0, None, 2)
                merged = [p.copy() for p in host[slot]]
                for mp, fp in zip(merged, frame):
                    mp.reshape(h, -1)[lines] = fp.reshape(h, -1)[lines]
                frame = merged
            host[slot] = frame
    for slot, planes in host.items():
        for pl, wnt in enumerate(planes):
            bad = np.flatnonzero(got[slot][pl] != wnt)
            assert bad.size == 0, "%s [%s]: output %r plane %d: %d of %d bytes differ from the oracle, first at %d" % (what, t.route, slot, pl, bad.size, wnt.size, bad[0])
    return t.route


def clips(n, fmts=("yuv420p",), seed=3000, sw=128, sh=36, w=W, h=H, **kw):
    """n jobs' layers: one clip each, every one with its own seed, the formats taken in turn"""
    return [[clip(fmts[j % len(fmts)], sw, sh, w, h, seed + j, **kw)] for j in range(n)]


# ---- jobs 2, 3, 4 ------------------------------------------------------------------------------------------------------------------------
OUT_LISTS = [["nv12"], ["v210", "rgba8"], ["v210", "yuv422p8", "nv12", "rgba8"]]


@pytest.mark.parametrize("n_jobs", [2, 3, 4])
@pytest.mark.parametrize("outset", range(len(OUT_LISTS)))
def test_two_three_and_four_jobs_share_a_launch(n_jobs, outset):
    """(three jobs: the count that divides no CU count evenly)"""
    outs = [out(f) for f in OUT_LISTS[outset]]
    route = check_batch([(layers, outs) for layers in clips(n_jobs, seed=3000 + 10 * outset)], W, H, "%d jobs -> %r" % (n_jobs, OUT_LISTS[outset]))
    assert route == "clip_up_multi<rgb>x%dj%d" % (len(outs), n_jobs), route


# ---- which job reads which clip ----------------------------------------------------------------------------------------------------------
def test_every_job_reads_its_own_clip_whatever_its_wire_format():
    outs = [out("yuv422p8"), out("rgba8")]
    route = check_batch([(layers, outs) for layers in clips(4, ("yuv420p", "nv12", "p010", "yuv422p10"), 3100)], W, H, "four wire formats")
    assert route == "clip_up_multi<rgb>x2j4", route
    route = check_batch([(layers, outs) for layers in clips(3, ("yuv420p10", "v210", "yuv422p8"), 3110)], W, H, "three more wire formats")
    assert route == "clip_up_multi<rgb>x2j3", route
    route = check_batch([(layers, outs) for layers in clips(3, ("rgba8", "bgra8"), 3120)], W, H, "clips with alpha")
    assert route == "clip_up_multi<rgba>x2j3", route


def test_an_rgba8_job_beside_a_yuv420p_job_is_two_launches():
    outs = [out("yuv422p8"), out("rgba8")]
    jobs = clips(2, ("rgba8", "yuv420p"), 3130)
    route = check_batch([(layers, outs) for layers in jobs], W, H, "alpha beside none")
    assert route == "clip_up_multi<rgba>x2+clip_up_multi<rgb>x2", route
    jobs = clips(4, ("yuv420p", "nv12", "bgra8", "rgba8"), 3134)
    route = check_batch([(layers, outs) for layers in jobs], W, H, "two without alpha, two with")
    assert route == "clip_up_multi<rgb>x2j2+clip_up_multi<rgba>x2j2", route


def test_jobs_of_another_clip_size_or_placement_start_the_next_launch():
    outs = [out("nv12"), out("bgra8")]
    jobs = clips(2, seed=3140) + clips(2, seed=3142, sw=96, sh=20) + clips(2, seed=3144, sw=96, sh=20, scale_x=0.8, scale_y=0.8)
    route = check_batch([(layers, outs) for layers in jobs], W, H, "three shapes")
    assert route == "+".join(["clip_up_multi<rgb>x2j2"] * 3), route
    # ... and of another output list: a format, a field mode, a writer matrix
    lists = [[out("nv12"), out("bgra8")], [out("nv12"), out("rgba8")], [out("nv12", 1), out("rgba8")], [out("nv12", 1, spec="2020"), out("rgba8", spec="2020")]]
    route = check_batch([(layers, lists[j]) for j, layers in enumerate(clips(4, seed=3146, sw=96, sh=20))], W, H, "four output lists", specs=("709", "709"))
    assert route == "+".join(["clip_up_multi<rgb>x2"] * 4), route


# ---- which lines are composed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [1, 3])
def test_one_field_for_every_output_composes_that_field_only(field):
    """only that field's rows are composed and written - the other field's lines keep their poison (the oracle's frames are written into
    poisoned planes); 4:2:0 chroma from the written line of each pair"""
    outs = [out("v210", field), out("yuv420p", field), out("rgba8", field)]
    jobs = [(small_clip(3200 + j, f), outs) for j, f in enumerate(("yuv422p10", "nv12", "yuv420p"))]
    route = check_batch(jobs, W, H, "three jobs, field %d" % field)
    assert route == "clip_up_multi<rgb>x3j3", route


def test_a_field_beside_a_frame():
    """the whole frame is composed; 54 / 2 = 27 field lines: the last row pair is half; a 4:2:0 field takes its chroma from the written
    line of the pair"""
    outs = [out("yuv420p", 3), out("nv12", 0), out("rgba8", 1), out("v210", 3)]
    jobs = [(small_clip(3210 + j, f), outs) for j, f in enumerate(("yuv420p", "p010"))]
    route = check_batch(jobs, W, H, "fields beside a frame")
    assert route == "clip_up_multi<rgb>x4j2", route


# ---- the kernel's units -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(128, 10), (640, 36), (1280, 24), (2520, 12)])
def test_planar_outputs_around_the_kernels_units(w, h):
    """clips of a third of the channel's size: a short last wave-step column, one row of tiles, more column units than tiles per job"""
    sw, sh = max(8, w // 3 // 8 * 8), max(2, h // 3 // 2 * 2)
    outs = [out("yuv422p8"), out("nv12"), out("bgra8")]
    jobs = clips(3, ("yuv420p", "yuv422p10", "nv12"), 3300 + w, sw=sw, sh=sh, w=w, h=h)
    route = check_batch([(layers, outs) for layers in jobs], w, h, "%dx%d from %dx%d" % (w, h, sw, sh))
    assert route == "clip_up_multi<rgb>x3j3", route


@pytest.mark.parametrize("w,h", [(384, 54), (1920, 40)])
def test_a_v210_output_around_the_kernels_units(w, h):
    sw, sh = w // 3 // 8 * 8, h // 3 // 2 * 2
    outs = [out("v210"), out("yuv420p"), out("rgba8")]
    jobs = clips(4, ("p010", "yuv420p"), 3400 + w, sw=sw, sh=sh, w=w, h=h)
    route = check_batch([(layers, outs) for layers in jobs], w, h, "%dx%d with a v210 output" % (w, h))
    assert route == "clip_up_multi<rgb>x3j4", route


def test_frames_under_the_default_fill():
    """the clip has the frame's size: decoders' frames of the channel's format"""
    outs = [out("v210"), out("nv12")]
    route = check_batch([(layers, outs) for layers in clips(3, ("yuv420p", "yuv422p10", "v210"), 3500, sw=W, sh=H)], W, H, "default fill")
    assert route == "clip_up_multi<rgb>x2j3", route


# ---- hazards ---------------------------------------------------------------------------------------------------------------------------
def test_a_job_that_reads_an_earlier_jobs_output_starts_the_next_launch():
    """job 1's clip IS job 0's rgba8 frame: two launches in order, job 1's frame made from job 0's fresh bytes (the oracle's chain reads
    the oracle's frame of job 0)"""
    first = clips(1, ("rgba8",), 3600, sw=W, sh=H)[0]
    outs0 = [dict(out("rgba8"), slot="screen"), out("nv12")]
    outs1 = [out("rgba8"), out("nv12")]
    route = check_batch([(first, outs0), (Reads("screen", W, H), outs1)], W, H, "job 1 reads job 0's screen frame")
    assert route == "clip_up_multi<rgba>x2+clip_up_multi<rgba>x2", route
    # (the same two jobs with a clip of job 1's own: one launch)
    route = check_batch([(first, outs0), (clips(1, ("rgba8",), 3601, sw=W, sh=H)[0], outs1)], W, H, "no hazard")
    assert route == "clip_up_multi<rgba>x2j2", route


def test_a_job_that_writes_what_an_earlier_job_writes_starts_the_next_launch():
    """the later one wins"""
    outs = [dict(out("nv12"), slot="encoder"), out("rgba8")]
    route = check_batch([(layers, outs) for layers in clips(2, seed=3610)], W, H, "two jobs, one nv12 frame")
    assert route == "clip_up_multi<rgb>x2+clip_up_multi<rgb>x2", route
    route = check_batch([(layers, [dict(out("nv12"), slot="encoder") if j in (0, 2) else out("nv12"), out("rgba8")]) for j, layers in enumerate(clips(4, seed=3612))], W, H,
                        "the third job writes the first job's frame")
    assert route == "clip_up_multi<rgb>x2j2+clip_up_multi<rgb>x2j2", route


def test_a_job_that_writes_what_an_earlier_job_reads_starts_the_next_launch():
    """job 0's clip IS the rgba8 frame job 1 writes: two launches in order, job 0's frames made from what the buffer held before"""
    second = clips(1, ("rgba8",), 3620, sw=W, sh=H)[0]
    outs0 = [out("rgba8"), out("nv12")]
    outs1 = [dict(out("rgba8"), slot="screen"), out("nv12")]
    route = check_batch([(Reads("screen", W, H), outs0), (second, outs1)], W, H, "job 1 writes the frame job 0 reads")
    assert route == "clip_up_multi<rgba>x2+clip_up_multi<rgba>x2", route


def test_the_two_fields_of_one_frame_are_two_launches():
    """no launch of this kernel holds two field modes: the upper and the lower field of one yuv422p8 frame, from two clips, in their turn"""
    field = lambda il: [dict(out("yuv422p8", il), slot="frame"), out("rgba8", il)]
    jobs = [small_clip(3630 + j, "yuv420p") for j in range(2)]  # (enlarged per written row of a field too)
    route = check_batch([(jobs[0], field(1)), (jobs[1], field(3))], W, H, "two fields of one frame")
    assert route == "clip_up_multi<rgb>x2+clip_up_multi<rgb>x2", route
    route = check_batch([(jobs[0], field(3)), (jobs[1], field(3))], W, H, "one field twice")
    assert route == "clip_up_multi<rgb>x2+clip_up_multi<rgb>x2", route


def batch_args(jobs, w, h):
    """device arguments of (layers, outs) jobs, with the planes by job and output"""
    posted, planes = [], []
    for layers, outs in jobs:
        _, dst, outputs = outputs_of(outs, w, h)
        posted.append((device_layers(layers), outputs))
        planes.append(dst)
    return posted, planes


def test_refusals_answer_as_the_siblings_and_write_nothing():
    """two outputs of one job naming one first plane, and the refusals of tests/test_clip_batch_cpu.py on a device: ph_chan_compose_batch_out's
    code and text for the same call, under this entry's name; nothing is written"""
    import hip_harness as hh
    from phaneron_amd import capi
    k = hh.ctx()
    _, _, rd_d, _ = colour("709", "709")

    def both(posted, w=W, h=H):
        texts = []
        for call in (k.clip_compose_batch_out, k.chan_compose_batch_out):
            with pytest.raises(capi.PhaneronError) as e:
                call(posted, w, h, *rd_d)
            texts.append(str(e.value))
        assert "error -1" in texts[0] and texts[0].replace("ph_clip_compose_batch_out", "ph_chan_compose_batch_out") == texts[1], texts
        return texts[0]
    outs = [out("nv12"), out("rgba8"), out("bgra8")]
    posted, planes = batch_args([(layers, outs) for layers in clips(3, seed=3620)], W, H)
    posted[2][1][2]["planes"] = posted[2][1][1]["planes"]
    assert "job 2: outputs 1 and 2 name the same plane" in both(posted)
    posted, more = batch_args([(layers, outs) for layers in clips(3, seed=3620)], W, H)
    posted[1][1][0]["fmt"] = "p010"
    assert "does not write p010 frames" in both(posted)
    posted[1][1][0]["fmt"] = "nv12"
    posted[1][1][1]["interlace"] = 2
    assert "job 1: output 1: interlace must be 0, 1 or 3" in both(posted)
    posted[1][1][1]["interlace"] = 0
    assert "job 0: output 0: width 383" in both(posted, w=383)
    assert "4:2:0 frame needs an even height" in both(posted, h=53)
    k.wait()
    for dst in planes + more:
        for d in dst:
            for p in d:
                assert (hh.host(p, np.uint8) == POISON).all(), "a refused call wrote"


# ---- splits and turns -----------------------------------------------------------------------------------------------------------------
def test_five_jobs_are_four_and_one():
    outs = [out("yuv422p8"), out("rgba8")]
    route = check_batch([(layers, outs) for layers in clips(5, ("yuv420p", "nv12"), 3700)], W, H, "five jobs")
    assert route == "clip_up_multi<rgb>x2j4+clip_up_multi<rgb>x2", route
    outs = [out("v210"), out("nv12"), out("rgba8")]
    route = check_batch([(layers, outs) for layers in clips(9, seed=3710, sw=96, sh=20)], W, H, "nine jobs")
    assert route == "clip_up_multi<rgb>x3j4+clip_up_multi<rgb>x3j4+clip_up_multi<rgb>x3", route


def test_a_two_layer_job_between_two_batchable_ones_runs_in_its_turn():
    outs = [out("yuv422p8"), out("rgba8")]
    one = clips(2, seed=3720)
    two = [clip("yuv420p", 128, 36, W, H, 3722), clip("yuv420p", 128, 36, W, H, 3723, scale_x=0.8, scale_y=0.8, offset_x=0.1)]
    route = check_batch([(one[0], outs), (two, outs), (one[1], outs)], W, H, "a two-layer job in the middle")
    parts = route.split("+")
    assert parts[0] == "clip_up_multi<rgb>x2" == parts[-1] and parts[-2] == "compose_up_multi<rgba>x2j1" and all("read" in p for p in parts[1:-2]) and len(parts) >= 4, route
    assert "j2" not in route and "j3" not in route, route


def test_a_job_whose_outputs_name_two_writer_tables_runs_in_its_turn():
    outs = [out("yuv422p8"), out("rgba8")]
    tables = [out("yuv422p8"), out("rgba8", own_table=True)]
    jobs = clips(5, seed=3730)
    route = check_batch([(jobs[0], outs), (jobs[1], outs), (jobs[2], tables), (jobs[3], outs), (jobs[4], outs)], W, H, "two tables in the middle")
    assert route == "clip_up_multi<rgb>x2j2+clip_up_multi<rgb>x1+clip_up_multi<rgb>x1+clip_up_multi<rgb>x2j2", route
    # a lone v210 output is ph_chan_compose's; jobs that all name ANOTHER table than the launch's start the next launch
    route = check_batch([(jobs[0], [out("v210")]), (jobs[1], [out("v210")])], W, H, "v210 alone")
    assert route == "clip_up_write_v210<rgb>+clip_up_write_v210<rgb>", route
    route = check_batch([(jobs[0], outs), (jobs[1], outs), (jobs[2], [out("rgba8", own_table=True)]), (jobs[3], [out("rgba8", own_table=True)])], W, H, "another table")
    assert route == "clip_up_multi<rgb>x2j2+clip_up_multi<rgb>x1j2", route


def test_a_v210_tail_width_runs_every_job_in_its_turn():
    """1280 wide: the v210 frame's tail quad truncates table indices where the other writers round - ph_clip_compose_multi splits it off"""
    w, h = 1280, 10
    outs = [out("v210"), out("rgba8")]
    route = check_batch([(layers, outs) for layers in clips(3, seed=3740, sw=320, sh=6, w=w, h=h)], w, h, "v210 + rgba8 at 1280")
    parts = route.split("+")
    assert len(parts) == 6 and parts[1::2] == ["clip_up_multi<rgb>x1"] * 3 and "j" not in "".join(parts[1::2]), route
    # without the v210 output the same jobs share
    route = check_batch([(layers, [out("yuv422p8"), out("rgba8")]) for layers in clips(3, seed=3740, sw=320, sh=6, w=w, h=h)], w, h, "yuv422p8 + rgba8 at 1280")
    assert route == "clip_up_multi<rgb>x2j3", route


# ---- options -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0, 2])
def test_chan_enlarged_0_and_2_never_take_the_shared_launch(value):
    import hip_harness as hh
    outs = [out("nv12"), out("rgba8")]
    jobs = [(layers, outs) for layers in clips(3, seed=3800)]
    k = hh.ctx()
    k.set_option("chan_enlarged", value)
    try:
        route = check_batch(jobs, W, H, "chan_enlarged = %d" % value)
    finally:
        k.set_option("chan_enlarged", 1)
    assert "clip_up_multi" not in route and len(route.split("+")) >= 3, route
    assert check_batch(jobs, W, H, "chan_enlarged = 1 again") == "clip_up_multi<rgb>x2j3"


# ---- by name: clip_compose_multi_<n> jobs in one ph_run_programs call ---------------------------------------------------------------------
@pytest.fixture
def by_name():
    b = ByName(W, H)
    yield b
    b.close()


def four_jobs(b, prog):
    srcs = [Src.random("yuv420p", SW, SH, 3900 + j, m(b.w, b.h)) for j in range(4)]
    jobs, outs = [], []
    for s in srcs:
        params, o = clip_params(b, s.data)
        jobs.append((prog, params)), outs.append(o)
    b.ctx.wait(b.capi.QUEUE_LOAD)
    want = [expect_two(b, composite([dict(src=s)], b.w, b.h, b.rd_o)) for s in srcs]
    return jobs, outs, want


def expect_bytes(b, outs, want, what):
    for j, (job, frames_) in enumerate(zip(outs, want)):
        for i, (planes, wnt) in enumerate(zip(job, frames_)):
            for pl, (p, x) in enumerate(zip(planes, wnt)):
                assert np.array_equal(b.read(p), x), "%s: job %d output %d plane %d" % (what, j, i, pl)


@pytest.mark.parametrize("option", [1, 0])
def test_by_name_four_jobs_in_one_call(by_name, option):
    """clip_batch = 1: one launch; 0 (the default, as tests/test_clip_multi_gpu.py pins it): a launch of its own each, in its turn"""
    b = by_name
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [b.w, b.h])
    jobs, outs, want = four_jobs(b, prog)
    if option:
        b.ctx.set_option("clip_batch", 1)
    with b.capi.trace() as t:
        b.ctx.run_programs(jobs)
    b.ctx.wait()
    assert t.route == ("clip_up_multi<rgb>x2j4" if option else "+".join(["clip_up_multi<rgb>x2"] * 4)), t.route
    expect_bytes(b, outs, want, "clip_batch = %d" % option)
    with pytest.raises(b.capi.PhaneronError, match=r"error -1: .*clip_batch"):
        b.ctx.set_option("clip_batch", 2)
    prog.destroy()


def test_by_name_a_failure_in_the_second_group_leaves_the_first_groups_count(by_name):
    """three clip jobs and a v210 channel frame behind them: with clip_batch = 1 the clip jobs are ONE group (the injection is asked once in
    front of it), the channel frame the second; fail_launches = -1 lets one group through"""
    b = by_name
    capi = b.capi
    prog = b.ctx.create_program("phaneron:chan", "clip_compose_multi_1", [b.w, b.h])
    one = b.ctx.create_program("phaneron:chan", "chan_compose_v210_1", [b.w, b.h])
    jobs, outs, want = four_jobs(b, prog)
    last_out = b.planes("v210")[0]
    jobs = jobs[:3] + [(one, dict(b.recipe, l0In=b.upload(frames.v210_random(b.w, b.h, 3950), svm="coarse"), output=last_out))]
    b.ctx.wait(capi.QUEUE_LOAD)
    done = ctypes.c_int(-1)
    for option, count in ((1, 3), (0, 1)):
        b.ctx.set_option("clip_batch", option)
        b.ctx.set_option("fail_launches", -1)
        try:
            with pytest.raises(capi.PhaneronError, match="injected"):
                b.ctx.run_programs(jobs)
            assert capi.lib().ph_run_programs_progress(ctypes.byref(done)) == 0 and done.value == count, (option, done.value)
        finally:
            b.ctx.set_option("fail_launches", 0)
        b.ctx.wait()
        expect_bytes(b, outs[:count], want[:count], "the group that went through")
    assert (b.read(last_out) == POISON).all(), "the failed group wrote"
    prog.destroy(), one.destroy()


# ---- a seeded sweep ----------------------------------------------------------------------------------------------------------------------
def sweep_case(r, case):
    n_jobs = int(r.integers(2, 5))
    n_out = int(r.integers(1, 5))
    fmts = [str(f) for f in r.choice(ALL_OUT, n_out, replace=False)]
    if fmts == ["v210"]:
        fmts = ["v210", "rgba8"]  # (a lone v210 output is ph_chan_compose's)
    first = SOURCES[int(r.integers(0, len(SOURCES)))]
    alpha = first in ("rgba8", "bgra8")
    family = [f for f in SOURCES if (f in ("rgba8", "bgra8")) == alpha]
    srcs = [first] + [family[int(r.integers(0, len(family)))] for _ in range(n_jobs - 1)]
    interlaces = [int(r.choice([0, 1, 3])) for _ in fmts]
    sw, sh = 8 * int(r.integers(8, 25)), 2 * int(r.integers(6, 21))
    if interlaces[0] and all(i == interlaces[0] for i in interlaces):
        sh = min(sh, 26)  # (a field write: enlarged by two more)
    w = int(r.choice([384, 768]))
    return n_jobs, [out(f, il) for f, il in zip(fmts, interlaces)], srcs, sw, sh, w, alpha


@pytest.mark.parametrize("part", range(4))
def test_seeded_jobs_outputs_formats_sizes_and_fields(part):
    """24 cases in four parts, every one made to qualify for the shared launch - and asserted to take it"""
    r = np.random.default_rng(20261021 + part)
    for case in range(6):
        n_jobs, outs, srcs, sw, sh, w, alpha = sweep_case(r, case)
        jobs = [([clip(f, sw, sh, w, H, 4000 + 100 * part + 10 * case + j)], outs) for j, f in enumerate(srcs)]
        what = "sweep %d.%d: %r %dx%d on %dx%d -> %r" % (part, case, srcs, sw, sh, w, H, [(o["fmt"], o["interlace"]) for o in outs])
        route = check_batch(jobs, w, H, what)
        assert route == "clip_up_multi<%s>x%dj%d" % ("rgba" if alpha else "rgb", len(outs), n_jobs), (what, route)
